// pp_k_shortcut.hip — shorten the RRT* batch's paths by Dubins shortcuts along the chain
// (pp_star_shortcut / pp_star_shortcut_edges, DESIGN.md §3.7 "Shortcuts along the chain"; restated
// on the CPU in tests/star_shortcut_ref.py).
//
// Item b = (query, node).  Positions: c_0 the goal with its own yaw, c_1 the node, c_2 its parent,
// ..., c_D the root, each with its stored pose.  Edge (i -> j), i < j <= i + span, is RRT*'s
// feasible edge from c_i's pose (own yaw, like a rewire or goal edge) to c_j's stored pose, w(i, j)
// its Dubins cost or +inf.  In stream order:
//   shortcut_chain   one wave per item: lane 0 follows the parents into the item's chain row
//                    (cf_path's conventions: at most `stride` nodes, else err |= 1), D and the
//                    pair count; the host reads the sizes once
//   per steer round (the pairs of the call are numbered item by item, row by row; a round serves
//   a run of at most Q x 63 of these numbers, so rows of one item and of several items share it):
//   shortcut_emit    one thread per pair: its (item, i, j) by two binary searches, one own-yaw
//                    task into round B's task arrays, the band entry it will fill
//   steer_prep / steer_walk   the extend's round (pp_steer_launch.h), no cull
//   shortcut_settle  one lane per task: literal verdicts re-run one at a time, then the band entry
//                    = the edge's cost when Some and verified, else +inf
//   shortcut_dp      one wave per item, lanes over j: best[D] = 0, best[i] = the first strict
//                    minimum in increasing j of best[j] + w(i, j) (each sum rounded once); the
//                    last 64 best[] live in a lane ring (position p in lane p & 63), so a chain
//                    of any depth needs no LDS; then lane 0 follows next[] from 0 and compacts the
//                    chain row into the shortened path in place
//   shortcut_pack    the rows into the packed CSR output
// Nothing of the trees or the extend's own state is written: round B's arrays, the records and
// stB->W are rewritten by every extend step before it reads them (as the goal rounds).
// pp_star_shortcut_commit runs the same chain and rounds and then, instead of the DP and the pack,
//   shortcut_commit  one wave per item: the DP anchored at the tree's stored edges, its rewires
//                    written into the tree, and the costs of the subtrees below recomputed
// (the only kernel of this unit that writes trees: parent, elen, cost, mark, stamp, rewires).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pp_kernels.h"
#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

constexpr int kScWaves = 4;      // waves (items) per chain / DP workgroup
constexpr int kScPrefetch = 8;   // band rows the DP loads ahead of its serial steps

// the pairs of rows [0, i) of an item: rows up to `full` = D - sp hold sp = min(span, D) pairs,
// the later ones D - row
__device__ __forceinline__ int sc_row_base(int i, int D, int sp) {
    const int full = D - sp;
    const int m = i > full ? i - full : 0;
    return (i - m) * sp + m * sp - (m * (m - 1)) / 2;
}

__global__ __launch_bounds__(64 * kScWaves) void shortcut_chain_kernel(ShortcutArgs a) {
    const int lane = __lane_id();
    const int b = (int)blockIdx.x * kScWaves + (int)(threadIdx.x >> 6);
    if (b >= a.k || lane != 0) return;
    const MqDev& mq = a.a.sd.mq;
    const int* __restrict__ par = mq.parent + (size_t)a.qidx[b] * mq.cap;
    int* __restrict__ row = a.chain + (size_t)b * a.stride;
    int d = 0;
    int c = a.nodes[b];
    while (c >= 0 && d < a.stride) {
        row[d++] = c;
        c = par[c];
    }
    if (c >= 0) {  // deeper than the chain row (or a parent cycle)
        atomicOr(a.err, 1);
        d = 0;
    }
    a.depth[b] = d;
    const int sp = min(a.span, d);
    a.npair[b] = (int64_t)sc_row_base(d, d, sp);
}

__global__ __launch_bounds__(256) void shortcut_emit_kernel(ShortcutArgs a, int64_t g0, int cnt) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t == 0) a.a.sd.stB->W = cnt;  // the round's task count (steer_prep / steer_walk)
    if (t >= cnt) return;
    const int64_t g = g0 + t;
    // the item: the last b with pbase[b] <= g (an item without pairs shares its successor's base)
    int lo = 0, hi = a.k - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.pbase[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    const int b = lo;
    const int gl = (int)(g - a.pbase[b]);
    const int D = a.depth[b];
    const int sp = min(a.span, D);
    // the row: the last i < D with sc_row_base(i) <= gl
    lo = 0;
    hi = D - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sc_row_base(mid, D, sp) <= gl) lo = mid;
        else hi = mid - 1;
    }
    const int i = lo;
    const int l = gl - sc_row_base(i, D, sp);
    const int j = i + 1 + l;
    if (D <= 0 || l >= sp || j > D) {  // (cannot happen: the numbering is the host's own scan)
        atomicOr(a.err, 16);
        a.tdst[t] = -1;
        SteerTask tk{};
        tk.pnode = -1;
        a.a.tB[t] = tk;
        a.a.eB[t] = StarTaskExt{};
        return;
    }
    const MqDev& mq = a.a.sd.mq;
    const int q = a.qidx[b];
    const size_t row = (size_t)q * mq.cap;
    const int* __restrict__ ch = a.chain + (size_t)b * a.stride;
    const int pn = ch[j - 1];
    SteerTask tk{};
    StarTaskExt ex{};
    if (i == 0) {
        tk.x = a.goals[3 * (size_t)q];
        tk.y = a.goals[3 * (size_t)q + 1];
        ex.cyaw = a.goals[3 * (size_t)q + 2];
        ex.node = -1;
    } else {
        const int cn = ch[i - 1];
        tk.x = mq.x[row + cn];
        tk.y = mq.y[row + cn];
        ex.cyaw = mq.yaw[row + cn];  // the node keeps its pose, like a rewired one
        ex.node = cn;
    }
    tk.px = mq.x[row + pn];
    tk.py = mq.y[row + pn];
    tk.pyaw = mq.yaw[row + pn];
    tk.pnode = pn;
    ex.own_yaw = 1;
    ex.pad = q;
    a.a.tB[t] = tk;
    a.a.eB[t] = ex;
    a.tdst[t] = a.boff[b] + (int64_t)i * sp + l;
}

__global__ __launch_bounds__(256) void shortcut_settle_kernel(ShortcutArgs a, SceneDev sc,
                                                              int cnt) {
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int t = gw * 64 + lane;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.a.sd.stB->W = 0;  // the round's walk is done
    if (gw * 64 >= cnt) return;
    const bool act = t < cnt;
    SteerTask tk{};
    StarTaskExt ex{};
    int st = kReject;
    double e = __builtin_inf();
    int64_t dst = -1;
    if (act) {
        tk = a.a.tB[t];
        ex = a.a.eB[t];
        st = a.a.sB[t];
        e = a.a.cB[t];
        dst = a.tdst[t];
    }
    uint64_t lit = __ballot(act && st == kLiteral);
    if (lit) {  // the measure-zero trim cases, one at a time (as star_goal_reduce's star_settle)
        const int ls = lit_acquire(a.a.sd.lit_locks, gw);
        double* bx = a.a.lit_scratch + (size_t)ls * 3 * kLiteralCap;
        for (; lit; lit &= lit - 1) {
            const int l = __builtin_ctzll(lit);
            const int r = steer_collide_literal(sc, __shfl(tk.x, l), __shfl(tk.y, l),
                                                __shfl(ex.cyaw, l), __shfl(tk.px, l),
                                                __shfl(tk.py, l), __shfl(tk.pyaw, l), bx,
                                                bx + kLiteralCap, bx + 2 * kLiteralCap);
            if (lane == l) st = r;
        }
        lit_release(a.a.sd.lit_locks, ls);
    }
    if (act && st == kError) atomicOr(a.err, 4);  // n_point overflow: the reference panics
    // Some and verified (a finite cost), as star_feasible
    const bool feas = act && st == kAccept && e <= 1.7976931348623157e308;
    if (act && dst >= 0) a.band[dst] = feas ? e : __builtin_inf();
}

__global__ __launch_bounds__(64 * kScWaves) void shortcut_dp_kernel(ShortcutArgs a) {
    const int lane = __lane_id();
    const int b = (int)blockIdx.x * kScWaves + (int)(threadIdx.x >> 6);
    if (b >= a.k) return;
    const int D = a.depth[b];
    if (D <= 0) {
        if (lane == 0) {
            a.cost[b] = __builtin_inf();
            a.plen[b] = 0;
        }
        return;
    }
    const int sp = min(a.span, D);
    const double* __restrict__ W = a.band + a.boff[b];
    int* __restrict__ nx = a.next + (size_t)b * a.stride;
    // ring: lane p & 63 holds best[p] of the latest position p with that residue; row i reads the
    // positions i + 1 .. i + 63 (all distinct residues, none of them i's) and then stores best[i]
    double ring = lane == (D & 63) ? 0.0 : __builtin_inf();
    for (int i0 = D - 1; i0 >= 0; i0 -= kScPrefetch) {
        double w[kScPrefetch];
#pragma unroll
        for (int r = 0; r < kScPrefetch; ++r) {  // the rows' loads, ahead of their serial steps
            const int i = i0 - r;
            const bool has = i >= 0 && lane < sp && i + 1 + lane <= D;
            w[r] = has ? W[(size_t)i * sp + lane] : __builtin_inf();
        }
#pragma unroll
        for (int r = 0; r < kScPrefetch; ++r) {
            const int i = i0 - r;
            if (i < 0) break;
            const double bj = __shfl(ring, (i + 1 + lane) & 63);
            double v = w[r] <= 1.7976931348623157e308 ? bj + w[r] : __builtin_inf();
            if (!(v <= 1.7976931348623157e308)) v = __builtin_inf();
            int bl = lane;
            wave_argmin(v, bl);  // the lowest lane (the lowest j) on an exact tie
            if (lane == (i & 63)) ring = v;
            if (lane == 0) nx[i] = v <= 1.7976931348623157e308 ? i + 1 + bl : -1;
        }
    }
    const double c0 = __shfl(ring, 0);
    if (lane != 0) return;
    // the path from position 0: lane 0 reads what it stored itself.  The k-th hop lands on
    // position p_k >= k, so the chain row is compacted in place front to back.
    int* __restrict__ ch = a.chain + (size_t)b * a.stride;
    int m = 0;
    if (c0 <= 1.7976931348623157e308) {
        int p = 0;
        while (p < D && m < D) {
            p = nx[p];
            if (p <= 0 || p > D) {  // (cannot happen: a finite best[i] has a next)
                m = 0;
                break;
            }
            ch[m++] = ch[p - 1];
        }
    }
    a.cost[b] = m > 0 ? c0 : __builtin_inf();
    a.plen[b] = m;
}

__global__ __launch_bounds__(256) void shortcut_pack_kernel(ShortcutArgs a, int Q,
                                                            const int* __restrict__ slot,
                                                            const int64_t* __restrict__ off,
                                                            int* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= off[Q]) return;
    int lo = 0, hi = Q - 1;  // the last q with off[q] <= e (empty rows share their successor's)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    const int b = slot[lo];
    const int64_t r = e - off[lo];
    if (b < 0 || r >= a.plen[b]) return;
    out[e] = a.chain[(size_t)b * a.stride + (size_t)r];
}

// pp_star_shortcut_commit (DESIGN.md §3.7 "Committing shortcuts"; restated on the CPU in
// tests/star_shortcut_commit_ref.py): instead of shortcut_dp / shortcut_pack, the DP anchored at
// the tree and written back into it.  One wave per item, the wave that alone touches its query's
// rows.  c[D] = 0; for i = D - 1 .. 1 with m = the tree node of position i: cur = c[i + 1] +
// elen[m] (what propagation alone would give m), v = the first strict minimum in increasing j of
// c[j] + w(i, j); v < cur (strict, star_rewire's test) re-parents m onto position j's node with
// edge cost w(i, j) and c[i] = v, else c[i] = cur and the stored edge stays, whatever w(i, i + 1)
// says.  c[] lives in shortcut_dp's lane ring.  Lane 0 writes the rewired nodes' parent / elen and
// every changed c[i] with the query's level stamp; then the subtrees under the stamped nodes are
// recomputed level by level exactly as star_rewire_kernel does after one rewire, here once for
// the whole chain: a chain node that is recomputed gets cost[parent] + elen = c[i] again, bit for
// bit, and a node is only ever recomputed from a parent that is already final, so every store is
// the node's final cost and the first one alone can differ from the old cost (the count).
// A steer error of the rounds (a.err) leaves everything unwritten.
// res[3 b ..] = the goal's node (-1: no feasible goal edge), the rewires reported (0 then), the
// costs changed; a.cost[b] = the goal's cost or +inf.
__global__ __launch_bounds__(64 * kScWaves) void shortcut_commit_kernel(ShortcutArgs a) {
    const int lane = __lane_id();
    const int b = (int)blockIdx.x * kScWaves + (int)(threadIdx.x >> 6);
    if (b >= a.k) return;
    const int D = a.depth[b];
    if (D <= 0 || a.err[0] != 0) {
        if (lane == 0) {
            a.cost[b] = __builtin_inf();
            a.res[3 * b] = -1;
            a.res[3 * b + 1] = 0;
            a.res[3 * b + 2] = 0;
        }
        return;
    }
    const StarDev& sd = a.a.sd;
    const MqDev& mq = sd.mq;
    const int q = a.qidx[b];
    const size_t row = (size_t)q * mq.cap;
    double* __restrict__ cost = sd.cost + row;
    double* __restrict__ elen = sd.elen + row;
    int* __restrict__ par = mq.parent + row;
    int* __restrict__ mark = sd.mark + row;
    const int* __restrict__ ch = a.chain + (size_t)b * a.stride;
    const int sp = min(a.span, D);
    const double* __restrict__ W = a.band + a.boff[b];
    int s = sd.stamp[q];
    double ring = lane == (D & 63) ? 0.0 : __builtin_inf();
    int nrw = 0, nchg = 0;  // (lane 0's count of changed chain costs; nrw is wave-uniform)
    for (int i0 = D - 1; i0 >= 1; i0 -= kScPrefetch) {
        double w[kScPrefetch];
#pragma unroll
        for (int r = 0; r < kScPrefetch; ++r) {  // the rows' loads, ahead of their serial steps
            const int i = i0 - r;
            const bool has = i >= 1 && lane < sp && i + 1 + lane <= D;
            w[r] = has ? W[(size_t)i * sp + lane] : __builtin_inf();
        }
        // lane r: row i0 - r's tree node, its stored edge cost and cost (the rows' nodes are
        // distinct, so no store of an earlier row aliases these)
        int mn = 0;
        double me = 0.0, mc = 0.0;
        if (lane < kScPrefetch && i0 - lane >= 1) {
            mn = ch[i0 - lane - 1];
            me = elen[mn];
            mc = cost[mn];
        }
#pragma unroll
        for (int r = 0; r < kScPrefetch; ++r) {
            const int i = i0 - r;
            if (i < 1) break;
            const int m = __shfl(mn, r);
            const double cur = __shfl(ring, (i + 1) & 63) + __shfl(me, r);
            const double old = __shfl(mc, r);
            const double bj = __shfl(ring, (i + 1 + lane) & 63);
            double v = w[r] <= 1.7976931348623157e308 ? bj + w[r] : __builtin_inf();
            if (!(v <= 1.7976931348623157e308)) v = __builtin_inf();
            int bl = lane;
            wave_argmin(v, bl);  // the lowest lane (the lowest j) on an exact tie
            const double wj = __shfl(w[r], bl);
            const bool rw = v < cur;
            const double ci = rw ? v : cur;
            if (lane == (i & 63)) ring = ci;
            if (lane == 0) {
                if (rw) {
                    par[m] = ch[i + bl];  // position j = i + 1 + bl
                    elen[m] = wj;
                }
                if (ci != old) {
                    cost[m] = ci;
                    mark[m] = s;
                    ++nchg;
                }
            }
            nrw += rw ? 1 : 0;
        }
    }
    // the goal: position 0 over c[1 .. sp]
    const double bj0 = __shfl(ring, (1 + lane) & 63);
    const double w0 = lane < sp ? W[lane] : __builtin_inf();
    double v0 = w0 <= 1.7976931348623157e308 ? bj0 + w0 : __builtin_inf();
    if (!(v0 <= 1.7976931348623157e308)) v0 = __builtin_inf();
    int bl0 = lane;
    wave_argmin(v0, bl0);
    const bool reach = v0 <= 1.7976931348623157e308;
    // the subtrees under the changed chain nodes, level by level (star_rewire_kernel's pass): this
    // wave alone reads and writes query q's rows, so workgroup-scope fences order its lanes
    int cnt = 0;
    if (__shfl(nchg, 0) > 0) {
        const int n = mq.n[q];
        __threadfence_block();
        for (;;) {
            bool any = false;
            for (int j0 = 0; j0 < n; j0 += 64 * kRwReg) {
                int pr[kRwReg], mk[kRwReg];
#pragma unroll
                for (int r = 0; r < kRwReg; ++r) {
                    const int j = j0 + lane + 64 * r;
                    pr[r] = j < n ? par[j] : -1;
                }
#pragma unroll
                for (int r = 0; r < kRwReg; ++r) mk[r] = pr[r] >= 0 ? mark[pr[r]] : 0;
#pragma unroll
                for (int r = 0; r < kRwReg; ++r) {
                    if (pr[r] >= 0 && mk[r] == s) {
                        const int j = j0 + lane + 64 * r;
                        const double c = cost[pr[r]] + elen[j];
                        if (c != cost[j]) ++cnt;
                        cost[j] = c;
                        mark[j] = s + 1;
                        any = true;
                    }
                }
            }
            __threadfence_block();
            ++s;
            if (!__ballot(any)) break;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) {
        const int rep = reach ? nrw : 0;
        sd.stamp[q] = s;
        sd.rewires[q] += rep;
        a.cost[b] = reach ? v0 : __builtin_inf();
        a.res[3 * b] = reach ? ch[bl0] : -1;
        a.res[3 * b + 1] = rep;
        a.res[3 * b + 2] = nchg + cnt;
    }
}

hipError_t launch_shortcut_commit(hipStream_t s, const ShortcutArgs& a) {
    if (a.k <= 0 || !a.res) return hipErrorInvalidValue;
    shortcut_commit_kernel<<<(a.k + kScWaves - 1) / kScWaves, 64 * kScWaves, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_shortcut_chain(hipStream_t s, const ShortcutArgs& a) {
    if (a.k <= 0 || a.stride <= 0 || a.span < 1 || a.span > kStarKMax) return hipErrorInvalidValue;
    shortcut_chain_kernel<<<(a.k + kScWaves - 1) / kScWaves, 64 * kScWaves, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_shortcut_round(hipStream_t s, const ShortcutArgs& a, int64_t g0, int cnt,
                                 hipEvent_t* ev) {
    const int TB = a.a.sd.mq.Q * kStarKMax;  // round B's task capacity
    if (cnt <= 0 || cnt > TB) return hipErrorInvalidValue;
    const int blocks = (cnt + 255) / 256;
    const int prep = std::min((cnt + kPrepThreads / 8 - 1) / (kPrepThreads / 8), 2048);
    // (the walk grid of launch_star_steps' rounds B and C)
    const int walk =
        walk_blocks(cnt, a.a.sc.lds_bytes > 0 ? walk_grid_limit(kWalkStar, a.a.sc) : 1024);
    shortcut_emit_kernel<<<blocks, 256, 0, s>>>(a, g0, cnt);
    if (ev) (void)hipEventRecord(ev[0], s);
    launch_prep_tasks(s, prep, a.a.sd.stB, a.a.sc, a.a.rec, a.a.yB, a.a.tB, a.a.cB, a.a.eB);
    if (ev) (void)hipEventRecord(ev[1], s);
    launch_walk(kWalkStar, s, walk, a.a.sd.stB, a.a.sc, a.a.rec, nullptr, a.a.sB, nullptr, nullptr,
                a.a.wg_points);
    if (ev) (void)hipEventRecord(ev[2], s);
    shortcut_settle_kernel<<<blocks, 256, 0, s>>>(a, a.a.sc, cnt);
    if (ev) (void)hipEventRecord(ev[3], s);
    return hipGetLastError();
}

hipError_t launch_shortcut_dp(hipStream_t s, const ShortcutArgs& a) {
    if (a.k <= 0) return hipErrorInvalidValue;
    shortcut_dp_kernel<<<(a.k + kScWaves - 1) / kScWaves, 64 * kScWaves, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_shortcut_pack(hipStream_t s, const ShortcutArgs& a, int Q, const int* slot,
                                const int64_t* off, int64_t total, int* out) {
    if (total <= 0 || Q <= 0) return hipErrorInvalidValue;
    shortcut_pack_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(a, Q, slot, off, out);
    return hipGetLastError();
}

}  // namespace ppamd

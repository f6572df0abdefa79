// pp_k_relax.hip — let every node of an RRT* forest look for a cheaper parent among the nodes of
// its own tree (pp_star_relax, DESIGN.md §3.8 "Relaxing the trees"; restated on the CPU in
// tests/star_relax_ref.py).  It is the repair's round (pp_k_repair.hip) with every node a top.
//
// Node g of the `total` nodes is node i = g - off[q] of tree q (row q * cap + i).  One round, in
// stream order, per slice [g0, g1) of at most kRelaxNodesPerSlice nodes:
//   knn     one wave per node, a self-join of the tree with the emit fused into it: the
//           star_k(k, n - 1) nearest nodes j != i by exact f64 (d2, index), lane r the r-th; the
//           lanes that survive the culls (not the node's parent; cost[p] < cost[i]; cost[p] + the
//           chord bound < cost[i]) pack one own-yaw steer task each, in rank order, contiguous per
//           node (st->W counts them).  No candidate list is stored.
//   prep/walk  the steer round of pp_steer_launch.h on the slice's tasks (kWalkBatchPlan), with
//           cbase = cost[p], climit = cost[i]: steer_prep settles without a walk what cannot win
//   choose  one wave per node, one lane per task: literal verdicts re-run, the first strict
//           minimum of cost[p] + e (the lowest lane, so the lowest rank, on a tie), accepted when
//           it is below cost[i]; parent and elen are staged in wpar / welen
// and after the round's last slice:
//   commit  one wave per query: unless the error word is set, the staged rows into the tree, then
//           the costs rebuilt from the root level by level (cost[i] = cost[parent[i]] + elen[i],
//           parents final one pass before their children), at most n passes
// A round's knn and choose read the trees alone and commit alone writes them, so every node sees
// the state the round began with and the order of the nodes cannot matter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "pp_kernels.h"
#include "pp_reval_dev.h"
#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

constexpr int kRxWaves = 4;  // waves (nodes) per knn / choose workgroup

// exact lower bound of an edge's Dubins cost, star_knn_kernel's (pp_k_star.hip: star_chord_lb)
__device__ __forceinline__ double rx_chord_lb(double d2, double curv) {
    return sqrt(d2) * curv * (1.0 - 1e-9) - 1e-9;
}

// Bitonic sort of one (d, i) pair per lane across the wave, ascending in (d, i) lexicographic
// order: lane r ends up with the r-th smallest (repair_knn_kernel's)
struct RxKv {
    double d;
    int i;
};
__device__ __forceinline__ RxKv rx_sort64(double d, int i, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const double od = __shfl_xor(d, stride);
            const int oi = __shfl_xor(i, stride);
            const bool other_less = od < d || (od == d && oi < i);
            const bool up = (lane & size) == 0 || size == 64;
            const bool keep_min = ((lane & stride) == 0) == up;
            if (keep_min == other_less) {
                d = od;
                i = oi;
            }
        }
    }
    return RxKv{d, i};
}

// a query the call leaves alone: switched off by the caller, its root blocked, or a lone root
__device__ __forceinline__ bool rx_live(const RelaxArgs& a, int q, int n) {
    return n > 1 && !(a.active && !a.active[q]) && !(a.blocked && a.blocked[q]);
}

// One wave per node of the slice.  The distances are recomputed by every pass (the same expression
// gives the same bits): the k-th smallest lane minimum T bounds the k nearest; when at most 64
// nodes lie within T they are gathered and sorted, else the k nearest are taken one by one as
// (d2, index) successors.  Then the culls and the tasks.
__global__ __launch_bounds__(64 * kRxWaves) void relax_knn_kernel(RelaxArgs a, int g0s, int g1s) {
    __shared__ double s_cd[kRxWaves][64];
    __shared__ int s_ci[kRxWaves][64];
    __shared__ int s_cnt[kRxWaves], s_base, s_stat[kRxWaves][3];
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    double* cand_d = s_cd[wave];
    int* cand_i = s_ci[wave];
    const int g = g0s + (int)blockIdx.x * kRxWaves + wave;
    const bool in = g < g1s;
    int q = 0, gq = 0, n = 0, i = 0;
    if (in) {
        q = rv_tree_of(a.off, a.Q, g);
        gq = a.off[q];
        n = a.off[q + 1] - gq;
        i = g - gq;
    }
    const bool live = in && i > 0 && rx_live(a, q, n);
    const size_t row = (size_t)q * a.cap;
    const double* __restrict__ X = a.tr.x + row;
    const double* __restrict__ Y = a.tr.y + row;
    int k = 0, mine = -1;
    double x = 0.0, y = 0.0;
    if (live) {
        x = X[i];
        y = Y[i];
        k = a.ksched[n - 1];  // <= n - 1: the other nodes
        double lmin = __builtin_inf();
        for (int j = lane; j < n; j += 64)
            if (j != i) {
                const double dx = x - X[j], dy = y - Y[j];
                lmin = fmin(lmin, dx * dx + dy * dy);
            }
        const double T = readlane_f64(rx_sort64(lmin, 0, lane).d, k - 1);
        int c = 0;
        for (int j = lane; j < n; j += 64)
            if (j != i) {
                const double dx = x - X[j], dy = y - Y[j];
                c += dx * dx + dy * dy <= T;
            }
        int off = wave_incl_scan(c);
        const int C = __builtin_amdgcn_readlane(off, 63);
        if (C <= 64) {
            off -= c;
            for (int j = lane; j < n; j += 64)
                if (j != i) {
                    const double dx = x - X[j], dy = y - Y[j];
                    const double d2 = dx * dx + dy * dy;
                    if (d2 <= T) {
                        cand_d[off] = d2;
                        cand_i[off] = j;
                        ++off;
                    }
                }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            RxKv kv{__builtin_inf(), 0x7fffffff};
            if (lane < C) kv = RxKv{cand_d[lane], cand_i[lane]};
            kv = rx_sort64(kv.d, kv.i, lane);
            mine = lane < k ? kv.i : -1;
        } else {
            double pd = -1.0;
            int pi = -1;
            for (int r = 0; r < k; ++r) {
                double bd = __builtin_inf();
                int bi = 0x7fffffff;
                for (int j = lane; j < n; j += 64)
                    if (j != i) {
                        const double dx = x - X[j], dy = y - Y[j];
                        const double d2 = dx * dx + dy * dy;
                        if ((d2 > pd || (d2 == pd && j > pi)) && d2 < bd) {
                            bd = d2;
                            bi = j;
                        }
                    }
                wave_argmin(bd, bi);
                pd = bd;
                pi = bi;
                if (lane == r) mine = bi;
            }
        }
    }
    // the culls, each exact: the parent's total is the node's own cost; a candidate that costs no
    // less than the node cannot win (fl(cost[p] + e) >= cost[p]); the chord bound of the extend
    bool want = false, notp = false;
    double ci = 0.0, cp = 0.0;
    if (live && lane < k && mine >= 0 && mine < n) {
        ci = a.cost[row + i];
        cp = a.cost[row + mine];
        notp = mine != a.tr.parent[row + i];
        want = notp && cp < ci;
    }
    const int n_notp = __popcll(__ballot(notp)), n_cheap = __popcll(__ballot(want));
    if (want) {
        const double dx = x - X[mine], dy = y - Y[mine];
        want = cp + rx_chord_lb(dx * dx + dy * dy, a.curv) < ci;
    }
    const uint64_t wm = __ballot(want);
    const int cnt = __popcll(wm);
    // the slice's task reservation: one counter add per workgroup
    if (lane == 0) {
        s_cnt[wave] = cnt;
        s_stat[wave][0] = k;
        s_stat[wave][1] = n_notp;
        s_stat[wave][2] = n_cheap;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < kRxWaves; ++w) tot += s_cnt[w];
        s_base = tot > 0 ? atomicAdd(&a.st->W, tot) : 0;
        if (a.stats) {
            long long v[3] = {0, 0, 0};
            for (int w = 0; w < kRxWaves; ++w)
                for (int r = 0; r < 3; ++r) v[r] += s_stat[w][r];
            if (v[0]) atomicAdd((unsigned long long*)&a.rrec->cand, (unsigned long long)v[0]);
            if (v[1]) atomicAdd((unsigned long long*)&a.rrec->not_parent, (unsigned long long)v[1]);
            if (v[2]) atomicAdd((unsigned long long*)&a.rrec->cheaper, (unsigned long long)v[2]);
            if (tot) atomicAdd((unsigned long long*)&a.rrec->tasks, (unsigned long long)tot);
        }
    }
    __syncthreads();
    if (!in) return;
    int slot = s_base;
    for (int w = 0; w < wave; ++w) slot += s_cnt[w];
    if (lane == 0) {
        a.tslot[g - g0s] = slot;
        a.tcnt[g - g0s] = cnt;
        a.wpar[g] = -1;  // no choice yet
    }
    if (want && slot + cnt <= a.task_cap) {  // (cnt <= k <= the slice's tasks per node)
        const int ts = slot + __popcll(wm & ((1ull << lane) - 1ull));  // rank order
        SteerTask tk{};
        tk.x = x;
        tk.y = y;
        tk.px = X[mine];
        tk.py = Y[mine];
        tk.pyaw = a.tr.yaw[row + mine];
        tk.pnode = mine;
        a.tasks[ts] = tk;
        StarTaskExt ex{};
        ex.cyaw = a.tr.yaw[row + i];  // the node keeps its pose, like a rewired node
        ex.own_yaw = 1;
        ex.cull = 1;  // only a total strictly below the node's cost matters
        ex.cbase = cp;
        ex.climit = ci;
        ex.node = i;
        ex.pad = q;
        a.ext[ts] = ex;
    }
}

__global__ __launch_bounds__(64 * kRxWaves) void relax_choose_kernel(RelaxArgs a, SceneDev sc,
                                                                     int g0s, int g1s) {
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int g = g0s + gw;
    if (g >= g1s) return;
    const int cnt = a.tcnt[gw];
    if (cnt <= 0) return;  // every candidate was culled
    const int slot = a.tslot[gw];
    if (slot + cnt > a.task_cap) {  // (cannot happen: the host sizes the slice by its k)
        if (lane == 0) atomicOr(a.err, 2);
        return;
    }
    const bool act = lane < cnt;
    SteerTask tk{};
    StarTaskExt ex{};
    int st = kReject;
    double e = __builtin_inf();
    if (act) {
        tk = a.tasks[slot + lane];
        ex = a.ext[slot + lane];
        st = a.status[slot + lane];
        e = a.tcost[slot + lane];
    }
    uint64_t lit = __ballot(act && st == kLiteral);
    if (lit) {  // the measure-zero trim cases, one at a time (as repair_choose_kernel)
        const int ls = lit_acquire(a.lit_locks, gw);
        double* bx = a.lit_scratch + (size_t)ls * 3 * kLiteralCap;
        for (; lit; lit &= lit - 1) {
            const int l = __builtin_ctzll(lit);
            const int r = steer_collide_literal(sc, __shfl(tk.x, l), __shfl(tk.y, l),
                                                __shfl(ex.cyaw, l), __shfl(tk.px, l),
                                                __shfl(tk.py, l), __shfl(tk.pyaw, l), bx,
                                                bx + kLiteralCap, bx + 2 * kLiteralCap);
            if (lane == l) st = r;
        }
        lit_release(a.lit_locks, ls);
    }
    if (a.stats) {  // (steer_prep leaves kPrepFallback in the record of a task it hands to the walk)
        const int wk = __popcll(__ballot(act && a.rec[slot + lane].state == kPrepFallback));
        if (lane == 0 && wk) atomicAdd((unsigned long long*)&a.rrec->walked, (unsigned long long)wk);
    }
    if (__ballot(act && st == kError)) {  // the reference panics: the round is not applied
        if (lane == 0) atomicOr(a.err, 1);
        return;
    }
    // Some and verified (a finite cost); the first strict minimum in rank order
    const bool feas = act && st == kAccept && e <= 1.7976931348623157e308;
    double c = feas ? ex.cbase + e : __builtin_inf();
    int bl = lane;
    wave_argmin(c, bl);
    const int bp = __shfl(tk.pnode, bl);
    const double be = __shfl(e, bl);
    const double ci = __shfl(ex.climit, 0);
    if (lane == 0 && c < ci) {  // strict, the extend's own rewire test
        a.wpar[g] = bp;
        a.welen[g] = be;
    }
}

__global__ __launch_bounds__(256) void relax_commit_kernel(RelaxArgs a) {
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    if (*a.err) return;  // a steer overflowed: the round is not applied
    for (int q = gw; q < a.Q; q += nw) {
        const int g0 = a.off[q], n = a.off[q + 1] - g0;
        if (!rx_live(a, q, n)) continue;
        const size_t row = (size_t)q * a.cap;
        int* __restrict__ P = a.tr.parent + row;
        double* __restrict__ C = a.cost + row;
        double* __restrict__ E = a.elen + row;
        int* __restrict__ L = a.lvl + g0;
        const int* __restrict__ WP = a.wpar + g0;
        const double* __restrict__ WE = a.welen + g0;
        unsigned char* __restrict__ H = a.chg + g0;
        int rw = 0;
        for (int j = lane + (lane == 0 ? 64 : 0); j < n; j += 64) {  // (not the root)
            const int p = WP[j];
            if (p >= 0 && p < n) {
                P[j] = p;
                E[j] = WE[j];
                ++rw;
            }
        }
        rw = __builtin_amdgcn_readlane(wave_incl_scan(rw), 63);
        if (rw == 0) continue;  // nothing moved: every cost stands
        for (int j = lane; j < n; j += 64) L[j] = j == 0 ? 1 : 0;
        // this wave alone reads and writes query q's rows in this kernel (as repair_grow_kernel):
        // a workgroup-scope fence orders its lanes' stores and loads
        __threadfence_block();
        // level by level from the root: a node's parent got its final cost one pass earlier (a
        // pass compares levels with cur and stores cur + 1, so it never reads what it wrote); a
        // tree of n nodes has fewer than n levels
        int chg = 0;
        for (int cur = 1; cur < n; ++cur) {
            bool any = false;
            for (int j = lane; j < n; j += 64) {
                if (L[j] != 0) continue;
                const int p = P[j];
                if (p < 0 || p >= n || L[p] != cur) continue;
                const double c = C[p] + E[j];
                if (__double_as_longlong(c) != __double_as_longlong(C[j])) {
                    C[j] = c;
                    if (!H[j]) {  // costs only fall: a cost that moved never moves back
                        H[j] = 1;
                        ++chg;
                    }
                }
                L[j] = cur + 1;
                any = true;
            }
            __threadfence_block();
            if (!__ballot(any)) break;
        }
        chg = __builtin_amdgcn_readlane(wave_incl_scan(chg), 63);
        if (lane == 0) {
            a.nrw[q] += rw;
            a.rewires[q] += rw;
            atomicAdd(&a.rrec->rewired, rw);
            atomicAdd((unsigned long long*)&a.rrec->changed, (unsigned long long)chg);
        }
    }
}

hipError_t launch_relax_slice(hipStream_t s, const SceneDev& sc, const RelaxArgs& a, int g0,
                              int g1) {
    const int nt = g1 - g0;
    if (nt <= 0 || nt > kRelaxNodesPerSlice || g1 > a.total || a.kmax < 1 || a.kmax > kStarKMax ||
        (int64_t)nt * a.kmax > a.task_cap)
        return hipErrorInvalidValue;
    const int ub = nt * a.kmax;  // the slice's tasks at most; the count itself is st->W
    hipError_t e = hipMemsetAsync((char*)a.st + offsetof(DevState, W), 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    const int blocks = (nt + kRxWaves - 1) / kRxWaves;
    relax_knn_kernel<<<blocks, 64 * kRxWaves, 0, s>>>(a, g0, g1);
    launch_prep_tasks(s, std::min((ub + 31) / 32, 8192), a.st, sc, a.rec, a.yaw, a.tasks, a.tcost,
                      a.ext);
    launch_walk(kWalkBatchPlan, s, walk_blocks(ub, walk_grid_limit(kWalkBatchPlan, sc)), a.st, sc,
                a.rec, nullptr, a.status, nullptr, nullptr, a.wg_points);
    relax_choose_kernel<<<blocks, 64 * kRxWaves, 0, s>>>(a, sc, g0, g1);
    return hipGetLastError();
}

hipError_t launch_relax_commit(hipStream_t s, const RelaxArgs& a) {
    if (a.Q <= 0) return hipErrorInvalidValue;
    relax_commit_kernel<<<std::min((a.Q + 3) / 4, 4096), 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ppamd

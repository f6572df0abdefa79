// pp_k_repair.hip — hang dropped subtrees of an RRT* forest under kept nodes again after a scene
// change (pp_star_repair, DESIGN.md §3.8 "Re-attaching orphaned subtrees"; restated on the CPU in
// tests/star_repair_ref.py).
//
// The host runs these between the revalidation's jump and its compaction (pp_k_revalidate.hip).
// Node g of the `total` nodes is node i = g - off[q] of tree q (row q * cap + i).  K is the kept
// set (flag bit 0), K0 the revalidation's.  Round r, in stream order:
//   tops     one pass over the nodes: a top of round r is a dropped node that was no top before
//            and whose own edge failed (r = 1) or whose parent is a failed top (r > 1); packed
//            into tops[] with one counter add per workgroup
//   knn      one wave per top, all tops in one launch: the star_k(k, |K_q|) nearest kept nodes of
//            its tree by exact f64 (d2, index), listed in near[]
//   then per slice of kRepairTopsPerSlice tops (the host knows the round's top count):
//   emit     one own-yaw steer task per candidate (top -> candidate), packed (st->W counts them)
//   prep/walk  the steer round of pp_steer_launch.h on the slice's tasks (kWalkBatchPlan)
//   choose   one wave per top, one lane per candidate: literal verdicts re-run, the first strict
//            minimum of cost[p] + e; the top's parent / elen / cost are staged, K is not touched
//   grow     one wave per query with a re-attached top: the tops join K, then level by level
//            every dropped node that was never a top (so its own edge holds) and whose parent
//            joined one level earlier, with cost = cost[parent] + elen
// Within a round every top reads K and the costs of K as they stood when the round began (choose
// writes rows outside K only, grow runs after the round's last slice), so the result does not
// depend on the order of the tops.  Nothing is written into the trees before commit, which a
// steer overflow (the error word) turns into a no-op.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "pp_kernels.h"
#include "pp_reval_dev.h"
#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

constexpr int kRpWaves = 4;  // waves (tops) per knn / choose workgroup

__global__ __launch_bounds__(kRvThreads) void repair_init_kernel(RepairArgs a) {
    const RevalArgs& v = a.rv;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= v.total) return;
    const int q = rv_tree_of(v.off, v.Q, g);
    const size_t row = (size_t)q * v.cap + (size_t)(g - v.off[q]);
    a.flag[g] = rv_keep(a.vkeep[g], g, v.off, v.Q) ? 1 : 0;
    a.top[g] = kTopNever;
    a.wpar[g] = v.tr.parent[row];
    a.wcost[g] = v.cost[row];
    a.welen[g] = v.elen[row];
}

__global__ __launch_bounds__(kRvThreads) void repair_tops_kernel(RepairArgs a, int round) {
    const RevalArgs& v = a.rv;
    __shared__ int s_cnt[kRvThreads / 64], s_base;
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool is = false;
    if (g < v.total && !(a.flag[g] & 1) && a.top[g] == kTopNever) {
        const int q = rv_tree_of(v.off, v.Q, g);
        const int g0 = v.off[q], nq = v.off[q + 1] - g0;
        // (a blocked root fails every line that ends in it: its query re-attaches nothing)
        if (g > g0 && !(v.blocked && v.blocked[q])) {
            if (round == 1) {
                is = (a.vedge[g] & kRvBad) != 0;
            } else {  // (its own edge holds, or it would have been a top of round 1)
                const int p = a.wpar[g];
                is = p >= 0 && p < nq && a.top[g0 + p] == kTopFailed;
            }
        }
    }
    const uint64_t m = __ballot(is);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < kRvThreads / 64; ++w) tot += s_cnt[w];
        s_base = tot > 0 ? atomicAdd(&a.rec->ntops[round], tot) : 0;
    }
    __syncthreads();
    if (!is) return;
    int slot = s_base + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) slot += s_cnt[w];
    a.tops[slot] = g;
    a.top[g] = kTopNow;
}

// Bitonic sort of one (d, i) pair per lane across the wave, ascending in (d, i) lexicographic
// order: lane r ends up with the r-th smallest
struct RpKv {
    double d;
    int i;
};
__device__ __forceinline__ RpKv rp_sort64(double d, int i, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const double od = __shfl_xor(d, stride);
            const int oi = __shfl_xor(i, stride);
            const bool other_less = od < d || (od == d && oi < i);
            const bool up = (lane & size) == 0 || size == 64;  // this block sorts ascending
            const bool keep_min = ((lane & stride) == 0) == up;
            if (keep_min == other_less) {
                d = od;
                i = oi;
            }
        }
    }
    return RpKv{d, i};
}

// One wave per top.  The distances are recomputed by every pass (the same expression gives the
// same bits), so a tree of any size is served with 64 list entries of LDS per wave: the k-th
// smallest lane minimum T bounds the k nearest; when at most 64 kept nodes lie within T they are
// gathered and sorted, else the k nearest are taken one by one as (d2, index) successors.
__global__ __launch_bounds__(64 * kRpWaves) void repair_knn_kernel(RepairArgs a, int ntops) {
    const RevalArgs& v = a.rv;
    __shared__ double s_cd[kRpWaves][64];
    __shared__ int s_ci[kRpWaves][64];
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    double* cand_d = s_cd[wave];
    int* cand_i = s_ci[wave];
    const int t = (int)blockIdx.x * kRpWaves + wave;
    if (t >= ntops) return;
    int k = 0, mine = -1;
    {
        const int g = a.tops[t];
        const int q = rv_tree_of(v.off, v.Q, g);
        const int g0 = v.off[q], n = v.off[q + 1] - g0;
        const size_t row = (size_t)q * v.cap;
        const double* __restrict__ X = v.tr.x + row;
        const double* __restrict__ Y = v.tr.y + row;
        const unsigned char* __restrict__ F = a.flag + g0;
        const double x = X[g - g0], y = Y[g - g0];
        double lmin = __builtin_inf();
        int c = 0;
        for (int j = lane; j < n; j += 64)
            if (F[j] & 1) {
                const double dx = x - X[j], dy = y - Y[j];
                lmin = fmin(lmin, dx * dx + dy * dy);
                ++c;
            }
        const int nk = __builtin_amdgcn_readlane(wave_incl_scan(c), 63);  // |K| >= 1: the root
        k = a.ksched[nk];
        const double T = readlane_f64(rp_sort64(lmin, 0, lane).d, k - 1);
        c = 0;
        for (int j = lane; j < n; j += 64)
            if (F[j] & 1) {
                const double dx = x - X[j], dy = y - Y[j];
                c += dx * dx + dy * dy <= T;
            }
        int off = wave_incl_scan(c);
        const int C = __builtin_amdgcn_readlane(off, 63);
        if (C <= 64) {
            off -= c;
            for (int j = lane; j < n; j += 64)
                if (F[j] & 1) {
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
            RpKv kv{__builtin_inf(), 0x7fffffff};
            if (lane < C) kv = RpKv{cand_d[lane], cand_i[lane]};
            kv = rp_sort64(kv.d, kv.i, lane);
            mine = lane < k ? kv.i : -1;
        } else {
            double pd = -1.0;
            int pi = -1;
            for (int r = 0; r < k; ++r) {
                double bd = __builtin_inf();
                int bi = 0x7fffffff;
                for (int j = lane; j < n; j += 64)
                    if (F[j] & 1) {
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
    if (lane == 0) a.tcnt[t] = k;
    if (lane < k) a.near[(size_t)t * kStarKMax + lane] = mine;  // candidate order
}

// the steer tasks of the packed tops [t0, t1), one wave per top: candidate c of top t is task
// tslot[t - t0] + c
__global__ __launch_bounds__(64 * kRpWaves) void repair_emit_kernel(RepairArgs a, int t0, int t1) {
    const RevalArgs& v = a.rv;
    __shared__ int s_cnt[kRpWaves], s_base;
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const int t = t0 + (int)blockIdx.x * kRpWaves + wave;
    const bool live = t < t1;
    const int k = live ? a.tcnt[t] : 0;
    // the slice's task reservation: one counter add per workgroup
    if (lane == 0) s_cnt[wave] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < kRpWaves; ++w) tot += s_cnt[w];
        s_base = tot > 0 ? atomicAdd(&v.st->W, tot) : 0;
    }
    __syncthreads();
    if (!live) return;
    int slot = s_base;
    for (int w = 0; w < wave; ++w) slot += s_cnt[w];
    if (lane == 0) a.tslot[t - t0] = slot;
    if (lane < k) {
        const int g = a.tops[t];
        const int q = rv_tree_of(v.off, v.Q, g);
        const int i = g - v.off[q];
        const size_t row = (size_t)q * v.cap;
        const int mine = a.near[(size_t)t * kStarKMax + lane];
        SteerTask tk{};
        tk.x = v.tr.x[row + i];
        tk.y = v.tr.y[row + i];
        tk.px = v.tr.x[row + mine];
        tk.py = v.tr.y[row + mine];
        tk.pyaw = v.tr.yaw[row + mine];
        tk.pnode = mine;
        v.tasks[slot + lane] = tk;
        StarTaskExt ex{};
        ex.cyaw = v.tr.yaw[row + i];  // the top keeps its pose, like a rewired node
        ex.own_yaw = 1;
        ex.node = i;
        ex.pad = q;
        v.ext[slot + lane] = ex;
    }
}

__global__ __launch_bounds__(64 * kRpWaves) void repair_choose_kernel(RepairArgs a, SceneDev sc,
                                                                      int t0, int t1) {
    const RevalArgs& v = a.rv;
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int t = t0 + gw;
    if (t >= t1) return;
    const int g = a.tops[t];
    const int q = rv_tree_of(v.off, v.Q, g);
    const int g0 = v.off[q];
    const int slot = a.tslot[gw], cnt = a.tcnt[t];
    const bool act = lane < cnt;
    SteerTask tk{};
    StarTaskExt ex{};
    int st = kReject;
    double e = __builtin_inf();
    if (act) {
        tk = v.tasks[slot + lane];
        ex = v.ext[slot + lane];
        st = v.status[slot + lane];
        e = a.tcost[slot + lane];
    }
    uint64_t lit = __ballot(act && st == kLiteral);
    if (lit) {  // the measure-zero trim cases, one at a time (as reval_settle_kernel)
        const int ls = lit_acquire(v.lit_locks, gw);
        double* bx = v.lit_scratch + (size_t)ls * 3 * kLiteralCap;
        for (; lit; lit &= lit - 1) {
            const int l = __builtin_ctzll(lit);
            const int r = steer_collide_literal(sc, __shfl(tk.x, l), __shfl(tk.y, l),
                                                __shfl(ex.cyaw, l), __shfl(tk.px, l),
                                                __shfl(tk.py, l), __shfl(tk.pyaw, l), bx,
                                                bx + kLiteralCap, bx + 2 * kLiteralCap);
            if (lane == l) st = r;
        }
        lit_release(v.lit_locks, ls);
    }
    if (__ballot(act && st == kError)) {  // the reference panics: the call fails, the trees stay
        if (lane == 0) atomicOr(v.err, 1);
        return;
    }
    // Some and verified (a finite cost); the first strict minimum in candidate order
    const bool feas = act && st == kAccept && e <= 1.7976931348623157e308;
    double c = feas ? a.wcost[g0 + (act ? tk.pnode : 0)] + e : __builtin_inf();
    int bl = lane;
    wave_argmin(c, bl);
    const int bp = __shfl(tk.pnode, bl);
    const double be = __shfl(e, bl);
    if (lane != 0) return;
    if (c <= 1.7976931348623157e308) {
        a.top[g] = kTopAttached;
        a.wpar[g] = bp;
        a.welen[g] = be;
        a.wcost[g] = c;
        a.lvl[g] = 1;
        a.qhas[q] = 1;
    } else {
        a.top[g] = kTopFailed;
    }
}

__global__ __launch_bounds__(256) void repair_grow_kernel(RepairArgs a) {
    const RevalArgs& v = a.rv;
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    for (int q = gw; q < v.Q; q += nw) {
        if (!a.qhas[q]) continue;
        const int g0 = v.off[q], n = v.off[q + 1] - g0;
        unsigned char* __restrict__ F = a.flag + g0;
        const unsigned char* __restrict__ T = a.top + g0;
        int* __restrict__ L = a.lvl + g0;
        const int* __restrict__ P = a.wpar + g0;
        double* __restrict__ C = a.wcost + g0;
        const double* __restrict__ E = a.welen + g0;
        int rea = 0, rec = 0;
        for (int j = lane; j < n; j += 64)
            if (T[j] == kTopAttached && L[j] == 1) {  // this round's (lvl is zeroed per round)
                F[j] = 3;
                ++rea;
            }
        // this wave alone reads and writes query q's entries in this kernel (as
        // star_rewire_kernel): a workgroup-scope fence orders its lanes' stores and loads
        __threadfence_block();
        // level by level: a node's parent joined, with its final cost, one pass earlier (a pass
        // compares levels with cur and stores cur + 1, so it never reads what it wrote)
        for (int cur = 1;; ++cur) {
            bool any = false;
            for (int j = lane; j < n; j += 64) {
                if ((F[j] & 1) || T[j] != kTopNever) continue;
                const int p = P[j];
                if (p < 0 || p >= n || L[p] != cur) continue;
                C[j] = C[p] + E[j];
                L[j] = cur + 1;
                F[j] = 3;
                ++rec;
                any = true;
            }
            __threadfence_block();
            if (!__ballot(any)) break;
        }
        rea = __builtin_amdgcn_readlane(wave_incl_scan(rea), 63);
        rec = __builtin_amdgcn_readlane(wave_incl_scan(rec), 63);
        if (lane == 0) {
            atomicAdd((unsigned long long*)&a.rec->reattached, (unsigned long long)rea);
            atomicAdd((unsigned long long*)&a.rec->recovered, (unsigned long long)(rea + rec));
        }
    }
}

__global__ __launch_bounds__(kRvThreads) void repair_commit_kernel(RepairArgs a) {
    const RevalArgs& v = a.rv;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= v.total) return;
    const int q = rv_tree_of(v.off, v.Q, g);
    const int g0 = v.off[q];
    const unsigned char f = a.flag[g];
    a.vout[g] = (unsigned)g0 | ((f & 1) ? 0u : kRvBad);  // (rv_keep keeps a root with either)
    if (!(f & 2) || *v.err) return;  // a steer overflowed: the trees stay as they are
    const size_t row = (size_t)q * v.cap + (size_t)(g - g0);
    v.tr.parent[row] = a.wpar[g];
    v.cost[row] = a.wcost[g];
    v.elen[row] = a.welen[g];
}

hipError_t launch_repair_stage(hipStream_t s, const RepairArgs& a, int stage, int round) {
    const int total = a.rv.total;
    if (total <= 0) return hipErrorInvalidValue;
    const int g = (total + kRvThreads - 1) / kRvThreads;
    hipError_t e;
    switch (stage) {
    case kRepairInit:
        repair_init_kernel<<<g, kRvThreads, 0, s>>>(a);
        break;
    case kRepairTops:
        if (round < 1 || round > kRepairMaxRounds) return hipErrorInvalidValue;
        if ((e = hipMemsetAsync(a.lvl, 0, (size_t)total * sizeof(int), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(a.qhas, 0, (size_t)a.rv.Q, s)) != hipSuccess) return e;
        repair_tops_kernel<<<g, kRvThreads, 0, s>>>(a, round);
        break;
    case kRepairGrow:
        repair_grow_kernel<<<std::min((a.rv.Q + 3) / 4, 4096), 256, 0, s>>>(a);
        break;
    case kRepairCommit:
        repair_commit_kernel<<<g, kRvThreads, 0, s>>>(a);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_repair_knn(hipStream_t s, const RepairArgs& a, int ntops) {
    if (ntops <= 0) return hipErrorInvalidValue;
    repair_knn_kernel<<<(ntops + kRpWaves - 1) / kRpWaves, 64 * kRpWaves, 0, s>>>(a, ntops);
    return hipGetLastError();
}

hipError_t launch_repair_slice(hipStream_t s, const SceneDev& sc, const RepairArgs& a, int t0,
                               int t1) {
    const int nt = t1 - t0;
    if (nt <= 0 || nt > kRepairTopsPerSlice) return hipErrorInvalidValue;
    const int ub = nt * kStarKMax;  // the slice's tasks at most; the count itself is st->W
    hipError_t e = hipMemsetAsync((char*)a.rv.st + offsetof(DevState, W), 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    const int blocks = (nt + kRpWaves - 1) / kRpWaves;
    repair_emit_kernel<<<blocks, 64 * kRpWaves, 0, s>>>(a, t0, t1);
    launch_prep_tasks(s, std::min((ub + 31) / 32, 8192), a.rv.st, sc, a.rv.rec, a.rv.yaw,
                      a.rv.tasks, a.tcost, a.rv.ext);
    launch_walk(kWalkBatchPlan, s, walk_blocks(ub, walk_grid_limit(kWalkBatchPlan, sc)), a.rv.st,
                sc, a.rv.rec, nullptr, a.rv.status, nullptr, nullptr, a.rv.wg_points);
    repair_choose_kernel<<<blocks, 64 * kRpWaves, 0, s>>>(a, sc, t0, t1);
    return hipGetLastError();
}

}  // namespace ppamd

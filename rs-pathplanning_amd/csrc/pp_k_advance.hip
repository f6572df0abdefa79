// pp_k_advance.hip — move the root of every RRT* tree to one of its nodes (pp_star_advance,
// DESIGN.md §3.8 "Advancing the root"; restated on the CPU in tests/star_advance_ref.py).
//
// Node r = root[q] of tree q becomes its root.  What hangs under r (K0) stays as it is, with its
// costs rebuilt from r down; the proper ancestors of r (A, the old root among them) point the
// wrong way and are round 1's tops of the repair's rounds (pp_k_repair.hip), which run unchanged
// on the staged arrays this unit fills.  Node g of the `total` nodes is node i = g - off[q] of
// tree q (row q * cap + i).  In stream order:
//   walk     one thread per query: the depth d of nodes[q], then the node min(hops[q], d) edges
//            from the root on its chain; every walk is bounded by the tree's size, and a chain
//            that does not reach the root leaves its query alone
//   words    one thread per node: v[0][g] = parent | bad << 31 in reval_settle_kernel's encoding,
//            with r as a root of its own and the old root bad; the revalidation's doubling
//            (launch_reval_jump) then leaves exactly K0 with the word g0 + r
//   init     one thread per node: the staged copies of the repair (flag, top, wpar, wcost,
//            welen), r staged as the root with level 1
//   cost     one wave per advanced query, level by level as repair_grow_kernel: cost'[i] =
//            cost'[parent[i]] + elen[i], one rounded f64 add per edge, parents before children
//            (no difference of old costs and no prefix sum: the order of the adds is the
//            contract, and pp_star_forest_import checks the sum)
//   tops     one thread per advanced query: A packed into tops[], counted in rec->ntops[1]
//   keep     one thread per node: the word launch_reval_scan(koff = null) keeps a node by
//   gather   one thread per node: r to index 0, every other kept node behind it in old index
//            order (its count of kept nodes below it, plus one when it lies below r), parents
//            remapped the same way, rows staged for reval_write_kernel
//   starts   one thread per advanced query: the written row 0 into the stored start
// A query with root[q] = 0 keeps every node, stages its own rows and is written back bit for bit.
// Nothing is written into the trees before the write, which a steer overflow (the error word)
// turns into a no-op, like the starts.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pp_kernels.h"
#include "pp_reval_dev.h"

namespace ppamd {

__global__ __launch_bounds__(kRvThreads) void advance_walk_kernel(AdvanceArgs a) {
    const RevalArgs& v = a.rp.rv;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= v.Q) return;
    const int n = v.off[q + 1] - v.off[q];
    const int* __restrict__ P = v.tr.parent + (size_t)q * v.cap;
    const int i = a.nodes[q];
    int r = 0;
    if (i > 0 && i < n) {
        int d = 0, j = i;
        bool ok = false;
        for (int step = 0; step < n; ++step) {
            if (j == 0) {
                ok = true;
                break;
            }
            const int p = P[j];
            if (p < 0 || p >= n || p == j) break;
            j = p;
            ++d;
        }
        if (ok) {
            const int h = a.hops ? std::min(a.hops[q], d) : d;
            j = i;
            for (int s = d - h; s > 0; --s) j = P[j];
            r = j;
        }
    }
    a.root[q] = r;
}

__global__ __launch_bounds__(kRvThreads) void advance_words_kernel(AdvanceArgs a) {
    const RevalArgs& v = a.rp.rv;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= v.total) return;
    const int q = rv_tree_of(v.off, v.Q, g);
    const int g0 = v.off[q], i = g - g0, n = v.off[q + 1] - g0;
    const int r = a.root[q];
    unsigned w;
    if (i == r) {  // a root of its own (r = 0: the tree's)
        w = (unsigned)g;
    } else if (i == 0) {  // the old root hangs from nothing
        w = (unsigned)g | kRvBad;
    } else {
        const int p = v.tr.parent[(size_t)q * v.cap + i];
        const bool live = p >= 0 && p < n && p != i;
        w = (unsigned)(g0 + (live ? p : 0)) | (live ? 0u : kRvBad);
    }
    v.v[0][g] = w;
}

__global__ __launch_bounds__(kRvThreads) void advance_init_kernel(AdvanceArgs a,
                                                                 const unsigned* __restrict__ vk) {
    const RepairArgs& p = a.rp;
    const RevalArgs& v = p.rv;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= v.total) return;
    const int q = rv_tree_of(v.off, v.Q, g);
    const int g0 = v.off[q], i = g - g0;
    const size_t row = (size_t)q * v.cap + (size_t)i;
    const int r = a.root[q];
    const bool newroot = r > 0 && i == r;
    p.flag[g] = r == 0 || vk[g] == (unsigned)(g0 + r) ? 1 : 0;
    p.top[g] = kTopNever;
    p.lvl[g] = newroot ? 1 : 0;
    p.wpar[g] = newroot ? -1 : v.tr.parent[row];
    p.wcost[g] = newroot ? 0.0 : v.cost[row];
    p.welen[g] = newroot ? 0.0 : v.elen[row];
}

__global__ __launch_bounds__(256) void advance_cost_kernel(AdvanceArgs a) {
    const RepairArgs& p = a.rp;
    const RevalArgs& v = p.rv;
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    for (int q = gw; q < v.Q; q += nw) {
        if (a.root[q] == 0) continue;
        const int g0 = v.off[q], n = v.off[q + 1] - g0;
        const unsigned char* __restrict__ F = p.flag + g0;
        int* __restrict__ L = p.lvl + g0;
        const int* __restrict__ P = p.wpar + g0;
        double* __restrict__ C = p.wcost + g0;
        const double* __restrict__ E = p.welen + g0;
        // this wave alone reads and writes query q's entries in this kernel; a pass compares
        // levels with cur and stores cur + 1, so it never reads what it wrote (repair_grow_kernel)
        for (int cur = 1; cur <= n; ++cur) {
            bool any = false;
            for (int j = lane; j < n; j += 64) {
                if (!(F[j] & 1)) continue;
                const int par = P[j];
                if (par < 0 || par >= n || L[par] != cur) continue;
                C[j] = C[par] + E[j];
                L[j] = cur + 1;
                any = true;
            }
            __threadfence_block();
            if (!__ballot(any)) break;
        }
    }
}

// (the chain r -> ... -> 0 is part of the chain the walk followed to the root)
__global__ __launch_bounds__(kRvThreads) void advance_tops_kernel(AdvanceArgs a) {
    const RepairArgs& p = a.rp;
    const RevalArgs& v = p.rv;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= v.Q) return;
    const int r = a.root[q];
    if (r == 0) return;
    const int g0 = v.off[q], n = v.off[q + 1] - g0;
    const int* __restrict__ P = v.tr.parent + (size_t)q * v.cap;
    int m = 0;
    for (int j = r; j != 0 && m < n; ++m) j = P[j];
    int slot = atomicAdd(&p.rec->ntops[1], m);
    int j = r;
    for (int s = 0; s < m; ++s) {
        j = P[j];
        p.tops[slot++] = g0 + j;
        p.top[g0 + j] = kTopNow;
    }
}

__global__ __launch_bounds__(kRvThreads) void advance_keep_kernel(AdvanceArgs a) {
    const RepairArgs& p = a.rp;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= p.rv.total) return;
    // rv_keep without offsets: kept unless bad, or its own ancestor
    p.vout[g] = (p.flag[g] & 1) ? 0u : kRvBad | (g == 0 ? 1u : 0u);
}

// the index after the call of kept node i of a tree whose kept nodes below i number `below`
__device__ __forceinline__ int adv_index(int i, int r, int below) {
    return i == r ? 0 : below + (i < r ? 1 : 0);
}

__global__ __launch_bounds__(kRvThreads) void advance_gather_kernel(AdvanceArgs a) {
    const RepairArgs& p = a.rp;
    const RevalArgs& v = p.rv;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= v.total) return;
    if (!(p.flag[g] & 1)) {
        v.new_index[g] = -1;
        return;
    }
    const int q = rv_tree_of(v.off, v.Q, g);
    const int g0 = v.off[q], i = g - g0, n = v.off[q + 1] - g0;
    const size_t o = (size_t)q * v.cap;
    const int r = a.root[q], base = v.pos[g0];
    const int j = adv_index(i, r, v.pos[g] - base);
    const int k = base + j;
    v.new_index[g] = j;
    v.sx[k] = v.tr.x[o + i];
    v.sy[k] = v.tr.y[o + i];
    v.syaw[k] = v.tr.yaw[o + i];
    const int par = p.wpar[g];  // (a kept node's parent is kept)
    v.spar[k] = par < 0 || par >= n ? par : adv_index(par, r, v.pos[g0 + par] - base);
    v.srow[k] = (long long)(o + j);
    v.scost[k] = p.wcost[g];
    v.selen[k] = p.welen[g];
}

__global__ __launch_bounds__(kRvThreads) void advance_starts_kernel(AdvanceArgs a) {
    const RevalArgs& v = a.rp.rv;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= v.Q || a.root[q] == 0 || *v.err) return;
    const size_t o = (size_t)q * v.cap;
    a.starts[3 * (size_t)q] = v.tr.x[o];
    a.starts[3 * (size_t)q + 1] = v.tr.y[o];
    a.starts[3 * (size_t)q + 2] = v.tr.yaw[o];
}

hipError_t launch_advance_stage(hipStream_t s, const AdvanceArgs& a, int stage, int passes) {
    const RevalArgs& v = a.rp.rv;
    if (v.total <= 0 || v.Q <= 0) return hipErrorInvalidValue;
    const int g = (v.total + kRvThreads - 1) / kRvThreads;
    const int gq = (v.Q + kRvThreads - 1) / kRvThreads;
    hipError_t e;
    switch (stage) {
    case kAdvanceCore:
        advance_walk_kernel<<<gq, kRvThreads, 0, s>>>(a);
        advance_words_kernel<<<g, kRvThreads, 0, s>>>(a);
        if ((e = launch_reval_jump(s, v, passes)) != hipSuccess) return e;
        advance_init_kernel<<<g, kRvThreads, 0, s>>>(a, v.v[passes & 1]);
        advance_cost_kernel<<<std::min((v.Q + 3) / 4, 4096), 256, 0, s>>>(a);
        break;
    case kAdvanceTops:  // what launch_repair_stage(kRepairTops) zeroes before a round
        if ((e = hipMemsetAsync(a.rp.lvl, 0, (size_t)v.total * sizeof(int), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(a.rp.qhas, 0, (size_t)v.Q, s)) != hipSuccess) return e;
        advance_tops_kernel<<<gq, kRvThreads, 0, s>>>(a);
        break;
    case kAdvanceKeep:
        advance_keep_kernel<<<g, kRvThreads, 0, s>>>(a);
        break;
    case kAdvanceGather:
        advance_gather_kernel<<<g, kRvThreads, 0, s>>>(a);
        break;
    case kAdvanceStarts:
        advance_starts_kernel<<<gq, kRvThreads, 0, s>>>(a);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ppamd

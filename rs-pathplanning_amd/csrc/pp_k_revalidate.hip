// pp_k_revalidate.hip — re-verify a tree (or a forest of per-query trees) against the current
// scene and drop what no longer verifies (pp_rrt_revalidate / pp_batch_revalidate /
// pp_star_revalidate).
//
// Node g of the `total` nodes (tree q's nodes at off[q] .. off[q + 1], row q * cap + i) keeps its
// place exactly when its own edge verifies and its parent keeps its place (RRT::verify_node's
// line_to_origin decomposes over the edges).  In stream order, no host round trip:
//   emit      one explicit steer task per node of a slice: the child keeps its stored yaw
//             (own_yaw), the parent pose comes from the parent's row, no cull.  A parent is an
//             earlier node of the tree; with any_order (RRT*: a rewired node hangs under the
//             later node that rewired it) any other node of the tree
//   prep/walk the steer round of pp_steer_launch.h on the slice (kWalkBatchPlan)
//   settle    literal-path verdicts re-run (slot-locked scratch pool); v[g] = ancestor | bad << 31
//   jump      pointer doubling over the ping-pong v arrays: after k passes v[g] covers the 2^k
//             edges above g.  Doubling needs no index order: a tree is acyclic, so a chain has
//             at most n - 1 edges wherever its parents sit, and ceil(log2(largest tree)) passes
//             are exact.  any_order: a chain that does not end in its tree's root (a cyclic
//             parent array) is dropped
//   scan      exclusive scan of keep over all nodes (per-workgroup counts, their scan, positions);
//             a tree's new indices are the positions less the position of its root
//   gather    kept rows (RRT*: with their cost / elen) into a compact staging copy with remapped
//             parents, new_index
//   write     staging back into the trees' rows (skipped when a steer overflowed: the trees stay)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pp_kernels.h"
#include "pp_reval_dev.h"
#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

constexpr int kRvScan = 1024;  // nodes per scan workgroup

__global__ __launch_bounds__(kRvThreads) void reval_emit_kernel(RevalArgs a, int base, int count) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {  // the slice's task count for the steer round
        a.st->W = count;
        a.st->ncomp = 0;
        a.st->alist = nullptr;
    }
    if (t >= count) return;
    const int g = base + t;
    const int q = rv_tree_of(a.off, a.Q, g);
    const int i = g - a.off[q];
    const size_t o = (size_t)q * a.cap;
    SteerTask tk{};
    StarTaskExt ex{};
    tk.pnode = -1;  // (idle: the root, or a parent index that is no earlier / no other node)
    ex.own_yaw = 1;
    ex.node = i;
    ex.pad = q;
    if (i > 0) {
        const int p = a.tr.parent[o + i];
        const bool live = a.any_order ? p >= 0 && p < a.off[q + 1] - a.off[q] && p != i
                                      : p >= 0 && p < i;
        if (live) {
            tk.x = a.tr.x[o + i];
            tk.y = a.tr.y[o + i];
            tk.px = a.tr.x[o + p];
            tk.py = a.tr.y[o + p];
            tk.pyaw = a.tr.yaw[o + p];
            tk.pnode = p;
            ex.cyaw = a.tr.yaw[o + i];
        }
    }
    a.tasks[t] = tk;
    a.ext[t] = ex;
}

// one lane per task, literal-path verdicts settled one at a time per wave (as star_settle)
__global__ __launch_bounds__(kRvThreads) void reval_settle_kernel(RevalArgs a, SceneDev sc,
                                                                 int base) {
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    const int W = a.st->W;
    for (int c = gw; c * 64 < W; c += nw) {
        const int t = c * 64 + lane;
        const bool has = t < W;
        SteerTask tk{};
        StarTaskExt ex{};
        int st = kReject;
        if (has) {
            tk = a.tasks[t];
            ex = a.ext[t];
            st = a.status[t];
        }
        const bool live = has && tk.pnode >= 0;
        uint64_t lit = __ballot(live && st == kLiteral);
        if (lit) {
            const int slot = lit_acquire(a.lit_locks, gw);
            double* bx = a.lit_scratch + (size_t)slot * 3 * kLiteralCap;
            for (; lit; lit &= lit - 1) {
                const int l = __builtin_ctzll(lit);
                const int r = steer_collide_literal(sc, __shfl(tk.x, l), __shfl(tk.y, l),
                                                    __shfl(ex.cyaw, l), __shfl(tk.px, l),
                                                    __shfl(tk.py, l), __shfl(tk.pyaw, l), bx,
                                                    bx + kLiteralCap, bx + 2 * kLiteralCap);
                if (lane == l) st = r;
            }
            lit_release(a.lit_locks, slot);
        }
        if (__ballot(live && st == kError) && lane == 0) atomicOr(a.err, 1);  // the reference panics
        if (!has) continue;
        const int g = base + t;
        unsigned v;
        if (ex.node == 0)  // the root stays; a blocked root fails every line that ends in it
            v = (unsigned)g | (a.blocked && a.blocked[ex.pad] ? kRvBad : 0u);
        else
            v = (unsigned)(a.off[ex.pad] + (live ? tk.pnode : 0)) |
                (live && st == kAccept ? 0u : kRvBad);
        a.v[0][g] = v;
    }
}

__global__ __launch_bounds__(kRvThreads) void reval_jump_kernel(const unsigned* __restrict__ in,
                                                               unsigned* __restrict__ out,
                                                               int total) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const unsigned v = in[g];
    const unsigned w = in[v & ~kRvBad];
    out[g] = (w & ~kRvBad) | ((v | w) & kRvBad);
}

// (off / Q: rv_keep's, null / 0 unless any_order)
__global__ __launch_bounds__(kRvScan) void reval_count_kernel(const unsigned* __restrict__ v,
                                                             int total, int* __restrict__ bsum,
                                                             const int* __restrict__ off, int Q) {
    const int g = blockIdx.x * kRvScan + threadIdx.x;
    const int c = __syncthreads_count(g < total && rv_keep(v[g < total ? g : 0], g, off, Q));
    if (threadIdx.x == 0) bsum[blockIdx.x] = c;
}

// exclusive scan of one value per thread over a kRvScan workgroup; *sum: the workgroup's total
__device__ inline int rv_block_scan(int val, int* sum) {
    __shared__ int s_w[kRvScan / 64 + 1];
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    int inc = val;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // (s_w of an earlier call has been read)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < kRvScan / 64; ++w) {
            const int x = s_w[w];
            s_w[w] = run;
            run += x;
        }
        s_w[kRvScan / 64] = run;
    }
    __syncthreads();
    *sum = s_w[kRvScan / 64];
    return s_w[wave] + inc - val;
}

// the workgroup counts into their exclusive scan, in place (one workgroup)
__global__ __launch_bounds__(kRvScan) void reval_bscan_kernel(int* __restrict__ bsum, int nb) {
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += kRvScan) {
        const int b = b0 + threadIdx.x;
        int sum;
        const int e = rv_block_scan(b < nb ? bsum[b] : 0, &sum);
        if (b < nb) bsum[b] = carry + e;
        carry += sum;
    }
}

__global__ __launch_bounds__(kRvScan) void reval_pos_kernel(const unsigned* __restrict__ v,
                                                           int total, const int* __restrict__ bsum,
                                                           int* __restrict__ pos,
                                                           const int* __restrict__ off, int Q) {
    const int g = blockIdx.x * kRvScan + threadIdx.x;
    const int k = g < total && rv_keep(v[g < total ? g : 0], g, off, Q) ? 1 : 0;
    int sum;
    const int e = bsum[blockIdx.x] + rv_block_scan(k, &sum);
    if (g < total) pos[g] = e;
    if (g == total - 1) pos[total] = e + k;
}

__global__ __launch_bounds__(kRvThreads) void reval_gather_kernel(RevalArgs a,
                                                                 const unsigned* __restrict__ v) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.total) return;
    if (!rv_keep(v[g], g, a.any_order ? a.off : nullptr, a.Q)) {
        a.new_index[g] = -1;
        return;
    }
    const int q = rv_tree_of(a.off, a.Q, g);
    const int g0 = a.off[q], i = g - g0;
    const size_t o = (size_t)q * a.cap;
    const int k = a.pos[g], j = k - a.pos[g0];
    a.new_index[g] = j;
    a.sx[k] = a.tr.x[o + i];
    a.sy[k] = a.tr.y[o + i];
    a.syaw[k] = a.tr.yaw[o + i];
    // (a kept node's parent is kept)
    a.spar[k] = i == 0 ? -1 : a.pos[g0 + a.tr.parent[o + i]] - a.pos[g0];
    a.srow[k] = (long long)(o + j);
    if (a.cost) {  // RRT*: dropping other nodes changes no kept node's cost
        a.scost[k] = a.cost[o + i];
        a.selen[k] = a.elen[o + i];
    }
}

// RRT*'s mark[] / stamp[] stay as they are: star_rewire_kernel compares a mark only for equality
// with the current stamp and relies on mark[row] < stamp[q] for every row of query q alone, which
// holds before the call and so after any move of rows (rows past the new n keep their contents)
__global__ __launch_bounds__(kRvThreads) void reval_write_kernel(RevalArgs a) {
    if (*a.err) return;  // a steer overflowed: the trees stay as they are
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < a.Q && a.n) a.n[k] = a.pos[a.off[k + 1]] - a.pos[a.off[k]];
    if (k >= a.pos[a.total]) return;
    const size_t row = (size_t)a.srow[k];
    const double x = a.sx[k], y = a.sy[k];
    a.tr.x[row] = x;
    a.tr.y[row] = y;
    a.tr.yaw[row] = a.syaw[k];
    a.tr.parent[row] = a.spar[k];
    if (a.cost) {
        a.cost[row] = a.scost[k];
        a.elen[row] = a.selen[k];
    }
    if (a.tr.x32) {  // the one-tree planner's f32 screen copies
        a.tr.x32[row] = (float)x;
        a.tr.y32[row] = (float)y;
    }
}

// The three stages of a revalidation, so that pp_star_repair can work between the jump and the
// compaction: the edge test into a.v[0], the doubling into a.v[passes & 1], the compaction of the
// nodes rv_keep keeps in v.  The compaction is its scan, its gather and its write; the scan and
// the write are launched on their own by pp_star_advance, around a gather that puts the new root
// first (pp_k_advance.hip).
hipError_t launch_reval_edges(hipStream_t s, const SceneDev& sc, const RevalArgs& a) {
    if (a.total <= 0 || a.slice <= 0) return hipErrorInvalidValue;
    const int limit = walk_grid_limit(kWalkBatchPlan, sc);
    for (int base = 0; base < a.total; base += a.slice) {
        const int count = std::min(a.slice, a.total - base);
        reval_emit_kernel<<<(count + kRvThreads - 1) / kRvThreads, kRvThreads, 0, s>>>(a, base, count);
        launch_prep_tasks(s, std::min((count + 31) / 32, 8192), a.st, sc, a.rec, a.yaw, a.tasks,
                          nullptr, a.ext);
        launch_walk(kWalkBatchPlan, s, walk_blocks(count, limit), a.st, sc, a.rec, nullptr,
                    a.status, nullptr, nullptr, a.wg_points);
        const int waves = (count + 63) / 64;
        reval_settle_kernel<<<std::min((waves + 3) / 4, 1024), kRvThreads, 0, s>>>(a, sc, base);
    }
    return hipGetLastError();
}

hipError_t launch_reval_jump(hipStream_t s, const RevalArgs& a, int passes) {
    const int g = (a.total + kRvThreads - 1) / kRvThreads;
    for (int p = 0; p < passes; ++p)
        reval_jump_kernel<<<g, kRvThreads, 0, s>>>(a.v[p & 1], a.v[(p + 1) & 1], a.total);
    return hipGetLastError();
}

hipError_t launch_reval_scan(hipStream_t s, const RevalArgs& a, const unsigned* v, const int* koff) {
    const int nb = (a.total + kRvScan - 1) / kRvScan;
    reval_count_kernel<<<nb, kRvScan, 0, s>>>(v, a.total, a.bsum, koff, a.Q);
    reval_bscan_kernel<<<1, kRvScan, 0, s>>>(a.bsum, nb);
    reval_pos_kernel<<<nb, kRvScan, 0, s>>>(v, a.total, a.bsum, a.pos, koff, a.Q);
    return hipGetLastError();
}

hipError_t launch_reval_write(hipStream_t s, const RevalArgs& a) {
    reval_write_kernel<<<(std::max(a.total, a.Q) + kRvThreads - 1) / kRvThreads, kRvThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_reval_compact(hipStream_t s, const RevalArgs& a, const unsigned* v) {
    const int g = (a.total + kRvThreads - 1) / kRvThreads;
    hipError_t e = launch_reval_scan(s, a, v, a.any_order ? a.off : nullptr);
    if (e != hipSuccess) return e;
    reval_gather_kernel<<<g, kRvThreads, 0, s>>>(a, v);
    return launch_reval_write(s, a);
}

hipError_t launch_revalidate(hipStream_t s, const SceneDev& sc, const RevalArgs& a, int passes) {
    hipError_t e = launch_reval_edges(s, sc, a);
    if (e != hipSuccess) return e;
    if ((e = launch_reval_jump(s, a, passes)) != hipSuccess) return e;
    return launch_reval_compact(s, a, a.v[passes & 1]);
}

}  // namespace ppamd

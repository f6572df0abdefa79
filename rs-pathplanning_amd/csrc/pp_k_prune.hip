// pp_k_prune.hip — the verdicts of pp_star_prune (DESIGN.md §3.7 "Pruning by the focus bound"): an
// RRT* forest's nodes that, at their stored cost, cannot lie on a path to their query's focus
// within its bound.  The two kernels write the keep words v[0][g] = ancestor | bad << 31 in
// reval_settle_kernel's encoding; the doubling and the compaction that follow are the
// revalidation's own (launch_reval_jump, launch_reval_compact: pp_k_revalidate.hip).
//   mark     one thread per node: bad iff cost * R + |node - focus| > L (f64; the unit is built
//            with -ffp-contract=off like star_sample_kernel's focus test, so every product and sum
//            is rounded on its own, and sqrt is the correctly rounded one), or its parent is no
//            other node of its tree (emit's `live` test)
//   protect  one thread per query with a keep node: the bad bit of every node on the chain
//            keep -> parent -> ... -> root is cleared again
#include <hip/hip_runtime.h>

#include "pp_kernels.h"
#include "pp_reval_dev.h"

namespace ppamd {

// (threads of a wave mostly share a tree: the three per-query loads are near-uniform)
__global__ __launch_bounds__(kRvThreads) void prune_mark_kernel(PruneArgs p) {
    const RevalArgs& a = p.rv;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.total) return;
    const int q = rv_tree_of(a.off, a.Q, g);
    const int g0 = a.off[q], i = g - g0;
    if (i == 0) {  // the root stays
        a.v[0][g] = (unsigned)g;
        return;
    }
    const size_t o = (size_t)q * a.cap;
    const int par = a.tr.parent[o + i];
    const bool live = par >= 0 && par < a.off[q + 1] - g0 && par != i;
    const double dx = a.tr.x[o + i] - p.fxy[2 * (size_t)q];
    const double dy = a.tr.y[o + i] - p.fxy[2 * (size_t)q + 1];
    const bool fails = a.cost[o + i] * p.R + sqrt(dx * dx + dy * dy) > p.fbound[q];
    a.v[0][g] = (unsigned)(g0 + (live ? par : 0)) | (live && !fails ? 0u : kRvBad);
}

// A node without a live parent keeps its bad bit (its word points at the root, not at a parent the
// compaction could remap) and ends the walk; so does the n-th step of a cyclic parent array.
__global__ __launch_bounds__(kRvThreads) void prune_protect_kernel(PruneArgs p) {
    const RevalArgs& a = p.rv;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.Q) return;
    int i = p.keep[q];
    const int g0 = a.off[q], n = a.off[q + 1] - g0;
    if (i < 0 || i >= n) return;
    const size_t o = (size_t)q * a.cap;
    for (int step = 0; step < n && i > 0; ++step) {
        const int par = a.tr.parent[o + i];
        if (par < 0 || par >= n || par == i) return;
        a.v[0][g0 + i] &= ~kRvBad;
        i = par;
    }
}

hipError_t launch_prune_verdicts(hipStream_t s, const PruneArgs& p) {
    if (p.rv.total <= 0) return hipErrorInvalidValue;
    prune_mark_kernel<<<(p.rv.total + kRvThreads - 1) / kRvThreads, kRvThreads, 0, s>>>(p);
    if (p.keep)
        prune_protect_kernel<<<(p.rv.Q + kRvThreads - 1) / kRvThreads, kRvThreads, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace ppamd

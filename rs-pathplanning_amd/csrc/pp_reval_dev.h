// pp_reval_dev.h — the device helpers the revalidation kernels (pp_k_revalidate.hip) and the
// repair kernels (pp_k_repair.hip) share: the keep word v[g] = ancestor | bad << 31 and the tree
// of a global node index.
#pragma once

#include <hip/hip_runtime.h>

namespace ppamd {

constexpr unsigned kRvBad = 0x80000000u;
constexpr int kRvThreads = 256;

// the tree of node g: the last q with off[q] <= g
__device__ inline int rv_tree_of(const int* __restrict__ off, int Q, int g) {
    int lo = 0, hi = Q;  // off[lo] <= g < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a root's ancestor is itself (every other node's is an earlier node).  off != null (any_order):
// parents come in any order, so the final ancestor must also be the root of g's tree — a chain
// that never reaches it is dropped, not kept
__device__ inline bool rv_keep(unsigned v, int g, const int* __restrict__ off, int Q) {
    const unsigned anc = v & ~kRvBad;
    if (off) {
        const unsigned g0 = (unsigned)off[rv_tree_of(off, Q, g)];
        return anc == g0 && (!(v & kRvBad) || (unsigned)g == g0);
    }
    return !(v & kRvBad) || anc == (unsigned)g;
}

}  // namespace ppamd

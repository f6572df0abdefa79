// pp_k_forest_io.hip — the kernels of the packed forest export / import: the
// complete state of a set of query slots out of a batch's forest and into one.
//   sizes     one workgroup: the exclusive scan of the served slots' node counts into off[0 .. m],
//             and the slots' per-query values into the staged per-slot arrays
//   gather    one thread per packed row (paths_kernel's write-pass mapping: consecutive lanes,
//             consecutive addresses on both sides within a tree): forest rows -> staged rows
//   validate  one wave per staged tree: the parent rules, then the tree level by level from its
//             root (star_rewire_kernel's propagation): a node joins level s + 1 when its parent
//             sits on level s, and takes cost[parent] + elen as one f64 addition (the unit is
//             built with -ffp-contract=off).  Index order plays no part: a rewired node's parent
//             may be a later node.  A pass that reaches nobody ends the loop, so a cycle or an
//             island terminates it and shows as nodes left on level 0; the tree's verdict goes to
//             verdict[i], one word per served slot
//   scatter   gather's inverse, the per-slot values, and the slots' derived state (RRT*: mark rows
//             0 and stamp 1, star_init_kernel's; the extend batch: the verdict cache voided)
#include <hip/hip_runtime.h>

#include "pp_kernels.h"

namespace ppamd {

constexpr int kFioThreads = 256;
constexpr int kFioScan = 1024;

// the served slot of packed row k: the last i with off[i] <= k (every served tree has a row)
__device__ inline int fio_slot_of(const int64_t* __restrict__ off, int m, int64_t k) {
    int lo = 0, hi = m;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kFioScan) void fio_sizes_kernel(ForestIoArgs a) {
    __shared__ int64_t s_w[kFioScan / 64 + 1];
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int i0 = 0; i0 < a.m; i0 += kFioScan) {
        const int i = i0 + (int)threadIdx.x;
        const int q = i < a.m ? a.slots[i] : 0;
        const int64_t val = i < a.m ? a.n[q] : 0;
        int64_t inc = val;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        __syncthreads();  // (s_w of the chunk before has been read)
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t run = 0;
            for (int w = 0; w < kFioScan / 64; ++w) {
                const int64_t x = s_w[w];
                s_w[w] = run;
                run += x;
            }
            s_w[kFioScan / 64] = run;
        }
        __syncthreads();
        if (i < a.m) {
            a.off[i] = carry + s_w[wave] + inc - val;
            a.sit[i] = a.it[q];
            a.sevals[i] = a.evals[q];
            a.sseed[i] = a.seed[q];
            if (a.rew) {  // RRT*
                a.srew[i] = a.rew[q];
                a.sfxy[2 * (size_t)i] = a.fxy[2 * (size_t)q];
                a.sfxy[2 * (size_t)i + 1] = a.fxy[2 * (size_t)q + 1];
                a.sfbound[i] = a.fbound[q];
                a.sskipped[i] = a.skipped[q];
            }
        }
        carry += s_w[kFioScan / 64];
    }
    if (threadIdx.x == 0) a.off[a.m] = carry;
}

__global__ __launch_bounds__(kFioThreads) void fio_gather_kernel(ForestIoArgs a) {
    const int64_t k = (int64_t)blockIdx.x * kFioThreads + threadIdx.x;
    if (k >= a.total) return;
    const int i = fio_slot_of(a.off, a.m, k);
    const size_t row = (size_t)a.slots[i] * a.cap + (size_t)(k - a.off[i]);
    if (a.sx) a.sx[k] = a.tr.x[row];
    if (a.sy) a.sy[k] = a.tr.y[row];
    if (a.syaw) a.syaw[k] = a.tr.yaw[row];
    if (a.spar) a.spar[k] = a.tr.parent[row];
    if (a.scost) a.scost[k] = a.cost[row];
    if (a.selen) a.selen[k] = a.elen[row];
}

// the wave's maximum of a small non-negative code
__device__ inline int fio_wave_max(int v) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(kFioThreads) void fio_validate_kernel(ForestIoArgs a) {
    const int lane = __lane_id();
    const int i = (int)blockIdx.x * (kFioThreads / 64) + (int)(threadIdx.x >> 6);
    if (i >= a.m) return;  // (wave-uniform)
    const int64_t g0 = a.off[i];
    const int n = (int)(a.off[i + 1] - g0);
    const int* __restrict__ par = a.spar + g0;
    int bad = kFioOk;
    for (int j = lane; j < n; j += 64) {
        const int p = par[j];
        int code = kFioOk;
        if (j == 0) {
            if (p != -1) code = kFioRoot;
        } else if (p < 0 || p >= n || p == j) {
            code = kFioParent;
        } else if (a.ordered && p >= j) {
            code = kFioOrder;
        }
        if (code != kFioOk && (bad == kFioOk || code < bad)) bad = code;
    }
    // the lowest rule number broken anywhere in the tree (0 where none is)
    const int worst = fio_wave_max(bad == kFioOk ? 0 : 8 - bad);
    if (worst) {
        if (lane == 0) a.verdict[i] = 8 - worst;
        return;
    }
    if (a.ordered) {  // parent[j] < j for every j > 0: every chain ends in row 0
        if (lane == 0) a.verdict[i] = kFioOk;
        return;
    }
    // level by level from the root.  This wave alone reads and writes tree i's staged rows, so its
    // lanes exchange them through the CU's own cache behind a workgroup-scope fence
    // (star_rewire_kernel's argument)
    int* lvl = a.lvl + g0;
    double* cost = a.scost + g0;
    const double* __restrict__ elen = a.selen + g0;
    for (int j = lane; j < n; j += 64) lvl[j] = j == 0 ? 1 : 0;
    if (lane == 0) cost[0] = 0.0;
    __threadfence_block();
    int reached = lane == 0 ? 1 : 0;
    for (int s = 1; s <= n; ++s) {  // (a level holds a node: at most n - 1 productive passes)
        bool any = false;
        for (int j = lane; j < n; j += 64) {
            if (lvl[j] != 0) continue;
            const int p = par[j];
            if (lvl[p] == s) {
                cost[j] = cost[p] + elen[j];
                lvl[j] = s + 1;
                any = true;
                ++reached;
            }
        }
        __threadfence_block();
        if (!__ballot(any)) break;
    }
    for (int d = 32; d > 0; d >>= 1) reached += __shfl_xor(reached, d);
    int v = reached == n ? kFioOk : kFioUnreached;
    if (v == kFioOk && a.scost_in) {
        const double* __restrict__ given = a.scost_in + g0;
        bool diff = false;
        for (int j = lane; j < n; j += 64)
            diff |= __double_as_longlong(given[j]) != __double_as_longlong(cost[j]);
        if (__ballot(diff)) v = kFioCost;
    }
    if (lane == 0) a.verdict[i] = v;
}

__global__ __launch_bounds__(kFioThreads) void fio_scatter_kernel(ForestIoArgs a) {
    const int64_t k = (int64_t)blockIdx.x * kFioThreads + threadIdx.x;
    if (k >= a.total) return;
    const int i = fio_slot_of(a.off, a.m, k);
    const size_t row = (size_t)a.slots[i] * a.cap + (size_t)(k - a.off[i]);
    a.tr.x[row] = a.sx[k];
    a.tr.y[row] = a.sy[k];
    a.tr.yaw[row] = a.syaw[k];
    a.tr.parent[row] = a.spar[k];
    if (a.cost) {
        a.cost[row] = a.scost[k];
        a.elen[row] = a.selen[k];
    }
}

// RRT*'s rewire scratch of the served slots as pp_star_new leaves it: every row's mark below the
// stamp (rows past the tree too: a later insert lands there with the mark it finds)
__global__ __launch_bounds__(kFioThreads) void fio_mark_kernel(ForestIoArgs a, int blocks_per_slot) {
    const int i = (int)(blockIdx.x / (unsigned)blocks_per_slot);
    const size_t j = (size_t)(blockIdx.x % (unsigned)blocks_per_slot) * kFioThreads + threadIdx.x;
    if (j < a.cap) a.mark[(size_t)a.slots[i] * a.cap + j] = 0;
}

__global__ __launch_bounds__(kFioThreads) void fio_slots_kernel(ForestIoArgs a) {
    const int i = (int)(blockIdx.x * kFioThreads + threadIdx.x);
    if (i >= a.m) return;
    const int q = a.slots[i];
    const int64_t g0 = a.off[i];
    a.n[q] = (int)(a.off[i + 1] - g0);
    a.it[q] = a.sit[i];
    a.evals[q] = a.sevals[i];
    a.seed[q] = a.sseed[i];
    a.starts[3 * (size_t)q] = a.sx[g0];
    a.starts[3 * (size_t)q + 1] = a.sy[g0];
    a.starts[3 * (size_t)q + 2] = a.syaw[g0];
    if (a.blocked) a.blocked[q] = a.sblocked ? a.sblocked[i] : 0;
    if (a.rew) {  // RRT*
        a.rew[q] = a.srew[i];
        a.fxy[2 * (size_t)q] = a.sfxy[2 * (size_t)i];
        a.fxy[2 * (size_t)q + 1] = a.sfxy[2 * (size_t)i + 1];
        a.fbound[q] = a.sfbound[i];
        a.skipped[q] = a.sskipped[i];
        a.stamp[q] = 1;
    }
    // the verdict cache starts empty: it_prev far below any iteration (pp_batch_new's 0x80 bytes)
    if (a.itprev) a.itprev[q] = (int64_t)0x8080808080808080ull;
}

static unsigned fio_row_blocks(int64_t total) { return (unsigned)((total + kFioThreads - 1) / kFioThreads); }

hipError_t launch_forest_sizes(hipStream_t s, const ForestIoArgs& a) {
    if (a.m <= 0) return hipErrorInvalidValue;
    fio_sizes_kernel<<<1, kFioScan, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_forest_gather(hipStream_t s, const ForestIoArgs& a) {
    if (a.total <= 0) return hipErrorInvalidValue;
    fio_gather_kernel<<<fio_row_blocks(a.total), kFioThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_forest_validate(hipStream_t s, const ForestIoArgs& a) {
    if (a.m <= 0) return hipErrorInvalidValue;
    const int waves = kFioThreads / 64;
    fio_validate_kernel<<<(a.m + waves - 1) / waves, kFioThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_forest_scatter(hipStream_t s, const ForestIoArgs& a) {
    if (a.m <= 0 || a.total <= 0) return hipErrorInvalidValue;
    fio_scatter_kernel<<<fio_row_blocks(a.total), kFioThreads, 0, s>>>(a);
    if (a.mark) {
        const int bps = (int)((a.cap + kFioThreads - 1) / kFioThreads);
        fio_mark_kernel<<<(unsigned)a.m * (unsigned)bps, kFioThreads, 0, s>>>(a, bps);
    }
    fio_slots_kernel<<<(a.m + kFioThreads - 1) / kFioThreads, kFioThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ppamd

// pp_k_segments.hip — planned paths as Dubins segments, and their sampling (DESIGN.md §3.7
// "Segment export and sampling").
//   segments_kernel<P, kWrite>  one wave per line item over a pose provider (pp_chain_dev.h): a
//                               lane per edge in rounds of 64 — the edge's word by the same
//                               select_word call on the same local coordinates as the point
//                               export's cf_npoint_steer, then its three arc / straight / arc
//                               records serially, stored straight into the packed SoA row (or its
//                               mirror for reverse).  The count pass only needs E and the None
//                               flags.  No points, no line buffers, no literal pool.
//                               (CsrChainPoses: the chain is the caller's, no ancestor path.)
//   segments_prefix_kernel      one wave per row: the running arc position in row order (serial
//                               f64 additions, as the restatement's) and the row's sample count
//   segments_sample_kernel      one thread per sample: its row by binary search in poff, its
//                               segment by binary search in the row's P, the closed form
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "pp_chain_dev.h"
#include "pp_device.h"
#include "pp_kernels.h"

namespace ppamd {

constexpr int kSegThreads = 64;  // one wave per item (cf_path and the None ballots are wave-wide)

// the word of the edge a -> b: cf_npoint_steer's expressions.  Out of line: select_word's six
// closed forms are the register-heavy part, and the kernel's own body is bookkeeping.
__device__ __noinline__ Steer seg_word(double turn_radius, double ax, double ay, double ayaw,
                                       double bx, double by, double byaw) {
    const double ex = bx - ax, ey = by - ay;
    const double c = 1.0 / turn_radius;
    const double lex = cos(ayaw) * ex + sin(ayaw) * ey;
    const double ley = -(sin(ayaw)) * ex + cos(ayaw) * ey;
    return select_word(lex, ley, byaw - ayaw, c);
}

// the closed-form end of a segment of signed curvature k from (x, y, yaw), u along it
__device__ inline CfPose seg_end(double x, double y, double yaw, double k, double u) {
    if (k == 0.0) return CfPose{x + u * cos(yaw), y + u * sin(yaw), yaw};
    const double yaw1 = yaw + k * u;
    double s0, c0, s1, c1;
    sincos(yaw, &s0, &c0);
    sincos(yaw1, &s1, &c1);
    return CfPose{x + (s1 - s0) / k, y - (c1 - c0) / k, yaw1};
}

// a chain deeper than this tier's path: the item goes to the spill list (or err |= 1)
__device__ inline void seg_spill(const SegArgs& a, const int* o, int tid, int* err) {
    if (!a.spill) {
        if (tid == 0) atomicOr(err, 1);
        return;
    }
    int w = 0;
    if (tid == 0) w = atomicAdd(&a.spill[0], 1);
    w = __shfl(w, 0);
    if (w >= a.spill_cap) {
        if (tid == 0) atomicOr(err, 1);
    } else if (tid < kCfItem) {
        a.spill[1 + (size_t)w * kCfItem + tid] = o[tid];
    }
}

template <class P, bool kWrite>
__global__ __launch_bounds__(kSegThreads) void segments_kernel(SegArgs a, int* __restrict__ err,
                                                               const int* __restrict__ items,
                                                               int items_cap) {
    __shared__ int s_pos[kCfLevels];
    const int tid = threadIdx.x;
    int* path = a.path + (size_t)blockIdx.x * a.path_cap;
    const int n_items = min(items[0], items_cap);
    const double R = a.turn_radius;
    const double kl = 1.0 / R;
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int* o = items + 1 + (size_t)it * kCfItem;
        const int b = o[0];
        __syncthreads();  // path and s_pos served the previous item
        if (tid < kCfLevels) s_pos[tid] = o[4 + tid];
        const int q = a.qidx[b];
        TreeDev tr = a.tr;
        const size_t ro = (size_t)q * a.row_cap;
        tr.x += ro;
        tr.y += ro;
        tr.yaw += ro;
        tr.parent += ro;
        int D;
        const int* cpath = path;
        if constexpr (std::is_same<P, CsrChainPoses>::value) {  // the caller's chain, as given
            cpath = a.cchain + a.coff[q];
            D = (int)(a.coff[q + 1] - a.coff[q]);
        } else {
            D = cf_path(tr, a.nodes[b], path, a.path_cap);
        }
        __syncthreads();
        if (D < 0) {
            seg_spill(a, o, tid, err);
            continue;
        }
        const P p(tr, cpath, D, o, s_pos, a.goals + 3 * (size_t)q);
        const int E = p.edges();
        int64_t base = 0;
        if (kWrite) {
            // the packed row: the count pass and the scan sized it (an empty row: the goal edge
            // had no word); anything else is a bug, never a store outside the row
            base = a.off[q];
            const int64_t n = a.off[q + 1] - base;
            if (n == 0) continue;
            if (n != 3 * (int64_t)E) {
                if (tid == 0) atomicOr(err, 16);
                continue;
            }
        }
        bool none = false, none0 = false;
        for (int e0 = 0; e0 < E; e0 += 64) {
            const int e = e0 + tid;
            bool nw = false;
            if (e < E) {
                const CfPose pa = p.pose(e), pb = p.pose(e + 1);
                const Steer w = seg_word(R, pa.x, pa.y, pa.yaw, pb.x, pb.y, pb.yaw);
                nw = w.word < 0;
                if (kWrite && !nw) {
                    const double tpq[3] = {w.t, w.p, w.q};
                    double x = pa.x, y = pa.y, yaw = pa.yaw;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int m = word_mode(w.word, j);
                        const double k = m == kModeS ? 0.0 : (m == kModeL ? kl : -kl);
                        const double len = tpq[j] * R;
                        const CfPose en = seg_end(x, y, yaw, k, len);
                        const int64_t r = 3 * (int64_t)e + j;
                        const int64_t at = base + (a.reverse ? 3 * (int64_t)E - 1 - r : r);
                        if (a.reverse) {
                            if (a.ox) a.ox[at] = en.x;
                            if (a.oy) a.oy[at] = en.y;
                            if (a.oyaw) a.oyaw[at] = en.yaw + kPi;
                            if (a.okappa) a.okappa[at] = k == 0.0 ? 0.0 : -k;
                        } else {
                            if (a.ox) a.ox[at] = x;
                            if (a.oy) a.oy[at] = y;
                            if (a.oyaw) a.oyaw[at] = yaw;
                            if (a.okappa) a.okappa[at] = k;
                        }
                        if (a.olen) a.olen[at] = len;
                        x = en.x;
                        y = en.y;
                        yaw = en.yaw;
                    }
                }
            }
            const uint64_t nm = __ballot(nw);
            if (nm) {
                none0 |= e0 == 0 && (nm & 1);
                none |= (nm & ~(e0 == 0 ? 1ull : 0ull)) != 0;
            }
        }
        if (none || (none0 && !P::kGoalNoneOk)) {
            if (tid == 0) atomicOr(err, 2);
            continue;
        }
        if (!kWrite && tid == 0) {
            a.cnt[b] = none0 ? 0 : 3 * E;
            if (a.okf) a.okf[b] = none0 ? 0 : 1;
        }
    }
}

template <class P>
static hipError_t launch_segments_t(hipStream_t st, const SegArgs& a, int grid, int* err,
                                    const int* items, int items_cap, bool write) {
    if (write) segments_kernel<P, true><<<grid, kSegThreads, 0, st>>>(a, err, items, items_cap);
    else segments_kernel<P, false><<<grid, kSegThreads, 0, st>>>(a, err, items, items_cap);
    return hipGetLastError();
}

hipError_t launch_segments(hipStream_t st, const SegArgs& a, int grid, int* err, const int* items,
                           int items_cap, bool star, bool write) {
    if (grid <= 0) return hipSuccess;
    if (star && a.cchain)
        return launch_segments_t<CsrChainPoses>(st, a, grid, err, items, items_cap, write);
    return star ? launch_segments_t<StarChainPoses>(st, a, grid, err, items, items_cap, write)
                : launch_segments_t<CfChainPoses>(st, a, grid, err, items, items_cap, write);
}

// ------------------------------------------------------------------------------- the sampler

constexpr int kSegPrefixThreads = 256;  // 4 rows (waves) a workgroup
constexpr int kSegSampleThreads = 256;

__global__ __launch_bounds__(kSegPrefixThreads) void segments_prefix_kernel(SegSampleArgs a) {
    const int lane = __lane_id();
    const int gw = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    for (int r = gw; r < a.q; r += nw) {
        const int64_t j0 = a.off[r], j1 = a.off[r + 1];
        double run = 0.0;
        for (int64_t c0 = j0; c0 < j1; c0 += 64) {
            const int64_t j = c0 + lane;
            const double l = j < j1 ? a.len[j] : 0.0;
            const int m = (int)min((int64_t)64, j1 - c0);
            double mine = 0.0;
            for (int i = 0; i < m; ++i) {  // row order: one addition a segment
                run += readlane_f64(l, i);
                if (i == lane) mine = run;
            }
            if (j < j1) a.P[j] = mine;
        }
        if (lane == 0) {
            int64_t nf = 0, cnt = 0;
            if (j1 > j0) {
                const double f = floor(run / a.ds);
                nf = f < (double)a.max_samples ? (int64_t)f : a.max_samples;
                cnt = nf + 1 + (run > (double)nf * a.ds ? 1 : 0);
            }
            a.rowlen[r] = run;
            a.nfull[r] = nf;
            a.cnt[r] = cnt;
        }
    }
}

__global__ __launch_bounds__(kSegSampleThreads) void segments_sample_kernel(SegSampleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kSegSampleThreads + threadIdx.x;
    if (i >= a.total) return;
    // the row: the last r with poff[r] <= i (a row without samples is never that one)
    int lo = 0, hi = a.q;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.poff[mid] <= i) lo = mid;
        else hi = mid;
    }
    const int r = lo;
    const int64_t k = i - a.poff[r];
    const double s = k <= a.nfull[r] ? (double)k * a.ds : a.rowlen[r];
    // the first segment with s < P[j], else the last at its end
    const int64_t j0 = a.off[r], j1 = a.off[r + 1];
    int64_t jl = j0, jh = j1;
    while (jl < jh) {
        const int64_t mid = (jl + jh) >> 1;
        if (s < a.P[mid]) jh = mid;
        else jl = mid + 1;
    }
    int64_t j = jl;
    double u;
    if (j >= j1) {
        j = j1 - 1;
        u = a.len[j];
    } else {
        u = s - (j > j0 ? a.P[j - 1] : 0.0);
    }
    const double kap = a.kappa[j];
    const CfPose en = seg_end(a.x[j], a.y[j], a.yaw[j], kap, u);
    if (a.sx) a.sx[i] = en.x;
    if (a.sy) a.sy[i] = en.y;
    if (a.syaw) a.syaw[i] = en.yaw;
    if (a.skappa) a.skappa[i] = kap;
    if (a.ss) a.ss[i] = s;
}

hipError_t launch_segments_prefix(hipStream_t st, const SegSampleArgs& a) {
    if (a.q <= 0) return hipSuccess;
    const int grid = std::min((a.q + 3) / 4, 4096);
    segments_prefix_kernel<<<grid, kSegPrefixThreads, 0, st>>>(a);
    return hipGetLastError();
}

hipError_t launch_segments_sample(hipStream_t st, const SegSampleArgs& a) {
    if (a.total <= 0) return hipSuccess;
    const int64_t grid = (a.total + kSegSampleThreads - 1) / kSegSampleThreads;
    segments_sample_kernel<<<(unsigned)grid, kSegSampleThreads, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace ppamd

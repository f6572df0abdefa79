// pp_k_star.hip — hand-written CDNA4 (gfx950) kernels of the RRT* query batch (config 5, DESIGN.md
// §3.7): the lockstep step's star_sample, star_knn, star_insert and star_rewire around the steer
// rounds, star_init, and the goal connection (star_goal_*).
// steer_prep and steer_walk are compiled by pp_k_steer.hip alone and launched through
// pp_steer_launch.h; the device code the units inline is pp_steer_dev.h.
//
// No MFMA anywhere: there is no dense contraction on this path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pp_kernels.h"

// The literal paths of star_insert_kernel, star_rewire_kernel and star_goal_reduce_kernel are
// this unit's only callers of select_word, and the inliner folds the last use of a local
// function in (each kernel grows by about 2,450 lines), so this unit's
// own declaration pins it out of line, as the single file compiled it.  It has to precede the
// definition in pp_device.h (after it the compiler ignores the attribute, with a warning).
namespace ppamd {
struct Steer;
__device__ __noinline__ Steer select_word(double lex, double ley, double leyaw, double c);
}  // namespace ppamd

#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

// ------------------------------------------------------- RRT* query batch (config 5, §3.7)
//
// One lockstep step = one RRT* iteration of every query (oracle/pp_oracle.c orc_star_extend):
//   star_sample    one wave per query: rand_point (with a focus: the first draw inside the
//                  query's ellipse, 64 draws a wave round), the exact nearest node, Steer(eta)
//                  and the gate task (new → nearest)                              → round A
//   star_knn       gated queries: X_near = the k nearest nodes of the new point (exact f64,
//                  (d2, index) order, distances cached in LDS), one choose-parent task per
//                  X_near node other than the nearest                               → round B
//   star_insert    the first strict minimum of cost(p) + edge cost over the feasible candidates
//                  (nearest first), the append, one rewire task per X_near node that could
//                  still get cheaper (cost(new) < cost(m))                          → round C
//   star_rewire    the rewires in X_near order against the costs as they stand, each followed by
//                  a level-synchronous recomputation of the rewired node's subtree costs
// Rounds A/B/C are the window pipeline's steer_prep / steer_walk on explicit tasks; their task
// counts live in DevState W (stA: Q, stB / stC: counted on the device), so a step needs no host
// round trip.
constexpr int kKnnWaves = 4;
constexpr int kKnnCache = 2048;  // d2 values cached per wave (LDS: 4 x 16 KB)

__device__ __forceinline__ bool star_feasible(int status, double e) {
    return status == kAccept && e <= 1.7976931348623157e308;  // Some and verified (finite cost)
}

// Bitonic sort of one (d, i) pair per lane across the wave, ascending in (d, i) lexicographic
// order (lane r ends up with the r-th smallest): 21 compare-exchange stages over __shfl_xor.
struct Kv {
    double d;
    int i;
};
__device__ __forceinline__ Kv bitonic64(double d, int lane, int i = 0) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const double od = __shfl_xor(d, stride);
            const int oi = __shfl_xor(i, stride);
            const bool other_less = od < d || (od == d && oi < i);
            const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0 || size == 64);
            if (keep_min == other_less) {
                d = od;
                i = oi;
            }
        }
    }
    return Kv{d, i};
}

// exact lower bound of an edge's Dubins cost (normalised by the turn radius): the chord, with a
// slack far above the rounding of both (prunes only what cannot win, so results are unchanged)
__device__ __forceinline__ double star_chord_lb(double d2, double curv) {
    return sqrt(d2) * curv * (1.0 - 1e-9) - 1e-9;
}

__global__ __launch_bounds__(256) void star_sample_kernel(StarDev sd, double minx, double maxx,
                                                          double miny, double maxy,
                                                          SteerTask* __restrict__ tasks) {
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the step's round-B / round-C task counters
        sd.stB->W = 0;
        sd.stC->W = 0;
    }
    const MqDev& mq = sd.mq;
    for (int q = gw; q < mq.Q; q += nw) {
        const int64_t it = mq.it[q];
        // (the query's other scalars are read with it: one load latency, not one per use)
        const uint64_t seed = mq.seed[q];
        const int64_t skipped = sd.skipped[q];
        const double L = sd.fbound[q];  // (wave-uniform; +inf: no focus)
        if (it >= mq.target[q]) {
            if (lane == 0) {
                tasks[q].pnode = -1;
                sd.pn[q] = -1;
            }
            continue;
        }
        const size_t row = (size_t)q * mq.cap;
        const double* __restrict__ X = mq.x + row;
        const double* __restrict__ Y = mq.y + row;
        // focused sampling (§3.7): the draw counter runs `skipped` ahead of the iteration; with a
        // finite bound L the sample is the first of the next kStarFocusDraws draws whose distances
        // to the root and to the focus sum to less than L — 64 draws a round, one per lane
        uint64_t d = (uint64_t)it + (uint64_t)skipped;
        if (L < __builtin_inf()) {
            const double x0 = X[0], y0 = Y[0];
            const double fx = sd.fxy[2 * (size_t)q], fy = sd.fxy[2 * (size_t)q + 1];
            int hit = -1;
            for (int r = 0; r < kStarFocusDraws / 64; ++r) {
                const uint64_t dl = d + (uint64_t)(64 * r + lane);
                const double sx = gen_range(seed, 2 * dl, minx, maxx);
                const double sy = gen_range(seed, 2 * dl + 1, miny, maxy);
                const double ax = sx - x0, ay = sy - y0, bx = sx - fx, by = sy - fy;
                const uint64_t in = __ballot(sqrt(ax * ax + ay * ay) + sqrt(bx * bx + by * by) < L);
                if (in) {  // the lowest draw of the round; every lane redraws it below
                    hit = 64 * r + (int)__builtin_ctzll(in);
                    break;
                }
            }
            if (hit < 0) {  // no draw in the set: the iteration ends here (star_knn never sees it)
                if (lane == 0) {
                    sd.skipped[q] = (int64_t)(d - (uint64_t)it) + (kStarFocusDraws - 1);
                    tasks[q].pnode = -1;
                    sd.pn[q] = -1;
                    mq.it[q] = it + 1;
                }
                continue;
            }
            d += (uint64_t)hit;
            if (lane == 0 && hit > 0) sd.skipped[q] = (int64_t)(d - (uint64_t)it);
        }
        double x = gen_range(seed, 2 * d, minx, maxx);      // rrt.rs:139-146 (Q7)
        double y = gen_range(seed, 2 * d + 1, miny, maxy);
        const int n = mq.n[q];
        double bd = __builtin_inf();
        int bi = 0x7fffffff;
#pragma unroll 4
        for (int i = lane; i < n; i += 64) {  // rrt.rs:378-391 (Q9: exact, lowest index on ties)
            const double dx = x - X[i], dy = y - Y[i];
            const double d2 = dx * dx + dy * dy;
            if (d2 < bd) {
                bd = d2;
                bi = i;
            }
        }
        wave_argmin(bd, bi);
        const double nx = X[bi], ny = Y[bi];
        if (sd.eta > 0.0 && bd > sd.eta * sd.eta) {  // Steer(x_nearest, x_rand)
            const double f = sd.eta / sqrt(bd);
            x = nx + (x - nx) * f;
            y = ny + (y - ny) * f;
        }
        if (lane == 0) {
            SteerTask tk{};
            tk.x = x;
            tk.y = y;
            tk.px = nx;
            tk.py = ny;
            tk.pyaw = mq.yaw[row + bi];
            tk.pnode = bi;
            tasks[q] = tk;
            sd.px[q] = x;
            sd.py[q] = y;
            sd.pn[q] = bi;
        }
    }
}

__global__ __launch_bounds__(256) void star_knn_kernel(StarDev sd, const int* __restrict__ statusA,
                                                       const double* __restrict__ costA,
                                                       SteerTask* __restrict__ tasksB,
                                                       StarTaskExt* __restrict__ extB,
                                                       int* __restrict__ err) {
    __shared__ double s_d2[kKnnWaves][kKnnCache];
    __shared__ double s_cd[kKnnWaves][64];
    __shared__ int s_ci[kKnnWaves][64];
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    double* cand_d = s_cd[wave];
    int* cand_i = s_ci[wave];
    const MqDev& mq = sd.mq;
    double* cache = s_d2[wave];
    __shared__ int s_cnt[kKnnWaves], s_base;
    // wave w of workgroup b serves queries b * kKnnWaves + w (+ the grid's stride): every wave of
    // a workgroup runs the same iterations, so the round-B task reservation is one atomic per
    // workgroup instead of one per query (one counter address for the whole launch)
    for (int qb = (int)blockIdx.x * kKnnWaves; qb < mq.Q; qb += (int)gridDim.x * kKnnWaves) {
        const int q = qb + wave;
        const int p = q < mq.Q ? sd.pn[q] : -1;
        bool live = p >= 0;
        int n = 0, st = kReject;
        if (live) {
            n = mq.n[q];
            st = statusA[q];
            // the gate: the edge new → nearest (a literal-path verdict is settled by star_insert)
            const bool gate = (st == kLiteral || star_feasible(st, costA[q])) &&
                              !(mq.blocked && mq.blocked[q]);
            if (!gate) {
                if (lane == 0) {
                    if (st == kError) atomicOr(err, 1);  // n_point overflow: the reference panics
                    sd.nnear[q] = -1;
                    mq.it[q] += 1;
                    mq.evals[q] += n;
                }
                live = false;
            }
        }
        double x = 0.0, y = 0.0, c0 = 0.0;
        size_t row = 0;
        int k = 0, mine = -1;
        bool want = false;
        uint64_t bm = 0;
        const double* __restrict__ X = mq.x;
        const double* __restrict__ Y = mq.y;
        if (live) {
            x = sd.px[q];
            y = sd.py[q];
            row = (size_t)q * mq.cap;
            X = mq.x + row;
            Y = mq.y + row;
            k = sd.ksched[n];
            const bool cached = n <= kKnnCache;
            bool done = false;
            if (cached) {
                double lmin = __builtin_inf();
#pragma unroll 8
                for (int i = lane; i < n; i += 64) {
                    const double dx = x - X[i], dy = y - Y[i];
                    const double d2 = dx * dx + dy * dy;
                    cache[i] = d2;
                    lmin = fmin(lmin, d2);
                }
                // T = the k-th smallest lane minimum: k distinct nodes lie within it, so the k
                // nearest are among the nodes with d2 <= T (usually k..2k of them)
                const double T = readlane_f64(bitonic64(lmin, lane).d, k - 1);
                int c = 0;
                for (int i = lane; i < n; i += 64) c += cache[i] <= T;
                int off = wave_incl_scan(c);  // inclusive prefix over the lanes
                const int C = __builtin_amdgcn_readlane(off, 63);
                if (C <= 64) {  // gather them into one (d2, index) pair per lane and sort the wave
                    off -= c;
                    for (int i = lane; i < n; i += 64)
                        if (cache[i] <= T) {
                            cand_d[off] = cache[i];
                            cand_i[off] = i;
                            ++off;
                        }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    Kv kv{__builtin_inf(), 0x7fffffff};
                    if (lane < C) kv = Kv{cand_d[lane], cand_i[lane]};
                    kv = bitonic64(kv.d, lane, kv.i);
                    mine = lane < k ? kv.i : -1;
                    done = true;
                    __builtin_amdgcn_wave_barrier();  // the list is reused by the next query
                }
            }
            if (!done) {
                // k rounds of the lexicographic (d2, index) successor of the previous winner
                double pd = -1.0;
                int pi = -1;
                for (int r = 0; r < k; ++r) {
                    double bd = __builtin_inf();
                    int bi = 0x7fffffff;
                    for (int i = lane; i < n; i += 64) {
                        double d2;
                        if (cached) {
                            d2 = cache[i];
                        } else {
                            const double dx = x - X[i], dy = y - Y[i];
                            d2 = dx * dx + dy * dy;
                        }
                        if ((d2 > pd || (d2 == pd && i > pi)) && d2 < bd) {
                            bd = d2;
                            bi = i;
                        }
                    }
                    wave_argmin(bd, bi);
                    pd = bd;
                    pi = bi;
                    if (lane == r) mine = bi;
                }
            }
            const bool has = lane < k;
            if (has) sd.near[(size_t)q * kStarKMax + lane] = mine;
            // candidates that could still beat the nearest's cost c0 (chord lower bound): the
            // others can never be the first strict minimum, so they are not steered
            c0 = sd.cost[row + p] + costA[q];
            want = has && mine != p;
            if (want) {
                const double dx = x - X[mine], dy = y - Y[mine];
                want = sd.cost[row + mine] + star_chord_lb(dx * dx + dy * dy, sd.curv) < c0;
            }
            bm = __ballot(want);
        }
        const int cnt = __popcll(bm);
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int w = 0; w < kKnnWaves; ++w) tot += s_cnt[w];
            s_base = tot > 0 ? atomicAdd(&sd.stB->W, tot) : 0;
        }
        __syncthreads();
        if (live) {
            int slot = s_base;
            for (int w = 0; w < wave; ++w) slot += s_cnt[w];
            slot = cnt > 0 ? slot : 0;
            if (lane == 0) {
                sd.nnear[q] = k;
                sd.bmask[q] = bm;
                sd.bslot[q] = slot;
            }
            if (want) {  // X_near order
                const int idx = __popcll(bm & ((1ull << lane) - 1ull));
                SteerTask tk{};
                tk.x = x;
                tk.y = y;
                tk.px = X[mine];
                tk.py = Y[mine];
                tk.pyaw = mq.yaw[row + mine];
                tk.pnode = mine;
                tasksB[slot + idx] = tk;
                StarTaskExt ex{};
                ex.cull = 1;  // only a candidate strictly cheaper than the nearest's can win
                ex.cbase = sd.cost[row + mine];
                ex.climit = c0;
                extB[slot + idx] = ex;
            }
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

// settle literal-path verdicts of a wave's lanes (the measure-zero trim cases), one at a time
__device__ __forceinline__ int star_settle(const SceneDev& sc, int st, bool act, double x, double y,
                                           double yaw, double px, double py, double pyaw,
                                           double* lit_scratch, int* locks, int hint) {
    const int lane = __lane_id();
    uint64_t lit = __ballot(act && st == kLiteral);
    if (!lit) return st;
    const int slot = lit_acquire(locks, hint);
    double* bx = lit_scratch + (size_t)slot * 3 * kLiteralCap;
    for (; lit; lit &= lit - 1) {
        const int l = __builtin_ctzll(lit);
        const int r = steer_collide_literal(sc, __shfl(x, l), __shfl(y, l), __shfl(yaw, l),
                                            __shfl(px, l), __shfl(py, l), __shfl(pyaw, l), bx,
                                            bx + kLiteralCap, bx + 2 * kLiteralCap);
        if (lane == l) st = r;
    }
    lit_release(locks, slot);
    return st;
}

__global__ __launch_bounds__(256) void star_insert_kernel(
    StarDev sd, SceneDev sc, const int* __restrict__ statusA, const double* __restrict__ yawA,
    const double* __restrict__ costA, const SteerTask* __restrict__ tasksB,
    const int* __restrict__ statusB, const double* __restrict__ yawB,
    const double* __restrict__ costB, SteerTask* __restrict__ tasksC,
    StarTaskExt* __restrict__ extC, double* __restrict__ lit_scratch, int* __restrict__ err) {
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const MqDev& mq = sd.mq;
    const int wave = threadIdx.x >> 6;
    __shared__ int s_cnt[4], s_base;
    // every wave of a workgroup runs the same iterations (queries b * 4 + w, + the grid's
    // stride), so the round-C task reservation is one atomic per workgroup
    for (int qb = (int)blockIdx.x * 4; qb < mq.Q; qb += (int)gridDim.x * 4) {
        const int q = qb + wave;
        bool live = q < mq.Q && sd.pn[q] >= 0;
        const int k = live ? sd.nnear[q] : -1;
        live = live && k >= 0;  // (k < 0: no insert this step, settled by star_knn)
        const int p = live ? sd.pn[q] : 0;
        const int n = live ? mq.n[q] : 0;
        const size_t row = (size_t)(live ? q : 0) * mq.cap;
        double x = 0.0, y = 0.0, cb = 0.0, yb = 0.0;
        int mine = -1;
        uint64_t wm = 0;
        bool want = false;
        if (live) {
            x = sd.px[q];
            y = sd.py[q];
            mine = lane < k ? sd.near[(size_t)q * kStarKMax + lane] : -1;
            // the nearest, then the X_near nodes star_knn steered (the pruned ones cannot win)
            const int ncand = 1 + __popcll(sd.bmask[q]);
            const bool act = lane < ncand;
            int node = p, st = kReject;
            double yaw = 0.0, e = __builtin_inf();
            if (lane == 0) {
                st = statusA[q];
                yaw = yawA[q];
                e = costA[q];
            } else if (act) {
                const int t = sd.bslot[q] + lane - 1;
                node = tasksB[t].pnode;
                st = statusB[t];
                yaw = yawB[t];
                e = costB[t];
            }
            const double nx = mq.x[row + node], ny = mq.y[row + node], nyaw = mq.yaw[row + node];
            st = star_settle(sc, st, act, x, y, yaw, nx, ny, nyaw, lit_scratch, sd.lit_locks, gw);
            if (__ballot(act && st == kError)) {
                if (lane == 0) atomicOr(err, 1);
                live = false;
            } else {
                const bool feas = act && star_feasible(st, e);
                if (!__shfl((int)feas, 0)) {  // the gate failed on the literal path
                    if (lane == 0) {
                        sd.nnear[q] = -1;
                        mq.it[q] += 1;
                        mq.evals[q] += n;
                    }
                    live = false;
                } else {
                    // choose parent: the first strict minimum of cost(node) + edge cost in
                    // candidate order
                    double c = feas ? sd.cost[row + node] + e : __builtin_inf();
                    int bl = lane;
                    wave_argmin(c, bl);
                    const int best = __shfl(node, bl);
                    yb = __shfl(yaw, bl);
                    const double eb = __shfl(e, bl);
                    cb = c;
                    if (lane == 0) {
                        const size_t o = row + n;
                        mq.x[o] = x;
                        mq.y[o] = y;
                        mq.yaw[o] = yb;
                        mq.parent[o] = best;
                        sd.cost[o] = cb;
                        sd.elen[o] = eb;
                        mq.n[q] = n + 1;
                        mq.it[q] += 1;
                        mq.evals[q] += n;
                        sd.cb[q] = cb;
                    }
                    // rewire tasks: X_near nodes other than the parent that could still get
                    // cheaper (cost(new) + e >= cost(new) >= cost(m) otherwise; costs only
                    // decrease)
                    want = lane < k && mine != best;
                    if (want) {  // chord lower bound of the rewire edge (prunes only what cannot rewire)
                        const double dx = x - mq.x[row + mine], dy = y - mq.y[row + mine];
                        want = cb + star_chord_lb(dx * dx + dy * dy, sd.curv) < sd.cost[row + mine];
                    }
                    wm = __ballot(want);
                }
            }
        }
        const int cnt = __popcll(wm);
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = tot > 0 ? atomicAdd(&sd.stC->W, tot) : 0;
        }
        __syncthreads();
        if (live) {
            int slot = s_base;
            for (int w = 0; w < wave; ++w) slot += s_cnt[w];
            slot = cnt > 0 ? slot : -1;
            if (lane == 0) {
                sd.cslot[q] = slot;
                sd.cmask[q] = wm;
            }
            if (want) {
                SteerTask tk{};
                tk.x = mq.x[row + mine];
                tk.y = mq.y[row + mine];
                tk.px = x;
                tk.py = y;
                tk.pyaw = yb;
                tk.pnode = n;  // the new node (the edge's parent)
                const int tc = slot + __popcll(wm & ((1ull << lane) - 1ull));
                tasksC[tc] = tk;
                StarTaskExt ex{};
                ex.cyaw = mq.yaw[row + mine];
                ex.own_yaw = 1;
                ex.node = mine;
                ex.cull = 1;  // only a strictly cheaper path through the new node matters
                ex.cbase = cb;
                ex.climit = sd.cost[row + mine];
                extC[tc] = ex;
            }
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

__global__ __launch_bounds__(256) void star_rewire_kernel(
    StarDev sd, SceneDev sc, const SteerTask* __restrict__ tasksC,
    const StarTaskExt* __restrict__ extC, const int* __restrict__ statusC,
    const double* __restrict__ costC, double* __restrict__ lit_scratch, int* __restrict__ err) {
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    const MqDev& mq = sd.mq;
    for (int q = gw; q < mq.Q; q += nw) {
        if (sd.pn[q] < 0 || sd.nnear[q] < 0) continue;
        const int slot = sd.cslot[q];
        if (slot < 0) continue;
        const int cnt = __popcll(sd.cmask[q]);
        const bool act = lane < cnt;
        SteerTask tk{};
        StarTaskExt ex{};
        int st = kReject;
        double e = __builtin_inf();
        if (act) {
            tk = tasksC[slot + lane];
            ex = extC[slot + lane];
            st = statusC[slot + lane];
            e = costC[slot + lane];
        }
        st = star_settle(sc, st, act, tk.x, tk.y, ex.cyaw, tk.px, tk.py, tk.pyaw, lit_scratch,
                         sd.lit_locks, gw);
        if (__ballot(act && st == kError)) {
            if (lane == 0) atomicOr(err, 1);
            continue;
        }
        const uint64_t fm = __ballot(act && star_feasible(st, e));
        const size_t row = (size_t)q * mq.cap;
        const int n = mq.n[q];
        const int nwn = n - 1;  // the node star_insert appended
        const double cb = sd.cb[q];
        double* __restrict__ cost = sd.cost + row;
        double* __restrict__ elen = sd.elen + row;
        int* __restrict__ par = mq.parent + row;
        int* __restrict__ mark = sd.mark + row;
        int s = sd.stamp[q];
        int64_t rw = 0;
        for (uint64_t f = fm; f; f &= f - 1) {  // X_near order
            const int i = __builtin_ctzll(f);
            const int m = __shfl(ex.node, i);
            const double em = __shfl(e, i);
            const double cn = cb + em;
            if (!(cn < cost[m])) continue;
            if (lane == 0) {
                par[m] = nwn;
                elen[m] = em;
                cost[m] = cn;
                mark[m] = s;
            }
            ++rw;
            // this wave alone reads and writes query q's rows in this kernel, so its lanes
            // exchange them through the CU's own cache: a workgroup-scope fence (the stores
            // complete) orders them, with no L2 writeback or L1 invalidation per pass
            __threadfence_block();
            // the subtree of m, level by level: a node's parent is final one pass earlier
            // (lane l holds nodes l, l + 64, ...; a pass loads kRwReg rows of parents per lane,
            // then issues all of their mark gathers at once, instead of one dependent pair per
            // 64 nodes)
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
                            cost[j] = cost[pr[r]] + elen[j];
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
        if (lane == 0) {
            sd.stamp[q] = s;
            sd.rewires[q] += rw;
        }
    }
}

hipError_t launch_star_steps(hipStream_t s, const StarArgs& a, int steps) {
    const int Q = a.sd.mq.Q;
    const int TB = Q * kStarKMax;  // task capacity of rounds B and C
    const int qb = std::min((Q + 3) / 4, 4096);
    const int knn_blocks = std::min((Q + kKnnWaves - 1) / kKnnWaves, 4096);
    const int lit_blocks = std::min((Q + 3) / 4, 4096);  // literal scratch: slot locks
    const int prepA = std::min((Q + kPrepThreads / 8 - 1) / (kPrepThreads / 8), 2048);
    const int prepB = std::min((TB + kPrepThreads / 8 - 1) / (kPrepThreads / 8), 2048);
    const int walkA = walk_blocks(Q, walk_grid_limit(kWalkStar, a.sc));
    const int lds = a.sc.lds_bytes;
    // a scene read from global memory (no LDS image) makes the walk latency-bound: fill every
    // wave slot the walk's 48 VGPRs allow (4 workgroups of 8 waves per CU)
    const int walkB = walk_blocks(TB, lds > 0 ? walk_grid_limit(kWalkStar, a.sc) : 1024);
    // ev (profiling): 8 per step — around star_sample, then around each round's walk
    auto round = [&](DevState* st, int pb, int wb, const SteerTask* t, const StarTaskExt* ext,
                     int* status, double* yaw, double* cost, hipEvent_t* ev) {
        launch_prep_tasks(s, pb, st, a.sc, a.rec, yaw, t, cost, ext);
        if (ev) (void)hipEventRecord(ev[0], s);
        // (the analytic straight segments, s_classify: config 5 21.9 -> 25.1 M it/s, same digest)
        launch_walk(kWalkStar, s, wb, st, a.sc, a.rec, nullptr, status, nullptr, nullptr,
                    a.wg_points);
        if (ev) (void)hipEventRecord(ev[1], s);
    };
    for (int k = 0; k < steps; ++k) {
        hipEvent_t* ev = a.ev ? a.ev + 8 * k : nullptr;
        if (ev) (void)hipEventRecord(ev[0], s);
        star_sample_kernel<<<qb, 256, 0, s>>>(a.sd, a.sc.minx, a.sc.maxx, a.sc.miny, a.sc.maxy,
                                              a.tA);
        if (ev) (void)hipEventRecord(ev[1], s);
        round(a.sd.stA, prepA, walkA, a.tA, nullptr, a.sA, a.yA, a.cA, ev ? ev + 2 : nullptr);
        star_knn_kernel<<<knn_blocks, 64 * kKnnWaves, 0, s>>>(a.sd, a.sA, a.cA, a.tB, a.eB,
                                                              a.err);
        round(a.sd.stB, prepB, walkB, a.tB, a.eB, a.sB, a.yB, a.cB, ev ? ev + 4 : nullptr);
        star_insert_kernel<<<lit_blocks, 256, 0, s>>>(a.sd, a.sc, a.sA, a.yA, a.cA, a.tB, a.sB,
                                                      a.yB, a.cB, a.tC, a.eC, a.lit_scratch,
                                                      a.err);
        round(a.sd.stC, prepB, walkB, a.tC, a.eC, a.sC, a.yC, a.cC, ev ? ev + 6 : nullptr);
        star_rewire_kernel<<<lit_blocks, 256, 0, s>>>(a.sd, a.sc, a.tC, a.eC, a.sC, a.cC,
                                                      a.lit_scratch, a.err);
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void star_init_kernel(StarDev sd) {
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= sd.mq.Q) return;
    const size_t o = (size_t)q * sd.mq.cap;
    sd.cost[o] = 0.0;
    sd.elen[o] = 0.0;
    sd.stamp[q] = 1;
    sd.rewires[q] = 0;
}

hipError_t launch_star_init(hipStream_t s, const StarArgs& a, const double* starts) {
    hipError_t e = launch_mq_init(s, a.sd.mq, starts);
    if (e != hipSuccess) return e;
    star_init_kernel<<<(a.sd.mq.Q + 255) / 256, 256, 0, s>>>(a.sd);
    return hipGetLastError();
}

// ------------------------------------------------ RRT* goal connection (pp_star_plan, §3.7)
//
// The cheapest feasible goal edge of every query (oracle restatement: tests/star_goal_ref.py).
// The goal is the child and keeps its yaw, node m is the parent, total(m) = cost(m) + the edge's
// Dubins cost.  Round r serves node slice [63 r, 63 r + 63) of every query in [q0, q1):
//   star_goal_emit    one wave per query: one task per node of the slice whose chord lower bound
//                     stays under the query's running best, written compactly into round B's
//                     task arrays (stB->W counts them)
//   steer_prep / steer_walk   the extend's round, cull limit = the running best
//   star_goal_reduce  one wave per query: the slice's first strict minimum, which replaces the
//                     running best only when strictly smaller — so the result is the first
//                     strict minimum in node order, and a pruned or culled node (total >= the
//                     running best) could never have replaced it
// The trees and the extend's own state are only read; round B's arrays, the records and stB->W
// are rewritten by every extend step before it reads them (star_sample zeroes stB->W).
__global__ __launch_bounds__(256) void star_goal_init_kernel(StarGoalArgs g) {
    const int q = g.q0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q == g.q0) {
        g.a.sd.stB->W = 0;
        *g.steered = 0;
    }
    if (q >= g.q1) return;
    g.best[q] = __builtin_inf();
    g.best_node[q] = -1;
}

__global__ __launch_bounds__(256) void star_goal_emit_kernel(StarGoalArgs g, int round) {
    const StarDev& sd = g.a.sd;
    const MqDev& mq = sd.mq;
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    __shared__ int s_cnt[4], s_base;
    // every wave of a workgroup runs the same iterations (queries q0 + b * 4 + w, + the grid's
    // stride), so the task reservation is one atomic per workgroup (as star_knn / star_insert)
    for (int qb = g.q0 + (int)blockIdx.x * 4; qb < g.q1; qb += (int)gridDim.x * 4) {
        const int q = qb + wave;
        const bool live = q < g.q1;
        const size_t row = (size_t)(live ? q : 0) * mq.cap;
        const int n = live ? mq.n[q] : 0;
        const int m = 63 * round + lane;  // (lane 63 idles: kStarKMax task slots per query)
        const bool has = lane < kStarKMax && m < n;
        // polygon mode: a blocked root's tree is the root alone and no line through it verifies
        bool want = has && !(mq.blocked && mq.blocked[q]);
        double gx = 0.0, gy = 0.0, gyaw = 0.0, best = 0.0, cm = 0.0;
        if (live) {
            gx = g.goals[3 * (size_t)q];
            gy = g.goals[3 * (size_t)q + 1];
            gyaw = g.goals[3 * (size_t)q + 2];
            best = g.best[q];
        }
        if (has && g.total) g.total[m] = __builtin_inf();
        if (want) {
            cm = sd.cost[row + m];
            if (g.prune) {  // the chord lower bound already reaches the running best
                const double dx = gx - mq.x[row + m], dy = gy - mq.y[row + m];
                want = cm + star_chord_lb(dx * dx + dy * dy, sd.curv) < best;
            }
        }
        const uint64_t bm = __ballot(want);
        const int cnt = __popcll(bm);
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = tot > 0 ? atomicAdd(&sd.stB->W, tot) : 0;
        }
        __syncthreads();
        if (live) {
            int slot = s_base;
            for (int w = 0; w < wave; ++w) slot += s_cnt[w];
            if (lane == 0) {
                g.gslot[q] = cnt > 0 ? slot : 0;
                g.gmask[q] = bm;
            }
            if (want) {  // node order
                const int t = slot + __popcll(bm & ((1ull << lane) - 1ull));
                SteerTask tk{};
                tk.x = gx;
                tk.y = gy;
                tk.px = mq.x[row + m];
                tk.py = mq.y[row + m];
                tk.pyaw = mq.yaw[row + m];
                tk.pnode = m;
                g.a.tB[t] = tk;
                StarTaskExt ex{};
                ex.cyaw = gyaw;
                ex.own_yaw = 1;
                ex.node = m;
                ex.cull = g.prune;  // only a total strictly under the running best matters
                ex.cbase = cm;
                ex.climit = best;
                g.a.eB[t] = ex;
            }
        }
        __syncthreads();  // s_cnt / s_base are rewritten by the next iteration
    }
}

__global__ __launch_bounds__(256) void star_goal_reduce_kernel(StarGoalArgs g, SceneDev sc) {
    const StarDev& sd = g.a.sd;
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the round's walk is done: the next round's count
        *g.steered += sd.stB->W;
        sd.stB->W = 0;
    }
    for (int q = g.q0 + gw; q < g.q1; q += nw) {
        const uint64_t bm = g.gmask[q];
        if (!bm) continue;
        const bool act = lane < __popcll(bm);
        SteerTask tk{};
        StarTaskExt ex{};
        int st = kReject;
        double e = __builtin_inf();
        if (act) {
            const int t = g.gslot[q] + lane;
            tk = g.a.tB[t];
            ex = g.a.eB[t];
            st = g.a.sB[t];
            e = g.a.cB[t];
        }
        st = star_settle(sc, st, act, tk.x, tk.y, ex.cyaw, tk.px, tk.py, tk.pyaw, g.a.lit_scratch,
                         sd.lit_locks, gw);
        if (__ballot(act && st == kError)) {  // n_point overflow: the reference panics
            if (lane == 0) atomicOr(g.a.err, 1);
            continue;
        }
        double c = act && star_feasible(st, e) ? ex.cbase + e : __builtin_inf();
        if (act && g.total) g.total[ex.node] = c;
        int bl = lane;
        wave_argmin(c, bl);  // the lowest lane (node) on ties
        const int node = __shfl(ex.node, bl);
        if (lane == 0 && c < g.best[q]) {
            g.best[q] = c;
            g.best_node[q] = node;
        }
    }
}

hipError_t launch_star_goal(hipStream_t s, const StarGoalArgs& g, int rounds) {
    const StarArgs& a = g.a;
    const int Q = g.q1 - g.q0;
    const int TB = Q * kStarKMax;  // a round's task capacity: 63 per query
    const int qb = std::min((Q + 3) / 4, 4096);
    const int prep = std::min((TB + kPrepThreads / 8 - 1) / (kPrepThreads / 8), 2048);
    // (the walk grid of launch_star_steps' rounds B and C)
    const int walk =
        walk_blocks(TB, a.sc.lds_bytes > 0 ? walk_grid_limit(kWalkStar, a.sc) : 1024);
    star_goal_init_kernel<<<(Q + 255) / 256, 256, 0, s>>>(g);
    for (int r = 0; r < rounds; ++r) {
        star_goal_emit_kernel<<<qb, 256, 0, s>>>(g, r);
        launch_prep_tasks(s, prep, a.sd.stB, a.sc, a.rec, a.yB, a.tB, a.cB, a.eB);
        launch_walk(kWalkStar, s, walk, a.sd.stB, a.sc, a.rec, nullptr, a.sB, nullptr, nullptr,
                    a.wg_points);
        star_goal_reduce_kernel<<<qb, 256, 0, s>>>(g, a.sc);
    }
    return hipGetLastError();
}

}  // namespace ppamd

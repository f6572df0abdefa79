// pp_k_batch.hip — hand-written CDNA4 (gfx950) kernels of the query batch (config 3): the
// lockstep step's mq_sample_nn and mq_insert around the steer round, mq_target and mq_init.
// steer_prep and steer_walk are compiled by pp_k_steer.hip alone and launched through
// pp_steer_launch.h; the device code the units inline is pp_steer_dev.h.
//
// No MFMA anywhere: there is no dense contraction on this path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pp_kernels.h"

// mq_insert_kernel's literal path is this unit's only caller of select_word, and the inliner
// folds the last use of a local function in (the kernel grows by about 2,450 lines, DESIGN.md
// Appendix A.1), so this unit's own declaration pins it out of line, as the single file compiled
// it.  It has to precede the definition in pp_device.h (after it the compiler ignores the
// attribute, with a warning).
namespace ppamd {
struct Steer;
__device__ __noinline__ Steer select_word(double lex, double ley, double leyaw, double c);
}  // namespace ppamd

#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

// ------------------------------------------------- multi-query batch (config 3)
//
// One lockstep step advances every query by one plan_one extend iteration (rrt.rs:583-589):
//   mq_sample_nn   one wave per query: rand_point (the query's own seeded stream) and the exact
//                  f64 brute-force nearest node of its tree (lanes stride the SoA rows, lowest
//                  index on ties) — each step streams every tree once: the HBM-read-bound NN of
//                  SURVEY §8d
//   steer_prep / steer_walk   the window pipeline's kernels on the Q explicit tasks
//   mq_insert      the verdict (literal path for the measure-zero trim cases), append, it += 1
// Queries are independent, so there is no speculation and no resolve.
// One query's window of the lockstep step (one wave, all 64 lanes): lane l serves window slot
// k = l % K over node group g = l / K (nodes i = g mod 64/K), so every node row is loaded once per
// wave, not once per slot.  Space::rand_point of iteration it[q] + k on stream q (rrt.rs:139-146,
// Q7), the obstacle pre-test, the exact nearest node of tree q as the step found it (rrt.rs:378-391,
// Q9: lanes stride the rows, lowest index on ties), the verdict cache; the task into
// tasks[q K + k].
__device__ __forceinline__ bool mq_nn_query(const MqDev& mq, double minx, double maxx, double miny,
                                            double maxy, SteerTask* __restrict__ tasks,
                                            const SceneDev* __restrict__ scp, int q, int lane,
                                            SteerTask& tko) {
    const int K = mq.K, G = 64 / K;
    const int k = lane & (K - 1), g = lane / K;
    const int64_t it = mq.it[q] + k;
    const bool live = it < mq.target[q];
    const uint64_t seed = mq.seed[q];
    // the verdict cache: the task region still holds the previous step's window, which
    // started Tp iterations before this one, so iteration it sat in old slot k + Tp; its
    // parent, verdict and yaw are read before any lane overwrites the region.  Lane k reads slot
    // k + Tp, which lane k + Tp of the SAME wave rewrites below (tasks, status, tyaw of slot t):
    // that is ordered only because all K slots of a query are served by one wave (K <= 64, one
    // query per K lanes) and every load is issued before the first store: the wave barrier
    // keeps the compiler from sinking a load past the stores, and one wave's vector memory
    // requests to an address are served in issue order.  Serving a query's slots from more than
    // one wave would need a grid-wide ordering instead.
    int opn = -1, ost = -1;
    double oyw = 0.0;
    if (mq.it_prev && g == 0) {
        const int64_t Tp = mq.it[q] - mq.it_prev[q];
        if (Tp >= 0 && Tp < K && k + Tp < K) {
            const int to = q * K + k + (int)Tp;
            opn = tasks[to].pnode;
            ost = mq.status[to];
            if (mq.tyaw) oyw = mq.tyaw[to];
        }
    }
    __builtin_amdgcn_wave_barrier();
    double x = 0.0, y = 0.0;
    if (live) {
        x = gen_range(seed, 2 * (uint64_t)it, minx, maxx);
        y = gen_range(seed, 2 * (uint64_t)it + 1, miny, maxy);
    }
    // the pre-test first (its loads overlap the scan; its result is used after it)
    const bool blocked = live && scp && point_blocked<false, kSceneAny>(*scp, x, y);
    const int n = mq.n[q];
    const size_t row = (size_t)q * mq.cap;
    const double* __restrict__ X = mq.x + row;
    const double* __restrict__ Y = mq.y + row;
    double bd = __builtin_inf();
    int bi = 0x7fffffff;
#pragma unroll 4
    for (int i = g; i < n; i += G) {
        const double dx = x - X[i], dy = y - Y[i];
        const double d2 = dx * dx + dy * dy;
        if (d2 < bd) {
            bd = d2;
            bi = i;
        }
    }
    for (int m = K; m < 64; m <<= 1) {  // the G lanes of slot k
        if (m == 16)
            argmin_swap<false>(bd, bi);
        else if (m == 32)
            argmin_swap<true>(bd, bi);
        else
            argmin_pair(bd, bi, __shfl_xor(bd, m), __shfl_xor(bi, m));
    }
    bool need = false;  // the slot needs steer_prep + steer_walk
    const int t = q * K + k;
    if (g == 0) {
        if (!live) {
            tasks[t].pnode = -1;
        } else if (blocked) {
            // the sample lies in an obstacle: rejected whatever its parent (pnode -2: no steer,
            // and the insert never cuts the window there)
            tasks[t].x = x;
            tasks[t].y = y;
            tasks[t].pnode = -2;
            if (mq.alist) mq.status[t] = kReject;
        } else {
            // the same child (the counter RNG redraws it) and the same parent pose (rows are
            // never rewritten) as a task the previous step walked: its verdict (kReject 0 /
            // kAccept 1, as 2 + verdict) — settled here with the old slot's yaw (the same
            // compute_yaw of the same poses) when the batch lists its active tasks, else
            // steer_prep writes it as decided
            const int cached = (opn == bi && (ost == kAccept || ost == kReject)) ? 2 + ost : 0;
            tko = SteerTask{x, y, X[bi], Y[bi], mq.yaw[row + bi], bi, cached};
            tasks[t] = tko;
            mq.nnd2[t] = bd;
            if (mq.alist && cached) {
                mq.status[t] = cached - 2;
                mq.tyaw[t] = oyw;
            } else {
                need = true;
            }
        }
    }
    if (mq.it_prev && lane == 0) mq.it_prev[q] = mq.it[q];
    return need;
}

// The listed tasks take one reservation per workgroup (its waves' counts summed in LDS): one
// atomic per query on the batch's one counter serialised the 8192-query step (642 -> 612 M
// it/s).  NT: 1024 threads (16 queries) for large sub-batches, 256 for small ones, whose
// workgroups would otherwise crowd onto a few CUs (a 512-query sub-batch: 32 workgroups).
template <int NT>
__global__ __launch_bounds__(NT) void mq_sample_nn_kernel(MqDev mq, double minx,
                                                                    double maxx, double miny,
                                                                    double maxy,
                                                                    SteerTask* __restrict__ tasks,
                                                                    const SceneDev* __restrict__ scp) {
    constexpr int kMqNnWaves = NT / 64;
    __shared__ int s_cnt[kMqNnWaves];
    __shared__ int s_base;
    const int lane = __lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // (every wave of the workgroup makes the same trips: the barriers below)
    for (int qb = (int)blockIdx.x * kMqNnWaves; qb < mq.Q; qb += (int)gridDim.x * kMqNnWaves) {
        const int q = qb + wave;
        SteerTask tk{};
        const bool need =
            q < mq.Q && mq_nn_query(mq, minx, maxx, miny, maxy, tasks, scp, q, lane, tk);
        if (mq.alist) {
            const uint64_t nm = __ballot(need);
            if (lane == 0) s_cnt[wave] = __popcll(nm);
            __syncthreads();
            if (threadIdx.x == 0) {
                int tot = 0;
                for (int w = 0; w < kMqNnWaves; ++w) {
                    const int c = s_cnt[w];
                    s_cnt[w] = tot;
                    tot += c;
                }
                s_base = tot ? atomicAdd(&mq.st->W, tot) : 0;
            }
            __syncthreads();
            if (need) {
                const int i = s_base + s_cnt[wave] + __popcll(nm & ((1ull << lane) - 1ull));
                mq.alist[i] = q * mq.K + lane;  // (need: lane = slot k, node group 0)
                mq.status[q * mq.K + lane] = -2 - i;  // (the walk's verdict: lstat[i])
                tk.literal = 0;
                mq.ctask[i] = tk;
            }
            __syncthreads();  // (s_cnt / s_base: the next trip)
        }
    }
}

// the iteration targets of one pp_batch_extend call: n_steps more iterations, at most max_iter
__global__ __launch_bounds__(256) void mq_target_kernel(MqDev mq, int64_t n_steps,
                                                        int64_t* __restrict__ target) {
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= mq.Q) return;
    const int64_t t = mq.it[q] + n_steps;
    target[q] = t < mq.max_iter ? t : mq.max_iter;
}

__global__ __launch_bounds__(256) void mq_insert_kernel(MqDev mq, SceneDev sc,
                                                        const SteerTask* __restrict__ tasks,
                                                        int* __restrict__ status,
                                                        const double* __restrict__ yaw,
                                                        double* __restrict__ lit_scratch,
                                                        int* __restrict__ lit_locks,
                                                        int* __restrict__ err) {
    // a wave serves 64 / K queries, K lanes each (lane = g * K + k: the window's iteration
    // it[q] + k of its g-th query; K a power of two <= kMqMaxK = 64, automatically 32, halved
    // while Q * K > 262144).  Literal-path re-runs first (rare, the wave's one scratch buffer), then each query's in-order replay: iteration k keeps its
    // speculative verdict unless an accepted window sample k' < k is strictly nearer than its
    // snapshot NN (snapshot nodes have lower indices and win ties) — the window stops there and
    // the next step resumes at it; the accepted samples before it are appended in order
    // (rrt.rs:586-589).
    const int lane = __lane_id();
    const int gw = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    // the step's steer kernels are done: the next step's mq_sample_nn lists afresh
    if (mq.alist && gw == 0 && lane == 0) mq.st->W = 0;
    const int K = mq.K, G = 64 / K;
    const int g = lane / K, k = lane - g * K, g0 = g * K;
    const uint64_t gmask = (K == 64 ? ~0ull : ((1ull << K) - 1ull)) << g0;
    for (int base = gw * G; base < mq.Q; base += nw * G) {
        const int q = base + g;
        const bool in = q < mq.Q;
        const int t = q * K + k;
        SteerTask tk{};
        int st = kReject;
        double yw = 0.0, d2nn = 0.0;
        if (in) {
            tk = tasks[t];
            st = status[t];
            yw = yaw[t];
            if (st <= -2) {  // a listed slot: the walk's verdict, kept for the next step's cache
                const int i = -2 - st, lg = mq.st->lgrid;
                st = mq.lstat[(i % lg) * mq.st->lper + i / lg];
                status[t] = st;
            }
        }
        const bool live = in && tk.pnode != -1;  // (pnode -2: a sample in an obstacle)
        const bool act = in && tk.pnode >= 0;
        if (act) d2nn = mq.nnd2[t];
        if (uint64_t lit = __ballot(act && st == kLiteral)) {
            const int slot = lit_acquire(lit_locks, gw);
            double* bx = lit_scratch + (size_t)slot * 3 * kLiteralCap;
            for (; lit; lit &= lit - 1) {
                const int l = __builtin_ctzll(lit);
                const double x = __shfl(tk.x, l), y = __shfl(tk.y, l), w = __shfl(yw, l);
                const double px = __shfl(tk.px, l), py = __shfl(tk.py, l);
                const double pw = __shfl(tk.pyaw, l);
                const int r = steer_collide_literal(sc, x, y, w, px, py, pw, bx, bx + kLiteralCap,
                                                    bx + 2 * kLiteralCap);
                if (lane == l) st = r;
            }
            lit_release(lit_locks, slot);
        }
        const bool blocked = in && mq.blocked && mq.blocked[q];
        const uint64_t accm = __ballot(act && st == kAccept && !blocked);
        bool cut = !live;
        for (int j = 0; j < K; ++j) {  // slot j of every query against its later slots
            const double xj = __shfl(tk.x, g0 + j), yj = __shfl(tk.y, g0 + j);
            if (((accm >> (g0 + j)) & 1ull) && k > j && act) {
                const double dx = tk.x - xj, dy = tk.y - yj;
                if (dx * dx + dy * dy < d2nn) cut = true;
            }
        }
        const uint64_t cutm = __ballot(in && cut) & gmask;
        const int T = cutm ? (int)__builtin_ctzll(cutm) - g0 : K;  // iterations consumed
        const uint64_t keep = accm & gmask & ((T >= 64 ? ~0ull : ((1ull << T) - 1ull)) << g0);
        const bool bad = __ballot(k < T && act && st == kError) & gmask;
        const int n = in ? mq.n[q] : 0;
        const int before = __popcll(keep & ((1ull << lane) - 1ull));
        if (!bad && k < T && ((keep >> lane) & 1ull)) {
            const size_t o = (size_t)q * mq.cap + n + before;
            mq.x[o] = tk.x;
            mq.y[o] = tk.y;
            mq.yaw[o] = yw;
            mq.parent[o] = tk.pnode;
        }
        // NN node-distance evaluations of the sequential spec: iteration k scans the tree as it
        // stands then (n + the window samples accepted before it)
        int64_t ev = (in && k < T) ? (int64_t)(n + before) : 0;
        for (int o = 1; o < K; o <<= 1) ev += __shfl_xor(ev, o);
        if (in && k == 0 && T > 0) {
            if (bad) {
                atomicOr(err, 1);
            } else {
                mq.n[q] = n + __popcll(keep);
                mq.it[q] += T;
                mq.evals[q] += ev;
            }
        }
    }
}

// roots of a new batch (RRT::new, rrt.rs:344-346): row 0 of every tree
__global__ __launch_bounds__(256) void mq_init_kernel(MqDev mq, const double* __restrict__ starts) {
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= mq.Q) return;
    const size_t o = (size_t)q * mq.cap;
    mq.x[o] = starts[3 * q];
    mq.y[o] = starts[3 * q + 1];
    mq.yaw[o] = starts[3 * q + 2];
    mq.parent[o] = -1;
    mq.n[q] = 1;
    mq.it[q] = 0;
    mq.evals[q] = 0;
}

hipError_t launch_mq_init(hipStream_t s, const MqDev& mq, const double* starts) {
    mq_init_kernel<<<(mq.Q + 255) / 256, 256, 0, s>>>(mq, starts);
    return hipGetLastError();
}

hipError_t launch_mq_target(hipStream_t s, const MqDev& mq, int64_t n_steps, int64_t* target) {
    mq_target_kernel<<<(mq.Q + 255) / 256, 256, 0, s>>>(mq, n_steps, target);
    return hipGetLastError();
}

// tasks per step (per sub-batch) from which the batch walk runs at 6 waves per SIMD: with its
// spill down to 20 B (round 5) the 1024-query shard's 16k-task sub-batch steps gain too
// (276.8 -> 283.0 M it/s, gpurun_out/r05occ; 3 workgroups per CU instead of 2: no gain)
constexpr int kBigStepTasks = 16384;

hipError_t launch_mq_steps(hipStream_t s, const MqArgs& a, int steps) {
    const int Q = a.mq.Q;
    const int T = Q * a.mq.K;  // tasks per step
    // one wave per query: 16 per workgroup from 2048 queries (a sub-batch of the full batch), 4 below
    const bool big_nn = Q >= 2048;
    const int nn_waves = big_nn ? 16 : 4;
    const int nn_blocks = std::min((Q + nn_waves - 1) / nn_waves, 4096);
    const int prep_blocks = std::min((T + kPrepThreads / 8 - 1) / (kPrepThreads / 8), 2048);
    // The walk classifies straight segments analytically (s_classify).  A step of
    // kBigStepTasks tasks or more walks at 6 waves per SIMD (80 VGPRs, 20 B of spill), a smaller
    // one at 5 (96 VGPRs, no spill); the 8192-query batch at 5 waves: 641 -> 623 M it/s (round 5,
    // one box).  The grid cap is the chosen instantiation's.
    const WalkProfile walk = T >= kBigStepTasks ? kWalkBatchBig : kWalkBatchSmall;
    const int wblocks = walk_blocks(T, walk_grid_limit(walk, a.sc));
    const int ins_blocks = std::min((Q + 4 * (64 / a.mq.K) - 1) / (4 * (64 / a.mq.K)), 4096);
    int* wstat = a.mq.alist ? a.mq.lstat : a.status;  // the walk's verdicts (list order)

    for (int k = 0; k < steps; ++k) {
        hipEvent_t* ev = a.ev ? a.ev + 5 * k : nullptr;
        if (ev) (void)hipEventRecord(ev[0], s);
        if (big_nn)
            mq_sample_nn_kernel<1024><<<nn_blocks, 1024, 0, s>>>(a.mq, a.sc.minx, a.sc.maxx,
                                                                a.sc.miny, a.sc.maxy, a.tasks, a.scp);
        else
            mq_sample_nn_kernel<256><<<nn_blocks, 256, 0, s>>>(a.mq, a.sc.minx, a.sc.maxx,
                                                              a.sc.miny, a.sc.maxy, a.tasks, a.scp);
        if (ev) (void)hipEventRecord(ev[1], s);
        // (the listed tasks, compacted by mq_sample_nn)
        launch_prep_tasks(s, prep_blocks, a.st, a.sc, a.rec, a.yaw,
                          a.mq.alist ? a.mq.ctask : a.tasks);
        if (ev) (void)hipEventRecord(ev[2], s);
        launch_walk(walk, s, wblocks, a.st, a.sc, a.rec, nullptr, wstat, nullptr, nullptr,
                    a.wg_points);
        if (ev) (void)hipEventRecord(ev[3], s);
        mq_insert_kernel<<<ins_blocks, 256, 0, s>>>(a.mq, a.sc, a.tasks, a.status, a.yaw,
                                                    a.lit_scratch, a.lit_locks, a.err);
        if (ev) (void)hipEventRecord(ev[4], s);
    }
    return hipGetLastError();
}

}  // namespace ppamd

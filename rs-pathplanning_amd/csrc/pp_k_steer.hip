// pp_k_steer.hip — the one owner of the steer round's kernels: steer_prep_kernel, every
// steer_walk_kernel instantiation and the walk's grid cache, behind the launch layer of
// pp_steer_launch.h that the other kernel units call.  Also the small API kernels and their
// launchers: steer_tasks (verify_node batch), verify_lines and the three dubins_* kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

#include "pp_kernels.h"
#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

// --------------------------------------------------------------------------------- dubins

__global__ __launch_bounds__(64) void dubins_batch_kernel(const double* __restrict__ conf, int n,
                                                          int cap, double* __restrict__ px,
                                                          double* __restrict__ py,
                                                          double* __restrict__ pyaw,
                                                          int* __restrict__ n_out,
                                                          int* __restrict__ word_out,
                                                          double* __restrict__ cost_out,
                                                          int* __restrict__ status_out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const double* c = conf + (size_t)i * 8;
    int np = 0, word = -1;
    double cost = 0.0;
    const int r = dubins_literal(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7],
                                 px + (size_t)i * cap, py + (size_t)i * cap,
                                 pyaw + (size_t)i * cap, cap, &np, &word, &cost);
    n_out[i] = np;
    word_out[i] = word;
    cost_out[i] = cost;
    status_out[i] = r;
}

// dubins_path_planning_from_origin (dubins.rs:326-399) for n configurations (dx, dy, eyaw, c,
// step_size): local points, yaw as generated
__global__ __launch_bounds__(64) void dubins_origin_kernel(const double* __restrict__ conf, int n,
                                                           int cap, double* __restrict__ px,
                                                           double* __restrict__ py,
                                                           double* __restrict__ pyaw,
                                                           int* __restrict__ n_out,
                                                           int* __restrict__ word_out,
                                                           double* __restrict__ cost_out,
                                                           int* __restrict__ status_out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const double* c = conf + (size_t)i * 5;
    int np = 0, word = -1;
    double cost = 0.0;
    const int r = dubins_local(c[0], c[1], c[2], c[3], c[4], px + (size_t)i * cap,
                               py + (size_t)i * cap, pyaw + (size_t)i * cap, cap, &np, &word,
                               &cost);
    n_out[i] = np;
    word_out[i] = word;
    cost_out[i] = cost;
    status_out[i] = r;
}

// the six words lsl, rsr, lsr, rsl, rlr, lrl (dubins.rs:27-153) of n (alpha, beta, d) triples:
// tpq[18 i + 3 w ..] = (t, p, q) of word w, ok[6 i + w] = 0 where the word is None
__global__ __launch_bounds__(64) void dubins_words_kernel(const double* __restrict__ abd, int n,
                                                          double* __restrict__ tpq,
                                                          int* __restrict__ ok) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const double alpha = abd[3 * i], beta = abd[3 * i + 1], d = abd[3 * i + 2];
    const Trig g = make_trig(alpha, beta);
    Word w[6];
    w[0] = word_lsl(alpha, beta, d, g);
    w[1] = word_rsr(alpha, beta, d, g);
    w[2] = word_lsr(alpha, beta, d, g);
    w[3] = word_rsl(alpha, beta, d, g);
    w[4] = word_rlr(alpha, beta, d, g);
    w[5] = word_lrl(alpha, beta, d, g);
    for (int k = 0; k < 6; ++k) {
        ok[6 * i + k] = w[k].ok ? 1 : 0;
        tpq[18 * i + 3 * k] = w[k].ok ? w[k].t : 0.0;
        tpq[18 * i + 3 * k + 1] = w[k].ok ? w[k].p : 0.0;
        tpq[18 * i + 3 * k + 2] = w[k].ok ? w[k].q : 0.0;
    }
}

// pp_sincos_small_batch: the walk's sincos_small on the walk's own table (read as the walk reads
// it, behind an opaque pointer) beside the math library's sincos, both compiled with this unit's
// flags; |x| < 2^30 (the host checked)
__global__ __launch_bounds__(256) void sincos_small_kernel(const double* __restrict__ x, int n,
                                                           double* __restrict__ s,
                                                           double* __restrict__ c,
                                                           double* __restrict__ s_ocml,
                                                           double* __restrict__ c_ocml) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const double* tab = kSinCosTab;
    asm volatile("" : "+s"(tab));
    const double v = x[i];
    double s0, c0, s1, c1;
    sincos_small(v, tab, &s0, &c0);
    sincos(v, &s1, &c1);
    s[i] = s0;
    c[i] = c0;
    s_ocml[i] = s1;
    c_ocml[i] = c1;
}

// Task t of a window: t < W is (sample t → its snapshot NN); t >= W is candidate entry t - W
// (sample E.j → window sample E.i, with E.i's yaw under ITS snapshot parent: the speculation the
// resolve validates).
__device__ inline void window_task(int t, int W, const double* wsx, const double* wsy,
                                   const double* snap_pose, const CandEntry* cand, int* j_out,
                                   double* px, double* py, double* pyaw) {
    if (t < W) {  // parent = the snapshot NN, whose pose nn_finalize wrote
        *j_out = t;
        *px = snap_pose[3 * t];
        *py = snap_pose[3 * t + 1];
        *pyaw = snap_pose[3 * t + 2];
    } else {  // parent = window sample i, heading toward ITS snapshot NN (compute_yaw)
        const CandEntry ce = cand[t - W];
        *j_out = ce.j;
        *px = wsx[ce.i];
        *py = wsy[ce.i];
        *pyaw = atan2(snap_pose[3 * ce.i + 1] - *py, snap_pose[3 * ce.i] - *px);
    }
}

// steer_prep: kPrepLanes lanes per task, 8 tasks per wave (persistent grid over the
// window's W + ncomp tasks): compute_yaw (rrt.rs:267-271),
// dubins_path_planning's frame change and word choice (dubins.rs:333-363, 401-408) and the
// segment origins.  Every transcendental sits at a call site all lanes reach with per-lane
// arguments (lane r evaluates word r; one sin and one cos call give all the segment trig), so a
// task's chain is ~9 calls deep instead of ~32.  The `pd += d` walk of generate_local_course
// (dubins.rs:200-272) is left to steer_walk (lane-parallel, exact).
__global__ __launch_bounds__(kPrepThreads) void steer_prep_kernel(
    const DevState* __restrict__ st, SceneDev sc, const double* __restrict__ wsx,
    const double* __restrict__ wsy, const double* __restrict__ snap_pose,
    CandEntry* __restrict__ cand, PrepRec* __restrict__ rec, double* __restrict__ snap_yaw, const SteerTask* __restrict__ tasks,
    double* __restrict__ cost_out = nullptr, const StarTaskExt* __restrict__ ext = nullptr) {
    // tasks != nullptr: explicit (child, parent pose) tasks [0, W) (multi-query batch); a task
    // with pnode < 0 is idle; own_yaw: the child keeps its heading cyaw (RRT* rewire edges)
    const int W = st->W;
    const int total = W + st->ncomp;
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const int r = lane & (kPrepLanes - 1), g0 = lane & ~(kPrepLanes - 1);
    constexpr int TPW = 64 / kPrepLanes;  // tasks per wave in phase A
    static_assert(kPrepLanes == 8, "the per-task broadcasts are grp8_bcast (8-lane groups)");
    constexpr int TPB = kPrepThreads / 64 * TPW;  // tasks per workgroup
    const int* __restrict__ al = st->alist;  // (the batch's active-task list)
    for (int blk = blockIdx.x; blk * TPB < total; blk += gridDim.x) {
        const int ti = blk * TPB + wave * TPW + lane / kPrepLanes;
        const bool valid = ti < total;
        // t: the slot (the yaw's); list mode reads the compacted task and writes the record at ti
        const int t = (al && valid) ? al[ti] : ti;
        const int ri = al ? ti : t;
        bool act = valid;
        int j = 0, own = 0, cull = 0;
        double x = 0.0, y = 0.0, px = 1.0, py = 0.0, pyaw = 0.0, cyaw = 0.0;
        double cbase = 0.0, climit = 0.0;
        int force = -1;
        if (act && tasks) {
            const SteerTask tk = tasks[ri];
            act = tk.pnode >= 0;
            if (tk.literal >= 2) force = tk.literal - 2;  // (a cached verdict, mq_sample_nn)
            x = tk.x;
            y = tk.y;
            px = act ? tk.px : 1.0;
            py = act ? tk.py : 0.0;
            pyaw = act ? tk.pyaw : 0.0;
            if (ext) {
                const StarTaskExt ex = ext[t];
                own = ex.own_yaw;
                cyaw = ex.cyaw;
                cull = ex.cull;
                cbase = ex.cbase;
                climit = ex.climit;
            }
        } else if (act) {
            window_task(t, W, wsx, wsy, snap_pose, cand, &j, &px, &py, &pyaw);
            x = wsx[j];
            y = wsy[j];
        }
        double* yaw_dst = nullptr;
        if (valid) yaw_dst = (t < W || tasks) ? snap_yaw + t : &cand[t - W].yaw;
        prep_task(sc, r, g0, ri, valid, act, x, y, px, py, pyaw, own, cyaw, cull, cbase, climit,
                  rec, yaw_dst, cost_out, force);
    }
}

// Explicit tasks (the verify_node API); waves <= kLiteralWaves so each wave owns one literal
// scratch buffer.  The fast path is the product's walk (walk_rec through walk_edge, with the
// analytic S segments), so the API's verdicts test the same code the planners run.
__global__ __launch_bounds__(256) void steer_tasks_kernel(SceneDev sc, TreeDev tr,
                                                          const SteerTask* __restrict__ tasks,
                                                          int n, int* __restrict__ out_status,
                                                          double* __restrict__ out_yaw,
                                                          double* __restrict__ scratch) {
    const int lane = __lane_id();
    const int gw = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    double* bx = scratch ? scratch + (size_t)gw * 3 * kLiteralCap : nullptr;
    __shared__ double s_gen[4][kGenSlots];
    double* gs = s_gen[__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))];
    int np = 0, na = 0;
    for (int t = gw; t < n; t += nw) {
        const SteerTask tk = tasks[t];
        double px = tk.px, py = tk.py, pyaw = tk.pyaw;
        if (tk.pnode >= 0) {
            px = tr.x[tk.pnode];
            py = tr.y[tk.pnode];
            pyaw = tr.yaw[tk.pnode];
        }
        const double yaw = atan2(py - tk.y, px - tk.x);
        int s;
        if (tk.literal && bx)
            s = steer_collide_literal(sc, tk.x, tk.y, yaw, px, py, pyaw, bx, bx + kLiteralCap,
                                      bx + 2 * kLiteralCap);
        else if (tk.literal)
            s = kError;
        else
            s = walk_edge<false, true>(sc, steer_prep(sc, tk.x, tk.y, yaw, px, py, pyaw), gs, true,
                                       np, na);
        if (lane == 0) {
            out_status[t] = s;
            out_yaw[t] = yaw;
        }
    }
}

__host__ __device__ inline int walk_lds_bytes(int scene_bytes) {
    return scene_bytes + kWalkThreads / 64 * kGenSlots * 8;
}
// steer_walk, one task per wave (persistent grid, grid-stride over the W + ncomp tasks); kLds:
// the scene's disc grid is staged into this workgroup's LDS first.
// Window mode (pend != nullptr): a snapshot task whose verdict is not final (literal path,
// error) and that has no nearer window sample is queued for the resolve (the others were queued
// by nn_finalize's pair search).  wg_points (profiling only, else null): workgroup b adds its
// walked polyline points to wg_points[b] (its own slot: no atomics on a shared address).
// kMinW: minimum waves per SIMD the compiler must allow (register budget).  The window pipeline
// walks ~1 task per wave (1: 94 VGPRs, 2 workgroups per CU); the query batches walk dozens of
// tasks per wave, latency-bound, and run better at 6 (80 VGPRs, 3 workgroups per CU: config 3
// 279 -> 309 M it/s; 8 spills too much).
constexpr int kWalkMinWWindow = 1;
constexpr int kWalkMinWBatch = 6;
// RRT* scenes (config 5) carry a ~58 KB LDS image, so LDS holds the walk at 2 workgroups per CU
// whatever the register budget: the uncapped budget wins there (16.46 vs 15.96 M it/s, r02 A/B).
constexpr int kWalkMinWStar = kWalkMinWWindow;
template <bool kLds, int kMinW, int kScene, bool kS>
__global__ __launch_bounds__(kWalkThreads, kMinW) void steer_walk_kernel(DevState* __restrict__ st,
                                                         SceneDev sc,
                                                         const PrepRec* __restrict__ rec,
                                                         CandEntry* __restrict__ cand,
                                                         int* __restrict__ snap_status,
                                                         const int* __restrict__ cand_cnt,
                                                         int* __restrict__ pend,
                                                         long long* __restrict__ wg_points) {
    const int lane = __lane_id();
    const int W = st->W;
    const int total = W + st->ncomp;
    if ((int)blockIdx.x >= total) return;
    // (the wave index as a wave-uniform value: threadIdx.x itself need not stay live)
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool t0 = threadIdx.x == 0;
    if (kLds) stage_scene(sc);
    double* gs = reinterpret_cast<double*>(pp_smem + (kLds ? sc.lds_bytes : 0)) +
                 wv * kGenSlots;  // this wave's generator slots
    int npts = 0, napts = 0, ntasks = 0;
    // Workgroup b walks the tasks b, b + G, b + 2G, ... (G = the grid); its waves take them one
    // at a time from an LDS counter, so a wave that drew short paths takes more of them (a
    // workgroup's share is a sum of dozens of tasks: far more even than a wave's handful under a
    // static stride), and consecutive tasks — one query's window, similar paths — land on
    // different workgroups.  No global atomics.  (Contiguous ranges per workgroup measured 10%
    // slower on config 5's walk.)
    __shared__ int s_next;
    const int G = (int)gridDim.x;
    if (t0) s_next = 0;
    const int* __restrict__ al = st->alist;  // (the batch's active-task list)
    const int lper = (total + G - 1) / G;
    if (al && blockIdx.x == 0 && t0) {
        st->lgrid = G;
        st->lper = lper;
    }
    __syncthreads();
    for (;;) {
        int k = 0;
        if (lane == 0) k = atomicAdd(&s_next, 1);
        const int ti = (int)blockIdx.x + G * __builtin_amdgcn_readlane(k, 0);
        if (ti >= total) break;
        // (list mode: the record is at ti; the slot t only addresses the verdict's store)
        const int t = al ? al[ti] : ti;
        const int s = walk_rec<kLds, kScene, kS>(sc, rec + ti, gs, npts, napts);
        ++ntasks;
        if (lane == 0) {
            if (al || t < W) {
                // (list mode: the workgroup's run of verdicts, DevState::lgrid / lper)
                snap_status[al ? (int)blockIdx.x * lper + (ti - (int)blockIdx.x) / G : t] = s;
                if (pend && s != kAccept && s != kReject && cand_cnt[t] == 0)
                    pend[atomicAdd(&st->npend, 1)] = t;
            } else {
                cand[t - W].status = s;
            }
        }
    }
    if (wg_points) {  // [b]: points, [kWalkTallySlots + b]: their arc points, [2 kWalkTallySlots + b]: tasks
        __shared__ int s_np[3][kWalkThreads / 64];
        if (lane == 0) {
            s_np[0][wv] = npts;
            s_np[1][wv] = napts;
            s_np[2][wv] = ntasks;
        }
        __syncthreads();
        if (wv == 0 && lane < 3) {
            long long sum = 0;
            for (int w = 0; w < kWalkThreads / 64; ++w) sum += s_np[lane][w];
            wg_points[blockIdx.x + lane * kWalkTallySlots] += sum;
        }
    }
}

// The walk's persistent grid: the workgroups that can be resident at once, so no workgroup starts
// late with a share of tasks — the device's CU count times the workgroups per CU the occupancy
// API gives for this instantiation and its dynamic LDS (the scene image decides; at most 4 of 8
// waves each), read once per (device, image size) instead of assuming 256 CUs and 160 KB.
// kMaxPerCU: the query batch's walk runs beside the other sub-batch stream's kernels and does best
// at 2 workgroups per CU although 3 fit (a 1024-query shard 171 -> 179-183 M it/s, the 8192-query
// batch unchanged).
// The walk instantiation for a scene: LDS image or not, and its mode (scene_kind), as a callable
// applied to the kernel (launch or occupancy query).
// (polygon scenes walk at most 5 waves per SIMD: their edge tests do not fit the 6-wave budget
// without scratch; with the analytic S segments at most 4: s_classify_poly spills ~80 B at 5)
template <int kMinW, bool kS = false, typename F>
inline hipError_t walk_kernel_for(const SceneDev& sc, F&& f) {
    const bool lds = sc.lds_bytes > 0;
    constexpr int kPolyCap = kS ? 4 : 5;
    constexpr int kMinWPoly = kMinW > kPolyCap ? kPolyCap : kMinW;
    switch (scene_kind(sc)) {
        case kSceneGrid:
            return lds ? f(steer_walk_kernel<true, kMinW, kSceneGrid, kS>)
                       : f(steer_walk_kernel<false, kMinW, kSceneGrid, kS>);
        case kScenePoly:
            return lds ? f(steer_walk_kernel<true, kMinWPoly, kScenePoly, kS>)
                       : f(steer_walk_kernel<false, kMinWPoly, kScenePoly, kS>);
        default:
            return lds ? f(steer_walk_kernel<true, kMinW, kSceneDisc, kS>)
                       : f(steer_walk_kernel<false, kMinW, kSceneDisc, kS>);
    }
}

// A profile's walk instantiation for a scene (pp_steer_launch.h lists the profiles).  The grid
// cap is read for the instantiation that is launched: kMinW and the S classes (a polygon walk's
// budget) change what fits a CU.
template <typename F>
inline hipError_t walk_profile_for(WalkProfile p, const SceneDev& sc, F&& f) {
    switch (p) {
        case kWalkWindow:
            return walk_kernel_for<kWalkMinWWindow, false>(sc, f);
        case kWalkBatchPlan:
        case kWalkBatchBig:
            return walk_kernel_for<kWalkMinWBatch, true>(sc, f);
        case kWalkBatchSmall:
            return walk_kernel_for<kWalkMinWBatch - 1, true>(sc, f);
        case kWalkStar:
            return walk_kernel_for<kWalkMinWStar, true>(sc, f);
    }
    return hipErrorInvalidValue;
}
inline int walk_max_per_cu(WalkProfile p) {
    return (p == kWalkBatchBig || p == kWalkBatchSmall) ? 2 : 4;
}

int walk_grid_cap(WalkProfile p, const SceneDev& sc) {
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, int>, int> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    const std::tuple<int, int, int, int> key{(int)p, dev, sc.lds_bytes, scene_kind(sc)};
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int cus = 256, per_cu = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
    const hipError_t e = walk_profile_for(p, sc, [&](auto kern) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kWalkThreads,
                                                            walk_lds_bytes(sc.lds_bytes));
    });
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    per_cu = std::min(walk_max_per_cu(p), per_cu);
    const int cap = cus * per_cu;
    cache[key] = cap;
    return cap;
}

void launch_walk(WalkProfile p, hipStream_t s, int blocks, DevState* st, const SceneDev& sc,
                 const PrepRec* rec, CandEntry* cand, int* status, const int* cand_cnt, int* pend,
                 long long* wg_points) {
    (void)walk_profile_for(p, sc, [&](auto kern) {
        kern<<<blocks, kWalkThreads, walk_lds_bytes(sc.lds_bytes), s>>>(
            st, sc, rec, cand, status, cand_cnt, pend, wg_points);
        return hipSuccess;
    });
}

void launch_prep_window(hipStream_t s, int blocks, const DevState* st, const SceneDev& sc,
                        const double* wsx, const double* wsy, const double* snap_pose,
                        CandEntry* cand, PrepRec* rec, double* snap_yaw) {
    steer_prep_kernel<<<blocks, kPrepThreads, 0, s>>>(st, sc, wsx, wsy, snap_pose, cand, rec,
                                                      snap_yaw, nullptr, nullptr, nullptr);
}

void launch_prep_tasks(hipStream_t s, int blocks, const DevState* st, const SceneDev& sc,
                       PrepRec* rec, double* yaw, const SteerTask* tasks, double* cost,
                       const StarTaskExt* ext) {
    steer_prep_kernel<<<blocks, kPrepThreads, 0, s>>>(st, sc, nullptr, nullptr, nullptr, nullptr,
                                                      rec, yaw, tasks, cost, ext);
}

// Space::verify (rrt.rs:124-137) of whole polylines, one wave per line: chunks of 63 points
// (lane 0 carries the previous chunk's last point) through the walk's chunk test — every point
// in bounds (and in a free cell, config 4), every segment clear of the discs / edge buffers; a
// one-point line is its degenerate segment.  Polygon mode: point 0 outside every obstacle
// polygon (Q10p: with no segment meeting an edge buffer the line is on one side).
__global__ __launch_bounds__(256) void verify_lines_kernel(SceneDev sc, const double* __restrict__ X,
                                                          const double* __restrict__ Y,
                                                          const int64_t* __restrict__ off, int k,
                                                          uint8_t* __restrict__ ok) {
    const int lane = __lane_id();
    const int gw = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    for (int i = gw; i < k; i += nw) {
        const int64_t a = off[i], n = off[i + 1] - a;
        bool good = true;
        if (n > 0) {
            if (n == 1) {
                const bool has = lane == 0;
                good = !chunk_rejects<false>(sc, has, has, has, X[a], Y[a]);
            } else {
                // lane l holds point c0 + l; lane 0 is the previous chunk's last point (checked)
                for (int64_t c0 = 0; c0 + 1 < n && good; c0 += 63) {
                    const int64_t j = c0 + lane;
                    const bool has = j < n;
                    const double qx = has ? X[a + j] : 0.0, qy = has ? Y[a + j] : 0.0;
                    good = !chunk_rejects<false>(sc, has, has && (lane >= 1 || c0 == 0),
                                                 has && lane >= 1, qx, qy);
                }
            }
            if (good && sc.ne > 0 &&
                in_obstacle(sc.ne, sc.ex0, sc.ey0, sc.ex1, sc.ey1, sc.epoly, X[a], Y[a]))
                good = false;
        }
        if (lane == 0) ok[i] = good ? 1 : 0;
    }
}

hipError_t launch_verify_lines(hipStream_t st, const SceneDev& sc, const double* X,
                               const double* Y, const int64_t* off, int k, uint8_t* ok) {
    if (k <= 0) return hipSuccess;
    const int waves = std::min(k, 16384);
    verify_lines_kernel<<<(waves + 3) / 4, 256, 0, st>>>(sc, X, Y, off, k, ok);
    return hipGetLastError();
}

hipError_t launch_steer_tasks(hipStream_t st, const SceneDev& sc, const TreeDev& tr,
                              const SteerTask* tasks, int n, int* out_status, double* out_yaw,
                              double* scratch) {
    if (n <= 0) return hipSuccess;
    int waves = n;
    if (scratch && waves > kLiteralWaves) waves = kLiteralWaves;
    if (waves > 16384) waves = 16384;
    steer_tasks_kernel<<<(waves + 3) / 4, 256, 0, st>>>(sc, tr, tasks, n, out_status, out_yaw,
                                                        scratch);
    return hipGetLastError();
}

hipError_t launch_dubins_origin(hipStream_t st, const double* conf, int n, int cap, double* px,
                                double* py, double* pyaw, int* n_out, int* word_out,
                                double* cost_out, int* status_out) {
    if (n <= 0) return hipSuccess;
    dubins_origin_kernel<<<(n + 63) / 64, 64, 0, st>>>(conf, n, cap, px, py, pyaw, n_out, word_out,
                                                       cost_out, status_out);
    return hipGetLastError();
}

hipError_t launch_dubins_words(hipStream_t st, const double* abd, int n, double* tpq, int* ok) {
    if (n <= 0) return hipSuccess;
    dubins_words_kernel<<<(n + 63) / 64, 64, 0, st>>>(abd, n, tpq, ok);
    return hipGetLastError();
}

hipError_t launch_sincos_small(hipStream_t st, const double* x, int n, double* s, double* c,
                               double* s_ocml, double* c_ocml) {
    if (n <= 0) return hipSuccess;
    sincos_small_kernel<<<(n + 255) / 256, 256, 0, st>>>(x, n, s, c, s_ocml, c_ocml);
    return hipGetLastError();
}

hipError_t launch_dubins_batch(hipStream_t st, const double* conf, int n, int cap, double* px,
                               double* py, double* pyaw, int* n_out, int* word_out,
                               double* cost_out, int* status_out) {
    if (n <= 0) return hipSuccess;
    dubins_batch_kernel<<<(n + 63) / 64, 64, 0, st>>>(conf, n, cap, px, py, pyaw, n_out, word_out,
                                                      cost_out, status_out);
    return hipGetLastError();
}

}  // namespace ppamd

// pp_ctx.h — what the host API's source files share: the error helpers, the device / pinned
// buffers, the context (pp_ctx) with one member per subsystem, and the few cross-file helpers.
//   pp_context.cpp  context, errors, statistics, profiling, the Dubins entry points
//   pp_space.cpp    the scene
//   pp_rrt.cpp      the one-tree planner and its window buffers
//   pp_finish.cpp   check_finish / optimize / finalize, pp_rrt_plan, pp_batch_plan, pp_batch_paths
//   pp_batch.cpp    the forest of per-query trees, pp_batch_*, pp_star_*
//   pp_star_goal.cpp  the RRT* goal connection: pp_star_plan, pp_star_goal_costs, pp_star_path,
//                     pp_star_paths
//   pp_revalidate.cpp  a tree across a scene change: pp_rrt_revalidate, pp_batch_revalidate,
//                      pp_star_revalidate
//   pp_repair.cpp   the re-attachment rounds: pp_star_repair (that revalidation with the rounds) and
//                   pp_star_advance (a node becomes the root; the rounds on its ancestors)
//   pp_relax.cpp    pp_star_relax: choose-parent rounds over every node of the RRT* trees
//   pp_prune.cpp    pp_star_prune: its doubling and compaction behind the focus bound's verdicts
//   pp_forest_io.cpp  pp_star_forest_export / _import, pp_batch_forest_export / _import
//   pp_segments.cpp  pp_star_path_segments, pp_batch_path_segments, pp_star_chain_segments,
//                    pp_segments_sample
//   pp_shortcut.cpp  pp_star_shortcut, pp_star_shortcut_edges, pp_star_shortcut_commit
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pathplanning_amd.h"
#include "pp_device.h"
#include "pp_kernels.h"
#include "pp_scene.h"

namespace ppamd {

int set_err(int code, const std::string& msg);  // (the thread's pp_last_error)

#define PP_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return set_err(PP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

// a grow-only buffer of n elements in device memory, or (kPinned) in pinned host memory
template <typename T, bool kPinned = false>
struct DBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t reserve(size_t count) {
        if (count <= n) return hipSuccess;
        release();
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        hipError_t e = kPinned ? hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault)
                               : hipMalloc(reinterpret_cast<void**>(&p), bytes);
        if (e == hipSuccess) n = count;
        else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        n = 0;
    }
    ~DBuf() { release(); }
};
template <typename T>
using HBuf = DBuf<T, true>;  // pinned host staging

constexpr int kMaxBatch = 64;  // windows enqueued between two host synchronisations
constexpr int kInsideCells = 2048;  // the inside bitmap's cells per axis (point_blocked)
constexpr int kScreenPad = 64;  // f32 screen copies: the LDS-DMA reads whole float4s (<= 3 floats past)
constexpr int kMaxSub = 4;  // sub-batches of a query batch, each on its own stream

// ---- scene (Space)
struct Scene {
    bool valid = false;  // pp_space_new / pp_space_new_polygons succeeded
    double minx = 0, maxx = 0, miny = 0, maxy = 0;
    double width = 0, height = 0, max_steer = 0;
    int m = 0;
    DBuf<double> d_cx, d_cy, d_r2, d_rcull;
    DBuf<int> d_goff, d_gitems;
    DBuf<uint4> d_img, d_gimg;  // LDS images (discs / occupancy bits), contiguous
    double gx0 = 0, gy0 = 0, ginv = 1;
    int gnx = 1, gny = 1;
    int lds_bytes = 0, lds_goff = 0, lds_items = 0, lds_cx = 0, lds_cy = 0, lds_r2 = 0, lds_d4 = 0;
    DBuf<float4> d_d4;
    // occupancy grid (config 4)
    bool has_grid = false;
    DBuf<uint32_t> d_bits;
    int bw = 0, bh = 0, bwords = 0, lds_bits_bytes = 0;
    double bx0 = 0, by0 = 0, binv = 1;
    // polygon mode (pp_space_new_polygons, Q10p): obstacle edges, bounds ring; host copies for
    // the point checks (root / query starts)
    // disc scenes: the inside bitmap (scene::inside_bitmap), the point_blocked pre-test
    DBuf<uint32_t> d_ibits;
    int ibn = 0;
    double ibx0 = 0.0, iby0 = 0.0, ibinv = 1.0;
    // the share of the pre-test's cells that are set (inside bitmap / occupancy grid): what the
    // extend loop expects of a window's draws before it has counters of its own (0: no pre-test)
    double blocked_share = 0.0;
    int ne = 0, nbv = 0;
    double h2 = 0.0;
    float cull_slack = 1.0e-3f;
    DBuf<double> d_ex0, d_ey0, d_ex1, d_ey1, d_bvx, d_bvy;
    DBuf<int> d_epoly;
    std::vector<double> h_ex0, h_ey0, h_ex1, h_ey1, h_bvx, h_bvy;
    std::vector<int> h_epoly;

    bool polygons() const { return ne > 0 || nbv > 0; }
    // the kernels' view, with the caller's step size and (one-tree planner) blocked root
    SceneDev dev(double step, bool root_blocked) const {
        SceneDev s;
        s.minx = minx;
        s.maxx = maxx;
        s.miny = miny;
        s.maxy = maxy;
        s.turn_radius = max_steer;
        s.step_size = step;
        s.m = m;
        s.cx = d_cx.p;
        s.cy = d_cy.p;
        s.r2 = d_r2.p;
        s.rcull = d_rcull.p;
        s.gx0 = gx0;
        s.gy0 = gy0;
        s.ginv = ginv;
        s.gcell = 1.0 / ginv;
        s.gnx = gnx;
        s.gny = gny;
        s.goff = d_goff.p;
        s.gitems = d_gitems.p;
        s.lds_bytes = lds_bytes;
        s.lds_goff = lds_goff;
        s.lds_items = lds_items;
        s.lds_cx = lds_cx;
        s.lds_cy = lds_cy;
        s.lds_r2 = lds_r2;
        s.d4 = d_d4.p;
        s.lds_d4 = lds_d4;
        s.bits = has_grid ? d_bits.p : nullptr;
        s.bw = bw;
        s.bh = bh;
        s.bwords = bwords;
        s.bx0 = bx0;
        s.by0 = by0;
        s.binv = binv;
        s.img = d_img.p;
        if (has_grid) {
            s.lds_bytes = lds_bits_bytes;
            s.img = d_gimg.p;
        }
        s.ne = ne;
        s.ex0 = d_ex0.p;
        s.ey0 = d_ey0.p;
        s.ex1 = d_ex1.p;
        s.ey1 = d_ey1.p;
        s.epoly = d_epoly.p;
        s.h2 = h2;
        s.nbv = nbv;
        s.bvx = d_bvx.p;
        s.bvy = d_bvy.p;
        s.cull_slack = cull_slack;
        s.root_blocked = root_blocked ? 1 : 0;
        s.ibits = ibn > 0 ? d_ibits.p : nullptr;
        s.ibn = ibn;
        s.ibwords = ibn / 32;
        s.ibx0 = ibx0;
        s.iby0 = iby0;
        s.ibinv = ibinv;
        return s;
    }
    // Space::verify of the one-point line [(x, y)] on the host, polygon mode (Q10p; the same
    // arithmetic as the kernels and the oracle): bounds, edge buffers, inside an obstacle
    bool point_ok(double x, double y) const {
        SceneDev s = dev(0.0, false);  // (bounds, nbv, h2) with the ring's host copy
        s.bvx = h_bvx.data();
        s.bvy = h_bvy.data();
        if (!point_in_bounds(s, x, y)) return false;
        for (int k = 0; k < ne; ++k)
            if (seg_hits_edge(x, y, x, y, h_ex0[k], h_ey0[k], h_ex1[k], h_ey1[k], h2)) return false;
        return !in_obstacle(ne, h_ex0.data(), h_ey0.data(), h_ex1.data(), h_ey1.data(),
                            h_epoly.data(), x, y);
    }
};

// ---- planner (RRT): the one tree and its window buffers
struct Planner {
    bool valid = false;  // pp_rrt_new succeeded for the current scene
    bool stale = false;  // a scene change invalidated the planner, its tree is still on the device
    double start[3] = {0, 0, 0}, goal[3] = {0, 0, 0};
    int64_t max_iter = 0;
    double step = 0.1;
    uint64_t seed = 0;
    int64_t it = 0;   // mirror of DevState.it (exact after every synchronisation)
    int64_t seq = 0;  // windows enqueued so far (their sequence numbers)
    int64_t n = 0;    // mirror of DevState.n
    double blocked_share = -1.0;  // draws in an obstacle per iteration, last batch (< 0: none yet)
    int64_t cap = 0;  // tree capacity
    double eps_coord = 0.0;
    bool root_blocked = false;  // polygon mode: the root fails verify (nothing is ever inserted)
    DBuf<float> x32, y32;
    DBuf<double> X, Y, YAW;
    DBuf<int> PAR;
    DBuf<DevState> d_state, d_api_state;
    HBuf<DevState> h_state;
    // pp_rrt_extend_samples: the caller's samples and the per-iteration record (one chunk)
    DBuf<double> hs_x, hs_y, hs_yaw;
    DBuf<int> hs_par;
    DBuf<uint8_t> hs_ok;

    // ---- window buffers (sized for Kcap)
    int K = 4096;
    int Kcap = 0;
    DBuf<double> wsx, wsy, nn_d2, snap_yaw, snap_pose;
    DBuf<float> pbest, psecond, wsx32, wsy32;
    DBuf<int> perm, cofs, ipos;
    DBuf<float2> sxy;
    DBuf<double> sqb, ssx, ssy;
    DBuf<float2> ob;
    DBuf<int> pidx, nn_idx, cand_cnt, snap_status;
    DBuf<CandEntry> cand;
    DBuf<PrepRec> rec;   // per-task steer records
    DBuf<int> r_order, r_rep, pend, fin_par;
    DBuf<int> iter_off;        // [2 Kcap] window sample -> its iteration's offset in the window
    DBuf<SceneDev> d_scene;    // the scene in device memory (samples_role, the literal paths)
    DBuf<double> r_repyaw;
    DBuf<double> lit_scratch;  // resolve: one literal buffer per wave
    // verify_node API
    DBuf<SteerTask> tasks;
    DBuf<int> task_status;
    DBuf<double> task_yaw;
    HBuf<SteerTask> h_tasks;

    TreeDev tree_dev() const {
        TreeDev t;
        t.x32 = x32.p;
        t.y32 = y32.p;
        t.x = X.p;
        t.y = Y.p;
        t.yaw = YAW.p;
        t.parent = PAR.p;
        return t;
    }
    WindowArgs window_args(const SceneDev& sc, long long* wg_points, DevState* st) const {
        WindowArgs a;
        a.K = Kcap;
        a.Kcap = Kcap;
        a.seed = seed;
        a.eps_coord = eps_coord;
        a.st = st;
        a.sc = sc;
        a.tr = tree_dev();
        a.wsx = wsx.p;
        a.wsy = wsy.p;
        a.wsx32 = wsx32.p;
        a.wsy32 = wsy32.p;
        a.perm = perm.p;
        a.cofs = cofs.p;
        a.sxy = sxy.p;
        a.sq = sqb.p;
        a.ssx = ssx.p;
        a.ssy = ssy.p;
        a.ob = ob.p;
        a.ipos = ipos.p;
        a.pbest = pbest.p;
        a.psecond = psecond.p;
        a.pidx = pidx.p;
        a.nn_idx = nn_idx.p;
        a.nn_d2 = nn_d2.p;
        a.cand_cnt = cand_cnt.p;
        a.cand = cand.p;
        a.snap_status = snap_status.p;
        a.snap_yaw = snap_yaw.p;
        a.snap_pose = snap_pose.p;
        a.rec = rec.p;
        a.pend = pend.p;
        a.fin_par = fin_par.p;
        a.rs.order = r_order.p;
        a.rs.rep = r_rep.p;
        a.rs.repyaw = r_repyaw.p;
        a.lit_scratch = lit_scratch.p;
        a.wg_points = wg_points;
        a.scp = d_scene.p;
        a.iter_off = iter_off.p;
        a.pretest = d_scene.p ? 1 : 0;
        return a;
    }
};

// ---- check_finish buffers (cf_run, cf_run_rounds)
struct Finish {
    DBuf<SceneDev> scene;   // check_finish_kernel's scene (its step may be a batch's)
    SceneDev scene_host{};  // what `scene` holds (the source of its last upload)
    bool scene_ok = false;
    // the last cf_run's one line was counted, not stored (cf_line_kernel's error bit 32:
    // finalize's unverified line past the point capacity)
    bool counted_only = false;
    DBuf<int> nodes, ok, npts, chain, etab, err, path, items;
    DBuf<int> lpath, spill;  // cf_line_kernel's ancestor paths; tier 1's spill list
    DBuf<int> memo;  // check_finish_kernel's optimize memo (CfBatch::ftab / gtab), per launch
    DBuf<double> len, pts;
};

// ---- packed line export (pp_batch_paths / pp_star_paths): the call's items, counts, row
// offsets and the packed points, sized to the call
struct PathExport {
    DBuf<int> qidx, nodes, slot, ok, cnt, items;
    DBuf<double> len, x, y;
    DBuf<int64_t> off;
    DBuf<uint8_t> okq;
};
// the most points one export call stages on the device (x and y: 16 B a point, 1 GiB)
constexpr int64_t kPathsMaxPoints = (int64_t)1 << 26;

// ---- segment export and sampling (pp_*_path_segments, pp_segments_sample: SegArgs,
// SegSampleArgs), sized to the call: the ancestor paths and the spill list of the export's waves,
// the packed segment rows (the export's staging, the sampler's input), the sampler's per-row
// values and its packed samples
struct SegExport {
    DBuf<int> path, spill;
    DBuf<double> x, y, yaw, kappa, len;
    DBuf<int64_t> off, nfull, cnt, poff;
    DBuf<double> P, rowlen, sx, sy, syaw, skappa, ss;
};
// the most samples one pp_segments_sample call stages on the device
constexpr int64_t kSegMaxSamples = (int64_t)1 << 26;

// ---- a forest of per-query SoA trees: the host side of MqDev's shared part, under both the
// extend batch (config 3) and the RRT* batch (config 5).  Tree q lives in rows [q * cap, q * cap +
// n[q]); the forest runs as nsub sub-batches of consecutive queries, each on its own stream.
struct Forest {
    int Q = 0, cap = 0;
    int64_t max_iter = 0;
    double step = 0.1;
    int nsub = 1;  // fixed by init(): the sub-batch DevStates are written for this split
    bool any_blocked = false;
    DBuf<double> x, y, yaw;  // [Q * cap]
    DBuf<int> parent;
    DBuf<int> n;             // [Q] and below
    DBuf<int64_t> it, evals;
    DBuf<int64_t> target;    // iteration targets of the running extend call
    DBuf<uint64_t> seed;
    DBuf<uint8_t> blocked;   // polygon mode: the root fails verify
    DBuf<double> d_starts;   // [3Q] the roots as uploaded (the init kernels read them)

    // reserve q trees of max_iter + 1 rows, upload the roots (RRT::new per query, rrt.rs:344-346:
    // row 0 of each tree) and seeds, and test the roots (polygon mode); enqueued on c->stream
    int init(pp_ctx* c, int q, int64_t max_iter_, double step_, const double* starts,
             const uint64_t* seeds, int nsub_);
    MqDev dev() const;  // the kernels' view of the shared fields (the whole forest)
    int q_begin(int s) const { return (int)((int64_t)Q * s / nsub); }  // sub-batch s: [q_begin(s), q_begin(s + 1))
    // d restricted to the queries [q0, q1): the one place that offsets the shared pointers
    MqDev sub(MqDev d, int q0, int q1) const;
    const uint8_t* blocked_dev() const { return any_blocked ? blocked.p : nullptr; }
    TreeDev tree_dev() const;  // the SoA rows (query q: offset q * cap)
    // The copy-outs below take one more array of the same shape (`extra`: RRT*'s rewires / cost)
    // and synchronise once.  Sums over the queries of it, n and extra:
    int totals(pp_ctx* c, int64_t* it_sum, int64_t* n_sum, const int64_t* extra = nullptr,
               int64_t* extra_sum = nullptr) const;
    // the per-query counters (a null output is skipped)
    int copy_state(pp_ctx* c, int32_t* n_nodes, int64_t* iterations, int64_t* node_evals,
                   const int64_t* extra = nullptr, int64_t* extra_out = nullptr) const;
    // the trees' sizes on the host after one synchronise, and (may be null) their sum.  nodes (may
    // be null): one node per query, each -1 or a node of its tree, else PP_ERR_INVALID_ARGUMENT
    // with the caller's message
    int sizes(pp_ctx* c, std::vector<int>* hn, int64_t* total = nullptr,
              const int32_t* nodes = nullptr, const char* bad_node = nullptr) const;
    // what a revalidation of the forest reads first: the trees' sizes and, in polygon mode, the
    // roots that fail verify in the scene as it is now (*any: at least one does) ...
    int reval_inputs(pp_ctx* c, std::vector<int>* hn, std::vector<uint8_t>* blk, bool* any) const;
    // ... and what it leaves behind: the derived blocked[] and the sizes for the caller (may be
    // null), synchronised
    int reval_outputs(pp_ctx* c, const std::vector<uint8_t>& blk, bool any, int32_t* n_nodes);
    // one tree's rows (*n_out: its nodes, also when ocap is too small)
    int export_tree(pp_ctx* c, int query, double* ox, double* oy, double* oyaw, int32_t* oparent,
                    int64_t ocap, int64_t* n_out, const double* extra = nullptr,
                    double* extra_out = nullptr) const;
};

// ---- multi-query batch (config 3): the forest plus the speculative-window arrays, and
// pp_batch_plan's buffers
struct Batch {
    bool valid = false;  // false on entry to pp_batch_new, true only on its success
    bool stale = false;  // a scene change invalidated the batch, its forest is still on the device
    Forest f;
    DBuf<double> yawbuf;
    DBuf<int> status, err, alist, lstat;
    DBuf<int64_t> itprev;      // the lockstep NN's verdict cache (MqDev::it_prev)
    int K = 1;                 // speculative window per query of the current batch
    int K_user = 0;            // pp_batch_set_window (0: automatic)
    DBuf<double> nnd2;         // [Q * kMqMaxK]
    DBuf<SteerTask> tasks, ctask;
    DBuf<PrepRec> rec;
    DBuf<DevState> state;      // [1 + kMaxSub]: the whole batch, then one per sub-batch (mq_sub_args)
    DBuf<SceneDev> scene;      // the scene in device memory (point_blocked)
    std::vector<double> goal;  // 3 per query (RRT::new's goal; pp_batch_plan)
    DBuf<double> goal_d;       // [3Q] the goals on the device (pp_batch_plan)
    DBuf<int> mp_off, mp_qidx, mp_nodes, mp_ok, mp_npts, mp_best, mp_bpts, mp_nfin;
    DBuf<double> mp_len, mp_blen;
    // pp_batch_plan's check_finish in steer rounds (CfbArgs)
    DBuf<int> cfb_nodei;   // [4 (nitems + Q)]: depth, open, tfirst, tcnt
    DBuf<int> cfb_rows;    // [rows]: gclaim
    DBuf<unsigned char> cfb_rows8;  // [2 rows]: tnone, tnone_up
    DBuf<int> cfb_gotab, cfb_plist, cfb_tnode, cfb_status, cfb_misc, cfb_lit, cfb_dhist;
    DBuf<SteerTask> cfb_tasks;
    DBuf<StarTaskExt> cfb_ext;
    DBuf<PrepRec> cfb_rec;
    DBuf<unsigned char> cfb_none;
    DBuf<double> cfb_yaw;
    DBuf<DevState> cfb_state;
    DBuf<long long> cfb_pts;  // profiling: the rounds' walk point tallies
    bool cf_rounds = true;  // pp_batch_plan in steer rounds (pp_batch_set_finish_schedule)
    int cfb_span0 = kCfbSpan, cfb_span = kCfbSpan;  // phase A candidates per node: first / later rounds
};

// ---- RRT* query batch (BASELINE config 5, build-defined: DESIGN.md §3.7): the forest plus costs,
// the kNN slots and the three rounds' task arrays
struct StarBatch {
    bool valid = false;  // false on entry to pp_star_new, true only on its success
    Forest f;
    int kfix = 0;
    double eta = 0.0;
    DBuf<double> cost, elen, px, py, cb;
    DBuf<int> mark, stamp, ksched, pn, near, nnear, bslot, cslot, err;
    DBuf<uint64_t> cmask, bmask;
    DBuf<int64_t> rew;
    // focused sampling (pp_star_set_focus): focus point [2Q], bound [Q] (+inf none), draws skipped [Q]
    DBuf<double> fxy, fbound;
    DBuf<int64_t> skipped;
    DBuf<DevState> state;  // [3 * (1 + kMaxSub)]: rounds A, B, C of the batch, then per sub-batch
    DBuf<SteerTask> tA, tB, tC;
    DBuf<StarTaskExt> eB, eC;
    DBuf<int> sA, sB, sC;
    DBuf<double> yA, yB, yC, cA, cB, cC;
    DBuf<PrepRec> rec;
    // the goal connection (pp_star_plan / pp_star_goal_costs: StarGoalArgs), reserved on first use
    DBuf<double> goal_d, gbest, gtotal;
    DBuf<int> gslot, gnode;
    DBuf<uint64_t> gmask;
    DBuf<long long> gsteer;
};

// ---- revalidation (pp_rrt_revalidate / pp_batch_revalidate / pp_star_revalidate: RevalArgs),
// reserved on first use
constexpr int kRevalSlice = 32768;  // steer tasks per slice
struct Reval {
    DBuf<SteerTask> tasks;
    DBuf<StarTaskExt> ext;
    DBuf<PrepRec> rec;
    DBuf<int> status, off, bsum, pos, new_index, spar, err;
    DBuf<double> yaw, sx, sy, syaw;
    DBuf<double> scost, selen;  // RRT* only
    DBuf<long long> srow;
    DBuf<unsigned> v0, v1;
    DBuf<uint8_t> blocked;
    DBuf<DevState> state;
    // pp_star_repair only (RepairArgs)
    DBuf<unsigned> vedge;
    DBuf<unsigned char> flag, top, qhas;
    DBuf<int> lvl, wpar, tops, tslot, tcnt, near;
    DBuf<double> wcost, welen, tcost;
    DBuf<RepairRec> rrec;
    // pp_star_prune (PruneArgs); pp_star_advance's nodes, hops and roots (AdvanceArgs);
    // pp_star_relax's per-query rewires
    DBuf<int> keep;
    // pp_star_relax (RelaxArgs): its counters, and the last call's for pp_star_relax_counts; its
    // other buffers are the repair's (tasks .. yaw, tcost, tslot, tcnt, wpar, welen, lvl; flag:
    // the changed costs; qhas: the active queries)
    DBuf<RelaxRec> relax_rec;
    int64_t relax_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// ---- packed forest export / import (pp_*_forest_export / pp_*_forest_import: ForestIoArgs), sized
// to the call: the served slots, their row offsets, one staging buffer per row array and per
// per-slot array, the validation's levels and verdicts
struct ForestIo {
    DBuf<int> slots, spar, lvl, verdict;
    DBuf<int64_t> off, sit, sevals, srew, sskipped;
    DBuf<uint64_t> sseed;
    DBuf<double> sx, sy, syaw, scost, selen, scost_in, sfxy, sfbound;
    DBuf<uint8_t> sblocked;
};

// ---- shortcuts along the chain (pp_star_shortcut / pp_star_shortcut_edges: ShortcutArgs), sized
// to the call; cchain / coff: pp_star_chain_segments' uploaded chains
struct Shortcut {
    DBuf<int> chain, next, depth, plen, err, out, cchain, res;
    DBuf<int64_t> npair, pbase, boff, tdst, off, coff;
    DBuf<double> band, cost;
};
// the most (i, j) pairs one pp_star_shortcut call steers
constexpr int64_t kShortcutMaxPairs = (int64_t)1 << 26;

// ---- HIP events with an owner: created on demand, destroyed with it (a context's profiling
// events; one call's timing events, whichever way the call returns)
struct Events {
    std::vector<hipEvent_t> ev;
    Events() = default;
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    hipError_t reserve(size_t count) {  // at least `count` events
        while (ev.size() < count) {
            hipEvent_t e = nullptr;
            if (hipError_t r = hipEventCreate(&e)) return r;
            ev.push_back(e);
        }
        return hipSuccess;
    }
    hipEvent_t& operator[](size_t i) { return ev[i]; }
    hipEvent_t* data() { return ev.data(); }
    ~Events() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

// ---- profiling
struct Profiling {
    bool on = false;
    Events ev;  // 4 per window or batch step, 8 per RRT* step
    double nn_scan_ms = 0.0, steer_ms = 0.0, finish_ms = 0.0, finalize_ms = 0.0, prep_ms = 0.0,
           insert_ms = 0.0;
    int64_t nn_scan_launches = 0, steer_launches = 0, finish_launches = 0;
    int64_t batch_steps = 0, batch_passes = 0;
    int64_t cfb_nodes = 0, cfb_edges = 0, cfb_points = 0, cfb_arc = 0;  // the batch plan's steer rounds
    DBuf<long long> cf_tally;  // check_finish (profiling): nodes, edges, points, arc points
    DBuf<long long> wg_pts;  // walked polyline points per walk workgroup (profiling on)
    long long* points() const { return on ? wg_pts.p : nullptr; }
    // every counter of pp_stats that lives on the host or in the profiling tallies (not DevState)
    int reset_host_stats(hipStream_t stream) {
        nn_scan_ms = steer_ms = finish_ms = finalize_ms = prep_ms = insert_ms = 0.0;
        nn_scan_launches = steer_launches = finish_launches = 0;
        batch_steps = batch_passes = 0;
        cfb_nodes = cfb_edges = cfb_points = cfb_arc = 0;
        if (wg_pts.p && hipMemsetAsync(wg_pts.p, 0, wg_pts.n * sizeof(long long), stream) != hipSuccess)
            return PP_ERR_HIP;
        if (cf_tally.p && hipMemsetAsync(cf_tally.p, 0, cf_tally.n * sizeof(long long), stream) != hipSuccess)
            return PP_ERR_HIP;
        return hipStreamSynchronize(stream) == hipSuccess ? PP_OK : PP_ERR_HIP;
    }
};

}  // namespace ppamd

struct pp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t sub_stream[ppamd::kMaxSub] = {};  // sub-batch streams 1.. (0 is `stream`), created on first use
    hipEvent_t fork_ev = nullptr;
    ppamd::DBuf<double> api_lit_scratch;  // literal buffers of the API paths (kLiteralWaves slots)
    ppamd::DBuf<int> lit_locks;  // literal scratch slot locks (api_lit_scratch), zeroed once

    ppamd::Scene scene;
    ppamd::Planner rrt;
    ppamd::Finish cf;
    ppamd::Batch batch;
    ppamd::StarBatch star;
    ppamd::PathExport paths;
    ppamd::SegExport seg;
    ppamd::Reval reval;
    ppamd::ForestIo fio;
    ppamd::Shortcut shortcut;
    ppamd::Profiling prof;

    // the scene as the one-tree planner's kernels see it (its step, its blocked root)
    ppamd::SceneDev scene_dev() const { return scene.dev(rrt.step, rrt.root_blocked); }

    ~pp_ctx() {
        if (fork_ev) (void)hipEventDestroy(fork_ev);
        for (auto& ss : sub_stream)
            if (ss) (void)hipStreamDestroy(ss);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace ppamd {

int check_ctx(pp_ctx* c, bool need_scene, bool need_rrt);
// check_ctx with a scene, and an RRT* batch (pp_star_new succeeded): every pp_star_* entry point
int star_ready(pp_ctx* c);
// The coordinates v[0], v[stride], ... (n of them; a null v passes) are finite and at most
// PP_COORD_MAX in magnitude, else PP_ERR_INVALID_ARGUMENT naming `what`: every entry point that
// takes positions runs this on the host before it launches anything (pp_coord_check's test).
int check_coords(const double* v, int64_t n, int64_t stride, const char* what);
int ensure_events(pp_ctx* c, size_t count);
// reserve the API literal scratch pool and (once, zeroed on `st`) its slot locks
int ensure_literal_pool(pp_ctx* c, hipStream_t st);
// the RRT* batch's kernel arguments, the whole batch's view (pp_batch.cpp)
StarArgs star_args(pp_ctx* c);
// |X_near| of an insert into an n-node RRT* tree (pp_batch.cpp; the batch's ksched[] holds it)
int star_k(int k_fixed, int n);
// The steps pp_batch_paths and pp_star_paths share (pp_finish.cpp).  paths_items: the call's
// (query, node) items from nodes[0, Q) (-1: skipped; sizes: the trees' node counts) into
// paths.qidx / nodes / slot on the device, *k their count.  paths_sizes: the rows' offsets from
// paths.cnt / ok by the scan, to the caller (off, ok, n_total), and the capacity checks; *go:
// the caller wants the points and there are some.  paths_write: the write pass over `items`
// into paths.x / y and their copy to x / y (and of the k items' lengths, paths.len, to len_host),
// then one synchronise.
int paths_items(pp_ctx* c, const Forest& f, const int32_t* nodes, int* k);
int paths_sizes(pp_ctx* c, int Q, int64_t* off, const double* x, const double* y, int64_t cap,
                int64_t* n_total, uint8_t* ok, bool* go);
int paths_line_buffers(pp_ctx* c, int k, CfLines& lines);
// pp_batch_paths' check_finish step, shared with pp_batch_path_segments (pp_segments.cpp): the
// batch's goals to the device (batch.goal_d) and check_finish of the k items of paths_items —
// every item's verdict in paths.ok, its line's point count in paths.cnt, and a line item per
// verified finish (its optimize chain) in cf.items
int paths_batch_finish(pp_ctx* c, int k);
int paths_write(pp_ctx* c, const SceneDev& sd, PathsArgs a, const CfLines& lines,
                const int* items, int k, bool star, double* x, double* y, int64_t total,
                double* len_host = nullptr);
// The two host halves of a revalidation around its launches (pp_revalidate.cpp), shared with
// pp_repair.cpp and pp_prune.cpp.  reval_setup: the buffers (the steer slice's for at least
// min_tasks tasks; min_tasks < 0: no steer slice and no literal pool, pp_star_prune's verdicts
// need neither), the offsets and blocked roots on the device, the kernel arguments and the
// doubling passes, for Q trees of hn[q] nodes in the rows tr (tree q at q * cap).  reval_finish:
// the kept nodes over all trees, new_index (may be null) and the error word after one
// synchronisation; PP_ERR_STEER_OVERFLOW when a steer overflowed (the trees are unmodified).
int reval_setup(pp_ctx* c, const TreeDev& tr, int Q, size_t cap, const std::vector<int>& hn,
                const uint8_t* blocked, int* d_n, bool any_order, double* cost, double* elen,
                int min_tasks, RevalArgs* a, int* passes);
int reval_finish(pp_ctx* c, const RevalArgs& a, int64_t* kept, int32_t* new_index);

}  // namespace ppamd

// pp_kernels.h — host-side launch wrappers of the HIP kernels, the one header of them that the
// host side includes.  Every section names the unit that implements it.
#pragma once

#include <hip/hip_runtime.h>

#include "pp_types.h"

namespace ppamd {

// The window pipeline (pp_k_window.hip).
// Everything one window (or one nearest-neighbour batch) touches.  Buffers are sized for K.
struct WindowArgs {
    int K = 0;           // samples per window
    int Kcap = 0;        // buffer capacity per window (parity stride of wsx / wsy)
    int64_t target = 0;  // iteration the enqueued windows stop at
    uint64_t seed = 0;
    double eps_coord = 0.0;
    DevState* st = nullptr;
    SceneDev sc{};
    TreeDev tr{};
    double* wsx = nullptr;        // [2 * Kcap] samples, double-buffered by window parity
    double* wsy = nullptr;
    float* wsx32 = nullptr;       // [2 * Kcap] their f32 copies
    float* wsy32 = nullptr;
    int* perm = nullptr;          // [2 * Kcap] spatially sorted sample order (window_samples)
    int* cofs = nullptr;          // [2 * 257] start of each Morton cell in the sorted order
    float2* sxy = nullptr;        // [2 * Kcap] the samples in sorted order (f32)
    double* sq = nullptr;         // [2 * Kcap] |q - o|^2 about the screen block's centre
    double* ssx = nullptr;        // [2 * Kcap] the samples in sorted order (f64)
    double* ssy = nullptr;
    float2* ob = nullptr;         // [2 * kMaxWindow / 512] the screen blocks' centres
    int* ipos = nullptr;          // [2 * Kcap] sample -> sorted position
    float* pbest = nullptr;
    float* psecond = nullptr;
    int* pidx = nullptr;
    int* nn_idx = nullptr;
    double* nn_d2 = nullptr;
    int* cand_cnt = nullptr;
    CandEntry* cand = nullptr;
    int* snap_status = nullptr;
    double* snap_yaw = nullptr;
    double* snap_pose = nullptr;  // [3K] parent pose of each unflagged sample (nn_finalize)
    PrepRec* rec = nullptr;       // [K + K * kCandCap] per-task steer records
    int* pend = nullptr;          // [K] samples queued for the resolve's round passes
    int* fin_par = nullptr;       // [K] window parent of a resolved sample (kWinParent)
    ResolveScratch rs{};
    double* lit_scratch = nullptr;
    long long* wg_points = nullptr;  // profiling: walked points per walk workgroup (or null)
    const SceneDev* scp = nullptr;  // the scene in device memory (samples_role's point_blocked)
    int* iter_off = nullptr;        // [2 * Kcap] sample -> its iteration's offset in the window
    int pretest = 0;                // draws in an obstacle are settled where they are drawn
    // caller-drawn samples (pp_rrt_extend_samples): iteration it's sample is (hsx, hsy)[it -
    // hrec.base] instead of the seeded stream (null: the stream); hrec: the per-iteration record
    const double* hsx = nullptr;
    const double* hsy = nullptr;
    SampleRec hrec{0, nullptr, nullptr, nullptr};
};

// Enqueue window number `seq` on stream s: its window kernel also resolves and commits window
// seq - 1 when resolve_prev (the previous window of the same batch).  ev (optional) = 5 timing
// events: before the window kernel, then after it, nn_finalize, steer_prep and steer_walk.
hipError_t launch_window(hipStream_t s, const WindowArgs& a, hipEvent_t* ev, int64_t seq,
                         int resolve_prev);
// PP_FIN_STAMPS diagnostic builds: nn_finalize's wall-clock phase stamps per workgroup
constexpr int kFinStampSlots = 10, kFinStampWGs = 512;
#ifdef PP_FIN_STAMPS
hipError_t fin_stamps_copy(unsigned long long* out, size_t n);
#endif

// Resolve and commit the last enqueued window (seq_next - 1): ends a batch.
hipError_t launch_drain(hipStream_t s, const WindowArgs& a, int64_t seq_next);

// Exact nearest tree node of Wp[0] samples (wsx, wsy parity 0; nsp[0] = n): screen + finalize +
// rescan.
hipError_t launch_nearest(hipStream_t s, const WindowArgs& a);

// The API kernels (pp_k_steer.hip).
// Space::verify (rrt.rs:124-137) of k polylines, line i = points [off[i], off[i + 1]) of X/Y;
// ok[i] = 1 when it verifies.
hipError_t launch_verify_lines(hipStream_t st, const SceneDev& sc, const double* X,
                               const double* Y, const int64_t* off, int k, uint8_t* ok);

hipError_t launch_steer_tasks(hipStream_t st, const SceneDev& sc, const TreeDev& tr,
                              const SteerTask* tasks, int n, int* out_status, double* out_yaw,
                              double* scratch);

// check_finish, the packed line export and the batch plan's rounds (pp_k_finish.hip).
// RRT::check_finish for k tree nodes (one wave per node, at most `grid` workgroups of kCfWaves
// waves; gpath: grid * kCfWaves * kCfMaxDepth ints, the waves' ancestor paths).  ok/len/npts per
// node; chain (optional) = k rows of [levels, edges, optimize's chosen ancestors...] with
// kCfLevels + 2 ints per row; want_line: materialise the lines of the verified finishes (length;
// points of line item i in workgroup i's pts/etab, items: 1 + k * kCfItem ints, items[0] zeroed
// before the launch).  err |= 1 depth > kCfMaxDepth, 2 finalize panic, 4 steer overflow, 8 point
// capacity.  tally (profiling, optional): += nodes, edges steered + verified, polyline points
// walked.
// check_finish_kernel modes: check_finish (rrt.rs:428-438), optimize alone (rrt.rs:463-487),
// finalize of a caller-built goal node (rrt.rs:489-540)
enum : int { kCfCheck = 0, kCfOptimize = 1, kCfFinalize = 2 };
// check_finish over a query batch (pp_batch_plan): item b = node nodes[b] of query qidx[b]
struct CfBatch {
    const int* qidx = nullptr;  // null: the one-tree planner
    int row_cap = 0;            // SoA rows per query
    const double* goals = nullptr;   // [3Q] goal x, y, yaw
    const uint8_t* blocked = nullptr;  // [Q] polygon mode: the root fails verify (may be null)
    // optimize's memo (rows as the tree's SoA: query q at q * row_cap; zeroed per launch, may be
    // null): ftab[v] = 0 unknown, 1 no candidate of v verifies, 2 + m (| 1 << 30 when that edge's
    // steer is None) — v's first verifying candidate root first is its depth-m ancestor; gtab[v] =
    // 0 unknown, else 1 + the verdict of finalize's copy edge from v (see check_finish_kernel)
    int* ftab = nullptr;
    int* gtab = nullptr;
    // the batch plan's goal-edge verdicts per item (0 unknown, else 1 + verdict; may be null)
    const int* gotab = nullptr;
    // compact memo rows (may be null: q * row_cap): query q's nodes at moff[q] + q, moff = the
    // exclusive scan of the queries' items (n_q - 1)
    const int* moff = nullptr;
};

// check_finish of a query batch in steer rounds (pp_batch_plan, see pp_k_finish.hip): phase A
// fills ftab for every node, phase B the goal edges (gotab) and copy edges (gtab), the assemble
// kernel decides every item whose verdicts are all known and lists the others (plist, pcount)
// for check_finish_kernel.  Node b < nitems is item b, b - nitems < Q query's root.
constexpr int kCfbSpan = 2;  // phase A candidates per node and round (span A/B: DESIGN §3.3)
struct CfbArgs {
    TreeDev tr{};
    int row_cap = 0;
    int span = kCfbSpan;  // phase A candidates per node in the current round
    int nitems = 0, Q = 0;
    const int* qidx = nullptr;
    const int* nodes = nullptr;
    const double* goals = nullptr;
    const int* moff = nullptr;  // compact memo rows: query q's nodes at moff[q] + q
    int* ftab = nullptr;      // rows (the memo of CfBatch)
    int* gtab = nullptr;      // rows
    int* gotab = nullptr;     // [nitems]
    int* gclaim = nullptr;    // rows: copy edge claimed for phase B
    unsigned char* tnone = nullptr;     // rows: the node's own tree edge has a None steer
    unsigned char* tnone_up = nullptr;  // rows: any tree edge from the node down to the root has one
    int* depth = nullptr;     // [nitems + Q]
    int* open = nullptr;      // [nitems + Q] phase A: not settled yet
    int* tfirst = nullptr;    // [nitems + Q] the round's first task of the node
    int* tcnt = nullptr;      // [nitems + Q] ... and its count
    int* tnode = nullptr;     // [tasks] phase A: node b; phase B: item b, or -1 - row (copy edge)
    SteerTask* tasks = nullptr;
    StarTaskExt* ext = nullptr;
    PrepRec* rec = nullptr;   // (one chunk of the round's tasks at a time: launch_cfb_chunk)
    unsigned char* none = nullptr;  // per task: its steer was None (the record's kPrepNone)
    int* status = nullptr;
    double* yaw = nullptr;
    DevState* st = nullptr;   // st->W: the round's task count (ncomp 0)
    int* maxdepth = nullptr;
    int* pcount = nullptr;
    int* wsum = nullptr;      // (profiling) += every round's task count
    int* dhist = nullptr;     // [kCfbDepthBins] nodes per depth (the last bin: that depth or more)
};
constexpr int kCfbDepthBins = 64;
enum : int { kCfbDepth = 0, kCfbEmitA, kCfbConsumeA, kCfbEmitB, kCfbStoreB, kCfbAssemble };
hipError_t launch_cfb(hipStream_t s, const SceneDev& sc, CfbArgs a, int phase, int round,
                      int* ok = nullptr, double* len = nullptr, int* npts = nullptr,
                      int* err = nullptr, int* items = nullptr, int* plist = nullptr);
hipError_t launch_cfb_steer(hipStream_t s, const SceneDev& sc, const CfbArgs& a, int max_tasks,
                            bool own_yaw, long long* wg_points = nullptr);
// a chunk of a round's steer: begin (the chunk's task count from the round's) or, after its walk,
// the None flags of its records into none[0, chunk->W)
hipError_t launch_cfb_chunk(hipStream_t s, const DevState* all, DevState* chunk, int base,
                            int cap, bool begin, const PrepRec* rec, unsigned char* none);
// the rounds' literal-path tasks re-run by steer_collide_literal (a scratch slot per wave)
hipError_t launch_cfb_literal(hipStream_t s, const SceneDev& sc, const CfbArgs& a, int max_tasks,
                              int* list, int* count, double* lit_scratch);
// cf_line_kernel's per-workgroup buffers: pts (3 x pts_cap doubles: x, y, hypots / words), etab
// (2 x (path_cap + kCfLevels + 1) ints) and path (path_cap ints) per workgroup.  spill != null
// (tier 1): a line deeper than path_cap or longer than pts_cap is appended to spill (the items
// layout, spill[0] its count, zeroed before the launch) instead of failing, and tier 2 — the full
// capacities (kCfMaxDepth, kCfPtsCap) on a few workgroups — runs the spill list
struct CfLineBufs {
    double* pts = nullptr;
    int pts_cap = 0;
    int* etab = nullptr;
    int* path = nullptr;
    int path_cap = kCfMaxDepth;
    int* spill = nullptr;
    int spill_cap = 0;
};
struct CfLines {
    int grid1 = 0;  // 0: no line kernel
    CfLineBufs t1;
    int grid2 = 0;  // tier 2 (when t1.spill)
    CfLineBufs t2;
};
hipError_t launch_check_finish(hipStream_t st, const SceneDev& sc, const SceneDev* scg,
                               const TreeDev& tr,
                               const int* nodes, int k, double gx, double gy, double gyaw,
                               double gyaw_opt, int level0, int mode, int want_line, int* ok,
                               double* len, int* npts, int* chain, double* lit_scratch,
                               int* lit_locks, const CfLines& lines, int* err, int grid,
                               long long* tally, const CfBatch& cb, int* gpath, int* items,
                               const int* blist = nullptr);
constexpr int kCfWaves = 4;                     // check_finish: waves (nodes in flight) per workgroup
constexpr int kCfItem = 4 + kCfLevels;          // a line item: b, s, verified, 0, pos[kCfLevels]

// Packed line export (pp_batch_paths / pp_star_paths, pp_k_finish.hip): the lines of the line
// items (the layout
// above; item b = node nodes[b] of query qidx[b] of a forest) into one CSR buffer, every row root
// side first.  star = false: finalize's chain of a check_finish item (s, pos[] from the item;
// always the write pass — check_finish's own line pass counted); star = true: pp_star_path's chain
// goal -> node -> parent -> ... -> root, whose count pass (write = false) fills cnt[b] and okf[b]
// (0: the goal edge has no word).  The write pass stores row q = [off[q], off[q + 1]) of ox / oy
// and (len != null) the row's euclidean_length in len[b].  err bits as check_finish's, and 16: a
// row's size differs from the count pass (nothing is stored).  lines: cf_line_kernel's buffers
// and tiers, the spill count zeroed before every call; items holds at most k items.
struct PathsArgs {
    TreeDev tr{};
    int row_cap = 0;
    const int* qidx = nullptr;
    const int* nodes = nullptr;
    const double* goals = nullptr;  // [3Q] (gx, gy, gyaw)
    const int64_t* off = nullptr;   // [Q + 1]
    double* ox = nullptr;
    double* oy = nullptr;
    int* cnt = nullptr;
    int* okf = nullptr;
    double* len = nullptr;
};
hipError_t launch_paths(hipStream_t st, const SceneDev& sc, const PathsArgs& a,
                        const CfLines& lines, int* err, const int* items, int k, bool star,
                        bool write);
// off[0 .. Q] = the exclusive scan of the queries' point counts (cnt[slot[q]] where slot[q] >= 0
// and okf[slot[q]], else 0), okq[q] that flag
hipError_t launch_paths_scan(hipStream_t st, int Q, const int* slot, const int* okf,
                             const int* cnt, int64_t* off, uint8_t* okq);

// Segment export (pp_star_path_segments / pp_batch_path_segments, pp_k_segments.hip; DESIGN.md
// §3.7 "Segment export and sampling"): the chains of the same line items as arc / straight / arc
// records, three per Dubins edge, packed.  The count pass (write = false) stores cnt[b] = 3 E
// (star: and okf[b], 0 with cnt 0 when the goal edge has no word); the write pass stores row q =
// [off[q], off[q + 1]) of the five arrays (a null one is skipped), generation order or, reverse,
// the same curve from the root.  One wave per item with a path_cap-deep ancestor path each (path:
// grid x path_cap ints); spill != null: a deeper chain is appended to spill (the items layout,
// spill[0] zeroed before the launch) for a launch at the full depth.  err bits as check_finish's
// (1 depth, 2 an edge without a word) and 16: a row's size differs from the count pass.
struct SegArgs {
    TreeDev tr{};
    int row_cap = 0;
    const int* qidx = nullptr;
    const int* nodes = nullptr;
    const double* goals = nullptr;  // [3Q] (gx, gy, gyaw)
    double turn_radius = 1.0;
    int reverse = 0;
    const int64_t* off = nullptr;   // [Q + 1]
    double* ox = nullptr;
    double* oy = nullptr;
    double* oyaw = nullptr;
    double* okappa = nullptr;
    double* olen = nullptr;
    int* cnt = nullptr;
    int* okf = nullptr;
    int* path = nullptr;
    int path_cap = 0;
    int* spill = nullptr;
    int spill_cap = 0;
    // caller-supplied chains (pp_star_chain_segments; star only): query q's chain is cchain[coff[q]
    // .. coff[q + 1]), the node after the goal first and the root last; no ancestor path is walked
    const int* cchain = nullptr;
    const int64_t* coff = nullptr;
};
hipError_t launch_segments(hipStream_t st, const SegArgs& a, int grid, int* err, const int* items,
                           int items_cap, bool star, bool write);
// The sampler (pp_segments_sample, pp_k_segments.hip).  Prefix: per row r = segments
// [off[r], off[r + 1]) the running arc position P[j] = len[off[r]] + ... + len[j] added in row order, the row's length
// rowlen[r], nfull[r] = floor(rowlen / ds) (clamped to max_samples) and its sample count cnt[r]
// (nfull + 1, one more when rowlen > nfull * ds; 0 for a row without segments).  Sample: output i
// of row r (poff[r] <= i < poff[r + 1]) at s = k ds (k = i - poff[r] <= nfull[r]) or rowlen[r],
// on the first segment with s < P[j] or the last at its end; a null output is skipped.
struct SegSampleArgs {
    int q = 0;
    double ds = 1.0;
    int64_t max_samples = 0;
    const int64_t* off = nullptr;
    const double* x = nullptr;
    const double* y = nullptr;
    const double* yaw = nullptr;
    const double* kappa = nullptr;
    const double* len = nullptr;
    double* P = nullptr;
    double* rowlen = nullptr;
    int64_t* nfull = nullptr;
    int64_t* cnt = nullptr;
    const int64_t* poff = nullptr;  // [q + 1]
    int64_t total = 0;              // poff[q]
    double* sx = nullptr;
    double* sy = nullptr;
    double* syaw = nullptr;
    double* skappa = nullptr;
    double* ss = nullptr;
};
hipError_t launch_segments_prefix(hipStream_t st, const SegSampleArgs& a);
hipError_t launch_segments_sample(hipStream_t st, const SegSampleArgs& a);

// pp_batch_plan (pp_k_finish.hip): the (query, node) items of the accepted nodes (off: [Q + 1]
// exclusive scan of n_q - 1), and per query the first minimum length over its items'
// check_finish results
hipError_t launch_mq_plan_items(hipStream_t s, int Q, const int* off, int* qidx, int* nodes);
hipError_t launch_mq_plan_reduce(hipStream_t s, int Q, const int* off, const int* ok,
                                 const double* len, const int* npts, int* best_node,
                                 double* best_len, int* best_npts, int* n_fin);

// Multi-query batch (pp_k_batch.hip): `steps` lockstep extend iterations of every query
// (config 3).
struct MqArgs {
    MqDev mq{};
    SceneDev sc{};
    DevState* st = nullptr;  // W = Q, ncomp = 0 (the steer kernels' task count)
    SteerTask* tasks = nullptr;
    PrepRec* rec = nullptr;
    int* status = nullptr;
    double* yaw = nullptr;
    double* lit_scratch = nullptr;  // kLiteralWaves buffers
    int* lit_locks = nullptr;       // their slot locks (0 free)
    int* err = nullptr;
    hipEvent_t* ev = nullptr;  // optional: 5 per step: before mq_sample_nn, then after it, steer_prep,
                               // steer_walk and mq_insert
    long long* wg_points = nullptr;  // profiling: walked points per walk workgroup (or null)
    const SceneDev* scp = nullptr;   // the scene in device memory: point_blocked (or null: none)
};
hipError_t launch_mq_steps(hipStream_t s, const MqArgs& a, int steps);
hipError_t launch_mq_init(hipStream_t s, const MqDev& mq, const double* starts);
// the per-query iteration targets of a pp_batch_extend(n_steps) call
hipError_t launch_mq_target(hipStream_t s, const MqDev& mq, int64_t n_steps, int64_t* target);

// RRT* query batch (config 5, pp_k_star.hip): `steps` lockstep RRT* iterations of every query.
// Task arrays of round A hold Q entries, rounds B and C Q * kStarKMax; rec is shared by the rounds.
struct StarArgs {
    StarDev sd{};
    SceneDev sc{};
    SteerTask *tA = nullptr, *tB = nullptr, *tC = nullptr;
    StarTaskExt *eB = nullptr, *eC = nullptr;  // rounds B / C: cull limits, rewire child poses
    int *sA = nullptr, *sB = nullptr, *sC = nullptr;        // verdicts
    double *yA = nullptr, *yB = nullptr, *yC = nullptr;     // child yaw of each task
    double *cA = nullptr, *cB = nullptr, *cC = nullptr;     // Dubins cost of each task
    PrepRec* rec = nullptr;
    double* lit_scratch = nullptr;  // kLiteralWaves buffers
    int* err = nullptr;
    hipEvent_t* ev = nullptr;  // optional: 8 per step, around star_sample and each round's walk
    long long* wg_points = nullptr;  // profiling: walked points per walk workgroup (or null)
};
hipError_t launch_star_steps(hipStream_t s, const StarArgs& a, int steps);
hipError_t launch_star_init(hipStream_t s, const StarArgs& a, const double* starts);

// RRT* goal connection (pp_star_plan / pp_star_goal_costs, pp_k_star.hip): `rounds` rounds of 63
// nodes per query over the queries [q0, q1) of the batch `a` views, which lends round B's task arrays, the records
// and stB->W.  Per query: best (+inf none) and best_node (-1 none), the first strict minimum of
// cost(m) + the goal edge's Dubins cost over the feasible nodes.
struct StarGoalArgs {
    StarArgs a;
    int q0 = 0, q1 = 0;
    const double* goals = nullptr;  // [3 * queries of the batch] (gx, gy, gyaw)
    int* gslot = nullptr;           // [queries] first task of the query in the current round
    uint64_t* gmask = nullptr;      // [queries] lanes (nodes of the slice) with a task
    double* best = nullptr;         // [queries] the running best
    int* best_node = nullptr;
    long long* steered = nullptr;   // the tasks emitted over all rounds (the cull's effect)
    int prune = 1;                  // 0: every node gets a task and no cull limit (the un-pruned costs)
    double* total = nullptr;        // q1 == q0 + 1: total[m] of that query's nodes (or null)
};
hipError_t launch_star_goal(hipStream_t s, const StarGoalArgs& g, int rounds);

// Shortcuts along the chain (pp_star_shortcut / pp_star_shortcut_edges, pp_k_shortcut.hip;
// DESIGN.md §3.7 "Shortcuts along the chain").  Item b < k is (query qidx[b], node nodes[b]); its
// positions are c_0 = the goal, c_i = chain[b * stride + i - 1] for i = 1 .. D = depth[b] (c_1 the
// node, c_D the root).  Row i < D of its band holds sp = min(span, D) entries, entry l the edge
// c_i -> c_{i + 1 + l} (entries with i + 1 + l > D are never written or read); its pairs, row by
// row and l < min(span, D - i), are numbered pbase[b] .. pbase[b + 1] - 1 over the call, and a
// steer round serves a run of these numbers in the batch `a`'s round-B task arrays (as the goal
// rounds borrow them: StarGoalArgs).
struct ShortcutArgs {
    StarArgs a;
    int k = 0;
    int span = 1;
    const int* qidx = nullptr;      // [k]
    const int* nodes = nullptr;     // [k]
    const double* goals = nullptr;  // [3 * queries of the batch] (gx, gy, gyaw)
    int stride = 0;                 // chain / next entries per item
    int* chain = nullptr;           // [k * stride]; after the DP: the shortened path's nodes
    int* next = nullptr;            // [k * stride] the DP's next[i], i < D
    int* depth = nullptr;           // [k] D; 0: deeper than stride (err |= 1)
    int64_t* npair = nullptr;       // [k] the item's pairs
    const int64_t* pbase = nullptr; // [k + 1] exclusive scan of npair
    const int64_t* boff = nullptr;  // [k + 1] exclusive scan of D * min(span, D): the bands
    double* band = nullptr;         // w(i, j) or +inf
    int64_t* tdst = nullptr;        // [round's tasks] the band entry of each task
    double* cost = nullptr;         // [k] best[0]
    int* plen = nullptr;            // [k] nodes of the shortened path (0: no route)
    int* err = nullptr;             // |= 1 chain deeper than stride, 4 steer overflow
    int* res = nullptr;             // [3 * k] pp_star_shortcut_commit: the goal's node (-1 none), the
                                    // rewires reported, the costs changed (cost: the goal's cost)
};
// D and the pair count of every item, its chain into a.chain
hipError_t launch_shortcut_chain(hipStream_t s, const ShortcutArgs& a);
// one steer round: the pairs [g0, g0 + cnt), cnt <= the batch's round-B capacity — emit, prep,
// walk, settle (the band entries).  ev (profiling, optional): 4 events, after each of the four.
hipError_t launch_shortcut_round(hipStream_t s, const ShortcutArgs& a, int64_t g0, int cnt,
                                 hipEvent_t* ev = nullptr);
// the DP of every item over its band, then its path (a.chain compacted in place, plen, cost)
hipError_t launch_shortcut_dp(hipStream_t s, const ShortcutArgs& a);
// pp_star_shortcut_commit, after the rounds in place of the DP: the tree-anchored DP of every item,
// its rewires written into the tree (parent, elen, cost), the subtrees' costs recomputed (mark /
// stamp as star_rewire leaves them), rewires[q] advanced; a.res and a.cost.  Writes nothing when
// *a.err is set by the rounds.
hipError_t launch_shortcut_commit(hipStream_t s, const ShortcutArgs& a);
// out[off[q] + e] = the e-th node of query q's shortened path (slot[q] its item or -1; off[Q] =
// total, the device's copy of the host's scan of plen)
hipError_t launch_shortcut_pack(hipStream_t s, const ShortcutArgs& a, int Q, const int* slot,
                                const int64_t* off, int64_t total, int* out);

// Revalidation (pp_rrt_revalidate / pp_batch_revalidate / pp_star_revalidate,
// pp_k_revalidate.hip): re-verify every node's edge against the scene, propagate failures to the
// descendants and compact the trees in place.  `total` nodes in Q trees: tree q's nodes are g = off[q] .. off[q + 1] - 1, node i of it
// in row q * cap + i of tr (x32 / y32 null: a forest without screen copies).
struct RevalArgs {
    TreeDev tr{};
    int Q = 1;
    size_t cap = 0;
    const int* off = nullptr;          // [Q + 1] exclusive scan of the trees' node counts
    int total = 0;                     // off[Q]
    const uint8_t* blocked = nullptr;  // [Q] the root fails verify (polygon mode; may be null)
    int* n = nullptr;                  // [Q] the trees' node counts, rewritten (may be null)
    // RRT* (pp_star_revalidate): a node's parent is any other node of its tree (a rewired node
    // hangs under a later one), and a chain that does not end in the tree's root is dropped
    int any_order = 0;
    double* cost = nullptr;  // RRT*'s per-row arrays, carried with the rows (null: none)
    double* elen = nullptr;
    // one slice of steer tasks at a time
    int slice = 0;
    SteerTask* tasks = nullptr;
    StarTaskExt* ext = nullptr;
    PrepRec* rec = nullptr;
    int* status = nullptr;
    double* yaw = nullptr;
    DevState* st = nullptr;
    unsigned* v[2] = {nullptr, nullptr};  // [total] ping-pong: ancestor | bad << 31
    int* bsum = nullptr;       // [ceil(total / 1024)] scan workgroup counts
    int* pos = nullptr;        // [total + 1] exclusive scan of keep; pos[total]: the kept nodes
    int* new_index = nullptr;  // [total] index in its tree after the call, -1 dropped
    double* sx = nullptr;      // [total] and below: the kept rows, staged compactly
    double* sy = nullptr;
    double* syaw = nullptr;
    int* spar = nullptr;
    double* scost = nullptr;  // (cost != null)
    double* selen = nullptr;
    long long* srow = nullptr;  // ... and the row each goes back to
    int* err = nullptr;         // != 0: a steer overflowed n_point; the trees are left as they are
    double* lit_scratch = nullptr;  // kLiteralWaves buffers
    int* lit_locks = nullptr;
    long long* wg_points = nullptr;  // profiling: walked points per walk workgroup (or null)
};
// passes: ceil(log2(the largest tree's node count)) pointer-doubling passes
hipError_t launch_revalidate(hipStream_t s, const SceneDev& sc, const RevalArgs& a, int passes);
// ... and its three stages (launch_revalidate runs them in this order): the edge test of every
// node into a.v[0], the doubling into a.v[passes & 1], and the compaction of the nodes whose word
// in v keeps them (rv_keep)
hipError_t launch_reval_edges(hipStream_t s, const SceneDev& sc, const RevalArgs& a);
hipError_t launch_reval_jump(hipStream_t s, const RevalArgs& a, int passes);
hipError_t launch_reval_compact(hipStream_t s, const RevalArgs& a, const unsigned* v);
// ... and the compaction's two ends around its gather, for a caller with a gather of its own
// (pp_star_advance): the exclusive scan of rv_keep(v, g, koff, Q) into a.pos, and the staged rows
// back into the trees with the new sizes
hipError_t launch_reval_scan(hipStream_t s, const RevalArgs& a, const unsigned* v, const int* koff);
hipError_t launch_reval_write(hipStream_t s, const RevalArgs& a);

// Repair (pp_star_repair, pp_k_repair.hip): between the jump and the compaction
// of an RRT* forest's revalidation, dropped subtrees are hung under kept nodes again, in rounds.
// All per-node arrays are indexed by the global node g of RevalArgs.
constexpr int kRepairMaxRounds = 16;
constexpr int kRepairTopsPerSlice = 512;  // <= 512 * kStarKMax tasks a steer slice
enum : unsigned char { kTopNever = 0, kTopNow = 1, kTopAttached = 2, kTopFailed = 3 };
struct RepairRec {  // the counters the host reads
    int ntops[kRepairMaxRounds + 1];  // [r]: the tops of round r
    long long reattached, recovered;
};
struct RepairArgs {
    RevalArgs rv;  // the forest, its offsets, the steer slice's buffers (>= kRepairTopsPerSlice *
                   // kStarKMax tasks), the literal pool and the error word
    const int* ksched = nullptr;     // [cap + 1] star_k of the batch over the kept count
    const unsigned* vedge = nullptr; // [total] the settle's words: bad = the node's own edge fails
    const unsigned* vkeep = nullptr; // [total] the words after the jump: K0 by rv_keep
    unsigned* vout = nullptr;        // [total] the words the compaction keeps by (repair_commit)
    unsigned char* flag = nullptr;   // [total] bit 0: kept, bit 1: kept by the repair
    unsigned char* top = nullptr;    // [total] kTopNever .. kTopFailed
    int* lvl = nullptr;              // [total] the round's levels: 1 a re-attached top, d + 1 its
                                     // descendants at depth d (zeroed before every round)
    int* wpar = nullptr;             // [total] parent (index in its tree), staged
    double* wcost = nullptr;         // [total] cost, staged
    double* welen = nullptr;         // [total] elen, staged
    double* tcost = nullptr;         // [slice tasks] the Dubins cost of each task
    int* tops = nullptr;             // [total] the round's tops, packed
    int* near = nullptr;             // [round's tops * kStarKMax] a top's candidates in (d2, index) order
    int* tcnt = nullptr;             // [round's tops] ... and their count
    int* tslot = nullptr;            // [kRepairTopsPerSlice] first task of a slice's top
    unsigned char* qhas = nullptr;   // [Q] the query re-attached a top this round (zeroed per round)
    RepairRec* rec = nullptr;
};
enum : int { kRepairInit = 0, kRepairTops, kRepairGrow, kRepairCommit };
// one stage over all nodes: init (the staged copies, K0), tops (mark and pack round `round`'s
// tops, count them in rec->ntops[round]), grow (keep the subtrees under the re-attached tops
// again, their costs level by level) and commit (the staged rows into the trees unless a steer
// overflowed, the keep words into vout)
hipError_t launch_repair_stage(hipStream_t s, const RepairArgs& a, int stage, int round);
// the candidates of all `ntops` packed tops of the round: the kNN among the kept nodes, one wave
// per top in one launch
hipError_t launch_repair_knn(hipStream_t s, const RepairArgs& a, int ntops);
// the steer round of the packed tops [t0, t1), t1 - t0 <= kRepairTopsPerSlice: their tasks, prep,
// walk, choose
hipError_t launch_repair_slice(hipStream_t s, const SceneDev& sc, const RepairArgs& a, int t0,
                               int t1);

// Advance (pp_star_advance, pp_k_advance.hip; DESIGN.md §3.8 "Advancing the root"): node root[q]
// of tree q becomes its root.  The repair's staged arrays (rp) hold the kept core and its rebuilt
// costs; the repair's own rounds then run on them with the old root's chain as round 1's tops, and
// a gather of this unit puts the new root first.  Nothing is written into the trees before
// launch_reval_write.
struct AdvanceArgs {
    RepairArgs rp;
    const int* nodes = nullptr;  // [Q] the caller's nodes, -1: the query stays
    const int* hops = nullptr;   // [Q] edges from the root along the chain to nodes[q] (null: all)
    int* root = nullptr;         // [Q] the new root's index before the call, 0: the query stays
    double* starts = nullptr;    // [3Q] the stored roots (Forest::d_starts)
};
enum : int { kAdvanceCore = 0, kAdvanceTops, kAdvanceKeep, kAdvanceGather, kAdvanceStarts };
// one stage: core (the walk to root[q], the keep words of its subtree through the doubling of
// `passes` passes, the staged copies and the costs rebuilt level by level from the new root),
// tops (round 1's: the proper ancestors of root[q], counted in rec->ntops[1]), keep (the words
// launch_reval_scan(koff = null) keeps by, into rp.vout), gather (the kept rows staged with the
// new root first) and starts (row 0 into the stored start of every advanced query, unless a
// steer overflowed)
hipError_t launch_advance_stage(hipStream_t s, const AdvanceArgs& a, int stage, int passes);

// Relax (pp_star_relax, pp_k_relax.hip; DESIGN.md §3.8 "Relaxing the trees"): every node of an
// RRT* forest looks for a cheaper parent among the nodes of its own tree, in synchronous rounds.
// Node g of the `total` nodes is node g - off[q] of tree q, as in RevalArgs; arrays marked [total]
// are indexed by g.  Nothing is sized by nodes x candidates: a slice of nodes packs its steer tasks
// straight from the kNN.
constexpr int kRelaxMaxRounds = 16;
constexpr int kRelaxNodesPerSlice = 16384;  // <= 16384 * star_k tasks a steer slice
struct RelaxRec {  // the counters the host reads
    int rewired;        // re-parentings so far, all rounds
    int pad;
    long long changed;  // nodes whose cost differs from before the call
    // profiling only (RelaxArgs::stats): candidates of the live nodes, those left after the parent
    // skip, after the cost skip, after the chord bound (the steer tasks), and the tasks walked
    long long cand, not_parent, cheaper, tasks, walked;
};
struct RelaxArgs {
    TreeDev tr{};
    int Q = 0;
    size_t cap = 0;
    const int* off = nullptr;          // [Q + 1] exclusive scan of the trees' node counts
    int total = 0;                     // off[Q]
    const uint8_t* blocked = nullptr;  // [Q] the root fails verify: the query stays (may be null)
    const uint8_t* active = nullptr;   // [Q] 0: the query stays (null: every query takes part)
    double* cost = nullptr;            // the batch's rows
    double* elen = nullptr;
    int64_t* rewires = nullptr;        // [Q] the batch's rewire counters
    const int* ksched = nullptr;       // [cap + 1] star_k of the batch
    double curv = 0.0;                 // 1 / turn radius: the chord lower bound of a Dubins cost
    int kmax = 0;                      // the most candidates a node of this forest has
    // one slice of steer tasks at a time
    int task_cap = 0;                  // >= the largest slice's nodes * kmax
    SteerTask* tasks = nullptr;
    StarTaskExt* ext = nullptr;
    PrepRec* rec = nullptr;
    int* status = nullptr;
    double* yaw = nullptr;
    double* tcost = nullptr;           // the Dubins cost of each task
    DevState* st = nullptr;
    int* tslot = nullptr;              // [kRelaxNodesPerSlice] first task of a slice's node
    int* tcnt = nullptr;               // [kRelaxNodesPerSlice] ... and their count
    int* wpar = nullptr;               // [total] the round's staged parent, -1: the node stays
    double* welen = nullptr;           // [total] ... and its edge cost
    int* lvl = nullptr;                // [total] the commit's levels
    unsigned char* chg = nullptr;      // [total] the node's cost moved in this call
    int* nrw = nullptr;                // [Q] the call's re-parentings per query
    RelaxRec* rrec = nullptr;
    int stats = 0;                     // collect rrec's profiling counters
    int* err = nullptr;                // != 0: a steer overflowed n_point; the round is not applied
    double* lit_scratch = nullptr;     // kLiteralWaves buffers
    int* lit_locks = nullptr;
    long long* wg_points = nullptr;    // profiling: walked points per walk workgroup (or null)
};
// the steer round of the nodes [g0, g1), g1 - g0 <= kRelaxNodesPerSlice: the self-join kNN with
// its culls and tasks, prep, walk, choose (the staged rows)
hipError_t launch_relax_slice(hipStream_t s, const SceneDev& sc, const RelaxArgs& a, int g0,
                              int g1);
// after a round's last slice: the staged rows into the trees unless a steer overflowed, the costs
// rebuilt from the root level by level, the counters
hipError_t launch_relax_commit(hipStream_t s, const RelaxArgs& a);

// Prune (pp_star_prune, pp_k_prune.hip; DESIGN.md §3.7 "Pruning by the focus bound"): the keep
// words of an RRT* forest by its queries' focus bounds, in front of launch_reval_jump and
// launch_reval_compact.  No steer: rv's slice buffers are unused.
struct PruneArgs {
    RevalArgs rv;                    // the forest (any_order, cost), its offsets, v[0]
    const double* fxy = nullptr;     // [2Q] the queries' focus points (StarArgs::fxy, whole batch)
    const double* fbound = nullptr;  // [Q] their bounds L, +inf: no focus
    double R = 0.0;                  // the scene's turn radius: cost * R is a length
    const int* keep = nullptr;       // [Q] the protected chain's first node, -1 none (null: none)
};
// the node test of every node into rv.v[0], then the protected chains
hipError_t launch_prune_verdicts(hipStream_t s, const PruneArgs& p);

// Forest export / import (pp_*_forest_export / pp_*_forest_import, pp_k_forest_io.hip; DESIGN.md
// §3.9): the complete state of the slots slots[0 .. m) of a forest, packed.  Staged row k of the
// packed arrays belongs to served slot i with off[i] <= k < off[i + 1] and is row slots[i] * cap +
// (k - off[i]) of the forest.  Null forest pointers: that array does not exist in this batch kind
// (cost .. stamp: RRT*; itprev: the extend batch) or is not wanted.
struct ForestIoArgs {
    TreeDev tr{};
    size_t cap = 0;
    int m = 0;
    const int* slots = nullptr;   // [m] distinct slots of the forest
    int64_t* off = nullptr;       // [m + 1] exclusive scan of the served trees' node counts
    int64_t total = 0;            // off[m] (the row kernels' bound)
    // the forest: per row ...
    double* cost = nullptr;
    double* elen = nullptr;
    int* mark = nullptr;
    // ... and per slot
    int* n = nullptr;
    int64_t* it = nullptr;
    int64_t* evals = nullptr;
    uint64_t* seed = nullptr;
    int64_t* rew = nullptr;
    double* fxy = nullptr;
    double* fbound = nullptr;
    int64_t* skipped = nullptr;
    int* stamp = nullptr;
    double* starts = nullptr;     // [3Q] the stored roots (Forest::d_starts)
    uint8_t* blocked = nullptr;   // [Q] or null: no blocked roots in this forest
    int64_t* itprev = nullptr;
    // the staged rows [total] ...
    double* sx = nullptr;
    double* sy = nullptr;
    double* syaw = nullptr;
    int* spar = nullptr;
    double* scost = nullptr;            // export: the costs; import: the rebuilt costs
    double* selen = nullptr;
    const double* scost_in = nullptr;   // import: the caller's costs to check against (or null)
    int* lvl = nullptr;                 // import: the validation's levels (0: not reached)
    // ... and the staged per-slot values [m]
    int64_t* sit = nullptr;
    int64_t* sevals = nullptr;
    uint64_t* sseed = nullptr;
    int64_t* srew = nullptr;
    double* sfxy = nullptr;
    double* sfbound = nullptr;
    int64_t* sskipped = nullptr;
    const uint8_t* sblocked = nullptr;  // import: the new roots' blocked flags
    int ordered = 0;                    // import: parent[i] < i required (the extend batch)
    int* verdict = nullptr;             // [m] import: 0 or the first rule the tree breaks (kFio*)
};
enum : int { kFioOk = 0, kFioRoot = 1, kFioParent = 2, kFioOrder = 3, kFioUnreached = 4, kFioCost = 5 };
// off[0 .. m] from the served slots' node counts, and their per-slot values into the staged ones
hipError_t launch_forest_sizes(hipStream_t s, const ForestIoArgs& a);
// the served trees' rows into the staged arrays (a null staged array is skipped)
hipError_t launch_forest_gather(hipStream_t s, const ForestIoArgs& a);
// verdict[i] of every staged tree and, for RRT*, the rebuilt costs in scost; one wave per tree
hipError_t launch_forest_validate(hipStream_t s, const ForestIoArgs& a);
// the staged rows and per-slot values into the forest, and the slots' derived state
hipError_t launch_forest_scatter(hipStream_t s, const ForestIoArgs& a);

// The Dubins API kernels (pp_k_steer.hip).
// dubins_path_planning_from_origin for n (dx, dy, eyaw, c, step_size) configurations
hipError_t launch_dubins_origin(hipStream_t st, const double* conf, int n, int cap, double* px,
                                double* py, double* pyaw, int* n_out, int* word_out,
                                double* cost_out, int* status_out);
// the six Dubins words of n (alpha, beta, d) triples
hipError_t launch_dubins_words(hipStream_t st, const double* abd, int n, double* tpq, int* ok);
// sincos_small on the library's table and the math library's sincos of n arguments (|x| < 2^30)
hipError_t launch_sincos_small(hipStream_t st, const double* x, int n, double* s, double* c,
                               double* s_ocml, double* c_ocml);

hipError_t launch_dubins_batch(hipStream_t st, const double* conf, int n, int cap, double* px,
                               double* py, double* pyaw, int* n_out, int* word_out,
                               double* cost_out, int* status_out);

}  // namespace ppamd

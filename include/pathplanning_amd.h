/*
 * pathplanning_amd.h — C ABI of the MI355X-native RRT extend hot path.
 *
 * Drop-in boundary for tsturzl/rs-pathplanning's `rrt` / `dubins` public API (src/lib.rs:5-6):
 * a Rust host binds these symbols through a thin `extern "C"` block and keeps
 * its own types; everything here is plain pointers, sizes and status codes.
 *
 * Conventions
 *   - Every int-returning call returns PP_OK (0) or a negative PP_ERR_* code; no exception or
 *     panic crosses the boundary.  pp_last_error() gives the calling thread's last message.
 *   - The caller owns every host buffer; a context owns its device memory and HIP stream.
 *   - A context is not thread-safe: use one context per host thread (and per GPU).
 *   - Where the reference returns Option::None the ABI reports it in an output field
 *     (word = -1, idx = -1, ok = 0), not as an error.
 *   - The product path is HIP only: every compute call fails with PP_ERR_NO_DEVICE when no
 *     gfx950 device is present.  There is no CPU fallback.
 */
#ifndef PATHPLANNING_AMD_H
#define PATHPLANNING_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: pp_stats lost the diagnostic stamps and gained the batch / check_finish counters;
 *    pp_rrt_get_stats takes the caller's sizeof(pp_stats); pp_batch_plan added
 * 3: pp_batch_set_schedule, the persistent batch kernel; pp_stats appended its counters
 * 4: the persistent batch kernel and pp_batch_set_schedule removed (slower than the lockstep
 *    schedule on every workload measured: DESIGN.md §3.4); its pp_stats counters are reserved
 *    (always 0, the layout kept); pp_batch_set_finish_schedule replaces the library's former
 *    environment knobs
 * 5: pp_rrt_extend_samples and pp_rrt_tree_import (the host owns the RNG and the tree); nothing
 *    else changed
 * 5 (+): pp_star_plan / pp_star_goal_costs / pp_star_path added, nothing else changed
 * 5 (+): pp_batch_paths / pp_star_paths added, nothing else changed
 * 5 (+): pp_rrt_revalidate / pp_batch_revalidate added (a tree kept across a scene change),
 *    nothing else changed
 * 5 (+): pp_star_revalidate added (the RRT* batch's trees kept across a scene change), nothing
 *    else changed
 * 5 (+): pp_star_repair added (dropped subtrees re-attached under kept nodes after a scene
 *    change), nothing else changed
 * 5 (+): PP_COORD_MAX, pp_coord_check and pp_sincos_small_batch added; positions above
 *    PP_COORD_MAX are now PP_ERR_INVALID_ARGUMENT, nothing else changed
 * 5 (+): PP_STAR_FOCUS_DRAWS, pp_star_set_focus and pp_star_get_focus added (focused sampling of
 *    the RRT* batch); a batch that never sets a focus runs as before bit for bit
 * 5 (+): pp_star_prune added, nothing else changed
 * 5 (+): pp_forest_state, pp_star_forest_export / pp_star_forest_import and
 *        pp_batch_forest_export / pp_batch_forest_import added (the complete state of a set of
 *        query slots out of a batch and into one), nothing else changed
 * 5 (+): pp_path_segments, pp_star_path_segments / pp_batch_path_segments and
 *        pp_segments_sample added (planned paths as Dubins segments, sampled into
 *        trajectories), nothing else changed
 * 5 (+): pp_star_shortcut, pp_star_shortcut_edges and pp_star_chain_segments added (RRT* paths
 *        shortened by Dubins shortcuts along the chain), nothing else changed
 * 5 (+): pp_star_shortcut_commit added (the chain's shortcuts written back into the RRT* trees as
 *        rewires), nothing else changed
 * 5 (+): pp_star_advance added (a node of every RRT* tree becomes its root; what hung from its
 *        ancestors is re-attached by pp_star_repair's rounds), nothing else changed
 * 5 (+): pp_star_relax added, nothing else changed (every node of the RRT* trees looks for a
 *        cheaper parent in its own tree; pp_star_relax_counts reads its profiling counters) */
#define PP_ABI_VERSION 5

#define PP_OK 0
#define PP_ERR_INVALID_ARGUMENT (-1)
#define PP_ERR_HIP (-2)
#define PP_ERR_NO_DEVICE (-3)
#define PP_ERR_CAPACITY (-4)
#define PP_ERR_STATE (-5)          /* no scene / no planner configured yet */
#define PP_ERR_STEER_OVERFLOW (-6) /* generate_local_course would index past n_point (panic) */
#define PP_ERR_REFERENCE_PANIC (-7) /* finalize: an edge with no feasible Dubins word (panic) */

/* The largest |x| or |y| any entry point accepts for a position (bounds, discs, polygon and grid
 * corners, starts, goals, samples, tree nodes, query points, candidates, polyline vertices, Dubins
 * end points): 2^61.  The nearest-node screen works in f32 first, and this is the largest power of
 * two at which each of its intermediates stays finite: (float)q, the squared distance
 * (qx - nx)^2 + (qy - ny)^2 <= 8 c^2 and the expanded form |n - o|^2 - 2 (q - o).(n - o)
 * <= 24 c^2 about a block centre o, for |coordinates| <= c, against FLT_MAX < 2^128 (an infinite
 * screen value would tie every node and hide the nearest).  A larger or non-finite position is
 * refused on the host with PP_ERR_INVALID_ARGUMENT before anything is launched.  Inside the limit
 * positions need not lie in the scene's bounds: the f32 margins are widened by the magnitude of
 * the caller's points, and the answer is the sequential specification's (exact f64 nearest node,
 * lowest index on an exact tie of dx*dx + dy*dy; verify rejects a point outside the bounds).
 * Parity with that specification is tested up to 2^30. */
#define PP_COORD_MAX 2305843009213693952.0 /* 2^61 */

typedef struct pp_ctx pp_ctx;

/* DubinsConfig, src/dubins.rs:315-324 (field order and meaning kept) */
typedef struct pp_dubins_config {
    double sx, sy, syaw;
    double ex, ey, eyaw;
    double turn_radius;
    double step_size;
} pp_dubins_config;

/* Counters of the batched extend driver (since pp_rrt_new / pp_batch_new / pp_star_new or the
 * last pp_rrt_reset_stats).  pp_rrt_get_stats copies min(out_size, sizeof(pp_stats)) bytes: the
 * size argument guards ABI 2+ callers only (ABI 1's entry point had no out_size and a different
 * layout; a v1 binary must be rebuilt).  From ABI 2 on, fields are only ever appended, so an ABI 2
 * caller of a later library gets the prefix it knows and never an overrun.
 * The *_ms fields are HIP-event spans on the kernel's own stream: with the query batches' two or
 * three sub-batch streams a span also covers time the other streams' kernels held the GPU, so
 * their sums are stream-span times, not isolated kernel durations (those come from a rocprofv3
 * kernel trace: profiles/r*_kernel_durations.json). */
typedef struct pp_stats {
    int64_t iterations;       /* extend iterations consumed (plan_one calls, minus check_finish) */
    int64_t accepted;         /* nodes inserted */
    int64_t windows;          /* speculative windows launched */
    int64_t truncations;      /* windows cut short by an in-window candidate-list overflow */
    int64_t repair_rounds;    /* extra steer launches for parents that changed inside a window */
    int64_t repairs;          /* candidates re-steered in those rounds */
    int64_t literal_repairs;  /* candidates re-run on the literal single-lane path */
    int64_t nn_flagged;       /* samples whose f32 NN screen needed the exact f64 rescan */
    int64_t node_evals;       /* sample-node distance evaluations of the NN screen: screened
                                 samples (not in an obstacle) x the tree nodes the screen scanned */
    /* HIP events around every kernel of a window / batch step (profiling on), summed over the
     * launches; the batches keep their timed schedule (sub-batch streams) while profiled */
    double nn_scan_ms;        /* window_kernel (the NN screen + the previous window's resolve), or
                                 the batch NN (mq_sample_nn / star_sample) */
    int64_t nn_scan_launches;
    double steer_ms;          /* steer_walk */
    int64_t steer_launches;
    double finalize_ms;       /* nn_finalize (one tree: one launch per nn_scan launch) */
    double prep_ms;           /* steer_prep (one launch per steer launch) */
    double insert_ms;         /* mq_insert (query batch: one launch per nn_scan launch) */
    int64_t walk_points;      /* polyline points the steer walk generated and verified (profiling on) */
    int64_t walk_arc_points;  /* ... of them on L / R segments (one sincos each) */
    int64_t batch_steps;      /* query batches: lockstep steps launched (each up to the window per query) */
    int64_t batch_passes;     /* query batches: host passes (the first plus the top-ups of stopped windows) */
    double finish_ms;         /* device time of check_finish_kernel (HIP events; profiling on) */
    int64_t finish_launches;
    int64_t finish_nodes;     /* nodes check_finish ran on (profiling on) */
    int64_t finish_edges;     /* Dubins edges steered + verified by check_finish (profiling on) */
    int64_t finish_points;    /* polyline points those edges walked (profiling on) */
    int64_t finish_arc_points;  /* ... of them on L / R segments */
    /* ABI 3's persistent query-batch counters, removed in ABI 4: always 0 (layout kept) */
    int64_t reserved_abi3[8];
    int64_t samples_evaluated;  /* extend samples evaluated (one tree: the iterations) */
    int64_t samples_blocked;    /* ... of them whose point lies in an obstacle: rejected whatever
                                   the parent, without steer_prep / steer_walk or a pair list */
    int64_t walk_tasks;         /* steer_walk tasks walked (profiling on; ABI 5, appended) */
} pp_stats;

int pp_abi_version(void);
const char* pp_last_error(void);
/* number of visible HIP devices (0 when none); never fails on a CPU-only host */
int pp_device_count(int* n);

int pp_create(int device, pp_ctx** out);
int pp_destroy(pp_ctx* ctx);
int pp_synchronize(pp_ctx* ctx);
/* the position check every entry point applies (host only, no context): PP_OK when x[i] and y[i],
 * i < n, are all finite and at most PP_COORD_MAX in magnitude (either array may be NULL), else
 * PP_ERR_INVALID_ARGUMENT */
int pp_coord_check(const double* x, const double* y, int64_t n);

/* ------------------------------------------------------------- seeded sampling (host) */
/* SplitMix64 output `ctr` of stream `seed`: the build's replacement for rand::thread_rng
 * (src/rrt.rs:140).  Draw 2*it is x, 2*it+1 is y of iteration `it`. */
uint64_t pp_rng_u64(uint64_t seed, uint64_t ctr);
/* rand 0.7 gen_range(low, high) for f64 on that stream (src/rrt.rs:142-143) */
double pp_gen_range(uint64_t seed, uint64_t ctr, double low, double high);

/* --------------------------------------------------------------- dubins (src/dubins.rs) */
double pp_mod2pi(double theta);   /* dubins.rs:18-20 */
double pp_pi_2_pi(double angle);  /* dubins.rs:22-24 */
/* dubins_path_planning (dubins.rs:401-428) for n configurations on the GPU.  Output slot i of
 * px/py/pyaw is [i*cap, i*cap+cap).  word[i] is the ALL_PLANNERS index (0 LSL, 1 RSR, 2 LSR,
 * 3 RSL, 4 RLR, 5 LRL) or -1 for None; n_points[i] the kept point count; cost[i] the normalised
 * cost.  A configuration whose n_point exceeds cap gets word -2 and the call returns
 * PP_ERR_CAPACITY after filling the others. */
int pp_dubins_path_planning_batch(pp_ctx* ctx, const pp_dubins_config* confs, int n, int cap,
                                  double* px, double* py, double* pyaw, int32_t* n_points,
                                  int32_t* word, double* cost);

/* dubins_path_planning_from_origin (dubins.rs:326-399) for n configurations on the GPU, each the
 * 5 doubles (dx, dy, eyaw, c, step_size) of the Rust arguments (c = curvature, 1 / turn radius):
 * the LOCAL points after generate_local_course's trim (dubins.rs:281-288) and the yaw as generated
 * (not wrapped by pi_2_pi).  Outputs and errors as pp_dubins_path_planning_batch. */
int pp_dubins_path_planning_from_origin_batch(pp_ctx* ctx, const double* conf5, int n, int cap,
                                              double* px, double* py, double* pyaw,
                                              int32_t* n_points, int32_t* word, double* cost);
/* lsl, rsr, lsr, rsl, rlr, lrl (dubins.rs:27-153) of n (alpha, beta, d) triples on the GPU:
 * tpq[18 i + 3 w + {0, 1, 2}] = (t, p, q) of word w in ALL_PLANNERS order (dubins.rs:291),
 * ok[6 i + w] = 0 where the word is None (then its t, p, q are 0). */
int pp_dubins_words_batch(pp_ctx* ctx, const double* abd, int n, double* tpq, int32_t* ok);
/* The arc points' sine and cosine, for tests: s[i], c[i] = the library's own routine (the steer
 * walk's, on the constants the library ships) and s_ocml[i], c_ocml[i] = the HIP math library's
 * sincos of x[i] from the same compilation unit and flags, n arguments with |x[i]| < 2^30 (the
 * routine's range; PP_ERR_INVALID_ARGUMENT otherwise).  The two pairs must be equal bit for bit:
 * the walk's points are specified by the second and computed by the first. */
int pp_sincos_small_batch(pp_ctx* ctx, const double* x, int n, double* s, double* c,
                          double* s_ocml, double* c_ocml);

/* ------------------------------------------------------------------ scene (src/rrt.rs) */
/* create_circle(center, radius) (rrt.rs:43-60): the crate's polygon, n = ceil(2 pi r) chords and
 * the n + 1 vertices i = 0..=n at angle 2 pi / n * i, x then y interleaved in xy (2 (n + 1)
 * doubles, same evaluation order as the Rust expression; host arithmetic, like pp_mod2pi).
 * *n = the vertex count; PP_ERR_CAPACITY when cap (vertices) is too small. */
int pp_create_circle(double cx, double cy, double radius, double* xy, int cap, int* n);
/* Space::new(bounds, Robot::new(width, height, max_steer), obstacles) (rrt.rs:25,81-122) with
 * the bounds an axis-aligned rectangle (x0, y0)-(x1, y1) and the obstacles create_circle discs
 * (rrt.rs:43-60) given as centres and radii.  Bounds shrink and discs grow by width/2. */
int pp_space_new(pp_ctx* ctx, double x0, double y0, double x1, double y1, double robot_width,
                 double robot_height, double max_steer, const double* cx, const double* cy,
                 const double* r, int m);
/* BASELINE config 4: replace the obstacles of the current Space by a bit-packed occupancy grid
 * of w x h cells of size `cell` whose corner is (x0, y0): cell (i, j) is bit i % 32 of word
 * j * ceil(w / 32) + i / 32.  Verify then requires every point of the line inside the bounds and
 * in a free cell, with cell = (floor((x - x0) / cell), floor((y - y0) / cell)) and points outside
 * the grid counting as occupied; segments are not rasterised.  (The reference has no grid mode;
 * this is the build-defined semantics of SURVEY.md §8d config 4.)  A later pp_space_new clears
 * it; a planner must be created after it (pp_rrt_new / pp_batch_new). */
int pp_space_set_grid(pp_ctx* ctx, const uint32_t* bits, int w, int h, double x0, double y0,
                      double cell);
/* Space::new(bounds, Robot::new(width, height, max_steer), obstacles) (rrt.rs:25,81-122) with
 * polygon bounds and polygon obstacles, as examples/rrt/src/main.rs:30-45 builds them from its
 * JSON scene.  bounds_xy: nb vertices (x, y interleaved) of the bounds ring; obstacle o is the
 * ring obs_xy[2*obs_off[o] .. 2*obs_off[o+1]); a closing repeat of the first vertex is dropped.
 * Build-defined: geo-offset's buffers are the exact Minkowski buffers — an
 * obstacle grows by the closed disc of radius width/2 (a segment hits it when it crosses an edge
 * or comes within width/2 of one), the bounds shrink to the points at distance >= width/2 from
 * the ring inside it (tested on the line's points, like geo's Contains<LineString>).
 * rand_point samples the bounds' bbox shrunk by width/2.  Replaces the previous scene. */
int pp_space_new_polygons(pp_ctx* ctx, const double* bounds_xy, int nb, const double* obs_xy,
                          const int32_t* obs_off, int n_obs, double robot_width,
                          double robot_height, double max_steer);
/* Space::verify (rrt.rs:124-137) of k polylines on the GPU: line i is the points
 * [off[i], off[i+1]) of x / y; ok[i] = 1 when the line is inside the bounds and meets no
 * obstacle (a one-point line is tested as a point). */
int pp_space_verify_batch(pp_ctx* ctx, const double* x, const double* y, const int64_t* off,
                          int k, uint8_t* ok);
/* the shrunken bounds bbox (minx, maxx, miny, maxy) sampled by Space::rand_point (rrt.rs:84-106) */
int pp_space_get_bounds(pp_ctx* ctx, double out_minx_maxx_miny_maxy[4]);

/* ----------------------------------------------------------------- planner (src/rrt.rs) */
/* RRT::new(start, start_yaw, goal, goal_yaw, max_iter, step_size, space) (rrt.rs:335-355) plus
 * the sampling seed and an initial node capacity (grown on demand). */
int pp_rrt_new(pp_ctx* ctx, double sx, double sy, double syaw, double gx, double gy, double gyaw,
               int64_t max_iter, double step_size, uint64_t seed, int64_t capacity);
/* samples screened per speculative window (K in [1, 4096]; default 4096).  K bounds the samples
 * a window screens, steers and resolves, not the iterations it spans: an iteration whose sample
 * lies in an obstacle (the disc and grid scenes' pre-test) is rejected where it is drawn and takes
 * none of the K places, so a window spans up to 2 K iterations (the cap bounds its draws however
 * many are blocked).  Polygon scenes and pp_rrt_extend_samples with a nearest-node or yaw record
 * have no pre-test: a window is K iterations.  Results do not depend on K. */
int pp_rrt_set_window(pp_ctx* ctx, int k);
/* n_iter iterations of plan_one's extend (rrt.rs:583-589: rand_point, get_nearest_node,
 * Node::new, verify_node, insert) with the sequential semantics of one rayon thread. */
int pp_rrt_extend(pp_ctx* ctx, int64_t n_iter, int64_t* n_accepted);
/* plan_one's extend (rrt.rs:583-589) over k CALLER-DRAWN samples: iteration it + i takes
 * (sx[i], sy[i]) as its Space::rand_point (rrt.rs:139-146, 406-412) instead of the seeded stream,
 * so a host that owns its RNG drives the same speculative GPU windows (SURVEY.md §8(b)'s
 * pp_extend_batch).  Sequential semantics: sample i sees the tree after samples < i; accepted
 * samples are inserted in order (rrt.rs:586-589).  Per sample (each output may be NULL):
 * nearest[i] = get_nearest_node (rrt.rs:378-391) of the tree as it stood, i.e. the parent
 * Node::new took; yaw[i] = that node's compute_yaw (rrt.rs:169-175, 267-271); ok[i] = 1 when
 * verify_node (rrt.rs:414-426) accepted and the node was inserted (it then has index
 * n_before + the number of ok samples before i).  *n_accepted (may be NULL) = the inserts.
 * Samples must be finite; the iteration counter advances by k.  With samples drawn as
 * pp_gen_range(seed, 2 it, ..), pp_gen_range(seed, 2 it + 1, ..) the tree equals pp_rrt_extend's. */
int pp_rrt_extend_samples(pp_ctx* ctx, const double* sx, const double* sy, int64_t k,
                          int32_t* nearest, double* yaw, uint8_t* ok, int64_t* n_accepted);
/* replace the planner's tree by n host-owned nodes (root first, as pp_rrt_tree_export returns
 * them: Node x, y, yaw (rrt.rs:161-166) and parent, -1 for node 0, otherwise an earlier node:
 * the crate's insertion order, rrt.rs:586-589).  The scene, goal, step size, seed, iteration
 * counter and statistics stay; later extends continue from this tree.  Export -> import -> extend
 * equals extend on the original. */
int pp_rrt_tree_import(pp_ctx* ctx, const double* x, const double* y, const double* yaw,
                       const int32_t* parent, int64_t n);
/* one plan_one extend (rrt.rs:583-589); *accepted = 1 when the node was inserted */
int pp_rrt_plan_one(pp_ctx* ctx, int32_t* accepted);
int pp_rrt_tree_size(pp_ctx* ctx, int64_t* n);
int pp_rrt_iteration(pp_ctx* ctx, int64_t* it);
/* copy the tree out (root first): coordinates, yaw (Node.yaw, rrt.rs:161-166), parent (-1 root) */
int pp_rrt_tree_export(pp_ctx* ctx, double* x, double* y, double* yaw, int32_t* parent,
                       int64_t cap, int64_t* n);
/* line_to_origin(node, Robot.max_steer, step_size) (rrt.rs:291-321) of tree node `node`: the
 * concatenated polyline node -> ... -> root in the sequential order (each edge's Dubins points
 * child -> parent, steered on the GPU; [(x, y)] of the child where the steer is None; the root
 * contributes [(root x, root y)]).  *n = its points; PP_ERR_CAPACITY when cap is too small (call
 * with cap 0 for the size). */
int pp_rrt_line_to_origin(pp_ctx* ctx, int32_t node, double* x, double* y, int64_t cap,
                          int64_t* n);
/* RRT::get_nearest_node (rrt.rs:378-391) for k points: exact nearest by dx*dx+dy*dy, lowest
 * index on ties; d2 may be NULL */
int pp_rrt_get_nearest_node_batch(pp_ctx* ctx, const double* qx, const double* qy, int k,
                                  int32_t* idx, double* d2);
/* RRT::verify_node(Node::new(point, tree[parent])) (rrt.rs:169-175, 414-426) for k candidates:
 * ok[i] = 1 when the line to the root verifies; yaw[i] = the new node's yaw (may be NULL) */
int pp_rrt_verify_node_batch(pp_ctx* ctx, const double* x, const double* y,
                             const int32_t* parent, int k, uint8_t* ok, double* yaw);

/* Re-verify the planner's tree against the context's current Space and drop every node whose
 * line_to_origin no longer verifies (RRT::verify_node, rrt.rs:414-426, per node): node i > 0 stays
 * when Space::verify accepts the Dubins points from its stored pose to its parent's stored pose
 * followed by the parent's point (the stored yaw is used, rrt.rs:301-311; a None steer gives the
 * two-point line) and its parent stays.  The root always stays (RRT::new inserts it unverified,
 * rrt.rs:344-346); a root the new scene covers takes every other node with it.  Kept nodes keep
 * their order and their poses bit for bit, parents are remapped.  Accepted on a valid planner and
 * on one that a later pp_space_new, pp_space_new_polygons or pp_space_set_grid invalidated while
 * its tree is still on the device (every other call on such a planner stays PP_ERR_STATE, and
 * pp_rrt_new starts from a root as before); on success the planner is valid for the new scene
 * and later extends, plans and queries continue on the pruned tree.  The iteration counter, seed,
 * goal, step size, window and statistics stay; what pp_rrt_new derives from the scene is derived
 * again.  *n_kept (may be NULL) = the nodes that stay; new_index (may be NULL): one entry per node
 * before the call, its index afterwards or -1 when dropped.  PP_ERR_STATE without a tree;
 * PP_ERR_STEER_OVERFLOW leaves the tree unmodified.  (The RRT* batch: pp_star_revalidate.) */
int pp_rrt_revalidate(pp_ctx* ctx, int64_t* n_kept, int32_t* new_index);

/* --------------------------------------------------- goal connection (src/rrt.rs:428-619) */
/* RRT::check_finish (rrt.rs:428-438) for k tree nodes: optimize_from_goal's shortcut search
 * (rrt.rs:463-501, RECURSION_LIMIT 16), finalize's line (rrt.rs:503-540) and its verify.
 * ok[i] = 1 when the line verifies (Some); length[i] = its euclidean_length, n_points[i] its
 * points (both may be NULL; computed for verified lines only).  chain (may be NULL) receives k
 * rows of PP_CF_CHAIN ints: [levels, edges, optimize's chosen ancestor per level...]. */
#define PP_CF_CHAIN 18
int pp_rrt_check_finish_batch(pp_ctx* ctx, const int32_t* nodes, int k, uint8_t* ok,
                              double* length, int32_t* n_points, int32_t* chain);
/* check_finish for one node with the line itself (root side first, as finalize returns it);
 * *n = 0 when *ok = 0.  PP_ERR_CAPACITY when cap is too small. */
int pp_rrt_check_finish(pp_ctx* ctx, int32_t node, uint8_t* ok, double* x, double* y,
                        int64_t cap, int64_t* n, double* length);
/* RRT::optimize(node, i) (rrt.rs:463-487) for tree node `node`: *n_chain = 0 when it returns None
 * (also for i >= RECURSION_LIMIT = 16), else the depth of the returned chain: chain[l] (at most
 * 16 - i entries) is the tree node the l-th copy connects to, i.e. the returned Node sits at
 * node's coordinates with parent a copy of chain[0] at its coordinates, ..., ending at the tree
 * node chain[n - 1]; each copy's yaw is Node::new's compute_yaw toward its parent. */
int pp_rrt_optimize(pp_ctx* ctx, int32_t node, int i, int32_t* chain, int* n_chain);
/* RRT::finalize(goal) (rrt.rs:489-540) for the caller-built goal node Node::new_goal((gx, gy),
 * parent, gyaw) with `parent` a tree node: optimize_from_goal (the planner's goal yaw when
 * optimize succeeds, rrt.rs:494-498), then every edge's Dubins points, reversed.  The line is
 * returned whether or not it verifies; *verified (may be NULL) = Space::verify of it (what
 * check_finish adds).  *n = its points (cap 0 or x/y NULL: the size only); a None steer on the
 * chain returns PP_ERR_REFERENCE_PANIC (rrt.rs:529).  The line is assembled in a fixed device
 * buffer of 65536 points (a goal some 5000 turn radii from its parent at step 0.1).  A longer
 * line that does not verify — a goal far outside the scene — is still answered: *n is its exact
 * point count (counted on the device without storing it, edges of up to 2e9 steps) and
 * *verified = 0, PP_OK for the size-only call; asking for its points is PP_ERR_CAPACITY.  A longer
 * line that verifies is PP_ERR_CAPACITY (its length is part of the answer). */
int pp_rrt_finalize(pp_ctx* ctx, double gx, double gy, double gyaw, int32_t parent, double* x,
                    double* y, int64_t cap, int64_t* n, uint8_t* verified);
/* RRT::plan (rrt.rs:599-619), sequential spec: n_iter plan_one iterations (extend + check_finish
 * on every accepted node); *best_node = the node whose finish has the minimum euclidean_length
 * (first on ties, -1 when none verified); the line via pp_rrt_check_finish(best_node). */
int pp_rrt_plan(pp_ctx* ctx, int64_t n_iter, int32_t* best_node, double* best_length,
                int64_t* n_finishes);

/* ------------------------------------------------ independent query batch (BASELINE config 3) */
/* q independent planners on the context's scene — RRT::new (rrt.rs:335-355) per query with
 * start starts[3i..3i+2] (x, y, yaw), goal goals[3i..] (may be NULL), sampling stream seeds[i],
 * the shared max_iter and step_size.  Replaces any previous batch of the context. */
int pp_batch_new(pp_ctx* ctx, int q, const double* starts, const double* goals,
                 const uint64_t* seeds, int64_t max_iter, double step_size);
/* speculative iterations per query and step (a power of two <= 64; 0 = automatic: 32, halved
 * while a step would hold more than 262144 tasks, i.e. q * k > 262144).  Results do not depend on
 * it: every query's tree equals its one-at-a-time sequential run.  Applies to the current batch
 * and the next ones. */
int pp_batch_set_window(pp_ctx* ctx, int k);
/* How pp_batch_plan runs check_finish (results are identical; for A/B measurement and tests):
 * rounds = 1 (default) in steer rounds, phase A taking span0 candidate edges per
 * node in its first round and span in the later ones (0 = the default, else 1..16); rounds = 0:
 * check_finish_kernel alone, one wave per (query, node).  Applies to the context's later plans. */
int pp_batch_set_finish_schedule(pp_ctx* ctx, int rounds, int span0, int span);
/* n_steps lockstep steps: every query runs one plan_one extend iteration (rrt.rs:583-589) per
 * step until it reaches max_iter.  Totals over the batch are returned (may be NULL).  On the
 * GPU a step evaluates up to the batch window's iterations per query at once. */
int pp_batch_extend(pp_ctx* ctx, int64_t n_steps, int64_t* n_iterations, int64_t* n_accepted);
/* per-query tree sizes (q int32), consumed iterations and NN node-distance evaluations (q int64
 * each); any may be NULL.  With pp_set_profiling on, pp_batch_extend times its NN kernel with
 * HIP events into pp_stats.nn_scan_ms / nn_scan_launches. */
int pp_batch_state(pp_ctx* ctx, int32_t* n_nodes, int64_t* iterations, int64_t* node_evals);
/* RRT::plan (rrt.rs:599-619) of every query of the batch, on its tree as extended so far:
 * check_finish (rrt.rs:428-438: optimize_from_goal, finalize, verify) of every node the query
 * inserted (1 .. n_q - 1 in insertion order, rrt.rs:591) with the query's goal from
 * pp_batch_new, then the first minimum euclidean_length (rrt.rs:607-617).  Per query (q entries
 * each, any may be NULL): best_node (-1: no finish, the reference's None), length (inf when none),
 * n_points of the finalized line, n_finishes (verified check_finish lines); n_checked = the
 * (query, node) pairs checked. */
int pp_batch_plan(pp_ctx* ctx, int32_t* best_node, double* length, int32_t* n_points,
                  int32_t* n_finishes, int64_t* n_checked);
/* Every query's planned line in one call, packed.  finalize's line (rrt.rs:503-540) of
 * check_finish(nodes[i]) for every query i of the batch, with the query's own goal: exactly the
 * line pp_rrt_check_finish returns for that node on that tree (root side first).  nodes: q
 * entries, a node of query i's tree (0 .. n_i - 1) or -1 (skip).  off: q + 1 entries, row i =
 * points [off[i], off[i + 1]) of x / y; a row is empty when nodes[i] is -1 or check_finish is
 * None (ok[i] = 0).  ok (q, may be NULL).  *n_total = off[q].  With nodes = pp_batch_plan's
 * best_node, row i has that plan's n_points[i] points, so x / y can be sized from the plan.
 * x / y NULL or cap <= 0: sizes only (off, ok, n_total filled, PP_OK).  cap < *n_total:
 * PP_ERR_CAPACITY with off / ok / n_total filled; also when *n_total exceeds what one call stages
 * on the device, 2^26 points (1 GiB; export the queries in several calls then, -1 skips a query).
 * PP_ERR_STATE without a batch; PP_ERR_INVALID_ARGUMENT for a NULL nodes, off or n_total or a
 * node outside its query's tree; the check_finish errors as pp_batch_plan
 * (PP_ERR_REFERENCE_PANIC, ...).  Runs on the context's stream; the trees and the extend state
 * are not modified. */
int pp_batch_paths(pp_ctx* ctx, const int32_t* nodes, int64_t* off, double* x, double* y,
                   int64_t cap, int64_t* n_total, uint8_t* ok);
/* pp_rrt_revalidate for every query's tree of the batch, against the context's current Space; a
 * batch that a later pp_space_new or pp_space_new_polygons invalidated is accepted and valid again
 * afterwards.  The iteration counters, seeds, goals, step size, window and statistics stay.
 * n_nodes (q, may be NULL): the tree sizes after the call; *n_dropped (may be NULL): the nodes
 * dropped over the batch; new_index (may be NULL): the sum of the old tree sizes, query i's
 * entries at the prefix sum of pp_batch_state's n_nodes read before the call, each a node's index
 * in its tree afterwards or -1.  PP_ERR_STATE without a batch. */
int pp_batch_revalidate(pp_ctx* ctx, int32_t* n_nodes, int64_t* n_dropped, int32_t* new_index);
/* one query's tree (root first), like pp_rrt_tree_export */
int pp_batch_tree_export(pp_ctx* ctx, int query, double* x, double* y, double* yaw,
                         int32_t* parent, int64_t cap, int64_t* n);

/* ------------------------------------------------- RRT* query batch (BASELINE config 5) */
/* Build-defined: the reference has no RRT* (SURVEY.md §8d config 5, §8f row 4).  q independent
 * k-nearest RRT* planners (Karaman & Frazzoli) in the crate's conventions (DESIGN.md §3.7,
 * oracle/pp_oracle.c orc_star_extend): rand_point and the exact nearest node as in the extend
 * (rrt.rs:139-146, 378-391); with eta > 0 a sample farther than eta from its nearest node moves
 * onto the chord at distance eta (eta = 0: the node sits at the sample, like Node::new); the edge
 * to the nearest node (verify_node, rrt.rs:414-426) gates the insert; the parent is the first
 * strict minimum of cost(p) + Dubins cost (dubins.rs:351-361) over the nearest node and the k
 * nearest nodes of the new point; then every one of those k nodes whose edge to the new node is
 * feasible and makes it strictly cheaper is rewired (its pose kept), costs of its subtree
 * recomputed.  k = 0: ceil(2e ln n) (at most 63 and n); 1..63: fixed.  Replaces any previous RRT*
 * batch of the context. */
int pp_star_new(pp_ctx* ctx, int q, const double* starts, const uint64_t* seeds,
                int64_t max_iter, double step_size, int k, double eta);
/* n_steps lockstep steps: every query runs one RRT* iteration per step until max_iter.  Batch
 * totals (each may be NULL): iterations, inserted nodes, rewires.  A later pp_space_new,
 * pp_space_new_polygons or pp_space_set_grid does not invalidate the RRT* batch: this call,
 * pp_star_plan and pp_star_paths keep working, but until pp_star_revalidate has run the trees are
 * unverified in the new scene (they may hold edges through its obstacles). */
int pp_star_extend(pp_ctx* ctx, int64_t n_steps, int64_t* n_iterations, int64_t* n_accepted,
                   int64_t* n_rewires);
/* per-query tree sizes (q int32), iterations, NN node-distance evaluations and rewires (q int64
 * each); any may be NULL */
int pp_star_state(pp_ctx* ctx, int32_t* n_nodes, int64_t* iterations, int64_t* node_evals,
                  int64_t* rewires);
/* one query's tree (root first): coordinates, yaw, parent (-1 root) and node cost (root 0) */
int pp_star_tree_export(pp_ctx* ctx, int query, double* x, double* y, double* yaw,
                        int32_t* parent, double* cost, int64_t cap, int64_t* n);
/* Focused sampling (build-defined, DESIGN.md §3.7 "Focused sampling"; CPU restatement
 * tests/star_focus_ref.py): Informed RRT* as a rejection filter on the same counter RNG.  Every
 * query carries a focus point (fx, fy), a bound L in length units (finite and > 0, or +inf: no
 * focus) and a counter `skipped` of rejected draws; pp_star_new sets L = +inf and skipped = 0.
 * Draw d of a query is the point (gen_range(seed, 2d, minx, maxx), gen_range(seed, 2d + 1, miny,
 * maxy)), and (x0, y0) is its root's stored point.  Iteration `it` of a query:
 *   L = +inf:  the sample is draw it + skipped, then the iteration of pp_star_new's comment (with
 *              skipped = 0: that iteration exactly).
 *   L finite:  for j = 0 .. PP_STAR_FOCUS_DRAWS - 1 the draw it + skipped + j is in the set iff
 *              sqrt((x-x0)*(x-x0) + (y-y0)*(y-y0)) + sqrt((x-fx)*(x-fx) + (y-fy)*(y-fy)) < L
 *              (f64, uncontracted, correctly rounded square roots; the raw sample, before Steer).
 *              At the first j in the set skipped += j and the iteration runs with that sample.
 *              With none, skipped += PP_STAR_FOCUS_DRAWS - 1 and the iteration ends: no nearest
 *              node, no insert, no rewire, no node evaluations.
 * Either way it += 1: a step is still one iteration per query, and max_iter, the tree capacity
 * and the k schedule are untouched; only the draw counter runs ahead.  An empty set (L at most the
 * distance between the root and the focus) is legal: every iteration then rejects all its draws.
 * pp_star_revalidate, pp_star_repair, pp_star_prune, pp_space_*, pp_star_plan and pp_star_paths
 * leave the focus and skipped alone; only pp_star_set_focus and pp_star_new change them. */
#define PP_STAR_FOCUS_DRAWS 1024
/* fxy: q rows (fx, fy); bound: q values L.  Both NULL: every query's focus is cleared (L = +inf),
 * skipped is kept.  PP_ERR_INVALID_ARGUMENT for exactly one NULL, for a bound that is NaN, <= 0 or
 * -inf, and for a focus row that fails pp_coord_check; a failed call leaves the focus as it was.
 * PP_ERR_STATE without an RRT* batch. */
int pp_star_set_focus(pp_ctx* ctx, const double* fxy, const double* bound);
/* fxy (2q), bound (q), skipped (q int64); each may be NULL */
int pp_star_get_focus(pp_ctx* ctx, double* fxy, double* bound, int64_t* skipped);
/* Pruning by the focus bound (build-defined, DESIGN.md §3.7 "Pruning by the focus bound"; CPU
 * restatement tests/star_prune_ref.py): the second half of Informed RRT*.  One call prunes every
 * query's tree against the query's stored focus, the (fx, fy), L that pp_star_set_focus set and
 * pp_star_get_focus reads back.  R is the turn radius of the context's current Space.
 *   Node test.  Node i > 0 of query q fails iff
 *       cost[i] * R + sqrt((x[i]-fx)*(x[i]-fx) + (y[i]-fy)*(y[i]-fy)) > L
 *     in f64, uncontracted (every product and sum rounded on its own), the square root correctly
 *     rounded; cost is the stored cost-to-come in pp_star_tree_export's unit.  The comparison is
 *     strict: a node exactly on the bound stays.  The heuristic is admissible (a Dubins path is
 *     never shorter than the distance between its ends): a failing node cannot lie, at its current
 *     cost, on a path to the focus of length <= L.  With L = +inf the test never fails.
 *   Protected chain.  keep[q] is a node of query q's tree, or -1.  Every node on the chain
 *     keep[q] -> parent -> ... -> root passes, whatever the node test says: with L = (pp_star_plan's
 *     cost) * R and a straight goal edge the best node sits exactly on the bound, and one ulp of
 *     rounding in cost * R would otherwise drop the path that defined the bound.  keep =
 *     pp_star_plan's best_node is the intended use; keep NULL means all -1.
 *   Keep rule (pp_star_revalidate's).  The root always stays.  Node i stays iff it and every node
 *     on its chain to the root pass, so a failing node takes its descendants with it; chains are
 *     not index-ordered (a rewired node's parent may be a later node), and a chain that does not
 *     end in its tree's root is dropped.
 *   Compaction (pp_star_revalidate's).  Kept nodes keep their order and their x, y, yaw, cost and
 *     edge cost bit for bit; parents are remapped and may still exceed their child's index.
 * Untouched: the focus and skipped; the iteration counters, seeds, k, eta, step size and max_iter;
 * the per-query evaluations and rewires and pp_stats; the blocked roots of polygon mode.  The
 * scene is not consulted beyond R: the call neither verifies nor un-verifies anything.  Caveat: a
 * pruned node could have been made cheaper by a later rewire and then have passed — the usual
 * branch-and-bound trade of Informed RRT* (DESIGN.md §3.7 measures what it costs).
 * keep: q entries, or NULL.  n_nodes, n_dropped, new_index: exactly pp_star_revalidate's, each may
 * be NULL; new_index is laid out at the prefix sums of the sizes before the call.  PP_ERR_STATE
 * without an RRT* batch or a scene.  PP_ERR_INVALID_ARGUMENT for a keep[q] outside [-1, n_q),
 * checked on the host before anything is launched: trees and focus are unchanged. */
int pp_star_prune(pp_ctx* ctx, const int32_t* keep, int32_t* n_nodes, int64_t* n_dropped,
                  int32_t* new_index);
/* Re-verify every query's tree of the RRT* batch against the context's current Space and drop
 * what no longer holds (build-defined; CPU restatement
 * tests/star_revalidate_ref.py).  The edge of node i > 0 is RRT*'s feasible edge (§3.7) from its
 * stored pose to its parent's stored pose: the Dubins word is Some and Space::verify accepts the
 * edge's points followed by the parent's point.  The stored yaw is the edge's own for an inserted
 * node (compute_yaw toward the parent it chose) and for a rewired node (it kept its pose).  A None
 * steer is an infeasible edge (not pp_rrt_revalidate's two-point line); it cannot occur in a tree
 * this library grew — the word does not depend on the scene and every tree edge was feasible when
 * it was made — so the device reports for it whatever its steer round does.  A node stays when
 * every edge on its chain to the root is feasible; the chain is not index-ordered (a rewired
 * node's parent is the later node that rewired it).  The root always stays; in polygon mode a root
 * that fails verify as a point drops every other node and the query never inserts again.  Kept
 * nodes keep their order and their pose, cost and edge cost bit for bit (dropping other nodes
 * changes no kept node's cost); parents are remapped and may still exceed their child's index.
 * The iteration counters, seeds, k, eta, step size, per-query evaluations and rewires and the
 * statistics stay.  Accepted on any valid RRT* batch.  Outputs as pp_batch_revalidate's: n_nodes
 * (q, may be NULL): the tree sizes after the call; *n_dropped (may be NULL): the nodes dropped
 * over the batch; new_index (may be NULL): the sum of the old tree sizes, query i's entries at the
 * prefix sum of pp_star_state's n_nodes read before the call, each a node's index in its tree
 * afterwards or -1.  PP_ERR_STATE without an RRT* batch or a scene; PP_ERR_STEER_OVERFLOW leaves
 * every tree unmodified.  (A dropped subtree whose top still reaches a kept node is lost here;
 * pp_star_repair hangs it back.) */
int pp_star_revalidate(pp_ctx* ctx, int32_t* n_nodes, int64_t* n_dropped, int32_t* new_index);
/* pp_star_revalidate with up to `rounds` re-attachment rounds before the compaction (build-defined,
 * DESIGN.md §3.8; CPU restatement tests/star_repair_ref.py).  rounds = 0 is pp_star_revalidate,
 * result for result.  Round r (for as long as it has tops): a top is a dropped node that was no
 * top before and whose own edge fails (r = 1) or whose parent was a top of an earlier round that
 * found no parent (r > 1).  A top's candidates are the star_k(k, |K|) nearest nodes of its point
 * by (squared distance, index before the call) among the set K kept at the start of the round;
 * the edge top -> candidate keeps the top's stored pose (like a rewire), is feasible as above, and
 * total = cost[candidate] + its Dubins cost with the costs of the start of the round.  The first
 * strict minimum of total in candidate order becomes the top's parent (its edge cost and cost
 * with it); a top without a feasible candidate is dropped for good.  Every dropped node whose
 * chain of feasible stored edges reaches a re-attached top is kept again: its edge cost stays,
 * its cost becomes cost[parent] + edge cost, parents before children.  Tops read the start-of-
 * round state only, so the result does not depend on their order.  A root-blocked query (polygon
 * mode) re-attaches nothing.  Nodes pp_star_revalidate keeps keep cost and edge cost bit for bit;
 * compaction, counters and the derived state are pp_star_revalidate's.  rounds outside [0, 16]:
 * PP_ERR_INVALID_ARGUMENT.  n_nodes, n_dropped, new_index: as pp_star_revalidate's (each may be
 * NULL).  *n_reattached (may be NULL): the tops that found a parent; *n_recovered (may be NULL):
 * the nodes kept that pp_star_revalidate would have dropped, those tops included.  PP_ERR_STATE
 * without an RRT* batch or a scene; PP_ERR_STEER_OVERFLOW leaves every tree unmodified.  The host
 * synchronises once per round run (to read the round's top count), and once more at the end. */
int pp_star_repair(pp_ctx* ctx, int rounds, int32_t* n_nodes, int64_t* n_dropped,
                   int64_t* n_reattached, int64_t* n_recovered, int32_t* new_index);
/* Move every query's root along its tree (build-defined, DESIGN.md §3.8 "Advancing the root"; CPU
 * restatement tests/star_advance_ref.py): the vehicle has driven part of its plan, and the tree
 * follows it instead of being thrown away.  Below n_q, parent, cost and elen are tree q's values
 * before the call.
 *
 * The new root.  nodes: q entries in [-1, n_q).  hops: NULL, or q entries >= 0.  With hops NULL
 * the new root is r = nodes[q]; with hops, r is the node min(hops[q], depth(nodes[q])) edges from
 * the root on the chain root -> ... -> nodes[q] (pp_star_plan's best node with hops = 1: one edge
 * along the planned path).  A query with nodes[q] = -1, or whose r is 0, is left alone bit for bit
 * (rows, costs, new_index the identity), whatever rounds is.  Every chain walk on the device is
 * bounded by n_q steps: a tree this library grew or imported has no cycle; the result for one
 * that has is unspecified, but the call ends.
 *
 * The kept core, for r > 0.  Tree edges are directed Dubins edges from the child's stored pose to
 * the parent's, so everything under r stays valid as it is, and the edges of r's proper ancestors
 * A = parent[r], ..., node 0 (m = depth(r) nodes, the old root included) point the wrong way.
 * K0 = the nodes i whose chain i -> ... -> 0 passes through r: r and its descendants (chains are
 * not index-ordered).  r becomes the root: parent -1, edge cost 0, cost 0.  Every other node of
 * K0 keeps its pose, parent and edge cost bit for bit; its cost is rebuilt from the new root
 * down, cost'[i] = cost'[parent[i]] + elen[i], one rounded f64 add per edge, parents before
 * children (not cost[i] - cost[r]: the sum is the invariant pp_star_forest_import checks).
 *
 * Re-attachment, rounds in [0, 16].  rounds = 0 stops at K0.  Otherwise the rounds are
 * pp_star_repair's with three inputs replaced: K at the start of round 1 is K0, the costs are
 * cost', and the tops of round 1 are all m nodes of A (the old root is one of them and keeps its
 * stored pose, like any top).  Everything else is pp_star_repair's: a top's candidates are the
 * star_k(k, |K|) nearest nodes of K as it stood at the start of the round by exact f64 (squared
 * distance, index before the call); the edge top -> candidate keeps the top's pose and is feasible
 * when the word is Some and Space::verify accepts its points followed by the candidate's point;
 * total = cost[candidate] + edge cost, the first strict minimum in candidate order wins; a top
 * with a choice takes parent, edge cost and cost; every dropped node that was never a top and
 * whose chain of stored edges reaches a re-attached top is kept again with its parent and edge
 * cost, cost = cost[parent] + elen, parents first; round r > 1: the tops are the dropped nodes,
 * never a top before, whose parent is a top of an earlier round that found no parent.  Tops read
 * the start-of-round state only, so their order cannot matter.  A re-attachment is not counted as
 * a rewire.
 *
 * Compaction.  r goes to index 0; all other kept nodes follow in their old index order (a
 * re-attached old root lands at index 1).  Parents are remapped and may exceed their child's
 * index.  new_index is laid out as pp_star_revalidate's, -1 for dropped nodes, new_index[r] = 0.
 * n_nodes, n_dropped, n_reattached, n_recovered: as pp_star_repair's (each may be NULL).  The
 * stored start pose of the query (what pp_star_revalidate's polygon-mode root test and the forest
 * export / import read) becomes r's pose bit for bit, and the focused sampler, which reads row 0,
 * has the new root as its first focus from the next step on.
 *
 * Untouched: iterations, seeds, skipped draws, the focus (fx, fy) and its bound L, k, eta, step
 * size, max_iter, node_evals, rewires, pp_stats and the blocked flags (a root-blocked query has
 * one node, so only -1 or 0 is valid for it).  The old L stays admissible for the new root: the
 * path that set it, less its driven part, is still in the tree, so L is only looser than it could
 * be; pp_star_plan followed by pp_star_set_focus tightens it.  With rounds = 0 the scene is
 * consulted for nothing; with rounds > 0 as in pp_star_repair.  The trees are not re-verified:
 * that remains pp_star_revalidate's job.
 *
 * PP_ERR_STATE without an RRT* batch or a scene.  PP_ERR_INVALID_ARGUMENT for NULL nodes, a node
 * outside [-1, n_q), a negative hop or rounds outside [0, 16], all checked on the host before
 * anything is launched.  PP_ERR_STEER_OVERFLOW is possible only with rounds > 0.  A failed call
 * leaves every tree, cost and stored start exactly as it was.  The host synchronises to read the
 * sizes, once per round run, and once at the end (rounds = 0: no per-round reads). */
int pp_star_advance(pp_ctx* ctx, const int32_t* nodes, const int32_t* hops, int rounds,
                    int32_t* n_nodes, int64_t* n_dropped, int64_t* n_reattached,
                    int64_t* n_recovered, int32_t* new_index);
/* Relax the trees of the RRT* batch (build-defined, DESIGN.md §3.8 "Relaxing the trees"; CPU
 * restatement tests/star_relax_ref.py): up to `rounds` in [1, 16] synchronous choose-parent rounds
 * over all nodes, on the device and in place.  It is pp_star_repair's choose-parent pass with
 * every node a top: nothing else in the library lets existing nodes look for a cheaper parent
 * among existing nodes (RT-RRT*'s rewiring from the root, RRT#'s relaxation).  All quantities are
 * build-defined and follow §3.7's conventions.
 *
 * One query q with active[q] != 0 (active NULL: all), n its tree size, the context's current
 * Space, the batch's k.  An inactive query, a tree of one node and a root-blocked query are
 * untouched bit for bit.  A round reads parent, cost and edge cost as they stood when it began:
 *
 * Candidates.  The candidates of node i > 0 are the star_k(k, n - 1) nearest nodes j != i of its
 * tree by exact f64 (dx * dx + dy * dy, index).  The root is a candidate like any other.  The
 * candidate equal to parent[i] keeps its place in the order but is never evaluated: by the cost
 * invariant its total is the node's own cost, and deriving it again through another math library
 * would turn an exact tie into a coin toss.
 *
 * Edge.  The edge i -> p keeps i's stored pose, yaw included (like a rewire or a repair top), and
 * runs to p's stored pose; it is feasible when the word is Some and Space::verify accepts its
 * points followed by p's point.  total = cost[p] + e, one rounded f64 add.
 *
 * Choice.  The first strict minimum of total in candidate order among the feasible candidates,
 * accepted only when total < cost[i] (strict, the extend's own rewire test).  A node with a choice
 * stages parent = p and edge cost = e; no node reads another node's staged values, so the order
 * in which nodes are taken cannot matter.
 *
 * Apply and rebuild.  After every node has chosen, the staged parents and edge costs are applied
 * and cost is rebuilt from the root level by level, cost[i] = cost[parent[i]] + elen[i], parents
 * final before children (pp_star_advance's order of additions, never a prefix sum): the invariant
 * pp_star_forest_import checks holds bit for bit.  No cycle can form: a new edge i -> p has
 * cost[p] + e < cost[i] with e >= 0, a stored edge has cost[parent] <= cost[child], so a cycle
 * would need start-of-round costs that never rise around it, hence no new edge on it.  No cost
 * rises (induction from the root, a rounded add is monotone), and a node with no re-parented
 * ancestor-or-self keeps its cost bit for bit.
 *
 * Early stop.  A round that re-parents nothing in any active query ends the call; *rounds_run
 * (may be NULL) counts the rounds executed, that last one included.  A call that ended so,
 * repeated, runs one round and changes nothing; so does a call in which no query takes part
 * (all inactive, root-blocked or lone roots): one round, nothing changed.
 *
 * n_rewired[q] (may be NULL): the re-parentings of query q over all rounds; the query's rewire
 * counter of pp_star_state advances by it, as pp_star_shortcut_commit's does.  *n_changed (may be
 * NULL): the nodes over the batch whose cost differs bit-wise from before the call.
 *
 * Untouched: poses, node order, tree sizes, iterations, seeds, skipped draws, the focus and its
 * bound (it stays admissible: costs only fall), node_evals, pp_stats and the blocked flags.  The
 * call neither verifies nor un-verifies a stored edge: on a tree that was not revalidated after a
 * scene change it may hang a node under one whose own chain no longer holds.
 *
 * PP_ERR_STATE without an RRT* batch or a scene, PP_ERR_INVALID_ARGUMENT for a NULL ctx or rounds
 * outside [1, 16], checked on the host before anything is launched.  PP_ERR_STEER_OVERFLOW: the
 * failing round is not applied, the rounds before it stay (each leaves a valid tree), *rounds_run
 * says how many were applied and n_rewired / *n_changed describe them.  The host synchronises to
 * read the sizes, once per round run, and once at the end. */
int pp_star_relax(pp_ctx* ctx, int rounds, const uint8_t* active, int32_t* n_rewired,
                  int32_t* rounds_run, int64_t* n_changed);
/* The last pp_star_relax call's counters, summed over its rounds: out[0] nodes of the forest,
 * out[1] candidates of the nodes that took part, out[2] those left after the parent skip, out[3]
 * after the skip of cost[p] >= cost[i], out[4] after the chord bound (the steer tasks), out[5] the
 * tasks whose edge was walked, out[6] node slices per round, out[7] the largest candidate count.
 * out[1 .. 5] are collected only while profiling is on (pp_set_profiling) and are 0 otherwise. */
int pp_star_relax_counts(pp_ctx* ctx, int64_t out[8]);
/* Goal connection (build-defined; CPU restatement tests/star_goal_ref.py).  The
 * goal edge of tree node m: the goal (gx, gy, gyaw) is the child and keeps its yaw, node m is the
 * parent — Dubins from the goal pose to the node's stored pose; feasible when the word is Some and
 * Space::verify accepts the edge's points followed by the node's point.  total[m] = cost[m] + the
 * edge's Dubins cost (the unit of pp_star_tree_export's cost), +inf when infeasible; the root is a
 * candidate like any other.  The best node is the first strict minimum of total in node order
 * (the lowest index on an exact tie).
 *
 * goal connection of every query of the RRT* batch on its tree as extended so far.
 * goals: q rows (gx, gy, gyaw).  Per query (each may be NULL): best_node (-1 none), cost (+inf none);
 * *n_checked = the (query, node) pairs considered = sum of tree sizes.  Trees are not modified;
 * may be called again after more pp_star_extend steps or with other goals. */
int pp_star_plan(pp_ctx* ctx, const double* goals, int32_t* best_node, double* cost,
                 int64_t* n_checked);
/* un-pruned cost-to-goal of one query: total[m] = cost[m] + e[m] or +inf, m < *n (cap as in the
 * exports: PP_ERR_CAPACITY when cap < *n; total NULL: the size only) */
int pp_star_goal_costs(pp_ctx* ctx, int query, const double goal[3], double* total, int64_t cap,
                       int64_t* n);
/* the path of (query, goal, node), root first: with E(child, parent) the kept Dubins points of
 * the edge from the child's stored pose to the parent's stored pose (a rewired node keeps its
 * pose), the line E(goal, node) ++ E(node, parent[node]) ++ ... ++ E(., root) ++ [(x0, y0)],
 * reversed; *length = its euclidean_length.  cap 0 or NULL x/y: the size only; PP_ERR_CAPACITY
 * when too small; PP_ERR_INVALID_ARGUMENT for a node out of range or whose goal edge is
 * infeasible; PP_ERR_REFERENCE_PANIC when a tree edge of the chain has no Dubins word */
int pp_star_path(pp_ctx* ctx, int query, const double goal[3], int32_t node, double* x, double* y,
                 int64_t cap, int64_t* n, double* length);
/* pp_star_path's line of (query i, goals[3i..], nodes[i]) for every query of the RRT* batch in
 * one call, packed like pp_batch_paths (rows, off, cap, n_total, ok, -1, the 2^26-point limit):
 * E(goal, node) ++ E(node, parent) ++ ... ++ [(x0, y0)], reversed.  length (q, may be NULL): the
 * row's euclidean_length, 0 for an empty row; filled with the points (not by a sizes-only call).
 * ok[i] = 0 and an empty row when the goal edge has no Dubins word; a tree edge without one is
 * PP_ERR_REFERENCE_PANIC; a chain deeper than 8192 nodes or a line of more than 65536 points
 * PP_ERR_CAPACITY.  The goal edge's Space::verify is pp_star_plan's business and is not repeated
 * here: any node's line is returned.  PP_ERR_STATE without an RRT* batch;
 * PP_ERR_INVALID_ARGUMENT for a NULL goals, nodes, off or n_total, a non-finite goal or a node
 * outside its query's tree.  The trees are not modified. */
int pp_star_paths(pp_ctx* ctx, const double* goals, const int32_t* nodes, int64_t* off, double* x,
                  double* y, int64_t cap, int64_t* n_total, double* length, uint8_t* ok);

/* ------------------------------ segment export and sampling (build-defined) */
/* A planned path as what it is: a chain of Dubins edges, each three primitives (arc / straight /
 * arc) — with heading and curvature, exact, a few dozen records a path — and a sampler that turns
 * such rows into trajectories at a spacing of the caller's choosing (CPU restatement:
 * tests/path_segments_ref.py).
 * Caller-owned SoA arrays of segments.  size = sizeof(pp_path_segments) as the caller compiled it;
 * fields past it read as NULL (like pp_forest_state). */
typedef struct pp_path_segments {
    uint64_t size;
    double *x, *y, *yaw; /* the segment's start pose */
    double *kappa;       /* signed curvature: +1/R (L), 0 (S), -1/R (R); R = the Space's turn radius */
    double *len;         /* arc length in length units, >= 0 */
} pp_path_segments;
/* Row i = the chain of Dubins edges pp_star_paths walks for (query i, goals[3i..], nodes[i]):
 * goal -> node -> parent -> ... -> root, every edge from the child's stored pose, its word the
 * one the point export chooses.  Every edge gives exactly three segments (zero-length ones
 * included), so a row of E edges has 3 E segments and off (q + 1 entries) counts segments.  For an
 * edge a -> b with word w and (t, p, q): segment 0 starts at a's pose bit for bit; len[j] =
 * (t | p | q) * R; kappa[j] by w's mode table; segment j + 1 starts at the closed-form end of
 * segment j in f64 — S: x + len cos(yaw), y + len sin(yaw), yaw; L / R: x + (sin(yaw + kappa len)
 * - sin(yaw)) / kappa, y - (cos(yaw + kappa len) - cos(yaw)) / kappa, yaw + kappa len.  Yaw is
 * never wrapped, and the next edge starts from its own stored pose again.
 * reverse = 0: generation order (the crate's stored yaws point toward the parent: goal edge first,
 * goal -> root).  reverse = 1: the same curve from the root to the goal, pp_star_paths' row order:
 * the segments in reverse order, each starting at its own end pose with yaw = end yaw + pi
 * (unwrapped), kappa negated, len unchanged.  Any other value: PP_ERR_INVALID_ARGUMENT.
 * length (q, may be NULL): the sum of the row's len in row order, 0 for an empty row; filled with
 * the segments (not by a sizes-only call).  ok, the empty rows (-1, a goal edge without a word),
 * PP_ERR_REFERENCE_PANIC and the 8192-deep chain limit: as pp_star_paths.  Sizes-only protocol as
 * there: seg NULL or cap <= 0 fills off / ok / n_total, PP_OK; cap < *n_total (cap: the entries
 * each array holds) is PP_ERR_CAPACITY with the sizes filled; a NULL array inside *seg is simply
 * not written.  PP_ERR_STATE without an RRT* batch or a scene; PP_ERR_INVALID_ARGUMENT for a NULL
 * goals, nodes, off or n_total, a non-finite goal or a node outside its tree, all checked on the
 * host before any launch.  No Space::verify is repeated.  Nothing in the batch is modified. */
int pp_star_path_segments(pp_ctx* ctx, const double* goals, const int32_t* nodes, int reverse,
                          int64_t* off, const pp_path_segments* seg, int64_t cap,
                          int64_t* n_total, double* length, uint8_t* ok);
/* The same for the extend batch: row i = finalize's chain of check_finish(nodes[i]) on query i's
 * tree with its goal — the goal, optimize's copies (their yaw by compute_yaw), the tree path down
 * to the root — as pp_batch_paths walks it; ok and the empty rows as there (a finish that does not
 * verify: ok 0, an empty row). */
int pp_batch_path_segments(pp_ctx* ctx, const int32_t* nodes, int reverse, int64_t* off,
                           const pp_path_segments* seg, int64_t cap, int64_t* n_total,
                           double* length, uint8_t* ok);
/* Sample q rows of segments (row r = entries [off[r], off[r + 1]) of the five arrays of *seg) every
 * ds along the arc; a pure function of its arguments: a context, but no scene or batch.  With P_0
 * = 0, P_{j+1} = P_j + len[j] in row order and L = the last P: samples at s_i = i ds for i = 0 ..
 * floor(L / ds), and one more at s = L when L > the last s_i; a row without segments has none.  A
 * sample lies on the first segment j with s < P_{j+1} at u = s - P_j, else on the last segment at
 * u = len; x, y, yaw by the closed forms above at u, kappa the segment's, s the arc position (each
 * output may be NULL).  poff (q + 1 entries) counts samples; sizes-only and capacity protocol as
 * above (every output NULL or cap <= 0: poff and n_total only); more than 2^26 samples in one
 * call is PP_ERR_CAPACITY.  PP_ERR_INVALID_ARGUMENT, checked on the host: q < 0, a NULL off, seg,
 * poff, n_total or segment array, off[0] != 0 or off decreasing, a non-finite entry, a negative
 * len, ds not finite or <= 0.  The arrays are uploaded once and the samples copied back once. */
int pp_segments_sample(pp_ctx* ctx, int q, const int64_t* off, const pp_path_segments* seg,
                       double ds, int64_t* poff, double* x, double* y, double* yaw, double* kappa,
                       double* s, int64_t cap, int64_t* n_total);

/* ------------------------------ shortcuts along the chain (build-defined) */
/* Shorten the path goal -> nodes[i] -> parent -> ... -> root of every query by Dubins shortcuts
 * between the poses of its own chain (CPU restatement: tests/star_shortcut_ref.py).  Positions:
 * c_0 = the goal (its own yaw), c_1 = the node, c_2 = its parent, ..., c_D = the root, each with
 * its stored pose.  Edge (i -> j), i < j <= i + span, is RRT*'s feasible edge from c_i's pose (own
 * yaw, like a rewire or goal edge) to c_j's stored pose: feasible when the word is Some and
 * Space::verify accepts the edge's points followed by c_j's point; w(i, j) = its Dubins cost (the
 * unit of pp_star_tree_export's cost) or +inf.  Every edge, the chain's own included, is
 * evaluated afresh against the context's current Space.  best[D] = 0; for i = D - 1 .. 0, best[i]
 * = the first strict minimum in increasing j of best[j] + w(i, j) (each sum rounded once; the
 * lowest j on an exact tie) and next[i] that j; the path follows next from 0 and costs best[0].
 * With span 1 on an unchanged scene that is pp_star_plan's total for the node.
 * goals: q rows (gx, gy, gyaw); nodes: q entries (-1: skip); span in [1, 63].  Row i of chain
 * (int32, CSR by off, q + 1 entries) = the tree nodes of the shortened path after the goal: the
 * node the goal now connects to first, 0 (the root) last.  cost[i] = best[0], ok[i] = 1 — or +inf,
 * 0 and an empty row when nodes[i] is -1 or no feasible route exists within the span (cost, ok:
 * may be NULL).  *n_tested (may be NULL) = the (i, j) pairs considered.  Sizes-only and capacity
 * protocol as pp_star_paths: chain NULL or cap <= 0 fills off / cost / ok / n_total / n_tested;
 * cap < *n_total is PP_ERR_CAPACITY with those filled.  A chain deeper than 8192 nodes, or more
 * than 2^26 pairs in one call (checked before any steer launch), is PP_ERR_CAPACITY.
 * PP_ERR_INVALID_ARGUMENT, before any launch: span outside [1, 63], NULL goals, nodes, off or
 * n_total, a non-finite goal, a node outside its tree.  PP_ERR_STATE without an RRT* batch or a
 * scene; PP_ERR_STEER_OVERFLOW as pp_star_plan.  Trees, focus, counters and stats are untouched. */
int pp_star_shortcut(pp_ctx* ctx, const double* goals, const int32_t* nodes, int span,
                     int64_t* off, int32_t* chain, int64_t cap, int64_t* n_total, double* cost,
                     uint8_t* ok, int64_t* n_tested);
/* The band of one query, un-culled (the counterpart of pp_star_goal_costs): *depth = D; cnode[i - 1]
 * = the tree node of position i (D entries, may be NULL); w[i * span + (j - i - 1)] = w(i, j) for
 * i < D, +inf where infeasible or j > D.  cap counts rows of w (and entries of cnode): w NULL
 * gives the size only, cap < D is PP_ERR_CAPACITY.  Errors as pp_star_shortcut's, and
 * PP_ERR_INVALID_ARGUMENT for a query out of range or a NULL goal or depth. */
int pp_star_shortcut_edges(pp_ctx* ctx, int query, const double goal[3], int32_t node, int span,
                           double* w, int32_t* cnode, int64_t cap, int64_t* depth);
/* Commit the chain's shortcuts into the trees (CPU restatement: tests/star_shortcut_commit_ref.py):
 * a shortcut edge (i -> j) is an RRT* rewire of chain node c_i onto its ancestor c_j, and this call
 * performs those that pay.  goals, nodes (-1: skip), span, the positions and w(i, j) are
 * pp_star_shortcut's; write m_i for the tree node of position i = 1 .. D (m_D the root).  Per
 * query, on the device, in f64 with every sum one addition: c[D] = 0; for i = D - 1 down to 1, cur
 * = c[i + 1] + edge_cost[m_i] (what m_i costs through its stored edge) and v = the first strict
 * minimum in increasing j of c[j] + w(i, j), j = i + 1 .. min(i + span, D); when v < cur (strict,
 * pp_star_extend's own rewire test) parent[m_i] = m_j, edge_cost[m_i] = w(i, j) and c[i] = v,
 * else c[i] = cur and the node keeps its stored edge, whatever w(i, i + 1) says: the call neither
 * verifies nor un-verifies a stored edge (like pp_star_extend on a tree that was not
 * revalidated).  cost_out[q] = the first strict minimum over j = 1 .. min(span, D) of c[j] +
 * w(0, j), node_out[q] = that m_j, n_rewired[q] = the chain nodes re-parented; -1, +inf and 0 when
 * nodes[q] is -1 (the query is untouched) or no goal edge is feasible (the chain's rewires are
 * committed all the same: the improvement is real).  Afterwards every node's cost is cost[parent]
 * + edge_cost again, parents before children (the invariant pp_star_forest_import checks): c[i]
 * on the chain, recomputed below it; a node without a changed ancestor keeps its cost bit for
 * bit, and no cost rises.  The query's rewire counter (pp_star_state) advances by n_rewired[q];
 * *n_changed = the nodes over the batch whose cost changed; *n_tested = pp_star_shortcut's pair
 * count.  Poses, node order, tree sizes, iteration counters, seeds, focus, node_evals and stats
 * are untouched, and later pp_star_extend calls continue from the committed trees exactly as from
 * an imported copy of them.  When every w(i, i + 1) equals the stored edge cost (an unchanged
 * scene), cost_out is pp_star_shortcut's cost and the tree chain from node_out is its row.
 * Errors: everything pp_star_shortcut checks on the host, before any launch (NULL goals or nodes,
 * span outside [1, 63], a non-finite goal, a node outside its tree: PP_ERR_INVALID_ARGUMENT;
 * PP_ERR_STATE without an RRT* batch or a scene); a chain deeper than 8192 nodes or more than
 * 2^26 pairs: PP_ERR_CAPACITY before any steer launch; PP_ERR_STEER_OVERFLOW leaves every tree
 * unchanged bit for bit.  node_out, cost_out, n_rewired (q entries each), n_tested and n_changed
 * may be NULL. */
int pp_star_shortcut_commit(pp_ctx* ctx, const double* goals, const int32_t* nodes, int span,
                            int32_t* node_out, double* cost_out, int32_t* n_rewired,
                            int64_t* n_tested, int64_t* n_changed);
/* pp_star_path_segments over caller-supplied chains: row i = goal -> chain[coff[i]] -> ... ->
 * chain[coff[i + 1] - 1] on query i's tree (coff: q + 1 entries, coff[0] = 0, not decreasing) —
 * pp_star_shortcut's rows, or any chain of tree nodes that ends in the root.  The words, the three
 * records per edge, reverse, length, ok, the sizes-only protocol and the errors are as there; an
 * empty chain row gives an empty row with ok 0.  A chain entry outside its tree, a row that does
 * not end in node 0, a row longer than 8192 nodes or a NULL coff or chain (with coff[q] > 0) is
 * PP_ERR_INVALID_ARGUMENT, checked on the host against the tree sizes.  No Space::verify is
 * repeated here.  With pp_segments_sample a shortened path becomes a trajectory. */
int pp_star_chain_segments(pp_ctx* ctx, const double* goals, const int64_t* coff,
                           const int32_t* chain, int reverse, int64_t* off,
                           const pp_path_segments* seg, int64_t cap, int64_t* n_total,
                           double* length, uint8_t* ok);

/* ------------------------------------- forest export / import (build-defined) */
/* The complete state of m query slots of a batch, packed: what a checkpoint, a move of a query to
 * another context or the recycling of a finished query's slot needs (CPU restatement of the
 * validation and the cost rebuild: tests/forest_state_ref.py).  A plain struct of caller-owned
 * arrays; `size` = sizeof(pp_forest_state) as the caller compiled it (fields past it read as
 * NULL).  Rows are CSR over the m served slots: slot i's tree is rows [off[i], off[i + 1]), root
 * first, in the tree's own node order.
 *   rows:      off (m + 1), x, y, yaw (f64), parent (int32, -1 for a tree's row 0),
 *              cost, edge_cost (f64; RRT* only, cost in pp_star_tree_export's unit)
 *   per slot:  iterations, seeds, node_evals (m each); RRT*: rewires, focus_xy (2m), focus_bound
 *              (m, +inf: no focus), skipped; the extend batch: goals (3m)
 * Arrays of the other batch kind are ignored by both directions. */
typedef struct pp_forest_state {
    uint64_t size;
    int64_t* off;
    double* x;
    double* y;
    double* yaw;
    int32_t* parent;
    double* cost;
    double* edge_cost;
    int64_t* iterations;
    uint64_t* seeds;
    int64_t* node_evals;
    int64_t* rewires;
    double* focus_xy;
    double* focus_bound;
    int64_t* skipped;
    double* goals;
} pp_forest_state;
/* Export the slots queries[0 .. m) (m distinct slots in any order; NULL: the slots 0 .. m - 1) of
 * the RRT* batch into *state.  Any pointer of *state may be NULL: that part is skipped.  Sizing as
 * pp_star_paths: with every row pointer (x, y, yaw, parent, cost, edge_cost) NULL or cap <= 0 the
 * call returns the sizes only — off, the per-slot arrays and *n_total = off[m] are filled, PP_OK;
 * cap < *n_total (cap: the rows each row array holds) is PP_ERR_CAPACITY with the same outputs
 * filled.  The rows are gathered and packed on the device into one staging buffer per array and
 * copied out once per array (into pageable memory); there is no per-query copy or synchronisation.
 * Nothing in the batch is modified.  PP_ERR_STATE without an RRT* batch; PP_ERR_INVALID_ARGUMENT
 * for a NULL state or n_total, a state->size that does not reach `off`, m outside [1, q], a slot
 * out of range or named twice. */
int pp_star_forest_export(pp_ctx* ctx, const int32_t* queries, int m, pp_forest_state* state,
                          int64_t cap, int64_t* n_total);
/* Write *state into the slots queries[0 .. m) of the RRT* batch; every other slot stays untouched
 * bit for bit.  Everything is validated before any row of the forest is written: a failed call
 * leaves the batch unchanged bit for bit and sets *bad_query (may be NULL) to the first offending
 * entry of `queries` (the slot number; with queries NULL, the index).
 *   On the host, before anything is launched: every pointer but `cost` present; distinct slots in
 *   range; off[0] = 0 and n_i = off[i + 1] - off[i] >= 1; iterations within [0, max_iter];
 *   n_i <= iterations_i + 1, else PP_ERR_CAPACITY (a tree has max_iter + 1 rows and may still
 *   insert max_iter - iterations nodes; a tree pruned below that is fine); node_evals, rewires and
 *   skipped >= 0; pp_coord_check of the positions; finite yaw; finite edge_cost >= 0;
 *   pp_star_set_focus' rules for the bound and the focus row; in polygon mode a tree of more than
 *   one node on a root that fails verify is refused (this library never grows one).
 *   On the device, one pass over the staged rows, one wave per tree: row 0 has parent -1; every
 *   other parent lies in [0, n_i) and is not the node itself; every chain ends in row 0 (no cycle,
 *   no island — decided level by level from the root, without assuming index order: a rewired
 *   node's parent may be a later node); cost[0] = 0 and cost[i] = cost[parent[i]] + edge_cost[i],
 *   rebuilt parents before children as one f64 addition each, uncontracted.  A `cost` the caller
 *   passed must equal the rebuilt values bit for bit (a damaged checkpoint fails here); with cost
 *   NULL the rebuilt values are stored.
 * All of these are PP_ERR_INVALID_ARGUMENT except the capacity.  Then the rows, counters, seeds,
 * focus state and the stored root (row 0's pose) are scattered into the slots, and what the
 * library derives for a slot is derived again: the polygon-mode blocked flag of the new root and
 * RRT*'s rewire scratch.  The outcome does not depend on what the slot held before.
 * Import trusts the edges, as pp_rrt_tree_import does: it neither steers nor verifies.  A tree
 * that comes from another scene: import, then pp_star_revalidate.
 * Unchanged: k, eta, step size, max_iter, pp_stats, the other slots, the scene.
 *
 * The guarantee.  Batch A of some size and batch B of any size, on the same scene, step size,
 * max_iter, k and eta: export any slots of A at any step and import them into any slots of B.
 * Under further extend / plan / focus / prune calls those slots of B evolve exactly as the slots of
 * A do: x, y, yaw, parent, cost, edge cost, iterations, skipped, evaluations and rewires are equal
 * bit for bit.  The queries are independent and the state is complete. */
int pp_star_forest_import(pp_ctx* ctx, const int32_t* queries, int m,
                          const pp_forest_state* state, int32_t* bad_query);
/* The same pair for the extend batch (pp_batch_new): rows x, y, yaw, parent; per slot iterations,
 * seeds, node_evals and goals.  Export accepts a batch that a scene change invalidated (stale);
 * import needs a valid one.  Import requires parent[i] < i for every row i > 0 (pp_rrt_tree_import's
 * rule; the extend never rewires), finite goals, and voids the slot's verdict cache.  The guarantee
 * above holds with the window in place of k and eta (the trees do not depend on it).  A tree from
 * another scene: import, then pp_batch_revalidate. */
int pp_batch_forest_export(pp_ctx* ctx, const int32_t* queries, int m, pp_forest_state* state,
                           int64_t cap, int64_t* n_total);
int pp_batch_forest_import(pp_ctx* ctx, const int32_t* queries, int m,
                           const pp_forest_state* state, int32_t* bad_query);

int pp_rrt_get_stats(pp_ctx* ctx, pp_stats* out, uint64_t out_size);
int pp_rrt_reset_stats(pp_ctx* ctx);
/* record HIP events around the hot kernels (adds a little host overhead per window) */
int pp_set_profiling(pp_ctx* ctx, int enabled);

#ifdef __cplusplus
}
#endif

#endif /* PATHPLANNING_AMD_H */

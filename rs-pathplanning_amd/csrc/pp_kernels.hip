// pp_kernels.hip — hand-written CDNA4 (gfx950) kernels beside the window pipeline: check_finish
// with the packed line export and the batch plan's rounds, the query batch, and the RRT* batch
// with its goal connection.  The window pipeline (and the overview of the whole extend path) is
// pp_k_window.hip.  steer_prep, steer_walk and the API kernels (steer_tasks, verify_lines,
// dubins_*) are compiled by pp_k_steer.hip alone and launched through pp_steer_launch.h; the
// device code the units inline is pp_steer_dev.h.
//
// No MFMA anywhere: there is no dense contraction on this path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "pp_kernels.h"

// check_finish_kernel's register budget needs the polygon S classes as a call (as its cf_prep).
// It is their only caller in this unit, and the inliner folds the last use of a local function
// in, so this unit's own declaration pins them out of line.  It has to precede the definition in
// pp_steer_dev.h (after it the compiler ignores the attribute, with a warning).
namespace ppamd {
template <bool kLds>
__device__ __noinline__ int s_classify_poly(const SceneDev& sc, double ax, double ay, double bx,
                                            double by, double t_lo, double t_hi, double dl);
}  // namespace ppamd

#include "pp_chain_dev.h"
#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

// ---------------------------------------------------------------- check_finish
//
// RRT::check_finish (rrt.rs:428-438) for a batch of tree nodes, ONE WAVE PER NODE (kCfWaves
// independent waves per workgroup, nodes from a launch-wide counter), the node's ancestor path
// root..node in the wave's region of a global path buffer (kCfMaxDepth ints per wave):
//   optimize (rrt.rs:463-487)   level i: candidates path[0..L] root first, steered + collided one
//                               at a time on the wave, the first accepted one wins (memoised per
//                               tree node in ftab); recursion = the next level on that ancestor;
//                               RECURSION_LIMIT 16.  Every candidate parent is a tree node, so
//                               verifying edge ++ [to] is verify(line_to_origin(new)) (§3.2).
//   finalize (rrt.rs:503-540)   the chain goal → optimised copies → tree path → root; every edge
//                               is verified with its junction chord, the edge into the root
//                               without one (the root contributes no point); a None steer is the
//                               reference's panic (rrt.rs:529).
//   length                      verified finishes: the edges' literal Dubins points, then
//                               euclidean_length of the reversed line summed in line order.
// (CfPose, cf_path and the pose providers: pp_chain_dev.h)
constexpr int kCfThreads = 64 * kCfWaves;

__device__ inline bool same_pose(const CfPose& a, const CfPose& b) {
    return __double_as_longlong(a.x) == __double_as_longlong(b.x) &&
           __double_as_longlong(a.y) == __double_as_longlong(b.y) &&
           __double_as_longlong(a.yaw) == __double_as_longlong(b.yaw);
}

// verify one edge a → b (+ junction chord to b unless junction is false) on one wave; kCfPanic
// when the steer is None (finalize's panic; verify_node's callers never pass such an edge here).
enum : int { kCfPanic = 6 };
// returns the verdict | (polyline points walked << 4) | (their arc points << 34)
// The edge's steer_prep runs on the wave's eight 8-lane groups (prep_task: the word choice across
// a group's lanes, ~9 transcendental calls deep instead of ~32 on one lane), every group on the
// same edge; group 0 writes the record to the wave's LDS slot lrec, which walk_rec then walks.
// ONE out-of-line body for both call sites, reading the scene through a device-memory pointer
// (round 4): a reference to the kernel-argument SceneDev would copy the struct to the stack, and
// inlined at two sites (round 3) the kernel sat at 256 VGPRs with 608 B/lane of scratch and 571
// SGPR spills (the literal call's save area) — 2 waves per SIMD.
// the edge's prep and walk as separate bodies: each gets its own register allocation under the
// kernel's budget (one inlined body held both chains' values at once)
__device__ __noinline__ void cf_prep(const SceneDev* __restrict__ scg, double ax, double ay,
                                     double ayaw, double bx, double by, double byaw,
                                     PrepRec* lrec) {
    const int lane = __lane_id();
    prep_task(*scg, lane & 7, lane & ~7, 0, lane < 8, true, ax, ay, bx, by, byaw, 1, ayaw, 0,
              0.0, 0.0, lrec, nullptr, nullptr);
}
// (the walked point tallies go to the wave's LDS slot `tally`: reference out-parameters would
// live in the caller's stack frame, i.e. scratch)
__device__ __forceinline__ int cf_walk(const SceneDev* __restrict__ scg, const PrepRec* lrec,
                                    double* gs, bool junction, int* tally) {
    int w = 0, wa = 0;
    const int st = walk_rec<false, kSceneAny, true>(*scg, lrec, gs, w, wa, junction);
    if (__lane_id() == 0) {
        tally[0] = w;
        tally[1] = wa;
    }
    return st;
}
__device__ __forceinline__ long long cf_edge_check(const SceneDev* __restrict__ scg, double ax,
                                                double ay, double ayaw, double bx, double by,
                                                double byaw, int flags, double* lit_scratch,
                                                int* lit_locks, double* gs, PrepRec* lrec) {
    const SceneDev& sc = *scg;
    const bool junction = flags & 1, allow_none = flags & 2;
    cf_prep(scg, ax, ay, ayaw, bx, by, byaw, lrec);
    __builtin_amdgcn_wave_barrier();
    if (!allow_none && ufl(lrec->state) == kPrepNone) return kCfPanic;
    // (lrec's fb_seg / cnt[0] are dead once the walk started: its tallies come back there)
    int* tally = &lrec->cnt[0];
    int st = cf_walk(scg, lrec, gs, junction, tally);
    __builtin_amdgcn_wave_barrier();
    const long long walked = ufl(tally[0]), walked_arc = ufl(tally[1]);
    if (st == kLiteral) {  // (measure-zero) a scratch buffer from the pool, for this edge only
        const int slot = lit_acquire(lit_locks, (int)blockIdx.x);
        double* sx = lit_scratch + (size_t)slot * 3 * kLiteralCap;
        st = steer_collide_literal(sc, ax, ay, ayaw, bx, by, byaw, sx, sx + kLiteralCap,
                                   sx + 2 * kLiteralCap, junction);
        lit_release(lit_locks, slot);
    }
    return (long long)st | (walked << 4) | (walked_arc << 34);
}

// compute_yaw out of line: check_finish_kernel's own body is bookkeeping, and an inlined ocml
// atan2 (its polynomial constants hoisted out of the item loop) held ~100 VGPRs live across the
// edge calls
__device__ __noinline__ double cf_atan2(double y, double x) { return atan2(y, x); }

// n_point of dubins_path_planning(a → b) (dubins.rs:369), 0 when the steer is None; the chosen
// word in st
__device__ inline int cf_npoint_steer(const SceneDev& sc, CfPose a, CfPose b, Steer& st) {
    const double ex = b.x - a.x, ey = b.y - a.y;
    const double c = 1.0 / sc.turn_radius;
    const double lex = cos(a.yaw) * ex + sin(a.yaw) * ey;
    const double ley = -(sin(a.yaw)) * ex + cos(a.yaw) * ey;
    st = select_word(lex, ley, b.yaw - a.yaw, c);
    if (st.word < 0) return 0;
    double tot = 0.0;
    tot += st.t;
    tot += st.p;
    tot += st.q;
    const double nq = trunc(tot / sc.step_size);
    if (!(nq >= 0.0) || nq > 1.0e8) return -1;
    return (int)nq + 7;
}
__device__ inline int cf_npoint(const SceneDev& sc, CfPose a, CfPose b) {
    Steer st;
    return cf_npoint_steer(sc, a, b, st);
}

__device__ __noinline__ int cf_npoint_ool(const SceneDev* __restrict__ scg, CfPose a, CfPose b) {
    return cf_npoint(*scg, a, b);
}

// mode kCfCheck: check_finish of nodes[b] (the goal node Node::new_goal(goal, node, gyaw));
// kCfOptimize: optimize(nodes[b], level0) alone (ok_out: Some, chain_out: the chosen ancestors);
// kCfFinalize: finalize of the goal node (gx, gy, gyaw) with parent nodes[b] — the line is built
// whether it verifies or not (ok_out: it does).  optimize_from_goal gives the goal gyaw_opt when
// optimize succeeds (rrt.rs:489-501: the planner's goal yaw), else the goal node keeps gyaw.
// cb.qidx != nullptr (a query batch, pp_batch_plan): work item b is node nodes[b] of query
// qidx[b], whose tree is rows [q * row_cap, ...) of the SoA arrays and whose goal (both yaws) is
// goals[3q..3q+2]; its polygon-mode root block flag is blocked[q].
//
// Two launches.  check_finish_kernel: ONE WAVE PER NODE — the waves of a workgroup are
// independent (no barrier): each takes nodes from a launch-wide counter and runs optimize and
// finalize's verification edge by edge, in the reference's own order, so no edge is steered
// speculatively (the r02 form checked four candidates at a time across the workgroup's waves and
// discarded the ones past the first accept; it also held the workgroup at a barrier per round).
// A node whose line is wanted (a verified finish, or kCfFinalize) becomes a line item; the
// points and the length of the line items are cf_line_kernel's, one workgroup per item.
__device__ inline void cf_node_setup(const TreeDev& tr_in, const CfBatch& cb, int b,
                                     double gx_in, double gy_in, double gyaw_in,
                                     double gyaw_opt_in, int root_blocked_in, TreeDev& tr,
                                     double& gx, double& gy, double& gyaw, double& gyaw_opt,
                                     int& root_blocked, int** ftab = nullptr,
                                     int** gtab = nullptr) {
    tr = tr_in;
    if (ftab) *ftab = cb.ftab;
    if (gtab) *gtab = cb.gtab;
    gx = gx_in;
    gy = gy_in;
    gyaw = gyaw_in;
    gyaw_opt = gyaw_opt_in;
    root_blocked = root_blocked_in;
    if (cb.qidx) {
        const int q = cb.qidx[b];
        const size_t o = (size_t)q * cb.row_cap;
        tr.x += o;
        tr.y += o;
        tr.yaw += o;
        tr.parent += o;
        gx = cb.goals[3 * q];
        gy = cb.goals[3 * q + 1];
        gyaw = gyaw_opt = cb.goals[3 * q + 2];
        root_blocked = cb.blocked ? cb.blocked[q] : 0;
        // the memo rows are compact: query q's n_q nodes at mo(q) = its items before + q
        const size_t m = cb.moff ? (size_t)cb.moff[q] + q : o;
        if (ftab && *ftab) *ftab += m;
        if (gtab && *gtab) *gtab += m;
    }
}

__global__ __launch_bounds__(kCfThreads, kCfMinW) void check_finish_kernel(
    const SceneDev* __restrict__ scg, TreeDev tr_in, const int* __restrict__ nodes, int k, double gx_in, double gy_in,
    double gyaw_in, double gyaw_opt_in, int level0, int mode, int want_line,
    int* __restrict__ ok_out, double* __restrict__ len_out,
    int* __restrict__ npts_out, int* __restrict__ chain_out, double* __restrict__ lit_scratch,
    int* __restrict__ lit_locks, int* __restrict__ err, long long* __restrict__ tally, CfBatch cb,
    int* __restrict__ gpath, int* __restrict__ items, const int* __restrict__ blist) {
    __shared__ __attribute__((aligned(16))) double s_gs[kCfWaves][kGenSlots];  // walk_rec's LDS, one set per wave
    __shared__ int s_pos[kCfWaves][kCfLevels];  // the optimize chain's path positions per wave
    __shared__ PrepRec s_rec[kCfWaves];          // the wave's edge record (cf_edge_check)
    const SceneDev& sc = *scg;
    const int lane = __lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int* path = gpath + ((size_t)blockIdx.x * kCfWaves + wave) * kCfMaxDepth;  // this wave's
    double* gs = s_gs[wave];
    int* pos = s_pos[wave];
    PrepRec* lrec = &s_rec[wave];
    long long t_nodes = 0, t_edges = 0, t_pts = 0, t_arc = 0;  // this wave's work (profiling)
    for (;;) {
        // nodes one at a time from a launch-wide counter (err[1], zeroed with err): a node's
        // cost varies with its depth and how far optimize climbs
        int b = 0;
        if (lane == 0) b = atomicAdd(&err[1], 1);
        b = __builtin_amdgcn_readfirstlane(__shfl(b, 0));
        if (b >= k) break;
        if (blist) b = __builtin_amdgcn_readfirstlane(blist[b]);  // (a sub-list of the items)
        ++t_nodes;
        TreeDev tr;
        double gx, gy, gyaw, gyaw_opt;
        int root_blocked;
        int *ftab = nullptr, *gtab = nullptr;
        cf_node_setup(tr_in, cb, b, gx_in, gy_in, gyaw_in, gyaw_opt_in, sc.root_blocked, tr, gx,
                      gy, gyaw, gyaw_opt, root_blocked, &ftab, &gtab);
        const int D = cf_path(tr, nodes[b], path);
        if (D < 0) {
            if (lane == 0) {
                ok_out[b] = 0;
                atomicOr(err, 1);
            }
            continue;
        }
        // optimize (rrt.rs:463-487), level by level: candidates path[0..L] root first, the first
        // accepted one wins (kError before it: the reference's panic); RECURSION_LIMIT levels
        // The first verifying candidate of a tree node c (root first over c's ancestors and c)
        // depends on c alone — its ancestors' poses — not on the item whose chain reaches it, and
        // every item of a plan climbs through its ancestors' own levels: ftab memoises it
        // (cb.ftab; the value is the candidate's depth, which is its position in every path through
        // c).  Concurrent waves computing the same entry store the same value.
        int bad = 0;
        int L = D - 1, s_lv = 0;
        int fnone = 0;  // the last accepted candidate edge's steer was None (finalize panics)
        for (int level = 0; level < kCfLevels - level0; ++level) {
            const int Lstart = L;
            const int c = path[L];
            const int fm = ftab ? __builtin_amdgcn_readfirstlane(ftab[c]) : 0;
            int found = -1;
            if (fm >= 2) {
                found = fm & 0x3fffffff;
                found -= 2;
                fnone = fm >> 30;
            } else if (fm == 0) {
                const double ax = tr.x[c], ay = tr.y[c];
                for (int m = 0; m <= L && !root_blocked; ++m) {
                    const int to = path[m];
                    const CfPose bt{tr.x[to], tr.y[to], tr.yaw[to]};
                    const CfPose a{ax, ay, cf_atan2(bt.y - ay, bt.x - ax)};
                    const long long rv = cf_edge_check(scg, a.x, a.y, a.yaw, bt.x, bt.y, bt.yaw,
                                                       3, lit_scratch, lit_locks, gs, lrec);
                    const int st = (int)(rv & 15);
                    ++t_edges;
                    t_pts += (rv >> 4) & 0x3fffffff;
                    t_arc += rv >> 34;
                    if (st == kReject) continue;
                    found = st == kAccept ? m : -2;
                    fnone = lrec->state == kPrepNone ? 1 : 0;
                    break;
                }
                if (ftab && lane == 0 && found != -2)
                    ftab[c] = found >= 0 ? (2 + found) | (fnone << 30) : 1;
            }
            if (found == -2) {
                bad = 4;
                break;
            }
            if (found < 0) break;
            if (lane == 0) pos[level] = found;
            __builtin_amdgcn_wave_barrier();
            L = found;
            s_lv = level + 1;
            if (Lstart == 0) {
                // a level at the root tried its one candidate, the root copy (yaw atan2(0, 0))
                // into the root itself, and accepted it: every further level is the very same
                // edge with the same verdict — the chain of root copies
                // runs to the recursion limit
                if (lane == 0)
                    for (int l2 = level + 1; l2 < kCfLevels - level0; ++l2) pos[l2] = 0;
                __builtin_amdgcn_wave_barrier();
                s_lv = kCfLevels - level0;
                break;
            }
        }
        if (mode == kCfOptimize) {
            if (lane == 0) {
                ok_out[b] = (bad == 0 && s_lv > 0) ? 1 : 0;
                len_out[b] = 0.0;
                npts_out[b] = 0;
                if (bad) atomicOr(err, bad);
                if (chain_out) {
                    chain_out[(size_t)b * (kCfLevels + 2)] = s_lv;
                    chain_out[(size_t)b * (kCfLevels + 2) + 1] = 0;
                    for (int i = 0; i < s_lv; ++i)
                        chain_out[(size_t)b * (kCfLevels + 2) + 2 + i] = path[pos[i]];
                }
            }
            continue;
        }
        // finalize (rrt.rs:503-540): the chain goal -> optimised copies -> tree path -> root,
        // every edge verified with its junction chord, the edge into the root without one
        const int s = s_lv;
        const double gyaw_e = s > 0 ? gyaw_opt : gyaw;  // optimize_from_goal (rrt.rs:489-501)
        const int ps = s > 0 ? pos[s - 1] : D - 1;
        const int E = 1 + s + ps;
        bool vok = bad == 0;
        // pose j of the chain (cf_pose's indexing, the chain positions in registers)
        auto pose = [&](int j) -> CfPose {
            if (j == 0) return CfPose{gx, gy, gyaw_e};
            if (j <= s) {
                const int i = j - 1;
                const int here = path[i == 0 ? D - 1 : pos[i - 1]];
                const int to = path[pos[i]];
                const double x = tr.x[here], y = tr.y[here];
                return CfPose{x, y, cf_atan2(tr.y[to] - y, tr.x[to] - x)};  // Node::new (compute_yaw)
            }
            const int node = path[ps - (j - s - 1)];
            return CfPose{tr.x[node], tr.y[node], tr.yaw[node]};
        };
        // Only the goal edge and the s copy edges are steered: edges s + 1 .. E - 1 are tree edges
        // (node -> parent, both with their stored poses) whose polyline with its junction chord
        // passed verify when the node was inserted (verify_node, rrt.rs:414-426: the incremental
        // form, §2), and the edge into the root is checked without its chord, a subset.  Both
        // Contains and Intersects decompose over the concatenation, so those edges cannot change
        // the verdict (tests: every check_finish verdict equals the oracle's full-line verify).
        // Edge s (the last copy into the tree node optimize's last level accepted) is that
        // level's candidate edge: it verified with its junction chord (without the chord, into
        // the root, a subset), so only its None steer matters (finalize's panic; fnone).  Copy
        // edge e in 1..s-1 runs from the copy at chain node v = path[pos[e - 2]] (the item's node
        // for e = 1) toward F(v) to the copy at F(v) toward F(F(v)): a function of v alone, so
        // gtab memoises its verdict like ftab.
        const int Ev = 1 + s;
        if (vok) {
            CfPose prev{0.0, 0.0, 0.0}, a = pose(0);
            int prev_st = kAccept;
            for (int e = 0; e < Ev; ++e) {
                const CfPose bp = pose(e + 1);
                // an edge identical to the previous one (consecutive root copies: both poses
                // equal bit for bit, both with the junction) has that edge's verdict
                const bool dup = e >= 1 && e < E - 1 && same_pose(prev, a) && same_pose(a, bp);
                const int gv = (e >= 1 && e < s) ? path[e == 1 ? D - 1 : pos[e - 2]] : -1;
                // the goal edge's verdict from the batch plan's steer round (cb.gotab), the copy
                // edges' from gtab
                const int gm = (e == 0 && cb.gotab)
                                   ? __builtin_amdgcn_readfirstlane(cb.gotab[b])
                                   : ((gtab && gv >= 0) ? __builtin_amdgcn_readfirstlane(gtab[gv]) : 0);
                int st = prev_st;
                if (e >= 1 && e == s) {
                    st = fnone ? kCfPanic : kAccept;
                } else if (gm > 0) {
                    st = gm - 1;
                } else if (!dup) {
                    const long long rv = cf_edge_check(scg, a.x, a.y, a.yaw, bp.x, bp.y, bp.yaw,
                                                       e < E - 1 ? 1 : 0, lit_scratch, lit_locks,
                                                       gs, lrec);
                    st = (int)(rv & 15);
                    ++t_edges;
                    t_pts += (rv >> 4) & 0x3fffffff;
                    t_arc += rv >> 34;
                    if (gtab && gv >= 0 && lane == 0) gtab[gv] = st + 1;
                }
                if (st != kAccept) {
                    if (st == kCfPanic) bad = 2;
                    else if (st == kError) bad = 4;
                    vok = false;
                    break;
                }
                prev = a;
                a = bp;
                prev_st = st;
            }
        }
        // polygon mode: the chain's line is connected and no segment met an edge buffer, so it
        // lies on one side of every obstacle boundary — the goal decides (Q10p)
        if (vok && sc.ne > 0 && in_obstacle(sc.ne, sc.ex0, sc.ey0, sc.ex1, sc.ey1, sc.epoly, gx, gy))
            vok = false;
        // a panic anywhere in finalize wins over a rejection (the reference builds the whole line
        // before it verifies): the other edges' steers, lane-parallel.  A verified chain also
        // scans its tree edges s + 1 .. E - 1, which were not steered above: insertion accepts a
        // None steer as the straight polyline (rrt.rs:313), finalize panics on it (rrt.rs:529).
        // (None needs a non-finite pose — LSL's and RSR's p² differ only in the sign of one
        // term, so one of them is >= 0 — e.g. a NaN start yaw; only finishes pay the scan.)
        if (bad == 0 && (!vok || E > Ev)) {
            bool none = false;
            for (int e = (vok ? Ev : 0) + lane; e < E; e += 64)
                if (cf_npoint_ool(scg, pose(e), pose(e + 1)) == 0) none = true;
            if (__any(none)) bad = 2;
        }
        if ((vok || mode == kCfFinalize) && bad == 0 && want_line) {
            // the line's points and length: a cf_line_kernel item
            if (lane == 0) {
                const int it = atomicAdd(&items[0], 1);
                int* o = items + 1 + (size_t)it * kCfItem;
                o[0] = b;
                o[1] = s;
                o[2] = vok ? 1 : 0;
                o[3] = 0;
                for (int i = 0; i < kCfLevels; ++i) o[4 + i] = i < s ? pos[i] : 0;
            }
        } else if (lane == 0) {
            ok_out[b] = (vok && bad == 0) ? 1 : 0;
            len_out[b] = 0.0;
            npts_out[b] = 0;
            if (bad) atomicOr(err, bad);
        }
        if (lane == 0 && chain_out) {
            chain_out[(size_t)b * (kCfLevels + 2)] = s;
            chain_out[(size_t)b * (kCfLevels + 2) + 1] = E;
            for (int i = 0; i < s; ++i)
                chain_out[(size_t)b * (kCfLevels + 2) + 2 + i] = path[pos[i]];
        }
    }
    if (tally && lane == 0) {  // profiling: nodes, edges, points
        unsigned long long* tl = reinterpret_cast<unsigned long long*>(tally);
        atomicAdd(&tl[0], (unsigned long long)t_nodes);
        atomicAdd(&tl[1], (unsigned long long)t_edges);
        atomicAdd(&tl[2], (unsigned long long)t_pts);
        atomicAdd(&tl[3], (unsigned long long)t_arc);
    }
}

// cf_line_kernel's workgroup: one wave per line item.  An item's path walk and its ordered length
// sum are serial, so a 4-wave workgroup left 3 waves waiting at its barriers; one wave per item
// puts 4x the items in flight at the same occupancy
constexpr int kCfLineThreads = 64;
static_assert(kCfLineThreads == 64, "cf_line_kernel: one wave per item (its edge table and sums are wave-wide)");
#ifdef PP_LINE_TIMING  // diagnostic builds only: phase stamps of cf_line_kernel's items
#define LT(k) const unsigned long long lt##k = wall_clock64();
#else
#define LT(k)
#endif

// dubins_literal<false, false> (dubins.rs:326-428) of one edge by one wave: the WORLD points of
// the trimmed course into px / py (cap >= n_point), *n_out = their count.  generate_local_course
// (dubins.rs:200-272) writes the origin at index 0, each segment's grid points from the slot of
// the previous segment's end on (that end is overwritten), and the last segment's end after its
// grid points; the rest of the n_point slots stay 0.0.  The grid values of a segment are the
// serial chain pd, pd + d, ... (every lane runs the uniform chain and keeps its own term, the
// same rounding sequence), 64 per pass; each lane interpolates its point (dubins.rs:155-198) and
// moves it to the world frame (dubins.rs:412-422).  The trim (dubins.rs:281-288) keeps the
// indices below the last one whose local x is nonzero (none: 0), or all n_point when the last
// slot is written and nonzero.  Returns kSteerSome / kSteerNone / kSteerOverflow like the
// literal restatement.
// kCount: the kept count alone — nothing is stored (px / py / cap unused), so an edge of up to
// 2e9 steps is counted where the storing form stops at 1e8 steps and at its buffer: finalize's
// answer for a goal too far for the line buffer (the same chain of values, the same trim).
template <bool kCount = false>
__device__ int line_edge_wave(double sx, double sy, double syaw, const double* __restrict__ word,
                              double turn_radius, double step_size, double* px, double* py,
                              int cap, int lane, int* n_out) {
    // the word (dubins.rs:333-363) as cf_npoint_steer chose it for this edge: {word, t, p, q}
    const double c = 1.0 / turn_radius;
    const double rc = 1.0 / c;
    Steer s;
    s.word = (int)word[0];
    s.t = word[1];
    s.p = word[2];
    s.q = word[3];
    if (s.word < 0) return kSteerNone;
    const double lengths[3] = {s.t, s.p, s.q};
    double total = 0.0;
    total += s.t;
    total += s.p;
    total += s.q;
    const double nq = trunc(total / step_size);
    if (!(nq >= 0.0) || nq > (kCount ? 2.0e9 : 1.0e8)) return kSteerOverflow;
    const int n_point = (int)nq + 3 + 4;
    if (!kCount && n_point > cap) return kSteerOverflow;
    // every sin / cos the edge needs in one lane-parallel round (the same calls on the same
    // arguments as interp_local and the world transform make, so the same values): lanes 0..2 the
    // segment origins' yaw trig (S: cos / sin of the yaw; L, R: of minus the yaw), 3..5 sin / cos
    // of the segment lengths (their end points), 6 the world transform's cos / sin(-syaw)
    const int m0 = word_mode(s.word, 0), m1 = word_mode(s.word, 1), m2 = word_mode(s.word, 2);
    const double oy0 = 0.0;  // interpolate's yaw chain, dubins.rs:191-196
    const double oy1 = m0 == kModeL ? oy0 + s.t : (m0 == kModeR ? oy0 - s.t : oy0);
    const double oy2 = m1 == kModeL ? oy1 + s.p : (m1 == kModeR ? oy1 - s.p : oy1);
    double arg = 0.0;
    if (lane < 3) {
        const int ms = lane == 0 ? m0 : (lane == 1 ? m1 : m2);
        const double oys = lane == 0 ? oy0 : (lane == 1 ? oy1 : oy2);
        arg = ms == kModeS ? oys : -oys;
    } else if (lane < 6) {
        arg = lane == 3 ? s.t : (lane == 4 ? s.p : s.q);
    } else if (lane == 6) {
        arg = -syaw;
    }
    const double sv = sin(arg), cv = cos(arg);
    const double cs = readlane_f64(cv, 6), sn = readlane_f64(sv, 6);
    if (!kCount && lane == 0) {  // the origin, index 0
        px[0] = cs * 0.0 + sn * 0.0 + sx;
        py[0] = -sn * 0.0 + cs * 0.0 + sy;
    }
    int ind = 0;      // the last index written
    int lastnz = -1;  // the last index whose local x is nonzero
    double lastx = 0.0;
    Pose o{0.0, 0.0, 0.0};
    double ll = 0.0;
    for (int i = 0; i < 3; ++i) {
        const int m = word_mode(s.word, i);
        const double l = lengths[i];
        const double d = (l > 0.0) ? step_size : -step_size;
        // interp_local's trig of the segment's origin yaw (per point in the serial form, the same
        // values): S cos / sin(yaw), L / R cos / sin(-yaw)
        const double ca = readlane_f64(cv, i), sa = readlane_f64(sv, i);
        const double co = ca, so = sa, cmo = ca, smo = sa;
        const double al = fabs(l);
        double pd = (i >= 1 && (lengths[i - 1] * lengths[i]) > 0.0) ? (-d - ll) : (d - ll);
        int base = i == 0 ? 1 : ind;  // the slot of this segment's first grid point
        ind = base - 1;               // (dubins.rs:227: ind -= 1)
        for (;;) {
            double my = 0.0, w = pd;
            // walk_rec's closed form first: while the values keep pd's sign and exponent,
            // fl(w + d) = w + delta exactly (delta = w1 - pd, when the first two steps agree), so
            // lane k's value is one exact fma; checked over every value up to the first one past
            // |l| (the one the segment end needs).  Otherwise the serial chain.
            const double w1 = pd + d, w2 = w1 + d;
            bool cf = (w1 - pd) == (w2 - w1);
            if (cf) {
                const double vc = __builtin_fma((double)lane, w1 - pd, pd);
                const uint64_t fm = __ballot(!(fabs(vc) <= al));
                const int fl = fm ? (int)__builtin_ctzll(fm) : 63;
                cf = __ballot(lane <= fl && (__double2hiint(vc) >> 20) != (__double2hiint(pd) >> 20)) == 0;
                if (cf) {
                    my = vc;
                    w = readlane_f64(vc, 63) + d;
                }
            }
            if (!cf) {
                for (int u = 0; u < 64; ++u) {
                    if (lane == u) my = w;
                    w += d;
                }
            }
            const uint64_t bad = __ballot(!(fabs(my) <= al));
            const int cnt = bad ? (int)__builtin_ctzll(bad) : 64;
            if (cnt > 0 && base + cnt - 1 >= n_point) return kSteerOverflow;
            if (lane < cnt) {
                // (x / c as div_by: the correctly rounded quotient, bit-identical to the division)
                double lx, ly;
                if (m == kModeS) {
                    lx = o.x + div_by(my, c, rc) * co;
                    ly = o.y + div_by(my, c, rc) * so;
                } else {
                    const double ldx = div_by(sin(my), c, rc);
                    const double l1 = div_by(1.0 - cos(my), c, rc);
                    const double ldy = m == kModeL ? l1 : -l1;
                    lx = o.x + (cmo * ldx + smo * ldy);
                    ly = o.y + (-smo * ldx + cmo * ldy);
                }
                if (!kCount) {
                    px[base + lane] = cs * lx + sn * ly + sx;
                    py[base + lane] = -sn * lx + cs * ly + sy;
                }
                const uint64_t nz = __ballot(lx != 0.0);
                if (nz) lastnz = base + 63 - (int)__builtin_clzll(nz);
                lastx = lx;
            }
            if (cnt > 0) {
                ind = base + cnt - 1;
                lastx = readlane_f64(lastx, cnt - 1);
            }
            if (cnt < 64) {
                ll = l - readlane_f64(my, cnt) - d;
                break;
            }
            base += 64;
            pd = w;
        }
        // the segment's end (dubins.rs:262-267) at the next slot; the next segment starts there
        ind += 1;
        if (ind >= n_point) return kSteerOverflow;
        // interp_local(m, l, c, o) with the round's values
        Pose r;
        if (m == kModeS) {
            r.x = o.x + l / c * co;
            r.y = o.y + l / c * so;
        } else {
            const double sl = readlane_f64(sv, 3 + i), cl = readlane_f64(cv, 3 + i);
            const double ldx = sl / c;
            const double ldy = m == kModeL ? (1.0 - cl) / c : (1.0 - cl) / -c;
            r.x = o.x + (cmo * ldx + smo * ldy);
            r.y = o.y + (-smo * ldx + cmo * ldy);
        }
        r.yaw = 0.0;  // (the next segment's trig comes from the round)
        if (i == 2) {
            if (!kCount && lane == 0) {
                px[ind] = cs * r.x + sn * r.y + sx;
                py[ind] = -sn * r.x + cs * r.y + sy;
            }
            if (r.x != 0.0) lastnz = ind;
            lastx = r.x;
        }
        o = r;
    }
    // the trim: every trailing 0.0 (the unwritten slots) and one more element
    *n_out = (ind == n_point - 1 && lastx != 0.0) ? n_point : (lastnz > 0 ? lastnz : 0);
    return kSteerSome;
}

// The lines of check_finish_kernel's line items: workgroup w takes items w, w + grid, ... (item
// i < grid: the workgroup-i buffers, so a one-node call's line is in workgroup 0's); every
// edge's literal Dubins points (line_edge_wave, a wave per edge) into the workgroup's pts / etab,
// then l.reverse() and geo's euclidean_length in that order (rrt.rs:538: the hypots in parallel,
// their sum in line order).
// a line item past tier 1's capacities onto the spill list (all 64 lanes of the item's wave)
// (past the list's capacity: the point-capacity error)
__device__ inline void cf_spill(const CfLineBufs& lb, const int* __restrict__ o, int tid,
                                int* __restrict__ err) {
    int w = 0;
    if (tid == 0) w = atomicAdd(&lb.spill[0], 1);
    w = __shfl(w, 0);
    if (w >= lb.spill_cap) {
        if (tid == 0) atomicOr(err, 8);
    } else if (tid < kCfItem) {
        lb.spill[1 + (size_t)w * kCfItem + tid] = o[tid];
    }
}

// kCountLong (finalize's one-node launch only: the instantiation the plans run has none of it):
// an unverified line too long for the buffer at the full capacity is counted instead of stored.
template <bool kCountLong>
__global__ __launch_bounds__(kCfLineThreads) void cf_line_kernel(
    SceneDev sc, TreeDev tr_in, const int* __restrict__ nodes, double gx_in, double gy_in,
    double gyaw_in, double gyaw_opt_in, int* __restrict__ ok_out, double* __restrict__ len_out,
    int* __restrict__ npts_out, CfLineBufs lb, int* __restrict__ err, CfBatch cb,
    const int* __restrict__ items) {
    __shared__ int s_off, s_bad, s_count;
    __shared__ int s_pos[kCfLevels];
    const int tid = threadIdx.x;
    // this workgroup's buffers: points (x, y, hypots / words), edge table, ancestor path
    const int pts_cap = lb.pts_cap;
    double* px = lb.pts + (size_t)blockIdx.x * 3 * pts_cap;
    double* py = px + pts_cap;
    double* pyw = py + pts_cap;
    int* et = lb.etab + (size_t)blockIdx.x * 2 * (lb.path_cap + kCfLevels + 1);
    int* path = lb.path + (size_t)blockIdx.x * lb.path_cap;
    const int n_items = items[0];
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int* o = items + 1 + (size_t)it * kCfItem;
        const int b = o[0], s = o[1], vok = o[2];
        LT(0)
        if (tid < kCfLevels) s_pos[tid] = o[4 + tid];
        const int* pos = s_pos;
        TreeDev tr;
        double gx, gy, gyaw, gyaw_opt;
        int root_blocked;
        cf_node_setup(tr_in, cb, b, gx_in, gy_in, gyaw_in, gyaw_opt_in, sc.root_blocked, tr, gx,
                      gy, gyaw, gyaw_opt, root_blocked);
        int D = 0;
        if (tid < 64) D = cf_path(tr, nodes[b], path, lb.path_cap);
        if (tid == 0) s_off = D;
        __syncthreads();
        D = s_off;
        // tier 1: a path deeper than this tier's capacity goes to tier 2 (the spill list); at the
        // full capacity it is check_finish_kernel's depth error
        if (D < 0) {
            if (lb.spill) {
                cf_spill(lb, o, tid, err);
            } else if (tid == 0) {
                ok_out[b] = 0;
                atomicOr(err, 1);
            }
            __syncthreads();
            continue;
        }
        LT(1)
        const double gyaw_e = s > 0 ? gyaw_opt : gyaw;
        const int ps = s > 0 ? pos[s - 1] : D - 1;
        const int E = 1 + s + ps;
        auto pose = [&](int j) -> CfPose {
            if (j == 0) return CfPose{gx, gy, gyaw_e};
            if (j <= s) {
                const int i = j - 1;
                const int here = path[i == 0 ? D - 1 : pos[i - 1]];
                const int to = path[pos[i]];
                const double x = tr.x[here], y = tr.y[here];
                return CfPose{x, y, atan2(tr.y[to] - y, tr.x[to] - x)};
            }
            const int node = path[ps - (j - s - 1)];
            return CfPose{tr.x[node], tr.y[node], tr.yaw[node]};
        };
        if (tid == 0) {
            s_bad = 0;
            if (kCountLong) s_count = 0;
        }
        // every edge's word and point count, a lane per edge; the words wait in the hypot buffer
        // (4 doubles an edge, 4 kCfMaxEdges <= pts_cap) for the generation below
        for (int e = tid; e < E; e += kCfLineThreads) {
            Steer w;
            et[2 * e] = cf_npoint_steer(sc, pose(e), pose(e + 1), w);
            double* wd = pyw + 4 * (size_t)e;
            wd[0] = (double)w.word;
            wd[1] = w.t;
            wd[2] = w.p;
            wd[3] = w.q;
        }
        __syncthreads();
        if (tid == 0) {  // edge capacities -> offsets
            int off = 0;
            bool none = false, neg = false;
            for (int e = 0; e < E; ++e) {
                const int c = et[2 * e];
                none |= c == 0;
                neg |= c < 0;
                et[2 * e] = off;
                off += c > 0 ? c : 0;
            }
            // a None steer is finalize's panic (rrt.rs:529); an overflowing count or a line
            // past the point capacity is the capacity error — in tier 1, a line longer than the
            // tier's capacity goes to tier 2 (-3)
            s_off = none ? -2 : neg ? -1 : off <= pts_cap ? off : lb.spill ? -3 : -1;
        }
        __syncthreads();
        const int total = s_off;
        LT(2)
        if (total == -3) {  // spilled: tier 2 writes this item's outputs
            cf_spill(lb, o, tid, err);
            __syncthreads();
            continue;
        }
        if (kCountLong && total == -1 && !vok && !lb.spill) {
            // finalize's unverified line, too long for the buffer at the full capacity (a goal
            // far outside the scene): its points are counted, not stored — no length, error bit
            // 32 tells the host that the line itself is not there
            const int lane = tid & 63;
            for (int e = tid >> 6; e < E; e += kCfLineThreads / 64) {
                const CfPose a = pose(e);
                int n = 0;
                const int r = line_edge_wave<true>(a.x, a.y, a.yaw, pyw + 4 * (size_t)e,
                                                   sc.turn_radius, sc.step_size, nullptr, nullptr,
                                                   0, lane, &n);
                if (lane == 0) {
                    et[2 * e + 1] = r == kSteerSome ? n : 0;
                    if (r == kSteerNone) atomicOr(&s_bad, 2);
                    else if (r != kSteerSome) atomicOr(&s_bad, 4);
                }
            }
            if (tid == 0) s_count = 1;
        } else if (total < 0) {
            if (tid == 0) s_bad = total == -2 ? 2 : 8;
        } else {
            const int lane = tid & 63;
            for (int e = tid >> 6; e < E; e += kCfLineThreads / 64) {
                const int off = et[2 * e];
                const int cap = (e + 1 < E ? et[2 * e + 2] : total) - off;
                const CfPose a = pose(e);
                int n = 0;
                const int r = line_edge_wave(a.x, a.y, a.yaw, pyw + 4 * (size_t)e, sc.turn_radius,
                                             sc.step_size, px + off, py + off, cap, lane, &n);
                if (lane == 0) {
                    et[2 * e + 1] = r == kSteerSome ? n : 0;
                    // a None steer is finalize's panic (rrt.rs:529); an n_point overflow is the
                    // steer-overflow error (round 5 reported both as the panic)
                    if (r == kSteerNone) atomicOr(&s_bad, 2);
                    else if (r != kSteerSome) atomicOr(&s_bad, 4);
                }
            }
        }
        __syncthreads();
        // l.reverse() (rrt.rs:538), then euclidean_length in that order: the line's points in
        // forward order f = 0 .. np - 1 (edge by edge), the reversed line's k-th segment is
        // (f + 1 -> f) for f = np - 2 down to 0.  Every segment's hypot in parallel (into the
        // yaw buffer, by forward index), then one lane adds them in the reversed order — the
        // same operands, the same order of the sum
        const int counted = kCountLong ? s_count : 0;
        const int bad0 = s_bad | counted;  // (a counted line has no points to measure)
        LT(3)
        int npts_all = 0;
        if (bad0 == 0 && E <= 64) {
            // (one wave, at most 64 edges: the edge table in registers — lane e holds edge e's
            // offset, count, compact base and the offset of the next edge with points — so the
            // loop over the edges waits on no table load)
            const int eoff = tid < E ? et[2 * tid] : 0, en = tid < E ? et[2 * tid + 1] : 0;
            const uint64_t ne = __ballot(en > 0);
            const uint64_t above = tid >= 63 ? 0ull : (ne & (~0ull << (tid + 1)));
            const int nxl = above ? (int)__builtin_ctzll(above) : 0;
            const int nxo = __shfl(eoff, nxl);
            const int nx = above ? nxo : -1;
            const int incl = wave_incl_scan(en);
            const int cbv = incl - en;
            npts_all = __builtin_amdgcn_readlane(incl, 63);
            for (int e = 0; e < E; ++e) {
                const int off = __builtin_amdgcn_readlane(eoff, e);
                const int n = __builtin_amdgcn_readlane(en, e);
                const int cb = __builtin_amdgcn_readlane(cbv, e);
                const int nxe = __builtin_amdgcn_readlane(nx, e);
                for (int i = tid; i < n; i += kCfLineThreads) {
                    const int noff = i + 1 < n ? off + i + 1 : nxe;
                    if (noff >= 0)
                        pyw[cb + i] = hypot(px[off + i] - px[noff], py[off + i] - py[noff]);
                }
            }
        } else if (bad0 == 0) {
            int cb = 0;
            for (int e = 0; e < E; ++e) {
                const int off = et[2 * e], n = et[2 * e + 1];
                for (int i = tid; i < n; i += kCfLineThreads) {
                    int noff = -1;
                    if (i + 1 < n) {
                        noff = off + i + 1;
                    } else {
                        for (int e2 = e + 1; e2 < E; ++e2)
                            if (et[2 * e2 + 1] > 0) {
                                noff = et[2 * e2];
                                break;
                            }
                    }
                    if (noff >= 0)
                        pyw[cb + i] = hypot(px[off + i] - px[noff], py[off + i] - py[noff]);
                }
                cb += n;
            }
            npts_all = cb;
        }
        __syncthreads();
        LT(4)
        if (tid < 64) {
            // the reversed sum, wave 0: 64 hypots a load (lane j holds pyw[hi - j], the next
            // chunk's load in flight), added in lane order by readlane — the serial order
            double len = 0.0;
            int npts = 0;
            int bad = s_bad;
            if (bad == 0 && counted) {
                long long sum = 0;
                for (int e = 0; e < E; ++e) sum += et[2 * e + 1];
                if (sum > 0x7fffffffll) bad = 8;
                npts = (int)sum;
            } else if (bad == 0) {
                npts = npts_all;
                int hi = npts - 2;
                double v = hi - tid >= 0 ? pyw[hi - tid] : 0.0;
                for (; hi >= 0; hi -= 64) {
                    const double cur = v;
                    v = hi - 64 - tid >= 0 ? pyw[hi - 64 - tid] : 0.0;
                    if (hi >= 63) {  // a full chunk: constant lane indices
#pragma unroll
                        for (int j = 0; j < 64; ++j) len += readlane_f64(cur, j);
                    } else {
                        for (int j = 0; j <= hi; ++j) len += readlane_f64(cur, j);
                    }
                }
            }
            if (tid == 0) {
                ok_out[b] = (vok && bad == 0) ? 1 : 0;
                len_out[b] = bad == 0 ? len : 0.0;
                npts_out[b] = bad == 0 ? npts : 0;
                if (bad) atomicOr(err, bad);
                else if (counted) atomicOr(err, 32);
            }
        }
        __syncthreads();  // the buffers and s_off serve the next item
#ifdef PP_LINE_TIMING
        {
            LT(5)
            if (tid == 0 && it % 97 == 0)
                printf("LT it %d D %d E %d path %llu cnt %llu gen %llu hyp %llu sum %llu\n", it, D, E,
                       lt1 - lt0, lt2 - lt1, lt3 - lt2, lt4 - lt3, lt5 - lt4);
        }
#endif
    }
}

hipError_t launch_check_finish(hipStream_t st, const SceneDev& sc, const SceneDev* scg,
                               const TreeDev& tr,
                               const int* nodes, int k, double gx, double gy, double gyaw,
                               double gyaw_opt, int level0, int mode, int want_line, int* ok,
                               double* len, int* npts, int* chain, double* lit_scratch,
                               int* lit_locks, const CfLines& lines, int* err, int grid,
                               long long* tally, const CfBatch& cb, int* gpath, int* items,
                               const int* blist) {
    if (k <= 0 && lines.grid1 <= 0) return hipSuccess;
    const int wgs = std::min(grid, (k + kCfWaves - 1) / kCfWaves);
    if (k > 0)
        check_finish_kernel<<<wgs, kCfThreads, 0, st>>>(scg, tr, nodes, k, gx, gy, gyaw, gyaw_opt,
                                                        level0, mode, want_line, ok, len, npts,
                                                        chain, lit_scratch, lit_locks, err, tally,
                                                        cb, gpath, items, blist);
    if (want_line && mode != kCfOptimize && lines.grid1 > 0) {
        if (mode == kCfFinalize && !lines.t1.spill)  // (one node: a far goal's line is counted)
            cf_line_kernel<true><<<lines.grid1, kCfLineThreads, 0, st>>>(
                sc, tr, nodes, gx, gy, gyaw, gyaw_opt, ok, len, npts, lines.t1, err, cb, items);
        else
            cf_line_kernel<false><<<lines.grid1, kCfLineThreads, 0, st>>>(
                sc, tr, nodes, gx, gy, gyaw, gyaw_opt, ok, len, npts, lines.t1, err, cb, items);
        if (lines.t1.spill)  // the lines past tier 1's capacities, at the full ones
            cf_line_kernel<false><<<lines.grid2, kCfLineThreads, 0, st>>>(sc, tr, nodes, gx, gy, gyaw,
                                                                   gyaw_opt, ok, len, npts,
                                                                   lines.t2, err, cb,
                                                                   lines.t1.spill);
    }
    return hipGetLastError();
}

// ------------------------------------------- packed line export (pp_batch_paths, pp_star_paths)
//
// Every query's line in one CSR buffer, root side first.  The line generation is one template
// over a pose provider — the chain of poses whose consecutive pairs are the line's Dubins edges
// (CfChainPoses, StarChainPoses: pp_chain_dev.h).
// line_gen runs cf_line_kernel's steps for such a chain on one wave — every edge's word and slot
// count (cf_npoint_steer, a lane per edge), the slot offsets, the literal points edge by edge
// (line_edge_wave) into the workgroup's staging, forward order — and paths_kernel either counts
// the kept points (kWrite false) or copies them, reversed and compact, to the line's packed row:
// forward point f of npts goes to row[npts - 1 - f], a lane per point of an edge, so consecutive
// lanes store consecutive addresses.  Items, tiers and the spill list are cf_line_kernel's.
enum : int { kLgNone = -2, kLgCap = -1, kLgOverflow = -4, kLgNoneGoal = -5 };

// The chain's line by the calling wave (all 64 lanes of a one-wave workgroup): the edges' points
// in forward order in px / py, et[2e] / et[2e + 1] = edge e's offset there and kept count; pyw
// holds the words (4 doubles an edge).  Returns the kept points of all edges, or kLg*: a None
// steer (kLgNoneGoal: the goal edge alone), more slots than pts_cap, an n_point overflow.
template <class P>
__device__ int line_gen(const SceneDev& sc, const P& p, int E, double* px, double* py,
                        double* pyw, int* et, int pts_cap, int lane) {
    int total = 0;
    bool none = false, none0 = false;
    for (int e0 = 0; e0 < E; e0 += 64) {
        const int e = e0 + lane;
        int c = 0;
        if (e < E) {
            Steer w;
            c = cf_npoint_steer(sc, p.pose(e), p.pose(e + 1), w);
            double* wd = pyw + 4 * (size_t)e;
            wd[0] = (double)w.word;
            wd[1] = w.t;
            wd[2] = w.p;
            wd[3] = w.q;
        }
        const uint64_t nm = __ballot(e < E && c == 0);
        if (nm) {
            none0 |= e0 == 0 && (nm & 1);
            none |= (nm & ~(e0 == 0 ? 1ull : 0ull)) != 0;
        }
        // (an overflowing count, -1, or one past the capacity: one slot too many for any tier)
        const int cc = (c < 0 || c > pts_cap) ? pts_cap + 1 : c;
        const int incl = wave_incl_scan(cc);
        if (e < E) et[2 * e] = total + incl - cc;
        total = min(total + __builtin_amdgcn_readlane(incl, 63), pts_cap + 1);
    }
    __syncthreads();
    if (none) return kLgNone;
    if (none0) return kLgNoneGoal;
    if (total > pts_cap) return kLgCap;
    int kept = 0, bad = 0;
    for (int e = 0; e < E; ++e) {
        const int off = et[2 * e];
        const int cap = (e + 1 < E ? et[2 * e + 2] : total) - off;
        const CfPose a = p.pose(e);
        int n = 0;
        const int r = __builtin_amdgcn_readfirstlane(
            line_edge_wave(a.x, a.y, a.yaw, pyw + 4 * (size_t)e, sc.turn_radius, sc.step_size,
                           px + off, py + off, cap, lane, &n));
        // (the kept count is lane 0's: line_edge_wave's trim state lives in the lanes that wrote)
        n = __builtin_amdgcn_readfirstlane(n);
        if (r != kSteerSome) {
            bad |= r == kSteerNone ? 2 : 4;
            n = 0;
        }
        if (lane == 0) et[2 * e + 1] = n;
        kept += n;
    }
    __syncthreads();
    if (bad) return (bad & 2) ? kLgNone : kLgOverflow;
    return kept;
}

template <class P, bool kWrite>
__global__ __launch_bounds__(kCfLineThreads) void paths_kernel(SceneDev sc, PathsArgs a,
                                                               CfLineBufs lb,
                                                               int* __restrict__ err,
                                                               const int* __restrict__ items,
                                                               int items_cap) {
    __shared__ int s_pos[kCfLevels];
    const int tid = threadIdx.x;
    const int pts_cap = lb.pts_cap;
    double* px = lb.pts + (size_t)blockIdx.x * 3 * pts_cap;
    double* py = px + pts_cap;
    double* pyw = py + pts_cap;
    int* et = lb.etab + (size_t)blockIdx.x * 2 * (lb.path_cap + kCfLevels + 1);
    int* path = lb.path + (size_t)blockIdx.x * lb.path_cap;
    // (a spill list counts the lines it had no room for, too)
    const int n_items = min(items[0], items_cap);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int* o = items + 1 + (size_t)it * kCfItem;
        const int b = o[0];
        __syncthreads();  // the buffers and s_pos served the previous item
        if (tid < kCfLevels) s_pos[tid] = o[4 + tid];
        const int q = a.qidx[b];
        TreeDev tr = a.tr;
        const size_t ro = (size_t)q * a.row_cap;
        tr.x += ro;
        tr.y += ro;
        tr.yaw += ro;
        tr.parent += ro;
        const int D = cf_path(tr, a.nodes[b], path, lb.path_cap);
        __syncthreads();
        if (D < 0) {  // deeper than the tier's path capacity
            if (lb.spill) cf_spill(lb, o, tid, err);
            else if (tid == 0) atomicOr(err, 1);
            continue;
        }
        const P p(tr, path, D, o, s_pos, a.goals + 3 * (size_t)q);
        const int E = p.edges();
        const int r = line_gen(sc, p, E, px, py, pyw, et, pts_cap, tid);
        if (r == kLgCap) {
            if (lb.spill) cf_spill(lb, o, tid, err);
            else if (tid == 0) atomicOr(err, 8);
            continue;
        }
        if (r == kLgNoneGoal && P::kGoalNoneOk) {
            if (!kWrite && tid == 0) {
                a.cnt[b] = 0;
                a.okf[b] = 0;
            }
            continue;
        }
        if (r < 0) {
            if (tid == 0) atomicOr(err, r == kLgOverflow ? 4 : 2);
            continue;
        }
        const int npts = r + (P::kRootPoint ? 1 : 0);
        if (!kWrite) {
            if (tid == 0) {
                a.cnt[b] = npts;
                if (a.okf) a.okf[b] = 1;
            }
            continue;
        }
        // the packed row: the count pass and the scan sized it; anything else is a bug, never a
        // store outside the row
        const int64_t base = a.off[q];
        if (a.off[q + 1] - base != (int64_t)npts) {
            if (tid == 0) atomicOr(err, 16);
            continue;
        }
        double* __restrict__ rx = a.ox + base;
        double* __restrict__ ry = a.oy + base;
        int cbase = 0;  // the edge's compact forward base
        for (int e = 0; e < E; ++e) {
            const int off = et[2 * e], n = et[2 * e + 1];
            for (int i = tid; i < n; i += kCfLineThreads) {
                const int w = npts - 1 - (cbase + i);
                rx[w] = px[off + i];
                ry[w] = py[off + i];
            }
            cbase += n;
        }
        if (P::kRootPoint && tid == 0) {
            rx[0] = tr.x[path[0]];
            ry[0] = tr.y[path[0]];
        }
        if (a.len) {
            // euclidean_length of the row in line order: 64 hypots a round, added in lane order
            __threadfence();
            __syncthreads();
            const volatile double* vx = rx;
            const volatile double* vy = ry;
            double len = 0.0;
            for (int k0 = 0; k0 < npts - 1; k0 += 64) {
                const int k = k0 + tid;
                const double h = k < npts - 1 ? hypot(vx[k + 1] - vx[k], vy[k + 1] - vy[k]) : 0.0;
                const int m = min(64, npts - 1 - k0);
                for (int j = 0; j < m; ++j) len += readlane_f64(h, j);
            }
            if (tid == 0) a.len[b] = len;
        }
    }
}

// The packed rows' offsets: off[q] = the exclusive scan of the queries' point counts (slot[q]: the
// query's item or -1; an item counts when okf says so), off[Q] the total; okq[q] the flag.  One
// workgroup, 1024 queries a round.
__global__ __launch_bounds__(1024) void paths_scan_kernel(int Q, const int* __restrict__ slot,
                                                          const int* __restrict__ okf,
                                                          const int* __restrict__ cnt,
                                                          int64_t* __restrict__ off,
                                                          uint8_t* __restrict__ okq) {
    __shared__ int s_w[16];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int q0 = 0; q0 < Q; q0 += 1024) {
        const int q = q0 + tid;
        int c = 0;
        if (q < Q) {
            const int b = slot[q];
            const bool ok = b >= 0 && okf[b] != 0;
            c = ok ? cnt[b] : 0;
            okq[q] = ok ? 1 : 0;
        }
        const int incl = wave_incl_scan(c);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int wbase = 0;
        for (int w = 0; w < wave; ++w) wbase += s_w[w];
        const long long carry = s_carry;
        if (q < Q) off[q] = carry + wbase + incl - c;
        __syncthreads();
        if (tid == 1023) s_carry = carry + wbase + incl;
        __syncthreads();
    }
    if (tid == 0) off[Q] = s_carry;
}

template <class P, bool kWrite>
static hipError_t launch_paths_t(hipStream_t st, const SceneDev& sc, const PathsArgs& a,
                                 const CfLines& lines, int* err, const int* items, int k) {
    if (lines.grid1 <= 0) return hipSuccess;
    paths_kernel<P, kWrite><<<lines.grid1, kCfLineThreads, 0, st>>>(sc, a, lines.t1, err, items,
                                                                    k);
    if (lines.t1.spill)  // the lines past tier 1's capacities, at the full ones
        paths_kernel<P, kWrite><<<lines.grid2, kCfLineThreads, 0, st>>>(
            sc, a, lines.t2, err, lines.t1.spill, lines.t1.spill_cap);
    return hipGetLastError();
}

hipError_t launch_paths(hipStream_t st, const SceneDev& sc, const PathsArgs& a,
                        const CfLines& lines, int* err, const int* items, int k, bool star,
                        bool write) {
    if (!star) return launch_paths_t<CfChainPoses, true>(st, sc, a, lines, err, items, k);
    return write ? launch_paths_t<StarChainPoses, true>(st, sc, a, lines, err, items, k)
                 : launch_paths_t<StarChainPoses, false>(st, sc, a, lines, err, items, k);
}

hipError_t launch_paths_scan(hipStream_t st, int Q, const int* slot, const int* okf,
                             const int* cnt, int64_t* off, uint8_t* okq) {
    paths_scan_kernel<<<1, 1024, 0, st>>>(Q, slot, okf, cnt, off, okq);
    return hipGetLastError();
}

// ------------------------------------------------------------ RRT::plan of a query batch
//
// pp_batch_plan: check_finish (rrt.rs:428-438) of every accepted node of every query — nodes
// 1 .. n_q - 1 in insertion (= iteration) order, rrt.rs:591 — by check_finish_kernel over the
// flattened (query, node) items, then per query the first minimum euclidean_length
// (rrt.rs:607-617).  Items of query q are [off[q], off[q + 1]), node = 1 + (b - off[q]).
__global__ __launch_bounds__(256) void mq_plan_items_kernel(int Q, const int* __restrict__ off,
                                                            int* __restrict__ qidx,
                                                            int* __restrict__ nodes) {
    const int lane = __lane_id();
    const int gw = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    for (int q = gw; q < Q; q += nw) {
        const int a = off[q], e = off[q + 1];
        for (int b = a + lane; b < e; b += 64) {
            qidx[b] = q;
            nodes[b] = 1 + (b - a);
        }
    }
}

__global__ __launch_bounds__(256) void mq_plan_reduce_kernel(
    int Q, const int* __restrict__ off, const int* __restrict__ ok, const double* __restrict__ len,
    const int* __restrict__ npts, int* __restrict__ best_node, double* __restrict__ best_len,
    int* __restrict__ best_npts, int* __restrict__ n_fin) {
    const int lane = __lane_id();
    const int gw = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    for (int q = gw; q < Q; q += nw) {
        const int a = off[q], e = off[q + 1];
        double bd = __builtin_inf();
        int bi = 0x7fffffff, cnt = 0;
        for (int b = a + lane; b < e; b += 64) {
            if (!ok[b]) continue;
            ++cnt;
            argmin_pair(bd, bi, len[b], b);  // first minimum: the lowest item on ties
        }
        wave_argmin(bd, bi);
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) {
            const bool any = bi != 0x7fffffff;
            best_node[q] = any ? 1 + (bi - a) : -1;
            best_len[q] = any ? bd : __builtin_inf();
            best_npts[q] = any ? npts[bi] : 0;
            n_fin[q] = cnt;
        }
    }
}

hipError_t launch_mq_plan_items(hipStream_t s, int Q, const int* off, int* qidx, int* nodes) {
    mq_plan_items_kernel<<<std::min((Q + 3) / 4, 4096), 256, 0, s>>>(Q, off, qidx, nodes);
    return hipGetLastError();
}

hipError_t launch_mq_plan_reduce(hipStream_t s, int Q, const int* off, const int* ok,
                                 const double* len, const int* npts, int* best_node,
                                 double* best_len, int* best_npts, int* n_fin) {
    mq_plan_reduce_kernel<<<std::min((Q + 3) / 4, 4096), 256, 0, s>>>(
        Q, off, ok, len, npts, best_node, best_len, best_npts, n_fin);
    return hipGetLastError();
}

// --------------------------------- check_finish of a query batch in steer rounds (round 4)
//
// check_finish_kernel runs every item's edges one after the other on one wave, at 2 waves per
// SIMD (its register budget): a latency chain.  For a batch plan, every edge whose verdict
// depends on one tree node or one item is steered up front instead, by the query batch's own
// steer_prep / steer_walk at their occupancy, and written to the memo tables the kernel already
// reads (CfBatch::ftab / gtab, and gotab: the goal edge of each item):
//   phase A  ftab of every node (optimize's level for node c: the first of c's ancestors, root
//            first, and c itself whose edge verifies, rrt.rs:463-487): rounds of kCfbSpan
//            candidates per open node, in order; a node settles at its first verdict that is
//            not a rejection (a literal-path or error verdict leaves ftab unknown);
//   phase B  each item's chain follows ftab; its goal edge (Node::new_goal, rrt.rs:430-436,
//            the goal keeping its own yaw) and its copy edges (one per chain node v, claimed by
//            the first item that reaches v) are steered in one round: gotab / gtab;
//   assemble one lane per item: the chain, the verdicts in finalize's order, the panic scan from
//            the None flags (a None steer is a panic status in the memo; the tree edges' flags
//            are tnone_up), the outputs or a line item.  An item with any unknown verdict goes
//            to a list that check_finish_kernel runs as before (with every memo entry there).
// Results are those of check_finish_kernel: the same edges, the same verdicts, the same order
// of precedence (a panic anywhere wins over a rejection; verify decides the rest).

// phase A node list: b < nitems is item b (qidx[b], nodes[b]); b - nitems < Q is query's root
// query q's first memo row: the memo tables are compact, q's n_q nodes after the nodes of the
// queries before it (their items plus their roots)
__device__ inline size_t cfb_memo_row(const CfbArgs& a, int q) {
    return (size_t)a.moff[q] + q;
}

__device__ inline void cfb_node(const CfbArgs& a, int b, int& q, int& c) {
    if (b < a.nitems) {
        q = a.qidx[b];
        c = a.nodes[b];
    } else {
        q = b - a.nitems;
        c = 0;
    }
}

// depth of every phase-A node, its own tree edge's None flag (the steer from its pose to its
// parent's, rrt.rs:313 / 529), and the open state; maxdepth for the host
__global__ __launch_bounds__(256) void cfb_depth_kernel(CfbArgs a, SceneDev sc) {
    // (the depth histogram per workgroup in LDS, then one atomic per nonzero bin: the host bounds
    // each steer round's task count by it)
    __shared__ int s_h[kCfbDepthBins];
    if (threadIdx.x < kCfbDepthBins) s_h[threadIdx.x] = 0;
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = b < a.nitems + a.Q;
    if (in) {
        int q0, c0;
        cfb_node(a, b, q0, c0);
        const size_t o0 = (size_t)q0 * a.row_cap;
        int d0 = 0;
        for (int k = c0; a.tr.parent[o0 + k] >= 0; k = a.tr.parent[o0 + k]) ++d0;
        atomicAdd(&s_h[min(d0, kCfbDepthBins - 1)], 1);
        a.depth[b] = d0;
    }
    __syncthreads();
    if (a.dhist && threadIdx.x < kCfbDepthBins && s_h[threadIdx.x])
        atomicAdd(&a.dhist[threadIdx.x], s_h[threadIdx.x]);
    if (!in) return;
    int q, c;
    cfb_node(a, b, q, c);
    const size_t o = (size_t)q * a.row_cap;
    const int d = a.depth[b];
    a.open[b] = 1;
    atomicMax(a.maxdepth, d);
    int none = 0;
    if (c > 0) {
        const int p = a.tr.parent[o + c];
        const CfPose from{a.tr.x[o + c], a.tr.y[o + c], a.tr.yaw[o + c]};
        const CfPose to{a.tr.x[o + p], a.tr.y[o + p], a.tr.yaw[o + p]};
        none = cf_npoint(sc, from, to) == 0 ? 1 : 0;
    }
    a.tnone[cfb_memo_row(a, q) + c] = (unsigned char)none;
}

// tnone_up[c]: any tree edge from c down to the root has a None steer
__global__ __launch_bounds__(256) void cfb_tnone_up_kernel(CfbArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nitems + a.Q) return;
    int q, c;
    cfb_node(a, b, q, c);
    const size_t o = (size_t)q * a.row_cap;
    int any = 0;
    const size_t m = cfb_memo_row(a, q);
    for (int k = c; k > 0; k = a.tr.parent[o + k]) any |= a.tnone[m + k];
    a.tnone_up[m + c] = (unsigned char)any;
}

// a thread's task count -> its first task index: one atomic per 256-thread workgroup on the
// round's counter (per wave, ~9k waves contending for one address cost ~0.2 ms a round).  Every
// thread of the workgroup must call it.
__device__ inline int cfb_reserve(int* counter, int cnt, int* wsum) {
    __shared__ int s_wt[4], s_base;
    const int lane = __lane_id(), w = threadIdx.x >> 6;
    const int incl = wave_incl_scan(cnt);
    if (lane == 63) s_wt[w] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = s_wt[0] + s_wt[1] + s_wt[2] + s_wt[3];
        s_base = tot ? atomicAdd(counter, tot) : 0;
        if (wsum && tot) atomicAdd(wsum, tot);
    }
    __syncthreads();
    int wb = s_base;
    for (int k = 0; k < w; ++k) wb += s_wt[k];
    return wb + incl - cnt;
}

// phase A round r: the next `span` candidates (depth m0 .. m0 + span - 1, root first) of every open
// node, as explicit (child, parent pose) tasks: child = the node's position (compute_yaw toward
// the candidate, as Node::new does), parent = the candidate's stored pose
__global__ __launch_bounds__(256) void cfb_emit_a_kernel(CfbArgs a, int m0, int span) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int cnt = 0, q = 0, c = 0, d = 0;
    if (b < a.nitems + a.Q && a.open[b]) {
        cfb_node(a, b, q, c);
        d = a.depth[b];
        cnt = min(span, d + 1 - m0);
        if (cnt < 0) cnt = 0;
    }
    const int t0 = cfb_reserve(&a.st->W, cnt, a.wsum);
    if (b < a.nitems + a.Q) {
        a.tfirst[b] = t0;
        a.tcnt[b] = cnt;
    }
    if (cnt == 0) return;
    const size_t o = (size_t)q * a.row_cap;
    const double x = a.tr.x[o + c], y = a.tr.y[o + c];
    // climb to depth m0 + cnt - 1, then emit the candidates downward to depth m0
    int k = c;
    for (int dd = d; dd > m0 + cnt - 1; --dd) k = a.tr.parent[o + k];
    for (int i = cnt - 1; i >= 0; --i) {
        const int t = t0 + i;
        SteerTask tk;
        tk.x = x;
        tk.y = y;
        tk.px = a.tr.x[o + k];
        tk.py = a.tr.y[o + k];
        tk.pyaw = a.tr.yaw[o + k];
        tk.pnode = k;
        tk.literal = 0;
        a.tasks[t] = tk;
        a.tnode[t] = b;
        if (i > 0) k = a.tr.parent[o + k];
    }
}

// phase A round r, after the walk: a node settles at its first candidate (in order) that is not
// rejected — accepted: ftab = 2 + depth (| 1 << 30 for a None steer, finalize's panic); literal
// path or error: left unknown for check_finish_kernel — or when its last candidate was rejected:
// ftab = 1 (no candidate)
__global__ __launch_bounds__(256) void cfb_consume_a_kernel(CfbArgs a, int m0) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) a.st->W = 0;  // the next round's counter (every reader of W has finished)
    if (b >= a.nitems + a.Q) return;
    const int cnt = a.tcnt[b];
    if (cnt == 0) return;
    int q, c;
    cfb_node(a, b, q, c);
    const int t0 = a.tfirst[b];
    for (int i = 0; i < cnt; ++i) {
        const int s = a.status[t0 + i];
        if (s == kReject) continue;
        if (s == kAccept) {
            const int fnone = a.none[t0 + i];
            a.ftab[cfb_memo_row(a, q) + c] = (2 + m0 + i) | (fnone << 30);
        }
        a.open[b] = 0;
        return;
    }
    if (m0 + cnt > a.depth[b]) {
        a.ftab[cfb_memo_row(a, q) + c] = 1;
        a.open[b] = 0;
    }
}

// an item's optimize chain from ftab (check_finish_kernel's level loop): n[0] = the item's node,
// n[l + 1] = its level-l candidate (pos[l] = that node's depth); false when an entry on the way
// is unknown
__device__ inline bool cfb_chain(const CfbArgs& a, size_t o, size_t mr, int c, int d, int* n,
                                 int* pos, int& s, int& fnone) {
    s = 0;
    fnone = 0;
    n[0] = c;
    int cur = c, curd = d;
    for (int level = 0; level < kCfLevels; ++level) {
        const int fm = a.ftab[mr + cur];
        if (fm == 0) return false;
        if (fm == 1) break;
        const int found = (fm & 0x3fffffff) - 2;
        fnone = fm >> 30;
        pos[level] = found;
        s = level + 1;
        if (curd == 0) {  // a level at the root: root copies to the recursion limit
            for (int l2 = level + 1; l2 < kCfLevels; ++l2) pos[l2] = 0;
            for (int l2 = level + 1; l2 <= kCfLevels; ++l2) n[l2] = cur;
            s = kCfLevels;
            break;
        }
        while (curd > found) {
            cur = a.tr.parent[o + cur];
            --curd;
        }
        n[level + 1] = cur;
    }
    return true;
}

// phase B: every item's goal edge, and the copy edges of its chain that no other item claimed
__global__ __launch_bounds__(256) void cfb_emit_b_kernel(CfbArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    int n[kCfLevels + 1], pos[kCfLevels];
    int s = 0, fnone = 0, cnt = 0, q = 0, c = 0;
    size_t o = 0, mr = 0;
    bool ok = false;
    unsigned claimed = 0;  // bit e: this item steers copy edge e (1 <= e < s)
    if (b < a.nitems) {
        cfb_node(a, b, q, c);
        o = (size_t)q * a.row_cap;
        mr = cfb_memo_row(a, q);
        ok = cfb_chain(a, o, mr, c, a.depth[b], n, pos, s, fnone);
        if (ok) {
            cnt = 1;
            // (a plain L2 read first: the edges near a query's root are claimed once and read by
            // most of its items — an exchange each serialised on those few addresses)
            for (int e = 1; e < s; ++e)
                if (__hip_atomic_load(&a.gclaim[mr + n[e - 1]], __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT) == 0 &&
                    atomicExch(&a.gclaim[mr + n[e - 1]], 1) == 0) {
                    claimed |= 1u << e;
                    ++cnt;
                }
        }
    }
    const int t0 = cfb_reserve(&a.st->W, cnt, a.wsum);
    if (!ok) return;
    const double* X = a.tr.x + o;
    const double* Y = a.tr.y + o;
    // the goal edge: Node::new_goal (the goal keeps its yaw: the planner's optimised yaw when
    // optimize succeeded, rrt.rs:489-501) into pose 1 — the copy at the node toward n[1], or
    // the node's stored pose when the chain is empty
    const double gyaw = a.goals[3 * q + 2];
    SteerTask tk;
    tk.x = a.goals[3 * q];
    tk.y = a.goals[3 * q + 1];
    if (s > 0) {
        tk.px = X[c];
        tk.py = Y[c];
        tk.pyaw = cf_atan2(Y[n[1]] - Y[c], X[n[1]] - X[c]);
    } else {
        tk.px = X[c];
        tk.py = Y[c];
        tk.pyaw = a.tr.yaw[o + c];
    }
    tk.pnode = 0;
    tk.literal = 0;
    a.tasks[t0] = tk;
    StarTaskExt ex{};
    ex.own_yaw = 1;
    ex.cyaw = gyaw;
    a.ext[t0] = ex;
    a.tnode[t0] = b;
    int t = t0 + 1;
    for (int e = 1; e < s; ++e) {
        if (!((claimed >> e) & 1u)) continue;
        // copy edge e: from the copy at v = n[e - 1] toward n[e] (compute_yaw) to the copy at
        // n[e] toward n[e + 1]
        const int v = n[e - 1], w = n[e], w2 = n[e + 1];
        SteerTask ct;
        ct.x = X[v];
        ct.y = Y[v];
        ct.px = X[w];
        ct.py = Y[w];
        ct.pyaw = cf_atan2(Y[w2] - Y[w], X[w2] - X[w]);
        ct.pnode = w;
        ct.literal = 0;
        a.tasks[t] = ct;
        a.ext[t] = StarTaskExt{};
        a.tnode[t] = -1 - (int)(mr + v);
        ++t;
    }
}

// phase B, after the walk: the verdicts into gotab / gtab (a None steer: finalize's panic; a
// literal-path or error verdict stays unknown)
__global__ __launch_bounds__(256) void cfb_store_b_kernel(CfbArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.st->W) return;
    int s = a.status[t];
    if (a.none[t]) s = kCfPanic;
    else if (s != kAccept && s != kReject) return;
    const int n = a.tnode[t];
    if (n >= 0)
        a.gotab[n] = s + 1;
    else
        a.gtab[-1 - n] = s + 1;
}

// after a rounds walk: the literal-path tasks (the trim cases steer_walk hands back, e.g. the
// zero-length copy edges at a root, whose points are all 0.0) re-run by steer_collide_literal,
// as mq_insert does for the extend tasks, so their verdicts reach the memo instead of punting
// every item whose chain holds them to check_finish_kernel.  The list first, then one wave per
// listed task (wave w owns scratch slot w: no locks), so the serial generations run side by side
__global__ __launch_bounds__(256) void cfb_lit_list_kernel(CfbArgs a, int* __restrict__ list,
                                                           int* __restrict__ count) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.st->W && a.status[t] == kLiteral) list[atomicAdd(count, 1)] = t;
}

// steer_collide_literal with the literal course generated by the whole wave: the word of
// dubins_path_planning(child → parent) as cf_npoint_steer chooses it, then line_edge_wave (the
// line kernel's lane-parallel restatement of dubins_literal: the same points, the same trim), then
// the same chunk test.  A long trim-case course (thousands of points) no longer runs on one lane.
__device__ int steer_collide_literal_wave(const SceneDev& sc, double x, double y, double yaw,
                                          double px, double py, double pyaw, double* bx,
                                          double* by) {
    const int lane = __lane_id();
    Steer st;
    (void)cf_npoint_steer(sc, CfPose{x, y, yaw}, CfPose{px, py, pyaw}, st);
    const double w[4] = {(double)st.word, st.t, st.p, st.q};
    int n = 0;
    const int r = line_edge_wave(x, y, yaw, w, sc.turn_radius, sc.step_size, bx, by,
                                 kLiteralCap - 1, lane, &n);
    if (r == kSteerOverflow) return kError;
    if (lane == 0) {
        if (r == kSteerNone) {  // polyline [(x, y), (px, py)] (rrt.rs:313)
            bx[0] = x;
            by[0] = y;
            n = 1;
        }
        bx[n] = px;
        by[n] = py;
    }
    if (r == kSteerNone) n = 1;
    __threadfence_block();  // the wave's points before it reads them back
    const int np = n + 1;   // the junction point is bounds-checked too
    return stored_line_rejects(sc, bx, by, np, x, y) ? kReject : kAccept;
}

__global__ __launch_bounds__(256) void cfb_lit_run_kernel(CfbArgs a, SceneDev sc,
                                                          const int* __restrict__ list,
                                                          const int* __restrict__ count,
                                                          double* __restrict__ lit_scratch) {
    const int lane = __lane_id();
    const int gw = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int nw = (int)((gridDim.x * blockDim.x) >> 6);
    double* bx = lit_scratch + (size_t)gw * 3 * kLiteralCap;
    const int n = *count;
    for (int i = gw; i < n; i += nw) {
        const int t = list[i];
        const SteerTask tk = a.tasks[t];
        const int r = steer_collide_literal_wave(sc, tk.x, tk.y, a.yaw[t], tk.px, tk.py, tk.pyaw,
                                                 bx, bx + kLiteralCap);
        if (lane == 0) a.status[t] = r;
    }
}

hipError_t launch_cfb_literal(hipStream_t s, const SceneDev& sc, const CfbArgs& a, int max_tasks,
                              int* list, int* count, double* lit_scratch) {
    if (max_tasks <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(count, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    cfb_lit_list_kernel<<<(max_tasks + 255) / 256, 256, 0, s>>>(a, list, count);
    cfb_lit_run_kernel<<<kLiteralWaves / 4, 256, 0, s>>>(a, sc, list, count, lit_scratch);
    return hipGetLastError();
}

// one lane per item: finalize's verdict from the memo (check_finish_kernel's order and
// precedence), its outputs or its line item; an item with an unknown verdict goes to plist
__global__ __launch_bounds__(256) void cfb_assemble_kernel(CfbArgs a, int* __restrict__ ok_out,
                                                           double* __restrict__ len_out,
                                                           int* __restrict__ npts_out,
                                                           int* __restrict__ err,
                                                           int* __restrict__ items,
                                                           int* __restrict__ plist) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nitems) return;
    int q, c;
    cfb_node(a, b, q, c);
    const size_t o = (size_t)q * a.row_cap, mr = cfb_memo_row(a, q);
    int n[kCfLevels + 1], pos[kCfLevels];
    int s = 0, fnone = 0;
    bool known = cfb_chain(a, o, mr, c, a.depth[b], n, pos, s, fnone);
    // verdicts in finalize's order: 0 accept, 1 reject, 2 panic (the first non-accepted decides,
    // a None steer anywhere wins over a rejection)
    int first = 0;
    bool any_none = false;
    if (known) {
        const int g = a.gotab[b];
        known = g == 1 + kAccept || g == 1 + kReject || g == 1 + kCfPanic;
        if (known && g != 1 + kAccept) first = g == 1 + kReject ? 1 : 2;
        any_none = g == 1 + kCfPanic;
    }
    for (int e = 1; known && e < s; ++e) {
        const int g = a.gtab[mr + n[e - 1]];
        known = g == 1 + kAccept || g == 1 + kReject || g == 1 + kCfPanic;
        if (known && g != 1 + kAccept && first == 0) first = g == 1 + kReject ? 1 : 2;
        any_none |= g == 1 + kCfPanic;
    }
    if (!known) {
        plist[atomicAdd(&a.pcount[0], 1)] = b;
        return;
    }
    if (s >= 1 && fnone) {  // edge s: the last level's accepted candidate edge
        any_none = true;
        if (first == 0) first = 2;
    }
    const bool tree_none = a.tnone_up[mr + n[s]] != 0;  // edges s + 1 .. E - 1
    int bad = 0;
    bool vok = false;
    if (first == 2) {
        bad = 2;
    } else if (first == 1) {
        if (any_none || tree_none) bad = 2;
    } else {
        vok = true;
        if (tree_none) bad = 2;
    }
    if (vok && bad == 0) {
        const int it = atomicAdd(&items[0], 1);
        int* ob = items + 1 + (size_t)it * kCfItem;
        ob[0] = b;
        ob[1] = s;
        ob[2] = 1;
        ob[3] = 0;
        for (int i = 0; i < kCfLevels; ++i) ob[4 + i] = i < s ? pos[i] : 0;
    } else {
        ok_out[b] = 0;
        len_out[b] = 0.0;
        npts_out[b] = 0;
        if (bad) atomicOr(err, bad);
    }
}

hipError_t launch_cfb(hipStream_t s, const SceneDev& sc, CfbArgs a, int phase, int round,
                      int* ok, double* len, int* npts, int* err, int* items, int* plist) {
    const int nn = a.nitems + a.Q;
    const int g = (nn + 255) / 256;
    switch (phase) {
        case kCfbDepth:
            cfb_depth_kernel<<<g, 256, 0, s>>>(a, sc);
            cfb_tnone_up_kernel<<<g, 256, 0, s>>>(a);
            break;
        case kCfbEmitA:
            cfb_emit_a_kernel<<<g, 256, 0, s>>>(a, round, a.span);  // round: the first depth m0
            break;
        case kCfbConsumeA:
            cfb_consume_a_kernel<<<g, 256, 0, s>>>(a, round);
            break;
        case kCfbEmitB:
            cfb_emit_b_kernel<<<(a.nitems + 255) / 256, 256, 0, s>>>(a);
            break;
        case kCfbStoreB:
            cfb_store_b_kernel<<<(round + 255) / 256, 256, 0, s>>>(a);  // round: the task bound
            break;
        case kCfbAssemble:
            cfb_assemble_kernel<<<(a.nitems + 255) / 256, 256, 0, s>>>(a, ok, len, npts, err,
                                                                        items, plist);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the steer rounds' records in chunks of `cap` tasks: chunk [base, base + cap) of the round's
// a.st->W tasks gets its own task count (cfb_chunk_begin), and after its walk the None flags of
// its records (consume A / store B read them once every chunk's record is overwritten)
__global__ void cfb_chunk_begin_kernel(const DevState* __restrict__ all, DevState* __restrict__ chunk,
                                       int base, int cap) {
    const int w = all->W - base;
    chunk->W = w < 0 ? 0 : (w < cap ? w : cap);
    chunk->ncomp = 0;
    chunk->alist = nullptr;
}

__global__ __launch_bounds__(256) void cfb_chunk_none_kernel(const DevState* __restrict__ chunk,
                                                             const PrepRec* __restrict__ rec,
                                                             unsigned char* __restrict__ none) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < chunk->W) none[t] = rec[t].state == kPrepNone ? 1 : 0;
}

hipError_t launch_cfb_chunk(hipStream_t s, const DevState* all, DevState* chunk, int base,
                            int cap, bool begin, const PrepRec* rec, unsigned char* none) {
    if (begin)
        cfb_chunk_begin_kernel<<<1, 1, 0, s>>>(all, chunk, base, cap);
    else
        cfb_chunk_none_kernel<<<(cap + 255) / 256, 256, 0, s>>>(chunk, rec, none);
    return hipGetLastError();
}

// a steer round over the tasks the emit kernel counted in st->W (the query batch's kernels)
hipError_t launch_cfb_steer(hipStream_t s, const SceneDev& sc, const CfbArgs& a, int max_tasks,
                            bool own_yaw, long long* wg_points) {
    if (max_tasks <= 0) return hipSuccess;
    const int pb = std::min((max_tasks + 31) / 32, 8192);
    launch_prep_tasks(s, pb, a.st, sc, a.rec, a.yaw, a.tasks, nullptr, own_yaw ? a.ext : nullptr);
    // (max_tasks > 0: at least one workgroup)
    const int wb = walk_blocks(max_tasks, walk_grid_limit(kWalkBatchPlan, sc));
    launch_walk(kWalkBatchPlan, s, wb, a.st, sc, a.rec, nullptr, a.status, nullptr, nullptr,
                wg_points);
    return hipGetLastError();
}

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

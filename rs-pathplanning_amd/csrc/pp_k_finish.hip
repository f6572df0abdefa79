// pp_k_finish.hip — hand-written CDNA4 (gfx950) kernels of check_finish and what shares its cf_*
// helpers: check_finish_kernel, the line kernel (cf_line_kernel), the packed line export
// (paths_*), the batch plan's item lists (mq_plan_*) and its rounds (cfb_*).
// steer_prep and steer_walk are compiled by pp_k_steer.hip alone and launched through
// pp_steer_launch.h; the device code the units inline is pp_steer_dev.h.
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
// The same holds for the literal path: cf_edge_check, inlined into check_finish_kernel, is this
// unit's only caller of steer_collide_literal (folded in, the kernel grows from 13,410 to 20,712
// lines of assembly).
namespace ppamd {
template <bool kLds>
__device__ __noinline__ int s_classify_poly(const SceneDev& sc, double ax, double ay, double bx,
                                            double by, double t_lo, double t_hi, double dl);
__device__ __noinline__ int steer_collide_literal(const SceneDev& sc, double x, double y,
                                                  double yaw, double px, double py, double pyaw,
                                                  double* bx, double* by, double* byaw,
                                                  bool junction);
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

}  // namespace ppamd

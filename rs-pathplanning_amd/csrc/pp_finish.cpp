// pp_finish.cpp — RRT::check_finish / optimize / finalize of the one-tree planner, pp_rrt_plan, and
// the query batch's plan (pp_batch_plan) over the same kernels; the packed line export of a batch
// (pp_batch_paths) and the steps it shares with pp_star_paths.
#include "pp_ctx.h"

using namespace ppamd;

namespace {

static_assert(PP_CF_CHAIN == kCfLevels + 2, "chain row layout");
constexpr int kCfBatch = 16384;     // nodes per check_finish launch
constexpr int kCfPtsCap = 1 << 16;  // line points per check_finish workgroup
static_assert(4 * kCfMaxEdges <= kCfPtsCap, "cf_line_kernel keeps 4 doubles per edge in the hypot buffer");
// cf_line_kernel in two tiers (CfLines): tier 1 runs every line on kCfLineGrid workgroups with
// room for kCfLinePts1 points and a kCfLinePath1-deep path each (3 x 6144 doubles: 144 KB; the
// config-3 plan's lines have ~2400 points), tier 2 the few longer or deeper ones at the full
// capacities (kCfPtsCap points, kCfMaxDepth) on kCfLineGrid2 workgroups (1.5 MB each).  Round 5
// gave every one of 2048 workgroups the full capacity: 3.2 GB.  1024 tier-1
// workgroups cost the config-3 plan ~0.5 ms of its 12.5 (one wave per line: the lines in flight
// are the workgroups), so the grid stays at 2048 (300 MB).
constexpr int kCfLineGrid = 2048;
constexpr int kCfLinePts1 = 6144;
constexpr int kCfLinePath1 = 1024;
constexpr int kCfLineGrid2 = 64;
constexpr int kCfSpillCap = 1 << 17;  // tier-1 lines handed to tier 2 per launch
static_assert(4 * (kCfLinePath1 + kCfLevels + 1) <= kCfLinePts1, "tier 1: 4 doubles per edge");
// phase A's task arrays (status, lists, SteerTask, StarTaskExt, yaw, None flag per task) are
// sized for span x (items + queries) tasks: a span that would need more than this is clamped (the
// spans change which candidates are walked together, never a result); the records (PrepRec,
// 256 B a task) are steered in chunks of kCfbRecChunk tasks
constexpr size_t kCfbTaskBudget = (size_t)512 << 20;
constexpr size_t kCfbRecChunk = (size_t)1 << 20;

// check_finish for nodes[0, k) (device pointer already filled); results on the device
// The goal of a check_finish_kernel launch: the planner's (check_finish), or a caller-built goal
// node (finalize), and the kernel mode / optimize's starting level.
struct CfGoal {
    double x, y, yaw, yaw_opt;
    int level0 = 0, mode = kCfCheck;
};

// Where a check_finish_kernel launch writes its per-node results (device pointers).
struct CfOut {
    int* ok;
    double* len;
    int* npts;
    int* chain;  // may be null
};

// cf_line_kernel's buffers for a launch of `wgs` tier-1 workgroups (CfLines).  spill == 0: one
// tier at the full capacities (a one-node call, whose line the host reads from workgroup 0's
// buffer); else tier 1 hands up to `spill` lines to tier 2.  The spill count is zeroed on the
// stream.
int cf_line_buffers(pp_ctx* c, int wgs, int spill, CfLines& L) {
    const bool two = spill > 0;
    const int pc1 = two ? kCfLinePts1 : kCfPtsCap, dc1 = two ? kCfLinePath1 : kCfMaxDepth;
    const int g2 = two ? std::min(kCfLineGrid2, wgs) : 0;
    const size_t e1 = 2 * (size_t)(dc1 + kCfLevels + 1), e2 = 2 * (size_t)kCfMaxEdges;
    PP_HIP(c->cf.pts.reserve((size_t)wgs * 3 * pc1 + (size_t)g2 * 3 * kCfPtsCap));
    PP_HIP(c->cf.etab.reserve((size_t)wgs * e1 + (size_t)g2 * e2));
    PP_HIP(c->cf.lpath.reserve((size_t)wgs * dc1 + (size_t)g2 * kCfMaxDepth));
    L.grid1 = wgs;
    L.t1 = CfLineBufs{c->cf.pts.p, pc1, c->cf.etab.p, c->cf.lpath.p, dc1, nullptr};
    if (two) {
        PP_HIP(c->cf.spill.reserve(1 + (size_t)spill * kCfItem));
        PP_HIP(hipMemsetAsync(c->cf.spill.p, 0, sizeof(int), c->stream));
        L.t1.spill = c->cf.spill.p;
        L.t1.spill_cap = spill;
        L.grid2 = g2;
        L.t2 = CfLineBufs{c->cf.pts.p + (size_t)wgs * 3 * pc1, kCfPtsCap,
                          c->cf.etab.p + (size_t)wgs * e1, c->cf.lpath.p + (size_t)wgs * dc1,
                          kCfMaxDepth, nullptr};
    }
    return PP_OK;
}

// check_finish_kernel reads the scene from device memory (a reference to the kernel-argument
// struct would copy it to every lane's stack); uploaded when it changed.  The stream is
// synchronised at the end of every cf_run / cf_run_rounds, so the host copy is never overwritten
// in flight.
int cf_upload_scene(pp_ctx* c, const SceneDev& sd) {
    Finish& f = c->cf;
    if (f.scene_ok && std::memcmp(&f.scene_host, &sd, sizeof sd) == 0) return PP_OK;
    if (!f.scene.p) PP_HIP(f.scene.reserve(1));
    f.scene_host = sd;
    PP_HIP(hipMemcpyAsync(f.scene.p, &f.scene_host, sizeof sd, hipMemcpyHostToDevice, c->stream));
    f.scene_ok = true;
    return PP_OK;
}

// the kernels' error bits (cf.err[0]) as the API's error
int cf_error(int err) {
    if (err & 2) return set_err(PP_ERR_REFERENCE_PANIC, "finalize: a Dubins edge has no feasible word (rrt.rs:529 panics)");
    if (err & 4) return set_err(PP_ERR_STEER_OVERFLOW, "generate_local_course would index past n_point");
    if (err & 1) return set_err(PP_ERR_CAPACITY, "tree deeper than the check_finish path capacity");
    if (err & 8) return set_err(PP_ERR_CAPACITY, "finalized line longer than the point capacity");
    return PP_OK;
}

// check_finish_kernel over nodes[0, k) (device) with its error handling; the one-tree planner
// (cb.qidx null: the context's tree, goal g) or a query batch (cb)
int cf_run(pp_ctx* c, const TreeDev& tr, const int* nodes, int k, int want_line, int grid,
           const CfGoal& gg, const CfOut& o, const CfBatch& cb_in) {
    const CfGoal* g = &gg;
    PP_HIP(c->cf.err.reserve(2));  // [0] error bits, [1] the kernel's node counter
    // optimize's memo: two ints per tree row (the batch's Q * row_cap rows, or the tree's nodes),
    // zeroed for this launch
    CfBatch cb = cb_in;
    // (a batch's memo rows are compact: its items plus a root per query)
    const size_t rows = cb.qidx ? (cb.moff ? (size_t)k + c->batch.f.Q : (size_t)c->batch.f.Q * (size_t)cb.row_cap)
                                : (size_t)c->rrt.n;
    PP_HIP(c->cf.memo.reserve(2 * std::max<size_t>(rows, 1)));
    PP_HIP(hipMemsetAsync(c->cf.memo.p, 0, 2 * rows * sizeof(int), c->stream));
    cb.ftab = c->cf.memo.p;
    cb.gtab = c->cf.memo.p + rows;
    // the line buffers (per workgroup of the line kernel) only when lines are materialised: one
    // workgroup at the full capacities for a one-node call (the host reads workgroup 0's line),
    // else the two tiers
    const int wgs = std::min(grid, k);
    CfLines lines;
    if (want_line) {
        PP_HIP(c->cf.items.reserve(1 + (size_t)k * kCfItem));
        PP_HIP(hipMemsetAsync(c->cf.items.p, 0, sizeof(int), c->stream));
        int r = cf_line_buffers(c, wgs, wgs > 1 ? std::min(k, kCfSpillCap) : 0, lines);
        if (r) return r;
    }
    // the ancestor paths of check_finish_kernel's waves (kCfWaves per workgroup, at most
    // min(grid, k / kCfWaves) workgroups)
    PP_HIP(c->cf.path.reserve((size_t)std::min(grid, (k + kCfWaves - 1) / kCfWaves) * kCfWaves * kCfMaxDepth));
    if (int r = ensure_literal_pool(c, c->stream)) return r;
    PP_HIP(hipMemsetAsync(c->cf.err.p, 0, 2 * sizeof(int), c->stream));
    if (c->prof.on) {
        if (int r = ensure_events(c, 2)) return r;
        PP_HIP(hipEventRecord(c->prof.ev[0], c->stream));
    }
    SceneDev sd = c->scene_dev();
    if (cb.qidx) sd.step_size = c->batch.f.step;  // a query batch's edges use the batch's step
    if (int r = cf_upload_scene(c, sd)) return r;
    PP_HIP(launch_check_finish(c->stream, sd, c->cf.scene.p, tr, nodes, k, g->x, g->y,
                               g->yaw, g->yaw_opt, g->level0, g->mode, want_line, o.ok, o.len,
                               o.npts, o.chain, c->api_lit_scratch.p, c->lit_locks.p, lines,
                               c->cf.err.p, grid, c->prof.on ? c->prof.cf_tally.p : nullptr, cb,
                               c->cf.path.p, want_line ? c->cf.items.p : nullptr));
    if (c->prof.on) PP_HIP(hipEventRecord(c->prof.ev[1], c->stream));
    int err = 0;
    PP_HIP(hipMemcpyAsync(&err, c->cf.err.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PP_HIP(hipStreamSynchronize(c->stream));
    if (c->prof.on) {
        float ms = 0.f;
        PP_HIP(hipEventElapsedTime(&ms, c->prof.ev[0], c->prof.ev[1]));
        c->prof.finish_ms += ms;
        c->prof.finish_launches += 1;
    }
    c->cf.counted_only = (err & 32) != 0;
    return cf_error(err & ~32);
}

// pp_batch_plan's check_finish in steer rounds (CfbArgs, pp_k_finish.hip): phase A rounds fill
// ftab for every node, phase B the goal and copy edges, the assemble kernel decides every item
// whose verdicts are known, and check_finish_kernel runs the rest (literal paths, errors) with
// the memo filled.  The same results as cf_run over all items; polygon scenes and batches with
// a blocked root take cf_run.

int cf_run_rounds(pp_ctx* c, const TreeDev& tr, int total, const CfBatch& cb_in, const CfOut& o) {
    const int Q = c->batch.f.Q;
    const size_t nn = (size_t)total + Q;
    const size_t rows = nn;  // the compact memo rows (cb_in.moff): every item and root
    // phase A: <= span tasks per node; B: <= 2 per node.  The spans are clamped to the task budget
    // (at least 2: phase B's tasks)
    const size_t task_bytes = 3 * sizeof(int) + sizeof(SteerTask) + sizeof(StarTaskExt) +
                              sizeof(double) + 1;
    const int span_cap = (int)std::max<size_t>(2, kCfbTaskBudget / (task_bytes * std::max<size_t>(nn, 1)));
    const int span0 = std::min(c->batch.cfb_span0, span_cap), span1 = std::min(c->batch.cfb_span, span_cap);
    const size_t cap_tasks = std::max<size_t>((size_t)std::max({span0, span1, 2}) * nn, 1);
    hipStream_t st = c->stream;
    PP_HIP(c->cf.err.reserve(2));
    PP_HIP(c->cf.memo.reserve(2 * std::max<size_t>(rows, 1)));
    PP_HIP(c->cf.items.reserve(1 + (size_t)total * kCfItem));
    // cf_line_kernel's workgroups: one line at a time each — latency-bound, so more lines in
    // flight than check_finish_kernel's grid
    const int wgs = std::min(kCfLineGrid, total);
    CfLines lines;
    if (wgs > 0) {
        int r = cf_line_buffers(c, wgs, std::min(total, kCfSpillCap), lines);
        if (r) return r;
    }
    if (int r = ensure_literal_pool(c, st)) return r;
    PP_HIP(c->batch.cfb_nodei.reserve(4 * nn));
    PP_HIP(c->batch.cfb_rows.reserve(std::max<size_t>(rows, 1)));
    PP_HIP(c->batch.cfb_rows8.reserve(2 * std::max<size_t>(rows, 1)));
    PP_HIP(c->batch.cfb_gotab.reserve(std::max(total, 1)));
    PP_HIP(c->batch.cfb_plist.reserve(std::max(total, 1)));
    PP_HIP(c->batch.cfb_tnode.reserve(cap_tasks));
    PP_HIP(c->batch.cfb_status.reserve(cap_tasks));
    PP_HIP(c->batch.cfb_lit.reserve(cap_tasks));
    PP_HIP(c->batch.cfb_tasks.reserve(cap_tasks));
    PP_HIP(c->batch.cfb_ext.reserve(cap_tasks));
    const size_t rec_cap = std::min(cap_tasks, kCfbRecChunk);
    PP_HIP(c->batch.cfb_rec.reserve(rec_cap));
    PP_HIP(c->batch.cfb_none.reserve(cap_tasks));
    PP_HIP(c->batch.cfb_yaw.reserve(cap_tasks));
    PP_HIP(c->batch.cfb_state.reserve(2));  // [0] the round's, [1] a chunk's
    PP_HIP(c->batch.cfb_misc.reserve(4));
    PP_HIP(c->batch.cfb_dhist.reserve(kCfbDepthBins));
    if (c->prof.on) PP_HIP(c->batch.cfb_pts.reserve(3 * kWalkTallySlots));
    SceneDev sd = c->scene_dev();
    sd.step_size = c->batch.f.step;
    if (int r = cf_upload_scene(c, sd)) return r;
    CfbArgs a;
    a.tr = tr;
    a.row_cap = cb_in.row_cap;
    a.nitems = total;
    a.Q = Q;
    a.qidx = cb_in.qidx;
    a.nodes = c->batch.mp_nodes.p;
    a.goals = cb_in.goals;
    a.moff = cb_in.moff;
    a.ftab = c->cf.memo.p;
    a.gtab = c->cf.memo.p + rows;
    a.gotab = c->batch.cfb_gotab.p;
    a.gclaim = c->batch.cfb_rows.p;
    a.tnone = c->batch.cfb_rows8.p;
    a.tnone_up = c->batch.cfb_rows8.p + rows;
    a.depth = c->batch.cfb_nodei.p;
    a.open = c->batch.cfb_nodei.p + nn;
    a.tfirst = c->batch.cfb_nodei.p + 2 * nn;
    a.tcnt = c->batch.cfb_nodei.p + 3 * nn;
    a.tnode = c->batch.cfb_tnode.p;
    a.tasks = c->batch.cfb_tasks.p;
    a.ext = c->batch.cfb_ext.p;
    a.rec = c->batch.cfb_rec.p;
    a.none = c->batch.cfb_none.p;
    a.status = c->batch.cfb_status.p;
    a.yaw = c->batch.cfb_yaw.p;
    a.st = c->batch.cfb_state.p;
    a.maxdepth = c->batch.cfb_misc.p;
    a.pcount = c->batch.cfb_misc.p + 1;
    a.wsum = c->batch.cfb_misc.p + 2;  // (the rounds' task counts: profiling)
    a.dhist = c->batch.cfb_dhist.p;
    // per launch: memo, goal verdicts, claims, line items, error bits, counters, DevState
    PP_HIP(hipMemsetAsync(c->cf.memo.p, 0, 2 * rows * sizeof(int), st));
    PP_HIP(hipMemsetAsync(c->batch.cfb_gotab.p, 0, (size_t)total * sizeof(int), st));
    PP_HIP(hipMemsetAsync(c->batch.cfb_rows.p, 0, rows * sizeof(int), st));
    PP_HIP(hipMemsetAsync(c->cf.items.p, 0, sizeof(int), st));
    PP_HIP(hipMemsetAsync(c->cf.err.p, 0, 2 * sizeof(int), st));
    PP_HIP(hipMemsetAsync(c->batch.cfb_misc.p, 0, 4 * sizeof(int), st));
    PP_HIP(hipMemsetAsync(c->batch.cfb_dhist.p, 0, kCfbDepthBins * sizeof(int), st));
    PP_HIP(hipMemsetAsync(c->batch.cfb_state.p, 0, 2 * sizeof(DevState), st));
    if (c->prof.on) PP_HIP(hipMemsetAsync(c->batch.cfb_pts.p, 0, 3 * kWalkTallySlots * sizeof(long long), st));
    if (c->prof.on) {
        if (int r = ensure_events(c, 2)) return r;
        PP_HIP(hipEventRecord(c->prof.ev[0], st));
    }
    PP_HIP(launch_cfb(st, sd, a, kCfbDepth, 0));
    int misc[4] = {0, 0, 0, 0};
    int dh[kCfbDepthBins];
    PP_HIP(hipMemcpyAsync(misc, c->batch.cfb_misc.p, sizeof misc, hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(dh, c->batch.cfb_dhist.p, sizeof dh, hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    // a bound on round (m0, span)'s tasks: a node of depth d emits min(span, d + 1 - m0) of them
    // (fewer once it settled); the last bin's nodes (that depth or more) count span each
    auto round_bound = [&](int m0, int span) -> size_t {
        size_t t = 0;
        for (int d = 0; d < kCfbDepthBins; ++d) {
            const int e = d == kCfbDepthBins - 1 ? span : std::min(span, d + 1 - m0);
            if (e > 0) t += (size_t)e * (size_t)dh[d];
        }
        return t;
    };
    // round r tests the candidates at depths m0 .. m0 + span - 1 of every open node: the first
    // round cfb_span0 of them, the later ones cfb_span
    long long* wpts = c->prof.on ? c->batch.cfb_pts.p : nullptr;
    // a round's steer over its a.st->W (<= mt) tasks, rec_cap records at a time
    auto steer = [&](int mt, bool own_yaw) -> int {
        for (size_t base = 0; base < (size_t)mt; base += rec_cap) {
            const int cn = (int)std::min(rec_cap, (size_t)mt - base);
            CfbArgs ac = a;
            ac.st = c->batch.cfb_state.p + 1;
            ac.tasks += base;
            ac.ext += base;
            ac.status += base;
            ac.yaw += base;
            PP_HIP(launch_cfb_chunk(st, a.st, ac.st, (int)base, cn, true, nullptr, nullptr));
            PP_HIP(launch_cfb_steer(st, sd, ac, cn, own_yaw, wpts));
            PP_HIP(launch_cfb_chunk(st, a.st, ac.st, (int)base, cn, false, ac.rec, a.none + base));
        }
        return PP_OK;
    };
    int rounds = 0;
    for (int m0 = 0; m0 <= misc[0]; ++rounds) {
        a.span = rounds == 0 ? span0 : span1;
        const int mt = (int)std::min<size_t>(cap_tasks, std::min<size_t>((size_t)a.span * nn,
                                                                         round_bound(m0, a.span)));
        PP_HIP(launch_cfb(st, sd, a, kCfbEmitA, m0));
        if (int r = steer(mt, false)) return r;
        PP_HIP(launch_cfb_literal(st, sd, a, mt, c->batch.cfb_lit.p, c->batch.cfb_misc.p + 3, c->api_lit_scratch.p));
        PP_HIP(launch_cfb(st, sd, a, kCfbConsumeA, m0));
        m0 += a.span;
    }
    PP_HIP(launch_cfb(st, sd, a, kCfbEmitB, 0));
    if (int r = steer((int)std::min<size_t>(cap_tasks, 2 * nn), true)) return r;
    PP_HIP(launch_cfb_literal(st, sd, a, (int)std::min<size_t>(cap_tasks, 2 * nn), c->batch.cfb_lit.p,
                              c->batch.cfb_misc.p + 3, c->api_lit_scratch.p));
    PP_HIP(launch_cfb(st, sd, a, kCfbStoreB, (int)std::min<size_t>(cap_tasks, 2 * nn)));
    PP_HIP(launch_cfb(st, sd, a, kCfbAssemble, 0, o.ok, o.len, o.npts, c->cf.err.p, c->cf.items.p,
                      c->batch.cfb_plist.p));
    PP_HIP(hipMemcpyAsync(misc, c->batch.cfb_misc.p, sizeof misc, hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    const int np = misc[1];
    CfBatch cb = cb_in;
    cb.ftab = a.ftab;
    cb.gtab = a.gtab;
    cb.gotab = a.gotab;
    // the items left (unknown verdicts) on check_finish_kernel, then every line item's points
    PP_HIP(c->cf.path.reserve((size_t)std::max(1, std::min(kCfGrid, (np + kCfWaves - 1) / kCfWaves)) *
                              kCfWaves * kCfMaxDepth));
    PP_HIP(launch_check_finish(st, sd, c->cf.scene.p, tr, c->batch.mp_nodes.p, np, 0.0, 0.0, 0.0, 0.0, 0,
                               kCfCheck, 1, o.ok, o.len, o.npts, nullptr, c->api_lit_scratch.p,
                               c->lit_locks.p, lines, c->cf.err.p, kCfGrid,
                               c->prof.on ? c->prof.cf_tally.p : nullptr, cb, c->cf.path.p, c->cf.items.p,
                               c->batch.cfb_plist.p));
    if (c->prof.on) PP_HIP(hipEventRecord(c->prof.ev[1], st));
    int err = 0;
    PP_HIP(hipMemcpyAsync(&err, c->cf.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(misc, c->batch.cfb_misc.p, sizeof misc, hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    if (c->prof.on) {
        float ms = 0.f;
        PP_HIP(hipEventElapsedTime(&ms, c->prof.ev[0], c->prof.ev[1]));
        c->prof.finish_ms += ms;
        c->prof.finish_launches += 1;
        c->prof.cfb_nodes += total - np;
        c->prof.cfb_edges += misc[2];
        std::vector<long long> v(3 * kWalkTallySlots);
        PP_HIP(hipMemcpy(v.data(), c->batch.cfb_pts.p, v.size() * sizeof(long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < 2 * (size_t)kWalkTallySlots; ++i)
            (i < (size_t)kWalkTallySlots ? c->prof.cfb_points : c->prof.cfb_arc) += v[i];
    }
    return cf_error(err);
}

// check_finish of the one-tree planner for cf_nodes[0, k) into the context's cf_* buffers
int cf_launch(pp_ctx* c, int k, int want_line, int grid, const CfGoal* g = nullptr) {
    const CfGoal dflt{c->rrt.goal[0], c->rrt.goal[1], c->rrt.goal[2], c->rrt.goal[2]};
    PP_HIP(c->cf.ok.reserve(kCfBatch));
    PP_HIP(c->cf.len.reserve(kCfBatch));
    PP_HIP(c->cf.npts.reserve(kCfBatch));
    PP_HIP(c->cf.chain.reserve((size_t)kCfBatch * (kCfLevels + 2)));
    return cf_run(c, c->rrt.tree_dev(), c->cf.nodes.p, k, want_line, grid, g ? *g : dflt,
                  CfOut{c->cf.ok.p, c->cf.len.p, c->cf.npts.p, c->cf.chain.p}, CfBatch{});
}

// ... for one node, on one workgroup
int cf_launch_one(pp_ctx* c, int32_t node, int want_line, const CfGoal* g = nullptr) {
    PP_HIP(c->cf.nodes.reserve(kCfBatch));
    PP_HIP(hipMemcpyAsync(c->cf.nodes.p, &node, sizeof(int), hipMemcpyHostToDevice, c->stream));
    return cf_launch(c, 1, want_line, 1, g);
}

// the line of a one-node launch (workgroup 0's buffer, E edges) into x / y; *n: its points
int cf_copy_line(pp_ctx* c, int E, double* x, double* y, int64_t* n) {
    std::vector<int> et(2 * (size_t)E);
    std::vector<double> hx(kCfPtsCap), hy(kCfPtsCap);
    PP_HIP(hipMemcpy(et.data(), c->cf.etab.p, et.size() * sizeof(int), hipMemcpyDeviceToHost));
    PP_HIP(hipMemcpy(hx.data(), c->cf.pts.p, kCfPtsCap * sizeof(double), hipMemcpyDeviceToHost));
    PP_HIP(hipMemcpy(hy.data(), c->cf.pts.p + kCfPtsCap, kCfPtsCap * sizeof(double), hipMemcpyDeviceToHost));
    int64_t w = 0;  // l.reverse() (rrt.rs:538)
    for (int e = E - 1; e >= 0; --e)
        for (int i = et[2 * e + 1] - 1; i >= 0; --i) {
            x[w] = hx[et[2 * e] + i];
            y[w] = hy[et[2 * e] + i];
            ++w;
        }
    if (n) *n = w;
    return PP_OK;
}

}  // namespace

namespace ppamd {

int paths_items(pp_ctx* c, const Forest& f, const int32_t* nodes, int* k) {
    const int Q = f.Q;
    hipStream_t st = c->stream;
    std::vector<int> hn, qi, nd, slot(Q, -1);
    if (int r = f.sizes(c, &hn, nullptr, nodes, "node index outside its query's tree")) return r;
    for (int q = 0; q < Q; ++q) {
        if (nodes[q] == -1) continue;
        slot[q] = (int)qi.size();
        qi.push_back(q);
        nd.push_back(nodes[q]);
    }
    *k = (int)qi.size();
    PathExport& pe = c->paths;
    PP_HIP(pe.qidx.reserve(Q));
    PP_HIP(pe.nodes.reserve(Q));
    PP_HIP(pe.slot.reserve(Q));
    PP_HIP(pe.ok.reserve(Q));
    PP_HIP(pe.cnt.reserve(Q));
    PP_HIP(pe.len.reserve(Q));
    PP_HIP(pe.off.reserve((size_t)Q + 1));
    PP_HIP(pe.okq.reserve(Q));
    // (pageable sources: the copies are complete when the calls return)
    PP_HIP(hipMemcpyAsync(pe.slot.p, slot.data(), Q * sizeof(int), hipMemcpyHostToDevice, st));
    if (*k > 0) {
        PP_HIP(hipMemcpyAsync(pe.qidx.p, qi.data(), *k * sizeof(int), hipMemcpyHostToDevice, st));
        PP_HIP(hipMemcpyAsync(pe.nodes.p, nd.data(), *k * sizeof(int), hipMemcpyHostToDevice, st));
    }
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

int paths_sizes(pp_ctx* c, int Q, int64_t* off, const double* x, const double* y, int64_t cap,
                int64_t* n_total, uint8_t* ok, bool* go) {
    PathExport& pe = c->paths;
    hipStream_t st = c->stream;
    *go = false;
    PP_HIP(launch_paths_scan(st, Q, pe.slot.p, pe.ok.p, pe.cnt.p, pe.off.p, pe.okq.p));
    PP_HIP(hipMemcpyAsync(off, pe.off.p, ((size_t)Q + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (ok) PP_HIP(hipMemcpyAsync(ok, pe.okq.p, Q, hipMemcpyDeviceToHost, st));
    // the one host round trip before the points: the staging and the capacity check need the total
    PP_HIP(hipStreamSynchronize(st));
    const int64_t total = off[Q];
    *n_total = total;
    if (!x || !y || cap <= 0 || total == 0) return PP_OK;  // the sizes only
    if (total > kPathsMaxPoints)
        return set_err(PP_ERR_CAPACITY, "the batch's lines exceed one call's staging (2^26 points): "
                                        "export the queries in several calls (nodes = -1 skips one)");
    if (cap < total) return set_err(PP_ERR_CAPACITY, "x / y smaller than the lines' total (n_total)");
    *go = true;
    return PP_OK;
}

int paths_line_buffers(pp_ctx* c, int k, CfLines& lines) {
    const int wgs = std::min(kCfLineGrid, k);
    return cf_line_buffers(c, wgs, wgs > 1 ? std::min(k, kCfSpillCap) : 0, lines);
}

int paths_write(pp_ctx* c, const SceneDev& sd, PathsArgs a, const CfLines& lines,
                const int* items, int k, bool star, double* x, double* y, int64_t total,
                double* len_host) {
    PathExport& pe = c->paths;
    hipStream_t st = c->stream;
    PP_HIP(pe.x.reserve((size_t)total));
    PP_HIP(pe.y.reserve((size_t)total));
    a.off = pe.off.p;
    a.ox = pe.x.p;
    a.oy = pe.y.p;
    PP_HIP(c->cf.err.reserve(2));
    PP_HIP(hipMemsetAsync(c->cf.err.p, 0, 2 * sizeof(int), st));
    PP_HIP(launch_paths(st, sd, a, lines, c->cf.err.p, items, k, star, true));
    int err = 0;
    PP_HIP(hipMemcpyAsync(&err, c->cf.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(x, pe.x.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(y, pe.y.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
    if (len_host)
        PP_HIP(hipMemcpyAsync(len_host, pe.len.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    if (err & 16) return set_err(PP_ERR_STATE, "packed export: a line's size changed between the passes");
    return cf_error(err);
}

int paths_batch_finish(pp_ctx* ctx, int k) {
    Batch& b = ctx->batch;
    PathExport& pe = ctx->paths;
    const int Q = b.f.Q;
    // check_finish of the k items: every item's verdict, optimize chain (a line item per verified
    // finish, cf.items) and, from its line pass, the line's point count
    PP_HIP(b.goal_d.reserve(3 * (size_t)Q));
    PP_HIP(hipMemcpyAsync(b.goal_d.p, b.goal.data(), 3 * (size_t)Q * sizeof(double),
                          hipMemcpyHostToDevice, ctx->stream));
    CfBatch cb;
    cb.qidx = pe.qidx.p;
    cb.row_cap = b.f.cap;
    cb.goals = b.goal_d.p;
    cb.blocked = b.f.blocked_dev();
    return cf_run(ctx, b.f.tree_dev(), pe.nodes.p, k, 1, kCfGrid, CfGoal{0.0, 0.0, 0.0, 0.0},
                  CfOut{pe.ok.p, pe.len.p, pe.cnt.p, nullptr}, cb);
}

}  // namespace ppamd

extern "C" {

int pp_batch_paths(pp_ctx* ctx, const int32_t* nodes, int64_t* off, double* x, double* y,
                   int64_t cap, int64_t* n_total, uint8_t* ok) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    Batch& b = ctx->batch;
    if (!b.valid) return set_err(PP_ERR_STATE, "pp_batch_new has not been called");
    if (!nodes || !off || !n_total) return set_err(PP_ERR_INVALID_ARGUMENT, "null nodes, off or n_total");
    const int Q = b.f.Q;
    PathExport& pe = ctx->paths;
    int k = 0;
    if ((r = paths_items(ctx, b.f, nodes, &k))) return r;
    *n_total = 0;
    if (k == 0) {
        std::fill(off, off + Q + 1, (int64_t)0);
        if (ok) std::fill(ok, ok + Q, (uint8_t)0);
        return PP_OK;
    }
    if ((r = paths_batch_finish(ctx, k))) return r;
    const TreeDev tr = b.f.tree_dev();
    bool go = false;
    if ((r = paths_sizes(ctx, Q, off, x, y, cap, n_total, ok, &go)) || !go) return r;
    CfLines lines;
    if ((r = paths_line_buffers(ctx, k, lines))) return r;
    SceneDev sd = ctx->scene_dev();
    sd.step_size = b.f.step;
    PathsArgs a;
    a.tr = tr;
    a.row_cap = b.f.cap;
    a.qidx = pe.qidx.p;
    a.nodes = pe.nodes.p;
    a.goals = b.goal_d.p;
    return paths_write(ctx, sd, a, lines, ctx->cf.items.p, k, false, x, y, *n_total);
}

int pp_rrt_check_finish_batch(pp_ctx* ctx, const int32_t* nodes, int k, uint8_t* ok,
                              double* length, int32_t* n_points, int32_t* chain) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (k < 0 || (k > 0 && (!nodes || !ok))) return set_err(PP_ERR_INVALID_ARGUMENT, "bad arguments");
    for (int i = 0; i < k; ++i)
        if (nodes[i] < 0 || nodes[i] >= ctx->rrt.n)
            return set_err(PP_ERR_INVALID_ARGUMENT, "node index outside the tree");
    const int want_line = (length || n_points) ? 1 : 0;
    std::vector<int> okv, npv;
    PP_HIP(ctx->cf.nodes.reserve(kCfBatch));
    for (int b = 0; b < k; b += kCfBatch) {
        const int nb = std::min(kCfBatch, k - b);
        PP_HIP(hipMemcpyAsync(ctx->cf.nodes.p, nodes + b, nb * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        if ((r = cf_launch(ctx, nb, want_line, kCfGrid))) return r;
        okv.resize(nb);
        PP_HIP(hipMemcpy(okv.data(), ctx->cf.ok.p, nb * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < nb; ++i) ok[b + i] = (uint8_t)okv[i];
        if (length) PP_HIP(hipMemcpy(length + b, ctx->cf.len.p, nb * sizeof(double), hipMemcpyDeviceToHost));
        if (n_points) PP_HIP(hipMemcpy(n_points + b, ctx->cf.npts.p, nb * sizeof(int), hipMemcpyDeviceToHost));
        if (chain)
            PP_HIP(hipMemcpy(chain + (size_t)b * (kCfLevels + 2), ctx->cf.chain.p,
                             (size_t)nb * (kCfLevels + 2) * sizeof(int), hipMemcpyDeviceToHost));
    }
    return PP_OK;
}

int pp_rrt_check_finish(pp_ctx* ctx, int32_t node, uint8_t* ok, double* x, double* y,
                        int64_t cap, int64_t* n, double* length) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (!ok || node < 0 || node >= ctx->rrt.n) return set_err(PP_ERR_INVALID_ARGUMENT, "bad arguments");
    if ((r = cf_launch_one(ctx, node, 1))) return r;
    int okv = 0, np = 0, row[kCfLevels + 2];
    double len = 0.0;
    PP_HIP(hipMemcpy(&okv, ctx->cf.ok.p, sizeof(int), hipMemcpyDeviceToHost));
    PP_HIP(hipMemcpy(&np, ctx->cf.npts.p, sizeof(int), hipMemcpyDeviceToHost));
    PP_HIP(hipMemcpy(&len, ctx->cf.len.p, sizeof(double), hipMemcpyDeviceToHost));
    PP_HIP(hipMemcpy(row, ctx->cf.chain.p, sizeof(row), hipMemcpyDeviceToHost));
    *ok = (uint8_t)okv;
    if (length) *length = len;
    if (n) *n = okv ? np : 0;
    if (!okv || !(x && y)) return PP_OK;
    if (cap < np) return set_err(PP_ERR_CAPACITY, "line buffer smaller than the finalized line");
    return cf_copy_line(ctx, row[1], x, y, n);
}

int pp_rrt_optimize(pp_ctx* ctx, int32_t node, int i, int32_t* chain, int* n_chain) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (!n_chain || node < 0 || node >= ctx->rrt.n || i < 0)
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad arguments");
    *n_chain = 0;
    if (i >= kCfLevels) return PP_OK;  // RECURSION_LIMIT (rrt.rs:464-466): None
    CfGoal g{ctx->rrt.goal[0], ctx->rrt.goal[1], ctx->rrt.goal[2], ctx->rrt.goal[2]};
    g.level0 = i;
    g.mode = kCfOptimize;
    if ((r = cf_launch_one(ctx, node, 0, &g))) return r;
    int row[kCfLevels + 2];
    PP_HIP(hipMemcpy(row, ctx->cf.chain.p, sizeof(row), hipMemcpyDeviceToHost));
    *n_chain = row[0];
    if (chain)
        for (int l = 0; l < row[0]; ++l) chain[l] = row[2 + l];
    return PP_OK;
}

int pp_rrt_finalize(pp_ctx* ctx, double gx, double gy, double gyaw, int32_t parent, double* x,
                    double* y, int64_t cap, int64_t* n, uint8_t* verified) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (!n || parent < 0 || parent >= ctx->rrt.n || !(std::fabs(gx) <= PP_COORD_MAX) ||
        !(std::fabs(gy) <= PP_COORD_MAX))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad arguments (the goal: finite, within PP_COORD_MAX)");
    CfGoal g{gx, gy, gyaw, ctx->rrt.goal[2]};
    g.mode = kCfFinalize;
    if ((r = cf_launch_one(ctx, parent, 1, &g))) return r;
    int okv = 0, np = 0, row[kCfLevels + 2];
    PP_HIP(hipMemcpy(&okv, ctx->cf.ok.p, sizeof(int), hipMemcpyDeviceToHost));
    PP_HIP(hipMemcpy(&np, ctx->cf.npts.p, sizeof(int), hipMemcpyDeviceToHost));
    PP_HIP(hipMemcpy(row, ctx->cf.chain.p, sizeof(row), hipMemcpyDeviceToHost));
    if (verified) *verified = (uint8_t)okv;
    *n = np;
    if (!(x && y) || cap == 0) return PP_OK;
    if (cap < np) return set_err(PP_ERR_CAPACITY, "line buffer smaller than the finalized line");
    // (an unverified line of more than 65536 points is counted on the device, never stored)
    if (ctx->cf.counted_only)
        return set_err(PP_ERR_CAPACITY, "finalized line longer than the point capacity");
    return cf_copy_line(ctx, row[1], x, y, n);
}

int pp_rrt_plan(pp_ctx* ctx, int64_t n_iter, int32_t* best_node, double* best_length,
                int64_t* n_finishes) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (n_iter < 0 || !best_node) return set_err(PP_ERR_INVALID_ARGUMENT, "bad arguments");
    const int64_t n0 = ctx->rrt.n;
    int64_t acc = 0;
    if ((r = pp_rrt_extend(ctx, n_iter, &acc))) return r;
    const int64_t n1 = ctx->rrt.n;
    std::vector<int32_t> nodes;
    nodes.reserve((size_t)(n1 - n0));
    for (int64_t i = n0; i < n1; ++i) nodes.push_back((int32_t)i);
    std::vector<uint8_t> okv(nodes.size());
    std::vector<double> lens(nodes.size());
    if (!nodes.empty() &&
        (r = pp_rrt_check_finish_batch(ctx, nodes.data(), (int)nodes.size(), okv.data(),
                                       lens.data(), nullptr, nullptr)))
        return r;
    // min_by(euclidean_length) over the finishes in iteration order: the first minimum wins
    int32_t bn = -1;
    double bl = __builtin_inf();
    int64_t nf = 0;
    for (size_t i = 0; i < nodes.size(); ++i) {
        if (!okv[i]) continue;
        ++nf;
        if (lens[i] < bl) {
            bl = lens[i];
            bn = nodes[i];
        }
    }
    *best_node = bn;
    if (best_length) *best_length = bl;
    if (n_finishes) *n_finishes = nf;
    return PP_OK;
}

int pp_batch_set_finish_schedule(pp_ctx* ctx, int rounds, int span0, int span) {
    if (!ctx) return set_err(PP_ERR_INVALID_ARGUMENT, "null context");
    if (rounds != 0 && rounds != 1) return set_err(PP_ERR_INVALID_ARGUMENT, "rounds must be 0 or 1");
    if (span0 < 0 || span0 > 16 || span < 0 || span > 16)
        return set_err(PP_ERR_INVALID_ARGUMENT, "span0 / span must be in [0, 16]");
    Batch& b = ctx->batch;
    b.cf_rounds = rounds != 0;
    b.cfb_span0 = span0 ? span0 : kCfbSpan;
    b.cfb_span = span ? span : kCfbSpan;
    return PP_OK;
}

int pp_batch_plan(pp_ctx* ctx, int32_t* best_node, double* length, int32_t* n_points,
                  int32_t* n_finishes, int64_t* n_checked) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    Batch& b = ctx->batch;
    if (!b.valid) return set_err(PP_ERR_STATE, "pp_batch_new has not been called");
    const int Q = b.f.Q;
    hipStream_t st = ctx->stream;
    // the accepted nodes of every query (1 .. n_q - 1, rrt.rs:591), flattened
    std::vector<int> hn, off((size_t)Q + 1, 0);
    if ((r = b.f.sizes(ctx, &hn))) return r;
    int64_t total = 0;
    for (int q = 0; q < Q; ++q) {
        off[q] = (int)total;
        total += std::max(hn[q] - 1, 0);
        if (total > (int64_t)0x7fff0000) return set_err(PP_ERR_CAPACITY, "too many nodes to plan");
    }
    off[Q] = (int)total;
    if (n_checked) *n_checked = total;
    const size_t tk = (size_t)std::max<int64_t>(total, 1);
    PP_HIP(b.mp_off.reserve((size_t)Q + 1));
    PP_HIP(b.mp_qidx.reserve(tk));
    PP_HIP(b.mp_nodes.reserve(tk));
    PP_HIP(b.mp_ok.reserve(tk));
    PP_HIP(b.mp_npts.reserve(tk));
    PP_HIP(b.mp_len.reserve(tk));
    PP_HIP(b.mp_best.reserve(Q));
    PP_HIP(b.mp_bpts.reserve(Q));
    PP_HIP(b.mp_nfin.reserve(Q));
    PP_HIP(b.mp_blen.reserve(Q));
    PP_HIP(b.goal_d.reserve(3 * (size_t)Q));
    PP_HIP(hipMemcpyAsync(b.mp_off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(b.goal_d.p, b.goal.data(), 3 * (size_t)Q * sizeof(double),
                          hipMemcpyHostToDevice, st));
    PP_HIP(launch_mq_plan_items(st, Q, b.mp_off.p, b.mp_qidx.p, b.mp_nodes.p));
    if (total > 0) {
        CfBatch cb;
        cb.qidx = b.mp_qidx.p;
        cb.row_cap = b.f.cap;
        cb.goals = b.goal_d.p;
        cb.blocked = b.f.blocked_dev();
        cb.moff = b.mp_off.p;  // compact memo rows
        const TreeDev tr = b.f.tree_dev();  // (query q: offset q * cb.row_cap)
        const CfGoal g{0.0, 0.0, 0.0, 0.0};  // (per query: cb.goals)
        const CfOut out{b.mp_ok.p, b.mp_len.p, b.mp_npts.p, nullptr};
        // steer rounds unless polygon mode or a blocked root (check_finish_kernel handles those)
        const bool rounds = b.cf_rounds && !cb.blocked && !ctx->scene.polygons();
        if ((r = rounds ? cf_run_rounds(ctx, tr, (int)total, cb, out)
                        : cf_run(ctx, tr, b.mp_nodes.p, (int)total, 1, kCfGrid, g, out, cb)))
            return r;
    }
    PP_HIP(launch_mq_plan_reduce(st, Q, b.mp_off.p, b.mp_ok.p, b.mp_len.p, b.mp_npts.p, b.mp_best.p,
                                 b.mp_blen.p, b.mp_bpts.p, b.mp_nfin.p));
    if (best_node) PP_HIP(hipMemcpyAsync(best_node, b.mp_best.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    if (length) PP_HIP(hipMemcpyAsync(length, b.mp_blen.p, Q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (n_points) PP_HIP(hipMemcpyAsync(n_points, b.mp_bpts.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    if (n_finishes) PP_HIP(hipMemcpyAsync(n_finishes, b.mp_nfin.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

}  // extern "C"

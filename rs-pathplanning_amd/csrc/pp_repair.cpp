// pp_repair.cpp — the re-attachment rounds of the RRT* batch and the two calls that run them.
// pp_star_repair: the batch's revalidation (pp_revalidate.cpp) with up to `rounds` rounds between
// its jump and its compaction, so that a dropped subtree whose top finds a feasible edge to a kept
// node is kept again (DESIGN.md §3.8 "Re-attaching orphaned subtrees"; the kernels:
// pp_k_repair.hip).  pp_star_advance: one node of every tree becomes its root.  The subtree under
// it is kept with its costs rebuilt from the new root; the new root's ancestors, whose edges point
// the wrong way, are round 1's tops, so that what hung from them is hung back where a feasible
// edge exists; the compaction puts the new root first (DESIGN.md §3.8 "Advancing the root"; the
// kernels: pp_k_advance.hip, pp_k_repair.hip).
#include "pp_ctx.h"

using namespace ppamd;

namespace {

// The rounds' buffers of Reval (for p->rv.total nodes; the slices' for slice_tasks tasks, <= 0: a
// call without rounds, none) and what of p points into them.  p->rv and the three keep-word rows
// are the caller's.
int repair_args(pp_ctx* c, int slice_tasks, const unsigned* vedge, const unsigned* vkeep,
                unsigned* vout, RepairArgs* p) {
    Reval& r = c->reval;
    const size_t z = (size_t)p->rv.total;
    for (auto* b : {&r.flag, &r.top}) PP_HIP(b->reserve(z));
    for (auto* b : {&r.lvl, &r.wpar, &r.tops}) PP_HIP(b->reserve(z));
    for (auto* b : {&r.wcost, &r.welen}) PP_HIP(b->reserve(z));
    if (slice_tasks > 0) {
        PP_HIP(r.tcost.reserve((size_t)slice_tasks));
        PP_HIP(r.tslot.reserve(kRepairTopsPerSlice));
    }
    PP_HIP(r.qhas.reserve((size_t)p->rv.Q));
    PP_HIP(r.rrec.reserve(1));
    p->ksched = c->star.ksched.p;
    p->vedge = vedge;
    p->vkeep = vkeep;
    p->vout = vout;
    p->flag = r.flag.p;
    p->top = r.top.p;
    p->lvl = r.lvl.p;
    p->wpar = r.wpar.p;
    p->wcost = r.wcost.p;
    p->welen = r.welen.p;
    p->tcost = r.tcost.p;
    p->tops = r.tops.p;
    p->tslot = r.tslot.p;
    p->qhas = r.qhas.p;
    p->rec = r.rrec.p;
    return PP_OK;
}

// Rounds 1 .. rounds over the staged arrays of p, stopping at a round without tops; *h: the last
// record read.  adv: pp_star_advance's arguments (p is their rp), whose round 1 takes the new
// root's ancestors as its tops; null: every round's tops are the repair's own.
int repair_rounds(pp_ctx* c, const SceneDev& sc, RepairArgs& p, int rounds, const AdvanceArgs* adv,
                  RepairRec* h) {
    Reval& r = c->reval;
    hipStream_t st = c->stream;
    for (int round = 1; round <= rounds; ++round) {
        if (adv && round == 1) PP_HIP(launch_advance_stage(st, *adv, kAdvanceTops, 0));
        else PP_HIP(launch_repair_stage(st, p, kRepairTops, round));
        // the one host read of a round: its tops (the slices' launch sizes, and the early
        // stop) and the error word of the rounds before it
        int herr = 0;
        PP_HIP(hipMemcpyAsync(h, r.rrec.p, sizeof(RepairRec), hipMemcpyDeviceToHost, st));
        PP_HIP(hipMemcpyAsync(&herr, r.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
        if (herr)
            return set_err(PP_ERR_STEER_OVERFLOW,
                           "generate_local_course would index past n_point (the reference panics)");
        const int ntops = h->ntops[round];
        if (ntops == 0) break;
        // (the stream is idle here: a buffer that grows frees nothing a kernel still reads)
        PP_HIP(r.tcnt.reserve((size_t)ntops));
        PP_HIP(r.near.reserve((size_t)ntops * kStarKMax));
        p.tcnt = r.tcnt.p;
        p.near = r.near.p;
        PP_HIP(launch_repair_knn(st, p, ntops));
        for (int t0 = 0; t0 < ntops; t0 += kRepairTopsPerSlice)
            PP_HIP(launch_repair_slice(st, sc, p, t0, std::min(ntops, t0 + kRepairTopsPerSlice)));
        PP_HIP(launch_repair_stage(st, p, kRepairGrow, round));
    }
    return PP_OK;
}

// a slice of tops steers at most kStarKMax candidates each
int slice_tasks(int64_t total) { return (int)std::min<int64_t>(total, kRepairTopsPerSlice) * kStarKMax; }

}  // namespace

extern "C" {

int pp_star_repair(pp_ctx* ctx, int rounds, int32_t* n_nodes, int64_t* n_dropped,
                   int64_t* n_reattached, int64_t* n_recovered, int32_t* new_index) {
    int rc = star_ready(ctx);
    if (rc) return rc;
    if (rounds < 0 || rounds > kRepairMaxRounds)
        return set_err(PP_ERR_INVALID_ARGUMENT, "rounds must be in [0, 16]");
    StarBatch& s = ctx->star;
    Forest& f = s.f;
    const int Q = f.Q;
    hipStream_t st = ctx->stream;
    std::vector<int> hn;
    std::vector<uint8_t> blk;
    bool any = false;
    if ((rc = f.reval_inputs(ctx, &hn, &blk, &any))) return rc;
    SceneDev sc = ctx->scene_dev();  // the scene of the batch's own steer rounds (star_args)
    sc.step_size = f.step;
    int64_t kept = 0, total = 0;
    for (int q = 0; q < Q; ++q) total += hn[(size_t)q];
    const int min_tasks = rounds > 0 ? slice_tasks(total) : 0;
    // a rewired node hangs under the later node that rewired it: parents in any order; cost and
    // elen travel with the rows, mark / stamp stay (reval_write_kernel)
    RevalArgs a;
    int passes = 0;
    if ((rc = reval_setup(ctx, f.tree_dev(), Q, (size_t)f.cap, hn, any ? blk.data() : nullptr,
                          f.n.p, true, s.cost.p, s.elen.p, min_tasks, &a, &passes)))
        return rc;
    Reval& r = ctx->reval;
    const size_t z = (size_t)a.total;
    if (rounds > 0) PP_HIP(r.vedge.reserve(z));
    PP_HIP(launch_reval_edges(st, sc, a));
    if (rounds > 0)  // the doubling overwrites the edge words
        PP_HIP(hipMemcpyAsync(r.vedge.p, a.v[0], z * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
    PP_HIP(launch_reval_jump(st, a, passes));
    const unsigned* v = a.v[passes & 1];
    RepairRec h{};
    if (rounds > 0) {
        RepairArgs p;
        p.rv = a;
        if ((rc = repair_args(ctx, min_tasks, r.vedge.p, v, a.v[(passes + 1) & 1], &p))) return rc;
        PP_HIP(hipMemsetAsync(r.rrec.p, 0, sizeof(RepairRec), st));
        PP_HIP(launch_repair_stage(st, p, kRepairInit, 0));
        if ((rc = repair_rounds(ctx, sc, p, rounds, nullptr, &h))) return rc;
        PP_HIP(launch_repair_stage(st, p, kRepairCommit, 0));
        PP_HIP(hipMemcpyAsync(&h, r.rrec.p, sizeof(RepairRec), hipMemcpyDeviceToHost, st));
        v = p.vout;
    }
    PP_HIP(launch_reval_compact(st, a, v));
    if ((rc = reval_finish(ctx, a, &kept, new_index))) return rc;
    if ((rc = f.reval_outputs(ctx, blk, any, n_nodes))) return rc;
    if (n_dropped) *n_dropped = total - kept;
    if (n_reattached) *n_reattached = h.reattached;
    if (n_recovered) *n_recovered = h.recovered;
    return PP_OK;
}

int pp_star_advance(pp_ctx* ctx, const int32_t* nodes, const int32_t* hops, int rounds,
                    int32_t* n_nodes, int64_t* n_dropped, int64_t* n_reattached,
                    int64_t* n_recovered, int32_t* new_index) {
    int rc = star_ready(ctx);
    if (rc) return rc;
    if (!nodes) return set_err(PP_ERR_INVALID_ARGUMENT, "nodes is NULL");
    if (rounds < 0 || rounds > kRepairMaxRounds)
        return set_err(PP_ERR_INVALID_ARGUMENT, "rounds must be in [0, 16]");
    StarBatch& s = ctx->star;
    Forest& f = s.f;
    const int Q = f.Q;
    hipStream_t st = ctx->stream;
    std::vector<int> hn;
    int64_t kept = 0, total = 0;
    if ((rc = f.sizes(ctx, &hn, &total, nodes, "a node must be -1 or a node of its query's tree")))
        return rc;
    for (int q = 0; hops && q < Q; ++q)
        if (hops[q] < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "a negative hop count");
    SceneDev sc = ctx->scene_dev();  // the scene of the batch's own steer rounds (star_args)
    sc.step_size = f.step;
    // rounds = 0: no steer at all.  No blocked roots: blocked[] stays (a root-blocked query has one
    // node and is left alone)
    const int min_tasks = rounds > 0 ? slice_tasks(total) : -1;
    AdvanceArgs a;
    RepairArgs& p = a.rp;
    int passes = 0;
    if ((rc = reval_setup(ctx, f.tree_dev(), Q, (size_t)f.cap, hn, nullptr, f.n.p, true, s.cost.p,
                          s.elen.p, min_tasks, &p.rv, &passes)))
        return rc;
    Reval& r = ctx->reval;
    PP_HIP(r.vedge.reserve((size_t)p.rv.total));
    PP_HIP(r.keep.reserve(3 * (size_t)Q));  // nodes, hops, root
    // (vout: the doubling's words are spent once the core is staged)
    if ((rc = repair_args(ctx, min_tasks, nullptr, nullptr, r.vedge.p, &p))) return rc;
    PP_HIP(hipMemcpy(r.keep.p, nodes, Q * sizeof(int), hipMemcpyHostToDevice));
    if (hops) PP_HIP(hipMemcpy(r.keep.p + Q, hops, Q * sizeof(int), hipMemcpyHostToDevice));
    a.nodes = r.keep.p;
    a.hops = hops ? r.keep.p + Q : nullptr;
    a.root = r.keep.p + 2 * (size_t)Q;
    a.starts = f.d_starts.p;
    RepairRec h{};
    PP_HIP(hipMemsetAsync(r.rrec.p, 0, sizeof(RepairRec), st));
    PP_HIP(launch_advance_stage(st, a, kAdvanceCore, passes));
    if ((rc = repair_rounds(ctx, sc, p, rounds, &a, &h))) return rc;
    if (rounds > 0)
        PP_HIP(hipMemcpyAsync(&h, r.rrec.p, sizeof(RepairRec), hipMemcpyDeviceToHost, st));
    PP_HIP(launch_advance_stage(st, a, kAdvanceKeep, 0));
    PP_HIP(launch_reval_scan(st, p.rv, p.vout, nullptr));
    PP_HIP(launch_advance_stage(st, a, kAdvanceGather, 0));
    PP_HIP(launch_reval_write(st, p.rv));
    PP_HIP(launch_advance_stage(st, a, kAdvanceStarts, 0));
    if (n_nodes) PP_HIP(hipMemcpyAsync(n_nodes, f.n.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    if ((rc = reval_finish(ctx, p.rv, &kept, new_index))) return rc;  // the synchronise at the end
    if (n_dropped) *n_dropped = total - kept;
    if (n_reattached) *n_reattached = h.reattached;
    if (n_recovered) *n_recovered = h.recovered;
    return PP_OK;
}

}  // extern "C"

// pp_advance.cpp — pp_star_advance: one node of every RRT* tree becomes its root.  The subtree
// under it is kept with its costs rebuilt from the new root; the new root's ancestors, whose edges
// point the wrong way, are round 1's tops of pp_star_repair's rounds (pp_repair.cpp), so that what
// hung from them is hung back where a feasible edge exists; the compaction puts the new root
// first (DESIGN.md §3.8 "Advancing the root"; the kernels: pp_k_advance.hip, pp_k_repair.hip).
#include "pp_ctx.h"

using namespace ppamd;

extern "C" {

int pp_star_advance(pp_ctx* ctx, const int32_t* nodes, const int32_t* hops, int rounds,
                    int32_t* n_nodes, int64_t* n_dropped, int64_t* n_reattached,
                    int64_t* n_recovered, int32_t* new_index) {
    int rc = check_ctx(ctx, true, false);
    if (rc) return rc;
    StarBatch& s = ctx->star;
    if (!s.valid) return set_err(PP_ERR_STATE, "no RRT* batch to advance: pp_star_new has not been called");
    if (!nodes) return set_err(PP_ERR_INVALID_ARGUMENT, "nodes is NULL");
    if (rounds < 0 || rounds > kRepairMaxRounds)
        return set_err(PP_ERR_INVALID_ARGUMENT, "rounds must be in [0, 16]");
    Forest& f = s.f;
    const int Q = f.Q;
    hipStream_t st = ctx->stream;
    std::vector<int> hn((size_t)Q, 0);
    PP_HIP(hipMemcpyAsync(hn.data(), f.n.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    int64_t kept = 0, total = 0;
    for (int q = 0; q < Q; ++q) {
        total += hn[(size_t)q];
        if (nodes[q] < -1 || nodes[q] >= hn[(size_t)q])
            return set_err(PP_ERR_INVALID_ARGUMENT, "a node must be -1 or a node of its query's tree");
        if (hops && hops[q] < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "a negative hop count");
    }
    SceneDev sc = ctx->scene_dev();  // the scene of the batch's own steer rounds (star_args)
    sc.step_size = f.step;
    // a slice of tops steers at most kStarKMax candidates each; rounds = 0: no steer at all.  No
    // blocked roots: blocked[] stays (a root-blocked query has one node and is left alone)
    const int min_tasks =
        rounds > 0 ? (int)std::min<int64_t>(total, kRepairTopsPerSlice) * kStarKMax : -1;
    AdvanceArgs a;
    RepairArgs& p = a.rp;
    int passes = 0;
    if ((rc = reval_setup(ctx, f.tree_dev(), Q, (size_t)f.cap, hn, nullptr, f.n.p, true, s.cost.p,
                          s.elen.p, min_tasks, &p.rv, &passes)))
        return rc;
    Reval& r = ctx->reval;
    const size_t z = (size_t)p.rv.total;
    for (auto* b : {&r.flag, &r.top}) PP_HIP(b->reserve(z));
    for (auto* b : {&r.lvl, &r.wpar, &r.tops}) PP_HIP(b->reserve(z));
    for (auto* b : {&r.wcost, &r.welen}) PP_HIP(b->reserve(z));
    PP_HIP(r.vedge.reserve(z));
    PP_HIP(r.qhas.reserve((size_t)Q));
    PP_HIP(r.rrec.reserve(1));
    PP_HIP(r.keep.reserve(3 * (size_t)Q));  // nodes, hops, root
    if (rounds > 0) {
        PP_HIP(r.tcost.reserve((size_t)min_tasks));
        PP_HIP(r.tslot.reserve(kRepairTopsPerSlice));
    }
    PP_HIP(hipMemcpy(r.keep.p, nodes, Q * sizeof(int), hipMemcpyHostToDevice));
    if (hops) PP_HIP(hipMemcpy(r.keep.p + Q, hops, Q * sizeof(int), hipMemcpyHostToDevice));
    a.nodes = r.keep.p;
    a.hops = hops ? r.keep.p + Q : nullptr;
    a.root = r.keep.p + 2 * (size_t)Q;
    a.starts = f.d_starts.p;
    p.ksched = s.ksched.p;
    p.vout = r.vedge.p;  // (the doubling's words are spent once the core is staged)
    p.flag = r.flag.p;
    p.top = r.top.p;
    p.lvl = r.lvl.p;
    p.wpar = r.wpar.p;
    p.wcost = r.wcost.p;
    p.welen = r.welen.p;
    p.tcost = r.tcost.p;
    p.tops = r.tops.p;
    p.tslot = r.tslot.p;
    p.qhas = r.qhas.p;
    p.rec = r.rrec.p;
    RepairRec h{};
    PP_HIP(hipMemsetAsync(r.rrec.p, 0, sizeof(RepairRec), st));
    PP_HIP(launch_advance_stage(st, a, kAdvanceCore, passes));
    for (int round = 1; round <= rounds; ++round) {
        // round 1's tops are the new root's ancestors; later rounds' are the repair's own
        if (round == 1) PP_HIP(launch_advance_stage(st, a, kAdvanceTops, 0));
        else PP_HIP(launch_repair_stage(st, p, kRepairTops, round));
        // the one host read of a round, as pp_star_repair's
        int herr = 0;
        PP_HIP(hipMemcpyAsync(&h, r.rrec.p, sizeof(RepairRec), hipMemcpyDeviceToHost, st));
        PP_HIP(hipMemcpyAsync(&herr, r.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
        if (herr)
            return set_err(PP_ERR_STEER_OVERFLOW,
                           "generate_local_course would index past n_point (the reference panics)");
        const int ntops = h.ntops[round];
        if (ntops == 0) break;
        PP_HIP(r.tcnt.reserve((size_t)ntops));
        PP_HIP(r.near.reserve((size_t)ntops * kStarKMax));
        p.tcnt = r.tcnt.p;
        p.near = r.near.p;
        PP_HIP(launch_repair_knn(st, p, ntops));
        for (int t0 = 0; t0 < ntops; t0 += kRepairTopsPerSlice)
            PP_HIP(launch_repair_slice(st, sc, p, t0, std::min(ntops, t0 + kRepairTopsPerSlice)));
        PP_HIP(launch_repair_stage(st, p, kRepairGrow, round));
    }
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

// pp_repair.cpp — pp_star_repair: the RRT* batch's revalidation (pp_revalidate.cpp) with up to
// `rounds` re-attachment rounds between its jump and its compaction, so that a dropped subtree
// whose top finds a feasible edge to a kept node is kept again (DESIGN.md §3.8 "Re-attaching
// orphaned subtrees"; the kernels: pp_k_repair.hip).
#include "pp_ctx.h"

using namespace ppamd;

extern "C" {

int pp_star_repair(pp_ctx* ctx, int rounds, int32_t* n_nodes, int64_t* n_dropped,
                   int64_t* n_reattached, int64_t* n_recovered, int32_t* new_index) {
    int rc = check_ctx(ctx, true, false);
    if (rc) return rc;
    StarBatch& s = ctx->star;
    if (!s.valid) return set_err(PP_ERR_STATE, "no RRT* batch to repair: pp_star_new has not been called");
    if (rounds < 0 || rounds > kRepairMaxRounds)
        return set_err(PP_ERR_INVALID_ARGUMENT, "rounds must be in [0, 16]");
    Forest& f = s.f;
    const int Q = f.Q;
    hipStream_t st = ctx->stream;
    std::vector<int> hn;
    std::vector<uint8_t> blk;
    bool any = false;
    if ((rc = star_reval_inputs(ctx, &hn, &blk, &any))) return rc;
    SceneDev sc = ctx->scene_dev();  // the scene of the batch's own steer rounds (star_args)
    sc.step_size = f.step;
    int64_t kept = 0, total = 0;
    for (int q = 0; q < Q; ++q) total += hn[(size_t)q];
    // a slice of tops steers at most kStarKMax candidates each
    const int min_tasks =
        rounds > 0 ? (int)std::min<int64_t>(total, kRepairTopsPerSlice) * kStarKMax : 0;
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
        for (auto* b : {&r.flag, &r.top}) PP_HIP(b->reserve(z));
        for (auto* b : {&r.lvl, &r.wpar, &r.tops}) PP_HIP(b->reserve(z));
        for (auto* b : {&r.wcost, &r.welen}) PP_HIP(b->reserve(z));
        PP_HIP(r.tcost.reserve((size_t)min_tasks));
        PP_HIP(r.tslot.reserve(kRepairTopsPerSlice));
        PP_HIP(r.qhas.reserve((size_t)Q));
        PP_HIP(r.rrec.reserve(1));
        RepairArgs p;
        p.rv = a;
        p.ksched = s.ksched.p;
        p.vedge = r.vedge.p;
        p.vkeep = v;
        p.vout = a.v[(passes + 1) & 1];
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
        PP_HIP(hipMemsetAsync(r.rrec.p, 0, sizeof(RepairRec), st));
        PP_HIP(launch_repair_stage(st, p, kRepairInit, 0));
        for (int round = 1; round <= rounds; ++round) {
            PP_HIP(launch_repair_stage(st, p, kRepairTops, round));
            // the one host read of a round: its tops (the slices' launch sizes, and the early
            // stop) and the error word of the rounds before it
            int herr = 0;
            PP_HIP(hipMemcpyAsync(&h, r.rrec.p, sizeof(RepairRec), hipMemcpyDeviceToHost, st));
            PP_HIP(hipMemcpyAsync(&herr, r.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
            PP_HIP(hipStreamSynchronize(st));
            if (herr)
                return set_err(PP_ERR_STEER_OVERFLOW,
                               "generate_local_course would index past n_point (the reference panics)");
            const int ntops = h.ntops[round];
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
        PP_HIP(launch_repair_stage(st, p, kRepairCommit, 0));
        PP_HIP(hipMemcpyAsync(&h, r.rrec.p, sizeof(RepairRec), hipMemcpyDeviceToHost, st));
        v = p.vout;
    }
    PP_HIP(launch_reval_compact(st, a, v));
    if ((rc = reval_finish(ctx, a, &kept, new_index))) return rc;
    if ((rc = star_reval_outputs(ctx, blk, any, n_nodes))) return rc;
    if (n_dropped) *n_dropped = total - kept;
    if (n_reattached) *n_reattached = h.reattached;
    if (n_recovered) *n_recovered = h.recovered;
    return PP_OK;
}

}  // extern "C"

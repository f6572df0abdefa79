// pp_relax.cpp — pp_star_relax: up to `rounds` synchronous choose-parent rounds over all nodes of
// the RRT* batch's trees, on the device and in place (DESIGN.md §3.8 "Relaxing the trees"; the
// kernels: pp_k_relax.hip).  A round is a run of node slices, each a kNN-and-emit, the steer round
// and a choose, then one commit; the host reads the round's rewire count and the error word once
// per round and everything else once at the end.
#include "pp_ctx.h"

using namespace ppamd;

extern "C" {

int pp_star_relax(pp_ctx* ctx, int rounds, const uint8_t* active, int32_t* n_rewired,
                  int32_t* rounds_run, int64_t* n_changed) {
    int rc = star_ready(ctx);
    if (rc) return rc;
    if (rounds < 1 || rounds > kRelaxMaxRounds)
        return set_err(PP_ERR_INVALID_ARGUMENT, "rounds must be in [1, 16]");
    StarBatch& s = ctx->star;
    Forest& f = s.f;
    const int Q = f.Q;
    hipStream_t st = ctx->stream;
    std::vector<int> hn;
    int64_t total64 = 0;
    if ((rc = f.sizes(ctx, &hn, &total64))) return rc;
    if (total64 > (int64_t)0x7fff0000)
        return set_err(PP_ERR_CAPACITY, "more than 2^31 nodes to relax");
    const int total = (int)total64;
    std::vector<int> off((size_t)Q + 1, 0);
    int nmax = 1;
    for (int q = 0; q < Q; ++q) {
        if (hn[(size_t)q] < 1) return set_err(PP_ERR_STATE, "a tree without its root");
        off[(size_t)q + 1] = off[(size_t)q] + hn[(size_t)q];
        nmax = std::max(nmax, hn[(size_t)q]);
    }
    if (rounds_run) *rounds_run = 0;
    if (n_changed) *n_changed = 0;
    if (n_rewired) std::fill(n_rewired, n_rewired + Q, 0);
    int64_t* last = ctx->reval.relax_last;  // what pp_star_relax_counts reports
    std::fill(last, last + 8, (int64_t)0);
    if (nmax < 2) {  // lone roots: the one round that re-parents nothing, without a launch
        if (rounds_run) *rounds_run = 1;
        return PP_OK;
    }
    // the most candidates of a node: star_k does not fall as the tree grows
    const int kmax = star_k(s.kfix, nmax - 1);
    SceneDev sc = ctx->scene_dev();  // the scene of the batch's own steer rounds (star_args)
    sc.step_size = f.step;

    Reval& r = ctx->reval;
    const size_t z = (size_t)total;
    const int slice = std::min(total, kRelaxNodesPerSlice);
    const size_t tasks = (size_t)slice * (size_t)kmax;
    PP_HIP(r.tasks.reserve(tasks));
    PP_HIP(r.ext.reserve(tasks));
    PP_HIP(r.rec.reserve(tasks));
    PP_HIP(r.status.reserve(tasks));
    PP_HIP(r.yaw.reserve(tasks));
    PP_HIP(r.tcost.reserve(tasks));
    PP_HIP(r.state.reserve(1));
    PP_HIP(r.err.reserve(1));
    PP_HIP(r.off.reserve((size_t)Q + 1));
    PP_HIP(r.tslot.reserve(kRelaxNodesPerSlice));
    PP_HIP(r.tcnt.reserve(kRelaxNodesPerSlice));
    PP_HIP(r.wpar.reserve(z));
    PP_HIP(r.welen.reserve(z));
    PP_HIP(r.lvl.reserve(z));
    PP_HIP(r.flag.reserve(z));           // chg
    PP_HIP(r.keep.reserve((size_t)Q));   // nrw
    PP_HIP(r.relax_rec.reserve(1));
    if (active) PP_HIP(r.qhas.reserve((size_t)Q));
    if ((rc = ensure_literal_pool(ctx, st))) return rc;
    PP_HIP(hipMemcpy(r.off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
    if (active) {
        std::vector<uint8_t> act((size_t)Q);
        for (int q = 0; q < Q; ++q) act[(size_t)q] = active[q] ? 1 : 0;
        PP_HIP(hipMemcpy(r.qhas.p, act.data(), (size_t)Q, hipMemcpyHostToDevice));
    }
    PP_HIP(hipMemsetAsync(r.state.p, 0, sizeof(DevState), st));
    PP_HIP(hipMemsetAsync(r.err.p, 0, sizeof(int), st));
    PP_HIP(hipMemsetAsync(r.flag.p, 0, z, st));
    PP_HIP(hipMemsetAsync(r.keep.p, 0, (size_t)Q * sizeof(int), st));
    PP_HIP(hipMemsetAsync(r.relax_rec.p, 0, sizeof(RelaxRec), st));

    RelaxArgs a;
    a.tr = f.tree_dev();
    a.Q = Q;
    a.cap = (size_t)f.cap;
    a.off = r.off.p;
    a.total = total;
    a.blocked = f.blocked_dev();
    a.active = active ? r.qhas.p : nullptr;
    a.cost = s.cost.p;
    a.elen = s.elen.p;
    a.rewires = s.rew.p;
    a.ksched = s.ksched.p;
    a.curv = 1.0 / ctx->scene.max_steer;
    a.kmax = kmax;
    a.task_cap = (int)tasks;
    a.tasks = r.tasks.p;
    a.ext = r.ext.p;
    a.rec = r.rec.p;
    a.status = r.status.p;
    a.yaw = r.yaw.p;
    a.tcost = r.tcost.p;
    a.st = r.state.p;
    a.tslot = r.tslot.p;
    a.tcnt = r.tcnt.p;
    a.wpar = r.wpar.p;
    a.welen = r.welen.p;
    a.lvl = r.lvl.p;
    a.chg = r.flag.p;
    a.nrw = r.keep.p;
    a.rrec = r.relax_rec.p;
    a.stats = ctx->prof.on ? 1 : 0;
    a.err = r.err.p;
    a.lit_scratch = ctx->api_lit_scratch.p;
    a.lit_locks = ctx->lit_locks.p;
    a.wg_points = ctx->prof.points();

    RelaxRec h{};
    int run = 0, herr = 0, before = 0;
    for (int round = 1; round <= rounds; ++round) {
        for (int g0 = 0; g0 < total; g0 += kRelaxNodesPerSlice)
            PP_HIP(launch_relax_slice(st, sc, a, g0, std::min(total, g0 + kRelaxNodesPerSlice)));
        PP_HIP(launch_relax_commit(st, a));
        // the one host read of a round: its rewires (the early stop) and the error word
        PP_HIP(hipMemcpyAsync(&h, r.relax_rec.p, sizeof(RelaxRec), hipMemcpyDeviceToHost, st));
        PP_HIP(hipMemcpyAsync(&herr, r.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
        if (herr) break;  // the round was not applied; the rounds before it stay
        run = round;
        if (h.rewired == before) break;
        before = h.rewired;
    }
    if (n_rewired)
        PP_HIP(hipMemcpyAsync(n_rewired, r.keep.p, (size_t)Q * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    if (rounds_run) *rounds_run = run;
    if (n_changed) *n_changed = h.changed;
    last[0] = total;
    last[1] = h.cand;
    last[2] = h.not_parent;
    last[3] = h.cheaper;
    last[4] = h.tasks;
    last[5] = h.walked;
    last[6] = (int64_t)((total + kRelaxNodesPerSlice - 1) / kRelaxNodesPerSlice);
    last[7] = kmax;
    if (herr)
        return set_err(PP_ERR_STEER_OVERFLOW,
                       "generate_local_course would index past n_point (the reference panics)");
    return PP_OK;
}

int pp_star_relax_counts(pp_ctx* ctx, int64_t out[8]) {
    int rc = star_ready(ctx);
    if (rc) return rc;
    if (!out) return set_err(PP_ERR_INVALID_ARGUMENT, "out is NULL");
    std::copy(ctx->reval.relax_last, ctx->reval.relax_last + 8, out);
    return PP_OK;
}

}  // extern "C"

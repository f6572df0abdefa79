// pp_revalidate.cpp — a tree across a scene change: pp_rrt_revalidate, pp_batch_revalidate and
// pp_star_revalidate re-verify the tree(s) on the device against the context's current Space, drop
// every node whose line_to_origin (RRT*: whose chain of stored edges to the root) no longer
// verifies and derive again what pp_rrt_new / pp_batch_new / pp_star_new derive from the scene
// (DESIGN.md §3.8).
#include "pp_ctx.h"

using namespace ppamd;

namespace ppamd {

int reval_setup(pp_ctx* c, const TreeDev& tr, int Q, size_t cap, const std::vector<int>& hn,
                const uint8_t* blocked, int* d_n, bool any_order, double* cost, double* elen,
                int min_tasks, RevalArgs* out, int* passes_out) {
    Reval& r = c->reval;
    std::vector<int> off((size_t)Q + 1, 0);
    int64_t total64 = 0;
    int nmax = 1;
    for (int q = 0; q < Q; ++q) {
        if (hn[q] < 1) return set_err(PP_ERR_STATE, "a tree without its root");
        total64 += hn[q];
        if (total64 > (int64_t)0x7fff0000)
            return set_err(PP_ERR_CAPACITY, "more than 2^31 nodes to revalidate");
        off[(size_t)q + 1] = (int)total64;
        nmax = std::max(nmax, hn[q]);
    }
    const int total = (int)total64;
    const size_t z = (size_t)total;
    const int slice = std::min(total, kRevalSlice);
    const bool steers = min_tasks >= 0;  // (pp_star_prune: verdicts without a steer round)
    const int tasks = steers ? std::max(slice, min_tasks) : 0;
    PP_HIP(r.tasks.reserve(tasks));
    PP_HIP(r.ext.reserve(tasks));
    PP_HIP(r.rec.reserve(tasks));
    PP_HIP(r.status.reserve(tasks));
    PP_HIP(r.yaw.reserve(tasks));
    PP_HIP(r.state.reserve(1));
    PP_HIP(r.err.reserve(1));
    PP_HIP(r.off.reserve((size_t)Q + 1));
    PP_HIP(r.bsum.reserve((z + 1023) / 1024));
    PP_HIP(r.pos.reserve(z + 1));
    for (auto* b : {&r.new_index, &r.spar}) PP_HIP(b->reserve(z));
    for (auto* b : {&r.sx, &r.sy, &r.syaw}) PP_HIP(b->reserve(z));
    if (cost)
        for (auto* b : {&r.scost, &r.selen}) PP_HIP(b->reserve(z));
    PP_HIP(r.srow.reserve(z));
    PP_HIP(r.v0.reserve(z));
    PP_HIP(r.v1.reserve(z));
    if (blocked) PP_HIP(r.blocked.reserve(Q));
    hipStream_t st = c->stream;
    int rc;
    if (steers && (rc = ensure_literal_pool(c, st))) return rc;
    PP_HIP(hipMemcpy(r.off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
    if (blocked) PP_HIP(hipMemcpy(r.blocked.p, blocked, Q, hipMemcpyHostToDevice));
    PP_HIP(hipMemsetAsync(r.state.p, 0, sizeof(DevState), st));
    PP_HIP(hipMemsetAsync(r.err.p, 0, sizeof(int), st));
    RevalArgs a;
    a.tr = tr;
    a.Q = Q;
    a.cap = cap;
    a.off = r.off.p;
    a.total = total;
    a.blocked = blocked ? r.blocked.p : nullptr;
    a.n = d_n;
    a.any_order = any_order ? 1 : 0;
    a.cost = cost;
    a.elen = elen;
    a.scost = cost ? r.scost.p : nullptr;
    a.selen = cost ? r.selen.p : nullptr;
    a.slice = slice;
    a.tasks = r.tasks.p;
    a.ext = r.ext.p;
    a.rec = r.rec.p;
    a.status = r.status.p;
    a.yaw = r.yaw.p;
    a.st = r.state.p;
    a.v[0] = r.v0.p;
    a.v[1] = r.v1.p;
    a.bsum = r.bsum.p;
    a.pos = r.pos.p;
    a.new_index = r.new_index.p;
    a.sx = r.sx.p;
    a.sy = r.sy.p;
    a.syaw = r.syaw.p;
    a.spar = r.spar.p;
    a.srow = r.srow.p;
    a.err = r.err.p;
    a.lit_scratch = c->api_lit_scratch.p;
    a.lit_locks = c->lit_locks.p;
    a.wg_points = c->prof.points();
    // a tree of n nodes is at most n - 1 edges deep, whatever the order of its parents
    int passes = 0;
    while (((int64_t)1 << passes) < nmax) ++passes;
    *out = a;
    *passes_out = passes;
    return PP_OK;
}

int reval_finish(pp_ctx* c, const RevalArgs& a, int64_t* kept, int32_t* new_index) {
    Reval& r = c->reval;
    hipStream_t st = c->stream;
    const int total = a.total;
    const size_t z = (size_t)total;
    int h[2] = {0, 0};  // kept nodes, error word
    PP_HIP(hipMemcpyAsync(&h[0], r.pos.p + total, sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(&h[1], r.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    if (new_index)
        PP_HIP(hipMemcpyAsync(new_index, r.new_index.p, z * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    if (h[1])
        return set_err(PP_ERR_STEER_OVERFLOW,
                       "generate_local_course would index past n_point (the reference panics)");
    *kept = h[0];
    return PP_OK;
}

}  // namespace ppamd

namespace {

// The device pass over Q trees of hn[q] nodes in the rows tr (tree q at q * cap): *kept the nodes
// that stay over all trees; new_index (may be null) the sum of hn entries.  blocked (host, may be
// null): the roots that fail verify.  d_n (may be null): the trees' node counts on the device.
// One synchronisation; on PP_ERR_STEER_OVERFLOW the trees are unmodified.
int reval_run(pp_ctx* c, const SceneDev& sc, const TreeDev& tr, int Q, size_t cap,
              const std::vector<int>& hn, const uint8_t* blocked, int* d_n, int64_t* kept,
              int32_t* new_index) {
    RevalArgs a;
    int passes = 0, rc;
    if ((rc = reval_setup(c, tr, Q, cap, hn, blocked, d_n, false, nullptr, nullptr, 0, &a, &passes)))
        return rc;
    PP_HIP(launch_revalidate(c->stream, sc, a, passes));
    return reval_finish(c, a, kept, new_index);
}

// the f32 screen tolerance pp_rrt_new derives from the scene and the root
double eps_coord_for(const Scene& s, double rx, double ry) {
    const double mx = std::max({std::fabs(s.minx), std::fabs(s.maxx), std::fabs(s.miny),
                                std::fabs(s.maxy), std::fabs(rx), std::fabs(ry)});
    return mx * std::ldexp(1.0, -23);
}

}  // namespace

extern "C" {

int pp_rrt_revalidate(pp_ctx* ctx, int64_t* n_kept, int32_t* new_index) {
    int rc = check_ctx(ctx, true, false);
    if (rc) return rc;
    Planner& p = ctx->rrt;
    if (!p.valid && !p.stale) return set_err(PP_ERR_STATE, "no tree to revalidate: pp_rrt_new has not been called");
    PP_HIP(hipStreamSynchronize(ctx->stream));
    if (p.n < 1 || p.n > p.cap) return set_err(PP_ERR_STATE, "the planner holds no tree");
    // what pp_rrt_new derives from the scene, for the scene as it is now (a root that fails verify
    // fails every line that ends in it; the kernels' incremental verify assumes a free root)
    const bool blocked = ctx->scene.polygons() && !ctx->scene.point_ok(p.start[0], p.start[1]);
    const SceneDev sc = ctx->scene.dev(p.step, blocked);
    const uint8_t blk = blocked ? 1 : 0;
    int64_t kept = 0;
    if ((rc = reval_run(ctx, sc, p.tree_dev(), 1, (size_t)p.cap, std::vector<int>{(int)p.n},
                        blocked ? &blk : nullptr, nullptr, &kept, new_index)))
        return rc;
    // the planner continues on the pruned tree, as after pp_rrt_tree_import: its iteration
    // counter, seed, goal, window and statistics stay
    DevState& s = p.h_state.p[0];
    PP_HIP(hipMemcpy(&s, p.d_state.p, sizeof(DevState), hipMemcpyDeviceToHost));
    s.n = (int)kept;
    s.n_scan = (int)kept;
    s.it_spec = s.it;
    s.void_seq = -1;
    s.kdyn = kMinDynWindow;
    PP_HIP(hipMemcpy(p.d_state.p, &s, sizeof(DevState), hipMemcpyHostToDevice));
    p.n = kept;
    p.eps_coord = eps_coord_for(ctx->scene, p.start[0], p.start[1]);
    p.root_blocked = blocked;
    p.stale = false;
    p.valid = true;
    if (n_kept) *n_kept = kept;
    return PP_OK;
}

int pp_batch_revalidate(pp_ctx* ctx, int32_t* n_nodes, int64_t* n_dropped, int32_t* new_index) {
    int rc = check_ctx(ctx, true, false);
    if (rc) return rc;
    Batch& b = ctx->batch;
    if (!b.valid && !b.stale) return set_err(PP_ERR_STATE, "no batch to revalidate: pp_batch_new has not been called");
    Forest& f = b.f;
    const int Q = f.Q;
    std::vector<int> hn;
    std::vector<uint8_t> blk;
    bool any = false;
    if ((rc = f.reval_inputs(ctx, &hn, &blk, &any))) return rc;
    SceneDev sc = ctx->scene.dev(f.step, false);
    int64_t kept = 0, total = 0;
    for (int q = 0; q < Q; ++q) total += hn[(size_t)q];
    if ((rc = reval_run(ctx, sc, f.tree_dev(), Q, (size_t)f.cap, hn, any ? blk.data() : nullptr,
                        f.n.p, &kept, new_index)))
        return rc;
    // the verdict cache holds the old scene's verdicts
    PP_HIP(hipMemsetAsync(b.itprev.p, 0x80, Q * sizeof(int64_t), ctx->stream));
    if ((rc = f.reval_outputs(ctx, blk, any, n_nodes))) return rc;
    b.stale = false;
    b.valid = true;
    if (n_dropped) *n_dropped = total - kept;
    return PP_OK;
}

int pp_star_revalidate(pp_ctx* ctx, int32_t* n_nodes, int64_t* n_dropped, int32_t* new_index) {
    // the repair (pp_repair.cpp) without a re-attachment round: its edge test, jump and compaction
    return pp_star_repair(ctx, 0, n_nodes, n_dropped, nullptr, nullptr, new_index);
}

}  // extern "C"

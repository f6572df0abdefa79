// pp_prune.cpp — pp_star_prune: drop from every tree of the RRT* batch the nodes that, at their
// stored cost, cannot lie on a path to the query's focus within its bound, and their descendants
// (the second half of Informed RRT*; DESIGN.md §3.7 "Pruning by the focus bound").  The verdicts
// are pp_k_prune.hip's; the doubling, the compaction and the two host halves around them are the
// revalidation's (pp_revalidate.cpp), without its steer slice: the scene gives the turn radius and
// nothing else.
#include "pp_ctx.h"

using namespace ppamd;

extern "C" {

int pp_star_prune(pp_ctx* ctx, const int32_t* keep, int32_t* n_nodes, int64_t* n_dropped,
                  int32_t* new_index) {
    int rc = star_ready(ctx);
    if (rc) return rc;
    StarBatch& s = ctx->star;
    Forest& f = s.f;
    const int Q = f.Q;
    hipStream_t st = ctx->stream;
    std::vector<int> hn;
    int64_t kept = 0, total = 0;
    if ((rc = f.sizes(ctx, &hn, &total, keep, "a keep node must be -1 or a node of its query's tree")))
        return rc;
    // parents in any order, cost and elen travel with the rows, mark / stamp stay
    // (pp_star_revalidate's); no blocked roots: the scene is not consulted, blocked[] stays
    PruneArgs p;
    int passes = 0;
    if ((rc = reval_setup(ctx, f.tree_dev(), Q, (size_t)f.cap, hn, nullptr, f.n.p, true, s.cost.p,
                          s.elen.p, -1, &p.rv, &passes)))
        return rc;
    Reval& r = ctx->reval;
    if (keep) {
        PP_HIP(r.keep.reserve((size_t)Q));
        PP_HIP(hipMemcpy(r.keep.p, keep, Q * sizeof(int), hipMemcpyHostToDevice));
        p.keep = r.keep.p;
    }
    p.fxy = s.fxy.p;  // the whole batch's arrays, not a sub-batch's view
    p.fbound = s.fbound.p;
    p.R = ctx->scene.max_steer;
    PP_HIP(launch_prune_verdicts(st, p));
    PP_HIP(launch_reval_jump(st, p.rv, passes));
    // (the error word stays 0: reval_write_kernel always commits)
    PP_HIP(launch_reval_compact(st, p.rv, p.rv.v[passes & 1]));
    if (n_nodes) PP_HIP(hipMemcpyAsync(n_nodes, f.n.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    if ((rc = reval_finish(ctx, p.rv, &kept, new_index))) return rc;  // the one synchronise
    if (n_dropped) *n_dropped = total - kept;
    return PP_OK;
}

}  // extern "C"

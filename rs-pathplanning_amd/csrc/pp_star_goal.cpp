// pp_star_goal.cpp — the RRT* batch's goal connection: the cheapest feasible goal edge of every
// query (pp_star_plan), the un-pruned totals of one query (pp_star_goal_costs) and the path along
// the rewired tree (pp_star_path; every query's at once, on the device: pp_star_paths).  DESIGN.md
// §3.7 "Goal connection".
#include "pp_ctx.h"

using namespace ppamd;

namespace {

// a goal pose: finite, its position within PP_COORD_MAX
bool finite3(const double* g) {
    return std::fabs(g[0]) <= PP_COORD_MAX && std::fabs(g[1]) <= PP_COORD_MAX && std::isfinite(g[2]);
}

// The goal rounds of the queries [q0, q1) on the context's stream: goals = 3 doubles per served
// query.  One read of the tree sizes gives the round count, the rounds are enqueued back to back,
// one synchronisation returns the results.  total (device, or null): the served query's totals.
int star_goal_run(pp_ctx* ctx, const double* goals, int q0, int q1, int prune, double* total,
                  int32_t* best_node, double* cost, int64_t* n_checked, int64_t* n_steered) {
    StarBatch& s = ctx->star;
    const int Q = s.f.Q, nq = q1 - q0;
    hipStream_t st = ctx->stream;
    PP_HIP(s.goal_d.reserve(3 * (size_t)Q));
    PP_HIP(s.gbest.reserve(Q));
    for (auto* b : {&s.gslot, &s.gnode}) PP_HIP(b->reserve(Q));
    PP_HIP(s.gmask.reserve(Q));
    PP_HIP(s.gsteer.reserve(1));
    std::vector<int> hn(nq);
    PP_HIP(hipMemcpyAsync(hn.data(), s.f.n.p + q0, nq * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(s.goal_d.p + 3 * (size_t)q0, goals, 3 * (size_t)nq * sizeof(double),
                          hipMemcpyHostToDevice, st));
    PP_HIP(hipStreamSynchronize(st));
    int max_n = 0;
    int64_t pairs = 0;
    for (int n : hn) {
        max_n = std::max(max_n, n);
        pairs += n;
    }
    StarGoalArgs g;
    g.a = star_args(ctx);
    g.q0 = q0;
    g.q1 = q1;
    g.goals = s.goal_d.p;
    g.gslot = s.gslot.p;
    g.gmask = s.gmask.p;
    g.best = s.gbest.p;
    g.best_node = s.gnode.p;
    g.steered = s.gsteer.p;
    g.prune = prune;
    g.total = total;
    PP_HIP(hipMemsetAsync(s.err.p, 0, sizeof(int), st));  // per call, not sticky
    PP_HIP(launch_star_goal(st, g, (max_n + kStarKMax - 1) / kStarKMax));
    std::vector<int> hnode(nq);
    std::vector<double> hbest(nq);
    long long steered = 0;
    int err = 0;
    PP_HIP(hipMemcpyAsync(hnode.data(), s.gnode.p + q0, nq * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(hbest.data(), s.gbest.p + q0, nq * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(&steered, s.gsteer.p, sizeof steered, hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(&err, s.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    if (err) return set_err(PP_ERR_STEER_OVERFLOW, "generate_local_course would index past n_point");
    for (int i = 0; i < nq; ++i) {
        if (best_node) best_node[i] = hnode[i];
        if (cost) cost[i] = hbest[i];
    }
    if (n_checked) *n_checked = pairs;
    if (n_steered) *n_steered = steered;
    return PP_OK;
}

int star_plan(pp_ctx* ctx, const double* goals, int prune, int32_t* best_node, double* cost,
              int64_t* n_checked, int64_t* n_steered) {
    int r = star_ready(ctx);
    if (r) return r;
    if (!goals) return set_err(PP_ERR_INVALID_ARGUMENT, "null goals");
    const int Q = ctx->star.f.Q;
    for (int q = 0; q < Q; ++q)
        if (!finite3(goals + 3 * (size_t)q)) return set_err(PP_ERR_INVALID_ARGUMENT, "non-finite goal");
    return star_goal_run(ctx, goals, 0, Q, prune, nullptr, best_node, cost, n_checked, n_steered);
}

}  // namespace

extern "C" {

int pp_star_plan(pp_ctx* ctx, const double* goals, int32_t* best_node, double* cost,
                 int64_t* n_checked) {
    return star_plan(ctx, goals, 1, best_node, cost, n_checked, nullptr);
}

// pp_star_plan with the pruning switch and the count of steered tasks: measurement only
// (scripts/bench_star_plan.py), not declared in the header and not part of the ABI
int ppamd_star_plan_debug(pp_ctx* ctx, const double* goals, int prune, int32_t* best_node,
                          double* cost, int64_t* n_checked, int64_t* n_steered) {
    return star_plan(ctx, goals, prune ? 1 : 0, best_node, cost, n_checked, n_steered);
}

int pp_star_goal_costs(pp_ctx* ctx, int query, const double goal[3], double* total, int64_t cap,
                       int64_t* n) {
    int r = star_ready(ctx);
    if (r) return r;
    StarBatch& s = ctx->star;
    if (query < 0 || query >= s.f.Q) return set_err(PP_ERR_INVALID_ARGUMENT, "query out of range");
    if (!goal || !finite3(goal)) return set_err(PP_ERR_INVALID_ARGUMENT, "null or non-finite goal");
    int nn = 0;
    PP_HIP(hipMemcpy(&nn, s.f.n.p + query, sizeof(int), hipMemcpyDeviceToHost));
    if (n) *n = nn;
    if (!total) return PP_OK;  // the size only
    if (cap < nn) return set_err(PP_ERR_CAPACITY, "buffer smaller than the tree");
    PP_HIP(s.gtotal.reserve((size_t)s.f.cap));
    if ((r = star_goal_run(ctx, goal, query, query + 1, 0, s.gtotal.p, nullptr, nullptr, nullptr,
                           nullptr)))
        return r;
    PP_HIP(hipMemcpy(total, s.gtotal.p, nn * sizeof(double), hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_star_path(pp_ctx* ctx, int query, const double goal[3], int32_t node, double* x, double* y,
                 int64_t cap, int64_t* n, double* length) {
    int r = star_ready(ctx);
    if (r) return r;
    StarBatch& s = ctx->star;
    if (query < 0 || query >= s.f.Q) return set_err(PP_ERR_INVALID_ARGUMENT, "query out of range");
    if (!goal || !finite3(goal)) return set_err(PP_ERR_INVALID_ARGUMENT, "null or non-finite goal");
    if (cap < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "cap < 0");
    // the query's tree, read once
    int64_t nt64 = 0;
    if ((r = s.f.export_tree(ctx, query, nullptr, nullptr, nullptr, nullptr, (int64_t)s.f.cap, &nt64)))
        return r;
    const size_t nt = (size_t)nt64;
    if (node < 0 || (size_t)node >= nt) return set_err(PP_ERR_INVALID_ARGUMENT, "node out of range");
    std::vector<double> hx(nt), hy(nt), hyaw(nt);
    std::vector<int32_t> hp(nt);
    if ((r = s.f.export_tree(ctx, query, hx.data(), hy.data(), hyaw.data(), hp.data(), nt64, &nt64)))
        return r;
    // a rewired node keeps its pose, so its stored yaw is not compute_yaw toward its current
    // parent: every edge is steered from the child's stored pose to the parent's stored pose
    std::vector<int> chain;  // node -> ... -> root
    for (int v = node; v >= 0; v = hp[(size_t)v]) {
        if (chain.size() > nt) return set_err(PP_ERR_STATE, "parent cycle in the tree");
        chain.push_back(v);
    }
    const double R = ctx->scene.max_steer, step = s.f.step;
    const int ne = (int)chain.size();  // the goal edge, then the chain's edges
    std::vector<pp_dubins_config> conf((size_t)ne);
    int pcap = 16;
    for (int e = 0; e < ne; ++e) {
        const size_t p = (size_t)chain[(size_t)e];
        double cx = goal[0], cy = goal[1], cyaw = goal[2];
        if (e > 0) {
            const size_t c = (size_t)chain[(size_t)e - 1];
            cx = hx[c];
            cy = hy[c];
            cyaw = hyaw[c];
        }
        conf[(size_t)e] = pp_dubins_config{cx, cy, cyaw, hx[p], hy[p], hyaw[p], R, step};
        // (the capacity bound of pp_rrt_line_to_origin's edges)
        const double d = std::hypot(hx[p] - cx, hy[p] - cy);
        pcap = std::max(pcap, (int)((6.0 * 3.14159265358979323846 + d / R + 4.0) / step) + 16);
    }
    std::vector<double> px((size_t)ne * pcap), py((size_t)ne * pcap), pyaw((size_t)ne * pcap);
    std::vector<double> ecost((size_t)ne);
    std::vector<int32_t> np((size_t)ne), word((size_t)ne);
    if ((r = pp_dubins_path_planning_batch(ctx, conf.data(), ne, pcap, px.data(), py.data(),
                                           pyaw.data(), np.data(), word.data(), ecost.data())))
        return r;
    // the goal edge must be feasible: Some, and verify of its points followed by the node's point
    if (word[0] < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "the node's goal edge is infeasible (no Dubins word)");
    {
        std::vector<double> lx(px.begin(), px.begin() + np[0]), ly(py.begin(), py.begin() + np[0]);
        lx.push_back(hx[(size_t)node]);
        ly.push_back(hy[(size_t)node]);
        const int64_t off[2] = {0, (int64_t)lx.size()};
        uint8_t ok = 0;
        if ((r = pp_space_verify_batch(ctx, lx.data(), ly.data(), off, 1, &ok))) return r;
        if (!ok) return set_err(PP_ERR_INVALID_ARGUMENT, "the node's goal edge is infeasible (verify)");
    }
    for (int e = 1; e < ne; ++e)
        if (word[(size_t)e] < 0)
            return set_err(PP_ERR_REFERENCE_PANIC, "a tree edge of the chain has no Dubins word");
    // E(goal -> node) ++ E(node -> parent) ++ ... ++ [root], returned reversed (root first)
    int64_t w = 1;
    for (int e = 0; e < ne; ++e) w += np[(size_t)e];
    if (n) *n = w;
    const bool fill = cap > 0 && x && y;
    if (fill && w > cap) return set_err(PP_ERR_CAPACITY, "line buffer smaller than the line");
    if (!fill && !length) return PP_OK;
    std::vector<double> lx, ly;
    lx.reserve((size_t)w);
    ly.reserve((size_t)w);
    lx.push_back(hx[0]);
    ly.push_back(hy[0]);
    for (int e = ne - 1; e >= 0; --e)
        for (int k = np[(size_t)e] - 1; k >= 0; --k) {
            lx.push_back(px[(size_t)e * pcap + k]);
            ly.push_back(py[(size_t)e * pcap + k]);
        }
    if (length) {  // euclidean_length of the returned line
        double len = 0.0;
        for (size_t i = 0; i + 1 < lx.size(); ++i) len += std::hypot(lx[i + 1] - lx[i], ly[i + 1] - ly[i]);
        *length = len;
    }
    if (fill) {
        std::memcpy(x, lx.data(), (size_t)w * sizeof(double));
        std::memcpy(y, ly.data(), (size_t)w * sizeof(double));
    }
    return PP_OK;
}

int pp_star_paths(pp_ctx* ctx, const double* goals, const int32_t* nodes, int64_t* off, double* x,
                  double* y, int64_t cap, int64_t* n_total, double* length, uint8_t* ok) {
    int r = star_ready(ctx);
    if (r) return r;
    StarBatch& s = ctx->star;
    if (!goals || !nodes || !off || !n_total)
        return set_err(PP_ERR_INVALID_ARGUMENT, "null goals, nodes, off or n_total");
    const int Q = s.f.Q;
    for (int q = 0; q < Q; ++q)
        if (!finite3(goals + 3 * (size_t)q)) return set_err(PP_ERR_INVALID_ARGUMENT, "non-finite goal");
    hipStream_t st = ctx->stream;
    PathExport& pe = ctx->paths;
    int k = 0;
    if ((r = paths_items(ctx, s.f, nodes, &k))) return r;
    *n_total = 0;
    if (length) std::fill(length, length + Q, 0.0);
    if (k == 0) {
        std::fill(off, off + Q + 1, (int64_t)0);
        if (ok) std::fill(ok, ok + Q, (uint8_t)0);
        return PP_OK;
    }
    // the line items (cf_line_kernel's layout): item b of the call, no optimize chain
    std::vector<int> items(1 + (size_t)k * kCfItem, 0);
    items[0] = k;
    for (int b = 0; b < k; ++b) items[1 + (size_t)b * kCfItem] = b;
    PP_HIP(pe.items.reserve(items.size()));
    PP_HIP(s.goal_d.reserve(3 * (size_t)Q));
    PP_HIP(hipMemcpyAsync(pe.items.p, items.data(), items.size() * sizeof(int), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(s.goal_d.p, goals, 3 * (size_t)Q * sizeof(double), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemsetAsync(pe.cnt.p, 0, (size_t)k * sizeof(int), st));
    PP_HIP(hipMemsetAsync(pe.ok.p, 0, (size_t)k * sizeof(int), st));
    PP_HIP(ctx->cf.err.reserve(2));
    PP_HIP(hipMemsetAsync(ctx->cf.err.p, 0, 2 * sizeof(int), st));
    const SceneDev sd = ctx->scene.dev(s.f.step, false);
    PathsArgs a;
    a.tr = s.f.tree_dev();
    a.row_cap = s.f.cap;
    a.qidx = pe.qidx.p;
    a.nodes = pe.nodes.p;
    a.goals = s.goal_d.p;
    a.cnt = pe.cnt.p;
    a.okf = pe.ok.p;
    CfLines lines;
    // the count pass: every item's points (and whether its goal edge has a word)
    if ((r = paths_line_buffers(ctx, k, lines))) return r;
    PP_HIP(launch_paths(st, sd, a, lines, ctx->cf.err.p, pe.items.p, k, true, false));
    int err = 0;
    PP_HIP(hipMemcpyAsync(&err, ctx->cf.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    bool go = false;
    r = paths_sizes(ctx, Q, off, x, y, cap, n_total, ok, &go);  // (synchronises: err is read)
    if (err & 2) return set_err(PP_ERR_REFERENCE_PANIC, "a tree edge of a chain has no Dubins word");
    if (err & 4) return set_err(PP_ERR_STEER_OVERFLOW, "generate_local_course would index past n_point");
    if (err & 1) return set_err(PP_ERR_CAPACITY, "tree deeper than the path capacity");
    if (err & 8) return set_err(PP_ERR_CAPACITY, "a line longer than the point capacity");
    if (r || !go) return r;
    // the write pass (the spill count zeroed again), with the rows' lengths
    if ((r = paths_line_buffers(ctx, k, lines))) return r;
    std::vector<double> hl(length ? (size_t)k : 0);
    if (length) {
        a.len = pe.len.p;
        PP_HIP(hipMemsetAsync(pe.len.p, 0, (size_t)k * sizeof(double), st));
    }
    if ((r = paths_write(ctx, sd, a, lines, pe.items.p, k, true, x, y, *n_total,
                         length ? hl.data() : nullptr)))
        return r;
    for (int q = 0, b = 0; length && q < Q; ++q)
        if (nodes[q] >= 0) length[q] = hl[(size_t)b++];  // (items are the chosen nodes in query order)
    return PP_OK;
}

}  // extern "C"

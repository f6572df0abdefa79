// pp_shortcut.cpp — shorten the RRT* batch's paths by Dubins shortcuts along the chain:
// pp_star_shortcut (every query's shortened chain in one call), pp_star_shortcut_edges (the
// un-culled band of one query, the test hook) and pp_star_shortcut_commit (the shortcuts written
// back into the trees as rewires).  The kernels are pp_k_shortcut.hip; the items and
// the sizes-only protocol are the packed exports' (pp_finish.cpp, pp_star_goal.cpp).  DESIGN.md
// §3.7 "Shortcuts along the chain".
#include <limits>

#include "pp_ctx.h"

using namespace ppamd;

namespace {

bool finite3(const double* g) {
    return std::fabs(g[0]) <= PP_COORD_MAX && std::fabs(g[1]) <= PP_COORD_MAX && std::isfinite(g[2]);
}

// one call's items and sizes on the host
struct ScRun {
    int k = 0;                       // items (the queries with a node)
    std::vector<int> slot;           // [Q] the query's item, -1 none
    std::vector<int> D;              // [k]
    std::vector<int64_t> pbase, boff;  // [k + 1]
    ShortcutArgs a;
    int rounds = 0;
};

// The items of nodes[0, Q), their chains and sizes (one read-back), the 2^26-pair check.  goals:
// 3 doubles per query of the batch.
int shortcut_sizes(pp_ctx* ctx, const double* goals, const int32_t* nodes, int span, ScRun& run) {
    StarBatch& s = ctx->star;
    Shortcut& sc = ctx->shortcut;
    const int Q = s.f.Q;
    hipStream_t st = ctx->stream;
    int r = paths_items(ctx, s.f, nodes, &run.k);
    if (r) return r;
    const int k = run.k;
    run.slot.assign((size_t)Q, -1);
    for (int q = 0, b = 0; q < Q; ++q)
        if (nodes[q] >= 0) run.slot[(size_t)q] = b++;  // (items are the chosen nodes in query order)
    if (k == 0) return PP_OK;
    const int stride = std::min(s.f.cap, kCfMaxDepth);
    const int T = Q * kStarKMax;
    PP_HIP(s.goal_d.reserve(3 * (size_t)Q));
    for (auto* b : {&sc.chain, &sc.next}) PP_HIP(b->reserve((size_t)k * stride));
    for (auto* b : {&sc.depth, &sc.plen}) PP_HIP(b->reserve(k));
    PP_HIP(sc.err.reserve(1));
    PP_HIP(sc.npair.reserve(k));
    for (auto* b : {&sc.pbase, &sc.boff}) PP_HIP(b->reserve((size_t)k + 1));
    PP_HIP(sc.tdst.reserve(T));
    PP_HIP(sc.cost.reserve(k));
    PP_HIP(hipMemcpyAsync(s.goal_d.p, goals, 3 * (size_t)Q * sizeof(double), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemsetAsync(sc.err.p, 0, sizeof(int), st));
    ShortcutArgs& a = run.a;
    a.a = star_args(ctx);
    a.k = k;
    a.span = span;
    a.qidx = ctx->paths.qidx.p;
    a.nodes = ctx->paths.nodes.p;
    a.goals = s.goal_d.p;
    a.stride = stride;
    a.chain = sc.chain.p;
    a.next = sc.next.p;
    a.depth = sc.depth.p;
    a.npair = sc.npair.p;
    a.tdst = sc.tdst.p;
    a.cost = sc.cost.p;
    a.plen = sc.plen.p;
    a.err = sc.err.p;
    PP_HIP(launch_shortcut_chain(st, a));
    run.D.resize((size_t)k);
    std::vector<int64_t> np((size_t)k);
    int err = 0;
    PP_HIP(hipMemcpyAsync(run.D.data(), sc.depth.p, (size_t)k * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(np.data(), sc.npair.p, (size_t)k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(&err, sc.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));  // the one read of the sizes
    if (err & 1) return set_err(PP_ERR_CAPACITY, "tree deeper than the path capacity");
    run.pbase.assign((size_t)k + 1, 0);
    run.boff.assign((size_t)k + 1, 0);
    for (int b = 0; b < k; ++b) {
        const int64_t D = run.D[(size_t)b];
        run.pbase[(size_t)b + 1] = run.pbase[(size_t)b] + np[(size_t)b];
        run.boff[(size_t)b + 1] = run.boff[(size_t)b] + D * std::min<int64_t>(span, D);
    }
    if (run.pbase[(size_t)k] > kShortcutMaxPairs)
        return set_err(PP_ERR_CAPACITY, "more than 2^26 (i, j) pairs in one call: shorten fewer "
                                        "queries at once (nodes = -1 skips one) or a smaller span");
    run.rounds = (int)((run.pbase[(size_t)k] + T - 1) / T);
    return PP_OK;
}

// the steer rounds over all pairs: the band.  ev (profiling): 4 events per round, or null
int shortcut_rounds(pp_ctx* ctx, ScRun& run, hipEvent_t* ev = nullptr) {
    Shortcut& sc = ctx->shortcut;
    hipStream_t st = ctx->stream;
    const int k = run.k;
    const int T = ctx->star.f.Q * kStarKMax;
    PP_HIP(sc.band.reserve((size_t)run.boff[(size_t)k]));
    PP_HIP(hipMemcpyAsync(sc.pbase.p, run.pbase.data(), ((size_t)k + 1) * sizeof(int64_t),
                          hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(sc.boff.p, run.boff.data(), ((size_t)k + 1) * sizeof(int64_t),
                          hipMemcpyHostToDevice, st));
    run.a.pbase = sc.pbase.p;
    run.a.boff = sc.boff.p;
    run.a.band = sc.band.p;
    const int64_t pairs = run.pbase[(size_t)k];
    int rd = 0;
    for (int64_t g0 = 0; g0 < pairs; g0 += T, ++rd)
        PP_HIP(launch_shortcut_round(st, run.a, g0, (int)std::min<int64_t>(T, pairs - g0),
                                     ev ? ev + 4 * rd : nullptr));
    return PP_OK;
}

int shortcut_error(int err) {
    if (err & 4) return set_err(PP_ERR_STEER_OVERFLOW, "generate_local_course would index past n_point");
    if (err & 16) return set_err(PP_ERR_STATE, "shortcut: a pair outside its item's band");
    return PP_OK;
}

// ms (profiling, may be null): [0] chain + sizes, [1 .. 4] the rounds' emit / prep / walk / settle,
// [5] the DP, [6] pack + copies; *rounds (may be null): the steer rounds
int star_shortcut(pp_ctx* ctx, const double* goals, const int32_t* nodes, int span, int64_t* off,
                  int32_t* chain, int64_t cap, int64_t* n_total, double* cost, uint8_t* ok,
                  int64_t* n_tested, double* ms, int64_t* rounds) {
    int r = star_ready(ctx);
    if (r) return r;
    if (span < 1 || span > kStarKMax) return set_err(PP_ERR_INVALID_ARGUMENT, "span outside [1, 63]");
    if (!goals || !nodes || !off || !n_total)
        return set_err(PP_ERR_INVALID_ARGUMENT, "null goals, nodes, off or n_total");
    StarBatch& s = ctx->star;
    Shortcut& sc = ctx->shortcut;
    const int Q = s.f.Q;
    for (int q = 0; q < Q; ++q)
        if (!finite3(goals + 3 * (size_t)q)) return set_err(PP_ERR_INVALID_ARGUMENT, "non-finite goal");
    hipStream_t st = ctx->stream;
    Events ev;  // (profiling) [0 .. 3] the stages' marks, then 4 per round
    if (ms) {
        PP_HIP(ev.reserve(4));
        PP_HIP(hipEventRecord(ev[0], st));
    }
    ScRun run;
    if ((r = shortcut_sizes(ctx, goals, nodes, span, run))) return r;
    const int k = run.k;
    const double inf = std::numeric_limits<double>::infinity();
    *n_total = 0;
    std::fill(off, off + Q + 1, (int64_t)0);
    if (cost) std::fill(cost, cost + Q, inf);
    if (ok) std::fill(ok, ok + Q, (uint8_t)0);
    if (n_tested) *n_tested = k ? run.pbase[(size_t)k] : 0;
    if (rounds) *rounds = run.rounds;
    if (k == 0) return PP_OK;
    hipEvent_t* rev = nullptr;  // the rounds' events
    if (ms) {
        PP_HIP(ev.reserve(4 + 4 * (size_t)run.rounds));
        rev = ev.data() + 4;
        PP_HIP(hipEventRecord(ev[1], st));
    }
    if ((r = shortcut_rounds(ctx, run, rev))) return r;
    PP_HIP(launch_shortcut_dp(st, run.a));
    if (ms) PP_HIP(hipEventRecord(ev[2], st));
    std::vector<int> plen((size_t)k);
    std::vector<double> hc((size_t)k);
    int err = 0;
    PP_HIP(hipMemcpyAsync(plen.data(), sc.plen.p, (size_t)k * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(hc.data(), sc.cost.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(&err, sc.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    if ((r = shortcut_error(err))) return r;
    // the rows' offsets on the host (as pp_star_paths sizes its rows after one read-back)
    int64_t total = 0;
    for (int q = 0; q < Q; ++q) {
        off[q] = total;
        const int b = run.slot[(size_t)q];
        if (b < 0 || plen[(size_t)b] <= 0) continue;
        total += plen[(size_t)b];
        if (cost) cost[q] = hc[(size_t)b];
        if (ok) ok[q] = 1;
    }
    off[Q] = total;
    *n_total = total;
    if (chain && cap > 0 && total > 0) {
        if (cap < total)
            return set_err(PP_ERR_CAPACITY, "chain smaller than the rows' total (n_total)");
        PP_HIP(sc.off.reserve((size_t)Q + 1));
        PP_HIP(sc.out.reserve((size_t)total));
        PP_HIP(hipMemcpyAsync(sc.off.p, off, ((size_t)Q + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        PP_HIP(launch_shortcut_pack(st, run.a, Q, ctx->paths.slot.p, sc.off.p, total, sc.out.p));
        PP_HIP(hipMemcpyAsync(chain, sc.out.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
    }
    if (ms) {
        PP_HIP(hipEventRecord(ev[3], st));
        PP_HIP(hipEventSynchronize(ev[3]));
        float f = 0.0f;
        for (int i = 0; i < 7; ++i) ms[i] = 0.0;
        PP_HIP(hipEventElapsedTime(&f, ev[0], ev[1]));
        ms[0] = f;
        // every round event's time since the one before it (the first round's: since ev[1])
        hipEvent_t from = ev[1];
        for (int i = 0; i < 4 * run.rounds; ++i) {
            PP_HIP(hipEventElapsedTime(&f, from, rev[i]));
            ms[1 + i % 4] += f;
            from = rev[i];
        }
        PP_HIP(hipEventElapsedTime(&f, from, ev[2]));
        ms[5] = f;
        PP_HIP(hipEventElapsedTime(&f, ev[2], ev[3]));
        ms[6] = f;
    }
    return PP_OK;
}

// pp_star_shortcut_commit.  ms (profiling, may be null): [0] chain + sizes, [1] the steer rounds,
// [2] the commit kernel (DP, writes, propagation), [3] the copies back
int star_shortcut_commit(pp_ctx* ctx, const double* goals, const int32_t* nodes, int span,
                         int32_t* node_out, double* cost_out, int32_t* n_rewired,
                         int64_t* n_tested, int64_t* n_changed, double* ms) {
    int r = star_ready(ctx);
    if (r) return r;
    if (span < 1 || span > kStarKMax) return set_err(PP_ERR_INVALID_ARGUMENT, "span outside [1, 63]");
    if (!goals || !nodes) return set_err(PP_ERR_INVALID_ARGUMENT, "null goals or nodes");
    StarBatch& s = ctx->star;
    Shortcut& sc = ctx->shortcut;
    const int Q = s.f.Q;
    for (int q = 0; q < Q; ++q)
        if (!finite3(goals + 3 * (size_t)q)) return set_err(PP_ERR_INVALID_ARGUMENT, "non-finite goal");
    hipStream_t st = ctx->stream;
    Events ev;  // (profiling) the marks between the stages
    if (ms) {
        PP_HIP(ev.reserve(5));
        PP_HIP(hipEventRecord(ev[0], st));
    }
    ScRun run;
    if ((r = shortcut_sizes(ctx, goals, nodes, span, run))) return r;
    const int k = run.k;
    if (node_out) std::fill(node_out, node_out + Q, (int32_t)-1);
    if (cost_out) std::fill(cost_out, cost_out + Q, std::numeric_limits<double>::infinity());
    if (n_rewired) std::fill(n_rewired, n_rewired + Q, (int32_t)0);
    if (n_tested) *n_tested = k ? run.pbase[(size_t)k] : 0;
    if (n_changed) *n_changed = 0;
    if (ms) std::fill(ms, ms + 4, 0.0);
    if (k == 0) return PP_OK;
    if (ms) PP_HIP(hipEventRecord(ev[1], st));
    if ((r = shortcut_rounds(ctx, run))) return r;
    if (ms) PP_HIP(hipEventRecord(ev[2], st));
    PP_HIP(sc.res.reserve(3 * (size_t)k));
    run.a.res = sc.res.p;
    // (the kernel reads the rounds' error word itself and writes nothing when it is set: no host
    // round trip between the rounds and the tree's stores)
    PP_HIP(launch_shortcut_commit(st, run.a));
    if (ms) PP_HIP(hipEventRecord(ev[3], st));
    std::vector<int> res(3 * (size_t)k);
    std::vector<double> hc((size_t)k);
    int err = 0;
    PP_HIP(hipMemcpyAsync(res.data(), sc.res.p, res.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(hc.data(), sc.cost.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(&err, sc.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    if (ms) PP_HIP(hipEventRecord(ev[4], st));
    PP_HIP(hipStreamSynchronize(st));
    if ((r = shortcut_error(err))) return r;
    int64_t changed = 0;
    for (int q = 0; q < Q; ++q) {
        const int b = run.slot[(size_t)q];
        if (b < 0) continue;
        if (node_out) node_out[q] = res[3 * (size_t)b];
        if (cost_out) cost_out[q] = hc[(size_t)b];
        if (n_rewired) n_rewired[q] = res[3 * (size_t)b + 1];
        changed += res[3 * (size_t)b + 2];
    }
    if (n_changed) *n_changed = changed;
    if (ms) {
        float f = 0.0f;
        for (int i = 0; i < 4; ++i) {
            PP_HIP(hipEventElapsedTime(&f, ev[i], ev[i + 1]));
            ms[i] = f;
        }
    }
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_star_shortcut_commit(pp_ctx* ctx, const double* goals, const int32_t* nodes, int span,
                            int32_t* node_out, double* cost_out, int32_t* n_rewired,
                            int64_t* n_tested, int64_t* n_changed) {
    return star_shortcut_commit(ctx, goals, nodes, span, node_out, cost_out, n_rewired, n_tested,
                                n_changed, nullptr);
}

// pp_star_shortcut_commit with its stages timed by events (ms: 4 values — chain + sizes, the steer
// rounds, the commit kernel, the copies back): measurement only
// (scripts/bench_star_shortcut_commit.py), not declared in the header and not part of the ABI
int ppamd_star_shortcut_commit_debug(pp_ctx* ctx, const double* goals, const int32_t* nodes,
                                     int span, int32_t* node_out, double* cost_out,
                                     int32_t* n_rewired, int64_t* n_tested, int64_t* n_changed,
                                     double* ms) {
    return star_shortcut_commit(ctx, goals, nodes, span, node_out, cost_out, n_rewired, n_tested,
                                n_changed, ms);
}


int pp_star_shortcut(pp_ctx* ctx, const double* goals, const int32_t* nodes, int span,
                     int64_t* off, int32_t* chain, int64_t cap, int64_t* n_total, double* cost,
                     uint8_t* ok, int64_t* n_tested) {
    return star_shortcut(ctx, goals, nodes, span, off, chain, cap, n_total, cost, ok, n_tested,
                         nullptr, nullptr);
}

// pp_star_shortcut with its stages timed by events (ms: 7 values — chain + sizes, the rounds'
// emit / prep / walk / settle, the DP, pack + copies) and the steer rounds: measurement only
// (scripts/bench_star_shortcut.py), not declared in the header and not part of the ABI
int ppamd_star_shortcut_debug(pp_ctx* ctx, const double* goals, const int32_t* nodes, int span,
                              int64_t* off, int32_t* chain, int64_t cap, int64_t* n_total,
                              double* cost, uint8_t* ok, int64_t* n_tested, double* ms,
                              int64_t* rounds) {
    return star_shortcut(ctx, goals, nodes, span, off, chain, cap, n_total, cost, ok, n_tested, ms,
                         rounds);
}

int pp_star_shortcut_edges(pp_ctx* ctx, int query, const double goal[3], int32_t node, int span,
                           double* w, int32_t* cnode, int64_t cap, int64_t* depth) {
    int r = star_ready(ctx);
    if (r) return r;
    StarBatch& s = ctx->star;
    Shortcut& sc = ctx->shortcut;
    const int Q = s.f.Q;
    if (query < 0 || query >= Q) return set_err(PP_ERR_INVALID_ARGUMENT, "query out of range");
    if (span < 1 || span > kStarKMax) return set_err(PP_ERR_INVALID_ARGUMENT, "span outside [1, 63]");
    if (!goal || !finite3(goal)) return set_err(PP_ERR_INVALID_ARGUMENT, "null or non-finite goal");
    if (!depth) return set_err(PP_ERR_INVALID_ARGUMENT, "null depth");
    if (node < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "node index outside its query's tree");
    // the one query as a call of the batch: every other query skipped
    std::vector<double> goals(3 * (size_t)Q, 0.0);
    std::vector<int32_t> nodes((size_t)Q, -1);
    std::copy(goal, goal + 3, goals.begin() + 3 * (size_t)query);
    nodes[(size_t)query] = node;
    ScRun run;
    if ((r = shortcut_sizes(ctx, goals.data(), nodes.data(), span, run))) return r;
    const int D = run.D[0];
    *depth = D;
    if (!w) return PP_OK;  // the size only
    if (cap < D) return set_err(PP_ERR_CAPACITY, "buffers smaller than the chain");
    if ((r = shortcut_rounds(ctx, run))) return r;
    hipStream_t st = ctx->stream;
    const int sp = std::min(span, D);
    std::vector<double> band((size_t)D * sp);
    int err = 0;
    PP_HIP(hipMemcpyAsync(band.data(), sc.band.p, band.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (cnode)
        PP_HIP(hipMemcpyAsync(cnode, sc.chain.p, (size_t)D * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(&err, sc.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    if ((r = shortcut_error(err))) return r;
    // the device's rows hold min(span, D) entries, and those with j > D were never written
    const double inf = std::numeric_limits<double>::infinity();
    for (int i = 0; i < D; ++i)
        for (int l = 0; l < span; ++l)
            w[(size_t)i * span + l] = (l < sp && i + 1 + l <= D) ? band[(size_t)i * sp + l] : inf;
    return PP_OK;
}

}  // extern "C"

// pp_forest_io.cpp — the packed forest export / import: the complete state of a
// set of query slots copied out of a batch in one call and written into a set of slots, for the
// RRT* batch (pp_star_forest_*) and the extend batch (pp_batch_forest_*).  One implementation
// over the Forest both batches share; what differs is which arrays exist.  The kernels are
// pp_k_forest_io.hip's.
#include "pp_ctx.h"

#include <cstddef>
#include <limits>

using namespace ppamd;

namespace {

// the batch a call works on: its forest, and the RRT* arrays (s) or the extend batch's (b)
struct Target {
    Forest* f = nullptr;
    StarBatch* s = nullptr;
    Batch* b = nullptr;
};

// the caller's struct as this library knows it: fields past the caller's `size` read as NULL
int load_state(const pp_forest_state* in, pp_forest_state* out) {
    if (!in) return set_err(PP_ERR_INVALID_ARGUMENT, "null forest state");
    if (in->size < offsetof(pp_forest_state, off) + sizeof(in->off))
        return set_err(PP_ERR_INVALID_ARGUMENT, "pp_forest_state.size does not reach `off`: set it to sizeof(pp_forest_state)");
    std::memset(out, 0, sizeof *out);
    std::memcpy(out, in, (size_t)std::min<uint64_t>(in->size, sizeof *out));
    return PP_OK;
}

// queries[0 .. m): distinct slots of a Q-slot forest (NULL: 0 .. m - 1); *bad: the first offender
int load_slots(const int32_t* queries, int m, int Q, std::vector<int>* slots, int32_t* bad) {
    if (m < 1 || m > Q) return set_err(PP_ERR_INVALID_ARGUMENT, "m must lie in [1, the batch's queries]");
    slots->resize((size_t)m);
    std::vector<uint8_t> seen((size_t)Q, 0);
    for (int i = 0; i < m; ++i) {
        const int q = queries ? queries[i] : i;
        if (q < 0 || q >= Q || seen[(size_t)q]) {
            if (bad) *bad = q;
            return set_err(PP_ERR_INVALID_ARGUMENT, q < 0 || q >= Q ? "a query slot is out of range"
                                                                    : "a query slot is named twice");
        }
        seen[(size_t)q] = 1;
        (*slots)[(size_t)i] = q;
    }
    return PP_OK;
}

// the kernels' view of the target's forest and of the per-slot staging for m served slots
int fio_args(pp_ctx* c, const Target& t, const std::vector<int>& slots, ForestIoArgs* out) {
    ForestIo& io = c->fio;
    const size_t m = slots.size();
    PP_HIP(io.slots.reserve(m));
    PP_HIP(io.off.reserve(m + 1));
    for (auto* b : {&io.sit, &io.sevals, &io.srew, &io.sskipped}) PP_HIP(b->reserve(m));
    PP_HIP(io.sseed.reserve(m));
    PP_HIP(io.sfxy.reserve(2 * m));
    PP_HIP(io.sfbound.reserve(m));
    PP_HIP(io.sblocked.reserve(m));
    PP_HIP(io.verdict.reserve(m));
    PP_HIP(hipMemcpy(io.slots.p, slots.data(), m * sizeof(int), hipMemcpyHostToDevice));
    const Forest& f = *t.f;
    ForestIoArgs a;
    a.tr = f.tree_dev();
    a.cap = (size_t)f.cap;
    a.m = (int)m;
    a.slots = io.slots.p;
    a.off = io.off.p;
    a.n = f.n.p;
    a.it = f.it.p;
    a.evals = f.evals.p;
    a.seed = f.seed.p;
    a.starts = f.d_starts.p;
    if (t.s) {
        a.cost = t.s->cost.p;
        a.elen = t.s->elen.p;
        a.mark = t.s->mark.p;
        a.rew = t.s->rew.p;
        a.fxy = t.s->fxy.p;
        a.fbound = t.s->fbound.p;
        a.skipped = t.s->skipped.p;
        a.stamp = t.s->stamp.p;
    } else {
        a.itprev = t.b->itprev.p;
        a.ordered = 1;
    }
    a.sit = io.sit.p;
    a.sevals = io.sevals.p;
    a.sseed = io.sseed.p;
    a.srew = io.srew.p;
    a.sfxy = io.sfxy.p;
    a.sfbound = io.sfbound.p;
    a.sskipped = io.sskipped.p;
    a.verdict = io.verdict.p;
    *out = a;
    return PP_OK;
}

int forest_export(pp_ctx* c, const Target& t, const int32_t* queries, int m,
                  pp_forest_state* state, int64_t cap, int64_t* n_total) {
    pp_forest_state st;
    int rc = load_state(state, &st);
    if (rc) return rc;
    if (!n_total) return set_err(PP_ERR_INVALID_ARGUMENT, "null n_total");
    std::vector<int> slots;
    if ((rc = load_slots(queries, m, t.f->Q, &slots, nullptr))) return rc;
    ForestIoArgs a;
    if ((rc = fio_args(c, t, slots, &a))) return rc;
    ForestIo& io = c->fio;
    hipStream_t s = c->stream;
    const size_t z = (size_t)m;
    PP_HIP(launch_forest_sizes(s, a));
    int64_t total = 0;
    PP_HIP(hipMemcpyAsync(&total, io.off.p + z, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    auto out = [&](void* dst, const void* src, size_t bytes) {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    };
    PP_HIP(out(st.off, io.off.p, (z + 1) * sizeof(int64_t)));
    PP_HIP(out(st.iterations, io.sit.p, z * sizeof(int64_t)));
    PP_HIP(out(st.seeds, io.sseed.p, z * sizeof(uint64_t)));
    PP_HIP(out(st.node_evals, io.sevals.p, z * sizeof(int64_t)));
    if (t.s) {
        PP_HIP(out(st.rewires, io.srew.p, z * sizeof(int64_t)));
        PP_HIP(out(st.focus_xy, io.sfxy.p, 2 * z * sizeof(double)));
        PP_HIP(out(st.focus_bound, io.sfbound.p, z * sizeof(double)));
        PP_HIP(out(st.skipped, io.sskipped.p, z * sizeof(int64_t)));
    }
    PP_HIP(hipStreamSynchronize(s));  // the sizes: the one synchronisation before the rows
    if (!t.s && st.goals)
        for (int i = 0; i < m; ++i)
            std::memcpy(st.goals + 3 * (size_t)i, t.b->goal.data() + 3 * (size_t)slots[(size_t)i],
                        3 * sizeof(double));
    *n_total = total;
    if (!t.s) st.cost = st.edge_cost = nullptr;  // (the extend batch has neither)
    const bool rows = st.x || st.y || st.yaw || st.parent || st.cost || st.edge_cost;
    if (!rows || cap <= 0) return PP_OK;
    if (cap < total) return set_err(PP_ERR_CAPACITY, "the row arrays are smaller than the exported trees");
    const size_t r = (size_t)total;
    if (st.x) PP_HIP(io.sx.reserve(r));
    if (st.y) PP_HIP(io.sy.reserve(r));
    if (st.yaw) PP_HIP(io.syaw.reserve(r));
    if (st.parent) PP_HIP(io.spar.reserve(r));
    if (st.cost) PP_HIP(io.scost.reserve(r));
    if (st.edge_cost) PP_HIP(io.selen.reserve(r));
    a.total = total;
    a.sx = st.x ? io.sx.p : nullptr;
    a.sy = st.y ? io.sy.p : nullptr;
    a.syaw = st.yaw ? io.syaw.p : nullptr;
    a.spar = st.parent ? io.spar.p : nullptr;
    a.scost = st.cost ? io.scost.p : nullptr;
    a.selen = st.edge_cost ? io.selen.p : nullptr;
    PP_HIP(launch_forest_gather(s, a));
    PP_HIP(out(st.x, io.sx.p, r * sizeof(double)));
    PP_HIP(out(st.y, io.sy.p, r * sizeof(double)));
    PP_HIP(out(st.yaw, io.syaw.p, r * sizeof(double)));
    PP_HIP(out(st.parent, io.spar.p, r * sizeof(int)));
    PP_HIP(out(st.cost, io.scost.p, r * sizeof(double)));
    PP_HIP(out(st.edge_cost, io.selen.p, r * sizeof(double)));
    PP_HIP(hipStreamSynchronize(s));
    return PP_OK;
}

const char* verdict_text(int v) {
    switch (v) {
        case kFioRoot: return "a tree's row 0 must have parent -1";
        case kFioParent: return "a parent must be another node of its tree";
        case kFioOrder: return "a parent must precede its child (pp_rrt_tree_import's rule)";
        case kFioUnreached: return "a chain does not end in its tree's row 0 (a cycle or an island)";
        case kFioCost: return "cost differs from cost[parent] + edge_cost rebuilt from the root";
    }
    return "invalid tree";
}

int forest_import(pp_ctx* c, const Target& t, const int32_t* queries, int m,
                  const pp_forest_state* state, int32_t* bad_query) {
    pp_forest_state st;
    int rc = load_state(state, &st);
    if (rc) return rc;
    Forest& f = *t.f;
    std::vector<int> slots;
    if ((rc = load_slots(queries, m, f.Q, &slots, bad_query))) return rc;
    const bool star = t.s != nullptr;
    if (!st.off || !st.x || !st.y || !st.yaw || !st.parent || !st.iterations || !st.seeds ||
        !st.node_evals ||
        (star ? !st.edge_cost || !st.rewires || !st.focus_xy || !st.focus_bound || !st.skipped
              : !st.goals))
        return set_err(PP_ERR_INVALID_ARGUMENT, "forest import: a required array of the state is NULL");
    // ---- the host's checks, slot by slot: the first offender is named
    const size_t z = (size_t)m;
    auto fail = [&](int i, int code, const char* msg) {
        if (bad_query) *bad_query = slots[(size_t)i];
        return set_err(code, std::string("forest import: ") + msg);
    };
    if (st.off[0] != 0) return fail(0, PP_ERR_INVALID_ARGUMENT, "off[0] must be 0");
    const bool polygons = c->scene.polygons();
    std::vector<uint8_t> blk(z, 0);
    bool any_blk = false;
    for (int i = 0; i < m; ++i) {
        const int64_t g0 = st.off[i], n = st.off[i + 1] - g0, it = st.iterations[i];
        if (n < 1) return fail(i, PP_ERR_INVALID_ARGUMENT, "a tree needs its root: off must increase");
        if (it < 0 || it > f.max_iter)
            return fail(i, PP_ERR_INVALID_ARGUMENT, "iterations outside [0, max_iter]");
        if (n > it + 1)
            return fail(i, PP_ERR_CAPACITY, "a tree of more than iterations + 1 nodes: the slot could not hold the inserts still to come");
        if (st.node_evals[i] < 0) return fail(i, PP_ERR_INVALID_ARGUMENT, "node_evals < 0");
        if (check_coords(st.x + g0, n, 1, "forest import: x") || check_coords(st.y + g0, n, 1, "forest import: y")) {
            if (bad_query) *bad_query = slots[(size_t)i];
            return PP_ERR_INVALID_ARGUMENT;
        }
        for (int64_t k = g0; k < g0 + n; ++k)
            if (!std::isfinite(st.yaw[k])) return fail(i, PP_ERR_INVALID_ARGUMENT, "a yaw is not finite");
        if (star) {
            if (st.rewires[i] < 0) return fail(i, PP_ERR_INVALID_ARGUMENT, "rewires < 0");
            if (st.skipped[i] < 0) return fail(i, PP_ERR_INVALID_ARGUMENT, "skipped < 0");
            if (!(st.focus_bound[i] > 0.0))  // (NaN fails the comparison too; +inf: no focus)
                return fail(i, PP_ERR_INVALID_ARGUMENT, "a focus bound must be > 0 or +inf");
            if (check_coords(st.focus_xy + 2 * (size_t)i, 2, 1, "forest import: focus points")) {
                if (bad_query) *bad_query = slots[(size_t)i];
                return PP_ERR_INVALID_ARGUMENT;
            }
            for (int64_t k = g0; k < g0 + n; ++k)
                if (!(st.edge_cost[k] >= 0.0) || !std::isfinite(st.edge_cost[k]))
                    return fail(i, PP_ERR_INVALID_ARGUMENT, "an edge cost must be finite and >= 0");
        } else {
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(st.goals[3 * (size_t)i + k]))
                    return fail(i, PP_ERR_INVALID_ARGUMENT, "a goal is not finite");
        }
        if (polygons && !c->scene.point_ok(st.x[g0], st.y[g0])) {
            if (n > 1)
                return fail(i, PP_ERR_INVALID_ARGUMENT, "a tree of more than one node on a root that fails verify (polygon mode)");
            blk[(size_t)i] = 1;
            any_blk = true;
        }
    }
    const int64_t total = st.off[m];
    // ---- stage everything, validate on the device
    ForestIoArgs a;
    if ((rc = fio_args(c, t, slots, &a))) return rc;
    ForestIo& io = c->fio;
    hipStream_t s = c->stream;
    const size_t r = (size_t)total;
    for (auto* b : {&io.sx, &io.sy, &io.syaw}) PP_HIP(b->reserve(r));
    PP_HIP(io.spar.reserve(r));
    if (star) {
        for (auto* b : {&io.scost, &io.selen}) PP_HIP(b->reserve(r));
        PP_HIP(io.lvl.reserve(r));
        if (st.cost) PP_HIP(io.scost_in.reserve(r));
    }
    auto in = [&](void* dst, const void* src, size_t bytes) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    };
    PP_HIP(in(io.off.p, st.off, (z + 1) * sizeof(int64_t)));
    PP_HIP(in(io.sx.p, st.x, r * sizeof(double)));
    PP_HIP(in(io.sy.p, st.y, r * sizeof(double)));
    PP_HIP(in(io.syaw.p, st.yaw, r * sizeof(double)));
    PP_HIP(in(io.spar.p, st.parent, r * sizeof(int)));
    PP_HIP(in(io.sit.p, st.iterations, z * sizeof(int64_t)));
    PP_HIP(in(io.sseed.p, st.seeds, z * sizeof(uint64_t)));
    PP_HIP(in(io.sevals.p, st.node_evals, z * sizeof(int64_t)));
    PP_HIP(in(io.sblocked.p, blk.data(), z));
    if (star) {
        PP_HIP(in(io.selen.p, st.edge_cost, r * sizeof(double)));
        if (st.cost) PP_HIP(in(io.scost_in.p, st.cost, r * sizeof(double)));
        PP_HIP(in(io.srew.p, st.rewires, z * sizeof(int64_t)));
        PP_HIP(in(io.sfxy.p, st.focus_xy, 2 * z * sizeof(double)));
        PP_HIP(in(io.sfbound.p, st.focus_bound, z * sizeof(double)));
        PP_HIP(in(io.sskipped.p, st.skipped, z * sizeof(int64_t)));
    }
    a.total = total;
    a.sx = io.sx.p;
    a.sy = io.sy.p;
    a.syaw = io.syaw.p;
    a.spar = io.spar.p;
    if (star) {
        a.scost = io.scost.p;
        a.selen = io.selen.p;
        a.scost_in = st.cost ? io.scost_in.p : nullptr;
        a.lvl = io.lvl.p;
    }
    a.sblocked = io.sblocked.p;
    PP_HIP(launch_forest_validate(s, a));
    std::vector<int> verdict(z, 0);
    PP_HIP(hipMemcpyAsync(verdict.data(), io.verdict.p, z * sizeof(int), hipMemcpyDeviceToHost, s));
    PP_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < m; ++i)
        if (verdict[(size_t)i] != kFioOk)
            return fail(i, PP_ERR_INVALID_ARGUMENT, verdict_text(verdict[(size_t)i]));
    // ---- nothing can fail any more: write the slots and what the library derives for them
    if (any_blk && !f.any_blocked) {  // the forest's first blocked root
        PP_HIP(f.blocked.reserve((size_t)f.Q));
        PP_HIP(hipMemsetAsync(f.blocked.p, 0, (size_t)f.Q, s));
        f.any_blocked = true;
    }
    a.blocked = f.any_blocked ? f.blocked.p : nullptr;
    PP_HIP(launch_forest_scatter(s, a));
    PP_HIP(hipStreamSynchronize(s));
    if (!star)
        for (int i = 0; i < m; ++i)
            std::memcpy(t.b->goal.data() + 3 * (size_t)slots[(size_t)i], st.goals + 3 * (size_t)i,
                        3 * sizeof(double));
    return PP_OK;
}

int star_target(pp_ctx* ctx, Target* t) {
    int rc = star_ready(ctx);
    if (rc) return rc;
    t->f = &ctx->star.f;
    t->s = &ctx->star;
    return PP_OK;
}

int batch_target(pp_ctx* ctx, bool stale_ok, Target* t) {
    int rc = check_ctx(ctx, false, false);
    if (rc) return rc;
    Batch& b = ctx->batch;
    if (!b.valid && !b.stale) return set_err(PP_ERR_STATE, "pp_batch_new has not been called");
    if (!b.valid && !stale_ok)
        return set_err(PP_ERR_STATE, "the batch is stale after a scene change: pp_batch_revalidate first");
    t->f = &b.f;
    t->b = &b;
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_star_forest_export(pp_ctx* ctx, const int32_t* queries, int m, pp_forest_state* state,
                          int64_t cap, int64_t* n_total) {
    Target t;
    int rc = star_target(ctx, &t);
    return rc ? rc : forest_export(ctx, t, queries, m, state, cap, n_total);
}

int pp_star_forest_import(pp_ctx* ctx, const int32_t* queries, int m,
                          const pp_forest_state* state, int32_t* bad_query) {
    Target t;
    int rc = star_target(ctx, &t);
    return rc ? rc : forest_import(ctx, t, queries, m, state, bad_query);
}

int pp_batch_forest_export(pp_ctx* ctx, const int32_t* queries, int m, pp_forest_state* state,
                           int64_t cap, int64_t* n_total) {
    Target t;
    int rc = batch_target(ctx, true, &t);
    return rc ? rc : forest_export(ctx, t, queries, m, state, cap, n_total);
}

int pp_batch_forest_import(pp_ctx* ctx, const int32_t* queries, int m,
                           const pp_forest_state* state, int32_t* bad_query) {
    Target t;
    int rc = batch_target(ctx, false, &t);
    return rc ? rc : forest_import(ctx, t, queries, m, state, bad_query);
}

}  // extern "C"

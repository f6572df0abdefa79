// pp_batch.cpp — the query batches: the forest of per-query trees, the config-3 extend batch
// (pp_batch_*) and the RRT* batch (pp_star_*) on top of it.
#include "pp_ctx.h"

#include <limits>

using namespace ppamd;

int Forest::init(pp_ctx* c, int q, int64_t max_iter_, double step_, const double* starts,
                 const uint64_t* seeds, int nsub_) {
    const size_t rows = (size_t)q * (size_t)(max_iter_ + 1);
    for (auto* b : {&x, &y, &yaw}) PP_HIP(b->reserve(rows));
    PP_HIP(parent.reserve(rows));
    PP_HIP(n.reserve(q));
    for (auto* b : {&it, &evals, &target}) PP_HIP(b->reserve(q));
    PP_HIP(seed.reserve(q));
    PP_HIP(d_starts.reserve(3 * (size_t)q));
    Q = q;
    cap = (int)(max_iter_ + 1);
    max_iter = max_iter_;
    step = step_;
    nsub = nsub_;
    any_blocked = false;
    hipStream_t st = c->stream;
    PP_HIP(hipMemcpyAsync(d_starts.p, starts, 3 * (size_t)q * sizeof(double), hipMemcpyHostToDevice, st));
    PP_HIP(launch_mq_init(st, dev(), d_starts.p));
    PP_HIP(hipMemcpyAsync(seed.p, seeds, q * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    // polygon mode: queries whose root fails verify never insert (see pp_rrt_new)
    if (c->scene.polygons()) {
        std::vector<uint8_t> blk(q);
        for (int i = 0; i < q; ++i) {
            blk[i] = c->scene.point_ok(starts[3 * i], starts[3 * i + 1]) ? 0 : 1;
            any_blocked |= blk[i] != 0;
        }
        PP_HIP(blocked.reserve(q));
        PP_HIP(hipMemcpy(blocked.p, blk.data(), q, hipMemcpyHostToDevice));
    }
    return PP_OK;
}

MqDev Forest::dev() const {
    MqDev d{};
    d.Q = Q;
    d.cap = cap;
    d.max_iter = max_iter;
    d.x = x.p;
    d.y = y.p;
    d.yaw = yaw.p;
    d.parent = parent.p;
    d.n = n.p;
    d.it = it.p;
    d.evals = evals.p;
    d.seed = seed.p;
    d.blocked = blocked_dev();
    d.K = 1;
    d.target = target.p;
    return d;
}

MqDev Forest::sub(MqDev d, int q0, int q1) const {
    const size_t r0 = (size_t)q0 * cap;
    d.Q = q1 - q0;
    d.x += r0;
    d.y += r0;
    d.yaw += r0;
    d.parent += r0;
    d.n += q0;
    d.it += q0;
    d.evals += q0;
    d.seed += q0;
    if (d.blocked) d.blocked += q0;
    d.target += q0;
    return d;
}

TreeDev Forest::tree_dev() const {
    TreeDev tr{};
    tr.x = x.p;
    tr.y = y.p;
    tr.yaw = yaw.p;
    tr.parent = parent.p;
    return tr;
}

int Forest::totals(pp_ctx* c, int64_t* it_sum, int64_t* n_sum, const int64_t* extra,
                   int64_t* extra_sum) const {
    std::vector<int> hn(Q);
    std::vector<int64_t> hit(Q), hex(extra ? Q : 0);
    PP_HIP(hipMemcpyAsync(hn.data(), n.p, Q * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PP_HIP(hipMemcpyAsync(hit.data(), it.p, Q * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (extra)
        PP_HIP(hipMemcpyAsync(hex.data(), extra, Q * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    PP_HIP(hipStreamSynchronize(c->stream));
    int64_t a = 0, b = 0, w = 0;
    for (int i = 0; i < Q; ++i) {
        a += hit[i];
        b += hn[i];
        if (extra) w += hex[i];
    }
    *it_sum = a;
    *n_sum = b;
    if (extra) *extra_sum = w;
    return PP_OK;
}

int Forest::copy_state(pp_ctx* c, int32_t* n_nodes, int64_t* iterations, int64_t* node_evals,
                       const int64_t* extra, int64_t* extra_out) const {
    hipStream_t st = c->stream;
    if (n_nodes) PP_HIP(hipMemcpyAsync(n_nodes, n.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    if (iterations) PP_HIP(hipMemcpyAsync(iterations, it.p, Q * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (node_evals) PP_HIP(hipMemcpyAsync(node_evals, evals.p, Q * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (extra_out) PP_HIP(hipMemcpyAsync(extra_out, extra, Q * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

int Forest::sizes(pp_ctx* c, std::vector<int>* hn, int64_t* total, const int32_t* nodes,
                  const char* bad_node) const {
    hn->assign((size_t)Q, 0);
    PP_HIP(hipMemcpyAsync(hn->data(), n.p, Q * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PP_HIP(hipStreamSynchronize(c->stream));
    int64_t sum = 0;
    for (int q = 0; q < Q; ++q) {
        sum += (*hn)[(size_t)q];
        if (nodes && (nodes[q] < -1 || nodes[q] >= (*hn)[(size_t)q]))
            return set_err(PP_ERR_INVALID_ARGUMENT, bad_node);
    }
    if (total) *total = sum;
    return PP_OK;
}

int Forest::reval_inputs(pp_ctx* c, std::vector<int>* hn, std::vector<uint8_t>* blk, bool* any) const {
    hipStream_t st = c->stream;
    hn->assign((size_t)Q, 0);
    std::vector<double> starts(3 * (size_t)Q);
    PP_HIP(hipMemcpyAsync(hn->data(), n.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(starts.data(), d_starts.p, starts.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    // the roots that fail verify in the scene as it is now (Forest::init)
    blk->assign((size_t)Q, 0);
    *any = false;
    if (c->scene.polygons())
        for (int q = 0; q < Q; ++q) {
            (*blk)[(size_t)q] = c->scene.point_ok(starts[3 * (size_t)q], starts[3 * (size_t)q + 1]) ? 0 : 1;
            *any |= (*blk)[(size_t)q] != 0;
        }
    return PP_OK;
}

int Forest::reval_outputs(pp_ctx* c, const std::vector<uint8_t>& blk, bool any, int32_t* n_nodes) {
    hipStream_t st = c->stream;
    if (any) {
        PP_HIP(blocked.reserve(Q));
        PP_HIP(hipMemcpy(blocked.p, blk.data(), Q, hipMemcpyHostToDevice));
    }
    any_blocked = any;
    if (n_nodes) PP_HIP(hipMemcpyAsync(n_nodes, n.p, Q * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

int Forest::export_tree(pp_ctx* c, int query, double* ox, double* oy, double* oyaw, int32_t* oparent,
                        int64_t ocap, int64_t* n_out, const double* extra, double* extra_out) const {
    if (query < 0 || query >= Q) return set_err(PP_ERR_INVALID_ARGUMENT, "query out of range");
    int nn = 0;
    PP_HIP(hipMemcpy(&nn, n.p + query, sizeof(int), hipMemcpyDeviceToHost));
    if (n_out) *n_out = nn;
    if (ocap < nn) return set_err(PP_ERR_CAPACITY, "export buffer smaller than the tree");
    const size_t o = (size_t)query * cap;
    hipStream_t st = c->stream;
    if (ox) PP_HIP(hipMemcpyAsync(ox, x.p + o, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    if (oy) PP_HIP(hipMemcpyAsync(oy, y.p + o, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    if (oyaw) PP_HIP(hipMemcpyAsync(oyaw, yaw.p + o, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    if (oparent) PP_HIP(hipMemcpyAsync(oparent, parent.p + o, nn * sizeof(int), hipMemcpyDeviceToHost, st));
    if (extra_out) PP_HIP(hipMemcpyAsync(extra_out, extra + o, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

namespace {

// streams: 2 for the extend batch (2: 289M it/s at 8192 queries, 177M on a 1024-query shard; 3:
// 291M / 160M; 4: 244M / 109M), 3 for RRT* (11 kernels a step: 16.4M / 4.5M against 15.0M / 4.2M
// with 2; 4 streams collapse to 10.7M / 2.4M, the box runs 4 hardware queues per process)
int mq_nsub(int Q, int dflt = 2) {
    int n = Q >= 256 ? dflt : 1;
    return std::min(n, std::max(Q, 1));
}

// `steps` lockstep steps of a forest's nsub sub-batches, each sub-batch on its own stream so one's
// small kernels overlap another's walk (results do not depend on the split: queries are
// independent), then the join and the error word.  fork: the first run after the extend call's
// target kernel (the sub-streams start after it).  launch(sub, stream, steps, ev) enqueues steps
// of sub-batch `sub` (of the whole forest when nsub == 1), its `evs` profiling events per step at
// ev (or null); account(ev) books one step's events.  before_err(stream) enqueues what the caller
// reads in the same synchronisation as the error word.
template <class Launch, class Account, class BeforeErr>
int run_sub_batches(pp_ctx* c, int nsub, bool fork, int64_t steps, int evs, const int* d_err,
                    Launch&& launch, Account&& account, BeforeErr&& before_err) {
    hipStream_t sst[kMaxSub] = {c->stream};
    for (int i = 1; i < nsub; ++i) {
        if (fork && !c->sub_stream[i])
            PP_HIP(hipStreamCreateWithFlags(&c->sub_stream[i], hipStreamNonBlocking));
        sst[i] = c->sub_stream[i];
    }
    if (fork && nsub > 1) {  // fork after the target kernel
        if (!c->fork_ev) PP_HIP(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
        PP_HIP(hipEventRecord(c->fork_ev, c->stream));
        for (int i = 1; i < nsub; ++i) PP_HIP(hipStreamWaitEvent(sst[i], c->fork_ev, 0));
    }
    Profiling& p = c->prof;
    for (int64_t done = 0; done < steps;) {
        const int chunk = (int)std::min<int64_t>(steps - done, 256);
        if (p.on)
            if (int r = ensure_events(c, (size_t)evs * chunk * nsub)) return r;
        if (nsub > 1) {  // interleaved, so every stream always holds work
            for (int k = 0; k < chunk; ++k)
                for (int i = 0; i < nsub; ++i)
                    PP_HIP(launch(i, sst[i], 1, p.on ? p.ev.data() + evs * ((size_t)k * nsub + i) : nullptr));
        } else {
            PP_HIP(launch(0, c->stream, chunk, p.on ? p.ev.data() : nullptr));
        }
        if (p.on) {  // (profiled too: the events time the schedule that runs)
            for (int i = 0; i < nsub; ++i) PP_HIP(hipStreamSynchronize(sst[i]));
            for (size_t e = 0; e < (size_t)chunk * nsub; ++e)
                if (int r = account(p.ev.data() + evs * e)) return r;
        }
        done += chunk;
    }
    for (int i = 1; i < nsub; ++i) {  // join: the host reads the counters on `stream`
        PP_HIP(hipEventRecord(c->fork_ev, sst[i]));
        PP_HIP(hipStreamWaitEvent(c->stream, c->fork_ev, 0));
    }
    if (int r = before_err(c->stream)) return r;
    int err = 0;
    PP_HIP(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PP_HIP(hipStreamSynchronize(c->stream));
    if (err) return set_err(PP_ERR_STEER_OVERFLOW, "generate_local_course would index past n_point");
    return PP_OK;
}

// the extend batch's (config 3) kernel arguments: the forest plus its window arrays
MqArgs mq_args(pp_ctx* c) {
    const Batch& b = c->batch;
    MqArgs a;
    a.mq = b.f.dev();
    a.mq.K = b.K;
    a.mq.nnd2 = b.nnd2.p;
    a.mq.it_prev = b.itprev.p;
    a.mq.status = b.status.p;
    a.mq.alist = b.alist.p;
    a.mq.ctask = b.ctask.p;
    a.mq.lstat = b.lstat.p;
    a.mq.tyaw = b.yawbuf.p;
    a.sc = c->scene_dev();
    a.sc.step_size = b.f.step;
    a.st = b.state.p;
    a.tasks = b.tasks.p;
    a.rec = b.rec.p;
    a.status = b.status.p;
    a.yaw = b.yawbuf.p;
    a.lit_scratch = c->api_lit_scratch.p;
    a.lit_locks = c->lit_locks.p;
    a.err = b.err.p;
    a.wg_points = c->prof.points();
    a.scp = b.scene.p;  // (uploaded by pp_batch_extend)
    a.mq.st = a.st;
    return a;
}

// Sub-batch s of the batch: the forest's view of its queries, the window arrays' task regions
// (K slots per query) and its own DevState.
constexpr size_t kLstatPad = 1024;  // >= the walk's grid (kWalkMaxWG, pp_steer_launch.h)
MqArgs mq_sub_args(pp_ctx* c, int sub) {
    const Batch& b = c->batch;
    MqArgs a = mq_args(c);
    const int q0 = b.f.q_begin(sub);
    const size_t t0 = (size_t)q0 * b.K;
    a.mq = b.f.sub(a.mq, q0, b.f.q_begin(sub + 1));
    a.mq.nnd2 += t0;
    if (a.mq.it_prev) a.mq.it_prev += q0;
    if (a.mq.status) a.mq.status += t0;
    if (a.mq.alist) a.mq.alist += t0;
    if (a.mq.ctask) a.mq.ctask += t0;
    // (a sub-batch's verdict array spans its tasks plus one walk grid: DevState::lper rounds up)
    if (a.mq.lstat) a.mq.lstat += t0 + (size_t)sub * kLstatPad;
    if (a.mq.tyaw) a.mq.tyaw += t0;
    a.st = b.state.p + 1 + sub;
    a.mq.st = a.st;
    a.tasks += t0;
    a.rec += t0;
    a.status += t0;
    a.yaw += t0;
    return a;
}

// DevState 0: the whole batch; 1 + s: sub-batch s of the forest's nsub
int mq_write_states(pp_ctx* c, hipStream_t st) {
    Batch& b = c->batch;
    DevState ds[1 + kMaxSub] = {};
    // W counts the step's active tasks (mq_sample_nn lists them, the insert resets it): 0 here;
    // each state's list is its task region's part of alist
    ds[0].alist = b.alist.p;
    for (int s = 0; s < b.f.nsub; ++s) ds[1 + s].alist = b.alist.p + (size_t)b.f.q_begin(s) * b.K;
    PP_HIP(hipMemcpyAsync(b.state.p, ds, sizeof ds, hipMemcpyHostToDevice, st));
    PP_HIP(hipStreamSynchronize(st));  // ds lives on this stack frame
    return PP_OK;
}

// per-step task buffers of the batch: K slots per query
int mq_reserve_tasks(pp_ctx* c, int q, int K) {
    Batch& b = c->batch;
    const size_t tq = (size_t)q * K;
    PP_HIP(b.tasks.reserve(tq));
    PP_HIP(b.ctask.reserve(tq));
    PP_HIP(b.status.reserve(tq));
    PP_HIP(b.yawbuf.reserve(tq));
    PP_HIP(b.rec.reserve(tq));
    PP_HIP(b.nnd2.reserve(tq));
    PP_HIP(b.alist.reserve(tq));
    PP_HIP(b.lstat.reserve(tq + (size_t)kMaxSub * kLstatPad));
    return PP_OK;
}

}  // namespace

// |X_near| of an insert into an n-node RRT* tree: k_fixed, or the k-nearest RRT* schedule
// ceil(2e ln n) (Karaman & Frazzoli), capped at kStarKMax and at n (orc_star_k restates it)
int ppamd::star_k(int k_fixed, int n) {
    int k;
    if (k_fixed > 0) {
        k = k_fixed;
    } else {
        const double v = n > 1 ? std::ceil(2.0 * 2.718281828459045 * std::log((double)n)) : 1.0;
        k = v < 1.0 ? 1 : (v > kStarKMax ? kStarKMax : (int)v);
    }
    if (k > kStarKMax) k = kStarKMax;
    return k < n ? k : n;
}

StarArgs ppamd::star_args(pp_ctx* c) {
    const StarBatch& s = c->star;
    StarArgs a;
    StarDev& d = a.sd;
    d.mq = s.f.dev();
    d.fxy = s.fxy.p;
    d.fbound = s.fbound.p;
    d.skipped = s.skipped.p;
    d.cost = s.cost.p;
    d.elen = s.elen.p;
    d.mark = s.mark.p;
    d.stamp = s.stamp.p;
    d.ksched = s.ksched.p;
    d.eta = s.eta;
    d.px = s.px.p;
    d.py = s.py.p;
    d.pn = s.pn.p;
    d.near = s.near.p;
    d.nnear = s.nnear.p;
    d.bslot = s.bslot.p;
    d.cslot = s.cslot.p;
    d.cmask = s.cmask.p;
    d.bmask = s.bmask.p;
    d.curv = 1.0 / c->scene.max_steer;
    d.lit_locks = c->lit_locks.p;
    d.cb = s.cb.p;
    d.rewires = s.rew.p;
    d.stA = s.state.p;
    d.stB = s.state.p + 1;
    d.stC = s.state.p + 2;
    a.sc = c->scene_dev();
    a.sc.step_size = s.f.step;
    a.tA = s.tA.p;
    a.tB = s.tB.p;
    a.tC = s.tC.p;
    a.eB = s.eB.p;
    a.eC = s.eC.p;
    a.sA = s.sA.p;
    a.sB = s.sB.p;
    a.sC = s.sC.p;
    a.yA = s.yA.p;
    a.yB = s.yB.p;
    a.yC = s.yC.p;
    a.cA = s.cA.p;
    a.cB = s.cB.p;
    a.cC = s.cC.p;
    a.rec = s.rec.p;
    a.lit_scratch = c->api_lit_scratch.p;
    a.err = s.err.p;
    a.wg_points = c->prof.points();
    return a;
}

namespace {

// Sub-batch s of the RRT* batch (as mq_sub_args): the forest's view of its queries, RRT*'s own
// per-query and per-row arrays, its own round states and task regions (rounds B / C: kStarKMax
// slots per query)
StarArgs star_sub_args(pp_ctx* c, int sub) {
    const StarBatch& s = c->star;
    StarArgs a = star_args(c);
    const int q0 = s.f.q_begin(sub);
    const size_t r0 = (size_t)q0 * s.f.cap, b0 = (size_t)q0 * kStarKMax;
    StarDev& d = a.sd;
    d.mq = s.f.sub(d.mq, q0, s.f.q_begin(sub + 1));
    d.fxy += 2 * (size_t)q0;
    d.fbound += q0;
    d.skipped += q0;
    d.cost += r0;
    d.elen += r0;
    d.mark += r0;
    d.stamp += q0;
    d.px += q0;
    d.py += q0;
    d.pn += q0;
    d.near += b0;
    d.nnear += q0;
    d.bslot += q0;
    d.bmask += q0;
    d.cslot += q0;
    d.cmask += q0;
    d.cb += q0;
    d.rewires += q0;
    d.stA = s.state.p + 3 * (1 + sub);
    d.stB = d.stA + 1;
    d.stC = d.stA + 2;
    a.tA += q0;
    a.sA += q0;
    a.yA += q0;
    a.cA += q0;
    a.tB += b0;
    a.tC += b0;
    a.eB += b0;
    a.eC += b0;
    a.sB += b0;
    a.sC += b0;
    a.yB += b0;
    a.yC += b0;
    a.cB += b0;
    a.cC += b0;
    a.rec += b0;
    return a;
}

}  // namespace

extern "C" {

int pp_batch_new(pp_ctx* ctx, int q, const double* starts, const double* goals,
                 const uint64_t* seeds, int64_t max_iter, double step_size) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    if (q <= 0 || !starts || !seeds || max_iter < 0 || max_iter > 0x7ffffff0 || !(step_size > 0.0))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad batch arguments");
    if ((int64_t)q * (max_iter + 1) > ((int64_t)1 << 34)) return set_err(PP_ERR_CAPACITY, "batch too large");
    for (const double* v : {starts, starts + 1, goals, goals ? goals + 1 : nullptr})
        if ((r = check_coords(v, q, 3, "starts and goals"))) return r;
    Batch& b = ctx->batch;
    b.valid = false;
    b.stale = false;
    hipStream_t st = ctx->stream;
    PP_HIP(b.itprev.reserve(q));
    PP_HIP(b.state.reserve(1 + kMaxSub));
    PP_HIP(b.err.reserve(1));
    if ((r = ensure_literal_pool(ctx, st))) return r;
    b.goal.assign(goals ? goals : starts, (goals ? goals : starts) + 3 * (size_t)q);
    // (the sub-batch DevStates below are written for the forest's split)
    if ((r = b.f.init(ctx, q, max_iter, step_size, starts, seeds, mq_nsub(q)))) return r;
    // default window: 32 iterations per query and step while that stays within 262144 tasks.
    // With the active-task list (round 5) a cut window's re-drawn slots cost neither a prep nor a
    // walk, and longer windows pay on the full batch too: 8192 queries 684 M it/s at K = 16
    // against 712 M at 32; the 1024-query shard 274 M at 16, 339 M at 32 and 64
    // (gpurun_out/r05kw; rounds 1-4 measured 16 best for the full batch without the list)
    if (b.K_user > 0) {
        b.K = b.K_user;
    } else {
        int K = kMqAutoK;
        while (K > 1 && (int64_t)q * K > 262144) K >>= 1;
        b.K = K;
    }
    if ((r = mq_reserve_tasks(ctx, q, b.K))) return r;
    // the verdict cache starts empty: it_prev far below any iteration (0x80.. bytes)
    PP_HIP(hipMemsetAsync(b.itprev.p, 0x80, q * sizeof(int64_t), st));
    if ((r = mq_write_states(ctx, st))) return r;
    PP_HIP(hipMemsetAsync(b.err.p, 0, sizeof(int), st));
    PP_HIP(hipStreamSynchronize(st));
    if ((r = ctx->prof.reset_host_stats(st))) return set_err(r, "resetting the statistics");
    b.valid = true;
    return PP_OK;
}

int pp_batch_set_window(pp_ctx* ctx, int k) {
    if (!ctx) return set_err(PP_ERR_INVALID_ARGUMENT, "null context");
    if (k < 0 || k > kMqMaxK || (k & (k - 1)))
        return set_err(PP_ERR_INVALID_ARGUMENT, "batch window must be 0 (automatic) or a power of two <= 64");
    Batch& b = ctx->batch;
    b.K_user = k;
    if (b.valid && k > 0) {  // applies from the next pp_batch_extend
        PP_HIP(hipStreamSynchronize(ctx->stream));
        int r = mq_reserve_tasks(ctx, b.f.Q, k);
        if (r) return r;
        b.K = k;
        // a new window length: the task region's layout changes, the verdict cache is void
        PP_HIP(hipMemsetAsync(b.itprev.p, 0x80, b.f.Q * sizeof(int64_t), ctx->stream));
        if ((r = mq_write_states(ctx, ctx->stream))) return r;
        PP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PP_OK;
}

int pp_batch_extend(pp_ctx* ctx, int64_t n_steps, int64_t* n_iterations, int64_t* n_accepted) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    Batch& b = ctx->batch;
    if (!b.valid) return set_err(PP_ERR_STATE, "pp_batch_new has not been called");
    if (n_steps < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "n_steps < 0");
    int64_t it0 = 0, n0 = 0, it1 = 0, n1 = 0;
    if ((n_iterations || n_accepted) && (r = b.f.totals(ctx, &it0, &n0))) return r;
    {  // the batch's scene in device memory (point_blocked)
        if (!b.scene.p) PP_HIP(b.scene.reserve(1));
        const SceneDev sd = mq_args(ctx).sc;
        PP_HIP(hipMemcpy(b.scene.p, &sd, sizeof sd, hipMemcpyHostToDevice));
    }
    const int K = b.K, Q = b.f.Q, nsub = b.f.nsub;
    const MqArgs all = mq_args(ctx);
    MqArgs sub[kMaxSub] = {all};  // (one sub-batch: the whole batch's view and DevState 0)
    for (int i = 0; i < nsub && nsub > 1; ++i) sub[i] = mq_sub_args(ctx, i);
    // an earlier call's PP_ERR_STEER_OVERFLOW does not stick to this one
    PP_HIP(hipMemsetAsync(b.err.p, 0, sizeof(int), ctx->stream));
    PP_HIP(launch_mq_target(ctx->stream, all.mq, n_steps, b.f.target.p));  // (every query's)
    Profiling& p = ctx->prof;
    auto launch = [&](int i, hipStream_t s, int steps, hipEvent_t* ev) {
        sub[i].ev = ev;
        return launch_mq_steps(s, sub[i], steps);
    };
    auto account = [&](const hipEvent_t* ev) {  // before mq_sample_nn, after it, prep, walk and insert
        double* acc[4] = {&p.nn_scan_ms, &p.prep_ms, &p.steer_ms, &p.insert_ms};
        for (int k = 0; k < 4; ++k) {
            float ms = 0.f;
            PP_HIP(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            *acc[k] += ms;
        }
        p.nn_scan_launches += 1;
        p.steer_launches += 1;
        return (int)PP_OK;
    };
    // every query advances n_steps iterations (to max_iter at most); a window advances up to K
    // of them, fewer when the in-order replay stops early, so the host tops the steps up until
    // every query has reached its target
    int64_t steps = (n_steps + K - 1) / K;
    std::vector<int64_t> hit(Q), htg(Q);
    auto counters = [&](hipStream_t s) {
        PP_HIP(hipMemcpyAsync(hit.data(), b.f.it.p, Q * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        PP_HIP(hipMemcpyAsync(htg.data(), b.f.target.p, Q * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        return (int)PP_OK;
    };
    for (int pass = 0; steps > 0; ++pass) {
        if (pass > 64 + n_steps) return set_err(PP_ERR_HIP, "batch extend made no progress");
        if ((r = run_sub_batches(ctx, nsub, pass == 0, steps, 5, b.err.p, launch, account, counters)))
            return r;
        p.batch_steps += steps;
        p.batch_passes += 1;
        steps = 0;  // the top-up pass: queries whose windows stopped early
        for (int q = 0; q < Q; ++q) steps = std::max(steps, (htg[q] - hit[q] + K - 1) / K);
    }
    if ((n_iterations || n_accepted) && (r = b.f.totals(ctx, &it1, &n1))) return r;
    if (n_iterations) *n_iterations = it1 - it0;
    if (n_accepted) *n_accepted = n1 - n0;
    return PP_OK;
}

int pp_batch_state(pp_ctx* ctx, int32_t* n_nodes, int64_t* iterations, int64_t* node_evals) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    if (!ctx->batch.valid) return set_err(PP_ERR_STATE, "pp_batch_new has not been called");
    return ctx->batch.f.copy_state(ctx, n_nodes, iterations, node_evals);
}

int pp_batch_tree_export(pp_ctx* ctx, int query, double* x, double* y, double* yaw,
                         int32_t* parent, int64_t cap, int64_t* n) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    if (!ctx->batch.valid) return set_err(PP_ERR_STATE, "pp_batch_new has not been called");
    return ctx->batch.f.export_tree(ctx, query, x, y, yaw, parent, cap, n);
}

int pp_star_new(pp_ctx* ctx, int q, const double* starts, const uint64_t* seeds,
                int64_t max_iter, double step_size, int k, double eta) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    if (q <= 0 || !starts || !seeds || max_iter < 0 || max_iter > 0x7ffffff0 ||
        !(step_size > 0.0) || k < 0 || k > kStarKMax || !(eta >= 0.0))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad RRT* batch arguments");
    const int64_t cap64 = max_iter + 1;
    if ((int64_t)q * cap64 > ((int64_t)1 << 34) || (int64_t)q * kStarKMax > 0x7fffffff)
        return set_err(PP_ERR_CAPACITY, "RRT* batch too large");
    if ((r = check_coords(starts, q, 3, "starts")) || (r = check_coords(starts + 1, q, 3, "starts")))
        return r;
    const size_t rows = (size_t)q * (size_t)cap64, tb = (size_t)q * kStarKMax;
    StarBatch& s = ctx->star;
    s.valid = false;
    hipStream_t st = ctx->stream;
    for (auto* b : {&s.cost, &s.elen}) PP_HIP(b->reserve(rows));
    PP_HIP(s.mark.reserve(rows));
    PP_HIP(s.ksched.reserve((size_t)cap64 + 1));
    for (auto* b : {&s.stamp, &s.pn, &s.nnear, &s.bslot, &s.cslot, &s.sA}) PP_HIP(b->reserve(q));
    for (auto* b : {&s.px, &s.py, &s.cb, &s.yA, &s.cA}) PP_HIP(b->reserve(q));
    PP_HIP(s.rew.reserve(q));
    PP_HIP(s.fxy.reserve(2 * (size_t)q));
    PP_HIP(s.fbound.reserve(q));
    PP_HIP(s.skipped.reserve(q));
    for (auto* b : {&s.cmask, &s.bmask}) PP_HIP(b->reserve(q));
    PP_HIP(s.tA.reserve(q));
    for (auto* b : {&s.tB, &s.tC}) PP_HIP(b->reserve(tb));
    for (auto* b : {&s.eB, &s.eC}) PP_HIP(b->reserve(tb));
    for (auto* b : {&s.near, &s.sB, &s.sC}) PP_HIP(b->reserve(tb));
    for (auto* b : {&s.yB, &s.yC, &s.cB, &s.cC}) PP_HIP(b->reserve(tb));
    PP_HIP(s.rec.reserve(tb));
    PP_HIP(s.state.reserve(3 * (1 + kMaxSub)));
    PP_HIP(s.err.reserve(1));
    if ((r = ensure_literal_pool(ctx, st))) return r;
    s.kfix = k;
    s.eta = eta;
    std::vector<int> ks((size_t)cap64 + 1);
    for (int64_t n = 0; n <= cap64; ++n) ks[n] = star_k(k, (int)n);
    PP_HIP(hipMemcpy(s.ksched.p, ks.data(), ks.size() * sizeof(int), hipMemcpyHostToDevice));
    PP_HIP(hipMemsetAsync(s.mark.p, 0, rows * sizeof(int), st));
    {  // no focus: every bound +inf, nothing skipped
        const std::vector<double> inf((size_t)q, std::numeric_limits<double>::infinity());
        PP_HIP(hipMemcpy(s.fbound.p, inf.data(), q * sizeof(double), hipMemcpyHostToDevice));
        PP_HIP(hipMemsetAsync(s.fxy.p, 0, 2 * (size_t)q * sizeof(double), st));
        PP_HIP(hipMemsetAsync(s.skipped.p, 0, q * sizeof(int64_t), st));
    }
    // (the sub-batch DevStates below are written for the forest's split)
    if ((r = s.f.init(ctx, q, max_iter, step_size, starts, seeds, mq_nsub(q, 3)))) return r;
    // the roots once more (launch_star_init starts with the forest's init kernel), then their
    // cost, edge length, stamp and rewire count
    PP_HIP(launch_star_init(st, star_args(ctx), s.f.d_starts.p));
    DevState ds[3 * (1 + kMaxSub)] = {};
    ds[0].W = q;  // round A of the whole batch; sub-batch sb: 3 * (1 + sb)
    for (int sb = 0; sb < s.f.nsub; ++sb) ds[3 * (1 + sb)].W = s.f.q_begin(sb + 1) - s.f.q_begin(sb);
    PP_HIP(hipMemcpyAsync(s.state.p, ds, sizeof ds, hipMemcpyHostToDevice, st));
    PP_HIP(hipMemsetAsync(s.err.p, 0, sizeof(int), st));
    PP_HIP(hipStreamSynchronize(st));
    if ((r = ctx->prof.reset_host_stats(st))) return set_err(r, "resetting the statistics");
    s.valid = true;
    return PP_OK;
}

int pp_star_extend(pp_ctx* ctx, int64_t n_steps, int64_t* n_iterations, int64_t* n_accepted,
                   int64_t* n_rewires) {
    int r = star_ready(ctx);
    if (r) return r;
    StarBatch& s = ctx->star;
    if (n_steps < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "n_steps < 0");
    const bool tot = n_iterations || n_accepted || n_rewires;
    int64_t it0 = 0, n0 = 0, w0 = 0, it1 = 0, n1 = 0, w1 = 0;
    if (tot && (r = s.f.totals(ctx, &it0, &n0, s.rew.p, &w0))) return r;
    const int nsub = s.f.nsub;
    const StarArgs all = star_args(ctx);
    StarArgs sub[kMaxSub] = {all};  // (one sub-batch: the whole batch's view and states)
    for (int i = 0; i < nsub && nsub > 1; ++i) sub[i] = star_sub_args(ctx, i);
    PP_HIP(hipMemsetAsync(s.err.p, 0, sizeof(int), ctx->stream));  // per call, not sticky
    PP_HIP(launch_mq_target(ctx->stream, all.sd.mq, n_steps, s.f.target.p));  // (every query's)
    const int64_t steps = std::min<int64_t>(n_steps, s.f.max_iter);  // one iteration a step
    Profiling& p = ctx->prof;
    auto launch = [&](int i, hipStream_t stream, int n, hipEvent_t* ev) {
        sub[i].ev = ev;
        return launch_star_steps(stream, sub[i], n);
    };
    auto account = [&](const hipEvent_t* ev) {  // around star_sample, then around each round's walk
        float ms = 0.f;
        PP_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        p.nn_scan_ms += ms;
        for (int w = 1; w < 4; ++w) {
            PP_HIP(hipEventElapsedTime(&ms, ev[2 * w], ev[2 * w + 1]));
            p.steer_ms += ms;
        }
        p.nn_scan_launches += 1;
        p.steer_launches += 3;
        return (int)PP_OK;
    };
    if ((r = run_sub_batches(ctx, nsub, true, steps, 8, s.err.p, launch, account,
                             [](hipStream_t) { return (int)PP_OK; })))
        return r;
    if (tot && (r = s.f.totals(ctx, &it1, &n1, s.rew.p, &w1))) return r;
    if (n_iterations) *n_iterations = it1 - it0;
    if (n_accepted) *n_accepted = n1 - n0;
    if (n_rewires) *n_rewires = w1 - w0;
    return PP_OK;
}

int pp_star_state(pp_ctx* ctx, int32_t* n_nodes, int64_t* iterations, int64_t* node_evals,
                  int64_t* rewires) {
    int r = star_ready(ctx);
    if (r) return r;
    const StarBatch& s = ctx->star;
    return s.f.copy_state(ctx, n_nodes, iterations, node_evals, s.rew.p, rewires);
}

int pp_star_tree_export(pp_ctx* ctx, int query, double* x, double* y, double* yaw,
                        int32_t* parent, double* cost, int64_t cap, int64_t* n) {
    int r = star_ready(ctx);
    if (r) return r;
    const StarBatch& s = ctx->star;
    return s.f.export_tree(ctx, query, x, y, yaw, parent, cap, n, s.cost.p, cost);
}

static_assert(kStarFocusDraws == PP_STAR_FOCUS_DRAWS && kStarFocusDraws % 64 == 0,
              "the kernel's draw limit is the header's, in whole wave rounds");

int pp_star_set_focus(pp_ctx* ctx, const double* fxy, const double* bound) {
    if (int r = star_ready(ctx)) return r;
    StarBatch& s = ctx->star;
    if (!fxy != !bound)
        return set_err(PP_ERR_INVALID_ARGUMENT, "focus points and bounds: both or neither");
    const int q = s.f.Q;
    std::vector<double> inf;
    if (bound) {
        for (int i = 0; i < q; ++i)
            if (!(bound[i] > 0.0))  // (NaN fails the comparison too; +inf: that query has no focus)
                return set_err(PP_ERR_INVALID_ARGUMENT, "a focus bound must be > 0 or +inf");
        int r = check_coords(fxy, q, 2, "focus points");
        if (r || (r = check_coords(fxy + 1, q, 2, "focus points"))) return r;
    } else {
        inf.assign((size_t)q, std::numeric_limits<double>::infinity());
        bound = inf.data();
    }
    PP_HIP(hipStreamSynchronize(ctx->stream));
    if (fxy) PP_HIP(hipMemcpy(s.fxy.p, fxy, 2 * (size_t)q * sizeof(double), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(s.fbound.p, bound, q * sizeof(double), hipMemcpyHostToDevice));
    return PP_OK;
}

int pp_star_get_focus(pp_ctx* ctx, double* fxy, double* bound, int64_t* skipped) {
    if (int r = star_ready(ctx)) return r;
    const StarBatch& s = ctx->star;
    const int q = s.f.Q;
    hipStream_t st = ctx->stream;
    if (fxy) PP_HIP(hipMemcpyAsync(fxy, s.fxy.p, 2 * (size_t)q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (bound) PP_HIP(hipMemcpyAsync(bound, s.fbound.p, q * sizeof(double), hipMemcpyDeviceToHost, st));
    if (skipped) PP_HIP(hipMemcpyAsync(skipped, s.skipped.p, q * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

}  // extern "C"

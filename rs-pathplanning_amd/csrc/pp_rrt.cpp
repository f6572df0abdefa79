// pp_rrt.cpp — the one-tree planner: device-resident tree and planner state, the window enqueue
// loop, tree import / export and the nearest / verify_node / line_to_origin queries.
//
// Extend semantics: iteration it samples (x, y) from the seeded stream, takes
// the exact nearest node of the tree as it stands after iterations < it, steers child→parent with
// Dubins, verifies, inserts.  The GPU evaluates a window of K iterations against the tree
// snapshot at the window start, and a one-workgroup resolve kernel replays the window in order:
//   * sample j's true parent is the nearest of {snapshot NN} ∪ {accepted window samples i < j};
//     nn_finalize's pair search lists the i that are strictly nearer than the snapshot NN, so the parent is
//     the first accepted entry of that list in (d2, i) order, or the snapshot NN;
//   * the verdict for (j, parent) was precomputed for the snapshot NN and for every listed i
//     under i's own snapshot parent; only a parent that itself changed needs a repair steer.
// The result is identical to the one-at-a-time sequential spec for every K.  All planner state
// (it, n, counters) lives in device memory, so the host enqueues windows back to back and
// synchronises once per batch of windows.
#include "pp_ctx.h"

using namespace ppamd;

namespace {

// The window pipeline is compiled for window sizes that are multiples of 256 (nn_scan sample
// blocks); any requested K runs inside a buffer of round_up(K, 256).
int ensure_window(pp_ctx* c, int K) {
    K = (K + 255) & ~255;
    if (K <= c->rrt.Kcap) return PP_OK;
    const size_t k = (size_t)K;
    PP_HIP(c->rrt.wsx.reserve(2 * k));  // double-buffered by window parity
    PP_HIP(c->rrt.wsy.reserve(2 * k));
    PP_HIP(c->rrt.wsx32.reserve(2 * k));
    PP_HIP(c->rrt.wsy32.reserve(2 * k));
    PP_HIP(c->rrt.perm.reserve(2 * k));
    PP_HIP(c->rrt.ipos.reserve(2 * k));
    PP_HIP(c->rrt.sxy.reserve(2 * k));
    PP_HIP(c->rrt.cofs.reserve(2 * 257));
    PP_HIP(c->rrt.sqb.reserve(2 * k));
    PP_HIP(c->rrt.ssx.reserve(2 * k));
    PP_HIP(c->rrt.ssy.reserve(2 * k));
    PP_HIP(c->rrt.ob.reserve(2 * (size_t)kMaxWindow / 256));
    PP_HIP(c->rrt.pbest.reserve(k * kMaxChunks));
    PP_HIP(c->rrt.psecond.reserve(k * kMaxChunks));
    PP_HIP(c->rrt.pidx.reserve(k * kMaxChunks));
    PP_HIP(c->rrt.nn_idx.reserve(k));
    PP_HIP(c->rrt.nn_d2.reserve(k));
    PP_HIP(c->rrt.cand_cnt.reserve(k));
    PP_HIP(c->rrt.cand.reserve(k * kCandCap));
    PP_HIP(c->rrt.rec.reserve(k + k * kCandCap));
    PP_HIP(c->rrt.snap_status.reserve(k));
    PP_HIP(c->rrt.snap_yaw.reserve(k));
    PP_HIP(c->rrt.snap_pose.reserve(3 * k));
    PP_HIP(c->rrt.r_order.reserve(k * kCandCap));
    PP_HIP(c->rrt.r_rep.reserve(k));
    PP_HIP(c->rrt.pend.reserve(k));
    PP_HIP(c->rrt.fin_par.reserve(k));
    PP_HIP(c->rrt.iter_off.reserve(2 * k));
    PP_HIP(hipMemsetAsync(c->rrt.cand_cnt.p, 0, k * sizeof(int), c->stream));
    PP_HIP(c->rrt.r_repyaw.reserve(k));
    PP_HIP(c->rrt.tasks.reserve(k));
    PP_HIP(c->rrt.task_status.reserve(k));
    PP_HIP(c->rrt.task_yaw.reserve(k));
    PP_HIP(c->rrt.h_tasks.reserve(k));
    PP_HIP(c->rrt.lit_scratch.reserve((size_t)(kResolveThreads / 64) * 3 * kLiteralCap));
    c->rrt.Kcap = K;
    return PP_OK;
}

template <typename T>
int grow_copy(pp_ctx* c, DBuf<T>& b, size_t old_n, size_t new_cap) {
    DBuf<T> nb;
    PP_HIP(nb.reserve(new_cap));
    if (old_n)
        PP_HIP(hipMemcpyAsync(nb.p, b.p, old_n * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    PP_HIP(hipStreamSynchronize(c->stream));
    std::swap(b.p, nb.p);
    std::swap(b.n, nb.n);
    return PP_OK;
}

int ensure_tree(pp_ctx* c, int64_t need) {
    if (need <= c->rrt.cap) return PP_OK;
    if (need > (int64_t)0x7fff0000) return set_err(PP_ERR_CAPACITY, "tree larger than 2^31 nodes");
    int64_t nc = std::max<int64_t>(need, c->rrt.cap * 2);
    nc = std::max<int64_t>(nc, 1024);
    int r;
    // the f32 screen copies get kScreenPad floats of slack: the screen's LDS-DMA reads whole
    // float4s, up to 3 floats past the last node
    if ((r = grow_copy(c, c->rrt.x32, c->rrt.n, nc + kScreenPad))) return r;
    if ((r = grow_copy(c, c->rrt.y32, c->rrt.n, nc + kScreenPad))) return r;
    if ((r = grow_copy(c, c->rrt.X, c->rrt.n, nc))) return r;
    if ((r = grow_copy(c, c->rrt.Y, c->rrt.n, nc))) return r;
    if ((r = grow_copy(c, c->rrt.YAW, c->rrt.n, nc))) return r;
    if ((r = grow_copy(c, c->rrt.PAR, c->rrt.n, nc))) return r;
    c->rrt.cap = nc;
    return PP_OK;
}

// rows [0, z) of the tree from the host, with their f32 screen copies (z <= the capacity)
int upload_tree(pp_ctx* c, const double* x, const double* y, const double* yaw,
                const int32_t* parent, size_t z) {
    std::vector<float> fx(z), fy(z);
    for (size_t i = 0; i < z; ++i) {
        fx[i] = (float)x[i];
        fy[i] = (float)y[i];
    }
    Planner& p = c->rrt;
    PP_HIP(hipMemcpy(p.x32.p, fx.data(), z * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(p.y32.p, fy.data(), z * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(p.X.p, x, z * sizeof(double), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(p.Y.p, y, z * sizeof(double), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(p.YAW.p, yaw, z * sizeof(double), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(p.PAR.p, parent, z * sizeof(int32_t), hipMemcpyHostToDevice));
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_rrt_new(pp_ctx* ctx, double sx, double sy, double syaw, double gx, double gy, double gyaw,
               int64_t max_iter, double step_size, uint64_t seed, int64_t capacity) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    if (!(step_size > 0.0) || max_iter < 0)
        return set_err(PP_ERR_INVALID_ARGUMENT, "step_size must be > 0 and max_iter >= 0");
    const double ends[4] = {sx, sy, gx, gy};
    if ((r = check_coords(ends, 4, 1, "start and goal"))) return r;
    ctx->rrt.valid = false;
    ctx->rrt.stale = false;
    PP_HIP(hipStreamSynchronize(ctx->stream));
    ctx->rrt.n = 0;
    ctx->rrt.it = 0;
    ctx->rrt.start[0] = sx;
    ctx->rrt.start[1] = sy;
    ctx->rrt.start[2] = syaw;
    ctx->rrt.goal[0] = gx;
    ctx->rrt.goal[1] = gy;
    ctx->rrt.goal[2] = gyaw;
    ctx->rrt.max_iter = max_iter;
    ctx->rrt.step = step_size;
    ctx->rrt.seed = seed;
    if ((r = ctx->prof.reset_host_stats(ctx->stream))) return set_err(r, "resetting the statistics");
    if ((r = ensure_tree(ctx, std::max<int64_t>(capacity, 1024)))) return r;
    if ((r = ensure_window(ctx, ctx->rrt.K))) return r;
    // f32 screen tolerance: coordinates are rounded to f32 with error <= max|c| * 2^-24
    double mx = std::max({std::fabs(ctx->scene.minx), std::fabs(ctx->scene.maxx), std::fabs(ctx->scene.miny),
                          std::fabs(ctx->scene.maxy), std::fabs(sx), std::fabs(sy)});
    ctx->rrt.eps_coord = mx * std::ldexp(1.0, -23);
    // polygon mode: a root that fails verify fails every line_to_origin (it ends the line), so
    // nothing is ever inserted; the kernels' incremental verify assumes a free root (Q10p)
    ctx->rrt.root_blocked = ctx->scene.polygons() && !ctx->scene.point_ok(sx, sy);
    // RRT::new inserts the root (rrt.rs:344-346)
    const int32_t par = -1;
    if ((r = upload_tree(ctx, &sx, &sy, &syaw, &par, 1))) return r;
    DevState s{};
    s.it = 0;
    s.n = 1;
    s.n_scan = 1;
    s.it_spec = 0;
    s.void_seq = -1;
    s.kdyn = kMinDynWindow;  // a young tree starts with short windows (the commit adapts them)
    PP_HIP(hipMemcpy(ctx->rrt.d_state.p, &s, sizeof(DevState), hipMemcpyHostToDevice));
    ctx->rrt.h_state.p[0] = s;
    ctx->rrt.n = 1;
    ctx->rrt.blocked_share = -1.0;
    ctx->rrt.valid = true;
    return PP_OK;
}

int pp_rrt_set_window(pp_ctx* ctx, int k) {
    if (!ctx) return set_err(PP_ERR_INVALID_ARGUMENT, "null context");
    if (k < 1 || k > kMaxWindow)
        return set_err(PP_ERR_INVALID_ARGUMENT, "window must be in [1, 4096] (resolve state lives in LDS)");
    ctx->rrt.K = k;
    return PP_OK;
}

}  // extern "C"

namespace {

// The extend loop behind pp_rrt_extend (src: null, the seeded stream) and pp_rrt_extend_samples
// (src: the caller's samples of the iterations [ctx->rrt.it, ctx->rrt.it + n_iter), on the device, and
// the per-iteration record).  eps: the f32 screen tolerance of this call (the samples' magnitude).
struct SampleSrc {
    const double* x;
    const double* y;
    SampleRec rec;
    bool pretest;  // the obstacle pre-test may settle a sample without its nearest node
};

#ifdef PP_FIN_STAMPS
// diagnostic builds: append the last nn_finalize launch's phase stamps (per workgroup) to
// gpurun_out/fin_stamps.txt, one line per batch of windows: tree size, windows, then the stamps
void dump_fin_stamps(int64_t n, int nw) {
    std::vector<unsigned long long> v(kFinStampSlots * kFinStampWGs);
    if (fin_stamps_copy(v.data(), v.size()) != hipSuccess) return;
    FILE* f = std::fopen("gpurun_out/fin_stamps.txt", "a");
    if (!f) return;
    std::fprintf(f, "%lld %d", (long long)n, nw);
    for (unsigned long long x : v) std::fprintf(f, " %llu", x);
    std::fprintf(f, "\n");
    std::fclose(f);
}
#endif

int rrt_extend_impl(pp_ctx* ctx, int64_t n_iter, int64_t* n_accepted, const SampleSrc* src,
                    double eps) {
    int r;
    if ((r = ensure_window(ctx, ctx->rrt.K))) return r;
    if (ctx->rrt.root_blocked) {  // every iteration rejects: only the iteration counters advance
        DevState& s = ctx->rrt.h_state.p[0];
        PP_HIP(hipMemcpy(&s, ctx->rrt.d_state.p, sizeof(DevState), hipMemcpyDeviceToHost));
        s.it += n_iter;
        s.it_spec = s.it;
        s.iterations += n_iter;
        s.node_evals += n_iter * ctx->rrt.n;  // the NN of every iteration scans the fixed tree
        PP_HIP(hipMemcpy(ctx->rrt.d_state.p, &s, sizeof(DevState), hipMemcpyHostToDevice));
        ctx->rrt.it = s.it;
        if (n_accepted) *n_accepted = 0;
        return PP_OK;
    }
    const int64_t target = ctx->rrt.it + n_iter;
    const int64_t n_before = ctx->rrt.n;
    hipStream_t st = ctx->stream;
    {  // the scene in device memory for samples_role's point_blocked pre-test
        if (!ctx->rrt.d_scene.p) PP_HIP(ctx->rrt.d_scene.reserve(1));
        const SceneDev sd = ctx->scene_dev();
        PP_HIP(hipMemcpy(ctx->rrt.d_scene.p, &sd, sizeof sd, hipMemcpyHostToDevice));
    }
    // the pre-test settles the draws in an obstacle where they are drawn: a window holds Kd live
    // samples and spans more iterations (pp_window_fill.h)
    const bool pretest = !ctx->scene.polygons() && (!src || src->pretest);
    while (ctx->rrt.it < target) {
        const int K = ctx->rrt.K;
        // windows hold min(K, kdyn) samples (the device adapts kdyn): enough windows for the live
        // draws expected of the remaining iterations — their share from the previous batch's
        // counters, else from the pre-test's set cells — three standard deviations up; never
        // more than one per Kd iterations nor fewer than one per 2 Kd (a window's bounds).  A
        // window past the target is four empty launches, a shortfall another batch (this loop).
        const int64_t Kd = std::max(1, std::min(K, ctx->rrt.h_state.p[0].kdyn > 0 ? ctx->rrt.h_state.p[0].kdyn : K));
        const int64_t rem = target - ctx->rrt.it;
        const double share = !pretest ? 0.0
                             : ctx->rrt.blocked_share >= 0.0 ? ctx->rrt.blocked_share
                                                             : ctx->scene.blocked_share;
        const double live = (double)rem * (1.0 - share) +
                            3.0 * std::sqrt((double)rem * share * (1.0 - share));
        int64_t nw64 = (int64_t)std::ceil(live / (double)Kd);
        nw64 = std::max(nw64, (rem + 2 * Kd - 1) / (2 * Kd));
        nw64 = std::min(nw64, (rem + Kd - 1) / Kd);
        nw64 = std::min<int64_t>(std::max<int64_t>(nw64, 1), kMaxBatch);
        const int nw = (int)nw64;
        const int64_t it_before = ctx->rrt.it, blocked_before = ctx->rrt.h_state.p[0].blocked;
        if ((r = ensure_tree(ctx, ctx->rrt.n + (int64_t)nw * K))) return r;
        WindowArgs a = ctx->rrt.window_args(ctx->scene_dev(), ctx->prof.points(), ctx->rrt.d_state.p);
        a.K = K;
        a.target = target;
        a.eps_coord = eps;
        if (src) {
            a.hsx = src->x;
            a.hsy = src->y;
            a.hrec = src->rec;
            if (!src->pretest) a.pretest = 0;
        }
        if (ctx->prof.on && (r = ensure_events(ctx, 5 * (size_t)nw))) return r;
        const int64_t windows_before = ctx->rrt.h_state.p[0].windows;
        // windows are pipelined: window w's kernel resolves and commits w - 1; the drain launch
        // commits the batch's last window before the host reads the state
        for (int w = 0; w < nw; ++w)
            PP_HIP(launch_window(st, a, ctx->prof.on ? &ctx->prof.ev[5 * w] : nullptr, ctx->rrt.seq++, w > 0));
        PP_HIP(launch_drain(st, a, ctx->rrt.seq));
        PP_HIP(hipMemcpyAsync(ctx->rrt.h_state.p, ctx->rrt.d_state.p, sizeof(DevState), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
        const DevState& s = ctx->rrt.h_state.p[0];
        if (s.error)
            return set_err(PP_ERR_STEER_OVERFLOW,
                           "generate_local_course would index past n_point (the reference panics)");
        if (s.it <= ctx->rrt.it && nw > 0 && s.windows == windows_before)
            return set_err(PP_ERR_HIP, "extend made no progress");
        if (ctx->prof.on) {
            const int64_t active = std::min<int64_t>(s.windows - windows_before, nw);
            for (int64_t w = 0; w < active; ++w) {
                double* acc[4] = {&ctx->prof.nn_scan_ms, &ctx->prof.finalize_ms, &ctx->prof.prep_ms, &ctx->prof.steer_ms};
                for (int k = 0; k < 4; ++k) {
                    float ms = 0.f;
                    PP_HIP(hipEventElapsedTime(&ms, ctx->prof.ev[5 * w + k], ctx->prof.ev[5 * w + k + 1]));
                    *acc[k] += ms;
                }
            }
            ctx->prof.nn_scan_launches += active;
            ctx->prof.steer_launches += active;
        }
        ctx->rrt.it = s.it;
        ctx->rrt.n = s.n;
        if (pretest && s.it > it_before && s.blocked >= blocked_before)
            ctx->rrt.blocked_share = (double)(s.blocked - blocked_before) / (double)(s.it - it_before);
#ifdef PP_FIN_STAMPS
        dump_fin_stamps(ctx->rrt.n, nw);
#endif
    }
    if (n_accepted) *n_accepted = ctx->rrt.n - n_before;
    return PP_OK;
}

// pp_rrt_extend_samples' device buffers: samples and records of kHostChunk iterations at a time
constexpr int64_t kHostChunk = (int64_t)1 << 20;

// RRT::get_nearest_node of k points on the tree as it stands, Kcap points a launch.  eps: the f32
// screen's tolerance for this call — the planner's own, widened by the caller's points where they
// are larger than anything the scene bounds (their f32 copies round by up to |q| 2^-24).
int nearest_batch(pp_ctx* ctx, const double* qx, const double* qy, int k, int32_t* idx, double* d2,
                  double eps) {
    hipStream_t st = ctx->stream;
    WindowArgs a = ctx->rrt.window_args(ctx->scene_dev(), ctx->prof.points(), ctx->rrt.d_api_state.p);
    a.eps_coord = eps;
    for (int b = 0; b < k; b += ctx->rrt.Kcap) {
        const int nb = std::min(ctx->rrt.Kcap, k - b);
        DevState* hs = &ctx->rrt.h_state.p[1];
        *hs = DevState{};
        hs->W = nb;
        hs->Wp[0] = nb;
        hs->n = (int)ctx->rrt.n;
        hs->nsp[0] = (int)ctx->rrt.n;
        hs->n_scan = (int)ctx->rrt.n;
        hs->void_seq = -1;
        PP_HIP(hipMemcpyAsync(ctx->rrt.d_api_state.p, hs, sizeof(DevState), hipMemcpyHostToDevice, st));
        PP_HIP(hipMemcpyAsync(ctx->rrt.wsx.p, qx + b, nb * sizeof(double), hipMemcpyHostToDevice, st));
        PP_HIP(hipMemcpyAsync(ctx->rrt.wsy.p, qy + b, nb * sizeof(double), hipMemcpyHostToDevice, st));
        PP_HIP(launch_nearest(st, a));
        PP_HIP(hipMemcpyAsync(idx + b, ctx->rrt.nn_idx.p, nb * sizeof(int), hipMemcpyDeviceToHost, st));
        if (d2) PP_HIP(hipMemcpyAsync(d2 + b, ctx->rrt.nn_d2.p, nb * sizeof(double), hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
    }
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_rrt_extend(pp_ctx* ctx, int64_t n_iter, int64_t* n_accepted) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (n_iter < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "n_iter < 0");
    return rrt_extend_impl(ctx, n_iter, n_accepted, nullptr, ctx->rrt.eps_coord);
}

int pp_rrt_extend_samples(pp_ctx* ctx, const double* sx, const double* sy, int64_t k,
                          int32_t* nearest, double* yaw, uint8_t* ok, int64_t* n_accepted) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (k < 0 || (k > 0 && (!sx || !sy)))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad extend_samples arguments");
    double mx = 0.0;
    for (int64_t i = 0; i < k; ++i) {
        if (!std::isfinite(sx[i]) || !std::isfinite(sy[i]))
            return set_err(PP_ERR_INVALID_ARGUMENT, "a sample is not finite");
        mx = std::max({mx, std::fabs(sx[i]), std::fabs(sy[i])});
    }
    if (mx > PP_COORD_MAX) return set_err(PP_ERR_INVALID_ARGUMENT, "a sample exceeds PP_COORD_MAX");
    // the f32 screen's tolerance covers the coordinates it rounds: nodes and these samples
    const double eps = std::max(ctx->rrt.eps_coord, mx * std::ldexp(1.0, -23));
    int64_t acc_all = 0;
    if (ctx->rrt.root_blocked) {  // nothing is ever inserted: the tree is fixed, every verdict false
        const size_t n_before = (size_t)ctx->rrt.n;
        std::vector<double> tx, ty;  // the fixed tree, read once
        if (yaw && k > 0) {
            tx.resize(n_before);
            ty.resize(n_before);
            PP_HIP(hipMemcpy(tx.data(), ctx->rrt.X.p, n_before * sizeof(double), hipMemcpyDeviceToHost));
            PP_HIP(hipMemcpy(ty.data(), ctx->rrt.Y.p, n_before * sizeof(double), hipMemcpyDeviceToHost));
        }
        std::vector<int32_t> idx;
        for (int64_t b = 0; b < k && (nearest || yaw); b += kHostChunk) {
            const int nb = (int)std::min(kHostChunk, k - b);
            idx.resize((size_t)nb);
            if ((r = nearest_batch(ctx, sx + b, sy + b, nb, idx.data(), nullptr, eps))) return r;
            for (int i = 0; i < nb; ++i) {
                if (nearest) nearest[b + i] = idx[(size_t)i];
                if (yaw) yaw[b + i] = std::atan2(ty[(size_t)idx[i]] - sy[b + i], tx[(size_t)idx[i]] - sx[b + i]);
            }
        }
        if (ok) std::memset(ok, 0, (size_t)k);
        if ((r = rrt_extend_impl(ctx, k, nullptr, nullptr, eps))) return r;
        if (n_accepted) *n_accepted = 0;
        return PP_OK;
    }
    for (int64_t b = 0; b < k; b += kHostChunk) {
        const int64_t nb = std::min(kHostChunk, k - b);
        const size_t z = (size_t)nb;
        PP_HIP(ctx->rrt.hs_x.reserve(z));
        PP_HIP(ctx->rrt.hs_y.reserve(z));
        if (nearest) PP_HIP(ctx->rrt.hs_par.reserve(z));
        if (yaw) PP_HIP(ctx->rrt.hs_yaw.reserve(z));
        if (ok) PP_HIP(ctx->rrt.hs_ok.reserve(z));
        hipStream_t st = ctx->stream;
        PP_HIP(hipMemcpyAsync(ctx->rrt.hs_x.p, sx + b, z * sizeof(double), hipMemcpyHostToDevice, st));
        PP_HIP(hipMemcpyAsync(ctx->rrt.hs_y.p, sy + b, z * sizeof(double), hipMemcpyHostToDevice, st));
        SampleSrc src{ctx->rrt.hs_x.p, ctx->rrt.hs_y.p,
                      SampleRec{ctx->rrt.it, nearest ? ctx->rrt.hs_par.p : nullptr,
                                yaw ? ctx->rrt.hs_yaw.p : nullptr, ok ? ctx->rrt.hs_ok.p : nullptr},
                      !nearest && !yaw};
        int64_t acc = 0;
        if ((r = rrt_extend_impl(ctx, nb, &acc, &src, eps))) return r;
        acc_all += acc;
        if (nearest)
            PP_HIP(hipMemcpyAsync(nearest + b, ctx->rrt.hs_par.p, z * sizeof(int), hipMemcpyDeviceToHost, st));
        if (yaw) PP_HIP(hipMemcpyAsync(yaw + b, ctx->rrt.hs_yaw.p, z * sizeof(double), hipMemcpyDeviceToHost, st));
        if (ok) PP_HIP(hipMemcpyAsync(ok + b, ctx->rrt.hs_ok.p, z, hipMemcpyDeviceToHost, st));
        PP_HIP(hipStreamSynchronize(st));
    }
    if (n_accepted) *n_accepted = acc_all;
    return PP_OK;
}

int pp_rrt_tree_import(pp_ctx* ctx, const double* x, const double* y, const double* yaw,
                       const int32_t* parent, int64_t n) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (n < 1 || !x || !y || !yaw || !parent)
        return set_err(PP_ERR_INVALID_ARGUMENT, "a tree has at least its root");
    if (n > (int64_t)0x7fff0000) return set_err(PP_ERR_CAPACITY, "tree larger than 2^31 nodes");
    if (parent[0] != -1) return set_err(PP_ERR_INVALID_ARGUMENT, "node 0 must be the root (parent -1)");
    double mx = std::max({std::fabs(ctx->scene.minx), std::fabs(ctx->scene.maxx), std::fabs(ctx->scene.miny),
                          std::fabs(ctx->scene.maxy)});
    for (int64_t i = 0; i < n; ++i) {
        if (i > 0 && (parent[i] < 0 || parent[i] >= i))
            return set_err(PP_ERR_INVALID_ARGUMENT,
                           "parent[i] must be an earlier node (insertion order, rrt.rs:586-589)");
        if (!std::isfinite(x[i]) || !std::isfinite(y[i]) || !std::isfinite(yaw[i]))
            return set_err(PP_ERR_INVALID_ARGUMENT, "a node coordinate is not finite");
        mx = std::max({mx, std::fabs(x[i]), std::fabs(y[i])});
    }
    if (mx > PP_COORD_MAX) return set_err(PP_ERR_INVALID_ARGUMENT, "a node exceeds PP_COORD_MAX");
    PP_HIP(hipStreamSynchronize(ctx->stream));
    if ((r = ensure_tree(ctx, n + 1024))) return r;
    if ((r = upload_tree(ctx, x, y, yaw, parent, (size_t)n))) return r;
    // the planner continues from this tree: its iteration counter and statistics stay
    DevState& s = ctx->rrt.h_state.p[0];
    PP_HIP(hipMemcpy(&s, ctx->rrt.d_state.p, sizeof(DevState), hipMemcpyDeviceToHost));
    s.n = (int)n;
    s.n_scan = (int)n;
    s.it_spec = s.it;
    s.void_seq = -1;
    s.kdyn = kMinDynWindow;
    PP_HIP(hipMemcpy(ctx->rrt.d_state.p, &s, sizeof(DevState), hipMemcpyHostToDevice));
    ctx->rrt.n = n;
    ctx->rrt.start[0] = x[0];
    ctx->rrt.start[1] = y[0];
    ctx->rrt.start[2] = yaw[0];
    ctx->rrt.eps_coord = mx * std::ldexp(1.0, -23);
    ctx->rrt.root_blocked = ctx->scene.polygons() && !ctx->scene.point_ok(x[0], y[0]);
    return PP_OK;
}

int pp_rrt_plan_one(pp_ctx* ctx, int32_t* accepted) {
    int64_t acc = 0;
    int r = pp_rrt_extend(ctx, 1, &acc);
    if (r) return r;
    if (accepted) *accepted = (int32_t)acc;
    return PP_OK;
}

int pp_rrt_tree_size(pp_ctx* ctx, int64_t* n) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (!n) return set_err(PP_ERR_INVALID_ARGUMENT, "null output");
    *n = ctx->rrt.n;
    return PP_OK;
}

int pp_rrt_iteration(pp_ctx* ctx, int64_t* it) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (!it) return set_err(PP_ERR_INVALID_ARGUMENT, "null output");
    *it = ctx->rrt.it;
    return PP_OK;
}

int pp_rrt_tree_export(pp_ctx* ctx, double* x, double* y, double* yaw, int32_t* parent,
                       int64_t cap, int64_t* n) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (n) *n = ctx->rrt.n;
    if (cap < ctx->rrt.n) return set_err(PP_ERR_CAPACITY, "export buffer smaller than the tree");
    const size_t k = (size_t)ctx->rrt.n;
    hipStream_t st = ctx->stream;
    if (x) PP_HIP(hipMemcpyAsync(x, ctx->rrt.X.p, k * sizeof(double), hipMemcpyDeviceToHost, st));
    if (y) PP_HIP(hipMemcpyAsync(y, ctx->rrt.Y.p, k * sizeof(double), hipMemcpyDeviceToHost, st));
    if (yaw) PP_HIP(hipMemcpyAsync(yaw, ctx->rrt.YAW.p, k * sizeof(double), hipMemcpyDeviceToHost, st));
    if (parent) PP_HIP(hipMemcpyAsync(parent, ctx->rrt.PAR.p, k * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

int pp_rrt_line_to_origin(pp_ctx* ctx, int32_t node, double* x, double* y, int64_t cap,
                          int64_t* n) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (!n || node < 0 || node >= ctx->rrt.n || cap < 0 || (cap > 0 && (!x || !y)))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad line_to_origin arguments");
    // the path node -> root (NodeIter, rrt.rs:248-265): the tree's rows, read once
    const size_t nt = (size_t)ctx->rrt.n;
    std::vector<double> hx(nt), hy(nt), hyaw(nt);
    std::vector<int> hp(nt);
    hipStream_t st = ctx->stream;
    PP_HIP(hipMemcpyAsync(hx.data(), ctx->rrt.X.p, nt * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(hy.data(), ctx->rrt.Y.p, nt * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(hyaw.data(), ctx->rrt.YAW.p, nt * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(hp.data(), ctx->rrt.PAR.p, nt * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    std::vector<int> path;
    for (int v = node; v >= 0; v = hp[(size_t)v]) {
        if (path.size() > nt) return set_err(PP_ERR_STATE, "parent cycle in the tree");
        path.push_back(v);
    }
    // every edge child -> parent as dubins_path_planning(child pose, parent pose, R, step) on the
    // GPU (rrt.rs:297-311); the capacity bound of pp_dubins_path_planning_batch's callers
    const int ne = (int)path.size() - 1;
    std::vector<pp_dubins_config> conf((size_t)std::max(ne, 1));
    int pcap = 16;
    for (int e = 0; e < ne; ++e) {
        const int c = path[(size_t)e], p = path[(size_t)e + 1];
        conf[(size_t)e] = pp_dubins_config{hx[(size_t)c], hy[(size_t)c], hyaw[(size_t)c],
                                           hx[(size_t)p], hy[(size_t)p], hyaw[(size_t)p],
                                           ctx->scene.max_steer, ctx->rrt.step};
        const double d = std::hypot(hx[(size_t)p] - hx[(size_t)c], hy[(size_t)p] - hy[(size_t)c]);
        pcap = std::max(pcap, (int)((6.0 * 3.14159265358979323846 + d / ctx->scene.max_steer + 4.0) /
                                    ctx->rrt.step) + 16);
    }
    std::vector<double> px, py, pyaw, cost((size_t)std::max(ne, 1));
    std::vector<int32_t> np((size_t)std::max(ne, 1)), word((size_t)std::max(ne, 1));
    if (ne > 0) {
        px.resize((size_t)ne * pcap);
        py.resize((size_t)ne * pcap);
        pyaw.resize((size_t)ne * pcap);
        if ((r = pp_dubins_path_planning_batch(ctx, conf.data(), ne, pcap, px.data(), py.data(),
                                               pyaw.data(), np.data(), word.data(), cost.data())))
            return r;
    }
    int64_t w = 0;
    auto put = [&](double a, double b) {
        if (w < cap) {
            x[w] = a;
            y[w] = b;
        }
        ++w;
    };
    for (int e = 0; e < ne; ++e) {
        if (word[(size_t)e] < 0) {  // None: the child's own point (rrt.rs:313)
            put(hx[(size_t)path[(size_t)e]], hy[(size_t)path[(size_t)e]]);
            continue;
        }
        for (int k = 0; k < np[(size_t)e]; ++k) put(px[(size_t)e * pcap + k], py[(size_t)e * pcap + k]);
    }
    put(hx[(size_t)path.back()], hy[(size_t)path.back()]);  // the root (rrt.rs:316)
    *n = w;
    if (cap > 0 && w > cap) return set_err(PP_ERR_CAPACITY, "line buffer smaller than the line");
    return PP_OK;
}

int pp_rrt_get_nearest_node_batch(pp_ctx* ctx, const double* qx, const double* qy, int k,
                                  int32_t* idx, double* d2) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (k < 0 || (k > 0 && (!qx || !qy || !idx))) return set_err(PP_ERR_INVALID_ARGUMENT, "bad arguments");
    if ((r = check_coords(qx, k, 1, "query points")) || (r = check_coords(qy, k, 1, "query points")))
        return r;
    double mx = 0.0;
    for (int i = 0; i < k; ++i) mx = std::max({mx, std::fabs(qx[i]), std::fabs(qy[i])});
    return nearest_batch(ctx, qx, qy, k, idx, d2,
                         std::max(ctx->rrt.eps_coord, mx * std::ldexp(1.0, -23)));
}

int pp_rrt_verify_node_batch(pp_ctx* ctx, const double* x, const double* y,
                             const int32_t* parent, int k, uint8_t* ok, double* yaw) {
    int r = check_ctx(ctx, true, true);
    if (r) return r;
    if (k < 0 || (k > 0 && (!x || !y || !parent || !ok))) return set_err(PP_ERR_INVALID_ARGUMENT, "bad arguments");
    for (int i = 0; i < k; ++i)
        if (parent[i] < 0 || parent[i] >= ctx->rrt.n)
            return set_err(PP_ERR_INVALID_ARGUMENT, "parent index outside the tree");
    if ((r = check_coords(x, k, 1, "candidates")) || (r = check_coords(y, k, 1, "candidates")))
        return r;
    hipStream_t st = ctx->stream;
    const SceneDev sc = ctx->scene_dev();
    const TreeDev tr = ctx->rrt.tree_dev();
    std::vector<int> status(ctx->rrt.Kcap);
    for (int b = 0; b < k; b += ctx->rrt.Kcap) {
        const int nb = std::min(ctx->rrt.Kcap, k - b);
        for (int pass = 0; pass < 2; ++pass) {
            int nt = 0;
            std::vector<int> which;
            for (int i = 0; i < nb; ++i) {
                if (pass == 1 && status[i] != kLiteral) continue;
                SteerTask tk;
                tk.x = x[b + i];
                tk.y = y[b + i];
                tk.px = tk.py = tk.pyaw = 0.0;
                tk.pnode = parent[b + i];
                tk.literal = pass;
                ctx->rrt.h_tasks.p[nt++] = tk;
                which.push_back(i);
            }
            if (nt == 0) break;
            if (pass == 1)
                PP_HIP(ctx->api_lit_scratch.reserve((size_t)kLiteralWaves * 3 * kLiteralCap));
            std::vector<int> stv(nt);
            std::vector<double> yv(nt);
            PP_HIP(hipMemcpyAsync(ctx->rrt.tasks.p, ctx->rrt.h_tasks.p, nt * sizeof(SteerTask), hipMemcpyHostToDevice, st));
            PP_HIP(launch_steer_tasks(st, sc, tr, ctx->rrt.tasks.p, nt, ctx->rrt.task_status.p,
                                      ctx->rrt.task_yaw.p, pass ? ctx->api_lit_scratch.p : nullptr));
            PP_HIP(hipMemcpyAsync(stv.data(), ctx->rrt.task_status.p, nt * sizeof(int), hipMemcpyDeviceToHost, st));
            PP_HIP(hipMemcpyAsync(yv.data(), ctx->rrt.task_yaw.p, nt * sizeof(double), hipMemcpyDeviceToHost, st));
            PP_HIP(hipStreamSynchronize(st));
            for (int t = 0; t < nt; ++t) {
                const int i = which[t];
                if (stv[t] == kError)
                    return set_err(PP_ERR_STEER_OVERFLOW, "generate_local_course would index past n_point");
                status[i] = stv[t];
                ok[b + i] = stv[t] == kAccept && !ctx->rrt.root_blocked ? 1 : 0;
                if (yaw) yaw[b + i] = yv[t];
            }
        }
    }
    return PP_OK;
}

}  // extern "C"

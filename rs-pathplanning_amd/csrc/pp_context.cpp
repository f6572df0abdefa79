// pp_context.cpp — the context, errors, the stateless helpers and Dubins entry points, statistics
// and profiling of the C ABI (include/pathplanning_amd.h).
#include "pp_ctx.h"

using namespace ppamd;

namespace ppamd {

static thread_local std::string g_err;

int set_err(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int check_ctx(pp_ctx* c, bool need_scene, bool need_rrt) {
    if (!c) return set_err(PP_ERR_INVALID_ARGUMENT, "null context");
    if (need_scene && !c->scene.valid) return set_err(PP_ERR_STATE, "pp_space_new has not been called");
    if (need_rrt && !c->rrt.valid) return set_err(PP_ERR_STATE, "pp_rrt_new has not been called");
    PP_HIP(hipSetDevice(c->device));
    return PP_OK;
}

int check_coords(const double* v, int64_t n, int64_t stride, const char* what) {
    if (!v) return PP_OK;
    for (int64_t i = 0; i < n; ++i)
        if (!(std::fabs(v[i * stride]) <= PP_COORD_MAX))  // (NaN fails the comparison too)
            return set_err(PP_ERR_INVALID_ARGUMENT,
                           std::string(what) + ": a coordinate is not finite or exceeds PP_COORD_MAX (2^61)");
    return PP_OK;
}

int star_ready(pp_ctx* c) {
    int r = check_ctx(c, true, false);
    if (r) return r;
    if (!c->star.valid) return set_err(PP_ERR_STATE, "pp_star_new has not been called");
    return PP_OK;
}

int ensure_events(pp_ctx* c, size_t count) {
    PP_HIP(c->prof.ev.reserve(count));
    return PP_OK;
}

int ensure_literal_pool(pp_ctx* c, hipStream_t st) {
    PP_HIP(c->api_lit_scratch.reserve((size_t)kLiteralWaves * 3 * kLiteralCap));
    if (!c->lit_locks.p) {  // the pool's slot locks (zero: free)
        PP_HIP(c->lit_locks.reserve(kLiteralWaves));
        PP_HIP(hipMemsetAsync(c->lit_locks.p, 0, kLiteralWaves * sizeof(int), st));
    }
    return PP_OK;
}

}  // namespace ppamd

namespace {

using DubinsLauncher = hipError_t (*)(hipStream_t, const double*, int, int, double*, double*, double*,
                                      int*, int*, double*, int*);

// The two Dubins batch entry points after their argument checks: n configurations of `width`
// doubles each through `launch`, at most cap points per path
int dubins_batch(pp_ctx* ctx, const double* conf, int width, DubinsLauncher launch, int n, int cap,
                 double* px, double* py, double* pyaw, int32_t* n_points, int32_t* word,
                 double* cost) {
    const size_t nn = (size_t)n, tot = nn * (size_t)cap;
    DBuf<double> dconf, dpx, dpy, dpyaw, dcost;
    DBuf<int> dn, dword, dstat;
    PP_HIP(dconf.reserve(nn * width));
    PP_HIP(dpx.reserve(tot));
    PP_HIP(dpy.reserve(tot));
    PP_HIP(dpyaw.reserve(tot));
    PP_HIP(dcost.reserve(nn));
    PP_HIP(dn.reserve(nn));
    PP_HIP(dword.reserve(nn));
    PP_HIP(dstat.reserve(nn));
    hipStream_t st = ctx->stream;
    PP_HIP(hipMemcpyAsync(dconf.p, conf, nn * width * sizeof(double), hipMemcpyHostToDevice, st));
    PP_HIP(launch(st, dconf.p, n, cap, dpx.p, dpy.p, dpyaw.p, dn.p, dword.p, dcost.p, dstat.p));
    std::vector<int> stat(nn), nv(nn), wv(nn);
    PP_HIP(hipMemcpyAsync(px, dpx.p, tot * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(py, dpy.p, tot * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(pyaw, dpyaw.p, tot * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(cost, dcost.p, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(nv.data(), dn.p, nn * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(wv.data(), dword.p, nn * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(stat.data(), dstat.p, nn * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    bool overflow = false;
    for (size_t i = 0; i < nn; ++i) {
        if (stat[i] == kSteerOverflow) {
            overflow = true;
            word[i] = -2;
            n_points[i] = 0;
        } else if (stat[i] == kSteerNone) {
            word[i] = -1;
            n_points[i] = 0;
        } else {
            word[i] = wv[i];
            n_points[i] = nv[i];
        }
    }
    if (overflow) return set_err(PP_ERR_CAPACITY, "a configuration needs more than cap points");
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_abi_version(void) { return PP_ABI_VERSION; }

const char* pp_last_error(void) { return g_err.c_str(); }

int pp_device_count(int* n) {
    if (!n) return set_err(PP_ERR_INVALID_ARGUMENT, "null output");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return PP_OK;
}

int pp_coord_check(const double* x, const double* y, int64_t n) {
    if (n < 0) return set_err(PP_ERR_INVALID_ARGUMENT, "n < 0");
    int r = check_coords(x, n, 1, "x");
    return r ? r : check_coords(y, n, 1, "y");
}

int pp_create(int device, pp_ctx** out) {
    if (!out) return set_err(PP_ERR_INVALID_ARGUMENT, "null output");
    *out = nullptr;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
        return set_err(PP_ERR_NO_DEVICE, "no HIP device visible (the product path has no CPU fallback)");
    if (device < 0 || device >= cnt) return set_err(PP_ERR_INVALID_ARGUMENT, "device index out of range");
    PP_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    PP_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(PP_ERR_NO_DEVICE, std::string("built for gfx950, device is ") + prop.gcnArchName);
    pp_ctx* c = new pp_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = c->rrt.d_state.reserve(1);
    if (e == hipSuccess) e = c->rrt.d_api_state.reserve(1);
    if (e == hipSuccess) e = c->rrt.h_state.reserve(2);
    if (e != hipSuccess) {
        delete c;
        return set_err(PP_ERR_HIP, std::string("context setup: ") + hipGetErrorString(e));
    }
    *out = c;
    return PP_OK;
}

int pp_destroy(pp_ctx* ctx) {
    if (!ctx) return PP_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
    return PP_OK;
}

int pp_synchronize(pp_ctx* ctx) {
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    PP_HIP(hipStreamSynchronize(ctx->stream));
    return PP_OK;
}

uint64_t pp_rng_u64(uint64_t seed, uint64_t ctr) { return rng_u64(seed, ctr); }

double pp_gen_range(uint64_t seed, uint64_t ctr, double low, double high) {
    return gen_range(seed, ctr, low, high);
}

double pp_mod2pi(double theta) { return mod2pi(theta); }

double pp_pi_2_pi(double angle) { return pi_2_pi(angle); }

int pp_dubins_path_planning_batch(pp_ctx* ctx, const pp_dubins_config* confs, int n, int cap,
                                  double* px, double* py, double* pyaw, int32_t* n_points,
                                  int32_t* word, double* cost) {
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    if (n < 0 || cap <= 0 || (n > 0 && (!confs || !px || !py || !pyaw || !n_points || !word || !cost)))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad dubins batch arguments");
    if (n == 0) return PP_OK;
    for (int i = 0; i < n; ++i)
        if (!(confs[i].turn_radius > 0.0) || !(confs[i].step_size > 0.0))
            return set_err(PP_ERR_INVALID_ARGUMENT, "turn_radius and step_size must be > 0");
    static_assert(sizeof(pp_dubins_config) == 8 * sizeof(double), "DubinsConfig layout");
    for (int o : {0, 1, 3, 4})  // sx, sy, ex, ey
        if ((r = check_coords(reinterpret_cast<const double*>(confs) + o, n, 8, "dubins end points")))
            return r;
    return dubins_batch(ctx, reinterpret_cast<const double*>(confs), 8, launch_dubins_batch, n, cap,
                        px, py, pyaw, n_points, word, cost);
}

int pp_dubins_path_planning_from_origin_batch(pp_ctx* ctx, const double* conf5, int n, int cap,
                                              double* px, double* py, double* pyaw,
                                              int32_t* n_points, int32_t* word, double* cost) {
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    if (n < 0 || cap <= 0 || (n > 0 && (!conf5 || !px || !py || !pyaw || !n_points || !word || !cost)))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad dubins batch arguments");
    if (n == 0) return PP_OK;
    for (int i = 0; i < n; ++i)
        if (!(conf5[5 * i + 4] > 0.0))
            return set_err(PP_ERR_INVALID_ARGUMENT, "step_size must be > 0");
    for (int o : {0, 1})  // dx, dy
        if ((r = check_coords(conf5 + o, n, 5, "dubins end point"))) return r;
    return dubins_batch(ctx, conf5, 5, launch_dubins_origin, n, cap, px, py, pyaw, n_points, word,
                        cost);
}

int pp_dubins_words_batch(pp_ctx* ctx, const double* abd, int n, double* tpq, int32_t* ok) {
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    if (n < 0 || (n > 0 && (!abd || !tpq || !ok)))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad dubins words arguments");
    if (n == 0) return PP_OK;
    const size_t nn = (size_t)n;
    DBuf<double> dabd, dtpq;
    DBuf<int> dok;
    PP_HIP(dabd.reserve(3 * nn));
    PP_HIP(dtpq.reserve(18 * nn));
    PP_HIP(dok.reserve(6 * nn));
    hipStream_t st = ctx->stream;
    PP_HIP(hipMemcpyAsync(dabd.p, abd, 3 * nn * sizeof(double), hipMemcpyHostToDevice, st));
    PP_HIP(launch_dubins_words(st, dabd.p, n, dtpq.p, dok.p));
    static_assert(sizeof(int) == sizeof(int32_t), "ok words");
    PP_HIP(hipMemcpyAsync(tpq, dtpq.p, 18 * nn * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipMemcpyAsync(ok, dok.p, 6 * nn * sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

int pp_sincos_small_batch(pp_ctx* ctx, const double* x, int n, double* s, double* c,
                          double* s_ocml, double* c_ocml) {
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    if (n < 0 || (n > 0 && (!x || !s || !c || !s_ocml || !c_ocml)))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad sincos arguments");
    for (int i = 0; i < n; ++i)
        if (!(std::fabs(x[i]) < 0x1p30))
            return set_err(PP_ERR_INVALID_ARGUMENT, "sincos_small takes |x| < 2^30");
    if (n == 0) return PP_OK;
    const size_t nn = (size_t)n;
    DBuf<double> dx, dout;
    PP_HIP(dx.reserve(nn));
    PP_HIP(dout.reserve(4 * nn));
    hipStream_t st = ctx->stream;
    PP_HIP(hipMemcpyAsync(dx.p, x, nn * sizeof(double), hipMemcpyHostToDevice, st));
    PP_HIP(launch_sincos_small(st, dx.p, n, dout.p, dout.p + nn, dout.p + 2 * nn, dout.p + 3 * nn));
    double* out[4] = {s, c, s_ocml, c_ocml};
    for (int k = 0; k < 4; ++k)
        PP_HIP(hipMemcpyAsync(out[k], dout.p + k * nn, nn * sizeof(double), hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

int pp_rrt_get_stats(pp_ctx* ctx, pp_stats* out, uint64_t out_size) {
    if (!ctx || !out) return set_err(PP_ERR_INVALID_ARGUMENT, "null argument");
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    pp_stats s{};
    if (ctx->rrt.valid) {
        PP_HIP(hipMemcpyAsync(ctx->rrt.h_state.p, ctx->rrt.d_state.p, sizeof(DevState), hipMemcpyDeviceToHost, ctx->stream));
        PP_HIP(hipStreamSynchronize(ctx->stream));
        const DevState& d = ctx->rrt.h_state.p[0];
        s.iterations = d.iterations;
        s.accepted = d.accepted;
        s.windows = d.windows;
        s.truncations = d.truncations;
        s.repair_rounds = d.repair_rounds;
        s.repairs = d.repairs;
        s.literal_repairs = d.literal_repairs;
        s.nn_flagged = d.nn_flagged;
        s.node_evals = d.node_evals;
        s.samples_evaluated = d.iterations;
        s.samples_blocked = d.blocked;
    }
    s.nn_scan_ms = ctx->prof.nn_scan_ms;
    s.nn_scan_launches = ctx->prof.nn_scan_launches;
    s.steer_ms = ctx->prof.steer_ms;
    s.steer_launches = ctx->prof.steer_launches;
    s.finalize_ms = ctx->prof.finalize_ms;
    s.prep_ms = ctx->prof.prep_ms;
    s.insert_ms = ctx->prof.insert_ms;
    s.batch_steps = ctx->prof.batch_steps;
    s.batch_passes = ctx->prof.batch_passes;
    s.finish_ms = ctx->prof.finish_ms;
    s.finish_launches = ctx->prof.finish_launches;
    if (ctx->prof.wg_pts.p) {  // profiling: the walk workgroups' point tallies
        std::vector<long long> v(ctx->prof.wg_pts.n);
        PP_HIP(hipMemcpyAsync(v.data(), ctx->prof.wg_pts.p, v.size() * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        PP_HIP(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < v.size(); ++i) {
            const size_t k = i / (size_t)kWalkTallySlots;  // points, arc points, tasks
            (k == 0 ? s.walk_points : k == 1 ? s.walk_arc_points : s.walk_tasks) += v[i];
        }
    }
    if (ctx->prof.cf_tally.p) {
        long long t[4];
        PP_HIP(hipMemcpyAsync(t, ctx->prof.cf_tally.p, sizeof t, hipMemcpyDeviceToHost, ctx->stream));
        PP_HIP(hipStreamSynchronize(ctx->stream));
        // (+ the batch plan's steer rounds: their nodes, edges and walked points)
        s.finish_nodes = t[0] + ctx->prof.cfb_nodes;
        s.finish_edges = t[1] + ctx->prof.cfb_edges;
        s.finish_points = t[2] + ctx->prof.cfb_points;
        s.finish_arc_points = t[3] + ctx->prof.cfb_arc;
    }
    std::memcpy(out, &s, (size_t)std::min<uint64_t>(out_size, sizeof s));
    return PP_OK;
}

int pp_rrt_reset_stats(pp_ctx* ctx) {
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    if (ctx->rrt.valid) {
        PP_HIP(hipMemcpyAsync(ctx->rrt.h_state.p, ctx->rrt.d_state.p, sizeof(DevState), hipMemcpyDeviceToHost, ctx->stream));
        PP_HIP(hipStreamSynchronize(ctx->stream));
        DevState d = ctx->rrt.h_state.p[0];
        d.iterations = d.accepted = d.windows = d.truncations = d.repair_rounds = d.repairs =
            d.literal_repairs = d.nn_flagged = d.node_evals = d.blocked = 0;
        ctx->rrt.h_state.p[0] = d;
        PP_HIP(hipMemcpyAsync(ctx->rrt.d_state.p, ctx->rrt.h_state.p, sizeof(DevState), hipMemcpyHostToDevice, ctx->stream));
        PP_HIP(hipStreamSynchronize(ctx->stream));
    }
    if ((r = ctx->prof.reset_host_stats(ctx->stream))) return set_err(r, "resetting the statistics");
    return PP_OK;
}

int pp_set_profiling(pp_ctx* ctx, int enabled) {
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    if (enabled && !ctx->prof.wg_pts.p) {  // one tally slot per walk workgroup (any walk grid)
        PP_HIP(ctx->prof.wg_pts.reserve(3 * kWalkTallySlots));
        PP_HIP(hipMemsetAsync(ctx->prof.wg_pts.p, 0, 3 * kWalkTallySlots * sizeof(long long), ctx->stream));
        PP_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (enabled && !ctx->prof.cf_tally.p) {
        PP_HIP(ctx->prof.cf_tally.reserve(4));
        PP_HIP(hipMemsetAsync(ctx->prof.cf_tally.p, 0, 4 * sizeof(long long), ctx->stream));
        PP_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->prof.on = enabled != 0;
    return PP_OK;
}

}  // extern "C"

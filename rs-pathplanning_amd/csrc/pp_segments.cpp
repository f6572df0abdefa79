// pp_segments.cpp — planned paths as Dubins segments (pp_star_path_segments,
// pp_batch_path_segments; over caller-supplied chains: pp_star_chain_segments) and their sampling
// into trajectories (pp_segments_sample).  The chains,
// items, counts, scan and sizes-only protocol are the packed line exports' (pp_finish.cpp,
// pp_star_goal.cpp); the kernels are pp_k_segments.hip.  DESIGN.md §3.7 "Segment export and
// sampling".
#include <cstddef>

#include "pp_ctx.h"

using namespace ppamd;

namespace {

// the export's waves: tier 1 runs every item with a kSegPath1-deep ancestor path (512 KB in all;
// config 5's chains are ~20 deep), the few deeper chains go through the spill list to tier 2 at
// the full depth (2 MB)
constexpr int kSegGrid = 2048;
constexpr int kSegPath1 = 64;
constexpr int kSegGrid2 = 64;

// the five arrays of a pp_path_segments as the caller compiled it (a field past `size`: NULL)
struct SegPtrs {
    double *x = nullptr, *y = nullptr, *yaw = nullptr, *kappa = nullptr, *len = nullptr;
};
SegPtrs seg_ptrs(const pp_path_segments* s) {
    SegPtrs p;
    if (!s) return p;
    const uint64_t sz = s->size;
    auto has = [&](size_t offset) { return offset + sizeof(double*) <= sz; };
    if (has(offsetof(pp_path_segments, x))) p.x = s->x;
    if (has(offsetof(pp_path_segments, y))) p.y = s->y;
    if (has(offsetof(pp_path_segments, yaw))) p.yaw = s->yaw;
    if (has(offsetof(pp_path_segments, kappa))) p.kappa = s->kappa;
    if (has(offsetof(pp_path_segments, len))) p.len = s->len;
    return p;
}

bool finite3(const double* g) {
    return std::fabs(g[0]) <= PP_COORD_MAX && std::fabs(g[1]) <= PP_COORD_MAX && std::isfinite(g[2]);
}

struct SegTiers {
    int grid1 = 0, grid2 = 0;
    int* path2 = nullptr;
};

// the ancestor paths of both tiers and the spill list (its count zeroed on the stream)
int seg_buffers(pp_ctx* c, int k, SegArgs& a, SegTiers& t) {
    SegExport& se = c->seg;
    t.grid1 = std::min(kSegGrid, k);
    t.grid2 = std::min(kSegGrid2, k);
    PP_HIP(se.path.reserve((size_t)t.grid1 * kSegPath1 + (size_t)t.grid2 * kCfMaxDepth));
    PP_HIP(se.spill.reserve(1 + (size_t)k * kCfItem));
    PP_HIP(hipMemsetAsync(se.spill.p, 0, sizeof(int), c->stream));
    a.path = se.path.p;
    a.path_cap = kSegPath1;
    a.spill = se.spill.p;
    a.spill_cap = k;
    t.path2 = se.path.p + (size_t)t.grid1 * kSegPath1;
    return PP_OK;
}

// one pass over `items` (at most k of them): tier 1, then its spill list at the full depth
int seg_launch(pp_ctx* c, SegArgs a, const int* items, int k, bool star, bool write) {
    SegTiers t;
    if (int r = seg_buffers(c, k, a, t)) return r;
    PP_HIP(launch_segments(c->stream, a, t.grid1, c->cf.err.p, items, k, star, write));
    SegArgs a2 = a;
    a2.path = t.path2;
    a2.path_cap = kCfMaxDepth;
    a2.spill = nullptr;
    a2.spill_cap = 0;
    PP_HIP(launch_segments(c->stream, a2, t.grid2, c->cf.err.p, a.spill, k, star, write));
    return PP_OK;
}

int seg_error(int err) {
    if (err & 2) return set_err(PP_ERR_REFERENCE_PANIC, "an edge of a chain has no Dubins word");
    if (err & 1) return set_err(PP_ERR_CAPACITY, "tree deeper than the path capacity");
    if (err & 16) return set_err(PP_ERR_STATE, "segment export: a row's size changed between the passes");
    return PP_OK;
}

// The rows' offsets from paths.cnt / ok by the scan, to the caller, and the capacity check; the
// kernels' error word arrives with them (one synchronisation).  *go: the caller wants the
// segments and there are some.
int seg_sizes(pp_ctx* c, int Q, int64_t* off, bool want, int64_t cap, int64_t* n_total,
              uint8_t* ok, bool* go) {
    PathExport& pe = c->paths;
    hipStream_t st = c->stream;
    *go = false;
    int err = 0;
    PP_HIP(hipMemcpyAsync(&err, c->cf.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PP_HIP(launch_paths_scan(st, Q, pe.slot.p, pe.ok.p, pe.cnt.p, pe.off.p, pe.okq.p));
    PP_HIP(hipMemcpyAsync(off, pe.off.p, ((size_t)Q + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (ok) PP_HIP(hipMemcpyAsync(ok, pe.okq.p, Q, hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    if (int r = seg_error(err)) return r;
    const int64_t total = off[Q];
    *n_total = total;
    if (!want || cap <= 0 || total == 0) return PP_OK;  // the sizes only
    if (cap < total) return set_err(PP_ERR_CAPACITY, "the segment arrays are smaller than the rows' total (n_total)");
    *go = true;
    return PP_OK;
}

// the write pass into the staging rows, their copies to the caller's arrays and the rows' lengths
// (the sum of a row's len in row order, on the host: the rows are a few dozen segments)
int seg_write(pp_ctx* c, SegArgs a, const int* items, int k, bool star, int Q, const int64_t* off,
              const SegPtrs& out, double* length) {
    SegExport& se = c->seg;
    hipStream_t st = c->stream;
    const size_t total = (size_t)off[Q];
    for (auto* b : {&se.x, &se.y, &se.yaw, &se.kappa, &se.len}) PP_HIP(b->reserve(total));
    a.off = c->paths.off.p;
    a.ox = out.x ? se.x.p : nullptr;
    a.oy = out.y ? se.y.p : nullptr;
    a.oyaw = out.yaw ? se.yaw.p : nullptr;
    a.okappa = out.kappa ? se.kappa.p : nullptr;
    a.olen = (out.len || length) ? se.len.p : nullptr;
    PP_HIP(hipMemsetAsync(c->cf.err.p, 0, 2 * sizeof(int), st));
    if (int r = seg_launch(c, a, items, k, star, true)) return r;
    int err = 0;
    PP_HIP(hipMemcpyAsync(&err, c->cf.err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    const size_t bytes = total * sizeof(double);
    if (out.x) PP_HIP(hipMemcpyAsync(out.x, se.x.p, bytes, hipMemcpyDeviceToHost, st));
    if (out.y) PP_HIP(hipMemcpyAsync(out.y, se.y.p, bytes, hipMemcpyDeviceToHost, st));
    if (out.yaw) PP_HIP(hipMemcpyAsync(out.yaw, se.yaw.p, bytes, hipMemcpyDeviceToHost, st));
    if (out.kappa) PP_HIP(hipMemcpyAsync(out.kappa, se.kappa.p, bytes, hipMemcpyDeviceToHost, st));
    std::vector<double> hl;
    const double* lens = out.len;
    if (out.len) {
        PP_HIP(hipMemcpyAsync(out.len, se.len.p, bytes, hipMemcpyDeviceToHost, st));
    } else if (length) {
        hl.resize(total);
        PP_HIP(hipMemcpyAsync(hl.data(), se.len.p, bytes, hipMemcpyDeviceToHost, st));
        lens = hl.data();
    }
    PP_HIP(hipStreamSynchronize(st));
    if (int r = seg_error(err)) return r;
    for (int q = 0; length && q < Q; ++q) {
        double sum = 0.0;
        for (int64_t j = off[q]; j < off[q + 1]; ++j) sum += lens[j];
        length[q] = sum;
    }
    return PP_OK;
}

void seg_empty(int Q, int64_t* off, int64_t* n_total, double* length, uint8_t* ok) {
    *n_total = 0;
    std::fill(off, off + Q + 1, (int64_t)0);
    if (length) std::fill(length, length + Q, 0.0);
    if (ok) std::fill(ok, ok + Q, (uint8_t)0);
}

}  // namespace

extern "C" {

int pp_star_path_segments(pp_ctx* ctx, const double* goals, const int32_t* nodes, int reverse,
                          int64_t* off, const pp_path_segments* seg, int64_t cap,
                          int64_t* n_total, double* length, uint8_t* ok) {
    int r = star_ready(ctx);
    if (r) return r;
    StarBatch& s = ctx->star;
    if (!goals || !nodes || !off || !n_total)
        return set_err(PP_ERR_INVALID_ARGUMENT, "null goals, nodes, off or n_total");
    if (reverse != 0 && reverse != 1) return set_err(PP_ERR_INVALID_ARGUMENT, "reverse is 0 or 1");
    const int Q = s.f.Q;
    for (int q = 0; q < Q; ++q)
        if (!finite3(goals + 3 * (size_t)q)) return set_err(PP_ERR_INVALID_ARGUMENT, "non-finite goal");
    hipStream_t st = ctx->stream;
    PathExport& pe = ctx->paths;
    int k = 0;
    if ((r = paths_items(ctx, s.f, nodes, &k))) return r;
    seg_empty(Q, off, n_total, length, ok);
    if (k == 0) return PP_OK;
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
    SegArgs a;
    a.tr = s.f.tree_dev();
    a.row_cap = s.f.cap;
    a.qidx = pe.qidx.p;
    a.nodes = pe.nodes.p;
    a.goals = s.goal_d.p;
    a.turn_radius = ctx->scene.max_steer;
    a.reverse = reverse;
    a.cnt = pe.cnt.p;
    a.okf = pe.ok.p;
    // the count pass: every item's edges (and whether its goal edge has a word)
    if ((r = seg_launch(ctx, a, pe.items.p, k, true, false))) return r;
    const SegPtrs out = seg_ptrs(seg);
    bool go = false;
    if ((r = seg_sizes(ctx, Q, off, seg != nullptr, cap, n_total, ok, &go)) || !go) return r;
    return seg_write(ctx, a, pe.items.p, k, true, Q, off, out, length);
}

int pp_star_chain_segments(pp_ctx* ctx, const double* goals, const int64_t* coff,
                           const int32_t* chain, int reverse, int64_t* off,
                           const pp_path_segments* seg, int64_t cap, int64_t* n_total,
                           double* length, uint8_t* ok) {
    int r = star_ready(ctx);
    if (r) return r;
    StarBatch& s = ctx->star;
    if (!goals || !coff || !off || !n_total)
        return set_err(PP_ERR_INVALID_ARGUMENT, "null goals, coff, off or n_total");
    if (reverse != 0 && reverse != 1) return set_err(PP_ERR_INVALID_ARGUMENT, "reverse is 0 or 1");
    const int Q = s.f.Q;
    for (int q = 0; q < Q; ++q)
        if (!finite3(goals + 3 * (size_t)q)) return set_err(PP_ERR_INVALID_ARGUMENT, "non-finite goal");
    if (coff[0] != 0) return set_err(PP_ERR_INVALID_ARGUMENT, "coff[0] must be 0");
    for (int q = 0; q < Q; ++q)
        if (coff[q + 1] < coff[q]) return set_err(PP_ERR_INVALID_ARGUMENT, "coff must not decrease");
    const int64_t nc = coff[Q];
    if (nc > 0 && !chain) return set_err(PP_ERR_INVALID_ARGUMENT, "null chain");
    hipStream_t st = ctx->stream;
    // the chains against the trees as they are: every entry a node of its tree, the root last
    std::vector<int> hn;
    if ((r = s.f.sizes(ctx, &hn))) return r;
    std::vector<int32_t> nodes((size_t)Q, -1);
    for (int q = 0; q < Q; ++q) {
        const int64_t c0 = coff[q], c1 = coff[q + 1];
        if (c1 == c0) continue;
        if (c1 - c0 > kCfMaxDepth) return set_err(PP_ERR_INVALID_ARGUMENT, "a chain row longer than 8192 nodes");
        for (int64_t e = c0; e < c1; ++e)
            if (chain[e] < 0 || chain[e] >= hn[(size_t)q])
                return set_err(PP_ERR_INVALID_ARGUMENT, "chain entry outside its query's tree");
        if (chain[c1 - 1] != 0) return set_err(PP_ERR_INVALID_ARGUMENT, "a chain row must end in node 0 (the root)");
        nodes[(size_t)q] = chain[c0];
    }
    PathExport& pe = ctx->paths;
    int k = 0;
    if ((r = paths_items(ctx, s.f, nodes.data(), &k))) return r;
    seg_empty(Q, off, n_total, length, ok);
    if (k == 0) return PP_OK;
    Shortcut& sc = ctx->shortcut;
    PP_HIP(sc.cchain.reserve((size_t)nc));
    PP_HIP(sc.coff.reserve((size_t)Q + 1));
    std::vector<int> items(1 + (size_t)k * kCfItem, 0);
    items[0] = k;
    for (int b = 0; b < k; ++b) items[1 + (size_t)b * kCfItem] = b;
    PP_HIP(pe.items.reserve(items.size()));
    PP_HIP(s.goal_d.reserve(3 * (size_t)Q));
    PP_HIP(hipMemcpyAsync(sc.cchain.p, chain, (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(sc.coff.p, coff, ((size_t)Q + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(pe.items.p, items.data(), items.size() * sizeof(int), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(s.goal_d.p, goals, 3 * (size_t)Q * sizeof(double), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemsetAsync(pe.cnt.p, 0, (size_t)k * sizeof(int), st));
    PP_HIP(hipMemsetAsync(pe.ok.p, 0, (size_t)k * sizeof(int), st));
    PP_HIP(ctx->cf.err.reserve(2));
    PP_HIP(hipMemsetAsync(ctx->cf.err.p, 0, 2 * sizeof(int), st));
    SegArgs a;
    a.tr = s.f.tree_dev();
    a.row_cap = s.f.cap;
    a.qidx = pe.qidx.p;
    a.nodes = pe.nodes.p;
    a.goals = s.goal_d.p;
    a.turn_radius = ctx->scene.max_steer;
    a.reverse = reverse;
    a.cnt = pe.cnt.p;
    a.okf = pe.ok.p;
    a.cchain = sc.cchain.p;
    a.coff = sc.coff.p;
    if ((r = seg_launch(ctx, a, pe.items.p, k, true, false))) return r;
    const SegPtrs out = seg_ptrs(seg);
    bool go = false;
    if ((r = seg_sizes(ctx, Q, off, seg != nullptr, cap, n_total, ok, &go)) || !go) return r;
    return seg_write(ctx, a, pe.items.p, k, true, Q, off, out, length);
}

int pp_batch_path_segments(pp_ctx* ctx, const int32_t* nodes, int reverse, int64_t* off,
                           const pp_path_segments* seg, int64_t cap, int64_t* n_total,
                           double* length, uint8_t* ok) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    Batch& b = ctx->batch;
    if (!b.valid) return set_err(PP_ERR_STATE, "pp_batch_new has not been called");
    if (!nodes || !off || !n_total) return set_err(PP_ERR_INVALID_ARGUMENT, "null nodes, off or n_total");
    if (reverse != 0 && reverse != 1) return set_err(PP_ERR_INVALID_ARGUMENT, "reverse is 0 or 1");
    const int Q = b.f.Q;
    hipStream_t st = ctx->stream;
    PathExport& pe = ctx->paths;
    int k = 0;
    if ((r = paths_items(ctx, b.f, nodes, &k))) return r;
    seg_empty(Q, off, n_total, length, ok);
    if (k == 0) return PP_OK;
    // check_finish of the k items, as pp_batch_paths runs it: the verdicts (paths.ok) and a line
    // item with its optimize chain per verified finish (cf.items)
    if ((r = paths_batch_finish(ctx, k))) return r;
    PP_HIP(hipMemsetAsync(pe.cnt.p, 0, (size_t)k * sizeof(int), st));
    PP_HIP(hipMemsetAsync(ctx->cf.err.p, 0, 2 * sizeof(int), st));
    SegArgs a;
    a.tr = b.f.tree_dev();
    a.row_cap = b.f.cap;
    a.qidx = pe.qidx.p;
    a.nodes = pe.nodes.p;
    a.goals = b.goal_d.p;
    a.turn_radius = ctx->scene.max_steer;
    a.reverse = reverse;
    a.cnt = pe.cnt.p;  // (the line pass's point counts give way to the segment counts)
    if ((r = seg_launch(ctx, a, ctx->cf.items.p, k, false, false))) return r;
    const SegPtrs out = seg_ptrs(seg);
    bool go = false;
    if ((r = seg_sizes(ctx, Q, off, seg != nullptr, cap, n_total, ok, &go)) || !go) return r;
    return seg_write(ctx, a, ctx->cf.items.p, k, false, Q, off, out, length);
}

int pp_segments_sample(pp_ctx* ctx, int q, const int64_t* off, const pp_path_segments* seg,
                       double ds, int64_t* poff, double* x, double* y, double* yaw, double* kappa,
                       double* s, int64_t cap, int64_t* n_total) {
    int r = check_ctx(ctx, false, false);
    if (r) return r;
    if (q < 0 || !off || !seg || !poff || !n_total)
        return set_err(PP_ERR_INVALID_ARGUMENT, "negative q or null off, seg, poff or n_total");
    if (!(std::isfinite(ds) && ds > 0.0)) return set_err(PP_ERR_INVALID_ARGUMENT, "ds must be finite and > 0");
    if (off[0] != 0) return set_err(PP_ERR_INVALID_ARGUMENT, "off[0] must be 0");
    for (int i = 0; i < q; ++i)
        if (off[i + 1] < off[i]) return set_err(PP_ERR_INVALID_ARGUMENT, "off must not decrease");
    const int64_t n = off[q];
    const SegPtrs in = seg_ptrs(seg);
    if (!in.x || !in.y || !in.yaw || !in.kappa || !in.len)
        return set_err(PP_ERR_INVALID_ARGUMENT, "the sampler needs all five segment arrays");
    for (int64_t j = 0; j < n; ++j) {
        if (!(std::isfinite(in.x[j]) && std::isfinite(in.y[j]) && std::isfinite(in.yaw[j]) &&
              std::isfinite(in.kappa[j])))
            return set_err(PP_ERR_INVALID_ARGUMENT, "non-finite segment");
        if (!(std::isfinite(in.len[j]) && in.len[j] >= 0.0))
            return set_err(PP_ERR_INVALID_ARGUMENT, "a segment's len must be finite and >= 0");
    }
    *n_total = 0;
    std::fill(poff, poff + q + 1, (int64_t)0);
    if (q == 0 || n == 0) return PP_OK;
    SegExport& se = ctx->seg;
    hipStream_t st = ctx->stream;
    for (auto* b : {&se.x, &se.y, &se.yaw, &se.kappa, &se.len, &se.P}) PP_HIP(b->reserve((size_t)n));
    for (auto* b : {&se.off, &se.poff}) PP_HIP(b->reserve((size_t)q + 1));
    for (auto* b : {&se.nfull, &se.cnt}) PP_HIP(b->reserve((size_t)q));
    PP_HIP(se.rowlen.reserve((size_t)q));
    // (pageable sources: the copies are complete when the calls return)
    const size_t bytes = (size_t)n * sizeof(double);
    PP_HIP(hipMemcpyAsync(se.off.p, off, ((size_t)q + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(se.x.p, in.x, bytes, hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(se.y.p, in.y, bytes, hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(se.yaw.p, in.yaw, bytes, hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(se.kappa.p, in.kappa, bytes, hipMemcpyHostToDevice, st));
    PP_HIP(hipMemcpyAsync(se.len.p, in.len, bytes, hipMemcpyHostToDevice, st));
    SegSampleArgs a;
    a.q = q;
    a.ds = ds;
    a.max_samples = kSegMaxSamples;
    a.off = se.off.p;
    a.x = se.x.p;
    a.y = se.y.p;
    a.yaw = se.yaw.p;
    a.kappa = se.kappa.p;
    a.len = se.len.p;
    a.P = se.P.p;
    a.rowlen = se.rowlen.p;
    a.nfull = se.nfull.p;
    a.cnt = se.cnt.p;
    PP_HIP(launch_segments_prefix(st, a));
    std::vector<int64_t> cnt((size_t)q);
    PP_HIP(hipMemcpyAsync(cnt.data(), se.cnt.p, (size_t)q * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    // the one host round trip before the samples: the staging and the capacity check need the total
    PP_HIP(hipStreamSynchronize(st));
    int64_t total = 0;
    bool over = false;
    for (int i = 0; i < q; ++i) {
        poff[i] = total;
        total += cnt[(size_t)i];
        over |= total > kSegMaxSamples;
        if (over) total = kSegMaxSamples + 1;  // (saturated: a row's count is clamped there too)
    }
    poff[q] = total;
    *n_total = total;
    if (over)
        return set_err(PP_ERR_CAPACITY, "more than 2^26 samples in one call: sample fewer rows or a larger ds");
    const bool want = x || y || yaw || kappa || s;
    if (!want || cap <= 0 || total == 0) return PP_OK;  // the sizes only
    if (cap < total) return set_err(PP_ERR_CAPACITY, "the sample arrays are smaller than the rows' total (n_total)");
    const size_t t = (size_t)total;
    if (x) PP_HIP(se.sx.reserve(t));
    if (y) PP_HIP(se.sy.reserve(t));
    if (yaw) PP_HIP(se.syaw.reserve(t));
    if (kappa) PP_HIP(se.skappa.reserve(t));
    if (s) PP_HIP(se.ss.reserve(t));
    PP_HIP(hipMemcpyAsync(se.poff.p, poff, ((size_t)q + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    a.poff = se.poff.p;
    a.total = total;
    a.sx = x ? se.sx.p : nullptr;
    a.sy = y ? se.sy.p : nullptr;
    a.syaw = yaw ? se.syaw.p : nullptr;
    a.skappa = kappa ? se.skappa.p : nullptr;
    a.ss = s ? se.ss.p : nullptr;
    PP_HIP(launch_segments_sample(st, a));
    const size_t ob = t * sizeof(double);
    if (x) PP_HIP(hipMemcpyAsync(x, se.sx.p, ob, hipMemcpyDeviceToHost, st));
    if (y) PP_HIP(hipMemcpyAsync(y, se.sy.p, ob, hipMemcpyDeviceToHost, st));
    if (yaw) PP_HIP(hipMemcpyAsync(yaw, se.syaw.p, ob, hipMemcpyDeviceToHost, st));
    if (kappa) PP_HIP(hipMemcpyAsync(kappa, se.skappa.p, ob, hipMemcpyDeviceToHost, st));
    if (s) PP_HIP(hipMemcpyAsync(s, se.ss.p, ob, hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

}  // extern "C"

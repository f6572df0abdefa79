// pp_k_window.hip — hand-written CDNA4 (gfx950) kernels of the RRT extend hot path.
//
// Window pipeline (one speculative window of up to K samples — the draws of up to 2 K iterations
// that are not in an obstacle, pp_window_fill.h — device-resident state):
//   window_samples Space::rand_point for the window's iterations (seeded stream), Morton-sorted
//                  (the first window of a batch; later ones come from nn_finalize) rrt.rs:139-146
//   window_kernel  workgroups 1..: the NN screen, K samples x N tree nodes, f32 SoA, expanded form
//                  about each sample block's centre, scalar-broadcast nodes, 4 samples per lane,
//                  exact per-chunk top-2, XCD-aware mapping                          rrt.rs:378-391
//                  workgroup 0: resolve + commit of the previous window (sequential-consistency
//                  replay, repairs inline, in-order insert)                          rrt.rs:414-426
//   nn_finalize    merge the chunk partials and the appended nodes, exact f64 d2 of the winner,
//                  near-ties decided exactly (wave, or workgroup brute force), window pairs
//                  (earlier samples nearer than the snapshot NN), next window's samples
//   steer_prep     8 lanes per (sample, parent): compute_yaw + Dubins word + grid-point distances
//   steer_walk     one wave per task: sampled-arc polyline, bounds + disc collision, f64
//                                                               rrt.rs:169-175,414-426, dubins.rs
// check_finish, the query batch and the RRT* batch with its goal connection are pp_k_finish.hip,
// pp_k_batch.hip and pp_k_star.hip.
// steer_prep, steer_walk and the API kernels (steer_tasks, verify_lines, dubins_*) are compiled by
// pp_k_steer.hip alone and launched through pp_steer_launch.h; the device code the units inline
// is pp_steer_dev.h.
//
// No MFMA anywhere: there is no dense contraction on this path.
#include <hip/hip_runtime.h>

#include "pp_kernels.h"
#include "pp_window_fill.h"
#include "pp_steer_dev.h"
#include "pp_steer_launch.h"

namespace ppamd {

typedef __attribute__((address_space(3))) void lds_void;  // LDS-DMA operands
typedef __attribute__((address_space(1))) void glb_void;

// ------------------------------------------------------------------------- window pipeline
//
// One speculative window w = window_kernel (w's NN screen ‖ resolve + commit of w - 1) →
// nn_finalize (+ window pairs, + w + 1's samples) → steer_prep → steer_walk; window w's resolve and commit
// run inside window w + 1's window_kernel (or the batch's drain launch).  Everything reads the
// device-resident DevState, so the host enqueues windows back to back and synchronises once per
// batch.

// (kQPL, kQPB, kScanWaves, kScanBlk, kScanGrid and the tiling itself: pp_screen_geom.h)
constexpr int kScanThreads = 512;                // window_kernel workgroup (8 waves, 256 VGPRs)
constexpr bool kWinRepair = true;                // repairs inside the window kernel (no spill)
static_assert(kScanWaves == kScanThreads / 64, "the tiling's waves per workgroup");
static_assert(kScreenBlocks * kQPB >= kMaxWindow, "the tiling's blocks cover a window");
// the screen's tiling and work list for every count of sample rows, built at compile time
__constant__ const ScreenTables kScreenTables = make_screen_tables();
constexpr int kStage = 7936;                     // chunk nodes staged in LDS per round
constexpr int kExactNode = 1 << 30;              // screen partial key: a node index, not a block
// LDS of a screen workgroup: the wave merge (best, second, key per wave and sample; sample ids;
// the samples' f32 operands), then the staged chunk
constexpr int kScreenStageOff = (3 * kScanWaves + 3) * kQPB * 4;

// the nearest API's node chunks for K given samples: nqb full sample blocks x chunks workgroups
// fill kScanGrid (the window's screen is tiled by screen_geom, from the samples it screens)
__host__ __device__ inline int scan_chunks(int K) {
    const int nqb = (K + kQPB - 1) / kQPB;
    int c = kScanGrid / nqb;
    if (c > kMaxChunks) c = kMaxChunks;
    return c < 1 ? 1 : c;
}

struct Top2 {
    float b, s;
    int i;
};
__device__ inline Top2 merge_top2(Top2 a, Top2 c) {
    Top2 r;
    float other;
    if (c.b < a.b || (c.b == a.b && c.i >= 0 && (a.i < 0 || c.i < a.i))) {
        r.b = c.b;
        r.i = c.i;
        other = a.b;
    } else {
        r.b = a.b;
        r.i = a.i;
        other = c.b;
    }
    r.s = fminf(fminf(a.s, c.s), other);
    return r;
}

__device__ __forceinline__ float scan_d2(float qx, float qy, float nx, float ny) {
    const float dx = qx - nx, dy = qy - ny;
    return __builtin_fmaf(dy, dy, dx * dx);
}

// window_samples: Space::rand_point for the iterations [start, start + span) of a window
// (rrt.rs:139-146, seeded: Q7 — x = draw 2*it, y = draw 2*it + 1).  The draws in an obstacle (the
// pre-test) are settled here and take no sample id: the window's W <= min(K, kdyn) samples are its
// live draws in iteration order, sample id drawn at iteration start + iter_off[id], and the window
// spans up to twice as many iterations (pp_window_fill.h).  Then
// a counting sort of the samples by the Morton index of their cell in a 16 x 16 grid over the
// sampling box: perm[pos] = sample, so a screen block of 256 consecutive sorted samples is
// spatially compact (the expanded screen's precision).  Within a cell the order is arbitrary —
// the results never depend on it (only which samples meet the exact rescan).
struct SamplesArgs {
    int K;
    int64_t target;
    uint64_t seed;
    double minx, maxx, miny, maxy;
    double* wsx[2];
    double* wsy[2];
    float* wsx32[2];
    float* wsy32[2];
    int* perm[2];
    int* cofs[2];     // [257] first sorted position of each Morton cell (cell 256: W)
    float2* sxy[2];   // sorted position -> (x, y) f32 (the pair search's prefilter)
    double* ssx[2];   // sorted position -> x, y (f64): the screen's coalesced sample loads
    double* ssy[2];
    float2* ob[2];    // [kScreenBlocks] the centre o (f32) of each screen block's sorted samples
    double* sq[2];    // sample -> |q - o|^2 about its block's centre (f64, exact)
    int* ipos[2];     // sample -> sorted position (the screen's partials are stored by position)
    const SceneDev* scp = nullptr;       // the scene in device memory (point_blocked)
    int pretest = 0;                     // draws in an obstacle are settled by samples_role
    int* iter_off[2] = {nullptr, nullptr};  // sample -> its iteration's offset in the window
    // caller-drawn samples (pp_rrt_extend_samples): iteration it's sample is (hsx, hsy)[it -
    // hs_base] instead of the seeded stream (null: the stream); hok: the per-iteration verdicts
    // (a draw in an obstacle: rejected, whichever window it falls in)
    const double* hsx = nullptr;
    const double* hsy = nullptr;
    int64_t hs_base = 0;
    unsigned char* hok = nullptr;
};

// Space::rand_point of iteration itj (rrt.rs:139-146): the seeded stream (Q7: x = draw 2 it,
// y = draw 2 it + 1), or the caller's own sample of that iteration
__device__ __forceinline__ void draw_sample(const SamplesArgs& g, uint64_t itj, double& x,
                                            double& y) {
    if (g.hsx) {
        const int64_t i = (int64_t)itj - g.hs_base;
        x = g.hsx[i];
        y = g.hsy[i];
    } else {
        x = gen_range(g.seed, 2 * itj, g.minx, g.maxx);
        y = gen_range(g.seed, 2 * itj + 1, g.miny, g.maxy);
    }
}

__device__ inline int morton16(int x, int y) {
    int m = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) m |= (((x >> b) & 1) << (2 * b)) | (((y >> b) & 1) << (2 * b + 1));
    return m;
}

// LDS of samples_role: the Morton histogram, each sample's cell, the sorted window's sample ids,
// each sample's iteration offset, the draw rounds' counters and per-wave live counts
constexpr int kSamplesLds = 256 * 4 + kMaxWindow + kMaxWindow * 4 + 16 + 2 * 64 * 4 + kMaxWindow * 2;

// (blockDim.x == 1024: both callers)
__device__ void samples_role(DevState* st, const SamplesArgs& g, int np, int64_t start,
                             char* smem) {
    int* s_hist = reinterpret_cast<int*>(smem);                  // [256]
    unsigned char* s_cell = reinterpret_cast<unsigned char*>(s_hist + 256);  // [K]
    int* s_j = reinterpret_cast<int*>(smem + 256 * 4 + kMaxWindow);  // [K] sorted position -> sample
    // [0] live draws so far, [1] the offset of live draw Kw (the next window's first), [2] a
    // round's live draws
    int* s_nb = s_j + kMaxWindow;
    int* s_wt = s_nb + 4;   // [64] a round's live draws per (pass, wave)
    int* s_wo = s_wt + 64;  // [64] their exclusive prefix
    unsigned short* s_io = reinterpret_cast<unsigned short*>(s_wo + 64);  // [K] sample -> offset
    static_assert(2 * kMaxWindow <= 65536, "samples_role: a window's offsets fit 16 bits");
    const int tid = threadIdx.x, NT = blockDim.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int64_t rem = g.target - start;
    // the adaptive window (kdyn, set by the commits; results never depend on the window size)
    const int Kw = st->kdyn > 0 ? min(g.K, st->kdyn) : g.K;
    for (int i = tid; i < 256; i += NT) s_hist[i] = 0;
    if (tid == 0) {
        s_nb[0] = 0;
        s_nb[1] = 0;
    }
    const double fx = 16.0 / (g.maxx - g.minx), fy = 16.0 / (g.maxy - g.miny);
    // (kU draws per thread per round: their pre-test loads are in flight together)
    constexpr int kU = 4;
    // the pre-test's scene fields, loaded once (through the pointer they would be reloaded after
    // every store below, which the compiler cannot prove disjoint)
    SceneDev scl{};
    bool pre = g.pretest != 0;
    if (pre) {
        scl.bits = g.scp->bits;
        scl.bw = g.scp->bw;
        scl.bh = g.scp->bh;
        scl.bwords = g.scp->bwords;
        scl.bx0 = g.scp->bx0;
        scl.by0 = g.scp->by0;
        scl.binv = g.scp->binv;
        scl.ne = g.scp->ne;
        scl.nbv = g.scp->nbv;
        scl.m = g.scp->m;
        scl.ibits = g.scp->ibits;
        scl.ibn = g.scp->ibn;
        scl.ibwords = g.scp->ibwords;
        scl.ibx0 = g.scp->ibx0;
        scl.iby0 = g.scp->iby0;
        scl.ibinv = g.scp->ibinv;
        scl.goff = g.scp->goff;
        scl.gitems = g.scp->gitems;
        scl.cx = g.scp->cx;
        scl.cy = g.scp->cy;
        scl.r2 = g.scp->r2;
        scl.gx0 = g.scp->gx0;
        scl.gy0 = g.scp->gy0;
        scl.ginv = g.scp->ginv;
        scl.gnx = g.scp->gnx;
        scl.gny = g.scp->gny;
    }
    // (a scene without a pre-test — polygons, no discs: every draw is live and the window is its
    // Kw iterations)
    pre = pre && (scl.bits || (scl.m > 0 && scl.ne == 0 && scl.nbv == 0));
    const int C = st->error ? 0 : window_fill_cap(Kw, rem, pre);
    // sample j, drawn at offset i of the window
    auto place = [&](int j, int i, double x, double y) {
        g.wsx[np][j] = x;
        g.wsy[np][j] = y;
        g.wsx32[np][j] = (float)x;
        g.wsy32[np][j] = (float)y;
        g.iter_off[np][j] = i;
        s_io[j] = (unsigned short)i;
        const int cx = min(max((int)((x - g.minx) * fx), 0), 15);  // == sample_cell
        const int cy = min(max((int)((y - g.miny) * fy), 0), 15);
        const int cell = morton16(cx, cy);
        s_cell[j] = (unsigned char)cell;
        atomicAdd(&s_hist[cell], 1);
    };
    __syncthreads();
    if (!pre) {  // every draw is live: sample j is draw j, one pass
        for (int j0 = tid; j0 < C; j0 += NT * kU) {
            double xs[kU], ys[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int j = j0 + u * NT;
                xs[u] = ys[u] = 0.0;
                if (j < C) draw_sample(g, (uint64_t)(start + j), xs[u], ys[u]);
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int j = j0 + u * NT;
                if (j < C) place(j, j, xs[u], ys[u]);
            }
        }
        if (tid == 0) s_nb[0] = C;
    }
    // the pre-test's draws, in rounds: draw i of the window is iteration start + i; a wave takes
    // 64 consecutive draws, so a ballot and the waves' prefix give every live draw its id in
    // iteration order.  A round is kU draws per thread, kept in registers from the pre-test to
    // the stores, then half as many.  (One longer round with the masks in LDS and the draws made
    // again for the stores was slower: 27.7 against 26.5 us for the benched window.)
    for (int drawn = 0; pre;) {
        __syncthreads();
        const int live0 = s_nb[0];
        if (!window_fill_more(Kw, C, drawn, live0)) break;
        const int end = window_fill_round_end(C, drawn, NT * kU, NT * kU / 2);
        double xs[kU], ys[kU];
        uint64_t mk[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = drawn + u * NT + tid;
            xs[u] = ys[u] = 0.0;
            if (i < end) draw_sample(g, (uint64_t)(start + i), xs[u], ys[u]);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const bool in = drawn + u * NT + tid < end;
            const bool lv = in && !point_blocked<false, kSceneAny>(scl, xs[u], ys[u]);
            mk[u] = __ballot(lv);
            if (lane == 0) s_wt[u * (1024 / 64) + wv] = (int)__popcll(mk[u]);
        }
        __syncthreads();
        if (tid < 64) {
            const int v = s_wt[tid];
            const int x = wave_incl_scan(v);
            s_wo[tid] = x - v;
            if (tid == 63) s_nb[2] = x;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = drawn + u * NT + tid;
            if (i >= end) continue;
            if (!((mk[u] >> lane) & 1)) {
                // in an obstacle: rejected whatever its parent, whichever window it falls in
                if (g.hok) g.hok[start + i - g.hs_base] = 0;
                continue;
            }
            const int j = live0 + s_wo[u * (1024 / 64) + wv] + (int)__popcll(mk[u] & ((1ull << lane) - 1));
            if (j == Kw) s_nb[1] = i;
            if (j < Kw) place(j, i, xs[u], ys[u]);
        }
        __syncthreads();
        if (tid == 0) s_nb[0] = live0 + s_nb[2];
        drawn = end;
    }
    __syncthreads();
    const WindowFill wf = window_fill_close(Kw, C, s_nb[0], s_nb[1]);
    const int W = wf.W, Ws = W;  // every sample is screened: sorted positions [0, W)
    if (tid == 0) {
        st->Wp[np] = W;
        st->Wsp[np] = W;
        st->span[np] = wf.span;
        st->wsp[np] = start;
    }
    // the screen's blocks of rows for Ws samples (the tiling's split; its chunks are the
    // screen's and nn_finalize's business)
    const int R = screen_rows(Ws), nqb = (R + kQPL - 1) / kQPL;
    const int rbase = nqb ? R / nqb : 0, rextra = R - rbase * nqb;  // (screen_geom's row split)
    if (tid < 64) {  // exclusive prefix of the 256 cell counts, 4 per lane
        int v[4], sum = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = s_hist[4 * tid + u];
            sum += v[u];
        }
        const int x = wave_incl_scan(sum);
        int base = x - sum;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s_hist[4 * tid + u] = base;
            base += v[u];
        }
    }
    __syncthreads();
    for (int i = tid; i < 256; i += NT) g.cofs[np][i] = s_hist[i];
    if (tid == 0) g.cofs[np][256] = Ws;
    __syncthreads();  // the cell starts are read before the scatter advances them
    for (int j = tid; j < W; j += NT) s_j[atomicAdd(&s_hist[s_cell[j]], 1)] = j;
    __syncthreads();
    // the screen's blocks of sorted samples (rows of 64, split as the tiling's): the sorted window
    // (coalesced; the coordinates drawn again from the stream, bit-identical), the centre o of the block's
    // bounding box (f32) and every sample's |q - o|^2 in f64 — (q - o) rounded to f32 per axis,
    // the screen's own operands, squared exactly (nn_finalize adds it back to the screen values)
    // every thread takes sorted positions tid, tid + NT, ... (a wave: 64 consecutive positions,
    // inside one block): the coordinates again from the stream, the position's stores, and the
    // wave's f32 bounding box into LDS slot pos / 64 (s_hist is free by now); then one thread per
    // block merges its waves' boxes into the centre o, and every position stores |q - o|^2.  (r03
    // gave each block to one wave, 8 samples per lane, and 16 waves shared 4-8 blocks: the
    // sampling workgroup was nn_finalize's long pole, ~30 of its 27-30 us)
    // s_bb: [kMaxWindow / 64][4] wave boxes (x0, x1, y0, y1), then [kMaxWindow / kQPB][2] block
    // centres, then [kMaxWindow / 64] each row's block — over s_hist and the head of s_cell, both
    // dead after the scatter
    float* s_bb = reinterpret_cast<float*>(s_hist);
    int* s_rb = reinterpret_cast<int*>(s_bb + 4 * (kMaxWindow / 64) + 2 * (kMaxWindow / kQPB));  // [rows]
    __syncthreads();  // (s_hist's last readers: the scatter above)
    constexpr int kMaxK = 4;  // positions per thread: both callers run 1024 threads
    static_assert(kMaxWindow <= 1024 * kMaxK, "samples_role: positions per thread");
    static_assert((5 * (kMaxWindow / 64) + 2 * (kMaxWindow / kQPB)) * 4 <= 256 * 4 + kMaxWindow,
                  "samples_role: the box slots fit s_hist and s_cell");
    double xs[kMaxK], ys[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        const int pos = tid + k * NT;
        xs[k] = ys[k] = 0.0;
        const bool in = pos < Ws;
        if (in) {
            const int j = s_j[pos];
            draw_sample(g, (uint64_t)(start + s_io[j]), xs[k], ys[k]);
            g.perm[np][pos] = j;
            g.ipos[np][j] = pos;
            g.sxy[np][pos] = make_float2((float)xs[k], (float)ys[k]);
            g.ssx[np][pos] = xs[k];
            g.ssy[np][pos] = ys[k];
        }
        const int wbase = pos - lane;  // the wave's first position (uniform)
        if (wbase < Ws) {
            const float inff = __builtin_inff();
            const float bx0 = wave_min_f32(in ? f32_below(xs[k]) : inff);
            const float bx1 = wave_max_f32(in ? f32_above(xs[k]) : -inff);
            const float by0 = wave_min_f32(in ? f32_below(ys[k]) : inff);
            const float by1 = wave_max_f32(in ? f32_above(ys[k]) : -inff);
            if (lane == 0) {
                float* b = s_bb + 4 * (wbase >> 6);
                b[0] = bx0;
                b[1] = bx1;
                b[2] = by0;
                b[3] = by1;
            }
        }
        if (NT * (k + 1) >= kMaxWindow) break;
    }
    __syncthreads();
    if (tid < nqb) {  // block tid's centre: the middle of its samples' box (f32)
        float x0 = __builtin_inff(), x1 = -__builtin_inff(), y0 = __builtin_inff(), y1 = -__builtin_inff();
        const int w0 = screen_split_row0(rbase, rextra, tid), w1 = screen_split_row0(rbase, rextra, tid + 1);
        for (int w = w0; w < w1 && w * 64 < Ws; ++w) {
            s_rb[w] = tid;  // (row -> block, for the |q - o|^2 pass)
            const float* b = s_bb + 4 * w;
            x0 = fminf(x0, b[0]);
            x1 = fmaxf(x1, b[1]);
            y0 = fminf(y0, b[2]);
            y1 = fmaxf(y1, b[3]);
        }
        const float2 o = make_float2((float)(0.5 * ((double)x0 + (double)x1)),
                                     (float)(0.5 * ((double)y0 + (double)y1)));
        g.ob[np][tid] = o;
        s_bb[4 * (kMaxWindow / 64) + 2 * tid] = o.x;  // (after the wave slots)
        s_bb[4 * (kMaxWindow / 64) + 2 * tid + 1] = o.y;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        const int pos = tid + k * NT;
        if (pos < Ws) {
            const int qb = s_rb[pos >> 6];
            const float oxf = s_bb[4 * (kMaxWindow / 64) + 2 * qb];
            const float oyf = s_bb[4 * (kMaxWindow / 64) + 2 * qb + 1];
            const float qpx = (float)(xs[k] - (double)oxf), qpy = (float)(ys[k] - (double)oyf);
            g.sq[np][s_j[pos]] = (double)qpx * (double)qpx + (double)qpy * (double)qpy;
        }
        if (NT * (k + 1) >= kMaxWindow) break;
    }
}

// the Morton cell coordinate of v along one axis (samples_role's binning, clamped)
__device__ inline int sample_cell(double v, double v0, double f) {
    return min(max((int)((v - v0) * f), 0), 15);
}

// Arguments of the window kernel.  Sample buffers are double-buffered by window parity: the
// screen of window w writes wsx/wsy[p], the resolve of w - 1 reads [1 - p].
struct WinKArgs {
    DevState* st;
    SceneDev sc;
    TreeDev tr;
    int K;              // samples per window
    int Kcap;           // buffer capacity per window (stride of the partials)
    int nqb, chunks;    // screen geometry (scan_chunks)
    int p;              // parity of the screened window
    int gen;            // 1: window mode (sorted samples, expanded screen); 0: given wsx/wsy[p]
    int resolve;        // 1: workgroup 0 resolves + commits the previous window
    int scan;           // 0: the drain launch (resolve only)
    int64_t seq;        // sequence number of the screened window
    int64_t target;     // iteration the enqueued windows stop at
    uint64_t seed;
    double* wsx[2];
    double* wsy[2];
    float* wsx32[2];    // f32 copies (the pair search's prefilter)
    float* wsy32[2];
    int* perm[2];       // window mode: sorted position -> sample (window_samples)
    double* sq[2];      // window mode: |q - o|^2 of every sample (the screen's block origin)
    float* pbest;
    float* psecond;
    int* pidx;
    // resolve + commit of the previous window (parity 1 - p)
    const int* nn_idx;
    int* cand_cnt;
    const CandEntry* cand;
    const int* pend;
    int* snap_status;
    double* snap_yaw;
    int* fin_par;
    ResolveScratch rs;
    double* lit_scratch;
    // window mode: workgroup 0 draws the next window's samples (parity 1 - p) after its commit
    int gen_next;
    SamplesArgs g;
    SampleRec hrec;     // pp_rrt_extend_samples: the commit's per-iteration record
};

// RRT::get_nearest_node screen (rrt.rs:378-391): f32 SoA nodes x the window's samples.  The
// screen workgroup b (mapped XCD-aware, so the sample blocks that stream one node chunk share an
// XCD's L2) takes sample block qb and node chunk c.  Its waves split the chunk; every lane holds 4
// samples; node coordinates are wave-uniform scalar loads (the next block in flight) used directly
// as SGPR operands.  Per block of kScanBlk nodes each sample keeps only the block minimum (v_min3),
// merges it into (best, second) with med3 and records the block that first attained the best; the
// winning block is re-evaluated afterwards with the same arithmetic (bit-identical) for the lowest
// index and the in-block second best.  Result: the exact per-chunk top-2 of the screen values.
//
// kExp (window mode): the samples come spatially sorted (window_samples: perm), so a block of 256
// is compact and the screen runs in the expanded form about the block's centre o:
//     e(n) = |n - o|^2 - 2 (q - o).(n - o)  =  |q - n|^2 - |q - o|^2
// two FMAs per (node, sample) after a per-node prologue (n - o, |n - o|^2: four ops per wave,
// shared by the lane's 4 samples) — 3.5 VALU per evaluation instead of 4.5.  nn_finalize adds
// |q - o|^2 back (sq) and widens the near-tie margin by the expanded form's rounding bound.
// !kExp (nearest API): the given samples, direct form (sub, sub, mul, fma).
// The screen's winner re-evaluation of a block no longer in LDS (trees past one staging round):
// the block's 16 nodes from global memory with the screen's own prep and arithmetic, the lowest
// u with value == best and the minimum of the others.  Out of line: inlined, the compiler merges
// it with the LDS path into flat loads.  The result comes back by value, in registers: passed by
// reference, ui and other lived in scratch, 8 bytes stored and reloaded by every sample's thread.
struct BlockPick {
    int ui;       // the lowest node of the block with value == best (-1: none)
    float other;  // the minimum of the block's other nodes
};
template <bool kExp, int kNodes = kScanBlk>
__device__ __attribute__((noinline)) BlockPick screen_block_global(const float* __restrict__ bx,
                                                                   const float* __restrict__ by,
                                                                   float qx, float qy, float oxf,
                                                                   float oyf, float best) {
    int ui = -1;
    float other = __builtin_inff();
    for (int u = 0; u < kNodes; ++u) {
        float px = bx[u], py = by[u], pw = 0.0f;
        if (kExp) {
            px = px - oxf;
            py = py - oyf;
            pw = __builtin_fmaf(py, py, px * px);
        }
        const float d = kExp ? __builtin_fmaf(qx, px, __builtin_fmaf(qy, py, pw))
                             : scan_d2(qx, qy, px, py);
        if (ui < 0 && d == best)
            ui = u;
        else
            other = __builtin_fminf(other, d);
    }
    return BlockPick{ui, other};
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// A block of kScanBlk staged nodes in registers: x | y | |n-o|^2, read as broadcast ds_read_b128.
struct NodeBlk {
    float4 vx[kScanBlk / 4], vy[kScanBlk / 4], vw[kScanBlk / 4];
    __device__ __forceinline__ void load(const float* stg, int u0) {
#pragma unroll
        for (int v = 0; v < kScanBlk / 4; ++v) {
            vx[v] = *reinterpret_cast<const float4*>(stg + u0 + 4 * v);
            vy[v] = *reinterpret_cast<const float4*>(stg + kStage + u0 + 4 * v);
            vw[v] = *reinterpret_cast<const float4*>(stg + 2 * kStage + u0 + 4 * v);
        }
    }
    static __device__ __forceinline__ float at(const float4& q, int i) {
        return i == 0 ? q.x : i == 1 ? q.y : i == 2 ? q.z : q.w;
    }
    __device__ __forceinline__ float x(int u) const { return at(vx[u >> 2], u & 3); }
    __device__ __forceinline__ float y(int u) const { return at(vy[u >> 2], u & 3); }
    __device__ __forceinline__ float w(int u) const { return at(vw[u >> 2], u & 3); }
};

// One screen workgroup: sample block qb (kR rows of 64 sorted positions from row0: kR samples per
// lane, none padded) against chunk c of the `chunks` the block splits the ns nodes into.
template <bool kExp, int kR>
__device__ __attribute__((always_inline)) inline void scan_tile(const WinKArgs& a, char* smem,
                                                               int qb, int row0, int c, int chunks,
                                                               int W, int ns) {
    static_assert(kR >= 1 && kR <= kQPL, "rows of a sample block");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qbase = row0 * 64;
    if (qbase >= W) return;
    const int cl = scan_chunk_len(ns, chunks);
    const int c0 = c * cl;
    if (c0 >= ns) return;
    const int L = min(c0 + cl, ns) - c0;  // the chunk's nodes
    const float* nx = a.tr.x32;
    const float* ny = a.tr.y32;
    // The chunk goes through the workgroup's LDS (x | y | |n-o|^2, kStage nodes a round; one
    // round up to ~250k tree nodes at K = 4096): LDS-DMA (global_load_lds_dwordx4, lane l brings
    // nodes 4l..4l+3 of a 256-node quarter, no registers) issued before the samples are read, so
    // the two latencies overlap; each thread then preps its own float4s in place — (n - o,
    // |n - o|^2) in the expanded form, each node once instead of once per lane.  The waves split
    // the round's blocks evenly, each a contiguous run in increasing order, so a wave's first block
    // to reach the best is its lowest.  (Until the balanced tiling the waves took 64-node pieces
    // from an LDS counter: a workgroup's time came in steps of 8 waves x 64 nodes, which ate the
    // tiling's gain.)  The block loop reads its 16 nodes as broadcast ds_read_b128.
    float* stg = reinterpret_cast<float*>(smem + kScreenStageOff);
    auto issue_round = [&](int r0) {
        const int len = min(kStage, L - r0);
        for (int q4 = wave; q4 * 256 < len; q4 += kScanWaves) {
            if (q4 * 256 + 4 * lane < len) {  // (a partial float4 reads up to 3 padding floats)
                const size_t gi = (size_t)(c0 + r0 + q4 * 256 + 4 * lane);
                __builtin_amdgcn_global_load_lds((glb_void*)(nx + gi), (lds_void*)(stg + q4 * 256), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((glb_void*)(ny + gi), (lds_void*)(stg + kStage + q4 * 256), 16, 0, 0);
            }
        }
    };
    issue_round(0);
    float qxr[kR], qyr[kR], best[kR], second[kR];
    int sid[kR], blk[kR], bi[kR];
    float oxf = 0.0f, oyf = 0.0f;
    if (kExp) {
        // window mode: samples_role left the window sorted (f64, coalesced), each screen block's
        // centre o and every sample's |q - o|^2 (for nn_finalize)
        const float2 o = a.g.ob[a.p][qb];
        oxf = o.x;
        oyf = o.y;
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int pos = qbase + r * 64 + lane;
            const bool in = pos < W;
            sid[r] = in ? a.perm[a.p][pos] : -1;
            const double xs = in ? a.g.ssx[a.p][pos] : (double)oxf;
            const double ys = in ? a.g.ssy[a.p][pos] : (double)oyf;
            const float qpx = (float)(xs - (double)oxf), qpy = (float)(ys - (double)oyf);
            qxr[r] = -2.0f * qpx;  // exact scaling
            qyr[r] = -2.0f * qpy;
        }
    } else {
        const double* qxs = a.wsx[a.p];
        const double* qys = a.wsy[a.p];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int pos = qbase + r * 64 + lane;
            sid[r] = pos < W ? pos : -1;
            qxr[r] = sid[r] >= 0 ? (float)qxs[pos] : 0.0f;
            qyr[r] = sid[r] >= 0 ? (float)qys[pos] : 0.0f;
        }
    }
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        best[r] = __builtin_inff();
        second[r] = __builtin_inff();
        blk[r] = -1;
        bi[r] = -1;
    }
    {  // wave 0 parks the samples' operands for the winner re-evaluation (read after barriers)
        float* s_qx = reinterpret_cast<float*>(smem) + (3 * kScanWaves + 1) * kQPB;
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < kR; ++r) {
                s_qx[r * 64 + lane] = qxr[r];
                s_qx[kQPB + r * 64 + lane] = qyr[r];
            }
        }
    }
    // screen value of (sample r, node (nx, ny)); expanded: the node's (x - ox, y - oy, |.|^2)
    auto val = [&](int r, float px, float py, float pw) {
        if (kExp) return __builtin_fmaf(qxr[r], px, __builtin_fmaf(qyr[r], py, pw));
        return scan_d2(qxr[r], qyr[r], px, py);
    };
    auto prep = [&](float& px, float& py, float& pw) {
        if (kExp) {
            px = px - oxf;
            py = py - oyf;
            pw = __builtin_fmaf(py, py, px * px);
        } else {
            pw = 0.0f;
        }
    };
    // One block of kScanBlk nodes (in registers) against the lane's samples: each sample's block
    // minimum, merged into (best, second, block).  Expanded form: two nodes per packed FMA
    // (v_pk_fma_f32: each half the exactly rounded fmaf of the scalar form, so the winner
    // re-evaluation below stays bit-identical), the pair folded in by one v_min3 per sample,
    // min(min(bm, d.x), d.y) — 8 three-input minima per sample and block (written as
    // min(bm, min(d.x, d.y)) it compiled to 12).  The compiler issues the block's inner FMAs
    // first, then the outer ones; pinning the order per node pair with scheduling barriers and
    // reading block u + 1 ahead into a second register set measured slower.
    auto block = [&](const NodeBlk& nb, int k) {
        float bm[kR];
        if (kExp) {
#pragma unroll
            for (int u = 0; u < kScanBlk; u += 2) {
                const f32x2 PX = {nb.x(u), nb.x(u + 1)}, PY = {nb.y(u), nb.y(u + 1)};
                const f32x2 PW = {nb.w(u), nb.w(u + 1)};
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const f32x2 QX = {qxr[r], qxr[r]}, QY = {qyr[r], qyr[r]};
                    const f32x2 d = __builtin_elementwise_fma(
                        QX, PX, __builtin_elementwise_fma(QY, PY, PW));
                    bm[r] = u == 0 ? __builtin_fminf(d.x, d.y)
                                   : __builtin_fminf(__builtin_fminf(bm[r], d.x), d.y);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < kScanBlk; ++u) {
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const float d = val(r, nb.x(u), nb.y(u), nb.w(u));
                    bm[r] = u == 0 ? d : __builtin_fminf(bm[r], d);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            second[r] = __builtin_amdgcn_fmed3f(best[r], bm[r], second[r]);
            if (bm[r] < best[r]) {
                best[r] = bm[r];
                blk[r] = k;
            }
        }
    };
    int r0 = 0;
    for (;;) {
        const int len = min(kStage, L - r0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA has landed
        __syncthreads();                                   // ... and every other wave's
        for (int i = 4 * tid; i < len; i += 4 * kScanThreads) {  // prep in place
            float4 x4 = *reinterpret_cast<const float4*>(stg + i);
            float4 y4 = *reinterpret_cast<const float4*>(stg + kStage + i);
            float4 w4;
            prep(x4.x, y4.x, w4.x);
            prep(x4.y, y4.y, w4.y);
            prep(x4.z, y4.z, w4.z);
            prep(x4.w, y4.w, w4.w);
            *reinterpret_cast<float4*>(stg + i) = x4;
            *reinterpret_cast<float4*>(stg + kStage + i) = y4;
            *reinterpret_cast<float4*>(stg + 2 * kStage + i) = w4;
        }
        __syncthreads();
        {
            // the round's whole blocks split evenly over the waves, each a contiguous run (at
            // most one block apart); the tail (< kScanBlk nodes, the chunk's last) is the last
            // wave's
            const int nblk = len / kScanBlk;
            const int wv = __builtin_amdgcn_readfirstlane(wave);  // (scalar loop bounds)
            const int g0 = (wv * nblk / kScanWaves) * kScanBlk;
            const int gb = ((wv + 1) * nblk / kScanWaves) * kScanBlk;
            const int g1 = wv == kScanWaves - 1 ? len : gb;
            for (int u0 = g0; u0 < gb; u0 += kScanBlk) {
                NodeBlk nb;
                nb.load(stg, u0);
                block(nb, c0 + r0 + u0);
            }
            for (int u = gb; u < g1; ++u) {  // the chunk's tail (< kScanBlk nodes): exact top-2
                const float px = stg[u], py = stg[kStage + u], pw = stg[2 * kStage + u];
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const float d = val(r, px, py, pw);
                    second[r] = __builtin_amdgcn_fmed3f(best[r], d, second[r]);
                    if (d < best[r]) {
                        best[r] = d;
                        bi[r] = c0 + r0 + u;
                        blk[r] = -1;  // the best is a tail node, not a block's
                    }
                }
            }
        }
        if (r0 + len >= L) break;
        r0 += len;
        __syncthreads();  // every wave is done with this round before the next overwrites it
        issue_round(r0);
    }
    // The waves' partials per sample go to LDS — (best, second, key): key = the best block's start,
    // or kExactNode | index when the best is a tail node (tail nodes follow every block of the
    // chunk, so keys order ties by node index either way), 0x7fffffff when the wave saw no node —
    // and one thread per sample merges them; only then is the winning block re-evaluated (one
    // block per sample, not one per wave): the same arithmetic again, bit-identical, for the lowest
    // index of the best value and the best of the block's other nodes (the block minima carried one
    // each).  From LDS when the block is in the last round (always up to ~250k nodes).
    float* s_b = reinterpret_cast<float*>(smem);              // [kScanWaves][kQPB]
    float* s_s = s_b + kScanWaves * kQPB;
    int* s_i = reinterpret_cast<int*>(s_s + kScanWaves * kQPB);
    int* s_sid = s_i + kScanWaves * kQPB;                      // [kQPB]
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        s_b[wave * kQPB + r * 64 + lane] = best[r];
        s_s[wave * kQPB + r * 64 + lane] = second[r];
        s_i[wave * kQPB + r * 64 + lane] =
            blk[r] >= 0 ? blk[r] : (bi[r] >= 0 ? (bi[r] | kExactNode) : 0x7fffffff);
        if (wave == 0) s_sid[r * 64 + lane] = sid[r];
    }
    __syncthreads();
    if (tid < 64 * kR) {  // one thread per sample (sorted position qbase + tid)
        float bb = s_b[tid], ss = s_s[tid];
        int key = s_i[tid];
#pragma unroll
        for (int w = 1; w < kScanWaves; ++w) {
            const float ob = s_b[w * kQPB + tid], os = s_s[w * kQPB + tid];
            const int ok = s_i[w * kQPB + tid];
            const bool take = ob < bb || (ob == bb && ok < key);  // (branch-free)
            ss = fminf(fminf(ss, os), take ? bb : ob);
            bb = take ? ob : bb;
            key = take ? ok : key;
        }
        const int q = s_sid[tid];
        int idx = key == 0x7fffffff ? -1 : (key & ~kExactNode);
        if (q >= 0 && key != 0x7fffffff && !(key & kExactNode)) {
            // the sample's screen operands, as wave 0 held them
            const float* s_qx = reinterpret_cast<const float*>(smem) + (3 * kScanWaves + 1) * kQPB;
            const float qx = s_qx[tid], qy = s_qx[kQPB + tid];
            const int rel = key - c0 - r0;
            int ui = -1;
            float other = __builtin_inff();
            if (rel >= 0) {  // (LDS only: a shared pointer select would make these flat loads)
                float vx[kScanBlk], vy[kScanBlk], vw[kScanBlk];
#pragma unroll
                for (int v = 0; v < kScanBlk / 4; ++v) {
                    const float4 a4 = *reinterpret_cast<const float4*>(stg + rel + 4 * v);
                    const float4 b4 = *reinterpret_cast<const float4*>(stg + kStage + rel + 4 * v);
                    const float4 w4 = *reinterpret_cast<const float4*>(stg + 2 * kStage + rel + 4 * v);
                    vx[4 * v] = a4.x, vx[4 * v + 1] = a4.y, vx[4 * v + 2] = a4.z, vx[4 * v + 3] = a4.w;
                    vy[4 * v] = b4.x, vy[4 * v + 1] = b4.y, vy[4 * v + 2] = b4.z, vy[4 * v + 3] = b4.w;
                    vw[4 * v] = w4.x, vw[4 * v + 1] = w4.y, vw[4 * v + 2] = w4.z, vw[4 * v + 3] = w4.w;
                }
#pragma unroll
                for (int u = 0; u < kScanBlk; ++u) {
                    const float d = kExp ? __builtin_fmaf(qx, vx[u], __builtin_fmaf(qy, vy[u], vw[u]))
                                         : scan_d2(qx, qy, vx[u], vy[u]);
                    if (ui < 0 && d == bb)
                        ui = u;
                    else
                        other = __builtin_fminf(other, d);
                }
            } else {
                const BlockPick g = screen_block_global<kExp>(nx + key, ny + key, qx, qy, oxf, oyf, bb);
                ui = g.ui;
                other = g.other;
            }
            idx = key + ui;
            ss = __builtin_fminf(ss, other);
        }
        if (q >= 0) {  // by sorted position: coalesced (nn_finalize maps samples through ipos)
            const size_t o = (size_t)c * a.Kcap + qbase + tid;
            a.pbest[o] = bb;
            a.psecond[o] = ss;
            a.pidx[o] = idx;
        }
    }
}

// Screen workgroup b: its tile, and the tile's loop with as many accumulators as the block has rows.
// Window mode: the tiling for the samples not in an obstacle (samples_role sorted them first) —
// workgroup b takes its XCD's share of the work list, so the workgroups that stream one node range
// share an L2.  The nearest API: the given samples in full blocks on the launch's geometry.
template <bool kExp>
__device__ __attribute__((always_inline)) inline void scan_role(const WinKArgs& a, int b,
                                                               char* smem) {
    DevState* st = a.st;
    const int ns = st->n_scan;
    if (b == 0 && threadIdx.x == 0) st->nsp[a.p] = ns;
    if constexpr (kExp) {
        const int W = st->Wsp[a.p];
        const ScreenWork w = screen_work_unpack(kScreenTables.wg[screen_rows(W)][b]);  // (one load)
        if (w.rows == 0) return;  // no tile for this workgroup
        const int qb = w.k, c = w.c, row0 = w.row0, chunks = w.chunks;
        switch (w.rows) {  // (uniform over the workgroup)
            case 1: scan_tile<kExp, 1>(a, smem, qb, row0, c, chunks, W, ns); break;
            case 2: scan_tile<kExp, 2>(a, smem, qb, row0, c, chunks, W, ns); break;
            case 3: scan_tile<kExp, 3>(a, smem, qb, row0, c, chunks, W, ns); break;
            case 4: scan_tile<kExp, 4>(a, smem, qb, row0, c, chunks, W, ns); break;
            case 5: scan_tile<kExp, 5>(a, smem, qb, row0, c, chunks, W, ns); break;
            case 6: scan_tile<kExp, 6>(a, smem, qb, row0, c, chunks, W, ns); break;
            case 7: scan_tile<kExp, 7>(a, smem, qb, row0, c, chunks, W, ns); break;
            case 8: scan_tile<kExp, 8>(a, smem, qb, row0, c, chunks, W, ns); break;
            default: break;
        }
    } else {
        const int G = a.nqb * a.chunks;
        if (b >= G) return;
        const int t = (G & 7) == 0 ? (b & 7) * (G >> 3) + (b >> 3) : b;
        const int qb = t % a.nqb, c = t / a.nqb;
        scan_tile<kExp, kQPL>(a, smem, qb, qb * kQPL, c, a.chunks, st->Wp[a.p], ns);
    }
}


// The first window of a batch: its samples (the later ones come from the previous window kernel
// workgroup 0, after the commit that decides where the next window starts).
__global__ __launch_bounds__(1024) void window_samples_kernel(DevState* st, SamplesArgs g, int np) {
    __shared__ __attribute__((aligned(16))) char smem[kSamplesLds];
    samples_role(st, g, np, st->it_spec, smem);
}


// nn_finalize: kFinSamples samples per workgroup, one wave per sample.
//  1. The wave merges the sample's screen partials (lane c: chunk c) and screens the nodes the
//     window's screen did not cover — the ones appended since (the previous window's commit) —
//     with the same f32 arithmetic (lanes stride them), then reduces the top-2 across the wave.
//     Margin test against the f32 rounding bound: certain → exact f64 d2 of the winner; else the
//     wave's exact f64 brute force over the screen chunks whose f32 minimum could hide the exact
//     nearest and over the appended nodes (rrt.rs:378-391; lowest index on exact ties, Q9).
//  2. Window pairs (window mode): for each of the workgroup's samples j (one wave each), the
//     earlier window samples i < j strictly nearer than j's snapshot NN — the candidates of the
//     sequential-consistency resolve.  The window's samples are binned in a 16 x 16 Morton grid
//     (samples_role: perm, cofs, sorted f32 copies), so the wave visits only the cells j's disc
//     of radius sqrt(D2) touches; an f32 distance within the rounding margin of the NN distance
//     goes to the exact f64 test (dx*dx + dy*dy < nn_d2, the oracle's arithmetic).  Hits stay in
//     LDS (at most kCandCap per sample, the count exact) and are appended with one global atomic
//     per workgroup.
// Workgroup 0 also publishes the window (W, or 0 when a truncated predecessor voided it) for the
// later kernels and advances the next window's screen position.
constexpr int kFinThreads = 1024;
constexpr int kFinWaves = kFinThreads / 64;
constexpr int kFinSamples = kFinWaves;  // one wave per sample
constexpr int kFinDelta = 4096;         // appended nodes staged in LDS (beyond: global loads)
// eps_coord (mx 2^-23) up to which the expanded screen's first-order coordinate term stands alone:
// mx = 2^12, past every scene whose fast-path rate is on record (their margin is unchanged)
constexpr double kEpsCoordNear = 0x1p-11;

// The window's samples binned by Morton cell (samples_role): the pair search's spatial index.
struct PairGrid {
    const int* perm;     // sorted position -> sample
    const int* cofs;     // [257] first sorted position of each cell
    const float2* sxy;   // sorted position -> (x, y) f32
    const double* ssx;   // sorted position -> x, y f64 (the samples' own coordinates, bit for bit)
    const double* ssy;
    double minx, miny, fx, fy;  // samples_role's binning: cell = (v - v0) * f, clamped to 0..15
    float slack;         // f32 prefilter margin for the coordinates' magnitude
};

// the wave's top-2 (every lane ends with it): butterfly steps that merge disjoint lane sets, on
// DPP and the gfx950 lane swaps (merge_top2 is not idempotent: a set merged with itself would
// report its best as its second)
template <int kCtrl>
__device__ inline Top2 top2_dpp(Top2 t) {
    return Top2{__builtin_bit_cast(float, dpp_pair<kCtrl>(__builtin_bit_cast(int, t.b))),
                __builtin_bit_cast(float, dpp_pair<kCtrl>(__builtin_bit_cast(int, t.s))),
                dpp_pair<kCtrl>(t.i)};
}
template <bool k32>
__device__ inline Top2 top2_swap(Top2 t) {
    const LanePair b = k32 ? swap32(__builtin_bit_cast(int, t.b)) : swap16(__builtin_bit_cast(int, t.b));
    const LanePair s = k32 ? swap32(__builtin_bit_cast(int, t.s)) : swap16(__builtin_bit_cast(int, t.s));
    const LanePair i = k32 ? swap32(t.i) : swap16(t.i);
    return merge_top2(Top2{__builtin_bit_cast(float, b.a), __builtin_bit_cast(float, s.a), i.a},
                      Top2{__builtin_bit_cast(float, b.b), __builtin_bit_cast(float, s.b), i.b});
}
__device__ inline Top2 wave_top2(Top2 t) {
    t = merge_top2(t, top2_dpp<0xB1>(t));   // quad_perm [1,0,3,2]
    t = merge_top2(t, top2_dpp<0x4E>(t));   // quad_perm [2,3,0,1]
    t = merge_top2(t, top2_dpp<0x141>(t));  // row_half_mirror
    t = merge_top2(t, top2_dpp<0x140>(t));  // row_mirror
    t = top2_swap<false>(t);
    return top2_swap<true>(t);
}

#ifdef PP_FIN_STAMPS  // diagnostic builds only: wall-clock phase stamps of nn_finalize per workgroup
__device__ unsigned long long g_fin_stamps[kFinStampSlots * kFinStampWGs];
#define FS(k)                                                                          \
    if (threadIdx.x == 0 && blockIdx.x < kFinStampWGs)                                 \
        g_fin_stamps[kFinStampSlots * blockIdx.x + (k)] = wall_clock64();
#define FSW(k)                                                                         \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < kFinStampWGs)                         \
        atomicMax(&g_fin_stamps[kFinStampSlots * blockIdx.x + (k)], wall_clock64());
hipError_t fin_stamps_copy(unsigned long long* out, size_t n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fin_stamps), n * sizeof(unsigned long long));
}
#else
#define FS(k)
#define FSW(k)
#endif

// 8 waves per SIMD (<= 64 VGPRs): two 1024-thread workgroups per CU, so the extra sampling
// workgroup (the grid's last) runs beside the others instead of waiting for a CU to drain.
__global__ __launch_bounds__(kFinThreads, 8) void nn_finalize_kernel(
    DevState* __restrict__ st, int p, int64_t seq, int chunks_api, const float* __restrict__ pbest,
    const float* __restrict__ psecond, const int* __restrict__ pidx, int stride,
    const double* __restrict__ qx, const double* __restrict__ qy, const float* __restrict__ x32,
    const float* __restrict__ y32, const double* __restrict__ X, const double* __restrict__ Y,
    const double* __restrict__ YAW, double eps_coord, int* __restrict__ out_idx,
    double* __restrict__ out_d2, double* __restrict__ out_pose, PairGrid pg,
    int* __restrict__ cand_cnt, CandEntry* __restrict__ cand,
    int* __restrict__ pend, const double* __restrict__ sq, const int* __restrict__ ipos,
    SamplesArgs gen, int gen_next) {
    __shared__ double s_nd2[kFinSamples];  // exact snapshot NN d2 of each sample
    __shared__ int s_pc[kFinSamples];      // pair search: nearer window samples found
    __shared__ int s_pi[kFinSamples][kCandCap];
    __shared__ double s_pd[kFinSamples][kCandCap];
    __shared__ int s_pbase, s_pnb;
    __shared__ uint32_t s_fmask;         // samples (waves) that need the exact brute force
    __shared__ double s_fd[kFinSamples];  // candidate-chunk bound on pbest of a near-tie
    __shared__ uint64_t s_cmask;
    __shared__ double s_rd[kFinWaves];
    __shared__ int s_ri[kFinWaves];
    __shared__ float2 s_dn[kFinDelta];   // nodes appended after the screen's snapshot (f32)
    // per row of 64 sorted positions: the chunks its samples' partials fill and their length (one
    // wave works them out for the workgroup: a block lookup and two divisions a row, not a wave)
    __shared__ int s_nch[kMaxWindow / 64], s_cl[kMaxWindow / 64];
    FS(0)
    const bool voided = st->void_seq == seq || st->error;
    if (gen_next && blockIdx.x == gridDim.x - 1) {
        // the extra workgroup: Space::rand_point of the window after this one, into the parity
        // the committed previous window freed — it starts where this window ends, or, when the
        // commit voided this window (a truncation), where the committed one stopped (it_spec;
        // workgroup 0 advances it_spec only when this window is not voided).  Off the critical
        // path: steer_prep and steer_walk of this window run before the next screen.
        __shared__ __attribute__((aligned(16))) char s_gen[kSamplesLds];
        const int64_t start = voided ? st->it_spec : st->wsp[p] + st->span[p];
        samples_role(st, gen, 1 - p, start, s_gen);
        FS(9)
        return;
    }
    const int W = voided ? 0 : st->Wp[p];
    const int ns = st->nsp[p], n = st->n;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->W = W;
        // (the iterations the window spans: its samples and the draws in an obstacle between them)
        st->span_cur = voided ? 0 : st->span[p];
        st->n_scan = n;
        if (!voided) st->it_spec = st->wsp[p] + st->span[p];
    }
    const int q0 = (int)blockIdx.x * kFinSamples;
    if (q0 >= W) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = q0 + wave;
    const bool in = q < W;
    const int D = n - ns, Dl = min(D, kFinDelta);  // appended nodes (staged: the first kFinDelta)
    for (int k = tid; k < Dl; k += kFinThreads) s_dn[k] = make_float2(x32[ns + k], y32[ns + k]);
    if (tid < kMaxWindow / 64) {
        // the node chunks of the samples in row tid — window mode: those of the row's block in the
        // tiling for the window's screened samples; the nearest API: the launch's
        const int chunks = cand ? screen_chunks_of_row(kScreenTables.g[screen_rows(st->Wsp[p])], tid)
                                : chunks_api;
        const int cl = scan_chunk_len(ns, chunks);
        s_cl[tid] = cl;
        s_nch[tid] = (ns + cl - 1) / cl;
    }
    if (tid < kFinSamples) s_pc[tid] = 0;
    if (tid == 0) s_fmask = 0;
    __syncthreads();
    FS(1)
    // ---- 1. the sample's nearest node
    if (in) {
        const int pq = ipos ? ipos[q] : q;  // the sample's sorted position (the partials' index)
        Top2 t{__builtin_inff(), __builtin_inff(), -1};
        const double qq = sq ? sq[q] : 0.0;  // window mode: screen values are d2 - |q - o|^2
        // this lane's chunk: raw screen top-2.  Every lane loads (the partials hold kMaxChunks
        // chunks per sample) and the lanes past the sample's chunks drop what they read: the
        // chunk count hangs on the sample's position and the loads do not wait for it.
        static_assert(kMaxChunks == 64, "one lane per chunk");
        const size_t po = (size_t)lane * stride + pq;
        float cb = pbest[po], cs = psecond[po];
        int ci = pidx[po];
        const int n_chunks = s_nch[pq >> 6];
        if (lane < n_chunks) {
            t = Top2{(float)((double)cb + qq), (float)((double)cs + qq), ci};
        } else {
            cb = cs = __builtin_inff();
            ci = -1;
        }
        FSW(2)
        const double xq = qx[q], yq = qy[q];
        const float fx = (float)xq, fy = (float)yq;
        for (int k = lane; k < D; k += 64) {  // appended nodes: exact top-2 per lane
            const float2 v = k < Dl ? s_dn[k] : make_float2(x32[ns + k], y32[ns + k]);
            const float d = scan_d2(fx, fy, v.x, v.y);
            const Top2 c{d, __builtin_inff(), ns + k};
            t = merge_top2(t, c);
        }
        t = wave_top2(t);
        bool flag = t.i < 0 || !(t.b < __builtin_inff());
        double cthr = __builtin_inf();  // near-tie: the chunks with pbest <= cthr are rescanned
        if (!flag) {
            const double D1 = sqrt((double)t.b);
            if (!sq) {  // direct screen: f32 rounding of the coordinates and the arithmetic
                const double tc = 16.0 * eps_coord + 4.0e-6 * (D1 + 1.0);
                cthr = (D1 + tc) * (D1 + tc);
                if (t.s < __builtin_inff()) {
                    const double D2 = sqrt((double)t.s);
                    flag = !(D2 - D1 > 8.0 * eps_coord + 1.0e-6 * D2);
                }
            } else {  // expanded screen: rounding of |n-o|^2 - 2(q-o).(n-o) about the block centre
                const double qn = sqrt(qq);
                double D = (t.s < __builtin_inff() ? sqrt((double)t.s) : D1) + 1.0;
                // |dE| <= 5u (|n-o|^2 + 2|q-o||n-o|) for the f32 inputs and arithmetic
                // (u = 2^-24, |n-o| <= |q-o| + D for the winner and the runner-up), plus the f32
                // rounding of the node coordinates (|dn| <= eps_coord / 2 per axis): a node at
                // the true distance d screens at d^2 + 2 dn.(n - q) + |dn|^2, |dn| < eps_coord.
                // The first-order term 8 eps_coord (D + 1) also covers |dn|^2 and the error of D
                // itself (read off the screen's own values) while eps_coord is far below 1 (it
                // holds to about eps_coord = 0.5); a frame whose f32 ulp is no longer small
                // against the node spacing needs both spelled out (d <= sqrt(s) + 2.5 eps_coord
                // for a screen value s), or two nodes in different f32 cells pass for told apart
                // (NaN from a negative t.s flags the sample: every comparison below fails)
                double e2 = 0.0;
                if (eps_coord > kEpsCoordNear) {
                    D += 2.5 * eps_coord;
                    e2 = eps_coord * eps_coord;
                }
                const double E = 4.0e-7 * ((qn + D) * (qn + D) + 2.0 * qn * (qn + D)) +
                                 8.0 * eps_coord * (D + 1.0) + e2;
                cthr = (double)t.b + 2.0 * E - qq;
                if (t.s < __builtin_inff()) flag = !((double)t.s - (double)t.b > 2.0 * E);
            }
        }
        FSW(3)
        if (!flag) {
            const int bi = t.i;
            const double dx = xq - X[bi], dy = yq - Y[bi];
            const double bd = dx * dx + dy * dy;
            FSW(4)
            if (lane == 0) {
                out_idx[q] = bi;
                out_d2[q] = bd;
                s_nd2[wave] = bd;
                if (out_pose) {
                    out_pose[3 * q] = X[bi];
                    out_pose[3 * q + 1] = Y[bi];
                    out_pose[3 * q + 2] = YAW[bi];
                }
            }
        } else {
            // a near-tie: the nodes that can still be the exact nearest are those whose screen
            // value is <= cthr.  When every candidate chunk holds one of them (its second > cthr),
            // they are the chunks' known winners: the wave decides exactly on those and the
            // appended nodes.  A chunk with two (or more) falls to the workgroup's brute force.
            // The appended nodes are screened again in the direct form against the exact
            // distance U of a known node: only those within its f32 rounding bound load f64.
            bool need = false;
            double bd = __builtin_inf();
            int bi = 0x7fffffff;
            if (t.i >= 0) {  // the screen's winner (a chunk's or an appended node)
                const double dx = xq - X[t.i], dy = yq - Y[t.i];
                bd = dx * dx + dy * dy;
                bi = t.i;
            }
            if (!((double)cb > cthr)) {
                if (!((double)cs > cthr) || ci < 0) {
                    need = true;
                } else {
                    const double dx = xq - X[ci], dy = yq - Y[ci];
                    argmin_pair(bd, bi, dx * dx + dy * dy, ci);
                }
            }
            wave_argmin(bd, bi);
            if (D > 0 && !__any(need)) {
                const double U = sqrt(bd), tu = 16.0 * eps_coord + 4.0e-6 * (U + 1.0);
                const double lim = (U + tu) * (U + tu);
                for (int k = lane; k < D; k += 64) {
                    const float2 v = k < Dl ? s_dn[k] : make_float2(x32[ns + k], y32[ns + k]);
                    if (!((double)scan_d2(fx, fy, v.x, v.y) > lim)) {
                        const double dx = xq - X[ns + k], dy = yq - Y[ns + k];
                        argmin_pair(bd, bi, dx * dx + dy * dy, ns + k);
                    }
                }
                wave_argmin(bd, bi);
            }
            if (lane == 0) atomicAdd(&st->flag_count, 1);  // statistics (nn_flagged)
            if (__any(need) || bi == 0x7fffffff) {
                if (lane == 0) {
                    atomicOr(&s_fmask, 1u << wave);
                    s_fd[wave] = cthr;
                }
            } else if (lane == 0) {
                out_idx[q] = bi;
                out_d2[q] = bd;
                s_nd2[wave] = bd;
                if (out_pose) {
                    out_pose[3 * q] = X[bi];
                    out_pose[3 * q + 1] = Y[bi];
                    out_pose[3 * q + 2] = YAW[bi];
                }
            }
        }
    }
    __syncthreads();
    FS(5)
    // near-ties: the workgroup's exact f64 brute force, over the screen chunks whose f32 minimum
    // could hide the exact nearest (f32 distance within the rounding bound of the f32 winner)
    // and over the appended nodes; lowest index on exact ties (rrt.rs:378-391, Q9)
    for (uint32_t fm = s_fmask; fm; fm &= fm - 1) {
        const int w = (int)__builtin_ctz(fm);
        const int qf = q0 + w;
        const double cthr = s_fd[w];
        const int pf = ipos ? ipos[qf] : qf;
        const int n_chunks = s_nch[pf >> 6];  // (uniform: every wave works on sample qf)
        if (wave == 0) {
            const bool cc = lane < n_chunks && !((double)pbest[(size_t)lane * stride + pf] > cthr);
            const uint64_t cm = __ballot(cc);
            if (lane == 0) s_cmask = cm;
        }
        __syncthreads();
        const int cl = s_cl[pf >> 6];
        const double xq = qx[qf], yq = qy[qf];
        double bd = __builtin_inf();
        int bi = 0x7fffffff;
        for (uint64_t cm = s_cmask; cm; cm &= cm - 1) {
            const int c = (int)__builtin_ctzll(cm);
            const int c1 = min(c * cl + cl, ns);
            for (int k = c * cl + tid; k < c1; k += kFinThreads) {
                const double dx = xq - X[k], dy = yq - Y[k];
                argmin_pair(bd, bi, dx * dx + dy * dy, k);
            }
        }
        for (int k = ns + tid; k < n; k += kFinThreads) {
            const double dx = xq - X[k], dy = yq - Y[k];
            argmin_pair(bd, bi, dx * dx + dy * dy, k);
        }
        wave_argmin(bd, bi);
        if (lane == 0) {
            s_rd[wave] = bd;
            s_ri[wave] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            double d = s_rd[0];
            int i = s_ri[0];
            for (int v = 1; v < kFinWaves; ++v) argmin_pair(d, i, s_rd[v], s_ri[v]);
            out_idx[qf] = i;
            out_d2[qf] = d;
            s_nd2[w] = d;
            if (out_pose) {
                out_pose[3 * qf] = X[i];
                out_pose[3 * qf + 1] = Y[i];
                out_pose[3 * qf + 2] = YAW[i];
            }
        }
        __syncthreads();
    }
    if (!cand) return;  // nearest-only launch (no window)
    FS(6)
    // ---- 2. window pairs
    {
        // wave w: sample j = q0 + w against the window samples i < j of the Morton cells its
        // disc of radius sqrt(D2) touches (the binning is monotone, so the cells are a superset)
        const int j = q0 + wave;
        if (j < W) {
            const double xj = qx[j], yj = qy[j];
            const float xjf = (float)xj, yjf = (float)yj;
            const double D2 = s_nd2[wave];
            const float df = __builtin_sqrtf((float)D2) + pg.slack;
            const float thr = df * df;
            const double R = sqrt(D2) * (1.0 + 1e-9) + 1e-9;
            const int cx0 = sample_cell(xj - R, pg.minx, pg.fx), cx1 = sample_cell(xj + R, pg.minx, pg.fx);
            const int cy0 = sample_cell(yj - R, pg.miny, pg.fy), cy1 = sample_cell(yj + R, pg.miny, pg.fy);
            for (int cy = cy0; cy <= cy1; ++cy) {
                for (int cx = cx0; cx <= cx1; ++cx) {
                    const int m = morton16(cx, cy);
                    const int a1 = pg.cofs[m + 1];
                    // (a candidate's index and f64 coordinates are read by sorted position,
                    // beside its f32 prefilter, not through perm)
                    for (int pos = pg.cofs[m] + lane; pos < a1; pos += 64) {
                        const float2 v = pg.sxy[pos];
                        const int ii = pg.perm[pos];
                        const double sx = pg.ssx[pos], sy = pg.ssy[pos];
                        if (!(scan_d2(xjf, yjf, v.x, v.y) <= thr)) continue;
                        if (ii >= j) continue;
                        const double dx = xj - sx, dy = yj - sy;
                        const double d2 = dx * dx + dy * dy;
                        if (d2 < D2) {  // strictly nearer than the snapshot NN (which wins ties)
                            const int at = atomicAdd(&s_pc[wave], 1);
                            if (at < kCandCap) {
                                s_pi[wave][at] = ii;
                                s_pd[wave][at] = d2;
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    FS(7)
    if (wave == 0) {
        const int j = q0 + lane;
        const bool jin = lane < kFinSamples && j < W;
        const int cnt = jin ? s_pc[lane] : 0;
        const int keep = min(cnt, kCandCap);
        if (jin) cand_cnt[j] = cnt;
        // one reservation per workgroup for the entries and for the queue of pending samples
        const int ex = wave_incl_scan(keep), pc = wave_incl_scan(cnt > 0 ? 1 : 0);
        const int eo = ex - keep, po = pc - (cnt > 0 ? 1 : 0);
        if (lane == 63) {
            s_pbase = ex > 0 ? atomicAdd(&st->ncomp, ex) : 0;
            s_pnb = pc > 0 ? atomicAdd(&st->npend, pc) : 0;
        }
        const uint64_t ov = __ballot(cnt > kCandCap);  // a list overflowed: the window stops there
        __builtin_amdgcn_wave_barrier();
        const int eb = s_pbase + eo, pb = s_pnb + po;
        for (int k = 0; k < keep; ++k)
            cand[eb + k] = CandEntry{j, s_pi[lane][k], s_pd[lane][k], 0.0, -1, 0};
        if (cnt > 0) pend[pb] = j;
        if (lane == 0 && ov) atomicMin(&st->weff, q0 + (int)__builtin_ctzll(ov));
        FS(8)
    }
}

// A resolve repair (one wave): the (child, parent pose) pair steered and collision-checked anew
// (only resolve_tail_kernel compiles it: inlined there it needs no scratch).
__device__ __forceinline__ int resolve_repair(const SceneDev& sc, double x, double y,
                                                        double yaw, double px, double py,
                                                        double pyaw, int lit, double* bx) {
    return lit ? steer_collide_literal(sc, x, y, yaw, px, py, pyaw, bx, bx + kLiteralCap,
                                       bx + 2 * kLiteralCap)
               : steer_collide_fast<false>(sc, x, y, yaw, px, py, pyaw);
}

// The sequential-consistency resolve of one window's PENDING samples, on one workgroup with its
// state in LDS.  A sample is pending when nn_finalize's pair search found an earlier window sample strictly
// nearer than its snapshot NN, or when its snapshot verdict is not final (literal path, error);
// every other sample is decided by its snapshot verdict and never touches the resolve.  The
// replay: sample j's parent is the first ACCEPTED entry of its candidate list in (d2, i) order,
// else its snapshot NN.  Output per pending j < weff: snap_status[j] = verdict | kWinParent
// (parent = window sample fin_par[j]), snap_yaw[j] = its final yaw.  commit_role then appends
// the window.
constexpr int kResolveEnt = 1024;  // candidate-list positions staged in LDS (the rest: rs.order)
struct ResolveLds {
    double yaw[kMaxWindow];          // slot: snapshot yaw, then a repair's, then the final one
    double ed[kResolveEnt];          // list position: d2 (the sort key), then the entry's yaw
    int j[kMaxWindow];               // slot -> sample
    int round[kMaxWindow];           // slot: decided flag (published last)
    int par[kMaxWindow];             // slot: -1 snapshot NN, else window sample index
    int off[kMaxWindow];             // slot: first list position
    int cnt[kMaxWindow];             // slot: list length (<= kCandCap); first the fill counter
    int ei[kResolveEnt];             // list position: candidate sample i
    int ee[kResolveEnt];             // list position: entry index into cand[]
    int ec[kResolveEnt];             // list position: i's slot, or -1 / -2 (rejected / accepted by
                                     // its snapshot verdict)
    short slot[kMaxWindow];          // sample -> pending slot, -1: decided by its snapshot
    signed char verdict[kMaxWindow]; // slot: snapshot status until decided, then 0/1
    signed char rep[kMaxWindow];     // slot: repair verdict (-1: none) | 16 if literal
    signed char es[kResolveEnt];     // list position: the entry's speculative status
    int total, err, bail;
    int stat[4];                     // repair passes, repairs, literal repairs, max passes of a wave
};

// kRepair = false (the window kernel): no repair code is compiled in (it would spill at the
// window kernel's 128-VGPR budget); a window that needs a repair returns false without
// publishing anything and resolve_tail_kernel redoes it with repairs.
template <bool kRepair, int NT>
__device__ __attribute__((always_inline)) inline bool resolve_role(
    DevState* __restrict__ st, const SceneDev& sc, const TreeDev& tr,
    const double* __restrict__ wsx, const double* __restrict__ wsy,
    const int* __restrict__ nn_idx, const int* __restrict__ cand_cnt,
    const CandEntry* __restrict__ cand, const int* __restrict__ pend,
    int* __restrict__ snap_status, double* __restrict__ snap_yaw, int* __restrict__ fin_par,
    ResolveScratch rs, double* __restrict__ lit_scratch, int W, char* smem) {
    constexpr int KW = kMaxWindow;
    constexpr int kEntLds = kResolveEnt;
    ResolveLds& L = *reinterpret_cast<ResolveLds*>(smem);
    auto& s_slot = L.slot;
    auto& s_j = L.j;
    auto& s_round = L.round;
    auto& s_par = L.par;
    auto& s_yaw = L.yaw;
    auto& s_off = L.off;
    auto& s_cnt = L.cnt;
    auto& s_verdict = L.verdict;
    auto& s_rep = L.rep;
    auto& s_ei = L.ei;
    auto& s_ee = L.ee;
    auto& s_ec = L.ec;
    auto& s_ed = L.ed;
    auto& s_es = L.es;
    auto& s_total = L.total;
    auto& s_err = L.err;
    auto& s_stat = L.stat;
    auto& s_bail = L.bail;
    const int Weff = min(W, st->weff);
    const int npend = min(st->npend, KW);
    const int ncomp = st->ncomp;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (tid < 4) s_stat[tid] = 0;
    if (tid == 0) {
        s_total = 0;
        s_err = 0;
        s_bail = 0;
    }
    for (int j = tid; j < W; j += NT) s_slot[j] = -1;
    __syncthreads();
    // 1. slots: every load of the pass is issued before any of them is used
    for (int q = tid; q < npend; q += NT) {
        const int j = pend[q];
        const int c = cand_cnt[j];
        const int ss = snap_status[j];
        const double sy = snap_yaw[j];
        s_slot[j] = (short)q;
        s_j[q] = j;
        s_round[q] = 0;
        const int k = min(c, kCandCap);
        s_off[q] = atomicAdd(&s_total, k);
        s_cnt[q] = 0;
        s_verdict[q] = (signed char)ss;
        s_yaw[q] = sy;
        s_rep[q] = -1;
    }
    __syncthreads();
    // 2. lists: each entry goes to its sample's segment (then sorted by (d2, i))
    for (int e = tid; e < ncomp; e += NT) {
        const CandEntry ce = cand[e];
        const int q = s_slot[ce.j];
        const int k = s_off[q] + atomicAdd(&s_cnt[q], 1);
        const int qi = s_slot[ce.i];
        const int code = qi >= 0 ? qi : (snap_status[ce.i] == kAccept ? -2 : -1);
        if (k < kEntLds) {
            s_ei[k] = ce.i;
            s_ee[k] = e;
            s_ec[k] = code;
            s_ed[k] = ce.d2;
        } else {
            rs.order[k] = e;
        }
    }
    __syncthreads();
    auto ent_e = [&](int k) { return k < kEntLds ? s_ee[k] : rs.order[k]; };
    auto ent_i = [&](int k) { return k < kEntLds ? s_ei[k] : cand[rs.order[k]].i; };
    auto ent_c = [&](int k) {
        if (k < kEntLds) return s_ec[k];
        const int i = cand[rs.order[k]].i;
        const int qi = s_slot[i];
        return qi >= 0 ? qi : (snap_status[i] == kAccept ? -2 : -1);
    };
    for (int q = tid; q < npend; q += NT) {  // insertion sort of each list by (d2, i)
        const int o = s_off[q], k = s_cnt[q];
        if (o + k > kEntLds) continue;  // lists past the LDS part: sorted below (global)
        for (int a2 = 1; a2 < k; ++a2) {
            const double d = s_ed[o + a2];
            const int ii = s_ei[o + a2], ee = s_ee[o + a2], cc = s_ec[o + a2];
            int b2 = a2 - 1;
            while (b2 >= 0 && (s_ed[o + b2] > d || (s_ed[o + b2] == d && s_ei[o + b2] > ii))) {
                s_ed[o + b2 + 1] = s_ed[o + b2];
                s_ei[o + b2 + 1] = s_ei[o + b2];
                s_ee[o + b2 + 1] = s_ee[o + b2];
                s_ec[o + b2 + 1] = s_ec[o + b2];
                --b2;
            }
            s_ed[o + b2 + 1] = d;
            s_ei[o + b2 + 1] = ii;
            s_ee[o + b2 + 1] = ee;
            s_ec[o + b2 + 1] = cc;
        }
    }
    for (int q = tid; q < npend; q += NT) {  // the rare lists that straddle or pass kEntLds
        const int o = s_off[q], k = s_cnt[q];
        if (o + k <= kEntLds) continue;
        // materialise the whole list in rs.order, then sort it there
        for (int a2 = 0; a2 < k; ++a2)
            if (o + a2 < kEntLds) rs.order[o + a2] = s_ee[o + a2];
        for (int a2 = 1; a2 < k; ++a2) {
            const int e = rs.order[o + a2];
            const double d = cand[e].d2;
            const int ii = cand[e].i;
            int b2 = a2 - 1;
            while (b2 >= 0) {
                const int eb = rs.order[o + b2];
                if (cand[eb].d2 < d || (cand[eb].d2 == d && cand[eb].i < ii)) break;
                rs.order[o + b2 + 1] = eb;
                --b2;
            }
            rs.order[o + b2 + 1] = e;
        }
        for (int a2 = 0; a2 < k && o + a2 < kEntLds; ++a2) {  // refresh the LDS part
            const int e = rs.order[o + a2];
            const int i = cand[e].i;
            const int qi = s_slot[i];
            s_ee[o + a2] = e;
            s_ei[o + a2] = i;
            s_ed[o + a2] = cand[e].d2;
            s_ec[o + a2] = qi >= 0 ? qi : (snap_status[i] == kAccept ? -2 : -1);
        }
    }
    __syncthreads();
    for (int k = tid; k < min(s_total, kEntLds); k += NT) {  // the entries' speculative verdicts
        const int e = s_ee[k];
        const int es = cand[e].status;
        const double ey = cand[e].yaw;
        s_es[k] = (signed char)es;
        s_ed[k] = ey;
    }
    __syncthreads();
    // 3. decisions, without workgroup barriers: every wave passes over its own slots until all of
    //    them are decided, reading the other slots' decisions from LDS as they appear.  A decision
    //    is final once published (its flag is stored last, with release order), and every
    //    dependency points to an earlier sample, so the earliest undecided slot can always be
    //    decided: the passes terminate.  A pair nobody speculated on is re-steered by the wave
    //    that owns the slot, between its passes.
    int64_t n_rounds_rep = 0, n_rep = 0, n_lit = 0, n_rounds = 0;
    for (int pass = 0; pass < (1 << 20); ++pass) {
        ++n_rounds;
        bool left = false;
        int rq = -1, rpar = -1, rlit = 0;  // this lane's repair request (one per pass)
        for (int q = tid; q < npend; q += NT) {
            if (__hip_atomic_load(&s_round[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
                continue;
            const int j = s_j[q];
            if (j >= Weff) continue;
            int parent = -1, pos = -1, pq = -1;
            bool blocked = false;
            const int k = s_cnt[q], o = s_off[q];
            int a2 = 0;
            for (; a2 < k; ++a2) {
                const int code = ent_c(o + a2);
                if (code >= 0) {
                    if (!__hip_atomic_load(&s_round[code], __ATOMIC_ACQUIRE,
                                           __HIP_MEMORY_SCOPE_WORKGROUP)) {
                        blocked = true;  // an earlier candidate is still undecided
                        break;
                    }
                    if (!s_verdict[code]) continue;
                } else if (code == -1) {
                    continue;
                }
                parent = ent_i(o + a2);
                pos = o + a2;
                pq = code;
                break;
            }
            if (blocked) {
                // the entries before the blocker are final rejections: the next pass starts at
                // the blocker (only this thread touches slot q's list bounds in the passes)
                s_off[q] = o + a2;
                s_cnt[q] = k - a2;
                left = true;
                continue;
            }
            int status = -1, lit_done = 0;
            double y = 0.0;
            const int rp = s_rep[q];
            if (rp >= 0) {
                status = rp & 15;
                lit_done = rp >> 4;
                y = s_yaw[q];
            } else if (parent < 0) {
                status = s_verdict[q];
                y = s_yaw[q];
            } else if (pq < 0 || s_par[pq] < 0) {  // parent kept its snapshot parent: speculated
                if (pos < kEntLds) {
                    status = s_es[pos];
                    y = s_ed[pos];
                } else {
                    const int e = ent_e(pos);
                    status = cand[e].status;
                    y = cand[e].yaw;
                }
            }
            if (status < 0 || (status == kLiteral && !lit_done)) {
                left = true;
                if (rq < 0) {
                    rq = q;
                    rpar = parent;
                    rlit = status == kLiteral;
                }
                continue;
            }
            if (status != kAccept && status != kReject) s_err = 1;  // kError
            s_verdict[q] = status == kAccept;
            s_par[q] = parent;
            s_yaw[q] = y;
            __hip_atomic_store(&s_round[q], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        // repairs requested by this wave's lanes, one wave-wide steer each
        uint64_t m = __ballot(rq >= 0);
        if constexpr (!kRepair) {
            if (m && lane == 0) s_bail = 1;
            if (__hip_atomic_load(&s_bail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        } else {
            if (m) ++n_rounds_rep;
            while (m) {
                const int l = (int)__builtin_ctzll(m);
                m &= m - 1;
                const int q = __shfl(rq, l), p = __shfl(rpar, l), lit = __shfl(rlit, l);
                const int j = s_j[q];
                const double x = wsx[j], y = wsy[j];
                double px, py, pyaw;
                if (p < 0) {
                    const int nq = nn_idx[j];
                    px = tr.x[nq];
                    py = tr.y[nq];
                    pyaw = tr.yaw[nq];
                } else {
                    px = wsx[p];
                    py = wsy[p];
                    const int pq = s_slot[p];
                    pyaw = pq >= 0 ? s_yaw[pq] : snap_yaw[p];
                }
                const double yaw = atan2(py - y, px - x);
                double* bx = lit_scratch + (size_t)wave * 3 * kLiteralCap;
                const int sres = resolve_repair(sc, x, y, yaw, px, py, pyaw, lit, bx);
                if (lane == 0) {
                    s_rep[q] = (signed char)(sres | (lit << 4));
                    s_yaw[q] = yaw;
                }
                ++n_rep;
                n_lit += lit;
            }
        }
        if (!__any(left)) break;
    }
    if (lane == 0) {  // per-wave statistics (wave-uniform values)
        atomicAdd(&s_stat[0], (int)n_rounds_rep);
        atomicAdd(&s_stat[1], (int)n_rep);
        atomicAdd(&s_stat[2], (int)n_lit);
        atomicMax(&s_stat[3], (int)n_rounds);
    }
    __syncthreads();
    if (!kRepair && s_bail) return false;
    // 4. publish the pending verdicts for window_commit
    for (int q = tid; q < npend; q += NT) {
        const int j = s_j[q];
        if (j >= Weff) continue;
        const int p = s_par[q];
        snap_status[j] = (s_verdict[q] ? kAccept : kReject) | (p >= 0 ? kWinParent : 0);
        snap_yaw[j] = s_yaw[q];
        fin_par[j] = p;
    }
    if (tid == 0) {
        if (s_err) st->error = 1;
        st->repair_rounds += s_stat[0];
        st->repairs += s_stat[1];
        st->literal_repairs += s_stat[2];
    }
    return true;
}

// Append the window (rrt.rs:586-589): the accepted samples j < weff get consecutive node indices
// in iteration order (a prefix sum of the verdict words in LDS, so a window parent's node index is
// known), then DevState advances.  A truncated window (weff < W) restarts the next window at
// sample weff: the window screened concurrently (seq) is void.
template <int NT>
__device__ __attribute__((always_inline)) inline void commit_role(
    DevState* __restrict__ st, const TreeDev& tr, const double* __restrict__ wsx,
    const double* __restrict__ wsy, const int* __restrict__ nn_idx,
    const int* __restrict__ snap_status, const double* __restrict__ snap_yaw,
    const int* __restrict__ fin_par, int* __restrict__ cand_cnt, int W, int64_t void_next,
    int64_t screened, const SampleRec& hrec, const int* __restrict__ iter_off, int span,
    char* smem) {
    constexpr int PER = kMaxWindow / NT;
    static_assert(PER % 4 == 0, "commit: whole int4 loads per thread");
    int* s_node = reinterpret_cast<int*>(smem);
    int* s_wave = s_node + kMaxWindow;
    const int Weff = min(W, st->weff);
    const int n0 = st->n;
    const int64_t it0 = st->it;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int j0 = tid * PER;
    int v[PER];
    if (j0 + PER <= Weff) {
#pragma unroll
        for (int u = 0; u < PER; u += 4) {
            const int4 w4 = *reinterpret_cast<const int4*>(snap_status + j0 + u);
            v[u] = w4.x;
            v[u + 1] = w4.y;
            v[u + 2] = w4.z;
            v[u + 3] = w4.w;
        }
    } else {
#pragma unroll
        for (int u = 0; u < PER; ++u) v[u] = j0 + u < Weff ? snap_status[j0 + u] : 0;
    }
    int local = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) local += v[u] & 1;
    const int x = wave_incl_scan(local);
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        base += w < wave ? s_wave[w] : 0;
        total += s_wave[w];
    }
    int node = n0 + base + x - local;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        s_node[j0 + u] = node;
        node += v[u] & 1;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int j = j0 + u;
        if (j < Weff && (v[u] & 1)) {
            const int nd = s_node[j];
            const double xx = wsx[j], yy = wsy[j];
            tr.x[nd] = xx;
            tr.y[nd] = yy;
            tr.x32[nd] = (float)xx;
            tr.y32[nd] = (float)yy;
            tr.yaw[nd] = snap_yaw[j];
            tr.parent[nd] = (v[u] & kWinParent) ? s_node[fin_par[j]] : nn_idx[j];
        }
        if (j < W) cand_cnt[j] = 0;  // the next window's pair counts start at zero
    }
    if (hrec.par || hrec.yaw || hrec.ok) {  // pp_rrt_extend_samples: every committed iteration
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int j = j0 + u;
            if (j >= Weff) continue;
            const int64_t r = it0 + iter_off[j] - hrec.base;
            if (hrec.ok) hrec.ok[r] = (unsigned char)(v[u] & 1);
            if (hrec.par) hrec.par[r] = (v[u] & kWinParent) ? s_node[fin_par[j]] : nn_idx[j];
            if (hrec.yaw) hrec.yaw[r] = snap_yaw[j];
        }
    }
    if (tid == 0) {
        // the iterations committed: the whole span, or, cut at sample Weff, up to that sample's
        // iteration (the draws in an obstacle before it were settled when they were drawn)
        const int adv = Weff < W ? iter_off[Weff] : span;
        st->n = n0 + total;
        st->it = it0 + adv;
        st->iterations += adv;
        st->blocked += adv - Weff;
        st->accepted += total;
        st->windows += 1;
        st->truncations += Weff < W;
        st->nn_flagged += st->flag_count;
        // the screen's distance evaluations: the samples it covered (not in an obstacle) x the
        // tree nodes it scanned (nodes past n_scan are nn_finalize's, a few per window)
        st->node_evals += screened;
        if (Weff < W) {
            st->it_spec = it0 + adv;
            if (void_next >= 0) st->void_seq = void_next;
        }
        // adaptive window (a young tree: the window's samples are mostly nearer to each other than
        // to the tree, lists overflow and windows are cut): a cut window shrinks the next draws to
        // the power of two at or above where it stopped, a full one doubles them (<= K, clamped by
        // the draws).  kdyn counts samples, not iterations.  Only the speed depends on it: the results are those of one sample at a time.
        int kd = st->kdyn > 0 ? st->kdyn : kMaxWindow;
        if (Weff < W) {
            kd = kMinDynWindow;
            while (kd < Weff) kd <<= 1;
        } else if (W >= kd) {
            kd = min(2 * kd, kMaxWindow);
        }
        st->kdyn = kd;
    }
}

// The window kernel: workgroup 0 resolves and commits the previous window (or, in the drain
// launch, the batch's last one) while workgroups 1.. screen this window's samples.  One LDS image
// serves the role of each workgroup (ResolveLds / the commit prefix / the screen's wave merge).
constexpr int kWinLds = (int)sizeof(ResolveLds);
static_assert(kWinLds <= 160 * 1024, "window kernel LDS");
static_assert((int)((3 * kScanWaves + 1) * kQPB * 4) <= kWinLds, "screen merge fits the LDS image");
static_assert(kSamplesLds <= kWinLds, "samples_role fits the window kernel's LDS image");
static_assert(kScreenStageOff % 16 == 0 && kScreenStageOff + 3 * kStage * 4 + 16 <= kWinLds,
              "screen staging (x, y, |n-o|^2 of kStage nodes) fits");
static_assert(kStage % 256 == 0, "whole DMA quarters");


__global__ __launch_bounds__(kScanThreads) void window_kernel(WinKArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kWinLds];
    if (blockIdx.x == 0) {
        DevState* st = a.st;
        if (a.resolve) {
            const int W = st->W;
            // (a window of draws in obstacles alone has no sample and still commits its span)
            if (st->span_cur > 0) {
                const int q = 1 - a.p;
                if (W > 0 && !resolve_role<kWinRepair, kScanThreads>(st, a.sc, a.tr, a.wsx[q], a.wsy[q], a.nn_idx,
                                                       a.cand_cnt, a.cand, a.pend, a.snap_status,
                                                       a.snap_yaw, a.fin_par, a.rs, a.lit_scratch,
                                                       W, smem)) {
                    if (threadIdx.x == 0) st->resolve_bail = 1;  // resolve_tail_kernel redoes it
                    return;
                }
                // (same workgroup: the barrier's workgroup-scope fence orders these stores)
                __syncthreads();
                commit_role<kScanThreads>(st, a.tr, a.wsx[q], a.wsy[q], a.nn_idx, a.snap_status,
                                          a.snap_yaw, a.fin_par, a.cand_cnt, W,
                                          a.scan ? a.seq : -1,
                                          (int64_t)st->Wsp[q] * st->nsp[q], a.hrec,
                                          a.g.iter_off[q], st->span_cur, smem);
            }
        }
        if (threadIdx.x == 0) {  // the screened window's counters start at zero
            st->flag_count = 0;
            st->ncomp = 0;
            st->npend = 0;
            // no cut yet: nn_finalize's workgroups lower it with atomicMin in any order (a plain
            // store there raced with the early finishers)
            st->weff = 0x7fffffff;
        }
        return;
    }
    if (a.scan) {
        if (a.gen)
            scan_role<true>(a, (int)blockIdx.x - 1, smem);
        else
            scan_role<false>(a, (int)blockIdx.x - 1, smem);
    }
}

// The resolve + commit of a window whose resolve in the window kernel needed a repair (a pair
// nobody speculated on, or the literal path): redone here with the repairs, at kResolveThreads
// (256 VGPRs each, no spill).  A no-op launch otherwise.
__global__ __launch_bounds__(kResolveThreads) void resolve_tail_kernel(WinKArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kWinLds];
    DevState* st = a.st;
    if (!st->resolve_bail) return;
    const int q = 1 - a.p;
    const int W = st->W;
    resolve_role<true, kResolveThreads>(st, a.sc, a.tr, a.wsx[q], a.wsy[q], a.nn_idx, a.cand_cnt,
                                         a.cand, a.pend, a.snap_status, a.snap_yaw, a.fin_par,
                                         a.rs, a.lit_scratch, W, smem);
    // (same workgroup: the barrier's workgroup-scope fence orders these stores)
    __syncthreads();
    commit_role<kResolveThreads>(st, a.tr, a.wsx[q], a.wsy[q], a.nn_idx, a.snap_status,
                                 a.snap_yaw, a.fin_par, a.cand_cnt, W, a.scan ? a.seq : -1,
                                 (int64_t)st->Wsp[q] * st->nsp[q], a.hrec, a.g.iter_off[q],
                                 st->span_cur, smem);
    if (threadIdx.x == 0) {
        st->resolve_bail = 0;
        st->flag_count = 0;
        st->ncomp = 0;
        st->npend = 0;
        st->weff = 0x7fffffff;
    }
}

// --------------------------------------------------------------------------- launch wrappers

namespace {
SamplesArgs samples_args(const WindowArgs& a) {
    SamplesArgs g;
    g.K = a.K;
    g.target = a.target;
    g.seed = a.seed;
    g.minx = a.sc.minx;
    g.maxx = a.sc.maxx;
    g.miny = a.sc.miny;
    g.maxy = a.sc.maxy;
    for (int q = 0; q < 2; ++q) {
        g.wsx[q] = a.wsx + (size_t)q * a.Kcap;
        g.wsy[q] = a.wsy + (size_t)q * a.Kcap;
        g.wsx32[q] = a.wsx32 + (size_t)q * a.Kcap;
        g.wsy32[q] = a.wsy32 + (size_t)q * a.Kcap;
        g.perm[q] = a.perm + (size_t)q * a.Kcap;
        g.cofs[q] = a.cofs + (size_t)q * 257;
        g.sxy[q] = a.sxy + (size_t)q * a.Kcap;
        g.ssx[q] = a.ssx + (size_t)q * a.Kcap;
        g.ssy[q] = a.ssy + (size_t)q * a.Kcap;
        g.ob[q] = a.ob + (size_t)q * (kMaxWindow / kQPB);
        g.sq[q] = a.sq + (size_t)q * a.Kcap;
        g.ipos[q] = a.ipos + (size_t)q * a.Kcap;
        g.iter_off[q] = a.iter_off + (size_t)q * a.Kcap;
    }
    g.scp = a.scp;
    g.hsx = a.hsx;
    g.hsy = a.hsy;
    g.hs_base = a.hrec.base;
    g.hok = a.hrec.ok;
    g.pretest = a.pretest;
    return g;
}
PairGrid pair_grid(const SamplesArgs& g, int p, double eps_coord) {
    PairGrid r;
    r.perm = g.perm[p];
    r.cofs = g.cofs[p];
    r.sxy = g.sxy[p];
    r.ssx = g.ssx[p];
    r.ssy = g.ssy[p];
    r.minx = g.minx;
    r.miny = g.miny;
    r.fx = 16.0 / (g.maxx - g.minx);  // samples_role's factors, bit for bit
    r.fy = 16.0 / (g.maxy - g.miny);
    // f32 rounding of both samples' coordinates (and of the distance arithmetic)
    r.slack = (float)(5.0e-4 + 4.0 * eps_coord);
    return r;
}

WinKArgs win_args(const WindowArgs& a, int p, int gen, int resolve, int scan, int64_t seq) {
    WinKArgs k;
    k.st = a.st;
    k.sc = a.sc;
    k.tr = a.tr;
    k.K = a.K;
    k.Kcap = a.Kcap;
    k.nqb = (a.K + kQPB - 1) / kQPB;
    k.chunks = scan_chunks(a.K);
    k.p = p;
    k.gen = gen;
    k.resolve = resolve;
    k.scan = scan;
    k.seq = seq;
    k.target = a.target;
    k.seed = a.seed;
    k.wsx[0] = a.wsx;
    k.wsx[1] = a.wsx + a.Kcap;
    k.wsy[0] = a.wsy;
    k.wsy[1] = a.wsy + a.Kcap;
    k.wsx32[0] = a.wsx32;
    k.wsx32[1] = a.wsx32 + a.Kcap;
    k.wsy32[0] = a.wsy32;
    k.wsy32[1] = a.wsy32 + a.Kcap;
    k.perm[0] = a.perm;
    k.perm[1] = a.perm + a.Kcap;
    k.sq[0] = a.sq;
    k.sq[1] = a.sq + a.Kcap;
    k.pbest = a.pbest;
    k.psecond = a.psecond;
    k.pidx = a.pidx;
    k.nn_idx = a.nn_idx;
    k.cand_cnt = a.cand_cnt;
    k.cand = a.cand;
    k.pend = a.pend;
    k.snap_status = a.snap_status;
    k.snap_yaw = a.snap_yaw;
    k.fin_par = a.fin_par;
    k.rs = a.rs;
    k.lit_scratch = a.lit_scratch;
    k.gen_next = gen && scan;
    k.g = samples_args(a);
    k.hrec = a.hrec;
    return k;
}
}  // namespace


hipError_t launch_window(hipStream_t s, const WindowArgs& a, hipEvent_t* ev, int64_t seq,
                         int resolve_prev) {
    const int K = a.K;
    const int p = (int)(seq & 1);
    const WinKArgs wk = win_args(a, p, 1, resolve_prev, 1, seq);
    if (!resolve_prev)  // the batch's first window: its samples (later: the previous window's draw)
        window_samples_kernel<<<1, 1024, 0, s>>>(a.st, wk.g, p);
    double* wsx = a.wsx + (size_t)p * a.Kcap;
    double* wsy = a.wsy + (size_t)p * a.Kcap;
    if (ev) (void)hipEventRecord(ev[0], s);
    // (the screen's geometry is decided on the device, from the samples not in an obstacle:
    // every workgroup past it returns at once)
    window_kernel<<<1 + kScanGrid, kScanThreads, 0, s>>>(wk);
    if (resolve_prev && !kWinRepair) resolve_tail_kernel<<<1, kResolveThreads, 0, s>>>(wk);
    if (ev) (void)hipEventRecord(ev[1], s);
    // one workgroup past the samples' draws the next window's samples
    nn_finalize_kernel<<<(K + kFinSamples - 1) / kFinSamples + 1, kFinThreads, 0, s>>>(
        a.st, p, seq, wk.chunks, a.pbest, a.psecond, a.pidx, a.Kcap, wsx, wsy, a.tr.x32, a.tr.y32,
        a.tr.x, a.tr.y, a.tr.yaw, a.eps_coord, a.nn_idx, a.nn_d2, a.snap_pose,
        pair_grid(wk.g, p, a.eps_coord), a.cand_cnt, a.cand, a.pend, wk.sq[p], wk.g.ipos[p], wk.g,
        1);
    if (ev) (void)hipEventRecord(ev[2], s);
    // snapshot and candidate tasks together: prep covers 2K tasks per pass, walk 4 per workgroup
    const int prep_blocks = (2 * K + kPrepThreads / 8 - 1) / (kPrepThreads / 8);
    launch_prep_window(s, prep_blocks, a.st, a.sc, wsx, wsy, a.snap_pose, a.cand, a.rec,
                       a.snap_yaw);
    if (ev) (void)hipEventRecord(ev[3], s);
    // snapshot tasks plus the usual few candidate tasks in one round of waves
    const int nwg = walk_blocks(K + K / 4, walk_grid_limit(kWalkWindow, a.sc));
    launch_walk(kWalkWindow, s, nwg, a.st, a.sc, a.rec, a.cand, a.snap_status, a.cand_cnt, a.pend,
                a.wg_points);
    if (ev) (void)hipEventRecord(ev[4], s);
    return hipGetLastError();
}

hipError_t launch_drain(hipStream_t s, const WindowArgs& a, int64_t seq_next) {
    const WinKArgs wk = win_args(a, (int)(seq_next & 1), 1, 1, 0, seq_next);
    window_kernel<<<1, kScanThreads, 0, s>>>(wk);
    if (!kWinRepair) resolve_tail_kernel<<<1, kResolveThreads, 0, s>>>(wk);
    return hipGetLastError();
}

hipError_t launch_nearest(hipStream_t s, const WindowArgs& a) {
    const int K = a.K;
    const WinKArgs wk = win_args(a, 0, 0, 0, 1, 0);
    window_kernel<<<1 + wk.nqb * wk.chunks, kScanThreads, 0, s>>>(wk);
    nn_finalize_kernel<<<(K + kFinSamples - 1) / kFinSamples, kFinThreads, 0, s>>>(
        a.st, 0, 0, wk.chunks, a.pbest, a.psecond, a.pidx, a.Kcap, a.wsx, a.wsy, a.tr.x32,
        a.tr.y32, a.tr.x, a.tr.y, a.tr.yaw, a.eps_coord, a.nn_idx, a.nn_d2, nullptr, PairGrid{},
        nullptr, nullptr, nullptr, nullptr, nullptr, wk.g, 0);
    return hipGetLastError();
}


}  // namespace ppamd

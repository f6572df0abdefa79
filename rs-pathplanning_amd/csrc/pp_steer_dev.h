// pp_steer_dev.h — device code that more than one kernel unit (pp_k_*.hip) inlines into its own
// kernels: the collision chunk test and the scene's LDS image, the analytic S-segment classes,
// steer_prep / steer_walk on one wave, the literal path, the per-task prep (prep_task) and the
// record walk (walk_rec, walk_edge), the literal scratch pool's locks and argmin_pair.
//
// Only templates and inline functions: no __global__ and no out-of-line __device__ function
// (every unit is its own code object, and two definitions would collide when the host objects
// link).  The single exception is one device variable, kSinCosTab, walk_rec's sincos constants:
// it is static, so every unit that includes this header carries its own 136-byte copy under an
// internal name.  Included by the .hip units only, never by the host .cpp files.
#pragma once

#include <hip/hip_runtime.h>

#include "pp_device.h"
#include "pp_types.h"

namespace ppamd {

// ------------------------------------------------------------------------------ collision

// One 64-point chunk of a polyline, one point per lane: bounds for the lanes flagged
// `check_bounds`, then the segment (lane-1 → lane) of every lane flagged `seg_valid` against the
// discs listed in the grid cells the chunk's bounding box touches (Space::verify,
// rrt.rs:124-137, Q10).  A disc whose cull box meets the chunk's box shares a cell with it (the
// cell index is monotone in the coordinate), so the cull is exact.  Must be called by all 64
// lanes.  Returns true when the chunk rejects the line.
// (the clamp in the integer domain: v_cvt_i32_f64 saturates — NaN gives 0 — so no f64 bound has
// to stay live in the walk's registers; the same cell as clamping the double)
__device__ inline int grid_cell(double v, double v0, double inv, int n) {
    const double f = floor((v - v0) * inv);
    int i;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(i) : "v"(f));
    return min(max(i, 0), n - 1);
}

// Dynamic LDS of the steer kernels: the scene image (SceneDev::lds_*) when kLds.
extern __shared__ __attribute__((aligned(16))) char pp_smem[];

// Copy the scene's LDS image (disc grid + discs, or the occupancy bits) into this workgroup's LDS
// (all threads call it): 16-byte words, 8 loads in flight per thread before their stores.
__device__ inline void stage_scene(const SceneDev& sc) {
    constexpr int U = 8;
    const int n16 = sc.lds_bytes >> 4;
    uint4* dst = reinterpret_cast<uint4*>(pp_smem);
    const int nt = blockDim.x;
    for (int base = threadIdx.x; base < n16; base += nt * U) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {  // unconditional (clamped) loads: all U stay in flight
            const int k = min(base + u * nt, n16 - 1);
            v[u] = sc.img[k];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = base + u * nt;
            if (k < n16) dst[k] = v[u];
        }
    }
    __syncthreads();
}

// The scene modes a walk can be compiled for: kSceneAny tests the SceneDev fields at run time;
// the others drop the code (and the kernel-argument registers) of the modes they exclude.
enum : int { kSceneAny = 0, kSceneDisc = 1, kSceneGrid = 2, kScenePoly = 3 };
__host__ __device__ inline int scene_kind(const SceneDev& sc) {
    if (sc.bits) return kSceneGrid;
    if (sc.ne > 0 || sc.nbv > 0) return kScenePoly;
    return kSceneDisc;
}

// box: the lane's point bounds the chunk's item search (default: every lane with a point; the
// walk leaves out lane 0 when its segment 0 -> 1 is an analytically cleared S chord, which is not
// tested, so the box need not cover it)
template <bool kLds, int kScene = kSceneAny>
__device__ __forceinline__ bool chunk_rejects(const SceneDev& sc, bool has, bool check_bounds,
                                              bool seg_valid, double qx, double qy,
                                              bool box = true) {
    bool oob =
        check_bounds && !(qx >= sc.minx && qx <= sc.maxx && qy >= sc.miny && qy <= sc.maxy);
    if (__any(oob)) return true;
    if ((kScene == kSceneAny || kScene == kScenePoly) && sc.nbv > 0) {
        // polygon bounds (Q10p): the eroded ring, per lane over every bounds edge
        oob = check_bounds && !in_poly_bounds(sc.nbv, sc.bvx, sc.bvy, sc.h2, qx, qy);
        if (__any(oob)) return true;
    }
    if (kScene == kSceneGrid || (kScene == kSceneAny && sc.bits)) {
        // config 4: every point of the line probes its cell (1 bit), no segments
        const uint32_t* B = kLds ? reinterpret_cast<const uint32_t*>(pp_smem) : sc.bits;
        const bool hit = check_bounds && grid_occupied(B, sc.bw, sc.bh, sc.bwords, sc.bx0, sc.by0,
                                                       sc.binv, qx, qy);
        return __any(hit);
    }
    if (kScene == kSceneDisc ? sc.m == 0
                             : (kScene == kScenePoly ? sc.ne == 0 : (sc.m == 0 && sc.ne == 0)))
        return false;
    // grid items are polygon edges (Q10p), else discs
    const bool poly = kScene == kScenePoly || (kScene == kSceneAny && sc.ne > 0);
    // the chunk's bounding box in f32, rounded outward (DPP reductions): a box that contains the
    // points selects a superset of the cells and items, and the exact test below decides
    const double ax = shfl_up1_f64(qx);
    const double ay = shfl_up1_f64(qy);
    const float inff = __builtin_inff();
    const bool inb = has && box;
    const float bx0 = wave_min_f32(inb ? f32_below(qx) : inff);
    const float bx1 = wave_max_f32(inb ? f32_above(qx) : -inff);
    const float by0 = wave_min_f32(inb ? f32_below(qy) : inff);
    const float by1 = wave_max_f32(inb ? f32_above(qy) : -inff);
    const int cx0 = __builtin_amdgcn_readfirstlane(grid_cell(bx0, sc.gx0, sc.ginv, sc.gnx));
    const int cx1 = __builtin_amdgcn_readfirstlane(grid_cell(bx1, sc.gx0, sc.ginv, sc.gnx));
    const int cy0 = __builtin_amdgcn_readfirstlane(grid_cell(by0, sc.gy0, sc.ginv, sc.gny));
    const int cy1 = __builtin_amdgcn_readfirstlane(grid_cell(by1, sc.gy0, sc.ginv, sc.gny));
    const int* goff = kLds ? reinterpret_cast<const int*>(pp_smem + sc.lds_goff) : sc.goff;
    const int* items = kLds ? reinterpret_cast<const int*>(pp_smem + sc.lds_items) : sc.gitems;
    const double* dcx = sc.cx;  // exact test: f64 discs from global memory (L2)
    const double* dcy = sc.cy;
    const double* dr2 = sc.r2;
    // the cull discs are in the LDS image too unless the scene only fit without them (lds_d4 < 0)
    const float4* d4 = (kLds && sc.lds_d4 >= 0)
                           ? reinterpret_cast<const float4*>(pp_smem + sc.lds_d4)
                           : sc.d4;
    // per-lane f32 cull: a segment a-b can only touch a disc / an edge buffer (exact test below)
    // if |a - c| <= rcull + |b - a| (c: the disc centre / the edge midpoint, rcull: the radius /
    // half length + h); cull_slack covers the f32 rounding of the scene's coordinates
    const float axf = (float)ax, ayf = (float)ay;
    const float vxf = (float)(qx - ax), vyf = (float)(qy - ay);
    const float l2f = vxf * vxf + vyf * vyf;
    const float Lf = __builtin_sqrtf(l2f) * 1.000001f + sc.cull_slack;
    // the closest-point parameter below uses 1 / |b - a|^2 (one reciprocal per lane and chunk, not
    // a division per item): t is only approximate anyway — any t in [0, 1] gives a point of the
    // segment, so "surely within" stays exact, and the error of "surely clear" is second order in
    // the error of t (t minimises the distance), far inside the band
    const float il2f = l2f > 0.0f ? __builtin_amdgcn_rcpf(l2f) : 0.0f;
    // the chunk's bbox in f32, widened by the rounding slack: an item whose cull disc misses it
    // cannot meet any of the chunk's segments
    const int lane = __lane_id();
    const float bxl = (float)bx0 - sc.cull_slack, bxh = (float)bx1 + sc.cull_slack;
    const float byl = (float)by0 - sc.cull_slack, byh = (float)by1 + sc.cull_slack;
    // up to 64 items in parallel, one per lane (kk: its index in the item list, valid: a lane with
    // an item): the cull disc against the chunk's bbox, then the survivors against every lane's
    // segment, one at a time
    auto items_reject = [&](bool valid, int kk) -> bool {
        int dl = 0;
        float4 Dl = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool ov = false;
        if (valid) {
            dl = items[kk];
            Dl = d4[dl];
            ov = Dl.x + Dl.z >= bxl && Dl.x - Dl.z <= bxh && Dl.y + Dl.z >= byl && Dl.y - Dl.z <= byh;
        }
        for (uint64_t m = __ballot(ov); m; m &= m - 1) {
            const int src = (int)__builtin_ctzll(m);
            const int d = __builtin_amdgcn_readlane(dl, src);
            float4 D;
            D.x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Dl.x), src));
            D.y = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Dl.y), src));
            D.z = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Dl.z), src));
            D.w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Dl.w), src));
            const float dxf = D.x - axf, dyf = D.y - ayf, thr = D.z + Lf;
            bool near = seg_valid && dxf * dxf + dyf * dyf <= thr * thr;
            if (!__any(near)) continue;
            if (!poly) {
                // f32 closest point of the segment to the disc centre, decisive outside a band of
                // +-eps around the radius (eps bounds the f32 rounding of the coordinates, the
                // radius and this arithmetic): only the band needs the exact f64 test and its
                // global loads
                const float t =
                    __builtin_fminf(__builtin_fmaxf((dxf * vxf + dyf * vyf) * il2f, 0.0f), 1.0f);
                const float ex = dxf - t * vxf, ey = dyf - t * vyf;
                const float e2 = ex * ex + ey * ey;
                const float eps = sc.cull_slack + 1.0e-4f * (1.0f + thr);
                const float lo = __builtin_fmaxf(D.w - eps, 0.0f), hi = D.w + eps;
                if (__any(near && e2 < lo * lo)) return true;  // surely within the disc
                near = near && e2 <= hi * hi;                  // else surely clear
                if (!__any(near)) continue;
            }
            const bool hit =
                near && (poly ? seg_hits_edge(ax, ay, qx, qy, sc.ex0[d], sc.ey0[d], sc.ex1[d],
                                              sc.ey1[d], sc.h2)
                              : seg_hits_disc(ax, ay, qx, qy, dcx[d], dcy[d], dr2[d]));
            if (__any(hit)) return true;
        }
        return false;
    };
    const int ncx = cx1 - cx0 + 1, ncy = cy1 - cy0 + 1;
    if (ncx <= 0 || ncy <= 0) return false;
    if (ncx * ncy <= 64) {
        // every cell of the box at once: lane c reads cell c's item range (one LDS round trip
        // instead of one per cell), then the cells' item lists are dealt out to the lanes as one
        // list (a cell's items follow the previous cell's), 64 at a time — the result is an OR
        // over (item, segment) pairs, so the order does not matter
        const int ncell = ncx * ncy;
        int k0v = 0, cntv = 0;
        if (lane < ncell) {
            const int ry = lane / ncx;
            const int cell = (cy0 + ry) * sc.gnx + cx0 + (lane - ry * ncx);
            k0v = goff[cell];
            cntv = goff[cell + 1] - k0v;
        }
        for (int mb = 0;; mb += 64) {
            const int m = mb + lane;
            int kk = -1, run = 0;
            for (int c = 0; c < ncell; ++c) {
                const int b = __builtin_amdgcn_readlane(k0v, c), n = __builtin_amdgcn_readlane(cntv, c);
                if (m >= run && m < run + n) kk = b + (m - run);
                run += n;
            }
            if (items_reject(kk >= 0, kk)) return true;
            if (mb + 64 >= run) break;
        }
        return false;
    }
    for (int gy = cy0; gy <= cy1; ++gy) {
        for (int gx = cx0; gx <= cx1; ++gx) {
            const int cell = gy * sc.gnx + gx;
            const int k0 = goff[cell], k1 = goff[cell + 1];
            for (int kb = k0; kb < k1; kb += 64)
                if (items_reject(kb + lane < k1, kb + lane)) return true;
        }
    }
    return false;
}

// ------------------------------------------------ straight segments, analytically (round 4)
//
// The S segment of LSL / LSR / RSL / RSR (segment 1) puts its grid points at A + (pd / c) u: A
// its origin, u its world direction, pd the generator's values (interpolate's S branch and the
// world transform, dubins.rs:168-171, 412-422), up to a few ulps of the coordinates (< 1e-12
// relative).  Against the discs of a Q10 scene, with dl = 1e-9 (1 + |A| + |B|) far above that
// rounding:
//   kSClear    every disc centre lies farther than r + dl from the ideal segment AB, and A, B lie
//              dl inside the bounds: every S point and every polyline segment between two S
//              points then lies farther than r from every centre and inside the bounds, so the
//              walk keeps only the first and the last S point (the chord between them clears
//              too) — the verdict is the one of the full polyline;
//   kSHit      some disc's (r - dl) chord on AB, clipped to the stretch the S points surely
//              cover (from 3d past A: the first pd is at most 3d, dubins.rs:239-241; to d
//              before B), is longer than the points' spacing: an S point lies strictly inside
//              the disc, and verify rejects (rrt.rs:124-137) whatever the other segments;
//   kSUnknown  otherwise: the walk tests every point.
// The discs come from the item grid's cells within dl of AB, row by row: lane r takes row
// cy0 + r, clips AB to the row's band (widened by dl; the edge rows extend to infinity, as the
// grid clamps), and the cells of that stretch (widened by dl) are one contiguous item range of
// the row-major CSR.  A disc within r + dl of AB has its cull box (>= r) within dl of AB, so in
// one of those cells.  Called by all 64 lanes; returns a wave-uniform class.
enum : int { kSUnknown = 0, kSClear = 1, kSHit = 2 };
constexpr int kSMinPts = 64;  // S segments shorter than this many points are walked as they are
template <bool kLds>
__device__ int s_classify(const SceneDev& sc, double ax, double ay, double bx, double by,
                          double t_lo, double t_hi, double gap, double dl) {
    const int lane = __lane_id();
    const double ux0 = bx - ax, uy0 = by - ay;
    const double len = sqrt(ux0 * ux0 + uy0 * uy0);
    if (!(len > 0.0)) return kSUnknown;
    const double ux = ux0 / len, uy = uy0 / len;
    int res = (fmin(ax, bx) >= sc.minx + dl && fmax(ax, bx) <= sc.maxx - dl &&
               fmin(ay, by) >= sc.miny + dl && fmax(ay, by) <= sc.maxy - dl)
                  ? kSClear
                  : kSUnknown;
    const int cy0 = __builtin_amdgcn_readfirstlane(grid_cell(fmin(ay, by) - dl, sc.gy0, sc.ginv, sc.gny));
    const int cy1 = __builtin_amdgcn_readfirstlane(grid_cell(fmax(ay, by) + dl, sc.gy0, sc.ginv, sc.gny));
    const int ny = cy1 - cy0 + 1;
    if (ny > 64) return kSUnknown;
    const int* goff = kLds ? reinterpret_cast<const int*>(pp_smem + sc.lds_goff) : sc.goff;
    const int* items = kLds ? reinterpret_cast<const int*>(pp_smem + sc.lds_items) : sc.gitems;
    int k0v = 0, cntv = 0;
    if (lane < ny) {
        const int gy = cy0 + lane;
        const double cell = sc.gcell;
        const double ylo = gy == 0 ? -__builtin_inf() : sc.gy0 + gy * cell - dl;
        const double yhi = gy == sc.gny - 1 ? __builtin_inf() : sc.gy0 + (gy + 1) * cell + dl;
        double t0 = 0.0, t1 = 1.0;
        if (uy0 != 0.0) {
            double ta = (ylo - ay) / uy0, tb = (yhi - ay) / uy0;
            if (ta > tb) {
                const double tt = ta;
                ta = tb;
                tb = tt;
            }
            t0 = fmax(t0, ta);
            t1 = fmin(t1, tb);
        } else if (!(ay >= ylo && ay <= yhi)) {
            t1 = -1.0;
        }
        if (t0 <= t1) {
            const double xa = ax + t0 * ux0, xb = ax + t1 * ux0;
            const int ca = grid_cell(fmin(xa, xb) - dl, sc.gx0, sc.ginv, sc.gnx);
            const int cb = grid_cell(fmax(xa, xb) + dl, sc.gx0, sc.ginv, sc.gnx);
            k0v = goff[gy * sc.gnx + ca];
            cntv = goff[gy * sc.gnx + cb + 1] - k0v;
        }
    }
    // the rows' item ranges dealt to the lanes as one list, 64 at a time (a disc listed in
    // several cells is tested several times).  Each disc is tested in f32 from its cull record
    // (LDS when the image holds it: no f64 loads, no f64 square roots), with margins that make
    // both answers conservative.  e = 2 cull_slack bounds the f32 error of a distance or of a
    // projection t here (cull_slack covers the rounding of the scene's coordinates, both ends
    // of a difference, both axes), and of D.w = fl(r + width / 2):
    //  - near: the f32 distance to AB within D.w + dl + 2e — every disc truly within r + dl;
    //  - hit: the f32 chord of radius ri = D.w - dl - 2e (<= the exact r - dl - e), shortened by
    //    e at each end, lies inside the exact (r - dl) chord, so its overlap with [t_lo, t_hi]
    //    of at least gap + 2e is an exact one of at least gap: an S point lies in the disc.
    // A disc the f32 test cannot decide either way only costs the walk its points (kSUnknown).
    const float4* d4 = (kLds && sc.lds_d4 >= 0)
                           ? reinterpret_cast<const float4*>(pp_smem + sc.lds_d4)
                           : sc.d4;
    const float e = 2.0f * sc.cull_slack;
    const float axf = (float)ax, ayf = (float)ay, uxf = (float)ux, uyf = (float)uy;
    const float lenf = (float)len, dlf = (float)dl;
    const float t_lof = (float)t_lo, t_hif = (float)t_hi, gapf = (float)gap + 2.0f * e;
    for (int mb = 0;; mb += 64) {
        const int m = mb + lane;
        int kk = -1, run = 0;
        for (int r = 0; r < ny; ++r) {
            const int b = __builtin_amdgcn_readlane(k0v, r), n = __builtin_amdgcn_readlane(cntv, r);
            if (m >= run && m < run + n) kk = b + (m - run);
            run += n;
        }
        bool near = false, hit = false;
        if (kk >= 0) {
            const float4 D = d4[items[kk]];
            const float wx = D.x - axf, wy = D.y - ayf;
            const float t = wx * uxf + wy * uyf;
            const float tc = __builtin_fminf(__builtin_fmaxf(t, 0.0f), lenf);
            const float ex = wx - tc * uxf, ey = wy - tc * uyf;
            const float ro = D.w + dlf + 2.0f * e;
            near = ex * ex + ey * ey <= ro * ro;
            const float px = wx - t * uxf, py = wy - t * uyf;
            const float p2 = px * px + py * py, ri = D.w - dlf - 2.0f * e;
            if (ri > 0.0f && p2 < ri * ri) {
                const float h = __builtin_sqrtf(ri * ri - p2) - e;
                hit = __builtin_fminf(t + h, t_hif) - __builtin_fmaxf(t - h, t_lof) >= gapf;
            }
        }
        if (__any(hit)) return kSHit;
        if (__any(near)) res = kSUnknown;
        if (mb + 64 >= run) break;
    }
    return res;
}

// Squared distance of the closed segments a-b and e0-e1: 0 when they cross properly, else the
// nearest endpoint-to-segment distance (the seg_hits_edge predicate as a distance).
__device__ __forceinline__ double seg_seg_d2(double ax, double ay, double bx, double by,
                                             double e0x, double e0y, double e1x, double e1y) {
    const double d1 = (e1x - e0x) * (ay - e0y) - (e1y - e0y) * (ax - e0x);
    const double d2 = (e1x - e0x) * (by - e0y) - (e1y - e0y) * (bx - e0x);
    const double d3 = (bx - ax) * (e0y - ay) - (by - ay) * (e0x - ax);
    const double d4 = (bx - ax) * (e1y - ay) - (by - ay) * (e1x - ax);
    if (((d1 > 0.0 && d2 < 0.0) || (d1 < 0.0 && d2 > 0.0)) &&
        ((d3 > 0.0 && d4 < 0.0) || (d3 < 0.0 && d4 > 0.0)))
        return 0.0;
    return fmin(fmin(seg_point_d2(e0x, e0y, e1x, e1y, ax, ay), seg_point_d2(e0x, e0y, e1x, e1y, bx, by)),
                fmin(seg_point_d2(ax, ay, bx, by, e0x, e0y), seg_point_d2(ax, ay, bx, by, e1x, e1y)));
}

// s_classify for polygon scenes (Q10p, round 5).  The S points lie within dl of AB and the
// polyline through them stays within dl of AB (the dl-neighbourhood of a segment is convex), and
// covers AB's stretch [t_lo, t_hi] continuously (its points advance monotonically along u).  So:
//   kSClear    A, B dl inside the rectangle; every bounds-ring edge farther than h + dl from AB
//              and A inside the ring (then every S point is inside and farther than h from the
//              ring: in_poly_bounds holds); every obstacle edge farther than h + dl from AB (no
//              polyline segment between S points comes within h: seg_hits_edge is false);
//   kSHit      some obstacle edge comes within h - 3 dl of the stretch [t_lo, t_hi]: the polyline
//              segment spanning the nearest point passes within h - 2 dl, so seg_hits_edge holds
//              for it and verify rejects (rrt.rs:124-137) whatever the other segments;
//   kSUnknown  otherwise.  (The bounds ring tests points only, so it never gives a sure hit.)
// The edges come from the item grid exactly as s_classify's discs: an edge within h + dl of AB
// has a point of its cull box (its h-neighbourhood) within dl of AB.  Wave-uniform result.
template <bool kLds>
__device__ int s_classify_poly(const SceneDev& sc, double ax, double ay, double bx, double by,
                               double t_lo, double t_hi, double dl) {
    const int lane = __lane_id();
    const double ux0 = bx - ax, uy0 = by - ay;
    const double len = sqrt(ux0 * ux0 + uy0 * uy0);
    if (!(len > 0.0)) return kSUnknown;
    const double ux = ux0 / len, uy = uy0 / len;
    int res = (fmin(ax, bx) >= sc.minx + dl && fmax(ax, bx) <= sc.maxx - dl &&
               fmin(ay, by) >= sc.miny + dl && fmax(ay, by) <= sc.maxy - dl)
                  ? kSClear
                  : kSUnknown;
    const double h = sqrt(sc.h2);
    const double ro = h + dl, ri = h - 3.0 * dl;
    if (res == kSClear && sc.nbv > 0) {
        // the ring, lane-parallel: clearance from every edge and A's crossing parity
        bool near = false;
        int par = 0;
        for (int i0 = 0; i0 < sc.nbv; i0 += 64) {
            const int i = i0 + lane;
            bool cr = false;
            if (i < sc.nbv) {
                const int j = i + 1 == sc.nbv ? 0 : i + 1;
                const double xi = sc.bvx[i], yi = sc.bvy[i], xj = sc.bvx[j], yj = sc.bvy[j];
                near = near || seg_seg_d2(ax, ay, bx, by, xi, yi, xj, yj) <= ro * ro;
                cr = ray_crosses(ax, ay, xi, yi, xj, yj);
            }
            par ^= __popcll(__ballot(cr)) & 1;
        }
        if (__any(near) || !par) res = kSUnknown;
    }
    if (sc.ne == 0) return res;
    const bool stretch = t_hi > t_lo && ri > 0.0;
    const double sax = ax + t_lo * ux, say = ay + t_lo * uy;
    const double sbx = ax + t_hi * ux, sby = ay + t_hi * uy;
    const int cy0 = __builtin_amdgcn_readfirstlane(grid_cell(fmin(ay, by) - dl, sc.gy0, sc.ginv, sc.gny));
    const int cy1 = __builtin_amdgcn_readfirstlane(grid_cell(fmax(ay, by) + dl, sc.gy0, sc.ginv, sc.gny));
    const int ny = cy1 - cy0 + 1;
    if (ny > 64) return kSUnknown;
    const int* goff = kLds ? reinterpret_cast<const int*>(pp_smem + sc.lds_goff) : sc.goff;
    const int* items = kLds ? reinterpret_cast<const int*>(pp_smem + sc.lds_items) : sc.gitems;
    int k0v = 0, cntv = 0;
    if (lane < ny) {
        const int gy = cy0 + lane;
        const double cell = sc.gcell;
        const double ylo = gy == 0 ? -__builtin_inf() : sc.gy0 + gy * cell - dl;
        const double yhi = gy == sc.gny - 1 ? __builtin_inf() : sc.gy0 + (gy + 1) * cell + dl;
        double t0 = 0.0, t1 = 1.0;
        if (uy0 != 0.0) {
            double ta = (ylo - ay) / uy0, tb = (yhi - ay) / uy0;
            if (ta > tb) {
                const double tt = ta;
                ta = tb;
                tb = tt;
            }
            t0 = fmax(t0, ta);
            t1 = fmin(t1, tb);
        } else if (!(ay >= ylo && ay <= yhi)) {
            t1 = -1.0;
        }
        if (t0 <= t1) {
            const double xa = ax + t0 * ux0, xb = ax + t1 * ux0;
            const int ca = grid_cell(fmin(xa, xb) - dl, sc.gx0, sc.ginv, sc.gnx);
            const int cb = grid_cell(fmax(xa, xb) + dl, sc.gx0, sc.ginv, sc.gnx);
            k0v = goff[gy * sc.gnx + ca];
            cntv = goff[gy * sc.gnx + cb + 1] - k0v;
        }
    }
    for (int mb = 0;; mb += 64) {
        const int m = mb + lane;
        int kk = -1, run = 0;
        for (int r = 0; r < ny; ++r) {
            const int b = __builtin_amdgcn_readlane(k0v, r), n = __builtin_amdgcn_readlane(cntv, r);
            if (m >= run && m < run + n) kk = b + (m - run);
            run += n;
        }
        bool near = false, hit = false;
        if (kk >= 0) {
            const int e = items[kk];
            const double e0x = sc.ex0[e], e0y = sc.ey0[e], e1x = sc.ex1[e], e1y = sc.ey1[e];
            near = seg_seg_d2(ax, ay, bx, by, e0x, e0y, e1x, e1y) <= ro * ro;
            hit = near && stretch && seg_seg_d2(sax, say, sbx, sby, e0x, e0y, e1x, e1y) < ri * ri;
        }
        if (__any(hit)) return kSHit;
        if (__any(near)) res = kSUnknown;
        if (mb + 64 >= run) break;
    }
    return res;
}

// Count-only run of the `pd += d` generator over one segment from its first value w (the same
// passes as walk_rec's generator, every lane a value: the closed form inside a binade, else the
// serial chain through the wave's LDS slots gs): n values with |pd| <= |Ls|, the last of them
// and the first one past (the segment's end, dubins.rs:243-256).  Wave-uniform results.
__device__ inline void seg_count(double w, double dd, double Ls, double* __restrict__ gs,
                                 long long& n, double& last, double& exitv) {
    const int lane = __lane_id();
    const double aL = fabs(Ls);
    n = 0;
    last = w;
    for (;;) {
        int u = 63;
        double v = w;
        const double w1 = w + dd, w2 = w1 + dd;
        bool cf = (w1 - w) == (w2 - w1);
        if (cf) {
            const double vc = __builtin_fma((double)lane, w1 - w, w);
            const uint64_t fm = __ballot(!(fabs(vc) <= aL));
            const int fl = fm ? (int)__builtin_ctzll(fm) : 63;
            cf = __ballot(lane <= fl && (__double2hiint(vc) >> 20) != (__double2hiint(w) >> 20)) == 0;
            v = vc;
        }
        if (!cf) {
            double s = w;
            if (lane == 0) gs[0] = s;
            u = 0;
            bool ended = !(fabs(s) <= aL);
            while (!ended && u < 63) {
                double t4[4];
#pragma unroll
                for (int z = 0; z < 4; ++z) {
                    s += dd;
                    t4[z] = s;
                }
                if (lane == 0) {
#pragma unroll
                    for (int z = 0; z < 4; ++z) gs[u + 1 + z] = t4[z];
                }
                u += 4;
                ended = !(fabs(s) <= aL);
            }
            u = min(u, 63);
            __builtin_amdgcn_wave_barrier();
            v = lane <= u ? gs[lane] : w;
            __builtin_amdgcn_wave_barrier();
        }
        const uint64_t bad = __ballot(lane > u || !(fabs(v) <= aL));
        const int m = bad ? (int)__builtin_ctzll(bad) : 64;
        n += m;
        if (m > 0) last = readlane_f64(v, m - 1);
        if (m <= 63) {
            exitv = readlane_f64(v, m);
            return;
        }
        w = readlane_f64(v, 63) + dd;
    }
}

// Point 0 of a candidate's line — the sample itself — inside an obstacle: the line is rejected
// whatever its parent and its Dubins path (verify, rrt.rs:124-137: the first segment starts inside
// the disc / on an occupied cell), so the candidate needs neither steer_prep nor steer_walk and its
// verdict cannot depend on which node is its parent.  Discs: one bit of the inside bitmap (the
// point's cell lies wholly inside a disc), else the disc grid's cell of the point (every disc is
// listed in each cell its cull box touches); clearly inside only — d2 below r2 by a relative 1e-9,
// far beyond the rounding of the walk's exact segment test, which therefore finds the same hit;
// the grid mode probes the very bit the walk probes.  Polygon scenes: no pre-test.
template <bool kLds, int kScene>
__device__ __forceinline__ bool point_blocked(const SceneDev& sc, double x, double y) {
    if (kScene == kSceneGrid || (kScene == kSceneAny && sc.bits)) {
        const uint32_t* B = kLds ? reinterpret_cast<const uint32_t*>(pp_smem) : sc.bits;
        return grid_occupied(B, sc.bw, sc.bh, sc.bwords, sc.bx0, sc.by0, sc.binv, x, y);
    }
    if (kScene == kScenePoly || (kScene == kSceneAny && (sc.ne > 0 || sc.nbv > 0)) || sc.m == 0)
        return false;
    if (sc.ibits) {  // one load: the cell lies wholly inside a disc (scene::inside_bitmap)
        const double fx = floor((x - sc.ibx0) * sc.ibinv), fy = floor((y - sc.iby0) * sc.ibinv);
        if (!(fx >= 0.0) || !(fy >= 0.0) || fx >= (double)sc.ibn || fy >= (double)sc.ibn)
            return false;
        const int i = (int)fx, j = (int)fy;
        return (sc.ibits[(size_t)j * sc.ibwords + (i >> 5)] >> (i & 31)) & 1u;
    }
    const int* goff = kLds ? reinterpret_cast<const int*>(pp_smem + sc.lds_goff) : sc.goff;
    const int* items = kLds ? reinterpret_cast<const int*>(pp_smem + sc.lds_items) : sc.gitems;
    const int cell = grid_cell(y, sc.gy0, sc.ginv, sc.gny) * sc.gnx + grid_cell(x, sc.gx0, sc.ginv, sc.gnx);
    const int k1 = goff[cell + 1];
    for (int k = goff[cell]; k < k1; ++k) {
        const int d = items[k];
        const double dx = x - sc.cx[d], dy = y - sc.cy[d];
        if (dx * dx + dy * dy < sc.r2[d] * (1.0 - 1.0e-9)) return true;
    }
    return false;
}

// Fast path of verify_node for the edge child (x, y, yaw) → parent (px, py, pyaw): the Dubins
// polyline of line_to_origin (rrt.rs:295-315) plus the junction to the parent, whose own line
// was verified when it was inserted.  Split in two:
//   steer_prep  per lane (one task per lane): word choice, lengths, segment origins, the trim
//               checks — all the per-task scalar math;
//   steer_walk  per wave (one task per wave): the `pd += d` walk of generate_local_course
//               (dubins.rs:239-255) replayed uniformly, each lane capturing one grid point so
//               every point carries exactly the reference's accumulated value; interpolation
//               and the collision test then run lane-parallel, 63 points per chunk.
// An edge too long to walk (more than 1e8 steps: the reference would allocate that many points)
// is an error, unless its verdict is known without the walk: the line starts at the child
// (point 0 of the Dubins polyline, and the None line's first point), and Space::verify rejects a
// line with a point outside the bounds' box in every scene mode (chunk_rejects' first test).  A
// caller's sample or candidate far outside the scene is such a child: rejected, its nearest node
// and yaw still reported.
__device__ __forceinline__ bool child_out_of_bounds(const SceneDev& sc, double x, double y) {
    return !(x >= sc.minx && x <= sc.maxx && y >= sc.miny && y <= sc.maxy);
}

struct SteerPrep {
    double x, y, px, py;      // child (point 0 of the edge) and parent (the junction)
    double c, cw, sw;         // curvature, cos/sin(-yaw) of the world transform
    double L0, L1, L2;        // segment lengths
    double o1x, o1y, o1yaw;   // origin of segment 1 (endpoint of segment 0)
    double o2x, o2y, o2yaw;   // origin of segment 2
    long long n_point;        // dubins.rs:369
    int m0, m1, m2;           // segment modes
    int state;                // -1: walk; kReject/kAccept: decided; kLiteral; kError; 4: None
};
static_assert(sizeof(SteerPrep) == kSteerPrepBytes, "SteerPrep layout");

__device__ __forceinline__ SteerPrep steer_prep(const SceneDev& sc, double x, double y,
                                                double yaw, double px, double py, double pyaw) {
    SteerPrep r;
    r.x = x;
    r.y = y;
    r.px = px;
    r.py = py;
    const double step = sc.step_size;
    // dubins_path_planning, dubins.rs:401-408 (s = child, e = parent)
    const double ex = px - x, ey = py - y;
    const double c = 1.0 / sc.turn_radius;
    const double lex = cos(yaw) * ex + sin(yaw) * ey;
    const double ley = -(sin(yaw)) * ex + cos(yaw) * ey;
    const double leyaw = pyaw - yaw;
    const Steer s = select_word(lex, ley, leyaw, c);
    r.c = c;
    r.cw = cos(-yaw);
    r.sw = sin(-yaw);
    if (s.word < 0) {  // steer failed: line_to_origin contributes [(sx, sy)] (rrt.rs:313)
        r.state = kPrepNone;
        return r;
    }
    r.L0 = s.t;
    r.L1 = s.p;
    r.L2 = s.q;
    r.m0 = word_mode(s.word, 0);
    r.m1 = word_mode(s.word, 1);
    r.m2 = word_mode(s.word, 2);
    double total = 0.0;
    total += s.t;
    total += s.p;
    total += s.q;
    const double nq = trunc(total / step);
    if (!(nq >= 0.0) || nq > 1.0e8) {
        r.state = child_out_of_bounds(sc, x, y) ? kReject : kError;
        return r;
    }
    r.n_point = (long long)nq + 3 + 4;
    // segment origins = previous segment's endpoint (dubins.rs:230, 258-271)
    const Pose O0{0.0, 0.0, 0.0};
    const Pose O1 = interp_local(r.m0, r.L0, c, O0);
    const Pose O2 = interp_local(r.m1, r.L1, c, O1);
    const Pose E = interp_local(r.m2, r.L2, c, O2);
    r.o1x = O1.x;
    r.o1y = O1.y;
    r.o1yaw = O1.yaw;
    r.o2x = O2.x;
    r.o2y = O2.y;
    r.o2yaw = O2.yaw;
    // The trim (dubins.rs:281-288) drops exactly the final endpoint unless its local x is 0.0
    // (then it keeps popping) or the array has no trailing zero: both go to the literal path.
    r.state = E.x == 0.0 ? kLiteral : kPrepWalk;
    return r;
}

// The record's fields travel as scalars (a struct passed by reference ends up on the private
// stack once the per-lane segment select turns into an indexed load).
struct WalkIn {
    double x, y, px, py, c, cw, sw, L0, L1, L2, o1x, o1y, o1yaw, o2x, o2y, o2yaw;
    long long n_point;
    int m0, m1, m2, state;
};
__device__ __forceinline__ WalkIn walk_in(const SteerPrep* __restrict__ p) {
    WalkIn w;
    w.x = p->x;
    w.y = p->y;
    w.px = p->px;
    w.py = p->py;
    w.c = p->c;
    w.cw = p->cw;
    w.sw = p->sw;
    w.L0 = p->L0;
    w.L1 = p->L1;
    w.L2 = p->L2;
    w.o1x = p->o1x;
    w.o1y = p->o1y;
    w.o1yaw = p->o1yaw;
    w.o2x = p->o2x;
    w.o2y = p->o2y;
    w.o2yaw = p->o2yaw;
    w.n_point = p->n_point;
    w.m0 = p->m0;
    w.m1 = p->m1;
    w.m2 = p->m2;
    w.state = p->state;
    return w;
}
__device__ __forceinline__ WalkIn walk_in(const SteerPrep& p) { return walk_in(&p); }

// walked / walked_arc (optional, wave-uniform): += the polyline points generated and verified /
// those of them on L and R segments (the sincos points of the walk's FLOP count)
template <bool kLds>
__device__ __forceinline__ int steer_walk(const SceneDev& sc, const WalkIn r,
                                          bool junction = true, int* walked = nullptr,
                                          int* walked_arc = nullptr) {
    const int lane = __lane_id();
    if (r.state == kPrepNone) {  // polyline [(x, y), (px, py)]
        if (walked) *walked += 2;
        const bool has = lane < 2;
        const double qx = lane == 0 ? r.x : r.px, qy = lane == 0 ? r.y : r.py;
        return chunk_rejects<kLds>(sc, has, has, lane == 1, qx, qy) ? kReject : kAccept;
    }
    if (r.state != kPrepWalk) return r.state;
    const double step = sc.step_size;
    const double L0 = r.L0, L1 = r.L1, L2 = r.L2;
    const int m0 = r.m0, m1 = r.m1, m2 = r.m2;
    const double o1x = r.o1x, o1y = r.o1y, o1yaw = r.o1yaw;
    const double o2x = r.o2x, o2y = r.o2y, o2yaw = r.o2yaw;
    int seg = 0;
    double dd = (L0 > 0.0) ? step : -step;
    double pd = dd - 0.0;
    long long grid = 0;
    double carry_x = r.x, carry_y = r.y;  // point 0 of the edge is the child itself
    bool first = true;
    for (;;) {
        int my_seg = 0;
        double my_pd = 0.0;
        int cnt = 0;
        while (cnt < 63 && seg < 3) {
            const double Ls = seg == 0 ? L0 : (seg == 1 ? L1 : L2);
            if (fabs(pd) <= fabs(Ls)) {
                if (lane == cnt + 1) {
                    my_seg = seg;
                    my_pd = pd;
                }
                ++cnt;
                pd += dd;
            } else {
                const double ll = Ls - pd - dd;
                ++seg;
                if (seg < 3) {
                    const double Ln = seg == 1 ? L1 : L2;
                    dd = (Ln > 0.0) ? step : -step;
                    pd = ((Ls * Ln) > 0.0) ? (-dd - ll) : (dd - ll);
                }
            }
        }
        grid += cnt;
        const bool end_here = (seg >= 3) && cnt < 63;
        const bool junction_here = end_here && junction;
        double qx = carry_x, qy = carry_y;
        bool has = (lane == 0), isgrid = false, isjunction = false, isarc = false;
        if (lane >= 1 && lane <= cnt) {
            Pose o;
            o.x = my_seg == 0 ? 0.0 : (my_seg == 1 ? o1x : o2x);
            o.y = my_seg == 0 ? 0.0 : (my_seg == 1 ? o1y : o2y);
            o.yaw = my_seg == 0 ? 0.0 : (my_seg == 1 ? o1yaw : o2yaw);
            const int mm = my_seg == 0 ? m0 : (my_seg == 1 ? m1 : m2);
            isarc = mm != kModeS;
            const Pose p = interp_local(mm, my_pd, r.c, o);
            qx = r.cw * p.x + r.sw * p.y + r.x;   // dubins.rs:415
            qy = -r.sw * p.x + r.cw * p.y + r.y;  // dubins.rs:420
            has = true;
            isgrid = true;
        } else if (junction_here && lane == cnt + 1) {
            qx = r.px;
            qy = r.py;
            has = true;
            isjunction = true;  // the parent: already checked unless it is the root
        }
        const bool check_bounds = isgrid || isjunction || (first && lane == 0);
        const bool rej = chunk_rejects<kLds>(sc, has, check_bounds, has && lane >= 1, qx, qy);
        if (walked) *walked += cnt + (first ? 1 : 0) + (junction_here ? 1 : 0);
        if (walked_arc) *walked_arc += __popcll(__ballot(isarc));
        if (rej) return kReject;
        if (end_here) break;
        carry_x = readlane_f64(qx, cnt);
        carry_y = readlane_f64(qy, cnt);
        first = false;
    }
    if (1 + grid > r.n_point - 2) return kLiteral;
    return kAccept;
}

// Both halves on one wave (uniform prep): the repair and verify_node paths.
// junction = false: the polyline ends at the edge's last point (finalize's edge into the root,
// rrt.rs:532, contributes no root point).
template <bool kLds>
__device__ int steer_collide_fast(const SceneDev& sc, double x, double y, double yaw, double px,
                                  double py, double pyaw, bool junction = true) {
    const SteerPrep r = steer_prep(sc, x, y, yaw, px, py, pyaw);
    return steer_walk<kLds>(sc, walk_in(r), junction);
}

// The walk's chunk test over a stored polyline (bx, by)[0, np): chunks of 63 segments, lane 0 the
// previous chunk's last point (bounds-checked in the first chunk only), lanes 1..63 the next
// points; lanes past the end hold (x, y), untested.  Called by all 64 lanes; true when a chunk
// rejects the line.
__device__ __forceinline__ bool stored_line_rejects(const SceneDev& sc, const double* bx,
                                                    const double* by, int np, double x, double y) {
    const int lane = __lane_id();
    for (int base = 0; base == 0 || base + 1 < np; base += 63) {
        const int i = base + lane;
        const bool has = i < np;
        const double qx = has ? bx[i] : x, qy = has ? by[i] : y;
        if (chunk_rejects<false>(sc, has, has && (lane >= 1 || base == 0), has && lane >= 1, qx, qy))
            return true;
    }
    return false;
}

// Literal path (the trim cases the fast walk cannot reproduce: an endpoint local x of 0.0, a
// buffer with no trailing zero): lane 0 runs dubins_literal into its scratch buffer, then the
// whole wave verifies the polyline with the walk's chunk test — chunks of 63 segments, lane 0 the
// previous chunk's last point (bounds-checked in the first chunk only), lanes 1..63 the next
// points — instead of one lane looping over every point and obstacle.  Rare in the extend, but
// check_finish meets it on optimize's self-connections (a node's copy into the node itself): the
// serial test held a scratch slot of the shared pool for a whole scene scan, and hundreds of waves
// queued for the slots.
template <bool kFI>
__device__ __forceinline__ int steer_collide_literal_body(const SceneDev& sc, double x, double y,
                                                          double yaw, double px, double py,
                                                          double pyaw, double* bx, double* by,
                                                          double* byaw, bool junction) {
    const int lane = __lane_id();
    int n = 0, r = 0;
    if (lane == 0) {
        int word = -1;
        double cost = 0.0;
        r = dubins_literal<kFI>(x, y, yaw, px, py, pyaw, sc.turn_radius, sc.step_size, bx, by, byaw,
                           kLiteralCap - 1, &n, &word, &cost);
        if (r != kSteerOverflow) {
            if (r == kSteerNone) {
                bx[0] = x;
                by[0] = y;
                n = 1;
            }
            bx[n] = px;
            by[n] = py;
        }
    }
    r = __shfl(r, 0);
    n = __shfl(n, 0);
    if (r == kSteerOverflow) return kError;
    __threadfence_block();  // lane 0's points before the wave reads them
    const int np = junction ? n + 1 : n;  // the junction point is bounds-checked too
    return stored_line_rejects(sc, bx, by, np, x, y) ? kReject : kAccept;
}
__device__ inline int steer_collide_literal(const SceneDev& sc, double x, double y, double yaw,
                                            double px, double py, double pyaw, double* bx,
                                            double* by, double* byaw, bool junction = true) {
    return steer_collide_literal_body<false>(sc, x, y, yaw, px, py, pyaw, bx, by, byaw, junction);
}

__device__ inline void argmin_pair(double& d, int& i, double od, int oi) {
    if (od < d || (od == d && oi < i)) {
        d = od;
        i = oi;
    }
}

// sincos_small's constants (pp_device.h): __ocml_sincos_f64's, bit for bit (static: one copy in
// the code object of every unit that includes this header — the header's one variable)
static __constant__ double kSinCosTab[17] = {
    0x1.45f306dc9c883p-1,  -0x1.921fb54442d18p+0,  -0x1.1a62633145c00p-54,
    0x1.1a62633145c00p-54, -0x1.b839a252049c0p-104,
    -0x1.907db46cc5e42p-37, 0x1.1eeb69037ab78p-29, -0x1.27e4fa17f65f6p-22,
    0x1.a01a019f4ec90p-16,  -0x1.6c16c16c16967p-10, 0x1.5555555555555p-5,
    0x1.5e0b2f9a43bb8p-33,  -0x1.ae600b42fdfa7p-26, 0x1.71de3796cde01p-19,
    -0x1.a01a019e83e5cp-13, 0x1.1111111110bb3p-7,   -0x1.5555555555555p-3};

// One segment's endpoint from its origin (interpolate at the full length, dubins.rs:155-198)
// with the transcendental values supplied: ca/sa as in PrepRec, sl/cl = sin/cos(length).
struct Pt {
    double x, y;
};
// (x / c as div_by: the correctly rounded FMA quotient, bit-identical to the division)
__device__ inline Pt seg_end(int mode, double len, double c, double rc, double ox, double oy,
                             double ca, double sa, double sl, double cl) {
    Pt r;
    if (mode == kModeS) {
        const double lc = div_by(len, c, rc);
        r.x = ox + lc * ca;
        r.y = oy + lc * sa;
    } else {
        const double ldx = div_by(sl, c, rc);
        const double l1 = div_by(1.0 - cl, c, rc);  // (1 - cos) / -c = -((1 - cos) / c)
        const double ldy = mode == kModeL ? l1 : -l1;
        const double gdx = ca * ldx + sa * ldy;
        const double gdy = -sa * ldx + ca * ldy;
        r.x = ox + gdx;
        r.y = oy + gdy;
    }
    return r;
}

// The per-task body of steer_prep: the 8 lanes r of one task group (all 64 lanes of the wave
// call it: the word choice broadcasts within 8-lane groups).  act: an active task (else a
// kReject record); write: this group owns task t (lane r == 0 stores rec[t], *yaw_dst and
// cost_out[t]).
__device__ __forceinline__ void prep_task(const SceneDev& sc, int r, int g0, int t, bool write,
                                          bool act, double x, double y, double px, double py,
                                          double pyaw, int own, double cyaw, int cull, double cbase,
                                          double climit, PrepRec* __restrict__ rec,
                                          double* yaw_dst, double* __restrict__ cost_out,
                                          int force_state = -1) {
    const double step = sc.step_size;
    const double c = 1.0 / sc.turn_radius;
    const double cy_atan = atan2(py - y, px - x);
    const double yaw = own ? cyaw : cy_atan;
    // dubins_path_planning, dubins.rs:401-408 (s = child, e = parent)
    const double ex = px - x, ey = py - y;
    const double cyw = cos(yaw), syw = sin(yaw);
    const double lex = cyw * ex + syw * ey;
    const double ley = -(syw)*ex + cyw * ey;
    const double leyaw = pyaw - yaw;
    // dubins_path_planning_from_origin, dubins.rs:333-348
    const double hyp = hypot(lex, ley);
    const double d = hyp * c;
    const double theta = mod2pi(atan2(ley, lex));
    const double alpha = mod2pi(-theta);
    const double beta = mod2pi(leyaw - theta);
    // lanes 0/1: sin(alpha), sin(beta); lanes 0/1/2: cos(alpha), cos(beta), cos(alpha - beta)
    const double s_in = sin(r == 0 ? alpha : beta);
    const double c_in = cos(r == 0 ? alpha : (r == 1 ? beta : alpha - beta));
    const double sa = grp8_bcast_f64<0>(s_in), sb = grp8_bcast_f64<1>(s_in);
    const double ca = grp8_bcast_f64<0>(c_in), cb = grp8_bcast_f64<1>(c_in),
                 c_ab = grp8_bcast_f64<2>(c_in);
    // lane r < 6 evaluates word r of ALL_PLANNERS (dubins.rs:27-153, 291)
    const double dd2 = d * d;
    double ya = 0.0, xa = 1.0, psq = -1.0, tmpc = 2.0;
    if (r == 0) {
        psq = 2.0 + dd2 - (2.0 * c_ab) + (2.0 * d * (sa - sb));
        ya = cb - ca;
        xa = d + sa - sb;
    } else if (r == 1) {
        psq = 2.0 + dd2 - (2.0 * c_ab) + (2.0 * d * (sb - sa));
        ya = ca - cb;
        xa = d - sa + sb;
    } else if (r == 2) {
        psq = -2.0 + dd2 + (2.0 * c_ab) + (2.0 * d * (sa + sb));
        ya = -ca - cb;
        xa = d + sa + sb;
    } else if (r == 3) {
        psq = -2.0 + dd2 + (2.0 * c_ab) - (2.0 * d * (sa + sb));
        ya = ca + cb;
        xa = d - sa - sb;
    } else if (r == 4) {
        tmpc = (6.0 - dd2 + 2.0 * c_ab + 2.0 * d * (sa - sb)) / 8.0;
        ya = ca - cb;
        xa = d - sa + sb;
    } else if (r == 5) {
        tmpc = (6.0 - dd2 + 2.0 * c_ab + 2.0 * d * (-sa + sb)) / 8.0;
        ya = ca - cb;
        xa = d + sa - sb;
    }
    const bool wok = r < 4 ? !(psq < 0.0) : (r < 6 ? !(fabs(tmpc) > 1.0) : false);
    const double A1 = atan2(ya, xa);
    const double pp = sqrt(r < 4 && wok ? psq : 0.0);
    const double A2 = atan2(r == 2 ? -2.0 : 2.0, pp);
    const double Cc = acos(r >= 4 && wok ? tmpc : 0.0);
    double wt = 0.0, wp = 0.0, wq = 0.0;
    if (r == 0) {
        wt = mod2pi(-alpha + A1);
        wp = pp;
        wq = mod2pi(beta - A1);
    } else if (r == 1) {
        wt = mod2pi(alpha - A1);
        wp = pp;
        wq = mod2pi(-beta + A1);
    } else if (r == 2) {
        const double tm = A1 - A2;
        wt = mod2pi(-alpha + tm);
        wp = pp;
        wq = mod2pi(-mod2pi(beta) + tm);
    } else if (r == 3) {
        const double tm = A1 - A2;
        wt = mod2pi(alpha - tm);
        wp = pp;
        wq = mod2pi(beta - tm);
    } else if (r == 4) {
        wp = mod2pi(2.0 * kPi - Cc);
        wt = mod2pi(alpha - A1 + mod2pi(wp / 2.0));
        wq = mod2pi(alpha - beta - wt + mod2pi(wp));
    } else if (r == 5) {
        wp = mod2pi(2.0 * kPi - Cc);
        wt = mod2pi(-alpha - A1 + wp / 2.0);
        wq = mod2pi(mod2pi(beta) - alpha - wt + mod2pi(wp));
    }
    const double wcost = fabs(wt) + fabs(wp) + fabs(wq);
    // first strict minimum in ALL_PLANNERS order (dubins.rs:351-360: bcost starts at inf and a
    // word wins on `bcost > cost`, so a NaN or inf cost never wins and ties keep the earlier
    // word) = the (cost, word) argmin over the group's valid words: a DPP butterfly over the
    // 8-lane group (xor 1, xor 2, half-row mirror), no per-word broadcasts
    double bc = (r < 6 && wok && wcost < __builtin_inf()) ? wcost : __builtin_inf();
    int bw = bc < __builtin_inf() ? r : 0x7fffffff;
    argmin_dpp<0xB1>(bc, bw);
    argmin_dpp<0x4E>(bc, bw);
    argmin_dpp<0x141>(bc, bw);
    if (!(bc < __builtin_inf())) bw = -1;
    const int src = g0 + (bw < 0 ? 0 : bw);
    const double L0 = __shfl(wt, src), L1 = __shfl(wp, src), L2 = __shfl(wq, src);
    const int m0 = word_mode(bw, 0), m1 = word_mode(bw, 1), m2 = word_mode(bw, 2);
    int state = !act ? kReject : (bw < 0 ? kPrepNone : kPrepWalk);
    double tot = 0.0;
    tot += L0;
    tot += L1;
    tot += L2;
    const double nq = trunc(tot / step);
    if (state == kPrepWalk && (!(nq >= 0.0) || nq > 1.0e8))
        state = child_out_of_bounds(sc, x, y) ? kReject : kError;
    // segment origin headings (interpolate's yaw, dubins.rs:191-196)
    const double oy0 = 0.0;
    const double oy1 = m0 == kModeL ? oy0 + L0 : (m0 == kModeR ? oy0 - L0 : oy0);
    const double oy2 = m1 == kModeL ? oy1 + L1 : (m1 == kModeR ? oy1 - L1 : oy1);
    // lanes 0..2: segment trig, 3..5: sin/cos of the lengths, 6: the world transform
    double arg = 0.0;
    if (r < 3) {
        const int ms = r == 0 ? m0 : (r == 1 ? m1 : m2);
        const double oys = r == 0 ? oy0 : (r == 1 ? oy1 : oy2);
        arg = ms == kModeS ? oys : -oys;
    } else if (r < 6) {
        arg = r == 3 ? L0 : (r == 4 ? L1 : L2);
    } else if (r == 6) {
        arg = -yaw;
    }
    const double sv = sin(arg), cv = cos(arg);
    const double ca0 = grp8_bcast_f64<0>(cv), ca1 = grp8_bcast_f64<1>(cv), ca2 = grp8_bcast_f64<2>(cv);
    const double sa0 = grp8_bcast_f64<0>(sv), sa1 = grp8_bcast_f64<1>(sv), sa2 = grp8_bcast_f64<2>(sv);
    const double sl0 = grp8_bcast_f64<3>(sv), sl1 = grp8_bcast_f64<4>(sv), sl2 = grp8_bcast_f64<5>(sv);
    const double cl0 = grp8_bcast_f64<3>(cv), cl1 = grp8_bcast_f64<4>(cv), cl2 = grp8_bcast_f64<5>(cv);
    const double cw = grp8_bcast_f64<6>(cv), sw = grp8_bcast_f64<6>(sv);
    const double rc = 1.0 / c;
    const Pt O1 = seg_end(m0, L0, c, rc, 0.0, 0.0, ca0, sa0, sl0, cl0);
    const Pt O2 = seg_end(m1, L1, c, rc, O1.x, O1.y, ca1, sa1, sl1, cl1);
    const Pt E = seg_end(m2, L2, c, rc, O2.x, O2.y, ca2, sa2, sl2, cl2);
    // the trim (dubins.rs:281-288) drops exactly the endpoint unless its local x is 0.0; then it
    // drops the last grid point too, and goes on while the dropped x is 0.0: the walk drops that
    // point and hands the rest (its x 0.0 as well) to the literal path
    const int trim1 = (state == kPrepWalk && E.x == 0.0) ? 1 : 0;
    int cnt0 = 0, cnt1 = 0, cnt2 = 0, fb_seg = 0;
    double fb_pd = 0.0, fb_dd = 0.0;
    // no grid points are stored: steer_walk generates them all, lane-parallel and bit-exact,
    // from the walk's initial state (segment 0, pd = d - 0.0, dubins.rs:239-241), and runs
    // the trailing-zero check itself
    if (state == kPrepWalk) {
        state = kPrepFallback;
        fb_dd = (L0 > 0.0) ? step : -step;
        fb_pd = fb_dd - 0.0;
    }
    // RRT* cull: an edge whose cost cannot beat the limit is settled without its walk
    if (act && cull && !(cbase + bc < climit)) state = kReject;
    // the query batch's verdict cache (mq_sample_nn): the same child and parent as a task the
    // previous step walked — its verdict, no walk
    if (act && force_state >= 0) state = force_state;
    if (write && r == 0) {  // idle batch tasks get a kReject record (act == false)
        PrepRec o;
        o.x = x;
        o.y = y;
        o.px = px;
        o.py = py;
        o.yaw = yaw;
        o.pyaw = pyaw;
        o.c = c;
        o.cw = cw;
        o.sw = sw;
        o.ox[0] = 0.0;
        o.oy[0] = 0.0;
        o.ox[1] = O1.x;
        o.oy[1] = O1.y;
        o.ox[2] = O2.x;
        o.oy[2] = O2.y;
        o.ca[0] = ca0;
        o.ca[1] = ca1;
        o.ca[2] = ca2;
        o.sa[0] = sa0;
        o.sa[1] = sa1;
        o.sa[2] = sa2;
        o.L[0] = L0;
        o.L[1] = L1;
        o.L[2] = L2;
        o.n_point = (long long)nq + 3 + 4;
        o.fb_pd = fb_pd;
        o.fb_dd = fb_dd;
        o.fb_seg = fb_seg;
        o.m[0] = m0;
        o.m[1] = m1;
        o.m[2] = m2;
        o.cnt[0] = cnt0;
        o.cnt[1] = cnt1;
        o.cnt[2] = cnt2;
        o.state = state;
        o.trim1 = trim1;
        rec[t] = o;
        if (yaw_dst) *yaw_dst = yaw;
        // the Dubins cost (dubins.rs:351-361; inf on None): the RRT* edge cost
        if (cost_out) cost_out[t] = bc;
    }
}

// steer_walk for one PrepRec (called by all 64 lanes; the record is wave-uniform).  Chunks of 63
// grid points: lane k >= 1 interpolates grid point base + k - 1 (interpolate, dubins.rs:155-198,
// then the world transform dubins.rs:412-422), lane 0 carries the previous chunk's last point,
// and the junction to the parent follows the last grid point.  The grid points' pd values come
// from the lane-parallel `pd += d` generator below, started from the state steer_prep kept
// (segment 0, pd = d), each lane capturing its own point.  npts (wave-uniform) += the polyline points generated and verified
// (grid points plus the junction; the profiled walk roofline's unit).
//
// gs: the wave's kGenSlots LDS doubles — the generator's kGenPts value slots, then the task's
// segment table (kSegRow doubles per segment: origin x, y, trig ca, sa, mode), written once per task
// by lanes 0-2, from which each point's lane reads its own segment's row (two ds_read_b128)
// instead of selecting among the twelve wave-uniform values.
//
// The three divisions by the curvature c per point (dubins.rs:169-178: length / c, sin / c,
// (1 - cos) / +-c) are x / c = q + (x - q c) / c rounded once: q = RN(x rc), the residual
// fma(-q, c, x) is exact, and RN(q + residual rc) with rc = RN(1 / c) is the correctly rounded
// quotient (Markstein's theorem; no x here is subnormal), i.e. bit-identical to the division —
// tests/test_div_identity.py checks the identity for the scenes' curvatures.  3 VALU instead of 9.
// A wave-uniform value into SGPRs: walk_rec's record fields.  A record in LDS is read with
// ds_read into VGPRs (~60 of them for the ~30 fields the walk keeps live); readfirstlane moves
// each into SGPRs, as the scalar loads of a global record do (there it folds away).
__device__ __forceinline__ double ufl(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ int ufl(int v) { return __builtin_amdgcn_readfirstlane(v); }
constexpr int kGenPts = 68;  // generator slots: 63 points + 4 overshoot + 1
constexpr int kSegRow = 6;   // segment-table row (16-byte aligned rows: ds_read_b128)
template <bool kLds, int kScene = kSceneAny, bool kS = false>
__device__ __forceinline__ int walk_rec(const SceneDev& sc, const PrepRec* __restrict__ p,
                                        double* __restrict__ gs, int& npts, int& napts,
                                        bool junction = true) {
    const int lane = __lane_id();
    const int state = ufl(p->state);
    const double x = ufl(p->x), y = ufl(p->y), px = ufl(p->px), py = ufl(p->py);
    if (state == kPrepNone) {  // steer failed: polyline [(x, y), (px, py)] (rrt.rs:313)
        const bool has = lane < 2;
        const double qx = lane == 0 ? x : px, qy = lane == 0 ? y : py;
        npts += 2;
        return chunk_rejects<kLds, kScene>(sc, has, has, lane == 1, qx, qy) ? kReject : kAccept;
    }
    // (steer_prep stores no grid points: every walkable record is kPrepFallback at point 0)
    if (state != kPrepFallback) return state == kPrepWalk ? kError : state;
    const double step = sc.step_size;
    const double c = ufl(p->c), cw = ufl(p->cw), sw = ufl(p->sw);
    const double ox1 = ufl(p->ox[1]), oy1 = ufl(p->oy[1]), ox2 = ufl(p->ox[2]), oy2 = ufl(p->oy[2]);
    const double ca0 = ufl(p->ca[0]), ca1 = ufl(p->ca[1]), ca2 = ufl(p->ca[2]);
    const double sa0 = ufl(p->sa[0]), sa1 = ufl(p->sa[1]), sa2 = ufl(p->sa[2]);
    const double L0 = ufl(p->L[0]), L1 = ufl(p->L[1]), L2 = ufl(p->L[2]);
    const int m0 = ufl(p->m[0]), m1 = ufl(p->m[1]), m2 = ufl(p->m[2]);
    const double rc = 1.0 / c;
    double* segt = gs + kGenPts;
    if (lane < 3) {
        double* row = segt + kSegRow * lane;
        row[0] = lane == 0 ? 0.0 : (lane == 1 ? ox1 : ox2);
        row[1] = lane == 0 ? 0.0 : (lane == 1 ? oy1 : oy2);
        row[2] = lane == 0 ? ca0 : (lane == 1 ? ca1 : ca2);
        row[3] = lane == 0 ? sa0 : (lane == 1 ? sa1 : sa2);
        row[4] = (double)(lane == 0 ? m0 : (lane == 1 ? m1 : m2));
    }
    __builtin_amdgcn_wave_barrier();
    // the generator's initial state (segment 0, pd = d - 0.0, dubins.rs:239-241), from steer_prep
    int gseg = ufl(p->fb_seg);
    double gdd = ufl(p->fb_dd);
    double gpd = ufl(p->fb_pd);
    long long grid = 0;  // grid points generated (and counted) so far
    double carry_x = x, carry_y = y;
    npts += 1;  // point 0, the child
    // a long S segment against the discs (s_classify) or the polygon edges and bounds ring
    // (s_classify_poly), analytically: a sure hit rejects at once,
    // a sure clearance keeps only its first and last point (s_state 1: counted, s_emit of them
    // placed in lanes so far)
    bool s_clear = false;
    int s_state = 0, s_emit = 0;
    long long s_n = 0;
    double s_first = 0.0, s_last = 0.0, s_exit = 0.0;
    const int trim1 = ufl(p->trim1);
    const bool discs = kS && !trim1 &&
                       (kScene == kSceneDisc ||
                        (kScene == kSceneAny && !sc.bits && sc.ne == 0 && sc.nbv == 0)) &&
                       sc.m > 0;
    const bool polys = kS && !trim1 &&
                       (kScene == kScenePoly ||
                        (kScene == kSceneAny && !sc.bits && (sc.ne > 0 || sc.nbv > 0)));
    if ((discs || polys) && m1 == kModeS && L1 >= kSMinPts * step) {
        const double ax = cw * ox1 + sw * oy1 + x, ay = -sw * ox1 + cw * oy1 + y;
        const double pcb = div_by(L1, c, rc);
        const double lxb = ox1 + pcb * ca1, lyb = oy1 + pcb * sa1;
        const double bx = cw * lxb + sw * lyb + x, by = -sw * lxb + cw * lyb + y;
        const double dl = 1.0e-9 * (1.0 + fabs(ax) + fabs(ay) + fabs(bx) + fabs(by));
        const double sp = step * rc;  // the S points' spacing along AB
        const double t_lo = 3.0 * sp * (1.0 + 1.0e-9) + dl;
        const double t_hi = (L1 - step) * rc * (1.0 - 1.0e-9) - dl;
        const int cls = polys ? s_classify_poly<kLds>(sc, ax, ay, bx, by, t_lo, t_hi, dl)
                              : s_classify<kLds>(sc, ax, ay, bx, by, t_lo, t_hi,
                                                 sp * (1.0 + 1.0e-9) + 2.0 * dl, dl);
        if (cls == kSHit) return kReject;
        s_clear = cls == kSClear;
    }
    for (int base = 0;; base += 63) {
        int cnt = 0, my_seg = 0;
        double my_pd = 0.0;
        bool done;
        bool chord = false;  // lane 1 holds the cleared S segment's last point, lane 0 its first
        {
            // lane-parallel `pd += d` (dubins.rs:239-255): lane l >= pos replays l - pos
            // additions from the uniform start value — the serial walk's exact rounding
            // sequence — and the first lane whose |pd| exceeds |L| ends the segment (its value
            // gives ll and the next segment's start, dubins.rs:256-259)
            int pos = 1;
            while (pos <= 63 && gseg < 3) {
                if (s_clear && gseg == 1) {
                    // the cleared S segment: its first and last points only (s_classify), the
                    // rest counted; then the segment's end as the generator would reach it
                    if (s_state == 0) {
                        seg_count(gpd, gdd, L1, gs, s_n, s_last, s_exit);
                        s_first = gpd;
                        s_state = 1;
                    }
                    // The chord between the two lies within rounding of AB, so it clears and is
                    // not tested: the chunk ends after the first point, and the next one starts
                    // with the chord (lanes 0 -> 1), its box without lane 0 — so the long chord
                    // neither widens a chunk's item search nor meets the exact tests
                    const int n_emit = s_n >= 2 ? 2 : (int)s_n;
                    while (s_emit < n_emit && pos <= 63) {
                        if (s_emit == 1 && pos > 1) break;
                        if (lane == pos) {
                            my_seg = 1;
                            my_pd = s_emit == 0 ? s_first : s_last;
                        }
                        if (s_emit == 1) chord = true;
                        ++s_emit;
                        ++pos;
                        ++cnt;
                    }
                    if (s_emit < n_emit) break;  // the chunk ends: the next one goes on
                    grid += s_n - n_emit;
                    npts += s_n - n_emit;
                    const double ll = L1 - s_exit - gdd;
                    gseg = 2;
                    gdd = (L2 > 0.0) ? step : -step;
                    gpd = ((L1 * L2) > 0.0) ? (-gdd - ll) : (gdd - ll);
                    continue;
                }
                const double Ls = gseg == 0 ? L0 : (gseg == 1 ? L1 : L2);
                // the serial chain w_u = gpd (+ gdd) x u is the same in every lane: one f64 add
                // per step, lane 0 parks the values in the wave's LDS slots (gs) and lane pos + u
                // picks w_u up afterwards.  Within a segment the passing values form a prefix
                // (|pd| can only shrink before it grows), so the chain stops, 4 steps at a time,
                // once its latest value fails; lanes past the last generated value count as failed
                const int kk = lane - pos;
                const double aL = fabs(Ls);
                const int umax = 63 - pos;
                int u = umax;
                double v = gpd;
                // Closed form first: while the values keep w0's sign and exponent (one ulp u),
                // fl(w + d) = w + RN_u(d), so when the first two steps agree (w1 - w0 == w2 - w1
                // = delta; a tie-to-even would alternate them) w_k = w0 + k delta exactly — one
                // fma per lane, representable, so exact.  Checked over every value up to the
                // first one past |L|; any other pass (a binade or sign crossing inside the
                // chunk) takes the serial chain.  tests/test_walk_generator.py restates both.
                const double w1 = gpd + gdd, w2 = w1 + gdd;
                bool cf = (w1 - gpd) == (w2 - w1);
                if (cf) {
                    const double vc = __builtin_fma((double)(kk > 0 ? kk : 0), w1 - gpd, gpd);
                    const uint64_t fm = __ballot(kk >= 0 && !(fabs(vc) <= aL));
                    const int fl = fm ? (int)__builtin_ctzll(fm) : 63;
                    cf = __ballot(kk >= 0 && lane <= fl &&
                                  (__double2hiint(vc) >> 20) != (__double2hiint(gpd) >> 20)) == 0;
                    if (kk >= 0) v = vc;
                }
                if (!cf) {
                    double w = gpd;
                    if (lane == 0) gs[0] = w;
                    u = 0;
                    bool ended = !(fabs(w) <= aL);
                    while (!ended && u < umax) {
                        double t4[4];
#pragma unroll
                        for (int z = 0; z < 4; ++z) {
                            w += gdd;
                            t4[z] = w;
                        }
                        if (lane == 0) {
#pragma unroll
                            for (int z = 0; z < 4; ++z) gs[u + 1 + z] = t4[z];
                        }
                        u += 4;
                        ended = !(fabs(w) <= aL);
                    }
                    u = min(u, umax);
                    __builtin_amdgcn_wave_barrier();
                    v = (kk >= 0 && kk <= u) ? gs[kk] : gpd;
                }
                const uint64_t bad = __ballot(lane >= pos && (kk > u || !(fabs(v) <= aL)));
                const int m = bad ? (int)__builtin_ctzll(bad) : 64;
                if (lane >= pos && lane < m) {
                    my_seg = gseg;
                    my_pd = v;
                }
                if (m <= 63) {
                    const double pend = readlane_f64(v, m);
                    const double ll = Ls - pend - gdd;
                    if (++gseg < 3) {
                        const double Ln = gseg == 1 ? L1 : L2;
                        gdd = (Ln > 0.0) ? step : -step;
                        gpd = ((Ls * Ln) > 0.0) ? (-gdd - ll) : (gdd - ll);
                    }
                    cnt += m - pos;
                    pos = m;
                } else {
                    gpd = readlane_f64(v, 63) + gdd;
                    cnt += 64 - pos;
                    pos = 64;
                }
            }
            grid += cnt;
            done = gseg >= 3;
            // trim1: the last segment's final grid point landed in lane 63 (its next value is
            // past |L|): end here, so the drop below pops it in this chunk instead of one already
            // tested (the segment's end, dubins.rs:256, needs no ll: nothing follows)
            if (trim1 && !done && gseg == 2 && pos > 63 && !(fabs(gpd) <= fabs(L2))) {
                gseg = 3;
                done = true;
            }
        }
        // trim1 (prep_task): the chunk where the last segment ends pops its last grid point with
        // the endpoint; one generated in the previous chunk was tested already: literal path
        const bool drop = trim1 && done;
        if (drop && cnt == 0) return kLiteral;
        const int cnt_gen = cnt;  // grid points generated in this chunk (lanes 1 .. cnt_gen)
        if (drop) cnt -= 1;       // ... and kept
        const bool junction_here = done && cnt < 63;
        const bool isgen = lane >= 1 && lane <= cnt_gen;
        const bool isgrid = lane >= 1 && lane <= cnt;
        const bool isj = junction && junction_here && lane == cnt + 1;
        double qx = carry_x, qy = carry_y;
        int mm = kModeS;
        bool pop_more = false;  // the popped point's local x is 0.0 too: the trim goes on
        bool bad_arg = false;   // an arc point's pd outside sincos_small's range
        if (isgen) {
            const double* row = segt + kSegRow * my_seg;
            const double2 o2 = *reinterpret_cast<const double2*>(row);
            const double2 t2 = *reinterpret_cast<const double2*>(row + 2);
            mm = (int)row[4];
            const double ox = o2.x, oy = o2.y, ca = t2.x, sa = t2.y;
            const double pd = my_pd;
            double lx, ly;
            if (mm == kModeS) {
                const double pc = div_by(pd, c, rc);
                lx = ox + pc * ca;
                ly = oy + pc * sa;
            } else {
                // one argument reduction for both (walk -2..3%): ocml's own sincos, restated with
                // its constants behind an opaque pointer (sincos_small: no hoisted, spilled
                // coefficients); |pd| >= 2^30 (never on an L / R segment) goes to the literal path
                const double* tab = kSinCosTab;
                asm volatile("" : "+s"(tab));
                bad_arg = !(fabs(pd) < 0x1p30);
                double sp, cp;
                sincos_small(pd, tab, &sp, &cp);
                const double ldx = div_by(sp, c, rc);
                const double ld1 = div_by(1.0 - cp, c, rc);  // (1 - cos) / -c = -((1 - cos) / c)
                const double ldy = mm == kModeL ? ld1 : -ld1;
                const double gdx = ca * ldx + sa * ldy;
                const double gdy = -sa * ldx + ca * ldy;
                lx = ox + gdx;
                ly = oy + gdy;
            }
            qx = cw * lx + sw * ly + x;   // dubins.rs:415
            qy = -sw * lx + cw * ly + y;  // dubins.rs:420
            pop_more = drop && lane == cnt_gen && lx == 0.0;
        }
        if (isj) {
            qx = px;
            qy = py;
        }
        if (__any(pop_more || bad_arg)) return kLiteral;
        const bool has = lane == 0 || isgrid || isj;
        const bool chk = isgrid || isj || (base == 0 && lane == 0);
        npts += cnt + (junction && junction_here ? 1 : 0);
        napts += __popcll(__ballot(isgrid && mm != kModeS));
        if (chunk_rejects<kLds, kScene>(sc, has, chk, has && lane >= 1 && !(chord && lane == 1),
                                        qx, qy, !(chord && lane == 0)))
            return kReject;
        if (junction_here) break;
        // (the last point: lane 63, or lane cnt of a chunk ended before the chord)
        carry_x = readlane_f64(qx, cnt);
        carry_y = readlane_f64(qy, cnt);
    }
    // no trailing zero left for the trim (dubins.rs:281-288): the literal path decides
    if (1 + grid > (long long)ufl((double)p->n_point) - 2) return kLiteral;
    return kAccept;
}

// One edge on one wave from the wave-uniform SteerPrep of steer_prep(): the PrepRec that
// steer_prep_kernel would have written for it (segment trig of the origin yaws, the generator's
// initial state, no stored grid points), walked by walk_rec — the lane-parallel exact `pd`
// generator instead of the serial one of steer_walk.  junction = false: the polyline ends at the
// edge's last point (finalize's edge into the root).  gs: this wave's kGenSlots LDS doubles.
template <bool kLds, bool kS = false>
__device__ __forceinline__ int walk_edge(const SceneDev& sc, const SteerPrep& r, double* gs,
                                         bool junction, int& npts, int& napts) {
    if (r.state != kPrepWalk && r.state != kPrepNone) return r.state;
    PrepRec p;
    p.x = r.x;
    p.y = r.y;
    p.px = r.px;
    p.py = r.py;
    p.c = r.c;
    p.cw = r.cw;
    p.sw = r.sw;
    p.ox[0] = 0.0;
    p.oy[0] = 0.0;
    p.ox[1] = r.o1x;
    p.oy[1] = r.o1y;
    p.ox[2] = r.o2x;
    p.oy[2] = r.o2y;
    // segment trig (dubins.rs:155-198): S cos/sin(origin yaw), L/R cos/sin(-origin yaw)
    const double a0 = 0.0;
    const double a1 = r.m1 == kModeS ? r.o1yaw : -r.o1yaw;
    const double a2 = r.m2 == kModeS ? r.o2yaw : -r.o2yaw;
    p.ca[0] = cos(a0);
    p.sa[0] = sin(a0);
    p.ca[1] = cos(a1);
    p.sa[1] = sin(a1);
    p.ca[2] = cos(a2);
    p.sa[2] = sin(a2);
    p.L[0] = r.L0;
    p.L[1] = r.L1;
    p.L[2] = r.L2;
    p.m[0] = r.m0;
    p.m[1] = r.m1;
    p.m[2] = r.m2;
    p.cnt[0] = p.cnt[1] = p.cnt[2] = 0;
    p.n_point = r.n_point;
    p.state = r.state == kPrepNone ? kPrepNone : kPrepFallback;
    p.fb_dd = (r.L0 > 0.0) ? sc.step_size : -sc.step_size;
    p.fb_pd = p.fb_dd - 0.0;  // dubins.rs:239-241
    p.fb_seg = 0;
    p.trim1 = 0;
    p.yaw = p.pyaw = 0.0;
    return walk_rec<kLds, kSceneAny, kS>(sc, &p, gs, npts, napts, junction);
}

constexpr int kGenSlots = kGenPts + 3 * kSegRow;  // per-wave LDS doubles of walk_rec

// A literal-path scratch buffer (3 x kLiteralCap doubles) from a pool of kLiteralWaves slots,
// so kernels of any width can run the measure-zero literal path: lane 0 takes a free slot with
// atomicCAS (0 free, 1 taken), spinning over the pool if every slot is held — a holder is a
// running wave that releases after its bounded literal walk.  Called by all lanes.
__device__ __forceinline__ int lit_acquire(int* locks, int hint) {
    int slot = 0;
    if ((__lane_id()) == 0)
        for (int i = 0;; ++i) {
            const int sl = (hint + i) % kLiteralWaves;
            if (atomicCAS(&locks[sl], 0, 1) == 0) {
                slot = sl;
                break;
            }
        }
    slot = __shfl(slot, 0);
    __threadfence();
    return slot;
}
__device__ __forceinline__ void lit_release(int* locks, int slot) {
    __threadfence();
    if ((__lane_id()) == 0) atomicExch(&locks[slot], 0);
}

}  // namespace ppamd

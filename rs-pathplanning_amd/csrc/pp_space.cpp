// pp_space.cpp — the scene (Space): disc and polygon scenes, the occupancy grid, Space::verify.
#include "pp_ctx.h"

using namespace ppamd;

namespace {
static_assert(sizeof(scene::CullDisc) == sizeof(float4), "cull disc layout");

// n elements of src into b (room for at least one)
template <typename T>
int upload(DBuf<T>& b, const T* src, size_t n) {
    PP_HIP(b.reserve(std::max<size_t>(n, 1)));
    if (n > 0) PP_HIP(hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return PP_OK;
}

// upload the item grid (pp_scene.cpp) and its LDS image; set the scene's grid fields
int upload_item_grid(Scene& s, double minx, double maxx, double miny, double maxy,
                     const scene::Items& items) {
    const scene::ItemGrid g =
        scene::build_item_grid(minx, maxx, miny, maxy, items, scene::kLdsImage);
    const int m = (int)items.d4.size();
    int rc;
    if ((rc = upload(s.d_goff, g.goff.data(), g.goff.size()))) return rc;
    if ((rc = upload(s.d_gitems, g.gitems.data(), g.gitems.size()))) return rc;
    s.lds_bytes = g.lds_total;
    if (g.lds_total > 0) {
        PP_HIP(s.d_img.reserve((size_t)g.lds_total / 16));
        PP_HIP(hipMemcpy(s.d_img.p, g.image.data(), (size_t)g.lds_total, hipMemcpyHostToDevice));
    }
    s.lds_goff = g.o_goff;
    s.lds_items = g.o_items;
    s.lds_cx = s.lds_cy = s.lds_r2 = -1;
    s.lds_d4 = g.o_d4;
    s.gx0 = g.x0;
    s.gy0 = g.y0;
    s.ginv = g.ginv;
    s.gnx = g.gnx;
    s.gny = g.gny;
    PP_HIP(s.d_d4.reserve((size_t)std::max(m, 1)));
    if (m > 0) PP_HIP(hipMemcpy(s.d_d4.p, items.d4.data(), m * sizeof(float4), hipMemcpyHostToDevice));
    return PP_OK;
}

// reset the polygon-mode part of the scene (pp_space_new / pp_space_new_polygons)
void clear_polygons(Scene& s) {
    s.ibn = 0;  // (pp_space_new builds its inside bitmap after this)
    s.ne = 0;
    s.nbv = 0;
    s.h_ex0.clear();
    s.h_ey0.clear();
    s.h_ex1.clear();
    s.h_ey1.clear();
    s.h_epoly.clear();
    s.h_bvx.clear();
    s.h_bvy.clear();
}

// what both scene constructors end with: the shrunken bounds, the robot, and a fresh Space (a
// planner belongs to one Space: RRT::new moves it in, rrt.rs:342)
void install_scene(pp_ctx* ctx, double minx, double maxx, double miny, double maxy, double item_mx,
                   double robot_width, double robot_height, double max_steer, int m) {
    Scene& s = ctx->scene;
    const double half = robot_width / 2.0;
    s.h2 = half * half;
    s.cull_slack = scene::cull_slack_for(item_mx);
    s.minx = minx;
    s.maxx = maxx;
    s.miny = miny;
    s.maxy = maxy;
    s.width = robot_width;
    s.height = robot_height;
    s.max_steer = max_steer;
    s.m = m;
    s.has_grid = false;
    s.blocked_share = 0.0;
    s.valid = true;
    // the trees stay on the device: pp_rrt_revalidate / pp_batch_revalidate carry them over
    ctx->rrt.stale |= ctx->rrt.valid;
    ctx->batch.stale |= ctx->batch.valid;
    ctx->rrt.valid = false;
    ctx->batch.valid = false;
}

}  // namespace

extern "C" {

int pp_create_circle(double cx, double cy, double radius, double* xy, int cap, int* n) {
    if (!n || !(radius > 0.0) || cap < 0 || (cap > 0 && !xy))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad create_circle arguments");
    // rrt.rs:43-60: circum = 2 PI r; n = ceil(circum / 1.0); vertices 0..(n + 1) as usize
    const double kPi = 3.14159265358979323846;
    const double circum = 2.0 * kPi * radius;
    const double nf = std::ceil(circum / 1.0);
    if (!(nf < 1.0e8)) return set_err(PP_ERR_INVALID_ARGUMENT, "radius too large");
    const int count = (int)(nf + 1.0);
    *n = count;
    if (cap < count) return cap == 0 ? PP_OK : set_err(PP_ERR_CAPACITY, "vertex buffer too small");
    for (int i = 0; i < count; ++i) {
        const double a = 2.0 * kPi / nf * (double)i;
        xy[2 * i] = std::cos(a) * radius + cx;
        xy[2 * i + 1] = std::sin(a) * radius + cy;
    }
    return PP_OK;
}

int pp_space_new(pp_ctx* ctx, double x0, double y0, double x1, double y1, double robot_width,
                 double robot_height, double max_steer, const double* cx, const double* cy,
                 const double* r, int m) {
    int rc = check_ctx(ctx, false, false);
    if (rc) return rc;
    if (!(robot_width >= 0.0) || !(max_steer > 0.0))
        return set_err(PP_ERR_INVALID_ARGUMENT, "robot width must be >= 0 and max_steer > 0");
    const double box[4] = {x0, y0, x1, y1};
    if ((rc = check_coords(box, 4, 1, "bounds"))) return rc;
    scene::DiscScene ds;  // (disc_scene checks the discs against PP_COORD_MAX)
    std::string err;
    if ((rc = scene::disc_scene(x0, y0, x1, y1, robot_width, cx, cy, r, m, &ds, &err)))
        return set_err(rc, err);
    if ((rc = upload_item_grid(ctx->scene,ds.minx, ds.maxx, ds.miny, ds.maxy, ds.items))) return rc;
    Scene& s = ctx->scene;
    const size_t mm = (size_t)std::max(m, 0);
    if ((rc = upload(s.d_cx, cx, mm)) || (rc = upload(s.d_cy, cy, mm)) ||
        (rc = upload(s.d_r2, ds.r2.data(), mm)) || (rc = upload(s.d_rcull, ds.rcull.data(), mm)))
        return rc;
    clear_polygons(s);
    double ib_share = 0.0;
    {  // the inside bitmap: 2048^2 cells (512 KB, L2-resident)
        const scene::InsideBits ib =
            scene::inside_bitmap(ds.minx, ds.maxx, ds.miny, ds.maxy, cx, cy, ds.r2, kInsideCells);
        s.ibn = ib.n;
        if (ib.n > 0) {
            PP_HIP(s.d_ibits.reserve(ib.bits.size()));
            PP_HIP(hipMemcpy(s.d_ibits.p, ib.bits.data(), ib.bits.size() * sizeof(uint32_t),
                             hipMemcpyHostToDevice));
            s.ibx0 = ib.x0;
            s.iby0 = ib.y0;
            s.ibinv = ib.inv;
            // set cells over the cells of the sampling box (the bitmap is square, the box may not be)
            const double nx = std::min((double)ib.n, std::ceil((ds.maxx - ds.minx) * ib.inv));
            const double ny = std::min((double)ib.n, std::ceil((ds.maxy - ds.miny) * ib.inv));
            uint64_t set = 0;
            for (uint32_t w : ib.bits) set += (uint64_t)__builtin_popcount(w);
            if (nx >= 1.0 && ny >= 1.0) ib_share = std::min(1.0, (double)set / (nx * ny));
        }
    }
    install_scene(ctx, ds.minx, ds.maxx, ds.miny, ds.maxy, ds.items.mx, robot_width, robot_height,
                  max_steer, m);
    s.blocked_share = ib_share;
    return PP_OK;
}

int pp_space_new_polygons(pp_ctx* ctx, const double* bounds_xy, int nb, const double* obs_xy,
                          const int32_t* obs_off, int n_obs, double robot_width,
                          double robot_height, double max_steer) {
    int rc = check_ctx(ctx, false, false);
    if (rc) return rc;
    if (!bounds_xy || nb < 3 || n_obs < 0 || (n_obs > 0 && (!obs_xy || !obs_off)))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad polygon arrays (bounds need >= 3 vertices)");
    if (!(robot_width >= 0.0) || !(max_steer > 0.0))
        return set_err(PP_ERR_INVALID_ARGUMENT, "robot width must be >= 0 and max_steer > 0");
    scene::PolygonScene ps;  // (polygon_scene checks the vertices against PP_COORD_MAX)
    std::string err;
    if ((rc = scene::polygon_scene(bounds_xy, nb, obs_xy, obs_off, n_obs, robot_width, &ps, &err)))
        return set_err(rc, err);
    if ((rc = upload_item_grid(ctx->scene,ps.minx, ps.maxx, ps.miny, ps.maxy, ps.items))) return rc;
    Scene& s = ctx->scene;
    const size_t ne = ps.ex0.size();
    if ((rc = upload(s.d_ex0, ps.ex0.data(), ne)) || (rc = upload(s.d_ey0, ps.ey0.data(), ne)) ||
        (rc = upload(s.d_ex1, ps.ex1.data(), ne)) || (rc = upload(s.d_ey1, ps.ey1.data(), ne)) ||
        (rc = upload(s.d_epoly, ps.epoly.data(), ne)) ||
        (rc = upload(s.d_bvx, ps.bvx.data(), ps.bvx.size())) ||
        (rc = upload(s.d_bvy, ps.bvy.data(), ps.bvy.size())))
        return rc;
    s.h_ex0 = std::move(ps.ex0);
    s.h_ey0 = std::move(ps.ey0);
    s.h_ex1 = std::move(ps.ex1);
    s.h_ey1 = std::move(ps.ey1);
    s.h_epoly = std::move(ps.epoly);
    s.h_bvx = std::move(ps.bvx);
    s.h_bvy = std::move(ps.bvy);
    s.ne = (int)ne;
    s.nbv = (int)s.h_bvx.size();
    install_scene(ctx, ps.minx, ps.maxx, ps.miny, ps.maxy, ps.items.mx, robot_width, robot_height,
                  max_steer, 0);
    return PP_OK;
}

int pp_space_set_grid(pp_ctx* ctx, const uint32_t* bits, int w, int h, double x0, double y0,
                      double cell) {
    int rc = check_ctx(ctx, true, false);
    if (rc) return rc;
    if (!bits || w <= 0 || h <= 0 || w > (1 << 16) || h > (1 << 16) || !(cell > 0.0))
        return set_err(PP_ERR_INVALID_ARGUMENT, "bad occupancy grid");
    const double corners[4] = {x0, y0, x0 + w * cell, y0 + h * cell};
    if ((rc = check_coords(corners, 4, 1, "grid corners"))) return rc;
    const int words = (w + 31) / 32;
    const size_t n = (size_t)words * h;
    Scene& s = ctx->scene;
    if ((rc = upload(s.d_bits, bits, n))) return rc;
    s.bw = w;
    s.bh = h;
    s.bwords = words;
    s.bx0 = x0;
    s.by0 = y0;
    s.binv = 1.0 / cell;
    const size_t img_bytes = (n * sizeof(uint32_t) + 15) & ~(size_t)15;
    s.lds_bits_bytes = img_bytes <= 64 * 1024 ? (int)img_bytes : 0;
    if (s.lds_bits_bytes) {
        std::vector<uint32_t> img(img_bytes / 4, 0u);
        std::memcpy(img.data(), bits, n * sizeof(uint32_t));
        PP_HIP(s.d_gimg.reserve(img_bytes / 16));
        PP_HIP(hipMemcpy(s.d_gimg.p, img.data(), img_bytes, hipMemcpyHostToDevice));
    }
    s.has_grid = true;
    {
        uint64_t set = 0;
        for (size_t i = 0; i < n; ++i) set += (uint64_t)__builtin_popcount(bits[i]);
        s.blocked_share = std::min(1.0, (double)set / ((double)w * (double)h));
    }
    ctx->rrt.stale |= ctx->rrt.valid;
    ctx->rrt.valid = false;  // the planner's Space changed (rrt.rs:342)
    return PP_OK;
}

int pp_space_verify_batch(pp_ctx* ctx, const double* x, const double* y, const int64_t* off,
                          int k, uint8_t* ok) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    if (k < 0 || (k > 0 && (!off || !ok))) return set_err(PP_ERR_INVALID_ARGUMENT, "bad arguments");
    if (k == 0) return PP_OK;
    if (off[0] != 0) return set_err(PP_ERR_INVALID_ARGUMENT, "off[0] must be 0");
    for (int i = 0; i < k; ++i)
        if (off[i + 1] < off[i]) return set_err(PP_ERR_INVALID_ARGUMENT, "off must be non-decreasing");
    const int64_t np = off[k];
    if (np > 0 && (!x || !y)) return set_err(PP_ERR_INVALID_ARGUMENT, "null points");
    if ((r = check_coords(x, np, 1, "line points")) || (r = check_coords(y, np, 1, "line points")))
        return r;
    hipStream_t st = ctx->stream;
    DBuf<double> dx, dy;
    DBuf<int64_t> doff;
    DBuf<uint8_t> dok;
    PP_HIP(dx.reserve((size_t)std::max<int64_t>(np, 1)));
    PP_HIP(dy.reserve((size_t)std::max<int64_t>(np, 1)));
    PP_HIP(doff.reserve((size_t)k + 1));
    PP_HIP(dok.reserve((size_t)k));
    if (np > 0) {
        PP_HIP(hipMemcpyAsync(dx.p, x, np * sizeof(double), hipMemcpyHostToDevice, st));
        PP_HIP(hipMemcpyAsync(dy.p, y, np * sizeof(double), hipMemcpyHostToDevice, st));
    }
    PP_HIP(hipMemcpyAsync(doff.p, off, ((size_t)k + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    PP_HIP(launch_verify_lines(st, ctx->scene_dev(), dx.p, dy.p, doff.p, k, dok.p));
    PP_HIP(hipMemcpyAsync(ok, dok.p, (size_t)k, hipMemcpyDeviceToHost, st));
    PP_HIP(hipStreamSynchronize(st));
    return PP_OK;
}

int pp_space_get_bounds(pp_ctx* ctx, double out[4]) {
    int r = check_ctx(ctx, true, false);
    if (r) return r;
    if (!out) return set_err(PP_ERR_INVALID_ARGUMENT, "null output");
    out[0] = ctx->scene.minx;
    out[1] = ctx->scene.maxx;
    out[2] = ctx->scene.miny;
    out[3] = ctx->scene.maxy;
    return PP_OK;
}

}  // extern "C"

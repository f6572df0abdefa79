"""``pathplanning::rrt`` (src/rrt.rs) with the extend hot path on the GPU.

Same names and argument meaning as the crate: ``Robot``, ``create_circle``, ``Space``, ``Node``,
``RRT`` with ``get_nearest_node``, ``get_random_node``, ``verify_node``, ``plan_one`` and the
batched ``extend``.  Build-defined differences: obstacles are analytic discs
and the bounds an axis-aligned rectangle (Q10), sampling is a seeded stream (Q7), iterations run
with the sequential semantics of one rayon thread (Q8), the nearest neighbour is exact (Q9).
Polygon scenes (the example's JSON format) use exact Minkowski buffers in place of geo-offset
(Q10p).  ``plan()`` runs the goal connection (``check_finish``, ``optimize``, ``finalize``).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi, scenes


class Robot:  # rrt.rs:16-40
    def __init__(self, width: float, height: float, max_steer: float):
        self.width = float(width)
        self.height = float(height)
        self.max_steer = float(max_steer)  # used as the Dubins turn radius (rrt.rs:37-39 → 424)

    def get_width(self) -> float:
        return self.width

    def get_steer(self) -> float:
        return self.max_steer


@dataclass(frozen=True)
class Circle:
    """Analytic stand-in for ``create_circle``'s polygon (rrt.rs:43-60)."""
    cx: float
    cy: float
    r: float


def create_circle(center, radius: float) -> Circle:  # rrt.rs:43
    return Circle(float(center[0]), float(center[1]), float(radius))


def _rect_of(bounds):
    """(x0, y0, x1, y1) when ``bounds`` is a 4-tuple or an axis-aligned rectangle ring, else None."""
    b = np.asarray(bounds, dtype=np.float64)
    if b.shape == (4,):
        return tuple(b)
    b = scenes.ring(b)
    if len(b) != 4:
        return None
    xs, ys = b[:, 0], b[:, 1]
    x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
    if not np.all(((xs == x0) | (xs == x1)) & ((ys == y0) | (ys == y1))):
        return None
    return (x0, y0, x1, y1)


class Space:  # rrt.rs:70-159
    """``Space::new(bounds, robot, obstacles)``.

    Disc mode (configs 1-4): ``bounds`` an axis-aligned rectangle (4-tuple or ring) and every
    obstacle a ``Circle`` — analytic discs (Q10).  Polygon mode (§8f row 3, Q10p): any obstacle
    given as a polygon ring ((M, 2) array-like) or non-rectangular bounds; ``Circle`` obstacles
    then become the crate's ``create_circle`` polygons.  ``grid`` (config 4, build-defined): an
    occupancy grid ``(bits uint32[h, ceil(w/32)], w, x0, y0, cell)`` that replaces the discs —
    every point of a line must lie in a free cell (pp_space_set_grid)."""

    def __init__(self, bounds, robot: Robot, obstacle_list, grid=None):
        self.robot = robot
        self.grid = grid
        obs = list(obstacle_list)
        rect = _rect_of(bounds)
        self.polygon_mode = rect is None or any(not isinstance(o, Circle) for o in obs)
        half = robot.get_width() / 2.0  # rrt.rs:82
        if self.polygon_mode:
            if grid is not None:
                raise ValueError("an occupancy grid replaces disc obstacles, not polygons")
            b = np.asarray(bounds, dtype=np.float64)
            if b.shape == (4,):
                x0, y0, x1, y1 = b
                b = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
            self.bounds_polygon = scenes.ring(b)
            self.obstacle_polygons = [
                scenes.create_circle_polygon((o.cx, o.cy), o.r) if isinstance(o, Circle)
                else scenes.ring(o) for o in obs]
            bp = self.bounds_polygon
            self.raw_bounds = (bp[:, 0].min(), bp[:, 1].min(), bp[:, 0].max(), bp[:, 1].max())
            self.circles = np.zeros((0, 3))
        else:
            self.raw_bounds = rect
            self.circles = np.array([[o.cx, o.cy, o.r] for o in obs],
                                    dtype=np.float64).reshape(-1, 3)
        x0, y0, x1, y1 = self.raw_bounds
        self.minx, self.miny, self.maxx, self.maxy = x0 + half, y0 + half, x1 - half, y1 - half
        self._ctx = None

    @classmethod
    def from_raw(cls, raw: dict) -> "Space":
        if "bounds_polygon" in raw:
            return cls(raw["bounds_polygon"], Robot(*raw["robot"]), raw["obstacle_polygons"])
        return cls(raw["bounds"], Robot(*raw["robot"]),
                   [create_circle((c[0], c[1]), c[2]) for c in raw["circles"]],
                   grid=raw.get("grid"))

    def get_steer(self) -> float:
        return self.robot.get_steer()

    def get_bounds(self):
        """bbox of the shrunken bounds (minx, maxx, miny, maxy) — what rand_point samples."""
        return (self.minx, self.maxx, self.miny, self.maxy)

    def get_obs(self):
        """Disc mode: the inflated discs (cx, cy, r + width/2) (rrt.rs:108-111, 152-154).
        Polygon mode: the obstacle rings before buffering (the buffer is analytic, Q10p)."""
        if self.polygon_mode:
            return [p.copy() for p in self.obstacle_polygons]
        half = self.robot.get_width() / 2.0
        c = self.circles.copy()
        c[:, 2] += half
        return c

    def verify_batch(self, lines, ctx: _ffi.Context | None = None):
        """``Space::verify`` (rrt.rs:124-137) of many polylines (each (n, 2)) on the GPU: bool
        array.  Uses ``ctx`` (the scene is uploaded into it) or a context of its own."""
        if ctx is None:
            if self._ctx is None:
                self._ctx = _ffi.Context(0)
                self._upload(self._ctx)
            ctx = self._ctx
        else:
            self._upload(ctx)
        pts = [np.asarray(l, dtype=np.float64).reshape(-1, 2) for l in lines]
        off = np.zeros(len(pts) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(p) for p in pts])
        allp = np.concatenate(pts) if pts and off[-1] > 0 else np.zeros((1, 2))
        x = np.ascontiguousarray(allp[:, 0])
        y = np.ascontiguousarray(allp[:, 1])
        ok = np.zeros(len(pts), dtype=np.uint8)
        dp = C.POINTER(C.c_double)
        _ffi.check(_ffi.lib().pp_space_verify_batch(
            ctx.handle, x.ctypes.data_as(dp), y.ctypes.data_as(dp),
            off.ctypes.data_as(C.POINTER(C.c_int64)), len(pts),
            ok.ctypes.data_as(C.POINTER(C.c_uint8))))
        return ok.astype(bool)

    def verify(self, line, ctx: _ffi.Context | None = None) -> bool:
        """``Space::verify(&LineString) -> bool`` (rrt.rs:124-137)."""
        return bool(self.verify_batch([line], ctx)[0])

    def _upload(self, ctx: _ffi.Context):
        dp = C.POINTER(C.c_double)
        if self.polygon_mode:
            b = np.ascontiguousarray(self.bounds_polygon.reshape(-1))
            rings = self.obstacle_polygons
            off = np.zeros(len(rings) + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(r) for r in rings])
            o = np.ascontiguousarray(np.concatenate(rings).reshape(-1)) if rings else np.zeros(2)
            _ffi.check(_ffi.lib().pp_space_new_polygons(
                ctx.handle, b.ctypes.data_as(dp), len(self.bounds_polygon), o.ctypes.data_as(dp),
                off.ctypes.data_as(C.POINTER(C.c_int32)), len(rings), self.robot.width,
                self.robot.height, self.robot.max_steer))
            return
        c = np.ascontiguousarray(self.circles)
        cx, cy, r = (np.ascontiguousarray(c[:, k]) for k in range(3))
        x0, y0, x1, y1 = self.raw_bounds
        _ffi.check(_ffi.lib().pp_space_new(
            ctx.handle, x0, y0, x1, y1, self.robot.width, self.robot.height,
            self.robot.max_steer, cx.ctypes.data_as(dp), cy.ctypes.data_as(dp),
            r.ctypes.data_as(dp), len(cx)))
        if self.grid is not None:
            bits, w, gx0, gy0, cell = self.grid
            bits = np.ascontiguousarray(bits, dtype=np.uint32)
            _ffi.check(_ffi.lib().pp_space_set_grid(
                ctx.handle, bits.ctypes.data_as(C.POINTER(C.c_uint32)), int(w), bits.shape[0],
                float(gx0), float(gy0), float(cell)))


@dataclass
class Node:  # rrt.rs:161-214 (a view of one tree row)
    index: int
    x: float
    y: float
    yaw: float
    parent: int  # -1 for the root

    def get_point(self):
        return (self.x, self.y)

    def get_yaw(self):
        return self.yaw


class RRT:  # rrt.rs:325-620
    """``RRT::new(start, start_yaw, goal, goal_yaw, max_iter, step_size, space)`` (rrt.rs:335).

    Extra keyword arguments: ``seed`` (sampling stream), ``device`` (GPU ordinal), ``window``
    (samples screened per speculative GPU window; an iteration whose sample lies in an obstacle is
    rejected where it is drawn and takes none of them, so a window spans up to twice as many
    iterations; results do not depend on it), ``capacity`` (initial node capacity, grown on
    demand)."""

    def __init__(self, start, start_yaw, goal, goal_yaw, max_iter, step_size, space: Space,
                 seed: int = 0, device: int = 0, window: int = 4096, capacity: int = 1 << 16,
                 ctx: _ffi.Context | None = None):
        self.ctx = ctx or _ffi.Context(device)
        self.space = space
        self.goal = (float(goal[0]), float(goal[1]))
        self.goal_yaw = float(goal_yaw)
        self.max_iter = int(max_iter)
        self.step_size = float(step_size)
        self.seed = int(seed)
        space._upload(self.ctx)
        _ffi.check(_ffi.lib().pp_rrt_set_window(self.ctx.handle, int(window)))
        _ffi.check(_ffi.lib().pp_rrt_new(
            self.ctx.handle, float(start[0]), float(start[1]), float(start_yaw), self.goal[0],
            self.goal[1], self.goal_yaw, self.max_iter, self.step_size, self.seed, int(capacity)))

    # ---------------------------------------------------------------- hot path
    def extend(self, n_iter: int) -> int:
        """``n_iter`` × plan_one's extend (rrt.rs:583-589); returns the nodes inserted."""
        acc = C.c_int64(0)
        _ffi.check(_ffi.lib().pp_rrt_extend(self.ctx.handle, int(n_iter), C.byref(acc)))
        return acc.value

    def extend_samples(self, sx, sy, record: bool = True):
        """plan_one's extend (rrt.rs:583-589) over caller-drawn samples: iteration it + i takes
        (sx[i], sy[i]) as its rand_point (rrt.rs:139-146) — the host owns the RNG.  Returns the
        nodes inserted, or with ``record`` (nearest int32[k], yaw f64[k], ok bool[k]): per sample
        the nearest node of the tree as it stood (Node::new's parent), its yaw and whether it was
        inserted.  ``record=False`` lets the obstacle pre-test settle samples without their
        nearest node (faster)."""
        sx = np.ascontiguousarray(sx, dtype=np.float64)
        sy = np.ascontiguousarray(sy, dtype=np.float64)
        k = len(sx)
        if len(sy) != k:
            raise ValueError("sx and sy differ in length")
        acc = C.c_int64(0)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        if not record:
            _ffi.check(_ffi.lib().pp_rrt_extend_samples(
                self.ctx.handle, sx.ctypes.data_as(dp), sy.ctypes.data_as(dp), k, None, None, None,
                C.byref(acc)))
            return acc.value
        nearest = np.zeros(k, dtype=np.int32)
        yaw = np.zeros(k)
        ok = np.zeros(k, dtype=np.uint8)
        _ffi.check(_ffi.lib().pp_rrt_extend_samples(
            self.ctx.handle, sx.ctypes.data_as(dp), sy.ctypes.data_as(dp), k,
            nearest.ctypes.data_as(ip), yaw.ctypes.data_as(dp),
            ok.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(acc)))
        return nearest, yaw, ok.astype(bool)

    def tree_import(self, x, y, yaw, parent):
        """Replace the tree by host-owned nodes (root first, parent -1 for the root, otherwise an
        earlier node); the iteration counter, scene and goal stay."""
        x, y, yaw = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, yaw))
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        if not (len(x) == len(y) == len(yaw) == len(parent)):
            raise ValueError("tree arrays differ in length")
        dp = C.POINTER(C.c_double)
        _ffi.check(_ffi.lib().pp_rrt_tree_import(
            self.ctx.handle, x.ctypes.data_as(dp), y.ctypes.data_as(dp), yaw.ctypes.data_as(dp),
            parent.ctypes.data_as(C.POINTER(C.c_int32)), len(x)))

    def revalidate(self, n_old: int | None = None):
        """Re-verify the tree against the context's current scene and drop every node whose
        line_to_origin no longer verifies (pp_rrt_revalidate; the root stays, kept nodes keep
        their order and poses).  Returns (n_kept, new_index int32[old n]): a node's index
        afterwards, -1 when dropped.  ``n_old``: the tree's size, for a planner whose scene was
        replaced behind its back (``tree_size`` refuses then)."""
        n_old = self.tree_size() if n_old is None else int(n_old)
        new_index = np.zeros(max(n_old, 1), dtype=np.int32)
        kept = C.c_int64(0)
        _ffi.check(_ffi.lib().pp_rrt_revalidate(
            self.ctx.handle, C.byref(kept), new_index.ctypes.data_as(C.POINTER(C.c_int32))))
        return kept.value, new_index[:n_old]

    def set_space(self, space: Space):
        """Replace the scene and keep the tree where it still verifies: uploads ``space`` into
        the planner's context and revalidates.  Returns (n_kept, new_index) as ``revalidate``."""
        n_old = self.tree_size()
        space._upload(self.ctx)
        self.space = space
        return self.revalidate(n_old)

    def plan_one(self) -> bool:
        """plan_one's extend (rrt.rs:583-589): True when the node was inserted."""
        acc = C.c_int32(0)
        _ffi.check(_ffi.lib().pp_rrt_plan_one(self.ctx.handle, C.byref(acc)))
        return bool(acc.value)

    def set_window(self, k: int):
        _ffi.check(_ffi.lib().pp_rrt_set_window(self.ctx.handle, int(k)))

    # ---------------------------------------------------------------- queries
    def tree_size(self) -> int:
        n = C.c_int64(0)
        _ffi.check(_ffi.lib().pp_rrt_tree_size(self.ctx.handle, C.byref(n)))
        return n.value

    def iteration(self) -> int:
        it = C.c_int64(0)
        _ffi.check(_ffi.lib().pp_rrt_iteration(self.ctx.handle, C.byref(it)))
        return it.value

    def tree(self):
        """(x, y, yaw, parent) arrays, root first."""
        n = self.tree_size()
        x, y, yaw = np.zeros(n), np.zeros(n), np.zeros(n)
        par = np.zeros(n, dtype=np.int32)
        out = C.c_int64(0)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _ffi.check(_ffi.lib().pp_rrt_tree_export(
            self.ctx.handle, x.ctypes.data_as(dp), y.ctypes.data_as(dp), yaw.ctypes.data_as(dp),
            par.ctypes.data_as(ip), n, C.byref(out)))
        return x, y, yaw, par

    def node(self, i: int) -> Node:
        x, y, yaw, par = self.tree()
        return Node(i, x[i], y[i], yaw[i], int(par[i]))

    def get_nearest_node_batch(self, qx, qy):
        """RRT::get_nearest_node (rrt.rs:378-391) for many points: (index, d2) arrays."""
        qx = np.ascontiguousarray(qx, dtype=np.float64)
        qy = np.ascontiguousarray(qy, dtype=np.float64)
        k = len(qx)
        idx = np.zeros(k, dtype=np.int32)
        d2 = np.zeros(k)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _ffi.check(_ffi.lib().pp_rrt_get_nearest_node_batch(
            self.ctx.handle, qx.ctypes.data_as(dp), qy.ctypes.data_as(dp), k,
            idx.ctypes.data_as(ip), d2.ctypes.data_as(dp)))
        return idx, d2

    def get_nearest_node(self, point) -> int:
        idx, _ = self.get_nearest_node_batch([point[0]], [point[1]])
        return int(idx[0])

    def get_random_node(self, it: int | None = None):
        """rrt.rs:406-412: (x, y, nearest index, yaw) of iteration ``it``'s sample (default: the
        next iteration) — does not advance the planner."""
        it = self.iteration() if it is None else int(it)
        x0, x1, y0, y1 = self.space.get_bounds()
        x = _ffi.lib().pp_gen_range(self.seed, 2 * it, x0, x1)
        y = _ffi.lib().pp_gen_range(self.seed, 2 * it + 1, y0, y1)
        p = self.get_nearest_node((x, y))
        tx, ty, _, _ = self.tree()
        return x, y, p, float(np.arctan2(ty[p] - y, tx[p] - x))

    def verify_node_batch(self, x, y, parent):
        """verify_node(Node::new(point, tree[parent])) (rrt.rs:169-175, 414-426): (ok, yaw)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        k = len(x)
        ok = np.zeros(k, dtype=np.uint8)
        yaw = np.zeros(k)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _ffi.check(_ffi.lib().pp_rrt_verify_node_batch(
            self.ctx.handle, x.ctypes.data_as(dp), y.ctypes.data_as(dp),
            parent.ctypes.data_as(ip), k, ok.ctypes.data_as(C.POINTER(C.c_uint8)),
            yaw.ctypes.data_as(dp)))
        return ok.astype(bool), yaw

    def verify_node(self, x, y, parent) -> bool:
        ok, _ = self.verify_node_batch([x], [y], [parent])
        return bool(ok[0])

    def line_to_origin(self, node: int):
        """line_to_origin (rrt.rs:291-321) of tree node ``node``: the (n, 2) polyline node -> root
        (each edge steered on the GPU with R = Robot.max_steer and the planner's step)."""
        n = C.c_int64(0)
        _ffi.check(_ffi.lib().pp_rrt_line_to_origin(self.ctx.handle, int(node), None, None, 0,
                                                    C.byref(n)))
        x, y = np.zeros(max(n.value, 1)), np.zeros(max(n.value, 1))
        dp = C.POINTER(C.c_double)
        _ffi.check(_ffi.lib().pp_rrt_line_to_origin(self.ctx.handle, int(node),
                                                    x.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                                    n.value, C.byref(n)))
        return np.stack([x[:n.value], y[:n.value]], axis=1)

    # ---------------------------------------------------------------- goal connection
    def optimize(self, node: int, i: int = 0):
        """RRT::optimize(node, i) (rrt.rs:463-487): None, or the list of tree nodes the returned
        chain of copies connects to, level by level (the last one is the tree node it ends at)."""
        chain = np.zeros(16, dtype=np.int32)
        n = C.c_int(0)
        _ffi.check(_ffi.lib().pp_rrt_optimize(self.ctx.handle, int(node), int(i),
                                              chain.ctypes.data_as(C.POINTER(C.c_int32)),
                                              C.byref(n)))
        return None if n.value == 0 else chain[:n.value].tolist()

    def finalize(self, goal, goal_yaw: float, parent: int):
        """RRT::finalize (rrt.rs:489-540) of the goal node Node::new_goal(goal, parent, goal_yaw):
        ((n, 2) line, verified) — the line whether or not it verifies."""
        n = C.c_int64(0)
        ok = C.c_uint8(0)
        gx, gy = goal
        L = _ffi.lib()
        _ffi.check(L.pp_rrt_finalize(self.ctx.handle, float(gx), float(gy), float(goal_yaw),
                                     int(parent), None, None, 0, C.byref(n), C.byref(ok)))
        x, y = np.zeros(max(n.value, 1)), np.zeros(max(n.value, 1))
        dp = C.POINTER(C.c_double)
        _ffi.check(L.pp_rrt_finalize(self.ctx.handle, float(gx), float(gy), float(goal_yaw),
                                     int(parent), x.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                     n.value, C.byref(n), C.byref(ok)))
        return np.stack([x[:n.value], y[:n.value]], axis=1), bool(ok.value)

    def check_finish_batch(self, nodes, with_length: bool = True):
        """RRT::check_finish (rrt.rs:428-438) for many tree nodes: dict of arrays ``ok``,
        ``length`` / ``n_points`` (verified lines only) and ``chain`` (rows of
        [levels, edges, optimize's chosen ancestor per level...])."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        k = len(nodes)
        ok = np.zeros(k, dtype=np.uint8)
        length = np.zeros(k)
        npts = np.zeros(k, dtype=np.int32)
        chain = np.zeros((k, _ffi.PP_CF_CHAIN), dtype=np.int32)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _ffi.check(_ffi.lib().pp_rrt_check_finish_batch(
            self.ctx.handle, nodes.ctypes.data_as(ip), k, ok.ctypes.data_as(C.POINTER(C.c_uint8)),
            length.ctypes.data_as(dp) if with_length else None,
            npts.ctypes.data_as(ip) if with_length else None, chain.ctypes.data_as(ip)))
        return {"ok": ok.astype(bool), "length": length, "n_points": npts, "chain": chain}

    def check_finish(self, node: int):
        """RRT::check_finish for one tree node: the finalized line as an (n, 2) array (root side
        first, rrt.rs:538), or None when it does not verify."""
        ok = C.c_uint8(0)
        n, ln = C.c_int64(0), C.c_double(0)
        _ffi.check(_ffi.lib().pp_rrt_check_finish(self.ctx.handle, int(node), C.byref(ok), None,
                                                  None, 0, C.byref(n), C.byref(ln)))
        if not ok.value:
            return None
        cap = n.value
        x, y = np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
        dp = C.POINTER(C.c_double)
        _ffi.check(_ffi.lib().pp_rrt_check_finish(
            self.ctx.handle, int(node), C.byref(ok), x.ctypes.data_as(dp), y.ctypes.data_as(dp),
            cap, C.byref(n), C.byref(ln)))
        return np.stack([x[:n.value], y[:n.value]], axis=1)

    def plan(self, n_iter: int | None = None):
        """RRT::plan (rrt.rs:599-619), sequential spec: ``n_iter`` (default max_iter) plan_one
        iterations, check_finish on every accepted node; the line with the minimum
        euclidean_length (first on ties) or None.  ``self.last_plan`` keeps (node, length,
        finishes)."""
        bn, bl, nf = C.c_int32(-1), C.c_double(0), C.c_int64(0)
        n_iter = self.max_iter if n_iter is None else int(n_iter)
        _ffi.check(_ffi.lib().pp_rrt_plan(self.ctx.handle, n_iter, C.byref(bn), C.byref(bl),
                                          C.byref(nf)))
        self.last_plan = (bn.value, bl.value, nf.value)
        if bn.value < 0:
            return None
        return self.check_finish(bn.value)

    # ---------------------------------------------------------------- instrumentation
    def stats(self) -> dict:
        s = _ffi.StatsC()
        _ffi.check(_ffi.lib().pp_rrt_get_stats(self.ctx.handle, C.byref(s), C.sizeof(s)))
        return s.as_dict()

    def reset_stats(self):
        _ffi.check(_ffi.lib().pp_rrt_reset_stats(self.ctx.handle))

    def set_profiling(self, on: bool):
        _ffi.check(_ffi.lib().pp_set_profiling(self.ctx.handle, int(bool(on))))

    def synchronize(self):
        _ffi.check(_ffi.lib().pp_synchronize(self.ctx.handle))

    def close(self):
        self.ctx.close()


_I32P = C.POINTER(C.c_int32)


def _compact_trees(ctx, q, n_old, fn, lead, n_counters):
    """One call that compacts a forest's trees (revalidate, repair, advance, prune):
    ``fn(ctx, *lead, n_nodes, <n_counters int64 counters>, new_index)``.  ``n_old``: the q old
    sizes.  Returns (n_nodes int32[q] after the call, new_index int32[sum of the old sizes], the
    counters)."""
    n_old = np.asarray(n_old)
    total = int(n_old.sum(dtype=np.int64))
    new_index = np.zeros(max(total, 1), dtype=np.int32)
    n = np.zeros(q, dtype=np.int32)
    counters = [C.c_int64(0) for _ in range(n_counters)]
    _ffi.check(fn(ctx.handle, *lead, n.ctypes.data_as(_I32P), *map(C.byref, counters),
                  new_index.ctypes.data_as(_I32P)))
    return n, new_index[:total], [c.value for c in counters]


def _forest_slots(queries, q):
    """(slot array or None, its ctypes pointer or None, m) of an export / import call"""
    if queries is None:
        return None, None, q
    s = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
    return s, s.ctypes.data_as(C.POINTER(C.c_int32)), len(s)


def _forest_struct(kind, arrays):
    """pp_forest_state over the dict's arrays of this batch kind ('s' RRT*, 'b' extend)"""
    st = _ffi.ForestStateC()
    st.size = C.sizeof(st)
    for name, (_, _, kinds) in _ffi.FOREST_FIELDS.items():
        a = arrays.get(name)
        if a is not None and kind in kinds:
            setattr(st, name, a.ctypes.data_as(type(getattr(st, name))))
    return st


def _forest_export(ctx, kind, q, queries):
    """pp_star_forest_export / pp_batch_forest_export: the sizes, then the rows.  A dict of numpy
    arrays (``_ffi.FOREST_FIELDS``), usable with ``np.savez`` / ``np.load`` as it is."""
    L = _ffi.lib()
    fn = L.pp_star_forest_export if kind == "s" else L.pp_batch_forest_export
    _, sp, m = _forest_slots(queries, q)
    out = {name: np.zeros(m * per + (name == "off"), dtype=dt)
           for name, (dt, per, kinds) in _ffi.FOREST_FIELDS.items() if per and kind in kinds}
    tot = C.c_int64(0)
    st = _forest_struct(kind, out)
    _ffi.check(fn(ctx.handle, sp, m, C.byref(st), 0, C.byref(tot)))
    n = tot.value
    for name, (dt, per, kinds) in _ffi.FOREST_FIELDS.items():
        if not per and kind in kinds:
            out[name] = np.zeros(n, dtype=dt)
    st = _forest_struct(kind, out)
    _ffi.check(fn(ctx.handle, sp, m, C.byref(st), n, C.byref(tot)))
    if "focus_xy" in out:
        out["focus_xy"] = out["focus_xy"].reshape(m, 2)
    if "goals" in out:
        out["goals"] = out["goals"].reshape(m, 3)
    return out


def _forest_import(ctx, kind, state, queries):
    """pp_star_forest_import / pp_batch_forest_import of a state dict (a missing or None entry is
    passed as NULL: only ``cost`` may be).  A refused call raises PPError with ``bad_query`` = the
    first offending slot (-1: none named) and leaves the batch as it was."""
    L = _ffi.lib()
    fn = L.pp_star_forest_import if kind == "s" else L.pp_batch_forest_import
    arrays = {}
    if state is not None:
        for name, (dt, _, kinds) in _ffi.FOREST_FIELDS.items():
            if kind in kinds and state.get(name) is not None:
                arrays[name] = np.ascontiguousarray(state[name], dtype=dt).reshape(-1)
    m = len(arrays["off"]) - 1 if "off" in arrays else 0
    _, sp, mq = _forest_slots(queries, m)
    if queries is not None and mq != m and state is not None:
        raise ValueError(f"{mq} query slots for a state of {m} trees")
    for name, (_, per, kinds) in _ffi.FOREST_FIELDS.items():
        if name in arrays and name != "off":
            want = m * per if per else int(arrays["off"][-1]) if m > 0 else 0
            if len(arrays[name]) < want:
                raise ValueError(f"state[{name!r}] holds {len(arrays[name])} entries, {want} needed")
    bad = C.c_int32(-1)
    st = _forest_struct(kind, arrays)
    try:
        _ffi.check(fn(ctx.handle, sp, mq, C.byref(st) if state is not None else None,
                      C.byref(bad)))
    except _ffi.PPError as e:
        e.bad_query = bad.value
        raise


def _forest_roots(kind, starts, seeds, goals=None):
    """the state of root-only trees: what pp_star_new / pp_batch_new leave in a slot"""
    starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
    m = len(starts)
    st = {"off": np.arange(m + 1, dtype=np.int64), "x": starts[:, 0].copy(),
          "y": starts[:, 1].copy(), "yaw": starts[:, 2].copy(),
          "parent": np.full(m, -1, dtype=np.int32), "iterations": np.zeros(m, dtype=np.int64),
          "seeds": np.ascontiguousarray(seeds, dtype=np.uint64).reshape(m),
          "node_evals": np.zeros(m, dtype=np.int64)}
    if kind == "s":
        st.update(cost=np.zeros(m), edge_cost=np.zeros(m), rewires=np.zeros(m, dtype=np.int64),
                  focus_xy=np.zeros((m, 2)), focus_bound=np.full(m, np.inf),
                  skipped=np.zeros(m, dtype=np.int64))
    else:
        st["goals"] = np.ascontiguousarray(goals, dtype=np.float64).reshape(m, 3)
    return st


def _segments_struct(seg):
    """A PathSegmentsC over the five arrays of ``seg`` (float64, contiguous; a missing or None
    entry: NULL), and the arrays it points into."""
    st = _ffi.PathSegmentsC()
    st.size = C.sizeof(st)
    keep = {}
    for name in _ffi.SEGMENT_FIELDS:
        a = seg.get(name)
        if a is None:
            continue
        keep[name] = np.ascontiguousarray(a, dtype=np.float64)
        setattr(st, name, keep[name].ctypes.data_as(C.POINTER(C.c_double)))
    return st, keep


def _path_segments(q, call):
    """The two-call protocol of pp_star_path_segments / pp_batch_path_segments: ``call(off, seg,
    cap, tot, length, ok)`` binds everything in front of ``off``."""
    i64, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    off = np.zeros(q + 1, dtype=np.int64)
    ok = np.zeros(q, dtype=np.uint8)
    length = np.zeros(q)
    tot = C.c_int64(0)
    okp = ok.ctypes.data_as(C.POINTER(C.c_uint8))
    _ffi.check(call(off.ctypes.data_as(i64), None, 0, C.byref(tot), None, okp))
    cap = tot.value
    seg = {name: np.zeros(cap) for name in _ffi.SEGMENT_FIELDS}
    if cap > 0:
        st, _ = _segments_struct(seg)
        _ffi.check(call(off.ctypes.data_as(i64), C.byref(st), cap, C.byref(tot),
                        length.ctypes.data_as(dp), okp))
    return off, seg, length, ok.astype(bool)


def sample_segments(ctx, off, seg, ds):
    """Sample rows of Dubins segments every ``ds`` along the arc (pp_segments_sample): row r =
    entries ``off[r]:off[r + 1]`` of the five arrays of the dict ``seg`` (``path_segments``'
    output, or hand-built).  Samples at s = 0, ds, 2 ds, ... and one more at the row's end when
    that is past the last; position and yaw by the segments' closed forms (yaw unwrapped), the
    segment's curvature.  Returns (poff int64[q + 1], x, y, yaw, kappa, s): row r's samples are
    ``[poff[r]:poff[r + 1]]``.  A pure function of its arguments; ``ctx``: any context."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    q = len(off) - 1
    st, keep = _segments_struct(seg)
    i64, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    poff = np.zeros(q + 1, dtype=np.int64)
    tot = C.c_int64(0)
    L = _ffi.lib()
    _ffi.check(L.pp_segments_sample(ctx.handle, q, off.ctypes.data_as(i64), C.byref(st),
                                    float(ds), poff.ctypes.data_as(i64), None, None, None, None,
                                    None, 0, C.byref(tot)))
    cap = tot.value
    out = [np.zeros(cap) for _ in range(5)]
    if cap > 0:
        _ffi.check(L.pp_segments_sample(ctx.handle, q, off.ctypes.data_as(i64), C.byref(st),
                                        float(ds), poff.ctypes.data_as(i64),
                                        *[a.ctypes.data_as(dp) for a in out], cap, C.byref(tot)))
    del keep
    return (poff, *out)


class RRTBatch:
    """Many independent planners on one scene (BASELINE config 3): ``RRT::new`` per query
    (rrt.rs:335-355) with its own start, goal and sampling stream, advanced in lockstep — one
    plan_one extend iteration (rrt.rs:583-589) of every query per step — on one GPU.  ``window``:
    iterations per query evaluated speculatively per GPU step (a power of two <= 64, 0 =
    automatic: 32, halved while a step would hold more than 262144 tasks); every query's tree
    equals its sequential run."""

    def __init__(self, starts, goals, max_iter, step_size, space: Space, seeds, device: int = 0,
                 ctx: _ffi.Context | None = None, window: int = 0):
        self.ctx = ctx or _ffi.Context(device)
        self.space = space
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        goals = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        self.q = len(starts)
        self.max_iter = int(max_iter)
        space._upload(self.ctx)
        # iterations per query evaluated per GPU step (0: automatic); results do not depend on it
        _ffi.check(_ffi.lib().pp_batch_set_window(self.ctx.handle, int(window)))
        dp = C.POINTER(C.c_double)
        _ffi.check(_ffi.lib().pp_batch_new(
            self.ctx.handle, self.q, starts.ctypes.data_as(dp), goals.ctypes.data_as(dp),
            seeds.ctypes.data_as(C.POINTER(C.c_uint64)), self.max_iter, float(step_size)))

    def extend(self, n_steps: int):
        """n_steps lockstep steps; returns (iterations consumed, nodes inserted) over the batch."""
        it, acc = C.c_int64(0), C.c_int64(0)
        _ffi.check(_ffi.lib().pp_batch_extend(self.ctx.handle, int(n_steps), C.byref(it),
                                              C.byref(acc)))
        return it.value, acc.value

    def set_finish_schedule(self, rounds: bool = True, span0: int = 0, span: int = 0):
        """How plan() runs check_finish (identical results): steer rounds with span0 / span
        candidate edges per node in the first / later rounds (0 = default), or rounds=False:
        check_finish_kernel alone."""
        _ffi.check(_ffi.lib().pp_batch_set_finish_schedule(self.ctx.handle, int(bool(rounds)),
                                                           int(span0), int(span)))

    def set_window(self, k: int):
        """The window for the following extend calls (a power of two <= 64); the trees do not
        depend on it."""
        _ffi.check(_ffi.lib().pp_batch_set_window(self.ctx.handle, int(k)))

    def state(self, with_evals: bool = False):
        """(tree sizes int32[q], iterations int64[q]) [+ NN node-distance evals int64[q]]."""
        n = np.zeros(self.q, dtype=np.int32)
        it = np.zeros(self.q, dtype=np.int64)
        ev = np.zeros(self.q, dtype=np.int64)
        i64 = C.POINTER(C.c_int64)
        _ffi.check(_ffi.lib().pp_batch_state(self.ctx.handle,
                                             n.ctypes.data_as(C.POINTER(C.c_int32)),
                                             it.ctypes.data_as(i64), ev.ctypes.data_as(i64)))
        return (n, it, ev) if with_evals else (n, it)

    def stats(self) -> dict:
        s = _ffi.StatsC()
        _ffi.check(_ffi.lib().pp_rrt_get_stats(self.ctx.handle, C.byref(s), C.sizeof(s)))
        return s.as_dict()

    def set_profiling(self, on: bool):
        _ffi.check(_ffi.lib().pp_set_profiling(self.ctx.handle, int(bool(on))))

    def revalidate(self, n_old=None):
        """Re-verify every query's tree against the context's current scene (pp_batch_revalidate)
        and drop the nodes whose line_to_origin no longer verifies.  Returns (n_nodes int32[q]
        after the call, new_index int32[sum of the old sizes]): query q's entries start at the
        prefix sum of the old sizes, each a node's index in its tree afterwards or -1.
        ``n_old``: the old sizes, for a batch whose scene was replaced behind its back."""
        n, new_index, (self.last_dropped,) = _compact_trees(
            self.ctx, self.q, self.state()[0] if n_old is None else n_old,
            _ffi.lib().pp_batch_revalidate, (), 1)
        return n, new_index

    def set_space(self, space: Space):
        """Replace the scene of the batch and keep every tree where it still verifies."""
        n_old = self.state()[0]
        space._upload(self.ctx)
        self.space = space
        return self.revalidate(n_old)

    def plan(self):
        """RRT::plan (rrt.rs:599-619) of every query on its tree as extended so far: check_finish
        of every node the query inserted, the first minimum euclidean_length.  dict of per-query
        arrays ``best_node`` (-1: None), ``length`` (inf: None), ``n_points`` (of the finalized
        line), ``n_finishes``; ``checked`` = the (query, node) pairs checked."""
        bn = np.zeros(self.q, dtype=np.int32)
        ln = np.zeros(self.q)
        npts = np.zeros(self.q, dtype=np.int32)
        nf = np.zeros(self.q, dtype=np.int32)
        chk = C.c_int64(0)
        ip = C.POINTER(C.c_int32)
        _ffi.check(_ffi.lib().pp_batch_plan(
            self.ctx.handle, bn.ctypes.data_as(ip), ln.ctypes.data_as(C.POINTER(C.c_double)),
            npts.ctypes.data_as(ip), nf.ctypes.data_as(ip), C.byref(chk)))
        return {"best_node": bn, "length": ln, "n_points": npts, "n_finishes": nf,
                "checked": chk.value}

    def paths(self, nodes=None):
        """The finalized lines of every query in one call (pp_batch_paths): row q is the line
        ``RRT.check_finish(nodes[q])`` returns on query q's tree with its goal, root side first.
        ``nodes``: one node per query (-1: skip), or None: the best nodes of a ``plan()`` run
        here (kept in ``self.last_plan``).  Returns (off int64[q + 1], xy float64[n, 2],
        ok bool[q]): row q = ``xy[off[q]:off[q + 1]]``, empty where ``ok[q]`` is False."""
        L = _ffi.lib()
        ip, dp, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        u8 = C.POINTER(C.c_uint8)
        off = np.zeros(self.q + 1, dtype=np.int64)
        ok = np.zeros(self.q, dtype=np.uint8)
        tot = C.c_int64(0)
        if nodes is None:
            # the plan's n_points are the rows' sizes: one call
            self.last_plan = self.plan()
            nodes = self.last_plan["best_node"]
            cap = int(self.last_plan["n_points"].sum(dtype=np.int64))
        else:
            nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(self.q)
            _ffi.check(L.pp_batch_paths(self.ctx.handle, nodes.ctypes.data_as(ip),
                                        off.ctypes.data_as(i64), None, None, 0, C.byref(tot),
                                        ok.ctypes.data_as(u8)))
            cap = tot.value
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        x, y = np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
        if cap > 0:
            _ffi.check(L.pp_batch_paths(self.ctx.handle, nodes.ctypes.data_as(ip),
                                        off.ctypes.data_as(i64), x.ctypes.data_as(dp),
                                        y.ctypes.data_as(dp), cap, C.byref(tot),
                                        ok.ctypes.data_as(u8)))
        return off, np.stack([x[:tot.value], y[:tot.value]], axis=1), ok.astype(bool)

    def path_segments(self, nodes=None, reverse=False):
        """The rows of ``paths(nodes)`` as Dubins segments (pp_batch_path_segments): every edge of
        finalize's chain as three arc / straight / arc records.  Returns (off int64[q + 1], seg,
        length float64[q], ok bool[q]): ``seg`` a dict of float64 arrays ``x``, ``y``, ``yaw``
        (the segment's start pose, yaw unwrapped), ``kappa`` (signed curvature) and ``len``; row q
        = entries ``off[q]:off[q + 1]``, three per edge, in generation order (goal edge first,
        headings as stored) or, ``reverse``, the same curve from the root to the goal (``paths``'
        order).  ``nodes`` as in ``paths``."""
        if nodes is None:
            self.last_plan = self.plan()
            nodes = self.last_plan["best_node"]
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(self.q)
        L, h, ip = _ffi.lib(), self.ctx.handle, C.POINTER(C.c_int32)
        return _path_segments(self.q, lambda *a: L.pp_batch_path_segments(
            h, nodes.ctypes.data_as(ip), int(bool(reverse)), *a))

    def trajectories(self, ds, nodes=None, reverse=True):
        """``path_segments(nodes, reverse)`` sampled every ``ds`` (``sample_segments``): (poff, x,
        y, yaw, kappa, s), root to goal by default."""
        off, seg, _, _ = self.path_segments(nodes, reverse)
        return sample_segments(self.ctx, off, seg, ds)

    def tree(self, query: int, n: int | None = None):
        """(x, y, yaw, parent) of one query's tree, root first (``n``: its size, when known)."""
        n = int(self.state()[0][query]) if n is None else int(n)
        x, y, yaw = np.zeros(n), np.zeros(n), np.zeros(n)
        par = np.zeros(n, dtype=np.int32)
        out = C.c_int64(0)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _ffi.check(_ffi.lib().pp_batch_tree_export(
            self.ctx.handle, int(query), x.ctypes.data_as(dp), y.ctypes.data_as(dp),
            yaw.ctypes.data_as(dp), par.ctypes.data_as(ip), n, C.byref(out)))
        return x, y, yaw, par

    # ---- forest export / import (pp_batch_forest_export / _import)
    def export_forest(self, queries=None):
        """The complete state of the slots ``queries`` (distinct, any order; None: all) in one
        call, packed: a dict of numpy arrays — ``off`` int64[m + 1] (slot i's tree is rows
        off[i]:off[i + 1]), rows ``x``, ``y``, ``yaw``, ``parent``, per slot ``iterations``,
        ``seeds``, ``node_evals``, ``goals`` [m, 3].  ``np.savez(path, **state)`` is a checkpoint.
        The batch is not modified."""
        return _forest_export(self.ctx, "b", self.q, queries)

    def import_forest(self, state, queries=None):
        """Write such a state into the slots ``queries`` (None: 0 .. m - 1) of this batch — of any
        size, on the same scene, step size and max_iter; the other slots stay untouched.  The
        slots then continue exactly as the exported ones would have.  Validated as a whole first
        (parents must precede their children); a refused call raises PPError with ``bad_query``
        and changes nothing."""
        _forest_import(self.ctx, "b", state, queries)

    def reset_queries(self, queries, starts, seeds, goals):
        """Recycle slots: new queries (start pose, seed, goal) in ``queries``, as ``pp_batch_new``
        would have set them up, while every other query keeps its tree and its progress."""
        _forest_import(self.ctx, "b", _forest_roots("b", starts, seeds, goals), queries)

    def close(self):
        self.ctx.close()


class RRTStarBatch:
    """Independent k-nearest RRT* planners on one scene (BASELINE config 5), one RRT* iteration
    of every query per lockstep step on one GPU.  Build-defined — the reference has no RRT*
    (SURVEY.md §8f row 4): the crate's rand_point / exact NN / Node::new / verify_node / Dubins
    steer (rrt.rs:139-175, 378-426; dubins.rs:401-428) around Karaman & Frazzoli's choose-parent
    and rewire, edge cost = the crate's Dubins cost (dubins.rs:351-361).  ``k``: neighbours per
    insert (0 = ceil(2e ln n), at most 63); ``eta``: Steer distance (0 = the node sits at the
    sample, like the crate).  DESIGN.md §3.7; oracle: oracle/pp_oracle.c orc_star_extend."""

    def __init__(self, starts, max_iter, step_size, space: Space, seeds, k: int = 0,
                 eta: float = 0.0, device: int = 0, ctx: _ffi.Context | None = None):
        self.ctx = ctx or _ffi.Context(device)
        self.space = space
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        self.q = len(starts)
        self.max_iter = int(max_iter)
        self.n_checked = 0  # (query, node) pairs of the last plan()
        space._upload(self.ctx)
        _ffi.check(_ffi.lib().pp_star_new(
            self.ctx.handle, self.q, starts.ctypes.data_as(C.POINTER(C.c_double)),
            seeds.ctypes.data_as(C.POINTER(C.c_uint64)), self.max_iter, float(step_size), int(k),
            float(eta)))

    def extend(self, n_steps: int):
        """n_steps lockstep steps; returns (iterations, nodes inserted, rewires) over the batch."""
        it, acc, rw = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _ffi.check(_ffi.lib().pp_star_extend(self.ctx.handle, int(n_steps), C.byref(it),
                                             C.byref(acc), C.byref(rw)))
        return it.value, acc.value, rw.value

    def state(self):
        """(tree sizes int32[q], iterations, NN node-distance evals, rewires: int64[q] each)"""
        n = np.zeros(self.q, dtype=np.int32)
        it, ev, rw = (np.zeros(self.q, dtype=np.int64) for _ in range(3))
        i64 = C.POINTER(C.c_int64)
        _ffi.check(_ffi.lib().pp_star_state(self.ctx.handle, n.ctypes.data_as(C.POINTER(C.c_int32)),
                                            it.ctypes.data_as(i64), ev.ctypes.data_as(i64),
                                            rw.ctypes.data_as(i64)))
        return n, it, ev, rw

    def set_profiling(self, on: bool):
        _ffi.check(_ffi.lib().pp_set_profiling(self.ctx.handle, int(bool(on))))

    def stats(self) -> dict:
        s = _ffi.StatsC()
        _ffi.check(_ffi.lib().pp_rrt_get_stats(self.ctx.handle, C.byref(s), C.sizeof(s)))
        return s.as_dict()

    def tree(self, query: int, n: int | None = None):
        """(x, y, yaw, parent, cost) of one query's tree, root first (``n``: its size, when
        known)."""
        n = int(self.state()[0][query]) if n is None else int(n)
        x, y, yaw, cost = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        par = np.zeros(n, dtype=np.int32)
        out = C.c_int64(0)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        _ffi.check(_ffi.lib().pp_star_tree_export(
            self.ctx.handle, int(query), x.ctypes.data_as(dp), y.ctypes.data_as(dp),
            yaw.ctypes.data_as(dp), par.ctypes.data_as(ip), cost.ctypes.data_as(dp), n,
            C.byref(out)))
        return x, y, yaw, par, cost

    def revalidate(self, n_old=None):
        """Re-verify every query's tree against the context's current scene (pp_star_revalidate)
        and drop the nodes whose chain of stored edges to the root no longer holds: RRT*'s
        feasible edge per node, chains in any index order (a rewired node's parent is a later
        node).  Kept nodes keep their order, pose and cost; parents are remapped.  Returns
        (n_nodes int32[q] after the call, new_index int32[sum of the old sizes]): query q's
        entries start at the prefix sum of the old sizes, each a node's index in its tree
        afterwards or -1.  ``n_old``: the old sizes, when already known.  ``last_dropped``: the
        nodes dropped over the batch."""
        n, new_index, (self.last_dropped,) = _compact_trees(
            self.ctx, self.q, self.state()[0] if n_old is None else n_old,
            _ffi.lib().pp_star_revalidate, (), 1)
        return n, new_index

    def repair(self, rounds: int = 1, n_old=None):
        """``revalidate`` with up to ``rounds`` (0..16) re-attachment rounds (pp_star_repair): a
        dropped node whose own edge failed looks for a new parent among the star_k nearest kept
        nodes of its tree (the edge keeps its pose, like a rewire; the first strict minimum of
        cost[parent] + edge cost), and the subtree under it is kept again with its costs
        recomputed; later rounds give the children of a top that found no parent their own try.
        ``rounds = 0`` is ``revalidate``.  Returns (n_nodes, new_index) as ``revalidate`` does and
        sets ``last_dropped``, ``last_reattached`` (tops that found a parent) and
        ``last_recovered`` (nodes kept that ``revalidate`` would have dropped)."""
        n, new_index, (self.last_dropped, self.last_reattached, self.last_recovered) = \
            _compact_trees(self.ctx, self.q, self.state()[0] if n_old is None else n_old,
                           _ffi.lib().pp_star_repair, (int(rounds),), 3)
        return n, new_index

    def advance(self, nodes, hops=None, rounds: int = 0, n_old=None):
        """Move every query's root along its tree (pp_star_advance): the vehicle has driven, and
        the tree follows it.  ``nodes``: one node per query, -1 to leave a query alone.  ``hops``
        (None, a scalar for all, or one per query): the new root is the node that many edges from
        the root on the chain root -> ``nodes[q]`` (clamped to the chain); None: ``nodes[q]``
        itself.  ``advance(best_node, hops=1)`` follows a plan by one edge.  The subtree under the
        new root is kept with its costs rebuilt from it; the rest hung from the new root's
        ancestors, whose edges point the wrong way: with ``rounds`` (0..16) > 0 those ancestors
        are the first tops of ``repair``'s rounds, which hang back what still finds a feasible
        edge.  The new root gets index 0, the other kept nodes follow in their old order.
        Counters, seeds and the focus stay (the old bound stays admissible; ``plan(goals,
        focus=True)`` tightens it).  Returns (n_nodes, new_index) as ``revalidate`` does and sets
        ``last_dropped``, ``last_reattached`` and ``last_recovered``."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(self.q)
        if hops is not None:
            hops = np.ascontiguousarray(np.broadcast_to(np.asarray(hops, dtype=np.int32),
                                                        (self.q,)))
        lead = (nodes.ctypes.data_as(_I32P), None if hops is None else hops.ctypes.data_as(_I32P),
                int(rounds))
        n, new_index, (self.last_dropped, self.last_reattached, self.last_recovered) = \
            _compact_trees(self.ctx, self.q, self.state()[0] if n_old is None else n_old,
                           _ffi.lib().pp_star_advance, lead, 3)
        return n, new_index

    def relax(self, rounds: int = 1, active=None):
        """Let every node of every tree look for a cheaper parent among the nodes of its own tree
        (pp_star_relax): up to ``rounds`` (1..16) synchronous choose-parent rounds, on the device
        and in place.  A node's candidates are its star_k nearest other nodes; the edge keeps the
        node's pose, like a rewire; the first strict minimum of cost[parent] + edge cost wins when
        it is strictly below the node's cost; after every node has chosen, the costs are rebuilt
        from the root.  A round that re-parents nothing ends the call.  ``active`` (None: all):
        one flag per query, 0 leaves the query untouched.  Poses, node order, sizes and every
        counter but ``rewires`` stay; no cost rises, so a focus bound stays admissible.  The call
        is what follows ``advance``: the trees that survived hang by detours until their nodes
        have looked around.  Returns n_rewired int32[q] and sets ``last_rounds`` (the rounds run)
        and ``last_changed`` (the nodes whose cost changed)."""
        act = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active).reshape(self.q) != 0, dtype=np.uint8)
        nrw = np.zeros(self.q, dtype=np.int32)
        run, changed = C.c_int32(0), C.c_int64(0)
        _ffi.check(_ffi.lib().pp_star_relax(
            self.ctx.handle, int(rounds),
            None if act is None else act.ctypes.data_as(C.POINTER(C.c_uint8)),
            nrw.ctypes.data_as(_I32P), C.byref(run), C.byref(changed)))
        self.last_rounds = run.value
        self.last_changed = changed.value
        return nrw

    def relax_counts(self) -> dict:
        """The last ``relax`` call's profiling counters (pp_star_relax_counts; all but ``nodes``,
        ``slices`` and ``kmax`` are zero unless ``set_profiling(True)``)."""
        v = np.zeros(8, dtype=np.int64)
        _ffi.check(_ffi.lib().pp_star_relax_counts(self.ctx.handle,
                                                   v.ctypes.data_as(C.POINTER(C.c_int64))))
        keys = ("nodes", "candidates", "not_parent", "cheaper", "tasks", "walked", "slices", "kmax")
        return dict(zip(keys, (int(a) for a in v)))

    def set_space(self, space: Space, repair_rounds: int | None = None):
        """Replace the scene of the batch and keep every tree where it still holds: uploads
        ``space`` into the batch's context and revalidates — with ``repair_rounds`` given, by
        ``repair(repair_rounds)``.  (Uploading a scene alone does not stop the batch: its trees
        are unverified until ``revalidate``.)"""
        n_old = self.state()[0]
        space._upload(self.ctx)
        self.space = space
        if repair_rounds is None:
            return self.revalidate(n_old)
        return self.repair(repair_rounds, n_old)

    # ---- focused sampling (pp_star_set_focus / pp_star_get_focus)
    def focus(self, goals=None, cost=None):
        """Informed RRT*: from now on query q samples only where |s - root| + |s - goal| <
        ``cost[q] * turn_radius`` — the region that can still hold a node of a path cheaper than
        ``cost[q]`` (``plan``'s unit) — by rejecting draws of its own RNG stream, at most
        ``PP_STAR_FOCUS_DRAWS`` per iteration.  ``goals``: (q, 2) or (q, 3) rows, or one row for
        all (a yaw is ignored); a ``cost`` of inf leaves that query unfocused.  ``focus()`` clears
        every query's focus; the draws skipped so far stay skipped."""
        if goals is None and cost is None:
            _ffi.check(_ffi.lib().pp_star_set_focus(self.ctx.handle, None, None))
            return
        if goals is None or cost is None:
            raise ValueError("focus() takes both goals and cost, or neither")
        g = np.asarray(goals, dtype=np.float64)
        g = np.tile(g, (self.q, 1)) if g.ndim == 1 else g
        fxy = np.ascontiguousarray(g.reshape(self.q, -1)[:, :2])
        cost = np.broadcast_to(np.asarray(cost, dtype=np.float64), (self.q,))
        bound = np.ascontiguousarray(cost * np.float64(self.space.get_steer()))
        dp = C.POINTER(C.c_double)
        _ffi.check(_ffi.lib().pp_star_set_focus(self.ctx.handle, fxy.ctypes.data_as(dp),
                                                bound.ctypes.data_as(dp)))

    def focus_state(self):
        """(fxy float64[q, 2], bound float64[q] in length units (inf: no focus), skipped int64[q]:
        the draws each query's filter has rejected so far)"""
        fxy, bound = np.zeros((self.q, 2)), np.zeros(self.q)
        skipped = np.zeros(self.q, dtype=np.int64)
        dp = C.POINTER(C.c_double)
        _ffi.check(_ffi.lib().pp_star_get_focus(
            self.ctx.handle, fxy.ctypes.data_as(dp), bound.ctypes.data_as(dp),
            skipped.ctypes.data_as(C.POINTER(C.c_int64))))
        return fxy, bound, skipped

    def prune(self, keep=None, n_old=None):
        """Informed RRT*'s other half (pp_star_prune): drop from every query's tree the nodes
        that, at their stored cost, cannot lie on a path to the query's focus within its bound —
        node i > 0 fails iff ``cost[i] * turn_radius + |node - focus| > bound`` (``focus_state``'s
        values; strict) — and their descendants.  ``keep``: one node per query (-1: none), e.g.
        ``plan``'s best nodes: the chain from it to the root stays whatever the test says.  An
        unfocused query keeps every node.  Kept nodes keep their order, pose and cost; parents
        are remapped; the focus, counters and seeds stay.  Returns (n_nodes, new_index) as
        ``revalidate`` does and sets ``last_dropped``.  A node pruned now could have been made
        cheaper by a later rewire: the usual branch-and-bound trade."""
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.int32).reshape(self.q)
        n, new_index, (self.last_dropped,) = _compact_trees(
            self.ctx, self.q, self.state()[0] if n_old is None else n_old, _ffi.lib().pp_star_prune,
            (None if keep is None else keep.ctypes.data_as(_I32P),), 1)
        return n, new_index

    # ---- goal connection (pp_star_plan / pp_star_goal_costs / pp_star_path)
    def plan(self, goals, focus: bool = False, prune: bool = False, commit=None):
        """The cheapest feasible goal edge of every query on its tree as extended so far: goal
        (gx, gy, gyaw) per query (one pose is broadcast to all).  Returns (best_node int32[q],
        cost float64[q]): -1 and inf where no node reaches the goal.  ``n_checked``: the
        (query, node) pairs considered.  ``focus``: then ``focus(goals, cost)`` on the result.
        ``prune`` (needs ``focus``): then ``prune(keep=best_node)``; the best nodes returned are
        their indices in the pruned trees.  ``commit`` (a span, 1..63): after the plan,
        ``shortcut_commit(goals, best_node, commit)``; the node and cost returned are the
        commit's, and ``focus`` / ``prune`` use them."""
        if prune and not focus:
            raise ValueError("plan(prune=True) needs focus=True: the prune reads the focus")
        if commit is not None:
            node, cost = self.plan(goals)
            node, cost, _ = self.shortcut_commit(goals, node, int(commit))
            if focus:
                self.focus(goals, cost)
            if prune:
                node = self._prune_keep(node)
            return node, cost
        if focus:
            node, cost = self.plan(goals)
            self.focus(goals, cost)
            if prune:
                node = self._prune_keep(node)
            return node, cost
        g = np.asarray(goals, dtype=np.float64)
        g = np.tile(g, (self.q, 1)) if g.ndim == 1 else g
        g = np.ascontiguousarray(g, dtype=np.float64).reshape(self.q, 3)
        node = np.zeros(self.q, dtype=np.int32)
        cost = np.zeros(self.q)
        chk = C.c_int64(0)
        dp = C.POINTER(C.c_double)
        _ffi.check(_ffi.lib().pp_star_plan(
            self.ctx.handle, g.ctypes.data_as(dp), node.ctypes.data_as(C.POINTER(C.c_int32)),
            cost.ctypes.data_as(dp), C.byref(chk)))
        self.n_checked = chk.value
        return node, cost

    def _prune_keep(self, node):
        """``prune(keep=node)``; the nodes' indices in the pruned trees"""
        n_old = self.state()[0]
        _, new_index = self.prune(keep=node, n_old=n_old)
        off = np.concatenate(([0], np.cumsum(n_old[:-1], dtype=np.int64)))
        has = node >= 0
        node = node.copy()
        node[has] = new_index[off[has] + node[has]]
        return node

    def goal_costs(self, query: int, goal):
        """total[m] = cost[m] + the goal edge's Dubins cost of every node of one query (inf where
        the edge is infeasible), without pruning."""
        g = np.ascontiguousarray(goal, dtype=np.float64).reshape(3)
        out = C.c_int64(0)
        dp = C.POINTER(C.c_double)
        L = _ffi.lib()
        _ffi.check(L.pp_star_goal_costs(self.ctx.handle, int(query), g.ctypes.data_as(dp), None, 0,
                                        C.byref(out)))  # (the tree's size)
        total = np.zeros(out.value)
        _ffi.check(L.pp_star_goal_costs(self.ctx.handle, int(query), g.ctypes.data_as(dp),
                                        total.ctypes.data_as(dp), out.value, C.byref(out)))
        return total

    def path(self, query: int, goal, node: int):
        """(xy[n, 2], length): the path root -> ... -> node -> goal along the tree's stored poses
        (``node``: one whose goal edge is feasible, e.g. plan()'s best node)."""
        g = np.ascontiguousarray(goal, dtype=np.float64).reshape(3)
        dp = C.POINTER(C.c_double)
        n, length = C.c_int64(0), C.c_double(0.0)
        L = _ffi.lib()
        _ffi.check(L.pp_star_path(self.ctx.handle, int(query), g.ctypes.data_as(dp), int(node),
                                  None, None, 0, C.byref(n), None))
        x, y = np.zeros(n.value), np.zeros(n.value)
        _ffi.check(L.pp_star_path(self.ctx.handle, int(query), g.ctypes.data_as(dp), int(node),
                                  x.ctypes.data_as(dp), y.ctypes.data_as(dp), n.value, C.byref(n),
                                  C.byref(length)))
        return np.stack([x, y], axis=1), length.value

    def paths(self, goals, nodes=None):
        """``path(q, goals[q], nodes[q])`` of every query in one call (pp_star_paths), generated
        on the device.  ``goals``: a pose per query (one pose is broadcast); ``nodes``: one node
        per query (-1: skip), or None: ``plan(goals)``'s best nodes.  The goal edge is not
        verified again: any node's line is returned.  Returns (off int64[q + 1], xy
        float64[n, 2], length float64[q], ok bool[q]): row q = ``xy[off[q]:off[q + 1]]``, root
        first; empty with ``ok[q]`` False and length 0 where the node is -1 or its goal edge has
        no Dubins word."""
        g = np.asarray(goals, dtype=np.float64)
        g = np.tile(g, (self.q, 1)) if g.ndim == 1 else g
        g = np.ascontiguousarray(g, dtype=np.float64).reshape(self.q, 3)
        if nodes is None:
            nodes = self.plan(g)[0]
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(self.q)
        L = _ffi.lib()
        ip, dp, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        u8 = C.POINTER(C.c_uint8)
        off = np.zeros(self.q + 1, dtype=np.int64)
        ok = np.zeros(self.q, dtype=np.uint8)
        length = np.zeros(self.q)
        tot = C.c_int64(0)
        _ffi.check(L.pp_star_paths(self.ctx.handle, g.ctypes.data_as(dp), nodes.ctypes.data_as(ip),
                                   off.ctypes.data_as(i64), None, None, 0, C.byref(tot), None,
                                   ok.ctypes.data_as(u8)))
        cap = tot.value
        x, y = np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
        if cap > 0:
            _ffi.check(L.pp_star_paths(self.ctx.handle, g.ctypes.data_as(dp),
                                       nodes.ctypes.data_as(ip), off.ctypes.data_as(i64),
                                       x.ctypes.data_as(dp), y.ctypes.data_as(dp), cap,
                                       C.byref(tot), length.ctypes.data_as(dp),
                                       ok.ctypes.data_as(u8)))
        return off, np.stack([x[:cap], y[:cap]], axis=1), length, ok.astype(bool)

    def path_segments(self, goals, nodes=None, reverse=False):
        """The rows of ``paths(goals, nodes)`` as Dubins segments (pp_star_path_segments): every
        edge of the chain goal -> node -> parent -> ... -> root as three arc / straight / arc
        records, generated on the device.  Returns (off int64[q + 1], seg, length float64[q],
        ok bool[q]): ``seg`` a dict of float64 arrays ``x``, ``y``, ``yaw`` (the segment's start
        pose, yaw unwrapped), ``kappa`` (signed curvature, +-1 / turn radius or 0) and ``len``;
        row q = entries ``off[q]:off[q + 1]``, three per edge, in generation order (goal edge
        first, headings as stored: toward the root) or, ``reverse``, the same curve from the root
        to the goal (``paths``' order).  ``length[q]``: the sum of the row's ``len``;
        ``length / turn_radius`` is ``plan``'s cost for its best node.  ``goals``, ``nodes``,
        ``ok`` and the empty rows as in ``paths``."""
        g = np.asarray(goals, dtype=np.float64)
        g = np.tile(g, (self.q, 1)) if g.ndim == 1 else g
        g = np.ascontiguousarray(g, dtype=np.float64).reshape(self.q, 3)
        if nodes is None:
            nodes = self.plan(g)[0]
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(self.q)
        L, h = _ffi.lib(), self.ctx.handle
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        return _path_segments(self.q, lambda *a: L.pp_star_path_segments(
            h, g.ctypes.data_as(dp), nodes.ctypes.data_as(ip), int(bool(reverse)), *a))

    def trajectories(self, goals, ds, nodes=None, reverse=True):
        """``path_segments(goals, nodes, reverse)`` sampled every ``ds`` (``sample_segments``):
        (poff, x, y, yaw, kappa, s), root to goal by default."""
        off, seg, _, _ = self.path_segments(goals, nodes, reverse)
        return sample_segments(self.ctx, off, seg, ds)

    # ---- shortcuts along the chain (pp_star_shortcut / _edges / pp_star_chain_segments, §3.7)
    def _goals(self, goals):
        g = np.asarray(goals, dtype=np.float64)
        g = np.tile(g, (self.q, 1)) if g.ndim == 1 else g
        return np.ascontiguousarray(g, dtype=np.float64).reshape(self.q, 3)

    def shortcut(self, goals, nodes=None, span=8):
        """Shorten every query's path goal -> node -> parent -> ... -> root by Dubins shortcuts
        between the poses of its own chain (pp_star_shortcut): from each position an edge may skip
        to any of the next ``span`` (1..63) positions when RRT*'s feasible edge between the two
        stored poses verifies in the context's current scene, and a DP over the chain picks the
        cheapest such route.  ``goals``, ``nodes`` as in ``paths`` (None: ``plan(goals)``'s best
        nodes).  Returns (off int64[q + 1], chain int32[n], cost float64[q], ok bool[q]): row q =
        ``chain[off[q]:off[q + 1]]``, the tree nodes after the goal, the root (0) last; empty
        with cost inf and ``ok[q]`` False where the node is -1 or no route exists within the span.
        ``n_tested``: the pairs considered.  ``span=1`` re-verifies the tree chain itself."""
        g = self._goals(goals)
        if nodes is None:
            nodes = self.plan(g)[0]
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(self.q)
        L = _ffi.lib()
        ip, dp, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        u8 = C.POINTER(C.c_uint8)
        off = np.zeros(self.q + 1, dtype=np.int64)
        ok = np.zeros(self.q, dtype=np.uint8)
        cost = np.zeros(self.q)
        tot, tested = C.c_int64(0), C.c_int64(0)
        # one call instead of sizes-then-fill (which would steer everything twice): a row is no
        # longer than its tree, so the trees' total always suffices
        cap = int(np.sum(self.state()[0], dtype=np.int64))
        chain = np.zeros(max(cap, 1), dtype=np.int32)
        _ffi.check(L.pp_star_shortcut(
            self.ctx.handle, g.ctypes.data_as(dp), nodes.ctypes.data_as(ip), int(span),
            off.ctypes.data_as(i64), chain.ctypes.data_as(ip), max(cap, 1), C.byref(tot),
            cost.ctypes.data_as(dp), ok.ctypes.data_as(u8), C.byref(tested)))
        self.n_tested = tested.value
        return off, chain[:tot.value].copy(), cost, ok.astype(bool)

    def shortcut_commit(self, goals, nodes=None, span=8):
        """Write ``shortcut``'s improvements back into the trees (pp_star_shortcut_commit): along
        every query's chain goal -> node -> parent -> ... -> root, from the root's end, a chain
        node is re-parented onto the ancestor at most ``span`` (1..63) positions up the chain whose
        feasible edge gives it a strictly cheaper cost than its stored edge does (RRT*'s rewire
        test); the costs of everything below are recomputed, so ``plan``, ``paths``,
        ``path_segments``, ``focus``, ``prune`` and ``extend`` see the shorter route.  Poses, node
        order and tree sizes stay; no cost rises.  ``goals``, ``nodes`` as in ``shortcut``.
        Returns (node int32[q], cost float64[q], n_rewired int32[q]): the chain node the goal
        connects to most cheaply within the span and that cost (-1, inf and 0 where the node is -1
        or no goal edge is feasible).  ``n_tested``: the pairs considered; ``n_changed``: the
        nodes whose cost changed."""
        g = self._goals(goals)
        if nodes is None:
            nodes = self.plan(g)[0]
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(self.q)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        node = np.zeros(self.q, dtype=np.int32)
        cost = np.zeros(self.q)
        nrw = np.zeros(self.q, dtype=np.int32)
        tested, changed = C.c_int64(0), C.c_int64(0)
        _ffi.check(_ffi.lib().pp_star_shortcut_commit(
            self.ctx.handle, g.ctypes.data_as(dp), nodes.ctypes.data_as(ip), int(span),
            node.ctypes.data_as(ip), cost.ctypes.data_as(dp), nrw.ctypes.data_as(ip),
            C.byref(tested), C.byref(changed)))
        self.n_tested = tested.value
        self.n_changed = changed.value
        return node, cost, nrw

    def shortcut_edges(self, query: int, goal, node: int, span: int):
        """The band ``shortcut`` runs its DP over, for one query, un-culled (pp_star_shortcut_edges):
        (cnode int32[D], w float64[D, span]) — ``cnode[i - 1]`` the tree node of chain position i
        (position 0 is the goal), ``w[i, j - i - 1]`` the Dubins cost of the feasible edge from
        position i to position j, inf where infeasible or j > D."""
        g = np.ascontiguousarray(goal, dtype=np.float64).reshape(3)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        L = _ffi.lib()
        d = C.c_int64(0)
        _ffi.check(L.pp_star_shortcut_edges(self.ctx.handle, int(query), g.ctypes.data_as(dp),
                                            int(node), int(span), None, None, 0, C.byref(d)))
        D = d.value
        w = np.zeros((D, int(span)))
        cnode = np.zeros(D, dtype=np.int32)
        _ffi.check(L.pp_star_shortcut_edges(self.ctx.handle, int(query), g.ctypes.data_as(dp),
                                            int(node), int(span), w.ctypes.data_as(dp),
                                            cnode.ctypes.data_as(ip), D, C.byref(d)))
        return cnode, w

    def chain_segments(self, goals, off, chain, reverse=False):
        """``path_segments`` over caller-supplied chains (pp_star_chain_segments): row q = the
        edges goal -> chain[off[q]] -> ... -> chain[off[q + 1] - 1] (``shortcut``'s rows, or any
        chain of tree nodes ending in the root), nothing verified again.  Returns what
        ``path_segments`` returns; an empty chain row gives an empty row with ``ok`` False."""
        g = self._goals(goals)
        coff = np.ascontiguousarray(off, dtype=np.int64).reshape(self.q + 1)
        chain = np.ascontiguousarray(chain, dtype=np.int32)
        L, h = _ffi.lib(), self.ctx.handle
        ip, dp, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        return _path_segments(self.q, lambda *a: L.pp_star_chain_segments(
            h, g.ctypes.data_as(dp), coff.ctypes.data_as(i64), chain.ctypes.data_as(ip),
            int(bool(reverse)), *a))

    def shortcut_trajectories(self, goals, ds, nodes=None, span=8, reverse=True):
        """``shortcut(goals, nodes, span)``'s rows as segments (``chain_segments``) sampled every
        ``ds`` (``sample_segments``): (poff, x, y, yaw, kappa, s), root to goal by default."""
        coff, chain, _, _ = self.shortcut(goals, nodes, span)
        off, seg, _, _ = self.chain_segments(goals, coff, chain, reverse)
        return sample_segments(self.ctx, off, seg, ds)

    # ---- forest export / import (pp_star_forest_export / _import)
    def export_forest(self, queries=None):
        """The complete state of the slots ``queries`` (distinct, any order; None: all) in one
        call, packed on the device: a dict of numpy arrays — ``off`` int64[m + 1] (slot i's tree
        is rows off[i]:off[i + 1]), rows ``x``, ``y``, ``yaw``, ``parent``, ``cost``,
        ``edge_cost``, per slot ``iterations``, ``seeds``, ``node_evals``, ``rewires``,
        ``focus_xy`` [m, 2], ``focus_bound`` (inf: no focus), ``skipped``.
        ``np.savez(path, **state)`` is a checkpoint.  The batch is not modified."""
        return _forest_export(self.ctx, "s", self.q, queries)

    def import_forest(self, state, queries=None):
        """Write such a state into the slots ``queries`` (None: 0 .. m - 1) of this batch — of any
        size, on the same scene, step size, max_iter, k and eta; the other slots stay untouched.
        Under further extend / plan / focus / prune calls the slots evolve exactly as the exported
        ones would have, bit for bit.  Validated as a whole first: every chain must end in its
        root, and ``cost`` (may be absent or None: rebuilt) must equal cost[parent] + edge_cost
        bit for bit.  A refused call raises PPError with ``bad_query`` and changes nothing.  The
        edges are trusted: ``revalidate`` after importing trees grown in another scene."""
        _forest_import(self.ctx, "s", state, queries)

    def reset_queries(self, queries, starts, seeds):
        """Recycle slots: new queries (start pose with its yaw, seed) in ``queries``, as
        ``pp_star_new`` would have set them up — a root, no iterations, evaluations, rewires or
        skipped draws, no focus — while every other query keeps its tree and its progress."""
        _forest_import(self.ctx, "s", _forest_roots("s", starts, seeds), queries)

    def close(self):
        self.ctx.close()

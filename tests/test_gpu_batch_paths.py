"""GPU: the batched path export of the extend batch (pp_batch_paths, RRTBatch.paths; DESIGN.md
§3.3 "Packed line export") — every query's finalized line in one packed call.

References: the oracle's check_finish line on the oracle's tree of the query (count exact,
coordinates within 1e-9 absolute — TOL of tests/test_gpu_api_surface.py — and the row's
oracle.line_length within 1e-9 relative of the plan's length), and the one-tree device path
(pp_batch_tree_export -> pp_rrt_new + pp_rrt_tree_import -> pp_rrt_check_finish), which runs the
same device code and must agree bit for bit.  The libm trim flips of DESIGN.md §2 (a query whose
line differs from the oracle's by exactly one point) are counted, not compared point by point:
at most 2 on the bench6_open recipe, tests/test_gpu_batch_plan.py's own bound for it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx1(pkg):
    """the one-tree planner's context"""
    c = pkg.Context(0)
    yield c
    c.close()


def _batch(ctx, raw, nq, max_iter, starts=None):
    from pathplanning_amd import rrt, scenes

    st, goals, seeds = scenes.config3_queries(raw, 0, nq)
    st = st if starts is None else starts
    b = rrt.RRTBatch(st, goals, max_iter, raw["step_size"], rrt.Space.from_raw(raw), seeds, ctx=ctx)
    return b, np.asarray(st, dtype=np.float64).reshape(-1, 3), np.asarray(goals).reshape(-1, 3), seeds


def _one_tree(ctx1, raw, b, q, starts, goals):
    """query q's tree in a one-tree planner with the query's start, goal and step"""
    from pathplanning_amd import rrt

    t = rrt.RRT(starts[q][:2], starts[q][2], goals[q][:2], goals[q][2], b.max_iter,
                raw["step_size"], rrt.Space.from_raw(raw), seed=0, ctx=ctx1)
    t.tree_import(*b.tree(q))
    return t


def _rows(off, xy):
    return [xy[off[q]:off[q + 1]] for q in range(len(off) - 1)]


def _oracle_tree(oracle_mod, raw, start, seed, n_iter):
    sc = oracle_mod.OracleScene.from_raw(raw)
    tr = oracle_mod.OracleTree(tuple(start), n_iter + 1)
    oracle_mod.rrt_extend(sc, tr, int(seed), 0, n_iter)
    return sc, tr


def _check_oracle(oracle_mod, raw, starts, goals, seeds, n_iter, plan, rows, ok, max_flips):
    """every finishing query's row against the oracle's check_finish of the plan's best node on
    the oracle's tree; returns (finishing queries, one-point flips).  max_flips: 2 for the
    bench6_open recipe (tests/test_gpu_batch_plan.py's bound, 1 measured); None: that file's rule
    for a recipe without a measurement, max(1, a tenth of the finishing queries)"""
    fin = flips = 0
    for q, row in enumerate(rows):
        bn = int(plan["best_node"][q])
        assert len(row) == plan["n_points"][q], q
        assert (len(row) == 0) == (bn < 0), q
        assert bool(ok[q]) == (bn >= 0), q
        if bn < 0:
            continue
        fin += 1
        sc, tr = _oracle_tree(oracle_mod, raw, starts[q], seeds[q], n_iter)
        exp = oracle_mod.check_finish(sc, tr, bn, goals[q][:2], goals[q][2])
        assert exp["ok"], q
        ln = oracle_mod.line_length(row[:, 0], row[:, 1])
        assert abs(ln - plan["length"][q]) <= 1e-9 * plan["length"][q], q
        if len(row) != exp["n"]:
            assert abs(len(row) - exp["n"]) == 1, (q, len(row), exp["n"])  # a libm trim flip
            flips += 1
            continue
        assert np.max(np.abs(row[:, 0] - exp["x"])) <= TOL, q
        assert np.max(np.abs(row[:, 1] - exp["y"])) <= TOL, q
    print(f"paths: {fin} finishing queries, {flips} one-point libm trim flips")
    assert flips <= (max_flips if max_flips is not None else max(1, fin // 10))
    return fin, flips


@pytest.fixture(scope="module")
def open64(pkg):
    """bench6_open, 64 queries x 300 iterations (test_batch_plan_bench6_open's recipe): the
    batch (on a context of its own: a context holds one batch), its plan and the plan's packed
    lines, computed once for the tests that share them"""
    from pathplanning_amd import scenes

    c = pkg.Context(0)
    raw = scenes.bench6_open()
    b, starts, goals, seeds = _batch(c, raw, 64, 300)
    b.extend(300)
    off, xy, ok = b.paths()
    plan = b.last_plan
    yield {"raw": raw, "b": b, "starts": starts, "goals": goals, "seeds": seeds, "plan": plan,
           "off": off, "xy": xy, "ok": ok}
    c.close()


def test_paths_oracle_parity(open64, oracle_mod):
    d = open64
    assert d["off"][0] == 0 and d["off"][-1] == len(d["xy"]) == int(d["plan"]["n_points"].sum())
    fin, _ = _check_oracle(oracle_mod, d["raw"], d["starts"], d["goals"], d["seeds"], 300,
                           d["plan"], _rows(d["off"], d["xy"]), d["ok"], 2)
    assert fin >= 16


def test_paths_equal_one_tree_bit_for_bit(open64, ctx1):
    d = open64
    rows = _rows(d["off"], d["xy"])
    qs = [int(q) for q in np.flatnonzero(d["plan"]["best_node"] >= 0)[:4]]
    assert len(qs) == 4
    for q in qs:
        t = _one_tree(ctx1, d["raw"], d["b"], q, d["starts"], d["goals"])
        line = t.check_finish(int(d["plan"]["best_node"][q]))
        assert line is not None and np.array_equal(line, rows[q]), q


def test_paths_arbitrary_nodes(open64, ctx1):
    """-1, node 0, a node whose check_finish is None, non-best finishing nodes and a best node
    in one call: ok, the counts and the rows equal the one-tree planner's on the imported tree"""
    d = open64
    b, plan = d["b"], d["plan"]
    qs = [int(q) for q in np.flatnonzero(plan["best_node"] >= 0)[:5]]
    nodes = np.full(64, -1, dtype=np.int32)
    exp = {}
    kinds = set()
    for i, q in enumerate(qs):
        t = _one_tree(ctx1, d["raw"], b, q, d["starts"], d["goals"])
        n = t.tree_size()
        cf = t.check_finish_batch(np.arange(n, dtype=np.int32))
        best = int(plan["best_node"][q])
        none = [m for m in range(1, n) if not cf["ok"][m]]
        other = [m for m in range(1, n) if cf["ok"][m] and m != best]
        pick = [0, none[0] if none else 0, other[0] if other else best,
                other[-1] if other else best, best][i]
        kinds.add("root" if pick == 0 else "none" if pick in none else
                  "best" if pick == best else "other")
        nodes[q] = pick
        line = t.check_finish(pick)
        exp[q] = (bool(cf["ok"][pick]), int(cf["n_points"][pick]) if cf["ok"][pick] else 0, line)
    assert kinds == {"root", "none", "other", "best"}
    off, xy, ok = b.paths(nodes)
    rows = _rows(off, xy)
    for q in range(64):
        if q not in exp:
            assert len(rows[q]) == 0 and not ok[q]
            continue
        eok, en, line = exp[q]
        assert bool(ok[q]) == eok and len(rows[q]) == en, (q, nodes[q])
        if eok:
            assert np.array_equal(rows[q], line), q


def test_paths_tier2(pkg, ctx, oracle_mod):
    """lines past the line kernels' tier-1 capacity (6144 points; step 0.003 on the config-3
    field): 4 queries x 2000 iterations.  The oracle's tree is rrt_extend's (what oracle.plan
    extends; its check_finish of every node takes 15 s at this step and is
    test_batch_plan_long_lines_tier2's business), the line oracle.check_finish of the best node"""
    from pathplanning_amd import scenes

    raw = dict(scenes.field512())
    raw["step_size"] = 0.003
    b, starts, goals, seeds = _batch(ctx, raw, 4, 2000)
    b.extend(2000)
    off, xy, ok = b.paths()
    rows = _rows(off, xy)
    assert max(len(r) for r in rows) > 6144
    fin, _ = _check_oracle(oracle_mod, raw, starts, goals, seeds, 2000, b.last_plan, rows, ok, None)
    assert fin >= 1


def test_paths_shapes(pkg, ctx, ctx1):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    b, starts, goals, _ = _batch(ctx, raw, 5, 100)
    off, xy, ok = b.paths()  # roots only
    assert np.array_equal(off, np.zeros(6, dtype=np.int64)) and len(xy) == 0 and not ok.any()
    b.extend(100)
    n = b.state()[0]
    assert len(set(int(v) for v in n)) >= 4
    off, xy, ok = b.paths()
    rows = _rows(off, xy)
    assert ok.sum() >= 3
    for q in range(5):
        bn = int(b.last_plan["best_node"][q])
        if bn < 0:
            assert len(rows[q]) == 0
            continue
        line = _one_tree(ctx1, raw, b, q, starts, goals).check_finish(bn)
        assert np.array_equal(line, rows[q]), q


def test_paths_sub_batches(pkg, ctx, ctx1):
    """300 queries (the extend runs them as sub-batches): the offsets, and the rows of queries
    on both sides of the split against the one-tree planner — the plan's best nodes, then the
    last node of each of those queries"""
    from pathplanning_amd import scenes

    raw = scenes.field512()
    b, starts, goals, _ = _batch(ctx, raw, 300, 200)
    b.extend(200)
    off, xy, ok = b.paths()
    plan = b.last_plan
    assert np.all(np.diff(off) >= 0) and off[300] == int(plan["n_points"].sum()) == len(xy)
    assert np.array_equal(np.diff(off), plan["n_points"])
    rows = _rows(off, xy)
    edge = [0, 149, 150, 299]
    fin = [int(q) for q in np.flatnonzero(plan["best_node"] >= 0)]
    assert fin
    for q in sorted(set(edge + fin[:3])):
        bn = int(plan["best_node"][q])
        if bn < 0:
            assert len(rows[q]) == 0 and not ok[q]
            continue
        line = _one_tree(ctx1, raw, b, q, starts, goals).check_finish(bn)
        assert np.array_equal(line, rows[q]), q
    n = b.state()[0]
    nodes = np.full(300, -1, dtype=np.int32)
    for q in edge:
        nodes[q] = n[q] - 1
    off2, xy2, ok2 = b.paths(nodes)
    rows2 = _rows(off2, xy2)
    assert np.all(np.diff(off2) >= 0)
    for q in range(300):
        if q not in edge:
            assert len(rows2[q]) == 0 and not ok2[q]
            continue
        line = _one_tree(ctx1, raw, b, q, starts, goals).check_finish(int(nodes[q]))
        assert bool(ok2[q]) == (line is not None), q
        if line is None:
            assert len(rows2[q]) == 0
        else:
            assert np.array_equal(line, rows2[q]), q


def test_paths_protocol_and_errors(pkg, open64):
    from pathplanning_amd import _ffi, rrt, scenes

    d = open64
    b, plan = d["b"], d["plan"]
    L = _ffi.lib()
    ip, dp, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    u8 = C.POINTER(C.c_uint8)
    nodes = np.ascontiguousarray(plan["best_node"], dtype=np.int32)
    off = np.zeros(65, dtype=np.int64)
    ok = np.zeros(64, dtype=np.uint8)
    tot = C.c_int64(-1)
    h = b.ctx.handle
    # the sizes-only call
    assert L.pp_batch_paths(h, nodes.ctypes.data_as(ip), off.ctypes.data_as(i64), None, None, 0,
                            C.byref(tot), ok.ctypes.data_as(u8)) == _ffi.PP_OK
    assert tot.value == off[64] == d["off"][64] and np.array_equal(off, d["off"])
    assert np.array_equal(ok.astype(bool), d["ok"])
    # one point short: PP_ERR_CAPACITY with the sizes filled
    n = tot.value
    x, y = np.zeros(n), np.zeros(n)
    off[:] = 0
    tot = C.c_int64(-1)
    assert L.pp_batch_paths(h, nodes.ctypes.data_as(ip), off.ctypes.data_as(i64),
                            x.ctypes.data_as(dp), y.ctypes.data_as(dp), n - 1, C.byref(tot),
                            None) == _ffi.PP_ERR_CAPACITY
    assert tot.value == n and np.array_equal(off, d["off"])
    # the full call with ok NULL
    assert L.pp_batch_paths(h, nodes.ctypes.data_as(ip), off.ctypes.data_as(i64),
                            x.ctypes.data_as(dp), y.ctypes.data_as(dp), n, C.byref(tot),
                            None) == _ffi.PP_OK
    assert np.array_equal(np.stack([x, y], axis=1), d["xy"])
    # NULL arguments, a node outside its tree
    for args in ((None, off.ctypes.data_as(i64), C.byref(tot)),
                 (nodes.ctypes.data_as(ip), None, C.byref(tot)),
                 (nodes.ctypes.data_as(ip), off.ctypes.data_as(i64), None)):
        assert L.pp_batch_paths(h, args[0], args[1], None, None, 0, args[2],
                                None) == _ffi.PP_ERR_INVALID_ARGUMENT
    sizes = b.state()[0]
    for bad in (int(sizes[3]), -2):
        nb = nodes.copy()
        nb[3] = bad
        with pytest.raises(_ffi.PPError) as e:
            b.paths(nb)
        assert e.value.code == _ffi.PP_ERR_INVALID_ARGUMENT
    # no batch
    raw = d["raw"]
    c = pkg.Context(0)
    rrt.Space.from_raw(raw)._upload(c)
    assert L.pp_batch_paths(c.handle, nodes.ctypes.data_as(ip), off.ctypes.data_as(i64), None,
                            None, 0, C.byref(tot), None) == _ffi.PP_ERR_STATE
    # a NaN start yaw: every edge into that root is a None steer, finalize's panic
    starts, goals, seeds = scenes.config3_queries(raw, 0, 24)
    st = np.array(starts, dtype=np.float64).reshape(-1, 3)
    st[5, 2] = float("nan")
    bb = rrt.RRTBatch(st, goals, 300, raw["step_size"], rrt.Space.from_raw(raw), seeds, ctx=c)
    bb.extend(300)
    nn = bb.state()[0]
    assert int(nn[5]) > 2
    with pytest.raises(_ffi.PPError) as e:
        bb.paths(np.asarray(nn - 1, dtype=np.int32))
    assert e.value.code == _ffi.PP_ERR_REFERENCE_PANIC
    nb = np.asarray(nn - 1, dtype=np.int32)
    nb[5] = -1  # without the NaN query the same call is fine
    bb.paths(nb)
    c.close()


@pytest.mark.parametrize("scene,n_iter", [("field512_grid", 300), ("bench6_polygons_open", 300)])
def test_paths_scene_modes(pkg, ctx, oracle_mod, scene, n_iter):
    """the occupancy grid and the polygon obstacles (blocked roots included), 8 queries"""
    from pathplanning_amd import scenes

    raw = getattr(scenes, scene)()
    b, starts, goals, seeds = _batch(ctx, raw, 8, n_iter)
    b.extend(n_iter)
    off, xy, ok = b.paths()
    fin, _ = _check_oracle(oracle_mod, raw, starts, goals, seeds, n_iter, b.last_plan,
                           _rows(off, xy), ok, None)
    assert fin >= 1


def test_paths_do_not_disturb_extend(pkg, ctx):
    """extend 100, plan, paths, extend 100 == a second batch's straight 200"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    b, _, _, _ = _batch(ctx, raw, 5, 200)
    b.extend(100)
    b.paths()
    n = b.state()[0]
    b.paths(np.asarray(n - 1, dtype=np.int32))
    b.extend(100)
    got = [b.tree(q) for q in range(5)]
    b2, _, _, _ = _batch(ctx, raw, 5, 200)
    b2.extend(200)
    for q in range(5):
        exp = b2.tree(q)
        assert len(got[q][0]) > 1
        for a, e in zip(got[q], exp):
            assert np.array_equal(a, e), q

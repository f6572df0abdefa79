"""GPU: the packed forest export / import (pp_star_forest_export / _import, pp_batch_forest_export /
_import) against the oracle: exported slots imported into another batch continue
exactly as they would have, an export disturbs nothing, a recycled slot runs its new query while
the others keep theirs, and a bad state is refused whole, naming the slot.

Tolerances are tests/test_gpu_rrtstar.py's against the oracle (coordinates, parents, sizes and
rewires exact; yaw 1e-9, cost 1e-9 relative); GPU against GPU everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import forest_state_ref as ref
from test_gpu_rrtstar import _assert_same, _batch, _oracle

pytestmark = pytest.mark.gpu

STARTS = [(-4.0, -4.5, 0.3), (-3.0, -3.0, 0.785), (2.0, -4.0, 1.2), (-4.5, 2.0, -0.4),
          (0.5, -4.2, 2.0), (-2.0, -4.0, 0.1), (3.0, -3.5, 1.0)]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_b(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_state(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].shape == b[key].shape, key
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key


def _tree_of(st, i):
    """slot i of a state as a forest_state_ref tree dict"""
    g0, g1 = int(st["off"][i]), int(st["off"][i + 1])
    return ref.star_tree(st["x"][g0:g1], st["y"][g0:g1], st["yaw"][g0:g1], st["parent"][g0:g1],
                         st["edge_cost"][g0:g1], cost=st["cost"][g0:g1],
                         iterations=int(st["iterations"][i]), seed=int(st["seeds"][i]),
                         node_evals=int(st["node_evals"][i]), rewires=int(st["rewires"][i]),
                         focus_xy=st["focus_xy"][i], focus_bound=float(st["focus_bound"][i]),
                         skipped=int(st["skipped"][i]))


def _rows(st, i):
    g0, g1 = int(st["off"][i]), int(st["off"][i + 1])
    return tuple(st[k][g0:g1] for k in ("x", "y", "yaw", "parent", "cost"))


def test_round_trip_and_continuation(pkg, oracle_mod, ctx, ctx_b):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, seeds = [raw["start"]] + STARTS[:4], [5, 11, 12, 13, 14]
    a = _batch(pkg, raw, starts, seeds, 400, 0, 0.0, ctx=ctx)
    a.extend(150)
    st = a.export_forest()
    assert list(st["iterations"]) == [150] * 5 and st["off"][5] == len(st["x"])
    assert np.array_equal(st["off"][1:] - st["off"][:-1], a.state()[0])
    for i in range(5):  # the device's own arrays satisfy the identity the import rebuilds by
        x, y, yaw, par, cost = _rows(st, i)
        e = st["edge_cost"][st["off"][i]:st["off"][i + 1]]
        assert cost[0] == 0.0 and par[0] == -1
        assert np.array_equal(_bits(cost[1:]), _bits(cost[par[1:]] + e[1:]))
    bstarts, bseeds = STARTS[::-1], [31, 32, 33, 34, 35, 36, 37]
    b = _batch(pkg, raw, bstarts, bseeds, 400, 0, 0.0, ctx=ctx_b)
    slots = [6, 0, 3, 2, 5]
    b.import_forest(st, slots)
    _same_state(b.export_forest(slots), st)
    b.extend(250)
    n, it, _, rw = b.state()
    for i, s in enumerate(slots):
        exp, erw = _oracle(oracle_mod, raw, starts[i], seeds[i], 400, 0, 0.0)
        _assert_same(b.tree(s), exp)
        assert rw[s] == erw and it[s] == 400
    for s in (1, 4):
        exp, erw = _oracle(oracle_mod, raw, bstarts[s], bseeds[s], 250, 0, 0.0)
        _assert_same(b.tree(s), exp)
        assert rw[s] == erw and it[s] == 250


def test_export_disturbs_nothing(pkg, oracle_mod, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, seeds = [raw["start"], STARTS[0]], [5, 11]
    a = _batch(pkg, raw, starts, seeds, 400, 4, 2.0, ctx=ctx)
    a.extend(150)
    st = a.export_forest([1, 0])
    _same_state(a.export_forest([1, 0]), st)
    a.extend(250)
    rw = a.state()[3]
    for q in range(2):
        exp, erw = _oracle(oracle_mod, raw, starts[q], seeds[q], 400, 4, 2.0)
        _assert_same(a.tree(q), exp)
        assert rw[q] == erw


def test_recycle(pkg, oracle_mod, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, seeds = [raw["start"]] + STARTS[:4], [5, 11, 12, 13, 14]
    a = _batch(pkg, raw, starts, seeds, 200, 0, 0.0, ctx=ctx)
    # a focus so wide that it rejects no draw: the trees stay the unfocused oracle's
    a.focus(raw["goal"], 1.0e6)
    a.extend(100)
    before = a.export_forest([0, 2, 4])
    new_starts, new_seeds = [STARTS[5], STARTS[6]], [91, 92]
    a.reset_queries([1, 3], new_starts, new_seeds)
    _same_state(a.export_forest([0, 2, 4]), before)
    n, it, ev, rw = a.state()
    assert list(n[[1, 3]]) == [1, 1] and list(it) == [100, 0, 100, 0, 100]
    assert list(ev[[1, 3]]) == [0, 0] and list(rw[[1, 3]]) == [0, 0]
    fxy, bound, skipped = a.focus_state()
    assert np.isinf(bound[[1, 3]]).all() and np.isfinite(bound[[0, 2, 4]]).all()
    assert (fxy[[1, 3]] == 0.0).all() and (skipped == 0).all()
    a.extend(100)
    n, it, _, rw = a.state()
    assert list(it) == [200, 100, 200, 100, 200]
    for q in (0, 2, 4):
        exp, erw = _oracle(oracle_mod, raw, starts[q], seeds[q], 200, 0, 0.0)
        _assert_same(a.tree(q), exp)
        assert rw[q] == erw
    for q, s, sd in zip((1, 3), new_starts, new_seeds):
        exp, erw = _oracle(oracle_mod, raw, s, sd, 100, 0, 0.0)
        _assert_same(a.tree(q), exp)
        assert rw[q] == erw


def test_focus_and_skipped_travel(pkg, ctx, ctx_b):
    """GPU against GPU: a focused, pruned batch continued in place and in another batch"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, seeds = [raw["start"], STARTS[0], STARTS[1]], [5, 11, 12]
    a = _batch(pkg, raw, starts, seeds, 400, 0, 0.0, ctx=ctx)
    a.extend(200)
    a.plan(raw["goal"], focus=True, prune=True)
    st = a.export_forest()
    assert np.isfinite(st["focus_bound"]).any()
    a.extend(200)
    b = _batch(pkg, raw, STARTS[3:6], [41, 42, 43], 400, 0, 0.0, ctx=ctx_b)
    b.import_forest(st)
    b.extend(200)
    sa, sb = a.export_forest(), b.export_forest()
    _same_state(sa, sb)
    assert (sa["skipped"] > 0).any()
    for va, vb in zip(a.focus_state() + a.state(), b.focus_state() + b.state()):
        assert np.array_equal(_bits(va), _bits(vb))


def test_sizes_at_the_wave_boundary(pkg, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    sizes = [1, 2, 63, 64, 65, 130]
    trees = [ref.chain_tree(n, reverse=n == 130) for n in sizes]
    st = ref.pack(trees)
    assert st["cost"] is None
    a = _batch(pkg, raw, STARTS[:6], [1, 2, 3, 4, 5, 6], 200, 0, 0.0, ctx=ctx)
    a.import_forest(st)
    got = a.export_forest()
    v, bad, cost = ref.check_state(st, 200)
    assert v == ref.OK
    st["cost"] = cost
    _same_state(got, st)
    assert list(a.state()[0]) == sizes


def _raw_export(pkg, fn, ctx, arrays, kind, m, cap, queries=None):
    from pathplanning_amd import rrt

    st = rrt._forest_struct(kind, arrays)
    tot = C.c_int64(-1)
    q = None if queries is None else np.asarray(queries, dtype=np.int32)
    rc = fn(ctx.handle, None if q is None else q.ctypes.data_as(C.POINTER(C.c_int32)), m,
            C.byref(st), cap, C.byref(tot))
    return rc, tot.value


def test_rejections(pkg, ctx):
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.bench6_open()
    a = _batch(pkg, raw, [raw["start"]] + STARTS[:4], [5, 11, 12, 13, 14], 400, 0, 0.0, ctx=ctx)
    a.extend(60)
    before = a.export_forest()
    good, other = _tree_of(before, 0), _tree_of(before, 1)
    for name, bad_tree, expected in ref.bad_variants(good):
        with pytest.raises(_ffi.PPError) as e:
            a.import_forest(ref.pack([other, bad_tree, good]), [4, 2, 0])
        want = _ffi.PP_ERR_CAPACITY if expected == ref.CAPACITY else _ffi.PP_ERR_INVALID_ARGUMENT
        assert (e.value.code, e.value.bad_query) == (want, 2), name
    for queries in ([1, 1, 2], [0, 1, 9], [0, -1, 2]):
        with pytest.raises(_ffi.PPError) as e:
            a.import_forest(ref.pack([other, good, good]), queries)
        assert e.value.code == _ffi.PP_ERR_INVALID_ARGUMENT, queries
    with pytest.raises(_ffi.PPError) as e:
        a.import_forest(None, [0])
    assert e.value.code == _ffi.PP_ERR_INVALID_ARGUMENT
    with pytest.raises(_ffi.PPError) as e:
        a.export_forest([0, 0])
    assert e.value.code == _ffi.PP_ERR_INVALID_ARGUMENT
    _same_state(a.export_forest(), before)  # every failed call left the batch as it was
    # the sizing protocol: sizes only, then a capacity one row short
    L = _ffi.lib()
    total = int(before["off"][5])
    arrays = {"off": np.zeros(6, dtype=np.int64), "iterations": np.zeros(5, dtype=np.int64)}
    assert _raw_export(pkg, L.pp_star_forest_export, ctx, arrays, "s", 5, 0) == (_ffi.PP_OK, total)
    assert np.array_equal(arrays["off"], before["off"]) and list(arrays["iterations"]) == [60] * 5
    arrays = {"off": np.zeros(6, dtype=np.int64), "x": np.full(total, 7.0)}
    assert _raw_export(pkg, L.pp_star_forest_export, ctx, arrays, "s", 5, total - 1) == \
        (_ffi.PP_ERR_CAPACITY, total)
    assert np.array_equal(arrays["off"], before["off"]) and (arrays["x"] == 7.0).all()
    assert _raw_export(pkg, L.pp_star_forest_export, ctx, arrays, "s", 5, total) == (_ffi.PP_OK, total)
    assert np.array_equal(_bits(arrays["x"]), _bits(before["x"]))
    # a context without a batch
    empty = pkg.Context(0)
    try:
        rrt.Space.from_raw(raw)._upload(empty)
        st = rrt._forest_struct("s", {})
        tot, bad = C.c_int64(0), C.c_int32(0)
        for fn in (L.pp_star_forest_export, L.pp_batch_forest_export):
            assert fn(empty.handle, None, 1, C.byref(st), 0, C.byref(tot)) == _ffi.PP_ERR_STATE
        for fn in (L.pp_star_forest_import, L.pp_batch_forest_import):
            assert fn(empty.handle, None, 1, C.byref(st), C.byref(bad)) == _ffi.PP_ERR_STATE
    finally:
        empty.close()


def test_sub_batches(pkg, oracle_mod, ctx, ctx_b):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, _, seeds = scenes.config3_queries(raw, 0, 300)
    a = _batch(pkg, raw, starts, seeds, 80, 0, 0.0, ctx=ctx)
    a.extend(40)
    st = a.export_forest()
    b = _batch(pkg, raw, starts[::-1], np.asarray(seeds)[::-1] + 7, 80, 0, 0.0, ctx=ctx_b)
    b.import_forest(st, np.arange(299, -1, -1))
    b.extend(40)
    rw = b.state()[3]
    for q in (0, 149, 150, 151, 299):  # query q of `a` lives in slot 299 - q
        exp, erw = _oracle(oracle_mod, raw, tuple(starts[q]), int(seeds[q]), 80, 0, 0.0)
        _assert_same(b.tree(299 - q), exp)
        assert rw[299 - q] == erw


def test_other_scene_modes(pkg, oracle_mod, ctx, ctx_b):
    from pathplanning_amd import _ffi, scenes

    raw = scenes.field512_grid()  # the occupancy grid, one query
    a = _batch(pkg, raw, [raw["start"]], [3], 300, 0, 10.0, ctx=ctx)
    a.extend(100)
    b = _batch(pkg, raw, [raw["goal"]], [9], 300, 0, 10.0, ctx=ctx_b)
    b.import_forest(a.export_forest())
    b.extend(200)
    exp, erw = _oracle(oracle_mod, raw, tuple(raw["start"]), 3, 300, 0, 10.0)
    _assert_same(b.tree(0), exp)
    assert b.state()[3][0] == erw

    raw = scenes.bench6_polygons_open()  # polygon mode: a blocked root
    inside = (10.0, 5.0, 0.3)
    a = _batch(pkg, raw, [raw["start"], inside, raw["start"]], [3, 4, 6], 120, 0, 0.0, ctx=ctx)
    a.extend(40)
    st = a.export_forest([1])
    assert st["off"][1] == 1 and (st["x"][0], st["y"][0], st["yaw"][0]) == inside
    b = _batch(pkg, raw, [raw["start"], raw["start"]], [7, 8], 120, 0, 0.0, ctx=ctx_b)
    b.import_forest(st, [0])  # the root-only state round-trips, and stays blocked over there
    _same_state(b.export_forest([0]), st)
    b.extend(40)
    n, it, _, _ = b.state()
    assert n[0] == 1 and n[1] > 1 and list(it) == [80, 40]
    grown = _tree_of(a.export_forest([0]), 0)  # a grown tree moved onto the blocked root: refused
    grown["x"][0], grown["y"][0] = inside[0], inside[1]
    with pytest.raises(_ffi.PPError) as e:
        a.import_forest(ref.pack([grown]), [2])
    assert (e.value.code, e.value.bad_query) == (_ffi.PP_ERR_INVALID_ARGUMENT, 2)
    a.reset_queries([1], [raw["start"]], [21])  # the blocked slot onto a free start: it grows
    a.reset_queries([0], [inside], [22])        # a free slot onto the blocked start: never inserts
    a.extend(40)
    n, it, _, rw = a.state()
    assert n[0] == 1 and rw[0] == 0 and list(it) == [40, 40, 80]
    exp, erw = _oracle(oracle_mod, raw, tuple(raw["start"]), 21, 40, 0, 0.0)
    assert len(exp[0]) > 1
    _assert_same(a.tree(1), exp)
    exp, erw = _oracle(oracle_mod, raw, tuple(raw["start"]), 6, 80, 0, 0.0)
    _assert_same(a.tree(2), exp)


def _assert_same_tree(got, exp):
    x, y, yaw, par = got
    ex, ey, eyaw, epar = exp
    assert len(x) == len(ex)
    assert np.array_equal(x, ex) and np.array_equal(y, ey) and np.array_equal(par, epar)
    assert np.max(np.abs(yaw - eyaw), initial=0.0) <= 1e-9


def test_extend_batch(pkg, oracle_mod, ctx, ctx_b):
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.bench6_open()
    space = rrt.Space.from_raw(raw)
    starts, goals, seeds = scenes.config3_queries(raw, 0, 10)
    starts, goals = np.asarray(starts).reshape(-1, 3), np.asarray(goals).reshape(-1, 3)
    a = rrt.RRTBatch(starts[:4], goals[:4], 400, raw["step_size"], space, seeds[:4], ctx=ctx)
    a.extend(150)
    st = a.export_forest()
    assert set(st) == {"off", "x", "y", "yaw", "parent", "iterations", "seeds", "node_evals",
                       "goals"}
    assert np.array_equal(st["goals"], goals[:4]) and list(st["iterations"]) == [150] * 4
    b = rrt.RRTBatch(starts[4:], goals[4:], 400, raw["step_size"], space, seeds[4:], ctx=ctx_b)
    slots = [5, 1, 0, 3]
    b.import_forest(st, slots)
    got = b.export_forest(slots)
    _same_state(got, st)
    a.extend(250)
    b.extend(250)
    sc = oracle_mod.OracleScene.from_raw(raw)
    for i, s in enumerate(slots):
        tr = oracle_mod.OracleTree(tuple(starts[i]), 401)
        oracle_mod.rrt_extend(sc, tr, int(seeds[i]), 0, 400)
        _assert_same_tree(b.tree(s), tr.arrays())
    for s in (2, 4):  # the slots the import did not name ran their own 250 iterations
        tr = oracle_mod.OracleTree(tuple(starts[4 + s]), 401)
        oracle_mod.rrt_extend(sc, tr, int(seeds[4 + s]), 0, 250)
        _assert_same_tree(b.tree(s), tr.arrays())
    pa, pb = a.plan(), b.plan()
    for key in ("best_node", "length", "n_points", "n_finishes"):
        assert np.array_equal(_bits(pa[key]), _bits(pb[key][slots])), key
    assert (pa["best_node"] >= 0).any()
    # a parent that does not precede its child: pp_rrt_tree_import's rule
    bad = {k: v.copy() for k, v in st.items()}
    i = int(np.argmax(st["off"][1:] - st["off"][:-1] >= 3))
    bad["parent"][st["off"][i] + 1] = 2
    before = b.export_forest()
    with pytest.raises(_ffi.PPError) as e:
        b.import_forest(bad, slots)
    assert (e.value.code, e.value.bad_query) == (_ffi.PP_ERR_INVALID_ARGUMENT, slots[i])
    _same_state(b.export_forest(), before)

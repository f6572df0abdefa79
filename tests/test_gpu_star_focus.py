"""GPU parity of the RRT* batch's focused sampling (pp_star_set_focus / pp_star_get_focus, DESIGN.md
§3.7 "Focused sampling") against the CPU restatement tests/star_focus_ref.py.

Tolerances are tests/test_gpu_rrtstar.py's: node coordinates, parents, tree sizes, rewire counts,
`iterations` and `skipped` EXACT; yaw within 1e-9 absolute, node costs within 1e-9 relative.  A
bound that comes from the device's plan is read back with focus_state() and handed to the
restatement as it is (the bound is an input of the spec, not a result of it).

Two sentences of the cases are read as follows.  "plan's cost <= bound / R for every focused
reachable query" (the mixed-bounds case) is asserted for the queries whose bound is the plan's: a
path is never shorter than the distance between its ends, so no cost can be <= 0.5 x that distance
/ R.  "At least two queries of each scene see a non-zero skip" (the other scene modes) is asserted
as min(2, queries of the scene): two of the three scenes run one query."""
import ctypes as C
import math

import numpy as np
import pytest

import star_focus_ref as ref
import star_revalidate_ref as reval_ref
from test_gpu_rrtstar import _assert_same, _batch

pytestmark = pytest.mark.gpu

INF = math.inf


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _set_focus(b, fxy, bound):
    """pp_star_set_focus with bounds in length units; returns the status (no exception)"""
    from pathplanning_amd import _ffi

    dp = C.POINTER(C.c_double)
    f = None if fxy is None else np.ascontiguousarray(fxy, dtype=np.float64)
    d = None if bound is None else np.ascontiguousarray(bound, dtype=np.float64)
    return _ffi.lib().pp_star_set_focus(b.ctx.handle, None if f is None else f.ctypes.data_as(dp),
                                        None if d is None else d.ctypes.data_as(dp))


def _refs(oracle_mod, raw, starts, seeds, max_iter, k, eta, queries=None):
    osc = oracle_mod.OracleScene.from_raw(raw)
    qs = range(len(starts)) if queries is None else queries
    return {q: ref.Query(osc, starts[q], seeds[q], max_iter, k, eta) for q in qs}


def _focus_refs(refs, fxy, bound):
    for q, r in refs.items():
        r.set_focus(fxy[q][:2], bound[q])


def _extend(b, refs, n):
    b.extend(n)
    for r in refs.values():
        r.extend(n)


def _check(b, refs):
    n, it, _, rw = b.state()
    fxy, bound, skipped = b.focus_state()
    for q, r in refs.items():
        _assert_same(b.tree(q, n[q]), r.arrays())
        assert rw[q] == r.rewires, q
        assert it[q] == r.it, q
        assert skipped[q] == r.skipped, (q, skipped[q], r.skipped)
        assert bound[q] == r.bound, q
        if r.bound < INF:
            assert tuple(fxy[q]) == r.fxy, q


def _plan_or(b, starts, goals, factor=1.05):
    """the bounds of plan(goals): cost x turn radius where finite, else factor x the distance
    between root and goal"""
    _, cost = b.plan(goals)
    R = b.space.get_steer()
    return np.array([c * R if math.isfinite(c) else factor * ref.foci_distance(s, g)
                     for c, s, g in zip(cost, starts, goals)])


# ---------------------------------------------------------------------- 1. clearing the focus
def test_cleared_focus_is_the_plain_run(pkg, oracle_mod, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 3)
    b = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=ctx)
    b.extend(150)
    assert _set_focus(b, goals[:, :2], [INF] * 3) == 0
    b.extend(75)
    assert _set_focus(b, None, None) == 0
    b.extend(75)
    n, it, _, rw = b.state()
    _, bound, skipped = b.focus_state()
    assert (it == 300).all() and (skipped == 0).all() and np.isinf(bound).all()
    osc = oracle_mod.OracleScene.from_raw(raw)
    for q in range(3):
        tr = oracle_mod.OracleStarTree(tuple(starts[q]), 301)
        _, erw, _, _ = oracle_mod.star_extend(osc, tr, int(seeds[q]), 0, 300, 0, 0.0)
        _assert_same(b.tree(q, n[q]), tr.star_arrays())
        assert rw[q] == erw


# ------------------------------------------------------- 2. mixed bounds in one workgroup
@pytest.mark.parametrize("k,eta", [(0, 0.0), (4, 2.0)])
def test_mixed_bounds_in_one_workgroup(pkg, oracle_mod, ctx, k, eta):
    """q0 the plan's bound, q1 1.002 x and q2 0.5 x the distance between the foci, q3 unfocused:
    the four waves of one workgroup leave the draw loop after different rounds"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    R = raw["robot"][2]
    starts, goals, seeds = scenes.config3_queries(raw, 0, 4)
    b = _batch(pkg, raw, starts, seeds, 300, k, eta, ctx=ctx)
    refs = _refs(oracle_mod, raw, starts, seeds, 300, k, eta)
    _extend(b, refs, 150)
    _check(b, refs)
    _, cost = b.plan(goals)
    assert math.isfinite(cost[0])
    dist = [ref.foci_distance(starts[q], goals[q]) for q in range(4)]
    bound = [cost[0] * R, 1.002 * dist[1], 0.5 * dist[2], INF]
    assert _set_focus(b, goals[:, :2], bound) == 0
    _focus_refs(refs, goals, bound)
    for n in (1, 37, 112):
        _extend(b, refs, n)
    _check(b, refs)
    assert (b.state()[1] == 300).all()
    # every class of iteration occurred: no skip, first round, a later round, a full miss
    tot = np.sum([ref.classes(refs[q].js[150:]) for q in range(3)], axis=0)
    assert (tot > 0).all(), tot
    assert ref.classes(refs[2].js[150:]) == (0, 0, 0, 150)
    assert refs[3].skipped == 0
    _, after = b.plan(goals)
    assert after[0] <= bound[0] / R


# ------------------------------------------------- 3. the focus changes between calls
def test_focus_changes_between_calls(pkg, oracle_mod, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 3)
    b = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=ctx)
    refs = _refs(oracle_mod, raw, starts, seeds, 300, 0, 0.0)
    _extend(b, refs, 150)
    _, cost1 = b.plan(goals, focus=True)
    fxy, bound1, _ = b.focus_state()
    assert np.array_equal(fxy, goals[:, :2])
    assert np.array_equal(bound1, cost1 * np.float64(raw["robot"][2]))
    assert np.isfinite(bound1).any()
    _focus_refs(refs, goals, bound1)
    _extend(b, refs, 50)
    _check(b, refs)
    _, cost2 = b.plan(goals, focus=True)  # tighter, or the same
    bound2 = b.focus_state()[1]
    assert (cost2 <= cost1).all()
    _focus_refs(refs, goals, bound2)
    _extend(b, refs, 50)
    _check(b, refs)
    b.focus()  # cleared: the skip stays in force
    for r in refs.values():
        r.set_focus()
    kept = b.focus_state()[2].copy()
    assert (kept > 0).any()
    _extend(b, refs, 50)
    _check(b, refs)
    assert np.array_equal(b.focus_state()[2], kept)


# ------------------------------------------------------------------------- 4. the max_iter cap
def test_max_iter_caps_a_focused_extend(pkg, oracle_mod, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 3)
    b = _batch(pkg, raw, starts, seeds, 200, 0, 0.0, ctx=ctx)
    refs = _refs(oracle_mod, raw, starts, seeds, 200, 0, 0.0)
    _extend(b, refs, 100)
    dist = [ref.foci_distance(starts[q], goals[q]) for q in range(3)]
    bound = [_plan_or(b, starts, goals)[0], 1.002 * dist[1], 0.5 * dist[2]]
    assert _set_focus(b, goals[:, :2], bound) == 0
    _focus_refs(refs, goals, bound)
    _extend(b, refs, 1000)
    n, it, _, _ = b.state()
    assert list(it) == [200] * 3 and (n <= 201).all()
    assert b.focus_state()[2][2] == refs[2].skipped == 100 * (ref.DRAWS - 1)
    _check(b, refs)
    _extend(b, refs, 5)  # at the cap nothing moves, the skip included
    _check(b, refs)


# ------------------------------------------------------------------------- 5. sub-batches
def test_focus_follows_the_sub_batch_split(pkg, oracle_mod, ctx):
    """300 queries run as sub-batches of consecutive queries: focused queries on both sides of
    the boundaries of a split in halves and in thirds and at both ends, and their neighbours"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 300)
    focused = (0, 99, 100, 149, 150, 199, 200, 299)
    others = (1, 98, 101, 148, 151, 198, 201, 298)
    b = _batch(pkg, raw, starts, seeds, 80, 0, 0.0, ctx=ctx)
    refs = _refs(oracle_mod, raw, starts, seeds, 80, 0, 0.0, queries=focused + others)
    _extend(b, refs, 40)
    bound = np.full(300, INF)
    for q in focused:
        bound[q] = 1.002 * ref.foci_distance(starts[q], goals[q])
    assert _set_focus(b, goals[:, :2], bound) == 0
    _focus_refs(refs, goals, bound)
    _extend(b, refs, 40)
    _check(b, refs)
    assert all(refs[q].skipped > 0 for q in focused)
    _, it, _, _ = b.state()
    skipped = b.focus_state()[2]
    assert (it == 80).all()
    assert (skipped[[q for q in range(300) if q not in focused]] == 0).all()


# ----------------------------------------------------------------- 6. the other scene modes
def _scene_cases():
    from pathplanning_amd import scenes

    for name, eta in (("field512_grid", 10.0), ("bench6_polygons_open", 0.0)):
        raw = getattr(scenes, name)()
        yield raw, [raw["start"]], np.array([raw["goal"]]), [3], eta
    raw = scenes.config5_field()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 6)
    yield raw, starts, goals, seeds, scenes.CONFIG5_ETA


@pytest.mark.parametrize("which", [0, 1, 2])
def test_focus_in_the_other_scene_modes(pkg, oracle_mod, ctx, which):
    """the occupancy grid, create_circle polygons and config 5's disc field"""
    raw, starts, goals, seeds, eta = list(_scene_cases())[which]
    b = _batch(pkg, raw, starts, seeds, 300, 0, eta, ctx=ctx)
    refs = _refs(oracle_mod, raw, starts, seeds, 300, 0, eta)
    _extend(b, refs, 150)
    bound = _plan_or(b, starts, goals)
    assert _set_focus(b, goals[:, :2], bound) == 0
    _focus_refs(refs, goals, bound)
    _extend(b, refs, 150)
    _check(b, refs)
    assert sum(r.skipped > 0 for r in refs.values()) >= min(2, len(refs))


# ------------------------------------------------------------------- 7. far from the origin
def test_focus_far_from_the_origin(pkg, oracle_mod, ctx):
    from pathplanning_amd import scenes
    from scene_xform import moved

    raw = moved(scenes.bench6_open(), 5e5, 4e6)
    starts, goals, seeds = scenes.config3_queries(raw, 0, 2)
    b = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=ctx)
    refs = _refs(oracle_mod, raw, starts, seeds, 300, 0, 0.0)
    _extend(b, refs, 150)
    bound = _plan_or(b, starts, goals)
    assert _set_focus(b, goals[:, :2], bound) == 0
    _focus_refs(refs, goals, bound)
    _extend(b, refs, 150)
    _check(b, refs)
    assert all(r.skipped > 0 for r in refs.values())


# ------------------------------------------------------ 8. a scene change keeps the focus
def test_scene_change_keeps_the_focus(pkg, oracle_mod, ctx):
    from pathplanning_amd import rrt, scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 4)
    b = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=ctx)
    refs = _refs(oracle_mod, raw, starts, seeds, 300, 0, 0.0)
    _extend(b, refs, 150)
    bound = _plan_or(b, starts, goals)
    assert _set_focus(b, goals[:, :2], bound) == 0
    _focus_refs(refs, goals, bound)
    _extend(b, refs, 100)
    _check(b, refs)
    n = b.state()[0]
    before = [b.tree(q, n[q]) for q in range(4)]
    focus_before = b.focus_state()
    v = reval_ref.quarter_subtree_node(before[0])
    raw2 = reval_ref.with_discs(raw, [(before[0][0][v], before[0][1][v], 0.3)])
    osc2 = oracle_mod.OracleScene.from_raw(raw2)
    n_new, _ = b.set_space(rrt.Space.from_raw(raw2))  # uploads the scene and revalidates
    for got, exp in zip(b.focus_state(), focus_before):
        assert np.array_equal(got, exp)
    dropped = 0
    for q, r in refs.items():
        e = reval_ref.revalidate(osc2, before[q])
        assert n_new[q] == e["kept"]
        dropped += len(before[q][0]) - e["kept"]
        r.osc = osc2
        r.tr = reval_ref.oracle_tree(starts[q], e["tree"], e["elen"][e["keep"]], 50)
        r.rewires_before = r.rewires
    assert dropped > 0
    rw0 = b.state()[3].copy()
    _extend(b, refs, 50)
    _check(b, refs)
    assert np.array_equal(b.state()[3] - rw0, [r.rewires - r.rewires_before for r in refs.values()])


# --------------------------------------------------------------------------------- 9. errors
def test_focus_errors_leave_the_state_unchanged(pkg, ctx):
    from pathplanning_amd import _ffi, scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 3)
    b = _batch(pkg, raw, starts, seeds, 50, 0, 0.0, ctx=ctx)
    good = [7.5, INF, 12.0]
    assert _set_focus(b, goals[:, :2], good) == 0
    b.extend(20)
    state = b.focus_state()
    assert np.array_equal(state[0], goals[:, :2]) and list(state[1]) == good
    far = goals[:, :2].copy()
    far[1, 1] = 2.0 * _ffi.PP_COORD_MAX
    nan_xy = goals[:, :2].copy()
    nan_xy[2, 0] = math.nan
    other = goals[:, :2] + 1.0
    for fxy, bound in ((other, [1.0, math.nan, 1.0]), (other, [1.0, 0.0, 1.0]),
                       (other, [1.0, 1.0, -2.0]), (other, [-INF, 1.0, 1.0]),
                       (far, [1.0, 1.0, 1.0]), (nan_xy, [1.0, 1.0, 1.0]),
                       (other, None), (None, [1.0, 1.0, 1.0])):
        assert _set_focus(b, fxy, bound) == _ffi.PP_ERR_INVALID_ARGUMENT
        for got, exp in zip(b.focus_state(), state):
            assert np.array_equal(got, exp)
    with pytest.raises(ValueError):
        b.focus(goals)
    # without an RRT* batch
    c = pkg.Context(0)
    try:
        L = _ffi.lib()
        dp = C.POINTER(C.c_double)
        x = np.ones(6)
        assert L.pp_star_set_focus(c.handle, x.ctypes.data_as(dp), x.ctypes.data_as(dp)) == _ffi.PP_ERR_STATE
        assert L.pp_star_set_focus(c.handle, None, None) == _ffi.PP_ERR_STATE
        assert L.pp_star_get_focus(c.handle, x.ctypes.data_as(dp), None, None) == _ffi.PP_ERR_STATE
    finally:
        c.close()
    # a new batch starts unfocused with nothing skipped
    b2 = _batch(pkg, raw, starts, seeds, 50, 0, 0.0, ctx=ctx)
    _, bound, skipped = b2.focus_state()
    assert np.isinf(bound).all() and (skipped == 0).all()

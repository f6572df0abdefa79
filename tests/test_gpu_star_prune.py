"""GPU: pp_star_prune (DESIGN.md §3.7 "Pruning by the focus bound") against the CPU restatement
tests/star_prune_ref.py.

Exactness rule: the restatement is fed the trees EXPORTED FROM THE DEVICE just before the call and
the focus read back by focus_state(); n_nodes, last_dropped, new_index and the exported trees after
the call (x, y, yaw, remapped parents, cost) are compared with ==.  No tolerance applies: the
inputs are the device's own and the node test is exact f64.  Only the continuation test compares
with trees the oracle grew, at tests/test_gpu_rrtstar.py's tolerances (coordinates, parents, tree
sizes, rewire counts, `iterations` and `skipped` exact; yaw 1e-9 absolute, cost 1e-9 relative),
under the margin condition of tests/test_star_prune_ref.py.

The four-wave case's q1 takes its bound factor from tests/test_star_prune_ref.py (Q1_FACTOR, and
why it is not the focus tests' 1.002; that bound runs in the sub-batch case here).  In its (4, 2)
run the kept nodes under a later parent all sit in the unfocused q3 (the restatement finds none in
the three small pruned trees); kept nodes under later parents next to real drops are asserted in
the plan-invariance case."""
import ctypes as C
import math

import numpy as np
import pytest

import star_focus_ref as focus_ref
import star_prune_ref as ref
import star_revalidate_ref as reval_ref
from star_tree_cases import _assert_exact, _set_space_checked, _trees
from test_gpu_rrtstar import _assert_same, _batch
from test_gpu_star_focus import _check, _extend, _focus_refs, _plan_or, _refs, _set_focus
from test_star_prune_ref import KETA, MARGIN, Q1_FACTOR

pytestmark = pytest.mark.gpu

INF = math.inf


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _offsets(n_old):
    return np.concatenate([[0], np.cumsum(n_old, dtype=np.int64)])


def _prune_checked(b, keep, check=None):
    """b.prune(keep) against the restatement on the trees exported just before it and the focus
    read back; everything the call returns and leaves behind.  `check`: the queries whose rows are
    compared (all).  Returns (the trees before, the restatements, n_nodes, new_index)."""
    before = _trees(b)
    fxy, bound, skipped = b.focus_state()
    n_old, it_old, ev_old, rw_old = b.state()
    R = b.space.get_steer()
    exp = [ref.prune(before[q], R, fxy[q], bound[q], -1 if keep is None else int(keep[q]))
           for q in range(b.q)]
    n_new, new_index = b.prune(keep, n_old)
    off = _offsets(n_old)
    assert len(new_index) == off[-1]
    assert np.array_equal(n_new, [e["kept"] for e in exp])
    assert b.last_dropped == int(n_old.sum()) - int(n_new.sum())
    assert np.array_equal(new_index, np.concatenate([e["new_index"] for e in exp]))
    n_state, it, ev, rw = b.state()
    assert np.array_equal(n_state, n_new)
    assert np.array_equal(it, it_old) and np.array_equal(ev, ev_old) and np.array_equal(rw, rw_old)
    for got, was in zip(b.focus_state(), (fxy, bound, skipped)):
        assert np.array_equal(got, was)
    for q in (range(b.q) if check is None else check):
        _assert_exact(b.tree(q, n_new[q]), exp[q]["tree"])
    return before, exp, n_new, new_index


def _four_waves(pkg, oracle_mod, ctx, k, eta, with_refs):
    """bench6_open, queries 0-3, 150 steps, then q0 the plan's bound with its best node kept, q1
    Q1_FACTOR x the distance between the foci, q2 0.5 x with the deepest node kept, q3 unfocused"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    R = raw["robot"][2]
    starts, goals, seeds = scenes.config3_queries(raw, 0, 4)
    b = _batch(pkg, raw, starts, seeds, 200, k, eta, ctx=ctx)
    refs = _refs(oracle_mod, raw, starts, seeds, 200, k, eta) if with_refs else {}
    _extend(b, refs, 150)
    node, cost = b.plan(goals)
    assert node[0] >= 0 and math.isfinite(cost[0])
    dist = [focus_ref.foci_distance(starts[q], goals[q]) for q in range(4)]
    bound = [cost[0] * R, Q1_FACTOR * dist[1], 0.5 * dist[2], INF]
    assert _set_focus(b, goals[:, :2], bound) == 0
    _focus_refs(refs, goals, bound)
    n = b.state()[0]
    deepest = int(np.argmax(reval_ref.depth(b.tree(2, n[2])[3])))
    keep = np.array([node[0], -1, deepest, -1], dtype=np.int32)
    return b, refs, raw, starts, goals, keep


# ------------------------------------------------------------------------------ 1. identity
def test_unfocused_prune_is_the_identity(pkg, oracle_mod, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, _, seeds = scenes.config3_queries(raw, 0, 3)
    b = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=ctx)
    b.extend(150)
    before, _, n_new, new_index = _prune_checked(b, None)
    assert b.last_dropped == 0
    assert np.array_equal(new_index, np.concatenate([np.arange(n) for n in n_new]))
    for q, t in enumerate(_trees(b)):
        _assert_exact(t, before[q])
    b.extend(150)
    n, it, _, rw = b.state()
    assert (it == 300).all()
    osc = oracle_mod.OracleScene.from_raw(raw)
    for q in range(3):
        tr = oracle_mod.OracleStarTree(tuple(starts[q]), 301)
        _, erw, _, _ = oracle_mod.star_extend(osc, tr, int(seeds[q]), 0, 300, 0, 0.0)
        _assert_same(b.tree(q, n[q]), tr.star_arrays())
        assert rw[q] == erw


# -------------------------------------------------------- 2. four waves of one workgroup
@pytest.mark.parametrize("k,eta", KETA)
def test_four_waves_of_one_workgroup(pkg, oracle_mod, ctx, k, eta):
    b, _, _, _, _, keep = _four_waves(pkg, oracle_mod, ctx, k, eta, False)
    before, exp, n_new, _ = _prune_checked(b, keep)
    for q in (0, 1):  # something goes, something beside the root stays
        assert 1 < exp[q]["kept"] < len(before[q][0]), (q, exp[q]["kept"])
    # q2: an empty set — exactly the protected chain
    d = reval_ref.depth(before[2][3])
    assert d[keep[2]] >= 2 and n_new[2] == d[keep[2]] + 1
    assert np.array_equal(np.flatnonzero(exp[2]["keep"]), np.sort(ref.chain(before[2][3], keep[2])))
    # q3: unfocused, bit-equal (the rows are compared in _prune_checked)
    assert n_new[3] == len(before[3][0]) and exp[3]["keep"].all()
    if k == 4:
        back = 0
        for q in range(4):
            par = b.tree(q, n_new[q])[3]
            back += int((par[1:] > np.arange(1, len(par))).sum())
        assert back > 0


# ------------------------------------------------------------------------ 3. plan invariance
def test_plan_is_invariant_under_its_own_prune(pkg, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    R = raw["robot"][2]
    starts, goals, seeds = scenes.config3_queries(raw, 0, 4)
    b = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=ctx)
    b.extend(150)
    before = _trees(b)
    totals = [b.goal_costs(q, goals[q]) for q in range(4)]
    n_old, it_old, _, rw_old = b.state()
    skipped_old = b.focus_state()[2]
    node0, cost0 = b.plan(goals)
    with pytest.raises(ValueError):
        b.plan(goals, prune=True)
    node, cost = b.plan(goals, focus=True, prune=True)
    assert np.array_equal(cost, cost0)
    assert (node0 >= 0).sum() >= 3
    fxy, bound, skipped = b.focus_state()
    assert np.array_equal(fxy, goals[:, :2])
    assert np.array_equal(bound, cost0 * np.float64(R))
    assert np.array_equal(skipped, skipped_old)
    n_new, it, _, rw = b.state()
    assert np.array_equal(it, it_old) and np.array_equal(rw, rw_old)
    exp = [ref.prune(before[q], R, fxy[q], bound[q], int(node0[q])) for q in range(4)]
    assert np.array_equal(n_new, [e["kept"] for e in exp]) and (n_new < n_old).any()
    assert sum(e["kept_back"] for e in exp if e["kept"] < len(e["keep"])) > 0
    for q in range(4):
        _assert_exact(b.tree(q, n_new[q]), exp[q]["tree"])
        assert node[q] == (exp[q]["new_index"][node0[q]] if node0[q] >= 0 else -1)
        assert np.array_equal(b.goal_costs(q, goals[q]), totals[q][exp[q]["keep"]])
    node2, cost2 = b.plan(goals)
    assert np.array_equal(cost2, cost0) and np.array_equal(node2, node)
    n2, idx2 = b.prune(node)
    assert b.last_dropped == 0 and np.array_equal(n2, n_new)
    assert np.array_equal(idx2, np.concatenate([np.arange(n) for n in n_new]))


# --------------------------------------------------------------------------- 4. continuation
@pytest.mark.parametrize("k,eta", KETA)
def test_pruned_trees_continue_like_the_oracle(pkg, oracle_mod, ctx, k, eta):
    """50 more focused steps on the shrunken trees: mark / stamp and the k schedule.  Every
    reference query prunes its own (oracle-grown) tree with the device's inputs and continues from
    the result."""
    b, refs, raw, starts, goals, keep = _four_waves(pkg, oracle_mod, ctx, k, eta, True)
    _check(b, refs)
    fxy, bound, _ = b.focus_state()
    R = b.space.get_steer()
    for q, r in refs.items():  # the condition under which the two prunes agree
        assert ref.margin(r.arrays(), R, fxy[q], bound[q], keep[q]) > MARGIN, q
    _, _, n_new, _ = _prune_checked(b, keep)
    for q, r in refs.items():
        e = ref.prune(r.arrays(), R, fxy[q], bound[q], int(keep[q]))
        assert e["kept"] == n_new[q], q
        r.tr = reval_ref.oracle_tree(starts[q], e["tree"], e["elen"], 50)
    _check(b, refs)
    _extend(b, refs, 50)
    _check(b, refs)
    assert (b.state()[1] == 200).all()
    assert sum(r.rewires for r in refs.values()) > 0


# -------------------------------------------------------- 5. sub-batches and scan blocks
def test_prune_across_sub_batches_and_scan_blocks(pkg, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 300)
    focused = (0, 99, 100, 149, 150, 199, 200, 299)
    b = _batch(pkg, raw, starts, seeds, 80, 0, 0.0, ctx=ctx)
    b.extend(40)
    bound = np.full(300, INF)
    for q in focused:
        bound[q] = 1.002 * focus_ref.foci_distance(starts[q], goals[q])
    assert _set_focus(b, goals[:, :2], bound) == 0
    b.extend(40)
    n_old = b.state()[0]
    # the 1024-node scan workgroups and the 256-node blocks split inside trees
    assert n_old.sum() > 2048 and n_old.max() < 256
    keep = np.full(300, -1, dtype=np.int32)
    for q in focused[::2]:
        keep[q] = int(np.argmax(reval_ref.depth(b.tree(q, n_old[q])[3])))
    before, exp, n_new, new_index = _prune_checked(b, keep)
    # (query 299 never leaves its root)
    grown = [q for q in focused if n_old[q] > 1]
    assert len(grown) >= 6 and all(n_new[q] < n_old[q] for q in grown)
    assert sum(exp[q]["kept_back"] for q in grown) > 0  # later parents, remapped past real drops
    off = _offsets(n_old)
    for q in range(300):
        if q not in focused:
            assert n_new[q] == n_old[q]
            assert np.array_equal(new_index[off[q]:off[q + 1]], np.arange(n_old[q]))


# ------------------------------------------------------------------- 6. far from the origin
def test_prune_far_from_the_origin(pkg, ctx):
    from pathplanning_amd import scenes
    from scene_xform import moved

    raw = moved(scenes.bench6_open(), 5e5, 4e6)
    starts, goals, seeds = scenes.config3_queries(raw, 0, 2)
    b = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=ctx)
    b.extend(150)
    node, _ = b.plan(goals)
    assert _set_focus(b, goals[:, :2], _plan_or(b, starts, goals)) == 0
    before, exp, n_new, _ = _prune_checked(b, node)
    for q in range(2):
        assert 1 <= n_new[q] < len(before[q][0]), q
    assert n_new.max() > 1


# ---------------------------------------------------------- 7. composes with a scene change
def test_prune_then_a_scene_change(pkg, oracle_mod, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 4)
    b = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=ctx)
    b.extend(150)
    node, _ = b.plan(goals, focus=True)
    _, exp, n_new, _ = _prune_checked(b, node)
    pruned = _trees(b)
    q = int(np.argmax(n_new))
    assert n_new[q] >= 8 and b.last_dropped > 0
    v = reval_ref.quarter_subtree_node(pruned[q])
    raw2 = reval_ref.with_discs(raw, [(pruned[q][0][v], pruned[q][1][v], 0.3)])
    focus_before = b.focus_state()
    _, rexp = _set_space_checked(oracle_mod, b, pruned, raw2)
    assert not rexp[q]["keep"][v] and rexp[q]["kept"] < n_new[q]
    for got, was in zip(b.focus_state(), focus_before):
        assert np.array_equal(got, was)


# ------------------------------------------------------------------------ 8. errors and NULLs
def test_prune_errors_and_nulls(pkg):
    from pathplanning_amd import _ffi, rrt, scenes

    L = _ffi.lib()
    ip = C.POINTER(C.c_int32)
    raw = scenes.bench6_open()
    c = pkg.Context(0)
    try:
        assert L.pp_star_prune(c.handle, None, None, None, None) == _ffi.PP_ERR_STATE  # no scene
        rrt.Space.from_raw(raw)._upload(c)
        assert L.pp_star_prune(c.handle, None, None, None, None) == _ffi.PP_ERR_STATE  # no batch
        starts, goals, seeds = scenes.config3_queries(raw, 0, 4)
        eb = rrt.RRTBatch(starts, goals, 300, raw["step_size"], rrt.Space.from_raw(raw), seeds, ctx=c)
        eb.extend(200)
        n_eb = eb.state()[0]
        eb_before = [eb.tree(q, n_eb[q]) for q in range(4)]
        sb = _batch(pkg, raw, starts, seeds, 300, 0, 0.0, ctx=c)
        sb.extend(150)
        node, _ = sb.plan(goals, focus=True)
        before, focus_before = _trees(sb), sb.focus_state()
        n_old = sb.state()[0]
        for q, bad in ((0, int(n_old[0])), (3, int(n_old[3])), (1, -2), (2, 1 << 30)):
            keep = np.array(node, dtype=np.int32)
            keep[q] = bad
            n_out = np.full(4, -7, dtype=np.int32)
            assert L.pp_star_prune(c.handle, keep.ctypes.data_as(ip), n_out.ctypes.data_as(ip),
                                   None, None) == _ffi.PP_ERR_INVALID_ARGUMENT
            assert (n_out == -7).all()
            for t, was in zip(_trees(sb), before):
                _assert_exact(t, was)
            for got, was in zip(sb.focus_state(), focus_before):
                assert np.array_equal(got, was)
        # every pointer NULL: accepted, and the trees are the restatement's with no protected chain
        R = sb.space.get_steer()
        exp = [ref.prune(before[q], R, focus_before[0][q], focus_before[1][q], -1) for q in range(4)]
        assert L.pp_star_prune(c.handle, None, None, None, None) == _ffi.PP_OK
        n_new = sb.state()[0]
        assert np.array_equal(n_new, [e["kept"] for e in exp]) and n_new.sum() < n_old.sum()
        for q in range(4):
            _assert_exact(sb.tree(q, n_new[q]), exp[q]["tree"])
        # the extend batch's forest in the same context is as it was: its own revalidation in the
        # unchanged scene keeps every node and every row
        n_back, idx = eb.revalidate(n_eb)
        assert np.array_equal(n_back, n_eb) and eb.last_dropped == 0
        assert np.array_equal(idx, np.concatenate([np.arange(n) for n in n_eb]))
        for q in range(4):
            _assert_exact(eb.tree(q, n_eb[q]), eb_before[q])
    finally:
        c.close()

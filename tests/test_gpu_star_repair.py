"""Dropped subtrees of an RRT* batch hung back under kept nodes after a scene change:
pp_star_repair (DESIGN.md §3.8 "Re-attaching orphaned subtrees") against the CPU restatement
tests/star_repair_ref.py.  The trees are grown on the GPU, exported, and restated on the CPU from
the exported poses, parents and costs.

Exact: the kept set, new_index, n_nodes, last_dropped / last_reattached / last_recovered, the
coordinates and stored yaw (bit-equal to the export before the call), the parents (a mismatch
prints the smallest runner-up gap of the tree's tops), and the cost of the nodes pp_star_revalidate
keeps (bit-equal to the export).  The cost of a recovered node: 1e-9 relative (its new edge's
Dubins cost is ocml's against glibc's, tests/test_gpu_rrtstar.py).  The continued runs against
orc_star_extend at that file's tolerances.

Each case asserts its own conditions on the restatement, so a scene that stops exercising the
case fails instead of passing vacuously.  Case 2's are: at least 3 re-attached tops, at least one
top without a parent and at least 30 recovered nodes per pruned tree — counted with the tops, as
n_recovered counts them: the smallest is 31 ((k 0, eta 2) tree 0, 23 of them below its 8 tops), so
"30 that are not tops" does not hold for the inputs themselves; instead more nodes must come back
below the tops than there are tops."""
import numpy as np
import pytest

import revalidate_ref
import star_goal_ref
import star_repair_ref as rep
import star_revalidate_ref as ref
from star_tree_cases import (_assert_exact, _continue_checked, _space, _square, _starts, _trees,
                             _with_ring)
from test_gpu_rrtstar import COST_RTOL, _batch

pytestmark = pytest.mark.gpu

SEEDS = [0, 5, 11, 12]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _assert_tree(q, got, e):
    """one query's tree after the call against its restatement e"""
    x, y, yaw, par, cost = got
    ex, ey, eyaw, epar, ecost = e["tree"]
    assert len(x) == len(ex), (q, len(x), len(ex))
    assert np.array_equal(x, ex) and np.array_equal(y, ey) and np.array_equal(yaw, eyaw), q
    assert np.array_equal(par, epar), (q, np.flatnonzero(par != epar)[:10], rep.min_gap(e))
    k0 = e["keep0"][e["keep"]]
    assert np.array_equal(cost[k0], ecost[k0]), q
    assert np.allclose(cost[~k0], ecost[~k0], rtol=COST_RTOL, atol=0.0), q


def _repair_checked(oracle_mod, b, before, raw_new, k, rounds):
    """set_space(raw_new, repair_rounds=rounds) on batch b holding the trees `before`: everything
    the call returns and leaves behind against the restatement.  Returns (the new scene, the
    restatements)."""
    osc = oracle_mod.OracleScene.from_raw(raw_new)
    exp = [rep.repair(osc, t, k, rounds) for t in before]
    assert sum(e["none_edges"] for e in exp) == 0
    n_old = np.array([len(t[0]) for t in before])
    _, it_old, ev_old, rw_old = b.state()
    n_new, new_index = b.set_space(_space(raw_new), repair_rounds=rounds)
    off = np.concatenate([[0], np.cumsum(n_old)])
    assert len(new_index) == off[-1]
    assert np.array_equal(n_new, [e["kept"] for e in exp])
    assert b.last_dropped == int((n_old - n_new).sum())
    assert b.last_reattached == sum(e["reattached"] for e in exp)
    assert b.last_recovered == sum(e["recovered"] for e in exp)
    n_state, it, ev, rw = b.state()
    assert np.array_equal(n_state, n_new)
    assert np.array_equal(it, it_old) and np.array_equal(ev, ev_old) and np.array_equal(rw, rw_old)
    for q, e in enumerate(exp):
        got_index = new_index[off[q]:off[q + 1]]
        assert np.array_equal(got_index, e["new_index"]), (q, np.flatnonzero(got_index != e["new_index"])[:10],
                                                           rep.min_gap(e))
        _assert_tree(q, b.tree(q, n_new[q]), e)
    return osc, exp


# ------------------------------------------- 1. rounds = 0, and the unchanged scene
def test_zero_rounds_is_revalidate_and_unchanged_scene_is_the_identity(pkg, ctx):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts = _starts(raw)
    a = _batch(pkg, raw, starts, SEEDS, 400, 0, 0.0, ctx=ctx)
    twin = _batch(pkg, raw, starts, SEEDS, 400, 0, 0.0)  # (a context holds one RRT* batch)
    a.extend(400)
    twin.extend(400)
    whole, whole_state = _trees(a), a.state()
    _assert_exact(sum((list(t) for t in _trees(twin)), []), sum((list(t) for t in whole), []))
    # the unchanged scene: nothing is dropped, so there is nothing to re-attach
    n_new, new_index = a.repair(3)
    assert np.array_equal(n_new, whole_state[0])
    assert a.last_dropped == 0 and a.last_reattached == 0 and a.last_recovered == 0
    assert np.array_equal(new_index, np.concatenate([np.arange(n) for n in n_new]))
    for q, t in enumerate(_trees(a)):
        _assert_exact(t, whole[q])
    for s, e in zip(a.state(), whole_state):
        assert np.array_equal(s, e)
    # rounds = 0 against revalidate() on the twin, a disc through tree 0
    v = ref.quarter_subtree_node(whole[0])
    raw2 = ref.with_discs(raw, [(whole[0][0][v], whole[0][1][v], 0.3)])
    n_a, idx_a = a.set_space(_space(raw2), repair_rounds=0)
    n_t, idx_t = twin.set_space(_space(raw2))
    assert np.array_equal(n_a, n_t) and np.array_equal(idx_a, idx_t) and n_a[0] < whole_state[0][0]
    assert a.last_dropped == twin.last_dropped > 0
    assert a.last_reattached == 0 and a.last_recovered == 0
    for ta, tt in zip(_trees(a), _trees(twin)):
        _assert_exact(ta, tt)
    for s, e in zip(a.state(), twin.state()):
        assert np.array_equal(s, e)
    twin.close()


# ------------------------------------------------------- 2. one disc, and what follows
@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("k,eta", [(0, 0.0), (0, 2.0), (4, 0.0), (63, 0.0)])
def test_one_disc_then_continue(pkg, ctx, oracle_mod, k, eta, rounds):
    """a disc of r 0.3 on the n/4-subtree node of each of the four trees in turn"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts = _starts(raw)
    n1, n2 = 400, 300
    goal = raw["goal"]
    later = 0
    for j in range(4):
        b = _batch(pkg, raw, starts, SEEDS, n1 + n2, k, eta, ctx=ctx)
        b.extend(n1)
        before = _trees(b)
        v = ref.quarter_subtree_node(before[j])
        raw2 = ref.with_discs(raw, [(before[j][0][v], before[j][1][v], 0.3)])
        osc2, exp = _repair_checked(oracle_mod, b, before, raw2, k, rounds)
        r = exp[j]
        assert not r["keep0"][v] and 1 < r["keep0"].sum() < r["kept"] <= len(before[j][0]), r["rounds"]
        assert r["reattached"] >= 3 and r["failed_tops"] >= 1, r["rounds"]
        assert r["recovered"] >= 30, r["rounds"]
        assert r["recovered"] - r["reattached"] > r["reattached"], r["rounds"]
        later += sum(d["reattached"] for d in r["rounds"][1:])
        _continue_checked(oracle_mod, b, osc2, exp, SEEDS, n1, n2, k, eta, range(4))
        # the goal connection on the repaired-and-extended trees, in the new scene
        after = _trees(b)
        node, cost = b.plan(goal)
        for q in range(4):
            enode, ecost, etotal = star_goal_ref.plan(osc2, after[q], goal)
            assert node[q] == enode, (q, node[q], enode, star_goal_ref.runner_up_gap(etotal))
        assert (node >= 0).any()
        off, xy, length, ok = b.paths(goal, node)
        assert np.array_equal(ok, node >= 0)
        for q in range(4):
            line = xy[off[q]:off[q + 1]]
            assert (len(line) > 0) == bool(ok[q])
            if ok[q]:
                assert osc2.verify_line(line[:, 0], line[:, 1]), q
    if rounds == 3 and (k, eta) in [(0, 2.0), (4, 0.0)]:
        assert later > 0  # a later round re-attaches (trees 2, 3 and trees 1, 3)


# ------------------------------------------------------------------------------ 3. the grid
def test_field512_trees_under_the_grid(pkg, ctx, oracle_mod):
    from pathplanning_amd import scenes

    raw = scenes.field512()
    starts, _, seeds = scenes.config3_queries(raw, 0, 4)
    n1, n2, eta = 1500, 300, 12.0
    b = _batch(pkg, raw, starts, seeds, n1 + n2, 0, eta, ctx=ctx)
    b.extend(n1)
    before = _trees(b)
    osc2, exp = _repair_checked(oracle_mod, b, before, scenes.field512_grid(), 0, 2)
    for q in (0, 1):
        r = exp[q]
        assert 1 < r["keep0"].sum() < r["kept"] < len(before[q][0]), (q, r["rounds"])
        assert r["reattached"] > 0 and r["failed_tops"] > 0, (q, r["rounds"])
    # the tree that shrinks to its root: its tops have one candidate (k is clipped to |K| = 1)
    r = exp[2]
    assert r["keep0"].sum() == 1 and len(before[2][0]) > 100
    assert r["rounds"][0]["tasks"] == r["rounds"][0]["tops"] > 0
    _continue_checked(oracle_mod, b, osc2, exp, seeds, n1, n2, 0, eta,
                      range(4))


# ---------------------------------------------------------------------------- 4. polygons
def test_polygons_with_an_added_ring(pkg, ctx, oracle_mod):
    """a square ring of half side 0.5 on the n/4-subtree node of each of the four trees in turn:
    a top inside the ring never attaches (every edge out of it crosses the ring's boundary)"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_polygons_open()
    starts = _starts(raw)
    for j in range(4):
        b = _batch(pkg, raw, starts, SEEDS, 400, 0, 0.0, ctx=ctx)
        b.extend(400)
        before = _trees(b)
        v = ref.quarter_subtree_node(before[j])
        ring = _square(before[j][0][v], before[j][1][v], 0.5)
        _, exp = _repair_checked(oracle_mod, b, before, _with_ring(raw, ring), 0, 2)
        r = exp[j]
        assert not r["keep"][v] and r["reattached"] > 0 and r["failed_tops"] > 0, r["rounds"]
        x, y = before[j][0], before[j][1]
        inside = (np.abs(x - x[v]) < 0.5) & (np.abs(y - y[v]) < 0.5)
        assert inside[v] and not r["keep"][inside].any()


def test_root_inside_a_polygon(pkg, ctx, oracle_mod):
    """the start inside obstacle polygon 5: the trees grow while that polygon is absent, then the
    full scene comes back — the blocked query re-attaches nothing and stays root-blocked; the
    free query beside it is repaired and goes on as its oracle run does"""
    from pathplanning_amd import scenes

    full = scenes.bench6_polygons_open()
    grow = dict(full)
    grow["obstacle_polygons"] = [o for i, o in enumerate(full["obstacle_polygons"]) if i != 5]
    inside = (10.0, 5.0, 0.3)
    starts = [inside, tuple(full["start"])]
    seeds = [7, 5]
    root = (np.array([inside[0]]), np.array([inside[1]]))
    assert revalidate_ref.root_ok(oracle_mod.OracleScene.from_raw(grow), root)
    assert not revalidate_ref.root_ok(oracle_mod.OracleScene.from_raw(full), root)
    b = _batch(pkg, grow, starts, seeds, 500, 0, 0.0, ctx=ctx)
    b.extend(400)
    before = _trees(b)
    assert len(before[0][0]) > 100
    osc2, exp = _repair_checked(oracle_mod, b, before, full, 0, 3)
    assert exp[0]["kept"] == 1 and exp[0]["rounds"] == [] and exp[1]["kept"] > 1
    rw0 = b.state()[3]
    _continue_checked(oracle_mod, b, osc2, exp, seeds, 400, 100, 0, 0.0, [1])
    n, it, _, rw = b.state()
    assert n[0] == 1 and it[0] == 500 and rw[0] == rw0[0]
    _assert_exact(b.tree(0, 1), [a[:1] for a in before[0]])


# -------------------------------------------------------- 5. more than two steer slices
def test_more_than_two_steer_slices(pkg, ctx, oracle_mod):
    """80 queries, six discs over the trees' extent: round 1 holds more than 2 * 32768 candidate
    tasks, in slices of 512 tops; every query is compared, one without a single top among them"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    Q, n1, n2 = 80, 400, 100
    starts, _, seeds = scenes.config3_queries(raw, 0, Q)
    b = _batch(pkg, raw, starts, seeds, n1 + n2, 0, 0.0, ctx=ctx)
    b.extend(n1)
    before = _trees(b)
    xs = np.concatenate([t[0] for t in before])
    ys = np.concatenate([t[1] for t in before])
    rng = np.random.default_rng(77)
    discs = []
    for _ in range(6):
        cx = rng.uniform(xs.min(), xs.max())
        cy = rng.uniform(ys.min(), ys.max())
        discs.append((cx, cy, rng.uniform(0.3, 0.8)))
    osc2, exp = _repair_checked(oracle_mod, b, before, ref.with_discs(raw, discs), 0, 2)
    first = [e["rounds"][0] if e["rounds"] else {"tops": 0, "tasks": 0} for e in exp]
    tops = np.array([d["tops"] for d in first])
    assert sum(d["tasks"] for d in first) > 2 * 32768
    assert tops.sum() > 2 * 512  # more than two slices of tops
    assert tops.min() == 0 < tops.max()
    assert sum(e["reattached"] for e in exp) > 0 and sum(e["failed_tops"] for e in exp) > 0
    # the queries that hold the tops at which the slices change (in node order), and one without
    cum = np.cumsum(tops)
    edge = [int(np.searchsorted(cum, t, side="right")) for t in (512, 1024)]
    none = int(np.flatnonzero(tops == 0)[0])
    _continue_checked(oracle_mod, b, osc2, exp, seeds, n1, n2, 0, 0.0,
                      sorted(set([0, Q - 1, none] + edge)))


# ----------------------------------------------------------------------- 6. errors
def test_errors_and_two_forests(pkg, oracle_mod):
    import ctypes as C

    from pathplanning_amd import _ffi, rrt, scenes

    L = _ffi.lib()
    raw = scenes.bench6_open()
    c = pkg.Context(0)
    null = (None,) * 5
    assert L.pp_star_repair(c.handle, 1, *null) == _ffi.PP_ERR_STATE  # no scene
    _space(raw)._upload(c)
    assert L.pp_star_repair(c.handle, 1, *null) == _ffi.PP_ERR_STATE  # no RRT* batch
    # an extend batch and an RRT* batch in one context
    starts, goals, seeds = scenes.config3_queries(raw, 0, 4)
    eb = rrt.RRTBatch(starts, goals, 300, raw["step_size"], _space(raw), seeds, ctx=c)
    eb.extend(200)
    n_eb = eb.state()[0]
    eb_before = [eb.tree(q, n_eb[q]) for q in range(4)]
    sb = _batch(pkg, raw, _starts(raw), SEEDS, 500, 0, 0.0, ctx=c)  # (its scene upload stales eb)
    sb.extend(400)
    sb_before, sb_state = _trees(sb), sb.state()
    for bad in (-1, 17):
        assert L.pp_star_repair(c.handle, bad, *null) == _ffi.PP_ERR_INVALID_ARGUMENT
        with pytest.raises(pkg.PPError):
            sb.repair(bad)
    for q, t in enumerate(_trees(sb)):
        _assert_exact(t, sb_before[q])
    # NULL outputs on the unchanged scene: accepted, nothing changes
    assert L.pp_star_repair(c.handle, 16, *null) == _ffi.PP_OK
    for q, t in enumerate(_trees(sb)):
        _assert_exact(t, sb_before[q])
    for s, e in zip(sb.state(), sb_state):
        assert np.array_equal(s, e)
    # a disc through the extend batch's first tree and the RRT* batch's first tree
    v = ref.quarter_subtree_node(sb_before[0])
    cnt = revalidate_ref.descendants(eb_before[0][3])
    w = 1 + int(np.argmin(np.abs(cnt[1:] - len(cnt) / 4.0)))
    raw2 = ref.with_discs(raw, [(sb_before[0][0][v], sb_before[0][1][v], 0.3),
                                (eb_before[0][0][w], eb_before[0][1][w], 0.3)])
    osc2 = oracle_mod.OracleScene.from_raw(raw2)
    _space(raw2)._upload(c)
    # NULL outputs on the changed scene, but for one counter
    rea = C.c_int64(-1)
    assert L.pp_star_repair(c.handle, 2, None, None, C.byref(rea), None, None) == _ffi.PP_OK
    exp = [rep.repair(osc2, t, 0, 2) for t in sb_before]
    assert rea.value == sum(e["reattached"] for e in exp) > 0
    sb_after = _trees(sb)
    for q in range(4):
        _assert_tree(q, sb_after[q], exp[q])
    # ... and left the extend batch's forest alone: its own call prunes the trees as they were
    n_new, new_index = eb.revalidate(n_eb)
    eexp = [revalidate_ref.revalidate(osc2, t) for t in eb_before]
    assert np.array_equal(n_new, [e["kept"] for e in eexp]) and eb.last_dropped > 0
    assert np.array_equal(new_index, np.concatenate([e["new_index"] for e in eexp]))
    for q in range(4):
        _assert_exact(eb.tree(q, n_new[q]), eexp[q]["tree"])
    # ... which in turn left the RRT* forest alone
    for q, t in enumerate(_trees(sb)):
        _assert_exact(t, sb_after[q])
    # a second call on the repaired trees is the identity
    n2, idx2 = sb.repair(3)
    assert sb.last_dropped == 0 and sb.last_reattached == 0 and sb.last_recovered == 0
    assert np.array_equal(idx2, np.concatenate([np.arange(n) for n in n2]))
    for q, t in enumerate(_trees(sb)):
        _assert_exact(t, sb_after[q])
    c.close()

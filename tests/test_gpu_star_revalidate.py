"""The RRT* batch's trees kept across a scene change: pp_star_revalidate (DESIGN.md §3.8 "RRT*
trees") against the CPU restatement tests/star_revalidate_ref.py (RRT*'s feasible edge with the
stored yaw, keep by walking chains that are not index-ordered, the stable compaction with the
costs).  The trees are grown on the GPU, exported, and restated on the CPU from the exported poses.

Exact: the kept set, new_index, n_nodes, last_dropped, coordinates, stored yaw, remapped parents,
and the cost bit-equal to the export before the call.  The continued runs against the oracle at
tests/test_gpu_rrtstar.py's tolerances (coordinates, parents and rewire deltas exact, yaw 1e-9,
cost 1e-9 relative).  Each case asserts its own conditions on the restatement (rewired nodes under
later parents that stay, orphans that hang under later parents, ...), so a scene that stops
exercising the case fails the test instead of passing vacuously."""
import numpy as np
import pytest

import revalidate_ref
import star_goal_ref
import star_revalidate_ref as ref
from star_tree_cases import (_assert_exact, _continue_checked, _set_space_checked, _space, _square,
                             _starts, _trees, _with_ring)
from test_gpu_rrtstar import _batch

pytestmark = pytest.mark.gpu

SEEDS = [0, 5, 11, 12]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. the unchanged scene
@pytest.mark.parametrize("k,eta", [(0, 0.0), (0, 2.0)])
def test_unchanged_scene_is_the_identity(pkg, ctx, k, eta):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts = _starts(raw)
    n1, n2 = 250, 150
    a = _batch(pkg, raw, starts, SEEDS, 400, k, eta, ctx=ctx)
    a.extend(n1 + n2)
    whole, whole_state = _trees(a), a.state()
    for t in whole:  # rewired nodes hang under later nodes
        assert (t[3][1:] > np.arange(1, len(t[3]))).sum() >= 10
    n_new, new_index = a.revalidate()
    assert np.array_equal(n_new, whole_state[0]) and a.last_dropped == 0
    assert np.array_equal(new_index, np.concatenate([np.arange(n) for n in n_new]))
    for q, t in enumerate(_trees(a)):
        _assert_exact(t, whole[q])
    for s, e in zip(a.state(), whole_state):
        assert np.array_equal(s, e)
    # ... and between two extends it changes nothing, rewires included
    b = _batch(pkg, raw, starts, SEEDS, 400, k, eta, ctx=ctx)
    b.extend(n1)
    n_mid = b.state()[0]
    n_new, new_index = b.set_space(_space(raw))
    assert np.array_equal(n_new, n_mid) and b.last_dropped == 0
    assert np.array_equal(new_index, np.concatenate([np.arange(n) for n in n_mid]))
    b.extend(n2)
    for q, t in enumerate(_trees(b)):
        _assert_exact(t, whole[q])
    for s, e in zip(b.state(), whole_state):
        assert np.array_equal(s, e)


# ------------------------------------------------------- 2. one disc, and what follows
@pytest.mark.parametrize("k,eta", [(0, 0.0), (0, 2.0)])
def test_one_disc_then_continue(pkg, ctx, oracle_mod, k, eta):
    """a disc of r 0.3 on the n/4-subtree node of each of the four trees in turn"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts = _starts(raw)
    n1, n2 = 400, 300
    goal = raw["goal"]
    for j in range(4):
        b = _batch(pkg, raw, starts, SEEDS, n1 + n2, k, eta, ctx=ctx)
        b.extend(n1)
        before = _trees(b)
        v = ref.quarter_subtree_node(before[j])
        raw2 = ref.with_discs(raw, [(before[j][0][v], before[j][1][v], 0.3)])
        osc2, exp = _set_space_checked(oracle_mod, b, before, raw2)
        r = exp[j]
        assert not r["keep"][v] and 1 < r["kept"] < len(before[j][0]), r
        assert r["failed"] > 0 and r["orphans"] > 0, r
        assert r["kept_back"] > 0 and r["orphans_via_later"] > 0, r
        _continue_checked(oracle_mod, b, osc2, exp, SEEDS, n1, n2, k, eta, range(4))
        # the goal connection on the pruned-and-extended trees, in the new scene
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


# ------------------------------------------------------------------------------ 3. the grid
def test_field512_trees_under_the_grid(pkg, ctx, oracle_mod):
    from pathplanning_amd import scenes

    raw = scenes.field512()
    starts, _, seeds = scenes.config3_queries(raw, 0, 4)
    n1, n2, eta = 1500, 300, 12.0
    b = _batch(pkg, raw, starts, seeds, n1 + n2, 0, eta, ctx=ctx)
    b.extend(n1)
    before = _trees(b)
    osc2, exp = _set_space_checked(oracle_mod, b, before, scenes.field512_grid())
    for q in (0, 1):
        r = exp[q]
        assert 1 < r["kept"] < len(before[q][0]), (q, r)
        assert r["kept_back"] > 0 and r["orphans_via_later"] > 0, (q, r)
    assert exp[2]["kept"] == 1 and len(before[2][0]) > 100  # only its root stays
    _continue_checked(oracle_mod, b, osc2, exp, seeds, n1, n2, 0, eta,
                      range(4))


# ---------------------------------------------------------------------------- 4. polygons
def test_polygons_with_an_added_ring(pkg, ctx, oracle_mod):
    """a square ring of half side 0.5 on the n/4-subtree node of each of the four trees in turn"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_polygons_open()
    starts = _starts(raw)
    for j in range(4):
        b = _batch(pkg, raw, starts, SEEDS, 400, 0, 0.0, ctx=ctx)
        b.extend(400)
        before = _trees(b)
        v = ref.quarter_subtree_node(before[j])
        raw2 = _with_ring(raw, _square(before[j][0][v], before[j][1][v], 0.5))
        _, exp = _set_space_checked(oracle_mod, b, before, raw2)
        r = exp[j]
        assert not r["keep"][v] and 1 < r["kept"] < len(before[j][0]), r
        assert r["orphans"] > 0 and r["kept_back"] > 0 and r["orphans_via_later"] > 0, r


# ------------------------------------------------------------------------ 5. a blocked root
def test_root_inside_a_polygon(pkg, ctx, oracle_mod):
    """the start inside obstacle polygon 5: the trees grow while that polygon is absent, then the
    full scene comes back — only the root stays, the query is root-blocked and never inserts or
    rewires again; the free query beside it goes on as its oracle run does"""
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
    par = before[0][3]
    assert len(par) > 100 and (par[1:] > np.arange(1, len(par))).sum() > 10
    osc2, exp = _set_space_checked(oracle_mod, b, before, full)
    assert exp[0]["kept"] == 1 and exp[1]["kept"] > 1
    rw0 = b.state()[3]
    _continue_checked(oracle_mod, b, osc2, exp, seeds, 400, 100, 0, 0.0, [1])
    n, it, _, rw = b.state()
    assert n[0] == 1 and it[0] == 500 and rw[0] == rw0[0]
    _assert_exact(b.tree(0, 1), [a[:1] for a in before[0]])


# --------------------------------- 6. more than one steer slice and more than one sub-batch
def test_three_slices_two_sub_batches(pkg, ctx, oracle_mod):
    """320 queries (two sub-batches on two streams) holding more than 2 * 32768 + 1024 nodes
    (three slices of steer tasks, several scan workgroups), six discs over the trees' extent"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    Q, n1, n2 = 320, 400, 100
    starts, _, seeds = scenes.config3_queries(raw, 0, Q)
    b = _batch(pkg, raw, starts, seeds, n1 + n2, 0, 0.0, ctx=ctx)
    b.extend(n1)
    before = _trees(b)
    n_old = np.array([len(t[0]) for t in before])
    off = np.concatenate([[0], np.cumsum(n_old)])
    assert off[-1] > 2 * 32768 + 1024
    xs = np.concatenate([t[0] for t in before])
    ys = np.concatenate([t[1] for t in before])
    rng = np.random.default_rng(77)
    discs = []
    for _ in range(6):
        cx = rng.uniform(xs.min(), xs.max())
        cy = rng.uniform(ys.min(), ys.max())
        discs.append((cx, cy, rng.uniform(0.3, 0.8)))
    osc2, exp = _set_space_checked(oracle_mod, b, before, ref.with_discs(raw, discs))
    # the queries that hold the global nodes at which the steer slices change
    straddle = [int(np.searchsorted(off, g, side="right") - 1) for g in (32768, 65536)]
    for q, g in zip(straddle, (32768, 65536)):
        assert off[q] <= g < off[q + 1]
    for q in [0, Q - 1] + straddle:
        assert exp[q]["failed"] > 0, q
    dropped = n_old - np.array([e["kept"] for e in exp])
    assert dropped.min() == 0 < dropped.max()
    assert sum(e["orphans"] for e in exp) > 0 and sum(e["kept_back"] for e in exp) > 0
    assert sum(e["orphans_via_later"] for e in exp) > 0
    _continue_checked(oracle_mod, b, osc2, exp, seeds, n1, n2, 0, 0.0,
                      [0, 159, 160, Q - 1] + straddle)


# ----------------------------------------------------------------------- 7. state errors
def test_state_errors_and_two_forests(pkg, oracle_mod):
    import ctypes as C

    from pathplanning_amd import _ffi, rrt, scenes

    L = _ffi.lib()
    raw = scenes.bench6_open()
    c = pkg.Context(0)
    assert L.pp_star_revalidate(c.handle, None, None, None) == _ffi.PP_ERR_STATE  # no scene
    _space(raw)._upload(c)
    assert L.pp_star_revalidate(c.handle, None, None, None) == _ffi.PP_ERR_STATE  # no RRT* batch
    # an extend batch and an RRT* batch in one context
    starts, goals, seeds = scenes.config3_queries(raw, 0, 4)
    eb = rrt.RRTBatch(starts, goals, 300, raw["step_size"], _space(raw), seeds, ctx=c)
    eb.extend(200)
    n_eb = eb.state()[0]
    eb_before = [eb.tree(q, n_eb[q]) for q in range(4)]
    sb = _batch(pkg, raw, _starts(raw), SEEDS, 500, 0, 0.0, ctx=c)  # (its scene upload stales eb)
    it = C.c_int64(0)
    assert L.pp_batch_extend(c.handle, 1, C.byref(it), None) == _ffi.PP_ERR_STATE
    sb.extend(400)
    sb_before = _trees(sb)
    # NULL outputs on the unchanged scene: accepted, nothing changes
    assert L.pp_star_revalidate(c.handle, None, None, None) == _ffi.PP_OK
    for q, t in enumerate(_trees(sb)):
        _assert_exact(t, sb_before[q])
    # a disc through the extend batch's first tree and the RRT* batch's first tree
    v = ref.quarter_subtree_node(sb_before[0])
    cnt = revalidate_ref.descendants(eb_before[0][3])
    w = 1 + int(np.argmin(np.abs(cnt[1:] - len(cnt) / 4.0)))
    raw2 = ref.with_discs(raw, [(sb_before[0][0][v], sb_before[0][1][v], 0.3),
                                (eb_before[0][0][w], eb_before[0][1][w], 0.3)])
    osc2 = oracle_mod.OracleScene.from_raw(raw2)
    _space(raw2)._upload(c)
    # a scene call does not stop the RRT* batch (its trees are unverified until the call)
    dropped = C.c_int64(-1)
    assert L.pp_star_revalidate(c.handle, None, C.byref(dropped), None) == _ffi.PP_OK
    exp = [ref.revalidate(osc2, t) for t in sb_before]
    assert dropped.value == sum(len(t[0]) - e["kept"] for t, e in zip(sb_before, exp)) > 0
    sb_after = _trees(sb)
    for q in range(4):
        _assert_exact(sb_after[q], exp[q]["tree"])
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
    # a second call on the pruned trees is the identity
    n2, idx2 = sb.revalidate()
    assert sb.last_dropped == 0 and np.array_equal(idx2, np.concatenate([np.arange(n) for n in n2]))
    c.close()

"""GPU: committing chain shortcuts into the RRT* trees (pp_star_shortcut_commit, DESIGN.md §3.7
"Committing shortcuts") against the CPU restatement tests/star_shortcut_commit_ref.py.

Exactness: the restatement run over the device's own band (shortcut_edges) and the tree exported
before the call must give the tree exported after it BIT FOR BIT — parent, edge_cost, cost, the
outputs, n_changed and the rewire counters; everything else of the state must not move.  Against
the all-CPU restatement (the oracle's band): COST_RTOL = 1e-9 relative, the standing tolerance of
tests/test_gpu_star_shortcut.py (ocml against glibc trig inside the Dubins cost), and the same
rewire list wherever the restatement's runner-up at every DP row, the stored edge's `cur` included,
is more than GAP = 1e-6 relative away."""
import ctypes as C

import numpy as np
import pytest

import star_goal_ref as goal_ref
import star_shortcut_commit_ref as ref
import star_shortcut_ref as sref
from test_gpu_rrtstar import _batch

pytestmark = pytest.mark.gpu

COST_RTOL = 1e-9
GAP = 1e-6
ROWS = ("x", "y", "yaw", "parent", "cost", "edge_cost")
KEPT = ("off", "x", "y", "yaw", "iterations", "seeds", "node_evals", "focus_xy", "focus_bound",
        "skipped")


def _tree(st, q):
    """((x, y, yaw, parent, cost), edge_cost) of slot q of an exported state"""
    s = slice(int(st["off"][q]), int(st["off"][q + 1]))
    return tuple(st[k][s] for k in ("x", "y", "yaw", "parent", "cost")), st["edge_cost"][s]


def _same(a, b, keys=None):
    return all(np.array_equal(a[k], b[k]) for k in (keys or a.keys()))


def _pairs(D, span):
    return sum(min(span, D - i) for i in range(D))


def _commit(b, goals, nodes, span):
    """One shortcut_commit call with everything the checks need taken around it: the state before
    and after, the device's own band of every served query, shortcut()'s costs before the call,
    and the restatement over that band and that tree (``exp``, None for a skipped query)."""
    goals = np.asarray(goals, dtype=np.float64).reshape(b.q, 3)
    nodes = np.asarray(nodes, dtype=np.int32)
    st0, fx0, cnt0 = b.export_forest(), b.focus_state(), b.state()
    bands = [b.shortcut_edges(q, goals[q], int(nodes[q]), span) if nodes[q] >= 0 else None
             for q in range(b.q)]
    short = b.shortcut(goals, nodes, span)
    assert _same(st0, b.export_forest())  # (neither of the two writes a tree)
    node, cost, nrw = b.shortcut_commit(goals, nodes, span)
    run = dict(b=b, goals=goals, nodes=nodes, span=span, st0=st0, st1=b.export_forest(),
               fx0=fx0, fx1=b.focus_state(), cnt0=cnt0, cnt1=b.state(), bands=bands, short=short,
               node=node, cost=cost, nrw=nrw, n_tested=b.n_tested, n_changed=b.n_changed, exp=[])
    for q in range(b.q):
        if nodes[q] < 0:
            run["exp"].append(None)
            continue
        tree, el = _tree(st0, q)
        run["exp"].append(ref.commit(tree, el, bands[q][0], bands[q][1], span))
    return run


def _expected_state(run):
    """the state the restatement says the call leaves: st0 with the new parents, edge costs, costs
    and rewire counters"""
    st = {k: np.array(v, copy=True) for k, v in run["st0"].items()}
    for q, e in enumerate(run["exp"]):
        if e is None:
            continue
        s = slice(int(st["off"][q]), int(st["off"][q + 1]))
        st["parent"][s], st["edge_cost"][s], st["cost"][s] = e["parent"], e["edge_cost"], e["cost"]
        st["rewires"][q] += e["n_rewired"]
    return st


def _check_exact(run):
    """(1) the call against the restatement over the device's band, bit for bit"""
    st0, st1, want = run["st0"], run["st1"], _expected_state(run)
    for k in ("parent", "edge_cost", "cost", "rewires"):
        assert np.array_equal(st1[k], want[k]), k
    assert np.array_equal(st1["cost"].view(np.uint64), want["cost"].view(np.uint64))
    assert np.array_equal(st1["edge_cost"].view(np.uint64), want["edge_cost"].view(np.uint64))
    assert _same(st0, st1, KEPT)
    assert all(np.array_equal(a, c) for a, c in zip(run["fx0"], run["fx1"]))
    for i in (0, 1, 2):  # tree sizes, iterations, node_evals
        assert np.array_equal(run["cnt0"][i], run["cnt1"][i])
    assert np.array_equal(run["cnt1"][3], want["rewires"])
    changed, tested = 0, 0
    for q, e in enumerate(run["exp"]):
        if e is None:  # a skipped query: -1, inf, 0 and its rows as they were
            assert run["node"][q] == -1 and run["cost"][q] == np.inf and run["nrw"][q] == 0
            s = slice(int(st0["off"][q]), int(st0["off"][q + 1]))
            assert all(np.array_equal(st0[k][s], st1[k][s]) for k in ROWS)
            continue
        assert run["node"][q] == e["node"] and run["nrw"][q] == e["n_rewired"], q
        assert run["cost"][q] == e["cost_out"], (q, run["cost"][q], e["cost_out"])
        assert np.all(e["cost"] <= _tree(st0, q)[0][4])  # no cost rises
        changed += e["n_changed"]
        tested += _pairs(len(run["bands"][q][0]), run["span"])
    assert run["n_changed"] == changed and run["n_tested"] == tested
    assert changed == int(np.count_nonzero(st1["cost"] != st0["cost"]))


def _grow(pkg, ctx, raw, starts, seeds, n_iter, k, eta, max_iter=None):
    b = _batch(pkg, raw, starts, seeds, max_iter or n_iter, k, eta, ctx=ctx)
    b.extend(n_iter)
    return b


def _single_specs():
    """the three rewiring cases of the CPU file, then the occupancy grid and the polygons (300
    iterations, near_goal, span 6: star_shortcut_ref.golden_specs)"""
    from pathplanning_amd import scenes

    out = ref.specs()[:3]
    for name, eta in (("field512_grid", 10.0), ("bench6_polygons_open", 0.5)):
        r = getattr(scenes, name)()
        out.append(dict(scene=name, start=list(r["start"]), seed=3, n_iter=300, k=0, eta=eta,
                        goal=None, span=6))
    return out


@pytest.fixture(scope="module")
def runs(pkg, oracle_mod):
    """every single-query case grown and committed once, each in a context of its own so that its
    batch stays alive for the tests that go on from the committed tree"""
    out, ctxs = [], []
    for spec in _single_specs():
        raw = goal_ref.scene(spec["scene"])
        osc = oracle_mod.OracleScene.from_raw(raw)
        c = pkg.Context(0)
        ctxs.append(c)
        # (room for test_continues' 200 further iterations; the capacity plays no part in a run)
        b = _grow(pkg, c, raw, [spec["start"]], [spec["seed"]], spec["n_iter"], spec["k"],
                  spec["eta"], max_iter=spec["n_iter"] + 200)
        tree = b.tree(0)
        goal = spec["goal"] if spec["goal"] is not None else sref.near_goal(tree)
        node = sref.deepest_reaching_node(osc, tree, goal)
        assert node >= 0
        plan0 = b.plan(goal)
        run = _commit(b, [goal], [node], spec["span"])
        run.update(spec=spec, raw=raw, osc=osc, plan0=plan0)
        out.append(run)
    yield out
    for c in ctxs:
        c.close()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def test_exact_single_queries(runs):
    """(1) the three rewiring cases, the grid and the polygons, bit for bit"""
    rewires = []
    for run in runs:
        _check_exact(run)
        rewires.append(len(run["exp"][0]["rewired"]))
    assert rewires[:3] == [6, 2, 4], rewires  # the CPU file's cases rewire as they do there
    e = runs[0]["exp"][0]
    assert [list(p) for p in e["rewired"]] == [[8, 10], [7, 10], [4, 6], [3, 6], [2, 6], [1, 5]]
    assert runs[0]["nodes"][0] == 108 and e["n_changed"] == 45


def test_exact_mixed_batch(pkg, oracle_mod, ctx):
    """(1) four queries on config5_field in one call: one that rewires, a no-op, a skipped one
    (node -1) and one whose goal no node reaches (the centre of a disc)"""
    from pathplanning_amd import scenes

    raw = scenes.config5_field()
    osc = oracle_mod.OracleScene.from_raw(raw)
    starts, _, seeds = scenes.config3_queries(raw, 0, 4)
    b = _grow(pkg, ctx, raw, starts, seeds, 300, 0, scenes.CONFIG5_ETA)
    trees = [b.tree(q) for q in range(4)]
    # (query 1 is the CPU file's case 2, query 0 its first no-op)
    goals = np.array([sref.near_goal(trees[0]), sref.near_goal(trees[1]), sref.near_goal(trees[2]),
                      (raw["circles"][0][0], raw["circles"][0][1], 0.5)])
    nodes = np.full(4, -1, dtype=np.int32)
    for q in (0, 1):
        nodes[q] = sref.deepest_reaching_node(osc, trees[q], goals[q])
    nodes[3] = len(trees[3][0]) - 1
    assert nodes[0] >= 0 and nodes[1] >= 0
    run = _commit(b, goals, nodes, 8)
    _check_exact(run)
    e = run["exp"]
    assert len(e[1]["rewired"]) >= 1 and e[1]["n_changed"] > len(e[1]["rewired"])
    assert not e[0]["rewired"] and e[0]["n_changed"] == 0 and run["node"][0] >= 0
    assert e[2] is None
    assert e[3]["node"] == -1 and run["node"][3] == -1 and run["cost"][3] == np.inf
    assert run["nrw"][3] == 0 and not np.isfinite(run["bands"][3][1][0]).any()


def test_exact_sub_batches(pkg, ctx):
    """(1) 300 queries (the extend runs >= 256 as sub-batches on streams of their own): every
    query of one call, bit for bit"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 300)
    b = _grow(pkg, ctx, raw, starts, seeds, 80, 0, 1.0)
    node, _ = b.plan(goals)
    assert (node >= 0).sum() > 30
    run = _commit(b, goals, node, 8)
    _check_exact(run)
    assert run["nrw"].sum() > 0  # (the call is not a no-op)


def test_against_the_oracles_band(runs):
    """(2) the all-CPU restatement (the oracle's band over the exported tree): cost_out within
    COST_RTOL, the same rewire list where no DP row is a near-tie, and shortcut()'s cost"""
    compared = 0
    for run in runs:
        tree, el = _tree(run["st0"], 0)
        goal, node = run["goals"][0], int(run["nodes"][0])
        ora, cnode, w, pairs = ref.commit_oracle(run["osc"], tree, el, goal, node, run["span"])
        assert np.array_equal(cnode, run["bands"][0][0]) and pairs == run["n_tested"]
        print(run["spec"]["scene"], "cost_out", repr(float(run["cost"][0])), "oracle band",
              repr(ora["cost_out"]), "gap", ora["gap"], "rewired", run["exp"][0]["rewired"])
        assert abs(run["cost"][0] - ora["cost_out"]) <= COST_RTOL * ora["cost_out"]
        if ora["gap"] > GAP:
            assert run["exp"][0]["rewired"] == ora["rewired"]
            assert run["node"][0] == ora["node"] and run["nrw"][0] == ora["n_rewired"]
            compared += 1
        short_cost = run["short"][2][0]
        assert run["short"][3][0]
        assert abs(run["cost"][0] - short_cost) <= COST_RTOL * short_cost
    assert compared >= 3


def test_committed_tree_is_a_valid_forest(pkg, runs):
    """(3) the export imports into a second batch (cost == cost[parent] + edge_cost bit for bit,
    every chain ends in the root), revalidate drops nothing, plan is no worse than cost_out or
    the plan before, and the tree chain from node_out has cost_out's length"""
    for run in runs:
        b, spec, goal = run["b"], run["spec"], run["goals"][0]
        c2 = pkg.Context(0)
        try:
            b2 = _batch(pkg, run["raw"], [spec["start"]], [spec["seed"]], spec["n_iter"] + 200,
                        spec["k"], spec["eta"], ctx=c2)
            b2.import_forest(run["st1"])
            assert _same(run["st1"], b2.export_forest())
        finally:
            c2.close()
        n, _ = b.revalidate()
        assert b.last_dropped == 0 and n[0] == run["cnt0"][0][0]
        assert _same(run["st1"], b.export_forest())
        _, cost = b.plan(goal)
        assert cost[0] <= run["cost"][0] and cost[0] <= run["plan0"][1][0]
        if run is runs[0]:  # (31.80 -> 31.35 on the oracle's tree)
            assert cost[0] < run["plan0"][1][0]
        _, _, length, ok = b.path_segments(goal, run["node"])
        R = run["osc"].turn_radius
        assert ok[0] and abs(length[0] / R - run["cost"][0]) <= 1e-9 * run["cost"][0]
        # the chain from node_out is shortcut()'s row, taken before the commit
        off, chain = run["short"][0], run["short"][1]
        assert sref.chain_nodes(_tree(run["st1"], 0)[0], int(run["node"][0])) \
            == [int(v) for v in chain[off[0]:off[1]]]


def test_continues_like_an_imported_copy(pkg, runs, ctx):
    """(4) commit then extend(200) == import the restatement's expected state into a fresh batch,
    then extend(200): the exports are equal bit for bit, rewires and node_evals included (the
    forest guarantee of DESIGN.md §3.9; pins the mark / stamp scratch)"""
    run = runs[0]
    spec = run["spec"]
    a = _grow(pkg, ctx, run["raw"], [spec["start"]], [spec["seed"]], spec["n_iter"], spec["k"],
              spec["eta"], max_iter=spec["n_iter"] + 200)
    assert _same(run["st0"], a.export_forest())
    a.shortcut_commit(run["goals"], run["nodes"], run["span"])
    a.extend(200)
    got = a.export_forest()
    b = _batch(pkg, run["raw"], [spec["start"]], [spec["seed"]], spec["n_iter"] + 200, spec["k"],
               spec["eta"], ctx=ctx)
    b.import_forest(_expected_state(run))
    b.extend(200)
    want = b.export_forest()
    assert got["iterations"][0] == spec["n_iter"] + 200
    assert got["rewires"][0] > run["st1"]["rewires"][0]  # the extend rewired on the committed tree
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["cost"].view(np.uint64), want["cost"].view(np.uint64))


def test_span_one_changes_nothing(pkg, oracle_mod, ctx):
    """(5) span 1 on an unchanged scene: 0 rewires, the export bit-identical, cost_out ==
    shortcut(span=1)'s cost"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts = [raw["start"], (-4.0, -4.5, 0.3), (-3.0, -3.0, 0.785)]
    b = _grow(pkg, ctx, raw, starts, [0, 5, 11], 300, 0, 1.0)
    node, _ = b.plan(raw["goal"])
    assert (node >= 0).any()
    st0 = b.export_forest()
    _, _, scost, ok = b.shortcut(raw["goal"], node, 1)
    n1, c1, nrw = b.shortcut_commit(raw["goal"], node, 1)
    assert _same(st0, b.export_forest())
    assert np.array_equal(nrw, np.zeros(3, dtype=np.int32)) and b.n_changed == 0
    assert np.array_equal(n1, node) and np.array_equal(c1, scost) and np.array_equal(ok, node >= 0)


def test_scene_change_without_revalidate(pkg, oracle_mod, ctx):
    """(6) a disc across a middle edge of case 1's chain, uploaded without revalidate: exact
    against the restatement over the device's band; the blocked node keeps its stored edge (no
    cheaper feasible one exists), others still rewire, no cost rises"""
    from pathplanning_amd import rrt

    spec = ref.specs()[0]
    raw = goal_ref.scene(spec["scene"])
    osc = oracle_mod.OracleScene.from_raw(raw)
    b = _grow(pkg, ctx, raw, [spec["start"]], [spec["seed"]], spec["n_iter"], spec["k"],
              spec["eta"])
    tree = b.tree(0)
    goal = spec["goal"]
    node = sref.deepest_reaching_node(osc, tree, goal)
    cnode, ps = sref.poses(tree, goal, node)
    i = 5  # the edge position 5 -> 6 of a chain of 10: the midpoint of its Dubins curve
    assert len(cnode) == 10
    d = oracle_mod.dubins(*ps[i], *ps[i + 1], osc.turn_radius, osc.step_size)
    mid = len(d[0]) // 2
    raw2 = dict(raw)
    raw2["circles"] = np.vstack([raw["circles"], [[d[0][mid], d[1][mid], 0.2]]])
    rrt.Space.from_raw(raw2)._upload(b.ctx)  # (no revalidate: the tree is stale)
    run = _commit(b, [goal], [node], spec["span"])
    _check_exact(run)
    e, (_, w) = run["exp"][0], run["bands"][0]
    own_blocked = [p for p in range(1, len(cnode)) if not np.isfinite(w[p, 0])]
    assert i in own_blocked
    assert len(e["rewired"]) >= 1
    el0 = _tree(run["st0"], 0)[1]
    kept = [p for p in own_blocked if p not in {a for a, _ in e["rewired"]}]
    assert i in kept  # nothing feasible is cheaper: the stored edge stays, unverified
    for p in kept:
        m = cnode[p - 1]
        assert _tree(run["st1"], 0)[1][m] == el0[m] and _tree(run["st1"], 0)[0][3][m] == cnode[p]
    assert np.all(_tree(run["st1"], 0)[0][4] <= _tree(run["st0"], 0)[0][4])
    # the all-CPU restatement in the new scene agrees on what is blocked and what is rewired
    osc2 = oracle_mod.OracleScene.from_raw(raw2)
    ora, _, w2, _ = ref.commit_oracle(osc2, *_tree(run["st0"], 0), goal, node, spec["span"])
    assert np.array_equal(np.isfinite(w), np.isfinite(w2))
    if ora["gap"] > GAP:
        assert ora["rewired"] == e["rewired"]


def test_refused_calls_change_nothing(pkg, ctx):
    """(7) argument and state errors before any launch; the export is the same afterwards"""
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.bench6_open()
    L = _ffi.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    b = _grow(pkg, ctx, raw, [raw["start"]], [5], 200, 0, 1.0)
    best, _ = b.plan(raw["goal"])
    assert best[0] >= 0
    st0 = b.export_forest()
    g = np.array(raw["goal"], dtype=np.float64)
    n = int(b.state()[0][0])

    def call(h=ctx.handle, goals=g, nodes=best, span=8):
        return L.pp_star_shortcut_commit(
            h, None if goals is None else goals.ctypes.data_as(dp),
            None if nodes is None else nodes.ctypes.data_as(ip), span, None, None, None, None,
            None)

    for kw in (dict(span=0), dict(span=64), dict(nodes=np.array([n], dtype=np.int32)),
               dict(nodes=np.array([-2], dtype=np.int32)), dict(goals=None), dict(nodes=None),
               dict(goals=np.array([np.nan, 0.0, 0.0]))):
        assert call(**kw) == _ffi.PP_ERR_INVALID_ARGUMENT, kw
        assert _same(st0, b.export_forest()), kw
    c2 = pkg.Context(0)
    try:
        assert call(h=c2.handle) == _ffi.PP_ERR_STATE  # no scene
        rrt.Space.from_raw(raw)._upload(c2)
        assert call(h=c2.handle) == _ffi.PP_ERR_STATE  # a scene, no RRT* batch
    finally:
        c2.close()
    assert _same(st0, b.export_forest())
    with pytest.raises(_ffi.PPError):
        b.shortcut_commit(raw["goal"], best, 0)
    assert call() == _ffi.PP_OK  # every output NULL: the commit still happens
    assert np.all(b.export_forest()["cost"] <= st0["cost"])


def test_plan_commit_focus_prune(pkg, ctx):
    """(8) plan(goals, focus=True, prune=True, commit=8): the nodes index the pruned trees, their
    plan total is the returned cost bit for bit, the focus bound is cost * R and the protected
    chain survives — against the same steps taken one by one on a twin batch"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts = [raw["start"], (-4.0, -4.5, 0.3), (-3.0, -3.0, 0.785)]
    goal = raw["goal"]

    twin = _grow(pkg, ctx, raw, starts, [0, 5, 11], 300, 0, 1.0)
    n0, c0 = twin.plan(goal)
    n1, c1, _ = twin.shortcut_commit(goal, n0, 8)
    chains = []
    for q in range(3):
        t = twin.tree(q)
        chains.append([(t[0][m], t[1][m], t[2][m], t[4][m])
                       for m in sref.chain_nodes(t, n1[q])] if n1[q] >= 0 else [])
    assert (n1 >= 0).any() and np.all(c1 <= c0)

    b = _grow(pkg, ctx, raw, starts, [0, 5, 11], 300, 0, 1.0)
    sizes0 = b.state()[0].copy()
    node, cost = b.plan(goal, focus=True, prune=True, commit=8)
    assert np.array_equal(cost, c1) and np.array_equal(node >= 0, n1 >= 0)
    sizes = b.state()[0]
    assert np.all(sizes <= sizes0) and b.last_dropped == int((sizes0 - sizes).sum())
    R = float(b.space.get_steer())
    _, bound, _ = b.focus_state()
    for q in range(3):
        if node[q] < 0:
            assert bound[q] == np.inf
            continue
        assert 0 <= node[q] < sizes[q]
        assert b.goal_costs(q, goal)[node[q]] == cost[q]
        assert bound[q] == cost[q] * np.float64(R)
        t = b.tree(q)
        assert [(t[0][m], t[1][m], t[2][m], t[4][m])
                for m in sref.chain_nodes(t, node[q])] == chains[q]
    pn, pc = b.plan(goal)
    assert np.all(pc <= cost)

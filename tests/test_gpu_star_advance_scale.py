"""pp_star_advance at batch scale (DESIGN.md §4 "Advance at batch scale; the loop, turn by turn"):
more than one block of queries, round-1 tops packed across blocks into several slices, trees that
straddle the 1024-node scan workgroups, sub-batches on their own streams and more queries than
advance_cost_kernel has waves.

The exactness rule is tests/test_gpu_star_advance.py's, through its _advance_checked: the
restatement tests/star_advance_ref.py is fed the device's own state exported just before the call;
n_nodes, new_index, the three counters, poses, parents and the costs and edge costs of K0 are
compared with ==, the costs of recovered nodes at COST_RTOL, and a parent mismatch prints
adv.min_gap.

The batch: bench6_open, scenes.config3_queries(raw, 0, 320), k = 0, eta = 0, 100 iterations in
rows of 200.  An RRT* batch of 256 queries or more runs as three sub-batches of consecutive
queries (Forest::q_begin: query Q * s / 3 opens sub-batch s)."""
import time

import numpy as np
import pytest

import forest_state_ref
import star_advance_ref as adv
import star_focus_ref
import star_revalidate_ref as ref
from star_tree_cases import _continue_checked, _space, _square, _with_ring
from test_gpu_rrtstar import _assert_same, _batch
from test_gpu_star_advance import _advance_checked

pytestmark = pytest.mark.gpu

Q, N_ITER, MAX_ITER = 320, 100, 199
SLICE, SCAN = 512, 1024  # kRepairTopsPerSlice, kRvScan


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _splits(q):
    """the first query of sub-batches 1 and 2"""
    return [q * s // 3 for s in (1, 2)]


def _grow(pkg, ctx, oracle_mod):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, Q)
    b = _batch(pkg, raw, starts, seeds, MAX_ITER, 0, 0.0, ctx=ctx)
    b.extend(N_ITER)
    return b, raw, oracle_mod.OracleScene.from_raw(raw), starts, goals, seeds


def _depths(st):
    """every node's edges to its root over a packed forest, by pointer jumps"""
    off, par = st["off"], st["parent"].astype(np.int64)
    n = off[1:] - off[:-1]
    tree = np.repeat(np.arange(len(n)), n)
    up = np.where(par >= 0, off[tree] + par, np.arange(len(par)))  # a root points at itself
    d = np.zeros(len(par), dtype=np.int64)
    v = np.arange(len(par))
    for _ in range(int(n.max())):
        d += par[v] >= 0
        v = up[v]
    assert (par[v] < 0).all()
    return d, tree, up


def _deepest(st):
    """per tree its deepest node (the first in index order), -1 for a one-node tree"""
    d, tree, _ = _depths(st)
    off = st["off"]
    top = np.maximum.reduceat(d, off[:-1])
    cand = np.flatnonzero(d == top[tree])
    _, first = np.unique(tree[cand], return_index=True)
    node = (cand[first] - off[:-1]).astype(np.int32)
    return np.where(top > 0, node, -1).astype(np.int32), top


def _round_tops(exp, rnd):
    return [e["rounds"][rnd - 1]["tops"] if len(e["rounds"]) >= rnd else 0 for e in exp]


def _straddled(off):
    """the multiples of the scan workgroup that fall strictly inside a tree"""
    inside = 0
    for m in range(SCAN, int(off[-1]), SCAN):
        q = int(np.searchsorted(off, m, side="right")) - 1
        inside += off[q] < m < off[q + 1]
    return inside


def _check_one_hop(st0, st1, nodes):
    """advance(nodes, hops=1, rounds=0) from forest st0 to forest st1, over all queries at once:
    row 0 is the chosen node with parent -1 and cost 0, the kept nodes are the chosen node's
    subtree, they follow row 0 in their old order with their poses and edge costs, and every tree
    is valid with its stored costs equal to their rebuild.  Returns the queries that moved."""
    off0, off1 = st0["off"], st1["off"]
    d, tree, up = _depths(st0)
    idx = np.arange(len(d))
    # the chosen node: one hop from the root on the chain to nodes[q]
    r = np.where(nodes >= 0, off0[:-1] + nodes, off0[:-1])
    for _ in range(int(d.max())):
        r = np.where(d[r] > 1, up[r], r)
    moved = d[r] == 1
    assert np.array_equal(moved, (nodes > 0))
    for key in ("x", "y", "yaw"):
        assert np.array_equal(st1[key][off1[:-1]], st0[key][r]), key
    assert (st1["parent"][off1[:-1]] == -1).all() and (st1["cost"][off1[:-1]] == 0.0).all()
    assert (st1["edge_cost"][off1[:-1]] == 0.0).all()
    # K0 by the definition on the old forest: the chosen node lies on the node's chain
    v, keep = idx, idx == r[tree]
    for _ in range(int(d.max())):
        v = up[v]
        keep = keep | (v == r[tree])
    assert np.array_equal(np.add.reduceat(keep.astype(np.int64), off0[:-1]), off1[1:] - off1[:-1])
    rest = keep & (idx != r[tree])
    cs = np.cumsum(rest)
    base = cs[off0[:-1]] - rest[off0[:-1]]  # the kept non-root nodes before each tree
    to = off1[tree] + 1 + (cs - rest - base[tree])  # old order behind row 0
    rest = np.flatnonzero(rest)
    for key in ("x", "y", "yaw", "edge_cost"):
        assert np.array_equal(st1[key][to[rest]], st0[key][rest]), key
    for q in range(len(off1) - 1):
        g0, g1 = off1[q], off1[q + 1]
        verdict, _ = forest_state_ref.check_tree(st1["parent"][g0:g1], st1["edge_cost"][g0:g1],
                                                 st1["cost"][g0:g1])
        assert verdict == forest_state_ref.OK, q
    return moved


# ------------------------------------------------- A1. several blocks, slices, scan groups
def test_many_queries_tops_in_several_slices(pkg, ctx, oracle_mod):
    t0 = time.perf_counter()
    b, raw, osc, starts, goals, seeds = _grow(pkg, ctx, oracle_mod)
    st = b.export_forest()
    off = st["off"]
    nodes, depth = _deepest(st)
    exp = _advance_checked(b, osc, 0, nodes, None, 2)
    tops1, tops2 = _round_tops(exp, 1), _round_tops(exp, 2)
    alone = np.flatnonzero(nodes < 0)
    below = [q for q, e in enumerate(exp) if e["below"] > 0]
    failed = sum(e["failed_tops"] for e in exp)
    print("A1: nodes", int(off[-1]), "one-node trees", len(alone), "deepest chain",
          int(depth.max()), "tops", sum(tops1), sum(tops2), "slices", -(-sum(tops1) // SLICE),
          -(-sum(tops2) // SLICE), "straddled", _straddled(off), "below", len(below), "reattached", b.last_reattached,
          "recovered", b.last_recovered, "failed tops", failed, "dropped", b.last_dropped)
    assert sum(tops1) > 2 * SLICE
    assert sum(tops2) > SLICE
    assert off[-1] > 2 * SCAN
    assert _straddled(off) >= 4
    assert len(alone) >= 1 and all(exp[q]["identity"] for q in alone)
    assert len(below) >= 1
    assert b.last_reattached > 0 and failed > 0
    # what follows, on both sides of the sub-batch splits, at a slice edge of round 1's tops in
    # node order and in a query that was left alone
    cum = np.cumsum(tops1)
    edge = [int(np.searchsorted(cum, m, side="left")) for m in (SLICE, 2 * SLICE)]
    assert all(tops1[q] > 0 for q in edge)
    sp = _splits(Q)
    chosen = sorted({0, Q - 1, sp[0] - 1, sp[0], sp[1] - 1, sp[1], edge[0], edge[1], int(alone[0])})
    _continue_checked(oracle_mod, b, osc, exp, seeds, N_ITER, 50, 0, 0.0, queries=chosen)
    print("A1 wall %.2f s" % (time.perf_counter() - t0))


# ------------------------------------------------------------ A2. the packed order of tops
def test_order_of_tops_does_not_matter(pkg, ctx, oracle_mod):
    t0 = time.perf_counter()
    b, raw, osc, starts, goals, seeds = _grow(pkg, ctx, oracle_mod)
    st = b.export_forest()
    nodes, _ = _deepest(st)
    out = []
    for other in (1000, 2000):
        c = pkg.Context(0)
        try:
            # other starts and seeds: everything has to come from the imported state
            twin = _batch(pkg, raw, goals, seeds + np.uint64(other), MAX_ITER, 0, 0.0, ctx=c)
            twin.import_forest(st)
            n_new, new_index = twin.advance(nodes, rounds=2)
            out.append((twin.export_forest(), n_new, new_index,
                        (twin.last_dropped, twin.last_reattached, twin.last_recovered)))
        finally:
            c.close()
    (sa, na, ia, ca), (sb, nb, ib, cb) = out
    assert ca == cb and ca[1] > 0
    assert np.array_equal(na, nb) and np.array_equal(ia, ib)
    assert sa.keys() == sb.keys()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert not np.array_equal(sa["off"], st["off"])  # (something moved)
    print("A2 wall %.2f s" % (time.perf_counter() - t0))


# --------------------------------------------------------------- A3. hops, rounds 0 and 1
@pytest.mark.parametrize("rounds", [0, 1])
def test_hops_and_mixed_rounds_at_scale(pkg, ctx, oracle_mod, rounds):
    t0 = time.perf_counter()
    b, raw, osc, starts, goals, seeds = _grow(pkg, ctx, oracle_mod)
    nodes, depth = _deepest(b.export_forest())
    qs = np.arange(Q)
    # hops by query: 0 (the identity), 1, half the depth, past the depth (clamped)
    hops = np.choose(qs % 4, [np.zeros(Q, dtype=np.int64), np.ones(Q, dtype=np.int64), depth // 2,
                              depth + 5]).astype(np.int32)
    nodes = np.where(qs % 3 == 0, -1, nodes).astype(np.int32)
    exp = _advance_checked(b, osc, 0, nodes, hops, rounds)
    moved = np.array([e["r"] > 0 for e in exp])
    for kind in range(4):
        live = (qs % 4 == kind) & (nodes >= 0)
        assert live.sum() >= 40
        if kind == 0:
            assert not moved[live].any()
        else:
            assert moved[live].sum() >= 20, kind
    clamped = [q for q in qs[(qs % 4 == 3) & (nodes >= 0)] if exp[q]["r"] == nodes[q]]
    assert len(clamped) >= 20
    sp = _splits(Q)
    assert all(moved[s:].any() and moved[:s].any() for s in sp) and moved[256:].any()
    print("A3 rounds", rounds, "moved", int(moved.sum()), "kept", sum(e["kept"] for e in exp),
          "reattached", b.last_reattached, "recovered", b.last_recovered)
    # the stored start of a moved query is its new root: the focus filter of the steps that follow
    # measures from it (tests/star_focus_ref.py), in every block of queries
    node, cost = b.plan(goals)
    # (plan's unit: a length over the turn radius)
    far = 1.5 * np.hypot(*(goals[:, :2] - starts[:, :2]).T) / b.space.get_steer()
    b.focus(goals, np.where(np.isfinite(cost), cost, far))
    fxy, fb, skipped = b.focus_state()
    n_steps = 30
    b.extend(n_steps)
    n = b.state()[0]
    after = b.focus_state()[2]
    chosen = [int(q) for part in (qs[:sp[0]], qs[sp[0]:sp[1]], qs[sp[1]:256], qs[256:])
              for q in part[moved[part]][:2]]
    assert len(chosen) == 8
    for q in chosen:
        t = exp[q]["tree"]
        root = (t[0][0], t[1][0], t[2][0])
        r = star_focus_ref.Query(osc, root, seeds[q], MAX_ITER, 0, 0.0)
        r.tr = ref.oracle_tree(root, t, exp[q]["elen"], n_steps)
        r.it, r.skipped = N_ITER, int(skipped[q])
        r.set_focus(fxy[q], fb[q])
        r.extend(n_steps)
        _assert_same(b.tree(q, n[q]), r.arrays())
        assert after[q] == r.skipped, q
    assert any(after[q] > skipped[q] for q in chosen)  # the filter rejected draws
    # the stored start follows in every block of queries: in polygon mode a scene change tests
    # each root by it.  A ring over the new root of one moved query of the last block empties that
    # query; the same ring over the old root of another does not
    from pathplanning_amd import scenes

    base = scenes.bench6_polygons_open()
    osc1 = oracle_mod.OracleScene.from_raw(base)
    trees = {}
    for q in qs[256:][moved[256:]]:  # moved far, and a tree that the polygons alone leave standing
        if np.hypot(exp[q]["tree"][0][0] - starts[q][0], exp[q]["tree"][1][0] - starts[q][1]) > 2.0:
            t = b.tree(q, n[q])
            if ref.revalidate(osc1, t)["kept"] >= 5:
                trees[int(q)] = t
        if len(trees) == 3:
            break
    qa, qb, qc = trees
    rings = [_square(trees[qa][0][0], trees[qa][1][0], 0.2),
             _square(starts[qb][0], starts[qb][1], 0.2)]
    poly = _with_ring(_with_ring(base, rings[0]), rings[1])
    osc2 = oracle_mod.OracleScene.from_raw(poly)
    want = {q: ref.revalidate(osc2, t) for q, t in trees.items()}
    assert want[qa]["kept"] == 1 and want[qb]["kept"] > 1
    n_new, _ = b.set_space(_space(poly))
    for q, e in want.items():
        assert n_new[q] == e["kept"], (q, n_new[q], e["kept"])
        for got, exact in zip(b.tree(q, n_new[q]), e["tree"]):
            assert np.array_equal(got, exact), q
    print("A3 wall %.2f s" % (time.perf_counter() - t0))


# ------------------------------------------------- A4. more queries than the cost kernel's waves
def test_more_queries_than_cost_waves(pkg, ctx, oracle_mod):
    """16,448 queries: advance_cost_kernel runs 4096 blocks of four waves, so the queries from
    16,384 on are a wave's second trip.  Through _advance_checked (everything the call returns and
    leaves behind): those 64 and 256 spread evenly below.  Every query: the exported forest after
    the call against the restatement of the exported forest before it, bit for bit (rounds = 0:
    every kept node is in K0), and on the forests alone: a valid tree whose stored costs are its
    rebuild, the chosen node in row 0, the kept nodes behind it in their old order."""
    from pathplanning_amd import scenes

    t0 = time.perf_counter()
    nq, waves, n_iter = 16448, 16384, 8
    raw = scenes.bench6_open()
    osc = oracle_mod.OracleScene.from_raw(raw)
    starts = scenes.config3_queries(raw, 0, 512)[0][np.arange(nq) % 512]
    seeds = np.arange(nq, dtype=np.uint64) + np.uint64(42)
    b = _batch(pkg, raw, starts, seeds, 15, 0, 0.0, ctx=ctx)
    b.extend(n_iter)
    t1 = time.perf_counter()
    st0 = b.export_forest()
    nodes, _ = _deepest(st0)
    check = np.concatenate([np.linspace(0, waves - 1, 256).astype(np.int64), np.arange(waves, nq)])
    exp = _advance_checked(b, osc, 0, nodes, 1, 0, check=check)
    assert any(exp[q]["r"] > 0 for q in range(waves, nq))
    st1 = b.export_forest()
    moved = _check_one_hop(st0, st1, nodes)
    assert moved[waves:].any() and (~moved).any()
    off0, off1 = st0["off"], st1["off"]
    rows = ("x", "y", "yaw", "parent", "cost")
    for q in range(nq):
        g0, g1, h0, h1 = off0[q], off0[q + 1], off1[q], off1[q + 1]
        e = adv.advance(osc, tuple(st0[key][g0:g1] for key in rows), st0["edge_cost"][g0:g1], 0,
                        int(nodes[q]), 1, 0)
        assert h1 - h0 == e["kept"], q
        for key, want in zip(rows + ("edge_cost",), e["tree"] + (e["elen"],)):
            assert np.array_equal(st1[key][h0:h1], want), (q, key)
    print("A4: nodes", int(off0[-1]), "->", int(off1[-1]), "moved", int(moved.sum()),
          "of them past", waves, ":", int(moved[waves:].sum()), "grow %.2f s" % (t1 - t0),
          "wall %.2f s" % (time.perf_counter() - t0))

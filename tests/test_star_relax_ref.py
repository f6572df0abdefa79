"""The CPU restatement of pp_star_relax (tests/star_relax_ref.py, DESIGN.md §3.8 "Relaxing the
trees") against its own specification, on trees grown by the RRT* oracle (orc_star_extend):
bench6_open, 400 iterations, seeds 0 / 5 / 11 / 12, tests/test_star_repair_ref.py's starts.  Chains
end in the root, the cost invariant holds bit for bit, no cost rises, untouched subtrees stay, the
order of the nodes cannot matter, a fixed point is the identity, the cost[p] >= cost[i] skip is
exact, an inactive tree stays, and after an advance the relaxed trees are markedly cheaper and
still hold edge by edge."""
import numpy as np
import pytest

import star_advance_ref as adv
import star_relax_ref as rlx
import star_revalidate_ref as ref

SEEDS = [0, 5, 11, 12]
CASES = [(0, 0.0), (0, 2.0), (4, 0.0)]


def _starts(raw):
    return [raw["start"], (-4.0, -4.5, 0.3), (-3.0, -3.0, 0.785), (2.0, -4.0, 1.2)]


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def grown(oracle_mod):
    """(k, eta) -> (the scene, the four trees, their edge costs, relax(1), relax(16)), computed once"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    osc = oracle_mod.OracleScene.from_raw(raw)
    out = {}
    for k, eta in CASES:
        trees, elens = [], []
        for j, start in enumerate(_starts(raw)):
            tr = oracle_mod.OracleStarTree(tuple(start), 401)
            oracle_mod.star_extend(osc, tr, SEEDS[j], 0, 400, k, eta)
            a = tr.star_arrays()
            trees.append(a[:5])
            elens.append(a[5])
        out[(k, eta)] = (osc, trees, elens, rlx.relax(osc, trees, elens, k, 1),
                         rlx.relax(osc, trees, elens, k, 16))
    return out


def _check_tree(tree, elen0, res, q):
    """the properties of one relaxed tree against the tree it came from"""
    par0, cost0 = np.asarray(tree[3]), np.asarray(tree[4])
    par, cost, elen = res["parent"][q], res["cost"][q], res["elen"][q]
    assert rlx.chains_end_in_root(par)
    # the invariant, bit for bit (the root: cost 0)
    assert cost[0] == 0.0
    assert np.array_equal(_bits(cost[1:]), _bits(cost[par[1:]] + elen[1:]))
    assert (cost <= cost0).all()  # no cost rises
    moved = res["moved"][q]  # (a node may move in more than one round, and back)
    assert int((par != par0).sum()) <= int(moved.sum()) <= res["n_rewired"][q]
    assert (cost[moved] < cost0[moved]).all()
    # a node without a re-parented ancestor-or-self: parent, elen and cost bit for bit
    same = ~rlx.touched(par0, par)
    assert same[0] or len(par) == 1
    assert np.array_equal(_bits(cost[same]), _bits(cost0[same]))
    assert np.array_equal(_bits(elen[same]), _bits(np.asarray(elen0)[same]))
    assert np.array_equal(_bits(elen[~moved]), _bits(np.asarray(elen0)[~moved]))


def _same(a, b):
    assert a["rounds_run"] == b["rounds_run"] and a["n_changed"] == b["n_changed"]
    assert np.array_equal(a["n_rewired"], b["n_rewired"])
    assert a["per_round"] == b["per_round"]
    for key in ("parent", "cost", "elen"):
        for u, v in zip(a[key], b[key]):
            assert np.array_equal(u, v) if key == "parent" else np.array_equal(_bits(u), _bits(v))


@pytest.mark.parametrize("k,eta", CASES)
def test_round_one_properties(grown, k, eta):
    osc, trees, elens, r1, _ = grown[(k, eta)]
    assert r1["rounds_run"] == 1 and r1["none_edges"] == 0
    for q in range(4):
        _check_tree(trees[q], elens[q], r1, q)
        assert r1["per_round"][q][0] >= 5, (q, r1["per_round"][q])  # (measured: at least 6)
        assert r1["n_rewired"][q] == int((r1["parent"][q] != trees[q][3]).sum())
        assert r1["margin"][q] >= 1e-8, (q, r1["margin"][q])  # what the GPU comparison relies on
    assert r1["n_changed"] == sum(int((_bits(r1["cost"][q]) != _bits(trees[q][4])).sum())
                                  for q in range(4))
    assert r1["n_changed"] >= int(r1["n_rewired"].sum())


@pytest.mark.parametrize("k,eta", CASES)
def test_order_of_the_nodes_cannot_matter(grown, k, eta):
    osc, trees, elens, _, r16 = grown[(k, eta)]
    rng = np.random.default_rng(3)
    _same(r16, rlx.relax(osc, trees, elens, k, 16, order=lambda v: v[::-1]))
    _same(r16, rlx.relax(osc, trees, elens, k, 16, order=lambda v: rng.permutation(v)))


@pytest.mark.parametrize("k,eta", CASES)
def test_fixed_point_is_the_identity(grown, k, eta):
    osc, trees, elens, _, r16 = grown[(k, eta)]
    assert 2 <= r16["rounds_run"] < 16  # (measured: 2 - 5)
    assert all(pr[-1] == 0 for pr in r16["per_round"])
    for q in range(4):
        _check_tree(trees[q], elens[q], r16, q)
    again_in = [tuple(trees[q][:3]) + (r16["parent"][q], r16["cost"][q]) for q in range(4)]
    again = rlx.relax(osc, again_in, r16["elen"], k, 16)
    assert again["rounds_run"] == 1 and again["n_changed"] == 0 and not again["n_rewired"].any()
    for q in range(4):
        assert np.array_equal(again["parent"][q], r16["parent"][q])
        assert np.array_equal(_bits(again["cost"][q]), _bits(r16["cost"][q]))
        assert np.array_equal(_bits(again["elen"][q]), _bits(r16["elen"][q]))


@pytest.mark.parametrize("k,eta", CASES)
def test_the_cost_skip_is_exact(grown, k, eta):
    osc, trees, elens, _, r16 = grown[(k, eta)]
    c = rlx.relax(osc, trees, elens, k, 16, cull=True)
    _same(r16, c)
    assert sum(c["culled"]) > 0 and sum(c["evaluated"]) < sum(r16["evaluated"])


def test_inactive_tree_and_one_node_tree(grown):
    k, eta = CASES[1]
    osc, trees, elens, _, r16 = grown[(k, eta)]
    one = tuple(np.asarray(a)[:1] for a in trees[3])
    ts, es = [trees[0], trees[1], trees[2], one], [elens[0], elens[1], elens[2], elens[3][:1]]
    r = rlx.relax(osc, ts, es, k, 16, active=[1, 0, 1, 1])
    for q in (1, 3):
        assert r["n_rewired"][q] == 0 and r["per_round"][q] == []
        assert np.array_equal(r["parent"][q], ts[q][3])
        assert np.array_equal(_bits(r["cost"][q]), _bits(ts[q][4]))
        assert np.array_equal(_bits(r["elen"][q]), _bits(es[q]))
    # a tree's result does not depend on the others (but the call's rounds do)
    for q in (0, 2):
        assert np.array_equal(r["parent"][q], r16["parent"][q])
        assert np.array_equal(_bits(r["cost"][q]), _bits(r16["cost"][q]))
    # a root-blocked tree stays
    rb = rlx.relax(osc, ts[:2], es[:2], k, 2, blocked=[1, 0])
    assert rb["n_rewired"][0] == 0 and np.array_equal(rb["parent"][0], ts[0][3])
    assert rb["n_rewired"][1] > 0


@pytest.mark.parametrize("k,eta", CASES)
def test_after_an_advance_the_trees_get_much_cheaper_and_still_hold(grown, k, eta):
    osc, trees, elens, _, _ = grown[(k, eta)]
    ts, es = [], []
    for q in range(4):
        deepest = int(np.argmax(ref.depth(np.asarray(trees[q][3]))))
        a = adv.advance(osc, trees[q], elens[q], k, deepest, hops=2, rounds=3)
        assert not a["identity"]
        ts.append(a["tree"])
        es.append(a["elen"])
    r = rlx.relax(osc, ts, es, k, 8)
    assert r["rounds_run"] >= 2 and r["none_edges"] == 0
    for q in range(4):
        _check_tree(ts[q], es[q], r, q)
        before, after = float(np.sum(ts[q][4])), float(np.sum(r["cost"][q]))
        assert after <= 0.96 * before, (q, before, after)  # (measured: at least 4.8 % lower)
        assert r["per_round"][q][0] >= 5
        assert r["margin"][q] >= 1e-8, (q, r["margin"][q])
        # edge by edge in the scene: every stored edge holds, its cost is the stored one
        tree = tuple(ts[q][:3]) + (r["parent"][q], r["cost"][q])
        again = ref.revalidate(osc, tree)
        assert again["none_edges"] == 0 and again["kept"] == len(tree[0])
        assert np.array_equal(_bits(again["elen"][1:]), _bits(r["elen"][q][1:]))

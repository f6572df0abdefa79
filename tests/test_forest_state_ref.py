"""CPU: the identity the forest import relies on, on the oracle's RRT* trees — every node's cost is
cost[parent] + edge_cost bit for bit, as one f64 addition with parents first, although rewired
trees are not index-ordered — and the validator's verdicts (tests/forest_state_ref.py, the numpy
restatement of pp_star_forest_import's checks)."""
import numpy as np
import pytest

import forest_state_ref as ref

N_ITER = 400
CASES = [(seed, k, eta) for seed in (5, 11) for k, eta in ((0, 0.0), (4, 0.0), (0, 2.0), (4, 2.0))]


def _oracle_tree(oracle_mod, seed, k, eta):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    sc = oracle_mod.OracleScene.from_raw(raw)
    tr = oracle_mod.OracleStarTree(raw["start"], N_ITER + 1)
    _, rw, _, _ = oracle_mod.star_extend(sc, tr, seed, 0, N_ITER, k, eta)
    x, y, yaw, par, cost, elen = tr.star_arrays()
    return ref.star_tree(x, y, yaw, par, elen, cost=cost, iterations=N_ITER, seed=seed,
                         rewires=rw), rw


@pytest.fixture(scope="module")
def trees(pkg, oracle_mod):
    return {c: _oracle_tree(oracle_mod, *c) for c in CASES}


@pytest.mark.parametrize("case", CASES)
def test_cost_is_parent_cost_plus_edge_cost_bit_for_bit(trees, case):
    t, _ = trees[case]
    rebuilt, lvl = ref.rebuild_costs(t["parent"], t["edge_cost"])
    assert (lvl > 0).all()
    assert np.array_equal(rebuilt.view(np.uint64), t["cost"].view(np.uint64))
    v, bad, out = ref.check_state(ref.pack([t]), N_ITER)
    assert (v, bad) == (ref.OK, None)
    assert np.array_equal(out.view(np.uint64), t["cost"].view(np.uint64))


@pytest.mark.parametrize("case", CASES)
def test_fixtures_are_not_vacuous(trees, case):
    """a rewire happened, and some node hangs under a later one: an index-order sweep would be
    wrong here"""
    t, rw = trees[case]
    assert rw >= 1
    assert (t["parent"] > np.arange(len(t["parent"]))).any()


def test_validator_rejects_each_defect_and_names_the_slot(trees):
    good, _ = trees[(5, 0, 0.0)]
    other, _ = trees[(11, 0, 0.0)]
    variants = ref.bad_variants(good)
    assert len(variants) == 10
    queries = [7, 2, 4]
    for name, bad_tree, expected in variants:
        v, bad, _ = ref.check_state(ref.pack([other, bad_tree, good]), N_ITER, queries)
        assert (v, bad) == (expected, 2), name
    v, bad, _ = ref.check_state(ref.pack([other, good, good]), N_ITER, queries)
    assert (v, bad) == (ref.OK, None)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_hand_built_chains_are_accepted(n):
    t = ref.chain_tree(n, reverse=n == 130)
    if n == 130:  # depth 129, every parent after its child
        assert (t["parent"][1:-1] == np.arange(2, n)).all() and t["parent"][-1] == 0
    v, bad, cost = ref.check_state(ref.pack([t]), 1000)
    assert (v, bad) == (ref.OK, None)
    # the same sums, walked chain by chain
    for i in range(n):
        c, j, chain = 0.0, i, []
        while j > 0:
            chain.append(j)
            j = int(t["parent"][j])
        for j in reversed(chain):
            c = c + float(t["edge_cost"][j])
        assert c == cost[i]


def test_ordered_rule_of_the_extend_batch():
    t = ref.chain_tree(8, reverse=True)
    assert ref.check_tree(t["parent"], ordered=True)[0] == ref.INVALID
    assert ref.check_tree(ref.chain_tree(8)["parent"], ordered=True)[0] == ref.OK

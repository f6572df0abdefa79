"""The CPU restatement of committing chain shortcuts into the tree
(tests/star_shortcut_commit_ref.py) on oracle trees: the numbers of the sketch that motivated the
feature (tests/golden/star_shortcut_commit.json), its agreement with the shortcut DP, and the
rule's properties.  Seven trees: three that rewire, three no-ops on the disc fields, one no-op on
the occupancy grid.  No GPU."""
import numpy as np
import pytest

import forest_state_ref as fs
import star_goal_ref as goal_ref
import star_shortcut_commit_ref as ref
import star_shortcut_ref as sref
from conftest import load_golden

# the figures of the motivating sketch, case by case (the first three rewire, the rest do not)
CASE1 = dict(node=108, D=10, span=4, rewired=[[8, 10], [7, 10], [4, 6], [3, 6], [2, 6], [1, 5]],
             n_changed=45, cost=31.835081761308558, plan_before=31.798491169747965,
             plan_after=31.354794565556862, best_node=78)
REWIRES = (6, 2, 4, 0, 0, 0, 0)
CHANGED = (45, 24, None, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """(spec, golden record, osc, tree, edge_cost, goal, node, result, cnode, w) per case, each
    tree grown and committed once"""
    specs, recs = ref.specs(), load_golden("star_shortcut_commit.json")
    assert len(specs) == len(recs) == 7
    out = []
    for spec, rec in zip(specs, recs):
        osc, tree, el, goal, node = ref.case(spec)
        res, cnode, w, _ = ref.commit_oracle(osc, tree, el, goal, node, spec["span"])
        out.append((spec, rec, osc, tree, el, goal, node, res, cnode, w))
    return out


def test_recorded_numbers(cases):
    """the rewire lists, costs and changed-cost counts of the sketch, and the golden file"""
    for k, (spec, rec, osc, tree, el, goal, node, res, cnode, w) in enumerate(cases):
        got = ref.golden_record(spec)
        assert set(got) == set(rec)
        for key in rec:
            if key in ("cost", "plan_before", "plan_after", "gap"):
                assert abs(got[key] - rec[key]) <= 1e-12 * abs(rec[key]), (k, key)
            elif key == "goal":
                assert np.allclose(got[key], rec[key], rtol=1e-12, atol=0.0)
            else:
                assert got[key] == rec[key], (k, key)
        assert len(rec["rewired"]) == REWIRES[k]
        if CHANGED[k] is not None:
            assert rec["n_changed"] == CHANGED[k]
        assert 43 <= rec["n_nodes"] <= 259
        assert rec["gap"] > 1e-6  # the GPU test compares these rewire lists
    spec, rec, osc, tree, el, goal, node, res, cnode, w = cases[0]
    assert node == CASE1["node"] and len(cnode) == CASE1["D"] and spec["span"] == CASE1["span"]
    assert [list(p) for p in res["rewired"]] == CASE1["rewired"]
    assert res["n_changed"] == CASE1["n_changed"]
    assert res["cost_out"] == CASE1["cost"]
    before = goal_ref.plan(osc, tree, goal)
    after = goal_ref.plan(osc, ref.committed_tree(tree, res), goal)
    assert before[0] == after[0] == CASE1["best_node"]
    assert before[1] == CASE1["plan_before"] and after[1] == CASE1["plan_after"]


def test_agrees_with_the_shortcut(cases):
    """every freshly steered own edge equals the stored edge cost bit for bit in all seven trees,
    and then cost_out is the shortcut DP's cost bit for bit and the tree chain from node_out is
    its chain row"""
    rich = 0
    for spec, rec, osc, tree, el, goal, node, res, cnode, w in cases:
        D = len(cnode)
        assert all(w[i, 0] == el[cnode[i - 1]] for i in range(1, D))
        s = sref.shortcut(osc, tree, goal, node, spec["span"])
        assert s["chain"] and res["cost_out"] == s["cost"]
        assert res["node"] == s["chain"][0] and res["n_rewired"] == len(res["rewired"])
        assert sref.chain_nodes(ref.committed_tree(tree, res), res["node"]) == s["chain"]
        on_chain = np.zeros(len(tree[0]), dtype=bool)
        on_chain[cnode] = True
        off_chain = int(np.count_nonzero((res["cost"] != tree[4]) & ~on_chain))
        rich += len(res["rewired"]) >= 2 and off_chain >= 1
    assert rich >= 1
    assert cases[0][7]["n_changed"] > cases[0][1]["D"]  # 45 changed costs against D = 10


def test_costs_never_rise_and_rebuild_exactly(cases):
    for spec, rec, osc, tree, el, goal, node, res, cnode, w in cases:
        par, cost, e = res["parent"], res["cost"], res["edge_cost"]
        assert np.all(cost <= tree[4])
        assert fs.check_tree(par, e, cost)[0] == fs.OK  # cost == cost[parent] + edge_cost exactly
        assert np.array_equal(cost[1:], cost[par[1:]] + e[1:]) and cost[0] == 0.0
        for i in range(1, len(cnode) + 1):  # on the chain the rebuilt cost is the DP's c[i]
            assert cost[cnode[i - 1]] == res["c"][i]
        # the tree is otherwise the same: only rewired chain nodes got a parent and an edge cost
        moved = np.flatnonzero((par != tree[3]) | (e != el))
        assert sorted(moved) == sorted(int(cnode[i - 1]) for i, _ in res["rewired"])
        for i, j in res["rewired"]:
            assert par[cnode[i - 1]] == cnode[j - 1] and e[cnode[i - 1]] == w[i, j - i - 1]
        if not res["rewired"]:
            assert np.array_equal(cost, tree[4]) and res["n_changed"] == 0


def test_plan_improves(cases):
    for k, (spec, rec, osc, tree, el, goal, node, res, cnode, w) in enumerate(cases):
        before = goal_ref.plan(osc, tree, goal)[1]
        after = goal_ref.plan(osc, ref.committed_tree(tree, res), goal)[1]
        assert after <= before
        assert after <= res["cost_out"]
        if k == 0:
            assert after < before


def test_second_commit_is_a_no_op(cases):
    """with span >= D a second commit on the new chain rewires nothing and returns the same cost"""
    for spec, rec, osc, tree, el, goal, node, res, cnode, w in cases[:3]:
        D = len(cnode)
        r1, _, _, _ = ref.commit_oracle(osc, tree, el, goal, node, D)
        t1 = ref.committed_tree(tree, r1)
        r2, cn2, _, _ = ref.commit_oracle(osc, t1, r1["edge_cost"], goal, r1["node"], D)
        assert r1["rewired"] and not r2["rewired"] and r2["n_changed"] == 0
        assert r2["cost_out"] == r1["cost_out"] and r2["node"] == r1["node"]
        assert np.array_equal(r2["parent"], r1["parent"]) and np.array_equal(r2["cost"], r1["cost"])


def test_span_one_rewires_nothing(cases):
    for spec, rec, osc, tree, el, goal, node, res, cnode, w in cases:
        r1 = ref.commit(tree, el, cnode, w, 1)
        assert not r1["rewired"] and r1["n_changed"] == 0
        assert np.array_equal(r1["parent"], tree[3]) and np.array_equal(r1["cost"], tree[4])
        assert r1["node"] == node and r1["cost_out"] == tree[4][node] + w[0, 0]


def test_stored_edges_are_kept(cases):
    """a node whose own edge no longer verifies keeps its stored edge unless a cheaper feasible one
    exists; an infeasible goal row gives -1, inf and 0 rewires reported while the chain commits"""
    spec, rec, osc, tree, el, goal, node, res, cnode, w = cases[0]
    w2 = w.copy()
    w2[1:, 0] = np.inf  # every own edge blocked
    r = ref.commit(tree, el, cnode, w2, spec["span"])
    assert np.all(r["cost"] <= tree[4]) and fs.check_tree(r["parent"], r["edge_cost"], r["cost"])[0] == fs.OK
    kept = [i for i in range(1, len(cnode)) if i not in {a for a, _ in r["rewired"]}]
    assert kept and all(r["edge_cost"][cnode[i - 1]] == el[cnode[i - 1]] for i in kept)
    w3 = w.copy()
    w3[0, :] = np.inf
    r = ref.commit(tree, el, cnode, w3, spec["span"])
    assert r["node"] == -1 and r["cost_out"] == np.inf and r["n_rewired"] == 0
    assert [list(p) for p in r["rewired"]] == [p for p in CASE1["rewired"]]
    assert np.array_equal(r["parent"], res["parent"]) and np.array_equal(r["cost"], res["cost"])

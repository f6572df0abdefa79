"""The CPU restatement of the shortcuts along the chain (tests/star_shortcut_ref.py) on oracle
trees: the recorded numbers of the measurement that motivated the feature, the DP's properties
and the golden file.  No GPU."""
import numpy as np
import pytest

import star_goal_ref as goal_ref
import star_shortcut_ref as ref
from conftest import load_golden


@pytest.fixture(scope="module")
def recorded(oracle_mod):
    """the recorded trees: (record, osc, tree, goal) per case, grown once"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    osc = oracle_mod.OracleScene.from_raw(raw)
    out = []
    for rec in ref.RECORDED:
        tree = ref.grow(raw, raw["start"], rec["seed"], rec["n_iter"], rec["k"], rec["eta"], osc)
        out.append((rec, osc, tree, raw["goal"]))
    return out


def test_recorded_numbers(recorded):
    rec, osc, tree, goal = recorded[0]
    assert len(tree[0]) == rec["n_nodes"]
    assert ref.deepest_reaching_node(osc, tree, goal) == rec["node"]
    s1 = ref.shortcut(osc, tree, goal, rec["node"], 1)
    assert s1["D"] == rec["D"] and s1["positions"] == list(range(rec["D"] + 1))
    assert abs(s1["cost"] - rec["tree_cost"]) <= 1e-12 * rec["tree_cost"]
    for span, want in rec["spans"].items():
        s = ref.shortcut(osc, tree, goal, rec["node"], span)
        assert abs(s["cost"] - want["cost"]) <= 1e-12 * want["cost"]
        assert len(s["positions"]) - 1 == want["edges"]
        assert s["pairs"] == want["pairs"]
        assert int(np.isfinite(s["w"]).sum()) == want["feasible"]
        if "positions" in want:
            assert s["positions"] == want["positions"]


def test_recorded_second_case(recorded):
    rec, osc, tree, goal = recorded[1]
    assert ref.deepest_reaching_node(osc, tree, goal) == rec["node"]
    s1 = ref.shortcut(osc, tree, goal, rec["node"], 1)
    assert s1["D"] == rec["D"]
    assert round(s1["cost"], 2) == rec["tree_cost"]
    for span, want in rec["spans"].items():
        assert round(ref.shortcut(osc, tree, goal, rec["node"], span)["cost"], 4) == want["cost"]


def test_span_one_is_plans_total(recorded):
    """span 1 accumulates like the tree (cost[child] = cost[parent] + edge): bit for bit the goal
    connection's total of the node"""
    for rec, osc, tree, goal in recorded:
        total = goal_ref.goal_costs(osc, tree, goal)
        assert ref.shortcut(osc, tree, goal, rec["node"], 1)["cost"] == total[rec["node"]]


def test_cost_non_increasing_in_span(recorded):
    rec, osc, tree, goal = recorded[0]
    _, w63, _ = ref.band(osc, tree, goal, rec["node"], 63)
    prev = np.inf
    for span in (1, 2, 3, 5, 8, 13, 24, 25, 26, 63):
        cost, pos, _ = ref.dp(w63[:, :span])  # (a narrower band is a prefix of the rows)
        assert cost <= prev
        assert pos[0] == 0 and pos[-1] == rec["D"]
        assert all(0 < b - a <= span for a, b in zip(pos, pos[1:]))
        prev = cost
    assert ref.dp(w63[:, :25])[0] == ref.dp(w63)[0]  # span past D changes nothing


def test_golden_file(oracle_mod):
    """the golden records are what the restatement gives; the DP equals the brute force over all
    subsets where D <= 10; every edge of a returned chain is feasible"""
    recs = load_golden("star_shortcut.json")
    assert {r["scene"] for r in recs} == set(ref.SCENES)
    specs = ref.golden_specs()
    assert len(specs) == len(recs)
    brute = 0
    for spec, rec in zip(specs, recs):
        got = ref.golden_record(spec)
        assert got["node"] == rec["node"] and got["D"] == rec["D"] and got["pairs"] == rec["pairs"]
        assert got["chain"] == rec["chain"] and got["feasible"] == rec["feasible"]
        assert rec["chain"] and abs(got["cost"] - rec["cost"]) <= 1e-12 * rec["cost"]
        assert rec["gap"] is None or rec["gap"] > 1e-6  # the GPU test compares these chains
        raw = ref.scene(rec["scene"])
        osc = oracle_mod.OracleScene.from_raw(raw)
        tree = ref.grow(raw, rec["start"], rec["seed"], rec["n_iter"], rec["k"], rec["eta"], osc)
        s = ref.shortcut(osc, tree, rec["goal"], rec["node"], rec["span"])
        feas = {tuple(p) for p in rec["feasible"]}
        assert all((a, b) in feas for a, b in zip(s["positions"], s["positions"][1:]))
        cn, ps = ref.poses(tree, rec["goal"], rec["node"])
        for a, b in zip(s["positions"], s["positions"][1:]):  # ... and verified afresh
            assert np.isfinite(ref.edge_cost(osc, ps[a], ps[b]))
        assert s["chain"][-1] == 0
        if rec["D"] <= 10:
            assert ref.brute(s["w"]) == s["cost"]
            brute += 1
    assert brute >= 3
    assert any(r["span"] > r["D"] for r in recs) and any(len(r["feasible"]) < r["pairs"] for r in recs)

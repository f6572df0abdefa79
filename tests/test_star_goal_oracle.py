"""CPU: the RRT* goal connection's restatement (tests/star_goal_ref.py — oracle.dubins +
verify_line per (goal, node) pair) against its golden file, the conditions the GPU
test relies on, and the C ABI's new entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

import star_goal_ref as ref
from conftest import ROOT, load_golden

GOLDEN = "star_goal.json"
SYMBOLS = ("pp_star_plan", "pp_star_goal_costs", "pp_star_path")


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """per golden record: (record, scene, tree, total) computed once"""
    out = []
    for rec in load_golden(GOLDEN):
        raw = ref.scene(rec["scene"])
        osc = oracle_mod.OracleScene.from_raw(raw)
        tree = ref.grow(raw, rec["start"], rec["seed"], rec["n_iter"], rec["k"], rec["eta"], osc)
        out.append((rec, osc, tree, ref.goal_costs(osc, tree, rec["goal"])))
    return out


def test_helper_reproduces_golden(oracle_mod, cases):
    specs = ref.golden_specs()
    assert len(specs) == len(cases)
    for spec, (rec, osc, tree, total) in zip(specs, cases):
        assert all(rec[k] == v for k, v in spec.items())
        b, c = ref.first_min(total)
        assert len(tree[0]) == rec["n_nodes"] and b == rec["best_node"]
        assert [int(i) for i in np.flatnonzero(np.isfinite(total))] == rec["feasible"]
        if b < 0:
            assert c == np.inf and rec["cost"] is None and rec["path_points"] == 0
            continue
        assert c == rec["cost"] and ref.runner_up_gap(total) == rec["gap"]
        xy, length = ref.path(osc, tree, rec["goal"], b)
        assert len(xy) == rec["path_points"] and length == rec["path_length"]


def test_golden_best_nodes_are_well_separated():
    """the GPU's best_node is demanded exactly: every reachable case keeps its best and second
    total > 1e-6 apart (relative), three orders above the 1e-9 cost tolerance between the device's
    and the host's trig"""
    recs = load_golden(GOLDEN)
    reach = [r for r in recs if r["best_node"] >= 0]
    assert len(reach) >= 8 and len(reach) < len(recs)  # (both unreachable cases are there too)
    for r in reach:
        assert r["gap"] is not None and r["gap"] > 1e-6, r


def test_golden_paths_verify(oracle_mod, cases):
    for rec, osc, tree, total in cases:
        if rec["best_node"] < 0:
            continue
        xy, length = ref.path(osc, tree, rec["goal"], rec["best_node"])
        assert osc.verify_line(xy[:, 0], xy[:, 1])
        assert (xy[0, 0], xy[0, 1]) == (tree[0][0], tree[1][0])  # root first
        assert length > 0.0


def test_best_cost_never_rises_with_more_iterations():
    """RRT* costs only fall and nodes are only added"""
    recs = [r for r in load_golden(GOLDEN) if r["scene"] == "bench6_open"]
    for seed in (5, 11):
        c = {r["n_iter"]: r["cost"] for r in recs if r["seed"] == seed}
        assert c[100] >= c[200] >= c[400]


def test_abi_exports_the_goal_connection(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._ffi.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\b(pp_[a-z0-9_]+)\b", out))
    with open(os.path.join(ROOT, "include", "pathplanning_amd.h")) as f:
        declared = set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", f.read()))
    for s in SYMBOLS:
        assert s in exported and s in declared and s in pkg._ffi.EXPORTED
    assert all(hasattr(pkg.rrt.RRTStarBatch, m) for m in ("plan", "goal_costs", "path"))

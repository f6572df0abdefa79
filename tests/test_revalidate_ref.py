"""CPU: the revalidation restatement (tests/revalidate_ref.py: per-edge verify with the stored yaw,
the sequential keep loop, the stable compaction) against the oracle's own full re-verify of
line_to_origin (orc_verify_candidate with full_reverify, RRT::verify_node, rrt.rs:414-426)."""
import numpy as np
import pytest

import revalidate_ref as ref


@pytest.fixture(scope="module")
def bench6_tree(oracle_mod, pkg):
    from pathplanning_amd import scenes

    raw = scenes.bench6()
    sc = oracle_mod.OracleScene.from_raw(raw)
    tr = oracle_mod.OracleTree(raw["start"], 1 << 13)
    oracle_mod.rrt_extend(sc, tr, 7, 0, 3000)
    return raw, sc, tr


def _disc_on_quarter_subtree(raw, tree):
    """bench6 plus one disc of r = 0.3 on the node whose descendant count is nearest n / 4"""
    x, y, _, par = tree
    cnt = ref.descendants(par)
    v = 1 + int(np.argmin(np.abs(cnt[1:] - len(x) / 4.0)))
    return ref.with_discs(raw, [(x[v], y[v], 0.3)]), v


def test_restatement_equals_full_reverify(oracle_mod, bench6_tree):
    raw, _, tr = bench6_tree
    tree = tr.arrays()
    x, y, _, par = tree
    raw2, v = _disc_on_quarter_subtree(raw, tree)
    sc2 = oracle_mod.OracleScene.from_raw(raw2)
    r = ref.revalidate(sc2, tree)
    assert 0 < r["kept"] < len(x) and r["orphans"] > 0 and not r["keep"][v]
    for i in range(1, len(x)):
        ok, _ = oracle_mod.verify_candidate(sc2, tr, x[i], y[i], int(par[i]), full_reverify=True)
        assert ok == bool(r["keep"][i]), i
    # the compaction: stable, poses untouched, parents remapped onto kept earlier nodes
    nx, ny, nyaw, npar = r["tree"]
    kept = np.flatnonzero(r["keep"])
    assert np.array_equal(r["new_index"][kept], np.arange(len(kept)))
    assert (r["new_index"][~r["keep"]] == -1).all()
    assert np.array_equal(nx, x[kept]) and np.array_equal(ny, y[kept])
    assert np.array_equal(nyaw, tree[2][kept])
    assert npar[0] == -1 and np.array_equal(kept[npar[1:]], par[kept[1:]])


def test_identity_under_the_unchanged_scene(bench6_tree):
    _, sc, tr = bench6_tree
    tree = tr.arrays()
    r = ref.revalidate(sc, tree)
    assert r["kept"] == len(tree[0]) and r["failed"] == 0 and r["orphans"] == 0
    assert np.array_equal(r["new_index"], np.arange(len(tree[0])))
    for a, b in zip(r["tree"], tree):
        assert np.array_equal(a, b)

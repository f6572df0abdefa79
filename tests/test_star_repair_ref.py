"""The CPU restatement of pp_star_repair (tests/star_repair_ref.py, DESIGN.md §3.8 "Re-attaching
orphaned subtrees") against its own specification, on trees grown by the RRT* oracle
(orc_star_extend): rounds = 0 is the revalidation, the order of the tops cannot matter, the
repaired tree holds in the new scene edge by edge, K0 is untouched, and more rounds only keep
more.  The inputs are tests/test_gpu_star_revalidate.py's: bench6_open, 400 iterations, seeds
0 / 5 / 11 / 12, a disc of r 0.3 on each tree's n/4-subtree node."""
import numpy as np
import pytest

import star_repair_ref as rep
import star_revalidate_ref as ref

SEEDS = [0, 5, 11, 12]
CASES = [(0, 0.0), (0, 2.0), (4, 0.0)]


def _starts(raw):
    return [raw["start"], (-4.0, -4.5, 0.3), (-3.0, -3.0, 0.785), (2.0, -4.0, 1.2)]


@pytest.fixture(scope="module")
def grown(oracle_mod):
    """(k, eta, j) -> (the old scene's raw, tree j, the scene with the disc on its n/4 node)"""
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    osc = oracle_mod.OracleScene.from_raw(raw)
    out = {}
    for k, eta in CASES:
        for j, start in enumerate(_starts(raw)):
            tr = oracle_mod.OracleStarTree(tuple(start), 401)
            oracle_mod.star_extend(osc, tr, SEEDS[j], 0, 400, k, eta)
            tree = tr.star_arrays()[:5]
            v = ref.quarter_subtree_node(tree)
            raw2 = ref.with_discs(raw, [(tree[0][v], tree[1][v], 0.3)])
            out[(k, eta, j)] = (raw, tree, oracle_mod.OracleScene.from_raw(raw2))
    return out


def _same(a, b):
    assert np.array_equal(a["keep"], b["keep"])
    assert np.array_equal(a["new_index"], b["new_index"])
    for u, v in zip(a["tree"], b["tree"]):
        assert np.array_equal(u, v)
    assert np.array_equal(a["elen"][a["keep"]], b["elen"][b["keep"]])
    assert a["rounds"] == b["rounds"]


@pytest.mark.parametrize("k,eta", CASES)
def test_zero_rounds_is_revalidate(grown, k, eta):
    for j in range(4):
        _, tree, osc2 = grown[(k, eta, j)]
        r0 = rep.repair(osc2, tree, k, 0)
        e = ref.revalidate(osc2, tree)
        assert np.array_equal(r0["keep"], e["keep"]) and np.array_equal(r0["keep0"], e["keep"])
        assert np.array_equal(r0["new_index"], e["new_index"])
        for u, v in zip(r0["tree"], e["tree"]):
            assert np.array_equal(u, v)
        assert r0["rounds"] == [] and r0["reattached"] == 0 and r0["recovered"] == 0


@pytest.mark.parametrize("k,eta", CASES)
def test_order_of_the_tops_cannot_matter(grown, k, eta):
    rng = np.random.default_rng(3)
    for j in range(4):
        _, tree, osc2 = grown[(k, eta, j)]
        a = rep.repair(osc2, tree, k, 3)
        assert a["rounds"] and a["rounds"][0]["tops"] > 1
        _same(a, rep.repair(osc2, tree, k, 3, order=lambda r, t: t[::-1]))
        _same(a, rep.repair(osc2, tree, k, 3, order=lambda r, t: rng.permutation(t)))


@pytest.mark.parametrize("k,eta", CASES)
def test_repaired_tree_holds_and_k0_is_untouched(grown, k, eta):
    later = 0
    for j in range(4):
        _, tree, osc2 = grown[(k, eta, j)]
        kept = []
        for rounds in (0, 1, 2, 3):
            r = rep.repair(osc2, tree, k, rounds)
            kept.append(r["keep"])
            # the repaired tree in the new scene: every edge holds, nothing is dropped
            again = ref.revalidate(osc2, r["tree"])
            assert again["none_edges"] == 0 and again["kept"] == r["kept"]
            assert np.array_equal(again["new_index"], np.arange(r["kept"]))
            # its costs are the sums of its edge costs along the chains
            par, cost = r["tree"][3], r["tree"][4]
            el = r["elen"][r["keep"]]
            k0 = r["keep0"][r["keep"]]
            assert np.allclose(cost[1:], cost[par[1:]] + el[1:], rtol=1e-12, atol=0.0)
            rec = ~k0
            assert np.array_equal(cost[rec], (cost[par] + el)[rec])  # recomputed: exactly
            # K0: rows, parents (remapped) and costs bit for bit
            for u, v in zip((tree[0], tree[1], tree[2], tree[4]),
                            (r["tree"][0], r["tree"][1], r["tree"][2], r["tree"][4])):
                assert np.array_equal(np.asarray(u)[r["keep0"]], v[k0])
            assert np.array_equal(r["new_index"][np.asarray(tree[3])[r["keep0"]][1:]],
                                  par[k0][1:])
            assert r["kept"] == int(r["keep0"].sum()) + r["recovered"]
            assert r["recovered"] >= r["reattached"]
            if rounds == 3:
                later += sum(d["reattached"] for d in r["rounds"][1:])
                # the figures the GPU cases rely on
                assert r["reattached"] >= 3 and r["failed_tops"] >= 1
                # (recovered counts the tops, as n_recovered does; the smallest is 31, of which
                # 23 hang below the 8 re-attached tops: (k 0, eta 2) tree 0)
                assert r["recovered"] >= 30
                assert r["recovered"] - r["reattached"] > r["reattached"]
        for a, b in zip(kept, kept[1:]):  # the kept set only grows with the rounds
            assert (b | ~a).all()
        assert kept[1].sum() > kept[0].sum()
    if (k, eta) != (0, 0.0):
        assert later > 0  # a later round re-attaches


def test_unchanged_scene_is_the_identity(grown, oracle_mod):
    raw, tree, _ = grown[(0, 2.0, 1)]
    r = rep.repair(oracle_mod.OracleScene.from_raw(raw), tree, 0, 3)
    assert r["keep"].all() and r["rounds"] == []
    for u, v in zip(r["tree"], tree):
        assert np.array_equal(u, v)
    assert np.array_equal(r["new_index"], np.arange(len(tree[0])))

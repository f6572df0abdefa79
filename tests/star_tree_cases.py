"""What the GPU tests of the tree-compaction calls share (revalidate, repair, advance, prune and the
replanning loop; tests/test_gpu_revalidate.py for the extend batch): the four bench6_open starts,
scene and tree helpers, the bit-for-bit comparison, and the two checked steps most of them take
— a scene change and a continued run against the oracle."""
import numpy as np

import star_revalidate_ref as ref
from test_gpu_rrtstar import _assert_same


def _starts(raw):
    return [raw["start"], (-4.0, -4.5, 0.3), (-3.0, -3.0, 0.785), (2.0, -4.0, 1.2)]


def _space(raw):
    from pathplanning_amd import rrt

    return rrt.Space.from_raw(raw)


def _trees(b):
    n = b.state()[0]
    return [b.tree(q, n[q]) for q in range(b.q)]


def _assert_exact(got, exp):
    for a, e in zip(got, exp):
        assert len(a) == len(e), (len(a), len(e))
        assert np.array_equal(a, e)


def _set_space_checked(oracle_mod, b, before, raw_new):
    """set_space(raw_new) on batch b holding the trees `before`; everything the call returns and
    leaves behind against the restatement.  Returns (the new scene, the restatements)."""
    osc = oracle_mod.OracleScene.from_raw(raw_new)
    exp = [ref.revalidate(osc, t) for t in before]
    assert sum(e["none_edges"] for e in exp) == 0
    n_old = np.array([len(t[0]) for t in before])
    _, it_old, ev_old, rw_old = b.state()
    n_new, new_index = b.set_space(_space(raw_new))
    off = np.concatenate([[0], np.cumsum(n_old)])
    assert len(new_index) == off[-1]
    assert np.array_equal(n_new, [e["kept"] for e in exp])
    assert b.last_dropped == int((n_old - n_new).sum())
    n_state, it, ev, rw = b.state()
    assert np.array_equal(n_state, n_new)
    assert np.array_equal(it, it_old) and np.array_equal(ev, ev_old) and np.array_equal(rw, rw_old)
    for q, e in enumerate(exp):
        got_index = new_index[off[q]:off[q + 1]]
        assert np.array_equal(got_index, e["new_index"]), (q, np.flatnonzero(got_index != e["new_index"])[:10])
        # x, y, yaw, the remapped parents, and the cost of the export before the call, bit for bit
        _assert_exact(b.tree(q, n_new[q]), e["tree"])
    return osc, exp


def _continue_checked(oracle_mod, b, osc, exp, seeds, it0, n_steps, k, eta, queries=None):
    """n_steps more lockstep steps, then `queries` (all) against orc_star_extend continued from
    the restated trees exp[q]: rows and cost from the restatement's tree, and its elen — which the
    revalidation and the repair hold per old node, the advance per kept node"""
    rw0 = b.state()[3]
    b.extend(n_steps)
    n, it, _, rw = b.state()
    assert (it == it0 + n_steps).all()
    for q in (range(len(exp)) if queries is None else queries):
        e = exp[q]
        t, elen = e["tree"], e["elen"]
        if len(elen) != len(t[0]):
            elen = elen[e["keep"]]
        tr = ref.oracle_tree((t[0][0], t[1][0], t[2][0]), t, elen, n_steps)
        _, erw, _, _ = oracle_mod.star_extend(osc, tr, int(seeds[q]), it0, n_steps, k, eta)
        _assert_same(b.tree(q, n[q]), tr.star_arrays())
        assert rw[q] - rw0[q] == erw, q


def _with_ring(raw, ring):
    out = dict(raw)
    out["obstacle_polygons"] = list(raw["obstacle_polygons"]) + [np.asarray(ring, dtype=np.float64)]
    return out


def _square(cx, cy, half):
    return np.array([(-half, -half), (half, -half), (half, half), (-half, half)]) + (cx, cy)

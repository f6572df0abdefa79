"""CPU: the far-query sets of tests/far_queries.py on the oracle alone, before any GPU sees them.

  * nearest_spec (numpy) is the oracle's get_nearest_node, index and d2 bit for bit, on every
    query of every tree — the exact ties included (lowest index);
  * the sets are not vacuous: at every magnitude at least a quarter of the queries have an exact
    runner-up within |q| 2^-23 of the winner (the f32 screen cannot tell them apart), and at 2^30
    at least 100 tie exactly in f64 with a winner that is not the tie's highest index;
  * a far sample's record built without walking its edge (far_queries.expected_records) is the
    record the oracle gives when it does walk it, at the magnitude where it can (8 B);
  * coordinates above PP_COORD_MAX are refused on the host (pp_coord_check, the check every entry
    point runs before it launches anything).
"""
import ctypes as C

import numpy as np
import pytest

import far_queries as fq


@pytest.mark.parametrize("name", list(fq.TREES))
def test_sets_are_not_vacuous_and_spec_is_the_oracle(oracle_mod, name):
    raw, (x, y, _, _) = fq.oracle_tree(oracle_mod, name)
    q = fq.build(x, y, raw["bounds"])
    assert 3000 <= len(q["qx"]) <= 5000
    B = float(np.max(np.abs(raw["bounds"])))
    assert q["M"] == (8.0 * B, 2.0 ** 12 * B, 2.0 ** 20 * B, 2.0 ** 30)
    rows, (idx, d2, run, ties) = fq.assert_not_vacuous(x, y, q)
    print(f"FARQ {name}: nodes {len(x)}; per magnitude (queries, unresolved by f32, exact ties) {rows}")
    for i in range(len(idx)):
        ei, ed2 = oracle_mod.nearest(x, y, float(q["qx"][i]), float(q["qy"][i]))
        assert ei == idx[i] and ed2 == d2[i], i
    # every kind and either sign at every magnitude; the far coordinate in x only, y only, both
    x0, y0, x1, y1 = raw["bounds"]
    for m, M in enumerate(q["M"]):
        sel = q["mag"] == m
        kinds = set(q["kind"][sel].tolist())
        assert {fq.KINDS.index(k) for k in ("axis_x", "axis_y", "diag", "rand", "bisector", "hull")} <= kinds
        qx, qy = q["qx"][sel], q["qy"][sel]
        far_x, far_y = np.abs(qx) > 0.7 * M, np.abs(qy) > 0.7 * M
        in_x, in_y = (qx >= x0) & (qx <= x1), (qy >= y0) & (qy <= y1)
        for case in (far_x & in_y, far_y & in_x, far_x & far_y):
            assert case.sum() >= 32
        for s in (qx[far_x], qy[far_y]):
            assert (s > 0).any() and (s < 0).any()
        assert (np.abs(qx) == M).any() and (np.abs(qy) == M).any()
    # an exact tie's winner is its lowest index: the tied nodes of ten queries, by hand
    for i in np.flatnonzero(ties >= 2)[:10]:
        v = (q["qx"][i] - x) * (q["qx"][i] - x) + (q["qy"][i] - y) * (q["qy"][i] - y)
        tied = np.flatnonzero(v == v.min())
        assert len(tied) == ties[i] and idx[i] == tied[0] < tied[-1]


def test_far_record_without_the_walk_is_the_oracles(oracle_mod):
    """bench6, 1500 stream samples with the 8 B class's far samples among them: the oracle walks
    the far edges too (1500 points each) and gives expected_records' rows"""
    raw, (x, y, _, _) = fq.oracle_tree(oracle_mod, "bench6")
    q = fq.build(x, y, raw["bounds"])
    sel = np.flatnonzero(q["mag"] == 0)[::3]
    half = raw["robot"][0] / 2.0
    x0, y0, x1, y1 = raw["bounds"]
    ix = np.array([oracle_mod.gen_range(7, 2 * k, x0 + half, x1 - half) for k in range(1500)])
    iy = np.array([oracle_mod.gen_range(7, 2 * k + 1, y0 + half, y1 - half) for k in range(1500)])
    sx, sy, far = fq.interleave(np.random.default_rng(2), ix, iy, q["qx"][sel], q["qy"][sel])
    tr, nn, yaw, ok = fq.expected_records(oracle_mod, raw, sx, sy, far, walk_far=True)
    assert tr.n > 500 and not ok[far].any() and ok[~far].sum() == tr.n - 1


def test_coordinates_above_the_ceiling_are_refused_on_the_host(pkg):
    """pp_coord_check needs no context and no device: PP_COORD_MAX = 2^61 passes, the next double
    and every non-finite value are PP_ERR_INVALID_ARGUMENT, in x or in y, at any position"""
    f = pkg._ffi
    L = f.lib()
    dp = C.POINTER(C.c_double)
    assert f.PP_COORD_MAX == 2.0 ** 61

    def rc(xs, ys):
        xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
        return L.pp_coord_check(xs.ctypes.data_as(dp), ys.ctypes.data_as(dp), len(xs))

    top = f.PP_COORD_MAX
    assert rc([0.0, top, -top, 2.0 ** 30], [-top, 0.0, top, 5.0]) == f.PP_OK
    assert rc([], []) == f.PP_OK
    for bad in (np.nextafter(top, np.inf), -np.nextafter(top, np.inf), 2.0 ** 62, 1e300, np.inf,
                -np.inf, np.nan):
        for pos in (0, 2):
            v = [1.0, 2.0, 3.0]
            v[pos] = bad
            assert rc(v, [0.0] * 3) == f.PP_ERR_INVALID_ARGUMENT, bad
            assert rc([0.0] * 3, v) == f.PP_ERR_INVALID_ARGUMENT, bad
            assert b"PP_COORD_MAX" in L.pp_last_error()
    assert L.pp_coord_check(None, None, 4) == f.PP_OK  # (either array may be NULL)
    assert L.pp_coord_check(None, None, -1) == f.PP_ERR_INVALID_ARGUMENT
    # the f32 screen's intermediates at the ceiling: 24 c^2 is finite in f32, at 2^62 it is not
    with np.errstate(over="ignore"):
        assert np.isfinite(np.float32(24.0) * np.float32(top) * np.float32(top))
        assert not np.isfinite(np.float32(24.0) * np.float32(2.0 ** 62) * np.float32(2.0 ** 62))

"""The scene transform helper (tests/scene_xform.py) and the scale symmetry of the sequential
spec, on the C oracle (no GPU).

Scaling a scene by a power of two is an exact symmetry of the spec: every product by ``s`` is
exact, every sum, difference, product and quotient of scaled lengths rounds to the scaled
result (no overflow or underflow at these magnitudes), the Dubins solver only sees lengths
divided by the turn radius, and rand_point's ``u * (high - low) + low`` scales too.  So the tree
of ``moved(raw, s=s)`` is the base tree with x and y times ``s`` BIT FOR BIT, with the same
parents, the same yaws (atan2 of scaled differences) and, for RRT*, the same costs (in units of
the turn radius) and rewires.  oracle/pp_oracle.c holds two absolute constants (the ``+ 1e-9``
of orc_verify_line's bbox culls); both only widen a speed-only cull, so no mode breaks the
symmetry: discs, polygons, the occupancy grid and RRT* are all pinned here.

tests/test_gpu_far_from_origin.py relies on this: the GPU's tree under a scale is compared with
the oracle's tree AND with the GPU's own base tree times ``s``.
"""
import functools

import numpy as np
import pytest

from scene_xform import moved

SCALES = [2.0 ** -20, 2.0 ** -10, 2.0 ** 10, 2.0 ** 20]
SCALE_IDS = ["s-20", "s-10", "s+10", "s+20"]

# scene -> (seed, iterations, nodes of the base tree).  The field's seed-7 run of 6000 iterations
# (also exactly covariant) holds only 23 nodes, so the field and its raster are pinned on seed 42.
RRT_CASES = {"bench6": (7, 3000, 1665), "field512": (42, 12288, 1649),
             "bench6_polygons": (7, 3000, 1675), "transit": (7, 3000, 1479),
             "field512_grid": (42, 12288, 1567)}
# scene -> (config3 query whose start and stream are used or None for the scene's own start and
# seed 7, iterations, nodes, rewires).  From the field's own start (8, 8) no Steer-2 edge fits
# between the corner and the bounds: the tree stays empty.
STAR_CASES = {"bench6_open": (None, 400, 272, 47), "field512": (7, 400, 89, 0),
              "bench6_polygons_open": (None, 400, 275, 56), "field512_grid": (11, 400, 75, 1)}


def _raw(built, name):
    from pathplanning_amd import scenes

    return getattr(scenes, name)()


@functools.lru_cache(maxsize=None)
def _rrt_tree(name, s):
    import oracle
    from pathplanning_amd import scenes

    seed, n_iter, _ = RRT_CASES[name]
    raw = moved(getattr(scenes, name)(), s=s)
    sc = oracle.OracleScene.from_raw(raw)
    tr = oracle.OracleTree(raw["start"], n_iter + 1)
    acc, nn, la = oracle.rrt_extend(sc, tr, seed, 0, n_iter)
    return tr.arrays(), nn, la


@functools.lru_cache(maxsize=None)
def _star_tree(name, s):
    import oracle
    from pathplanning_amd import scenes

    q, n_iter, _, _ = STAR_CASES[name]
    raw, seed = getattr(scenes, name)(), 7
    if q is not None:
        starts, _, seeds = scenes.config3_queries(raw, q, 1)
        raw["start"], seed = tuple(starts[0]), int(seeds[0])
    raw = moved(raw, s=s)
    sc = oracle.OracleScene.from_raw(raw)
    tr = oracle.OracleStarTree(raw["start"], n_iter + 1)
    acc, rw, nn, la = oracle.star_extend(sc, tr, seed, 0, n_iter, 0, 2.0 * s)
    return tr.star_arrays(), rw, nn, la


@pytest.mark.parametrize("s", SCALES, ids=SCALE_IDS)
@pytest.mark.parametrize("name", list(RRT_CASES))
def test_rrt_extend_scales_exactly(built, name, s):
    (bx, by, byaw, bpar), bnn, bla = _rrt_tree(name, 1.0)
    (x, y, yaw, par), nn, la = _rrt_tree(name, s)
    assert len(bx) == RRT_CASES[name][2]  # (not an empty tree)
    assert len(x) == len(bx)
    assert np.array_equal(x, bx * s) and np.array_equal(y, by * s)
    assert np.array_equal(par, bpar) and np.array_equal(yaw, byaw)
    assert np.array_equal(nn, bnn) and np.array_equal(la, bla)


@pytest.mark.parametrize("s", SCALES, ids=SCALE_IDS)
@pytest.mark.parametrize("name", list(STAR_CASES))
def test_star_extend_scales_exactly(built, name, s):
    """k = 0 (ceil(2e ln n) neighbours), Steer eta = 2 s: costs are in units of the turn radius,
    so they, the parents after rewiring and the rewire count are equal"""
    (bx, by, byaw, bpar, bcost, belen), brw, bnn, bla = _star_tree(name, 1.0)
    (x, y, yaw, par, cost, elen), rw, nn, la = _star_tree(name, s)
    assert (len(bx), brw) == STAR_CASES[name][2:]
    assert len(x) == len(bx) and rw == brw
    assert np.array_equal(x, bx * s) and np.array_equal(y, by * s)
    assert np.array_equal(par, bpar) and np.array_equal(yaw, byaw)
    assert np.array_equal(cost, bcost) and np.array_equal(elen, belen)
    assert np.array_equal(nn, bnn) and np.array_equal(la, bla)


# --------------------------------------------------------------------------------- the helper
def _same_scene(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k in ("bounds_polygon", "circles"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        elif k == "obstacle_polygons":
            assert len(a[k]) == len(b[k])
            for p, q in zip(a[k], b[k]):
                assert np.array_equal(np.asarray(p), np.asarray(q))
        elif k == "grid":
            assert np.array_equal(a[k][0], b[k][0]) and tuple(a[k][1:]) == tuple(b[k][1:])
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("name", ["bench6", "field512_grid", "bench6_polygons", "transit"])
def test_moved_pow2_round_trip(built, name):
    """a power-of-two scale and shift, then the inverse: the scene comes back bit for bit.
    (bench6 and the grid's origin are dyadic, so a shift by 2^20 loses no bit of them; the
    field's disc centres and transit's vertices are arbitrary doubles, so those scenes take
    the scale alone)"""
    raw = _raw(built, name)
    dyadic = name == "bench6"
    dx, dy, s = (2.0 ** 20, -(2.0 ** 21), 2.0 ** -10) if dyadic else (0.0, 0.0, 2.0 ** -10)
    there = moved(raw, dx, dy, s)
    back = moved(moved(there, -dx, -dy), s=1.0 / s)
    _same_scene(back, raw)
    # and the transform did something, without touching its input
    assert there["bounds"] != raw["bounds"]
    _same_scene(raw, _raw(built, name))
    assert there["step_size"] == raw["step_size"] and there["max_iter"] == raw["max_iter"]
    assert there["start"][2] == raw["start"][2] and there["goal"][2] == raw["goal"][2]


def test_moved_fields():
    raw = {"name": "t", "bounds": (0.0, 1.0, 4.0, 9.0), "robot": (1.0, 2.0, 0.5),
           "circles": np.array([[1.0, 2.0, 0.25]]), "start": (1.0, 2.0, 0.3),
           "goal": (3.0, 4.0, -0.7), "max_iter": 10, "step_size": 0.1,
           "bounds_polygon": np.array([[0.0, 1.0], [4.0, 1.0], [4.0, 9.0]]),
           "obstacle_polygons": [np.array([[1.0, 2.0], [2.0, 2.0], [2.0, 3.0]])],
           "grid": (np.array([[5]], dtype=np.uint32), 3, 0.5, 1.5, 2.0)}
    m = moved(raw, dx=10.0, dy=-20.0, s=4.0)
    assert m["bounds"] == (10.0, -16.0, 26.0, 16.0)
    assert m["robot"] == (4.0, 8.0, 2.0)
    assert m["circles"].tolist() == [[14.0, -12.0, 1.0]]
    assert m["start"] == (14.0, -12.0, 0.3) and m["goal"] == (22.0, -4.0, -0.7)
    assert m["bounds_polygon"].tolist() == [[10.0, -16.0], [26.0, -16.0], [26.0, 16.0]]
    assert m["obstacle_polygons"][0].tolist() == [[14.0, -12.0], [18.0, -12.0], [18.0, -8.0]]
    bits, w, x0, y0, cell = m["grid"]
    assert bits.tolist() == [[5]] and (w, x0, y0, cell) == (3, 12.0, -14.0, 8.0)
    assert m["step_size"] == 0.1 and m["max_iter"] == 10
    m["circles"][0, 0] = 99.0  # a deep copy
    assert raw["circles"][0, 0] == 1.0 and raw["bounds"] == (0.0, 1.0, 4.0, 9.0)


@pytest.mark.parametrize("xf", [(2.0 ** 20, -(2.0 ** 21), 1.0), (0.0, 0.0, 2.0 ** -10),
                                (4.0e6 + 0.3, 5.0e5 + 0.7, 1.0)],
                         ids=["pow2_shift", "s-10", "utm"])
def test_moved_grid_marks_the_same_cells(built, xf):
    """the oracle's cell probe on the transformed grid, at the transformed cell centres (and a
    quarter cell off them), reads the base grid's bits: the same cells are marked"""
    import oracle
    from pathplanning_amd import scenes

    dx, dy, s = xf
    raw = scenes.field512_grid()
    m = moved(raw, dx, dy, s)
    bits, w, x0, y0, cell = raw["grid"]
    assert np.array_equal(m["grid"][0], bits) and m["grid"][1] == w
    h = bits.shape[0]
    occ = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(h, -1)[:, :w] != 0
    sc = oracle.OracleScene.from_raw(m)
    half = raw["robot"][0] / 2.0
    rng = np.random.default_rng(0)
    # cells whose probes stay inside the shrunken bounds (verify_line tests bounds first)
    ii = rng.integers(1, w - 1, 4000)
    jj = rng.integers(1, h - 1, 4000)
    assert half <= cell
    for off in (0.5, 0.25, 0.75):
        px = (x0 + (ii + off) * cell) * s + dx
        py = (y0 + (jj + off) * cell) * s + dy
        got = np.array([sc.verify_line([px[k]], [py[k]]) for k in range(len(ii))])
        assert np.array_equal(got, ~occ[jj, ii])
    assert 0 < occ[jj, ii].sum() < len(ii)

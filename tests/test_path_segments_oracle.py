"""CPU, oracle only: the segment specification (tests/path_segments_ref.py; DESIGN.md §3.7 "Segment
export and sampling") is sound — an edge's three closed-form segments end at the edge's target
pose and carry every polyline point oracle.dubins keeps for the edge — and the sampler's
identities hold.  Measured on the oracle alone: the end pose misses the target by at most
1.8e-15 x max(1, box), a kept point lies within 1.3e-15 x max(1, box) of the curve; the tests use
the project's standing 1e-9 x max(1, box) (tests/test_gpu_star_paths.py)."""
import math

import numpy as np
import pytest

import path_segments_ref as ref

TOL = 1e-9
REGIMES = [(10.0, 1.0, 0.1), (2048.0, 4.0, 0.5), (2.0, 1.0, 0.1)]  # box, R, step


def _pairs(box, n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-box, box, size=(n, 4))
    yaw = rng.uniform(-math.pi, math.pi, size=(n, 2))
    return [((xy[i, 0], xy[i, 1], yaw[i, 0]), (xy[i, 2], xy[i, 3], yaw[i, 1])) for i in range(n)]


@pytest.fixture(scope="module")
def edges(oracle_mod):
    """400 random pose pairs per regime: (box, R, a, b, word, row, oracle.dubins' points)"""
    out = []
    for r, (box, R, step) in enumerate(REGIMES):
        for a, b in _pairs(box, 400, 100 + r):
            word, segs = ref.edge_segments(a, b, R, step)  # (asserts the oracle's word)
            arr = np.array(segs)
            row = {f: arr[:, i].copy() for i, f in enumerate(ref.FIELDS)}
            px, py = oracle_mod.dubins(*a, *b, R, step)[:2]
            out.append((r, box, R, a, b, word, row, px, py))
    return out


def test_every_word_occurs(edges):
    seen = [set(), set(), set()]
    for r, *_rest in edges:
        seen[r].add(_rest[4])
    assert seen[2] == {0, 1, 2, 3, 4, 5}
    assert seen[0] >= {0, 1, 2, 3}


def test_segments_end_at_the_target_pose(edges):
    worst = 0.0
    for r, box, R, a, b, word, row, _, _ in edges:
        assert row["x"][0] == a[0] and row["y"][0] == a[1] and row["yaw"][0] == a[2]
        assert np.all(row["len"] >= 0.0)
        assert ref.words_of(row) == [word]
        ex, ey, eyaw = ref.row_end(row)
        err = max(abs(ex - b[0]), abs(ey - b[1])) / max(1.0, box)
        worst = max(worst, err)
        assert err <= TOL, (a, b)
        assert abs(math.remainder(eyaw - b[2], 2.0 * math.pi)) <= TOL, (a, b)
    print(f"end pose: worst {worst:.3g} x max(1, box)")


def test_oracle_points_lie_on_the_curve(edges):
    worst = 0.0
    for r, box, R, a, b, word, row, px, py in edges:
        assert len(px) >= 2
        d = float(ref.curve_distance(row, px, py).max()) / max(1.0, box)
        worst = max(worst, d)
        assert d <= TOL, (a, b)
    print(f"kept points: worst {worst:.3g} x max(1, box) off the curve")


def _rows(edges, n=40):
    """a few multi-edge rows: consecutive random edges chained as a row (each edge starts from its
    own pose, as a planned chain's do)"""
    rows = []
    for i in range(0, n * 3, 3):
        parts = [edges[i + j][6] for j in range(3)]
        rows.append({f: np.concatenate([p[f] for p in parts]) for f in ref.FIELDS})
    return rows


def test_sampler_identities(edges):
    for row in _rows(edges):
        L = ref.row_length(row)
        for ds in (0.1, 0.73, 2.0 * L):
            x, y, yaw, kappa, s = ref.sample_row(row, ds)
            nf = math.floor(L / ds)
            assert len(x) == nf + 1 + (1 if L > nf * ds else 0)
            assert x[0] == row["x"][0] and y[0] == row["y"][0] and yaw[0] == row["yaw"][0]
            assert s[0] == 0.0 and s[-1] == L and np.all(np.diff(s) > 0.0)
            ex, ey, eyaw = ref.row_end(row)
            assert x[-1] == ex and y[-1] == ey and yaw[-1] == eyaw
            # consecutive samples on one edge are at most ds apart in chord (a chord is no longer
            # than its arc); across an edge junction the chain jumps to the next stored pose
            e = np.searchsorted(np.cumsum(row["len"]).reshape(-1, 3)[:, 2], s, side="right")
            same = e[1:] == e[:-1]
            chord = np.hypot(np.diff(x), np.diff(y))
            assert np.all(chord[same] <= ds * (1.0 + 1e-12) + 1e-12)
            assert set(np.unique(kappa)) <= set(np.unique(row["kappa"]))


def test_reverse_twice_is_the_same_geometry(edges):
    for row in _rows(edges, 20):
        rr = ref.reverse_row(row)
        assert np.array_equal(rr["len"], row["len"][::-1])
        assert np.array_equal(np.sign(rr["kappa"]), -np.sign(row["kappa"][::-1]))
        # the reversed row starts where the row ends, heading the other way
        ex, ey, eyaw = ref.row_end(row)
        assert rr["x"][0] == ex and rr["y"][0] == ey and rr["yaw"][0] == eyaw + math.pi
        back = ref.reverse_row(rr)
        scale = max(1.0, float(np.max(np.abs(row["x"]))), float(np.max(np.abs(row["y"]))))
        for f in ("x", "y"):
            assert np.max(np.abs(back[f] - row[f])) <= TOL * scale
        assert np.max(np.abs(back["yaw"] - (row["yaw"] + 2.0 * math.pi))) <= TOL
        assert np.array_equal(back["kappa"], row["kappa"]) and np.array_equal(back["len"], row["len"])
        # ... and sampled from either end it is the same set of points
        L = ref.row_length(row)
        ds = L / 7.5
        fx, fy = ref.sample_row(row, ds)[:2]
        assert np.max(ref.curve_distance(rr, fx, fy)) <= TOL * scale


def test_hand_built_rows():
    R = 2.0
    circle = {"x": np.array([1.0]), "y": np.array([2.0]), "yaw": np.array([0.5]),
              "kappa": np.array([1.0 / R]), "len": np.array([2.0 * math.pi * R])}
    x, y, yaw, kappa, s = ref.sample_row(circle, 0.37)
    assert abs(x[-1] - 1.0) <= 1e-12 and abs(y[-1] - 2.0) <= 1e-12
    assert yaw[-1] == 0.5 + (1.0 / R) * (2.0 * math.pi * R)
    cx, cy = 1.0 - math.sin(0.5) * R, 2.0 + math.cos(0.5) * R
    assert np.max(np.abs(np.hypot(x - cx, y - cy) - R)) <= 1e-12
    line = {"x": np.array([0.0]), "y": np.array([0.0]), "yaw": np.array([math.pi / 2]),
            "kappa": np.array([0.0]), "len": np.array([1.0])}
    x, y, yaw, kappa, s = ref.sample_row(line, 0.25)
    assert list(s) == [0.0, 0.25, 0.5, 0.75, 1.0] and np.allclose(y, s) and np.all(kappa == 0.0)
    zero = {f: np.zeros(3) for f in ref.FIELDS}
    zero["x"][:] = [1.0, 2.0, 3.0]
    x, y, yaw, kappa, s = ref.sample_row(zero, 0.5)
    assert list(x) == [3.0] and list(s) == [0.0]  # no s < P: the last segment at its end
    empty = {f: np.zeros(0) for f in ref.FIELDS}
    assert all(len(a) == 0 for a in ref.sample_row(empty, 0.5))

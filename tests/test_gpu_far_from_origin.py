"""GPU parity far from the origin: shifted, scaled and thin scenes (tests/scene_xform.py).

Every fast path decides in f32 first and falls back to exact f64 arithmetic inside a rounding
margin computed from the scene's coordinate magnitude mx (scene::cull_slack_for, eps_coord, the
pair grid's slack, the Morton binning of samples_role, the grid raster's corner widening,
star_chord_lb), each with an absolute floor sized for |c| <= 2^10.  The other GPU files stay in
[-6, 2048]; here the same workloads run under the transforms of XF and must still equal the
sequential oracle run ON THE SAME TRANSFORMED SCENE — node x and y, parents, nearest indices and
accept flags exactly, yaws within ANG_TOL (the conventions of tests/test_gpu_parity.py).  Under
the power-of-two scales the GPU's tree must also equal the GPU's own base tree times s (the
exact symmetry pinned on the oracle by tests/test_scene_xform_oracle.py).

Tolerances that are not exact: a Dubins point's world transform (x0 + local * R rotated) rounds
at the ulp of the coordinate, on the GPU (ocml) and in the oracle (glibc) alike, so line points
are compared within PTS_TOL(raw) = max(PT_TOL, 8 ulp(mx)) and lengths within that times the point
count (8 ulp: the rotate-scale-add of a point is a handful of roundings at the coordinate's
magnitude).  RRT* costs: tests/test_gpu_rrtstar.py's rule (1e-9 relative).
"""
import functools
import math

import numpy as np
import pytest

import star_goal_ref
import star_revalidate_ref
from scene_xform import moved
from star_tree_cases import _set_space_checked
from star_tree_cases import _trees as _star_trees
from test_gpu_parity import ANG_TOL, PT_TOL, _assert_same_tree, _planner
from test_gpu_rrtstar import COST_RTOL
from test_gpu_rrtstar import _assert_same as _assert_same_star
from test_gpu_rrtstar import _batch as _star_batch
from test_gpu_rrtstar import _oracle as _star_oracle
from test_gpu_star_repair import _repair_checked

pytestmark = pytest.mark.gpu

# id -> (dx, dy, s)
XF = {
    "pow2_shift": (2.0 ** 20, -(2.0 ** 21), 1.0),  # mx 2000 x the floors' range, mixed signs
    "utm": (4.0e6 + 0.3, 5.0e5 + 0.7, 1.0),        # a projected map frame, not f32-representable
    "negative": (-3.0e4, -3.0e4, 1.0),             # everything in the third quadrant
    "blind": (2.0 ** 30, 2.0 ** 30, 1.0),          # f32 ulp 128: every f32 screen is blind
    "s-20": (0.0, 0.0, 2.0 ** -20),
    "s-10": (0.0, 0.0, 2.0 ** -10),
    "s+10": (0.0, 0.0, 2.0 ** 10),
    "s+20": (0.0, 0.0, 2.0 ** 20),
}
ALL = list(XF)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2(pkg):
    """a second context: Space.verify_batch and the batches (a context holds one scene)"""
    c = pkg.Context(0)
    yield c
    c.close()


def _thin(discs):
    """bounds 4096 x 6: samples_role's 16 x 16 Morton grid degenerates to one row and a sorted
    block of 256 samples is a strip, not a compact tile.  With ``discs``: 64 discs of radius 0.5
    on the centre line (inflated to 1.0: two lanes of 1.5 remain beside each)"""
    c = [(64.0 * i + 32.0, 3.0, 0.5) for i in range(64)] if discs else []
    return {"name": "thin_discs" if discs else "thin", "bounds": (0.0, 0.0, 4096.0, 6.0),
            "robot": (1.0, 1.0, 0.8), "circles": np.array(c, dtype=np.float64).reshape(-1, 3),
            "start": (2.0, 3.0, 0.0), "goal": (4090.0, 3.0, 0.0), "max_iter": 8192,
            "step_size": 0.1}


@functools.lru_cache(maxsize=None)
def _scene(name, xid):
    """the (read-only) transformed scene; xid None: the base scene"""
    from pathplanning_amd import scenes

    if name in ("thin", "thin_discs"):
        raw = _thin(name == "thin_discs")
    else:
        raw = getattr(scenes, name)()
    return raw if xid is None else moved(raw, *XF[xid])


@functools.lru_cache(maxsize=None)
def _oracle_run(name, xid, seed, n_iter):
    """(OracleScene, OracleTree after the run, accepted, nearest log, accept log)"""
    import oracle

    raw = _scene(name, xid)
    sc = oracle.OracleScene.from_raw(raw)
    tr = oracle.OracleTree(raw["start"], n_iter + 1)
    acc, nn, la = oracle.rrt_extend(sc, tr, seed, 0, n_iter)
    return sc, tr, acc, nn, la


@functools.lru_cache(maxsize=None)
def _queries(name, xid, nq):
    """config 3's first nq queries of the BASE scene (starts[nq, 3], goals[nq, 3], seeds), their
    poses moved with the scene: scenes.config3_queries keeps poses 1.0 (an absolute length) clear
    of the discs, so on a scene scaled far down it would never find a free pose"""
    from pathplanning_amd import scenes

    starts, goals, seeds = scenes.config3_queries(_scene(name, None), 0, nq)
    if xid is not None:
        dx, dy, s = XF[xid]
        for a in (starts, goals):
            a[:, 0] = a[:, 0] * s + dx
            a[:, 1] = a[:, 1] * s + dy
    return starts, goals, seeds


_GPU_BASE = {}


def _gpu_base(pkg, ctx, name, seed, n_iter, window):
    """the GPU's own tree (and stats) on the base scene, grown once per recipe"""
    key = (name, seed, n_iter, window)
    if key not in _GPU_BASE:
        p = _planner(pkg, _scene(name, None), seed, window, ctx)
        p.reset_stats()
        p.extend(n_iter)
        _GPU_BASE[key] = (p.tree(), p.stats())
    return _GPU_BASE[key]


def _mx(raw):
    return float(np.max(np.abs(raw["bounds"])))


def PTS_TOL(raw):
    return max(PT_TOL, 8.0 * float(np.spacing(_mx(raw))))


def _assert_scaled(got, base, s):
    """got == base * s: x, y and parents exactly, yaw within ANG_TOL"""
    x, y, yaw, par = got[:4]
    bx, by, byaw, bpar = base[:4]
    assert len(x) == len(bx), (len(x), len(bx))
    assert np.array_equal(x, bx * s) and np.array_equal(y, by * s)
    assert np.array_equal(par, bpar)
    assert np.max(np.abs(yaw - byaw), initial=0.0) <= ANG_TOL


def _one_tree(pkg, ctx, name, xid, seed, n_iter, window, min_nodes):
    """grow on the GPU, compare with the oracle (and under a scale with the GPU's base tree);
    returns (planner, oracle run, stats)"""
    raw = _scene(name, xid)
    sc, tr, acc, _, _ = _oracle_run(name, xid, seed, n_iter)
    assert tr.n >= min_nodes, tr.n  # the case cannot pass on an empty tree
    scaled = xid is not None and XF[xid][2] != 1.0
    if scaled:  # (first: the base planner takes the context's scene and tree)
        base, _ = _gpu_base(pkg, ctx, name, seed, n_iter, window)
    p = _planner(pkg, raw, seed, window, ctx)
    p.reset_stats()
    assert p.extend(n_iter) == acc
    assert p.iteration() == n_iter
    got = p.tree()
    _assert_same_tree(got, tr.arrays())
    st = p.stats()
    if scaled:
        _assert_scaled(got, base, XF[xid][2])
    screened = st["samples_evaluated"] - st["samples_blocked"]
    print(f"FAR one-tree {name} {xid} window {window}: nodes {tr.n} nn_flagged "
          f"{st['nn_flagged']} of {screened} screened samples")
    return p, (sc, tr), st


# ------------------------------------------------------------------------------- one tree
@pytest.mark.parametrize("window", [7, 4096])
@pytest.mark.parametrize("xid", ALL)
def test_bench6_one_tree(pkg, ctx, xid, window):
    """bench6, seed 7, 3000 iterations: the oracle inserts 1664 nodes (1665 with the root) under
    every transform."""
    _one_tree(pkg, ctx, "bench6", xid, 7, 3000, window, 1000)


FIELD_ITERS = 16384


@pytest.mark.parametrize("xid", ALL)
def test_field512_one_tree(pkg, ctx, xid):
    """field512, seed 42, window 4096, 16384 iterations: test_field512_config2_parity's 40000 cut
    down to the smallest multiple of 4096 at which the oracle's tree has at least 2000 nodes
    (4096: 80, 8192: 660, 12288: 1649, 16384: 2752 nodes with the root) — more than one screen
    chunk plus appended nodes.  The oracle's run takes 0.6 s, the slowest oracle run of this
    file beside bench6_polygons' (1.5 s).

    nn_flagged: under ``blind`` the f32 ulp (128) is a quarter of the field and eps_coord = 128,
    so every margin exceeds the node spacing and every screened sample (samples_evaluated -
    samples_blocked) must be flagged and decided by the f64 paths.  The counter adds a sample
    once per nn_finalize pass (a window cut short by a commit finalizes its tail again), so the
    figure to hold is nn_flagged >= screened, not equality; the base scene must stay below its
    screened count and below the blind figure.  Measured on one MI355X: blind 34361 flagged of
    12308 screened (the f32 obstacle pre-test decides nothing there either, so more samples
    reach the screen), base 16 of 5952.  This case is the one that found nn_finalize's
    expanded-form bound first order in eps_coord: 2863 nodes against the oracle's 2751 before
    the bound's second-order term."""
    p, _, st = _one_tree(pkg, ctx, "field512", xid, 42, FIELD_ITERS, 4096, 2000)
    if xid == "blind":
        _, base = _gpu_base(pkg, ctx, "field512", 42, FIELD_ITERS, 4096)
        screened = st["samples_evaluated"] - st["samples_blocked"]
        bscreened = base["samples_evaluated"] - base["samples_blocked"]
        print(f"FAR field512 base: nn_flagged {base['nn_flagged']} of {bscreened}")
        assert st["nn_flagged"] >= screened, (st["nn_flagged"], screened)
        assert base["nn_flagged"] < bscreened and base["nn_flagged"] < st["nn_flagged"]


# ----------------------------------------------------------------- the query APIs on those trees
def _grazing_lines(raw, osc, s, count, seed):
    """short polylines that graze an inflated disc: tangent at the inflated radius + eps s, eps
    from -1e-9 to 1e-9 (and exactly 0), as 2-point segments and as 3-point lines through the
    tangent point; the oracle decides each, and both verdicts must occur"""
    circ = np.asarray(raw["circles"], dtype=np.float64).reshape(-1, 3)
    half = raw["robot"][0] / 2.0
    rng = np.random.default_rng(seed)
    epss = [0.0, 1e-9, -1e-9, 5e-10, -5e-10, 1e-10, -1e-10, 1e-12, -1e-12]
    lines = []
    while len(lines) < count:
        d = int(rng.integers(0, len(circ)))
        cx, cy, rr = circ[d, 0], circ[d, 1], circ[d, 2] + half
        a = rng.uniform(-math.pi, math.pi)
        rho = rr + epss[len(lines) % len(epss)] * s
        tx, ty = cx + rho * math.cos(a), cy + rho * math.sin(a)
        ux, uy = -math.sin(a), math.cos(a)
        l0, l1 = rng.uniform(0.05, 1.5, 2) * s
        pts = [(tx - l0 * ux, ty - l0 * uy), (tx + l1 * ux, ty + l1 * uy)]
        if len(lines) % 2:
            pts.insert(1, (tx, ty))
        lines.append(np.array(pts))
    exp = np.array([osc.verify_line(l[:, 0], l[:, 1]) for l in lines])
    return lines, exp


@pytest.mark.parametrize("xid", ["utm", "blind", "s-20"])
@pytest.mark.parametrize("name,seed,n_iter", [("bench6", 7, 3000), ("field512", 42, FIELD_ITERS)])
def test_query_apis(pkg, ctx, ctx2, oracle_mod, name, seed, n_iter, xid):
    from pathplanning_amd import rrt

    raw = _scene(name, xid)
    s = XF[xid][2]
    p, (sc, otr), _ = _one_tree(pkg, ctx, name, xid, seed, n_iter, 4096, 1000)
    x, y, yaw, par = p.tree()
    n = len(x)
    x0, y0, x1, y1 = raw["bounds"]
    rng = np.random.default_rng(5)
    # ---- get_nearest_node_batch: 4096 points, half of them node copies and one-ulp near-copies
    qx = rng.uniform(x0, x1, 4096)
    qy = rng.uniform(y0, y1, 4096)
    pick = rng.integers(0, n, 2048)
    qx[:2048], qy[:2048] = x[pick], y[pick]
    qx[1024:1536] = np.nextafter(qx[1024:1536], np.inf)
    qy[1536:2048] = np.nextafter(qy[1536:2048], -np.inf)
    idx, d2 = p.get_nearest_node_batch(qx, qy)
    for i in range(len(qx)):
        ei, ed2 = oracle_mod.nearest(x, y, qx[i], qy[i])
        assert idx[i] == ei and d2[i] == ed2, (i, idx[i], ei, d2[i], ed2)
    # ---- verify_node_batch: random candidates and parents, some exactly on their parent
    half = raw["robot"][0] / 2.0
    k = 600
    cx = rng.uniform(x0 + half, x1 - half, k)
    cy = rng.uniform(y0 + half, y1 - half, k)
    cp = rng.integers(0, n, k).astype(np.int32)
    cx[:20], cy[:20] = x[cp[:20]], y[cp[:20]]
    ok, gyaw = p.verify_node_batch(cx, cy, cp)
    for i in range(k):
        eok, eyaw = oracle_mod.verify_candidate(sc, otr, cx[i], cy[i], int(cp[i]))
        assert ok[i] == eok, i
        assert abs(gyaw[i] - eyaw) <= ANG_TOL
    assert 0 < int(ok.sum()) < k
    # ---- space_verify_batch: polylines that graze a disc, the oracle's verdict on each
    lines, exp = _grazing_lines(raw, sc, s, 900, 3)
    assert 0 < int(exp.sum()) < len(exp), int(exp.sum())
    got = rrt.Space.from_raw(raw).verify_batch(lines, ctx2)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), bad[:10])
    print(f"FAR queries {name} {xid}: {n} nodes, {int(ok.sum())} of {k} candidates verify, "
          f"{int(exp.sum())} of {len(exp)} grazing lines verify")


# ------------------------------------------------------------------------------ a thin scene
@pytest.mark.parametrize("xid", [None, "utm"], ids=["plain", "utm"])
@pytest.mark.parametrize("name", ["thin", "thin_discs"])
def test_thin_scene(pkg, ctx, name, xid):
    """4096 x 6, seed 7, 8192 iterations, window 4096: the oracle's tree holds 6034 nodes without
    and 5553 with the discs, plain and under utm (more nodes than one window)"""
    _one_tree(pkg, ctx, name, xid, 7, 8192, 4096, THIN_MIN[name])


THIN_MIN = {"thin": 4096, "thin_discs": 4096}


# -------------------------------------------------------------------------------- grid mode
@pytest.mark.parametrize("window", [64, 4096])
@pytest.mark.parametrize("xid", ["pow2_shift", "utm", "s-10"])
def test_field512_grid(pkg, ctx, xid, window):
    """test_field512_grid_parity_40k's seed 42 cut to 12288 iterations, the smallest multiple of
    4096 that still inserts at least 1000 nodes (8192: 601, 12288: 1567 with the root)"""
    _one_tree(pkg, ctx, "field512_grid", xid, 42, 12288, window, 1000)


# --------------------------------------------------------------------------------- polygons
@pytest.mark.parametrize("xid", ["utm", "negative", "s+10"])
@pytest.mark.parametrize("name", ["transit", "bench6_polygons"])
def test_polygons(pkg, ctx, name, xid):
    """seed 7, 2000 iterations, window 4096"""
    _one_tree(pkg, ctx, name, xid, 7, 2000, 4096, 500)


# ---------------------------------------------------------------------------- goal connection
@pytest.mark.parametrize("xid", ["utm", "s-10"])
def test_goal_connection(pkg, ctx, oracle_mod, xid):
    """bench6_open, seed 3, 2000 iterations: check_finish_batch over every node against
    oracle.check_finish — ok, the chains and the point counts exactly, the line points of 32
    finishing nodes within PTS_TOL and every length within PTS_TOL times the point count.
    1090 nodes, 167 finish.  Measured: worst point error 0 (utm) and 1.5e-17 (s-10), worst length
    error per point 1.6e-17 and 7.3e-20, against tolerances of 3.7e-9 and 1e-9: the bound of the
    issue holds as it stands, no wider one was needed."""
    raw = _scene("bench6_open", xid)
    p, (sc, otr), _ = _one_tree(pkg, ctx, "bench6_open", xid, 3, 2000, 4096, 500)
    n = otr.n
    nodes = np.arange(1, n, dtype=np.int32)
    r = p.check_finish_batch(nodes)
    goal, gyaw = raw["goal"][:2], raw["goal"][2]
    fin = [oracle_mod.check_finish(sc, otr, int(v), goal, gyaw) for v in nodes]
    assert [bool(v) for v in r["ok"]] == [f["ok"] for f in fin]
    n_ok = sum(f["ok"] for f in fin)
    assert 16 <= n_ok < len(fin), n_ok
    tol = PTS_TOL(raw)
    worst = 0.0
    for i, f in enumerate(fin):
        levels = int(r["chain"][i, 0])
        assert r["chain"][i, 2:2 + levels].tolist() == f["chain"], int(nodes[i])
        if f["ok"]:
            assert r["n_points"][i] == f["n"], int(nodes[i])
            worst = max(worst, abs(r["length"][i] - f["length"]) / f["n"])
            assert abs(r["length"][i] - f["length"]) <= tol * f["n"], int(nodes[i])
    oks = [i for i, f in enumerate(fin) if f["ok"]]
    worst_pt = 0.0
    for i in oks[::max(1, len(oks) // 32)][:32]:
        line = p.check_finish(int(nodes[i]))
        assert line is not None and line.shape == (fin[i]["n"], 2)
        e = max(np.max(np.abs(line[:, 0] - fin[i]["x"])), np.max(np.abs(line[:, 1] - fin[i]["y"])))
        worst_pt = max(worst_pt, e)
        assert e <= tol, (int(nodes[i]), e, tol)
    print(f"FAR goal {xid}: {n} nodes, {n_ok} finish, worst point error {worst_pt:.3g}, worst "
          f"length error per point {worst:.3g} (tolerance {tol:.3g})")


# ------------------------------------------------------------------------------------ batch
BATCH_Q, BATCH_ITERS = 32, 300


@functools.lru_cache(maxsize=None)
def _batch_case(name, xid, nq, n_iter):
    """(raw, starts, goals, seeds, per query (OracleScene, OracleTree, best node, best length,
    finishes, points of the best line)): every query's independent oracle plan run"""
    import oracle
    raw = _scene(name, xid)
    starts, goals, seeds = _queries(name, xid, nq)
    sc = oracle.OracleScene.from_raw(raw)
    exp = []
    for q in range(nq):
        tr = oracle.OracleTree(tuple(starts[q]), n_iter + 1)
        acc, bn, bl, log = oracle.plan(sc, tr, int(seeds[q]), 0, n_iter, goals[q][:2], goals[q][2])
        line = oracle.check_finish(sc, tr, bn, goals[q][:2], goals[q][2]) if bn >= 0 else None
        exp.append((tr, bn, bl, int((log == 1).sum()), line))
    return raw, starts, goals, seeds, exp


def _batch_checked(ctx, name, xid, window, with_paths, max_flips=0):
    """max_flips: the one-point libm trim flips allowed (tests/test_gpu_batch_plan.py: a query
    whose best line has one arc point more or less than the oracle's, its length one chord
    2 R sin(step / 2) off; such a row is counted, not compared point by point)"""
    from pathplanning_amd import rrt

    raw, starts, goals, seeds, exp = _batch_case(name, xid, BATCH_Q, BATCH_ITERS)
    b = rrt.RRTBatch(starts, goals, BATCH_ITERS, raw["step_size"], rrt.Space.from_raw(raw), seeds,
                     ctx=ctx, window=window)
    it, acc = b.extend(BATCH_ITERS)
    n, its = b.state()
    assert it == BATCH_Q * BATCH_ITERS and (its == BATCH_ITERS).all()
    assert acc == sum(e[0].n - 1 for e in exp)
    for q in range(BATCH_Q):
        _assert_same_tree(b.tree(q), exp[q][0].arrays())
    # ---- plan() against oracle.plan
    tol = PTS_TOL(raw)
    chord = 2.0 * raw["robot"][2] * math.sin(raw["step_size"] / 2.0)
    got = b.plan()
    flipped = set()
    for q, (tr, bn, bl, nf, line) in enumerate(exp):
        assert got["best_node"][q] == bn and got["n_finishes"][q] == nf, q
        if bn < 0:
            assert math.isinf(got["length"][q]) and got["n_points"][q] == 0
            continue
        if got["n_points"][q] != line["n"]:
            assert abs(int(got["n_points"][q]) - line["n"]) == 1, q
            assert abs(abs(got["length"][q] - bl) - chord) <= 1e-6 * chord, q
            flipped.add(q)
            continue
        assert abs(got["length"][q] - bl) <= tol * line["n"], q
    fin = sum(1 for e in exp if e[1] >= 0)
    print(f"FAR batch {name} {xid} window {window}: {int(n.sum())} nodes, {fin} queries finish, "
          f"{len(flipped)} one-point flips")
    assert len(flipped) <= max_flips, sorted(flipped)
    if with_paths:
        off, xy, ok = b.paths()
        assert off[0] == 0 and off[-1] == len(xy)
        for q, (tr, bn, bl, nf, line) in enumerate(exp):
            row = xy[off[q]:off[q + 1]]
            assert bool(ok[q]) == (bn >= 0) and (len(row) > 0) == (bn >= 0), q
            if bn >= 0 and q in flipped:
                assert len(row) == got["n_points"][q], q
            elif bn >= 0:
                assert row.shape == (line["n"], 2), q
                assert np.max(np.abs(row[:, 0] - line["x"])) <= tol, q
                assert np.max(np.abs(row[:, 1] - line["y"])) <= tol, q
    return fin


@pytest.mark.parametrize("window", [1, 32])
@pytest.mark.parametrize("xid", ["utm", "blind"])
def test_batch_field512(pkg, ctx2, xid, window):
    """32 queries x 300 iterations on field512: every tree against its independent oracle run,
    plan() against oracle.plan, and under utm paths() against the oracle's lines"""
    _batch_checked(ctx2, "field512", xid, window, xid == "utm")


def test_batch_bench6_open_paths_utm(pkg, ctx2):
    """the same on bench6_open, where 29 of the 32 queries finish (on the field's 300 iterations
    one does): plan() and paths() compare real lines.  Flips: tests/test_gpu_batch_plan.py's rule
    for a recipe without a committed measurement, max(1, finishing queries // 10) = 2"""
    assert _batch_checked(ctx2, "bench6_open", "utm", 32, True, max_flips=2) >= 16


# ------------------------------------------------------------------------------------- RRT*
STAR_Q, STAR_ITERS = 16, 400
_STAR_BASE = {}


@functools.lru_cache(maxsize=None)
def _star_queries(name, xid):
    return _queries(name, xid, STAR_Q)


def _star_grown(pkg, ctx, name, xid, eta_unit):
    raw = _scene(name, xid)
    s = 1.0 if xid is None else XF[xid][2]
    starts, _, seeds = _star_queries(name, xid)
    b = _star_batch(pkg, raw, starts, seeds, STAR_ITERS, 0, eta_unit * s, ctx=ctx)
    b.extend(STAR_ITERS)
    return b, raw, starts, seeds, s


@pytest.mark.parametrize("xid", ["utm", "s-20", "s+20"])
@pytest.mark.parametrize("eta_unit", [0.0, 2.0])
@pytest.mark.parametrize("name", ["bench6", "field512"])
def test_rrtstar(pkg, ctx2, oracle_mod, name, eta_unit, xid):
    """16 queries x 400 iterations, k = 0, Steer eta 0 and 2 s: parents, poses and rewires
    exact, costs by tests/test_gpu_rrtstar.py's rule.  (``blind`` is not in the list: its first
    run, bench6 with eta 0, did not return on the GPU and the cause is not found — DESIGN.md §4;
    the case comes back with the cause.)"""
    b, raw, starts, seeds, s = _star_grown(pkg, ctx2, name, xid, eta_unit)
    n, it, _, rw = b.state()
    assert (it == STAR_ITERS).all()
    trees = [b.tree(q, n[q]) for q in range(STAR_Q)]
    for q in range(STAR_Q):
        exp, erw = _star_oracle(oracle_mod, raw, tuple(starts[q]), int(seeds[q]), STAR_ITERS, 0,
                                eta_unit * s)
        _assert_same_star(trees[q], exp)
        assert rw[q] == erw, q
    print(f"FAR rrtstar {name} eta {eta_unit} {xid}: {int(n.sum())} nodes, {int(rw.sum())} rewires")
    assert int(n.sum()) >= (2000 if name == "bench6" else 100)
    if s != 1.0:
        key = (name, eta_unit)
        if key not in _STAR_BASE:
            bb, _, bstarts, _, _ = _star_grown(pkg, ctx2, name, None, eta_unit)
            bn = bb.state()[0]
            _STAR_BASE[key] = (bstarts, [bb.tree(q, bn[q]) for q in range(STAR_Q)])
        bstarts, base = _STAR_BASE[key]
        assert np.array_equal(np.asarray(starts)[:, :2], np.asarray(bstarts)[:, :2] * s)
        for q in range(STAR_Q):
            _assert_scaled(trees[q], base[q], s)
            assert np.allclose(trees[q][4], base[q][4], rtol=COST_RTOL, atol=0.0)


def test_rrtstar_scene_change_utm(pkg, ctx2, oracle_mod):
    """bench6 under utm, 16 queries x 400 iterations, eta 2: plan and paths against
    tests/star_goal_ref.py, then one disc of r 0.3 on the n/4-subtree node of tree 0:
    revalidate and repair(rounds = 1) on twin batches against tests/star_revalidate_ref.py and
    tests/star_repair_ref.py"""
    from pathplanning_amd import rrt

    a, raw, starts, seeds, _ = _star_grown(pkg, ctx2, "bench6", "utm", 2.0)
    twin, _, _, _, _ = _star_grown(pkg, None, "bench6", "utm", 2.0)  # (its own context)
    try:
        before = _star_trees(a)
        for t, u in zip(before, _star_trees(twin)):
            for c, d in zip(t, u):
                assert np.array_equal(c, d)
        # ---- the goal connection
        osc = oracle_mod.OracleScene.from_raw(raw)
        goal = raw["goal"]
        tol = PTS_TOL(raw)
        node, cost = a.plan(goal)
        off, xy, length, ok = a.paths(goal, node)
        assert np.array_equal(ok, node >= 0) and (node >= 0).any()
        for q in range(STAR_Q):
            enode, ecost, etotal = star_goal_ref.plan(osc, before[q], goal)
            assert node[q] == enode, (q, node[q], enode, star_goal_ref.runner_up_gap(etotal))
            if enode < 0:
                assert cost[q] == np.inf
                continue
            assert abs(cost[q] - ecost) <= COST_RTOL * ecost
            exy, elen = star_goal_ref.path(osc, before[q], goal, enode)
            row = xy[off[q]:off[q + 1]]
            assert row.shape == exy.shape, q
            assert np.max(np.abs(row - exy)) <= tol, q
            assert abs(length[q] - elen) <= tol * len(exy), q
        # ---- one added disc: revalidate on a, repair(1) on the twin
        v = star_revalidate_ref.quarter_subtree_node(before[0])
        raw2 = star_revalidate_ref.with_discs(raw, [(before[0][0][v], before[0][1][v], 0.3)])
        _, exp = _set_space_checked(oracle_mod, a, before, raw2)
        r = exp[0]
        assert not r["keep"][v] and 1 < r["kept"] < len(before[0][0]), r
        assert r["failed"] > 0 and r["orphans"] > 0, r
        _, rexp = _repair_checked(oracle_mod, twin, before, raw2, 0, 1)
        assert rexp[0]["reattached"] > 0 and rexp[0]["recovered"] > rexp[0]["reattached"], rexp[0]
        print(f"FAR rrtstar scene change utm: tree 0 keeps {r['kept']} of {len(before[0][0])}, "
              f"repair recovers {rexp[0]['recovered']}")
    finally:
        twin.close()


# --------------------------------------------------------- a tree kept across a move of nothing
@pytest.mark.parametrize("xid", ["utm", "blind"])
def test_set_space_same_scene_is_the_identity(pkg, ctx, ctx2, xid):
    """set_space with the same transformed scene drops nothing: one tree (field512, 16384
    iterations) and the batch (32 x 300)"""
    from pathplanning_amd import rrt

    raw = _scene("field512", xid)
    p, _, _ = _one_tree(pkg, ctx, "field512", xid, 42, FIELD_ITERS, 4096, 2000)
    before = p.tree()
    n = len(before[0])
    for call in (p.revalidate, lambda: p.set_space(rrt.Space.from_raw(raw))):
        kept, new_index = call()
        assert kept == n == p.tree_size() and p.iteration() == FIELD_ITERS
        assert np.array_equal(new_index, np.arange(n))
        for a, e in zip(p.tree(), before):
            assert np.array_equal(a, e)
    _, starts, goals, seeds, exp = _batch_case("field512", xid, BATCH_Q, BATCH_ITERS)
    b = rrt.RRTBatch(starts, goals, BATCH_ITERS, raw["step_size"], rrt.Space.from_raw(raw), seeds,
                     ctx=ctx2)
    b.extend(BATCH_ITERS)
    n_old = b.state()[0]
    whole = [b.tree(q, n_old[q]) for q in range(BATCH_Q)]
    n_new, new_index = b.set_space(rrt.Space.from_raw(raw))
    assert np.array_equal(n_new, n_old) and b.last_dropped == 0
    assert np.array_equal(new_index, np.concatenate([np.arange(k) for k in n_old]))
    for q in range(BATCH_Q):
        for a, e in zip(b.tree(q, n_new[q]), whole[q]):
            assert np.array_equal(a, e)
        _assert_same_tree(whole[q], exp[q][0].arrays())

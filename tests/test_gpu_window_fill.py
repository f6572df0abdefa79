"""A window is filled with K screened samples, not K iterations (csrc/pp_window_fill.h) — on the
device: ``extend_samples`` streams whose draws in an obstacle (the pre-test settles them where they
are drawn; they take no sample id) sit on every edge of the span rule, against the oracle's
sequential run over the same stream.

Free points lie >= 0.05 clear of every inflated disc, blocked ones within 0.25 of the centre of a
disc of inflated radius >= 4.5 (the pre-test's cells there lie wholly inside), as in
test_gpu_screen_tiling.  Exact: x, y, parent, the per-iteration verdicts, the iteration and
blocked counters.  Within 1e-9: yaw (ocml vs glibc atan2)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import ANG_TOL, _assert_same_tree, _planner

pytestmark = pytest.mark.gpu

K = 64


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _grow(pkg, raw, ctx):
    p = _planner(pkg, raw, 21, 4096, ctx)
    while p.tree_size() < 10000:
        p.extend(4096)
    return p


@pytest.fixture(scope="module")
def field(pkg, ctx):
    """field512, a planner on it grown to about 10k nodes, that tree, and pools of free and
    blocked points"""
    from pathplanning_amd import rrt, scenes

    raw = scenes.field512()
    p = _grow(pkg, raw, ctx)
    tree = p.tree()
    sp = rrt.Space.from_raw(raw)
    x0, x1, y0, y1 = sp.get_bounds()
    obs = sp.get_obs()  # (cx, cy, r + width / 2)
    rng = np.random.default_rng(17)
    pts = np.column_stack([rng.uniform(x0, x1, 40000), rng.uniform(y0, y1, 40000)])
    clear = np.concatenate([  # distance to the nearest inflated disc's rim, 4000 points at a time
        np.min(np.hypot(c[:, None, 0] - obs[None, :, 0], c[:, None, 1] - obs[None, :, 1])
               - obs[None, :, 2], axis=1) for c in np.split(pts, 10)])
    free = pts[clear > 0.05]
    big = obs[(obs[:, 2] >= 4.5) & (obs[:, 0] > x0 + 1.0) & (obs[:, 0] < x1 - 1.0)
              & (obs[:, 1] > y0 + 1.0) & (obs[:, 1] < y1 - 1.0)]  # (the pre-test covers the box)
    pick = big[rng.integers(0, len(big), 20000)]
    inside = pick[:, :2] + rng.uniform(-0.25, 0.25, (20000, 2))
    # a spot with 2.0 of clearance, far from the start: where the truncation test puts clusters
    far = pts[(clear > 2.0) & (np.hypot(pts[:, 0] - raw["start"][0], pts[:, 1] - raw["start"][1]) > 60.0)]
    assert len(free) > 20000 and len(far) >= 4
    return {"raw": raw, "p": p, "tree": tree, "free": free, "inside": inside, "far": far}


def _stream(field, live, rng):
    """the samples of a mask: live[i] — a free point, else a blocked one (fresh points each call)"""
    live = np.asarray(live, dtype=bool)
    s = np.empty((len(live), 2))
    nf, nb = int(live.sum()), int((~live).sum())
    s[live] = field["free"][rng.choice(len(field["free"]), nf, replace=False)]
    s[~live] = field["inside"][rng.choice(len(field["inside"]), nb, replace=False)]
    return np.ascontiguousarray(s[:, 0]), np.ascontiguousarray(s[:, 1])


def _extend_ok(pkg, p, sx, sy):
    """pp_rrt_extend_samples asking for the verdicts alone: the record that leaves the pre-test on
    (a nearest node or a yaw per iteration turns it off)"""
    ok = np.full(len(sx), 7, dtype=np.uint8)
    acc = C.c_int64(0)
    dp = C.POINTER(C.c_double)
    pkg._ffi.check(pkg._ffi.lib().pp_rrt_extend_samples(
        p.ctx.handle, sx.ctypes.data_as(dp), sy.ctypes.data_as(dp), len(sx), None, None,
        ok.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(acc)))
    return acc.value, ok


def _oracle(oracle_mod, raw, tree, cap=1 << 17):
    tr = oracle_mod.OracleTree(raw["start"], cap)
    x, y, yaw, par = tree
    n = len(x)
    tr.x[:n], tr.y[:n], tr.yaw[:n], tr.parent[:n] = x, y, yaw, par
    tr._c.n = n
    return tr


def _masks():
    rng = np.random.default_rng(3)

    def scattered(n, n_live):
        m = np.zeros(n, dtype=bool)
        m[rng.choice(n, n_live, replace=False)] = True
        return m

    one, zero = np.ones, np.zeros
    cases = {
        # live counts of K - 1, K and K + 1 inside 2 K draws
        "live_K-1_in_2K": scattered(2 * K, K - 1),
        "live_K_in_2K": scattered(2 * K, K),
        "live_K+1_in_2K": scattered(2 * K, K + 1),
        # a stream opening with K, 2 K and 2 K + 1 blocked samples
        "open_K_blocked": np.concatenate([zero(K, bool), one(K + 9, bool)]),
        "open_2K_blocked": np.concatenate([zero(2 * K, bool), one(K + 9, bool)]),
        "open_2K+1_blocked": np.concatenate([zero(2 * K + 1, bool), one(K + 9, bool)]),
        # nothing live for 5 K iterations: every window commits its span without a sample
        "all_blocked_5K": zero(5 * K, bool),
        # a blocked run straddling the 2 K cap of the first window
        "run_straddles_cap": np.concatenate([one(K - 20, bool), zero(K + 40, bool), one(30, bool)]),
        # the (K + 1)-th live draw is draw 2 K - 1, the last a window may make
        "next_on_last_draw": np.concatenate([one(K, bool), zero(K - 1, bool), one(1 + 30, bool)]),
        # ... and draw 2 K, one past it
        "next_past_last_draw": np.concatenate([one(K, bool), zero(K, bool), one(1 + 30, bool)]),
    }
    return cases


MASKS = _masks()


@pytest.mark.parametrize("name", list(MASKS))
def test_span_edges_against_the_oracle(pkg, oracle_mod, field, name):
    raw, p, tree = field["raw"], field["p"], field["tree"]
    live = MASKS[name]
    sx, sy = _stream(field, live, np.random.default_rng(len(name) + int(live.sum())))
    sc = oracle_mod.OracleScene.from_raw(raw)
    tr = _oracle(oracle_mod, raw, tree)
    oacc, onn, oyaw, ook = oracle_mod.rrt_extend_samples(sc, tr, sx, sy)
    assert not np.any(ook[~live])  # (the blocked points are the oracle's rejects too)
    p.set_window(K)
    # the pre-test on: the verdicts alone
    p.tree_import(*tree)
    p.reset_stats()
    it0 = p.iteration()
    acc, ok = _extend_ok(pkg, p, sx, sy)
    st = p.stats()
    print(f"{name}: {len(live)} iterations, {int(live.sum())} live, accepted {acc} (oracle {oacc}), "
          f"windows {st['windows']}, truncations {st['truncations']}, blocked {st['samples_blocked']}")
    assert p.iteration() - it0 == len(live) and st["iterations"] == len(live), st
    assert st["samples_blocked"] == int((~live).sum()), st
    assert acc == oacc
    assert np.array_equal(ok, ook.astype(np.uint8)), np.flatnonzero(ok != ook)[:10]
    _assert_same_tree(p.tree(), tr.arrays())
    # a window holds up to K samples however many iterations it spans, and spans at most 2 K
    assert st["windows"] >= max(-(-len(live) // (2 * K)), -(-int(live.sum()) // K))
    assert st["truncations"] > 0 or st["windows"] <= -(-len(live) // K)
    # the full record (nearest node and yaw of every iteration: no pre-test, K iterations a window)
    p.tree_import(*tree)
    p.reset_stats()
    nn, yaw, ok2 = p.extend_samples(sx, sy)
    assert p.stats()["samples_blocked"] == 0 and p.stats()["iterations"] == len(live)
    assert np.array_equal(nn, onn) and np.array_equal(ok2, ook.astype(bool))
    assert np.max(np.abs(yaw - oyaw)) <= ANG_TOL
    _assert_same_tree(p.tree(), tr.arrays())


def test_full_windows_of_4096_span_more_iterations(pkg, oracle_mod, field):
    """K = 4096, about 32 % of the draws blocked, one call of 3 K + 5 iterations on the grown
    planner (its windows are K samples by then): fewer windows than ceil((3 K + 5) / K)"""
    raw, tree = field["raw"], field["tree"]
    Kb = 4096
    n = 3 * Kb + 5
    rng = np.random.default_rng(32)
    live = rng.uniform(size=n) >= 0.32
    sx, sy = _stream(field, live, rng)
    q = _grow(pkg, raw, None)  # (a context of its own; the same seed and calls: the fixture's tree)
    _assert_same_tree(q.tree(), tree)
    q.reset_stats()
    acc, ok = _extend_ok(pkg, q, sx, sy)
    st = q.stats()
    tr = _oracle(oracle_mod, raw, tree)
    oacc, _, _, ook = oracle_mod.rrt_extend_samples(oracle_mod.OracleScene.from_raw(raw), tr, sx, sy)
    print(f"{n} iterations, {int(live.sum())} live: windows {st['windows']}, truncations "
          f"{st['truncations']}, blocked {st['samples_blocked']}")
    assert st["iterations"] == n and st["samples_blocked"] == int((~live).sum()), st
    assert st["windows"] < -(-n // Kb), st
    assert acc == oacc and np.array_equal(ok, ook.astype(np.uint8))
    _assert_same_tree(q.tree(), tr.arrays())
    q.close()


def test_call_split_independence(pkg, oracle_mod, field):
    """the same stream in calls of 1, K - 1, K + 1 and 2 K + 1 iterations: the tree of one call"""
    raw, p, tree = field["raw"], field["p"], field["tree"]
    rng = np.random.default_rng(8)
    n = 9 * K + 5
    live = rng.uniform(size=n) >= 0.4
    live[3 * K:5 * K + 3] = False  # (and a long blocked run: calls end inside it)
    sx, sy = _stream(field, live, rng)
    p.set_window(K)
    p.tree_import(*tree)
    acc_one, ok_one = _extend_ok(pkg, p, sx, sy)
    one = p.tree()
    tr = _oracle(oracle_mod, raw, tree)
    oacc, _, _, ook = oracle_mod.rrt_extend_samples(oracle_mod.OracleScene.from_raw(raw), tr, sx, sy)
    assert acc_one == oacc and np.array_equal(ok_one, ook.astype(np.uint8))
    _assert_same_tree(one, tr.arrays())
    p.tree_import(*tree)
    p.reset_stats()
    a, k, oks = 0, 0, []
    sizes = (1, K - 1, K + 1, 2 * K + 1)
    while a < n:
        b = min(n, a + sizes[k % 4])
        oks.append(_extend_ok(pkg, p, sx[a:b].copy(), sy[a:b].copy())[1])
        a, k = b, k + 1
    st = p.stats()
    assert st["iterations"] == n and st["samples_blocked"] == int((~live).sum()), st
    assert np.array_equal(np.concatenate(oks), ok_one)
    got = p.tree()
    for g, e in zip(got, one):
        assert np.array_equal(g, e)


@pytest.mark.parametrize("window", [64, 256])
def test_truncation_inside_a_widened_window(pkg, oracle_mod, field, window):
    """A young tree (the root alone) and tight clusters of live samples with a blocked draw between
    every two of them.  How the stream was chosen: a cluster is 24 free points within 0.3 of a spot
    that has 2.0 of clearance and lies more than 60 from the start, so every cluster sample is
    nearer to each earlier one than to any node a tree grown from the root can hold that early.
    The 18th sample of a cluster then has 17 nearer window samples — one more than a candidate
    list holds (kCandCap = 16) — and the window is cut at that sample, whose id (17 plus what
    came before) differs from its iteration offset (the blocked draws in between).  Each cluster
    fits a young tree's window (64 samples at K = 64, 128 at K = 256)."""
    raw = field["raw"]
    rng = np.random.default_rng(window)
    xs, ys, lv = [], [], []
    for c in range(3):
        cx, cy = field["far"][c]
        ang, rad = rng.uniform(0, 2 * np.pi, 24), 0.3 * np.sqrt(rng.uniform(size=24))
        bx, by = _stream(field, np.zeros(24, dtype=bool), rng)
        for k in range(24):  # live, blocked, live, blocked, ...
            xs += [cx + rad[k] * np.cos(ang[k]), bx[k]]
            ys += [cy + rad[k] * np.sin(ang[k]), by[k]]
            lv += [True, False]
        m = rng.uniform(size=90) >= 0.35  # then a scattered stretch
        fx, fy = _stream(field, m, rng)
        xs += list(fx)
        ys += list(fy)
        lv += list(m)
    sx, sy, live = np.array(xs), np.array(ys), np.array(lv)
    p = _planner(pkg, raw, 5, window)  # (a context of its own)
    p.reset_stats()
    acc, ok = _extend_ok(pkg, p, sx, sy)
    st = p.stats()
    tr = oracle_mod.OracleTree(raw["start"], 1 << 12)
    oacc, _, _, ook = oracle_mod.rrt_extend_samples(oracle_mod.OracleScene.from_raw(raw), tr, sx, sy)
    print(f"K={window}: {len(sx)} iterations, accepted {acc} (oracle {oacc}), windows "
          f"{st['windows']}, truncations {st['truncations']}, blocked {st['samples_blocked']}")
    assert st["truncations"] >= 1, st
    assert st["iterations"] == len(sx) and st["samples_blocked"] == int((~live).sum()), st
    assert acc == oacc and np.array_equal(ok, ook.astype(np.uint8))
    _assert_same_tree(p.tree(), tr.arrays())
    p.close()

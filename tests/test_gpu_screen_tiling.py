"""The NN screen's tiling (csrc/pp_screen_geom.h) on the device: single K = 4096 windows whose
number of screened samples L — the samples outside every inflated disc; the obstacle pre-test
takes the others out of the screen — sits on every edge of the tiling: one sample, one row of 64
and one either side, 7 rows and 8 rows (one block) and one either side, the benched 2797 (blocks of
8, 8, 7, 7, 7, 7 rows with different chunk counts), 4033 (a last row of one sample) and 4096.

The tree after every window is compared with the oracle's sequential run over the same samples:
x, y and parent bit for bit, yaw within 1e-9 (ocml vs glibc atan2, as everywhere in the suite)."""
import numpy as np
import pytest

from test_gpu_parity import _assert_same_tree, _planner

pytestmark = pytest.mark.gpu

K = 4096
LS = (1, 63, 64, 65, 447, 448, 449, 512, 513, 2797, 4033, 4096)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grown(pkg, ctx):
    """a field512 planner grown to about 10k nodes on its own stream, and that tree"""
    from pathplanning_amd import scenes

    raw = scenes.field512()
    p = _planner(pkg, raw, 21, K, ctx)
    while p.tree_size() < 10000:
        p.extend(K)
    return raw, p, p.tree()


def _window(raw, rng, L):
    """K samples, exactly L of them outside every inflated disc (by a margin), the others deep
    inside one (near the centre of a disc of radius >= 4: the pre-test's cells there lie wholly
    inside), in random order"""
    from pathplanning_amd import rrt

    sp = rrt.Space.from_raw(raw)
    x0, x1, y0, y1 = sp.get_bounds()
    obs = sp.get_obs()  # (cx, cy, r + width / 2)
    free = np.zeros((0, 2))
    while len(free) < L:
        pts = np.column_stack([rng.uniform(x0, x1, 2 * K), rng.uniform(y0, y1, 2 * K)])
        d = np.hypot(pts[:, None, 0] - obs[None, :, 0], pts[:, None, 1] - obs[None, :, 1])
        free = np.concatenate([free, pts[np.all(d > obs[None, :, 2] + 0.05, axis=1)]])
    big = obs[(obs[:, 2] >= 4.5) & (obs[:, 0] > x0 + 1.0) & (obs[:, 0] < x1 - 1.0)
              & (obs[:, 1] > y0 + 1.0) & (obs[:, 1] < y1 - 1.0)]  # (the pre-test covers the box)
    pick = big[rng.integers(0, len(big), K - L)]
    inside = pick[:, :2] + rng.uniform(-0.25, 0.25, (K - L, 2))
    s = np.concatenate([free[:L], inside])[rng.permutation(K)]
    return np.ascontiguousarray(s[:, 0]), np.ascontiguousarray(s[:, 1])


def _oracle_tree(oracle_mod, raw, tree):
    tr = oracle_mod.OracleTree(raw["start"], 1 << 17)
    x, y, yaw, par = tree
    n = len(x)
    tr.x[:n], tr.y[:n], tr.yaw[:n], tr.parent[:n] = x, y, yaw, par
    tr._c.n = n
    return tr


def test_single_windows_on_every_tiling_edge(pkg, oracle_mod, grown):
    """~10k nodes: the blocks' chunk counts differ above the 128-node chunk floor and the last
    chunks are ragged.  Each call is one window of exactly L screened samples."""
    raw, p, tree = grown
    sc = oracle_mod.OracleScene.from_raw(raw)
    tr = _oracle_tree(oracle_mod, raw, tree)
    rng = np.random.default_rng(5)
    for L in LS:
        sx, sy = _window(raw, rng, L)
        p.reset_stats()
        acc = p.extend_samples(sx, sy, record=False)
        st = p.stats()
        oacc = oracle_mod.rrt_extend_samples(sc, tr, sx, sy)[0]
        print(f"L={L}: accepted {acc} (oracle {oacc}), tree {p.tree_size()}, windows "
              f"{st['windows']}, truncations {st['truncations']}, blocked {st['samples_blocked']}")
        assert st["windows"] == 1 and st["truncations"] == 0, (L, st)
        assert st["samples_blocked"] == K - L, (L, st)
        assert acc == oacc, L
        _assert_same_tree(p.tree(), tr.arrays())


def test_windows_on_a_one_chunk_tree(pkg, ctx, oracle_mod, grown):
    """fewer than 128 nodes: every block has a single chunk.  (A tree this young cuts its windows
    — the samples are nearer to each other than to the tree — so a call is several windows and a
    cut window's pre-tested samples are counted again when they are drawn again.)"""
    raw, _, tree = grown
    small = tuple(a[:100].copy() for a in tree)
    sc = oracle_mod.OracleScene.from_raw(raw)
    q = _planner(pkg, raw, 21, K, ctx)
    rng = np.random.default_rng(6)
    for L in LS:
        sx, sy = _window(raw, rng, L)
        q.tree_import(*small)
        q.reset_stats()
        acc = q.extend_samples(sx, sy, record=False)
        st = q.stats()
        tr = _oracle_tree(oracle_mod, raw, small)
        oacc = oracle_mod.rrt_extend_samples(sc, tr, sx, sy)[0]
        print(f"L={L}: accepted {acc} (oracle {oacc}), windows {st['windows']}, truncations "
              f"{st['truncations']}, blocked {st['samples_blocked']}")
        assert st["iterations"] == K and st["samples_blocked"] >= K - L, (L, st)
        assert acc == oacc, L
        _assert_same_tree(q.tree(), tr.arrays())

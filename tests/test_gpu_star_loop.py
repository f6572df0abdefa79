"""The replanning loop of DESIGN.md §9, operation by operation, on the device: plan ->
shortcut_commit -> focus -> prune -> advance(hops 1, rounds 2) -> (a scene change with repair) ->
extend, six turns, each operation fed the compacted, re-rooted, rewired output of the one before.
The shapes, the discs and the continuation are tests/star_loop_ref.py's, whose CPU run
(tests/test_star_loop_ref.py) shows on the oracle alone that they are not vacuous.

Every operation is held to its own file's rule by that file's checked helper, on the state the
device exported just before it:
  plan             tests/test_gpu_star_goal.py's _check_query (best node exact, cost 1e-9 relative)
  shortcut_commit  tests/test_gpu_star_shortcut_commit.py's _commit / _check_exact (bit for bit)
  prune            tests/test_gpu_star_prune.py's _prune_checked (==)
  advance          tests/test_gpu_star_advance.py's _advance_checked
  set_space        tests/test_gpu_star_repair.py's _repair_checked
  extend           every query against star_focus_ref.Query continued from the exported state
                   (star_loop_ref.continued): the tree at tests/test_gpu_rrtstar.py's tolerances
                   (_assert_same), edge costs at COST_RTOL, `iterations`, `skipped`, the rewires
                   and the focus exact
After every operation each tree must be a valid one whose stored costs are their own rebuild
(forest_state_ref.check_tree), the export_forest keys the operation does not own must be as they
were, and the edge costs of the rows a compaction carries must be the old ones bit for bit."""
import time

import numpy as np
import pytest

import forest_state_ref
import star_loop_ref as loop
from star_tree_cases import _space, _trees
from test_gpu_rrtstar import COST_RTOL, _assert_same, _batch
from test_gpu_star_advance import PER_SLOT, _advance_checked
from test_gpu_star_goal import _check_query
from test_gpu_star_prune import _prune_checked
from test_gpu_star_repair import _repair_checked
from test_gpu_star_shortcut_commit import _check_exact, _commit

pytestmark = pytest.mark.gpu

Q = 4


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _same(st0, st1, keys):
    for key in keys:
        assert np.array_equal(st0[key], st1[key]), key


def _valid(st):
    off = st["off"]
    for q in range(len(off) - 1):
        s = slice(int(off[q]), int(off[q + 1]))
        verdict, _ = forest_state_ref.check_tree(st["parent"][s], st["edge_cost"][s], st["cost"][s])
        assert verdict == forest_state_ref.OK, q
    return st


def _rows(st, q, key):
    return st[key][int(st["off"][q]):int(st["off"][q + 1])]


def _tree(st, q):
    return tuple(_rows(st, q, key) for key in ("x", "y", "yaw", "parent", "cost"))


def _remap(node, new_index, off):
    return np.array([new_index[off[q] + node[q]] if node[q] >= 0 else -1 for q in range(Q)],
                    dtype=np.int32)


def _turn(oracle_mod, b, raw, raw_cur, turn, k, eta, log):
    """one turn with every operation checked; returns the scene that holds after it"""
    goal = raw["goal"]
    goals = np.tile(np.asarray(goal, dtype=np.float64), (Q, 1))
    R = b.space.get_steer()
    osc = oracle_mod.OracleScene.from_raw(raw_cur)
    row = {"turn": turn}
    # 1. plan
    st0 = _valid(b.export_forest())
    node, cost = b.plan(goal)
    for q in range(Q):
        _check_query(b, osc, q, goal, int(node[q]), float(cost[q]), path=False)
    _same(st0, b.export_forest(), st0.keys())
    log["no_plan"] += int((node < 0).sum())
    # 2. shortcut_commit: a query without a plan is skipped and comes out bit for bit
    run = _commit(b, goals, node, loop.SPAN)
    _check_exact(run)
    assert np.array_equal(run["node"] >= 0, node >= 0)
    node, cost = run["node"], run["cost"]
    log["commit_rewired"] += int(run["nrw"].sum())
    st0 = _valid(run["st1"])
    # 3. focus
    b.focus(goals, cost)
    fxy, bound, skipped = b.focus_state()
    assert np.array_equal(fxy, goals[:, :2]) and np.array_equal(bound, cost * np.float64(R))
    st1 = b.export_forest()
    _same(st0, st1, [key for key in st0 if key not in ("focus_xy", "focus_bound")])
    assert np.array_equal(st1["focus_xy"], fxy) and np.array_equal(st1["focus_bound"], bound)
    assert np.array_equal(st1["skipped"], skipped)
    # 4. prune
    st0 = st1
    _, pexp, n_new, new_index = _prune_checked(b, node)
    st1 = _valid(b.export_forest())
    _same(st0, st1, PER_SLOT)
    for q, e in enumerate(pexp):
        assert np.array_equal(_rows(st1, q, "edge_cost"), _rows(st0, q, "edge_cost")[e["keep"]]), q
        if node[q] < 0:
            assert e["keep"].all()
    log["prune_dropped"] += int(b.last_dropped)
    node = _remap(node, new_index, st0["off"])
    row["plan"], row["pruned"] = [int(v) for v in node], [int(v) for v in n_new]
    # 5. advance
    st0 = st1
    aexp = _advance_checked(b, osc, k, node, 1, loop.ROUNDS)
    loop.note_advance(log, turn, [int(v) for v in node], aexp)
    node = np.array([e["new_index"][node[q]] if node[q] >= 0 else -1 for q, e in enumerate(aexp)],
                    dtype=np.int32)
    st1 = _valid(b.export_forest())
    row["advanced"] = [int(v) for v in st1["off"][1:] - st1["off"][:-1]]
    row["reattached"] = [e["reattached"] for e in aexp]
    row["recovered"] = [e["recovered"] for e in aexp]
    # 6. a scene change with repair
    if turn in (loop.DISC_FIRST, loop.DISC_ON, loop.DISC_OFF):
        st0 = st1
        before = _trees(b)
        disc = (loop.disc_in_largest(before) if turn == loop.DISC_FIRST else
                loop.disc_for(before[0], int(node[0]), goal) if turn == loop.DISC_ON else None)
        raw_cur = loop.scene_with(raw, disc)
        osc, rexp = _repair_checked(oracle_mod, b, before, raw_cur, k, loop.ROUNDS)
        st1 = _valid(b.export_forest())
        _same(st0, st1, PER_SLOT)
        for q, e in enumerate(rexp):
            want = loop.repaired_elen(_rows(st0, q, "edge_cost"), e)
            new = np.zeros(len(e["keep"]), dtype=bool)
            new[list(e["gap"])] = True
            new = new[e["keep"]]
            got = _rows(st1, q, "edge_cost")
            assert np.array_equal(got[~new], want[~new]), q
            assert np.allclose(got[new], want[new], rtol=COST_RTOL, atol=0.0), q
            if turn == loop.DISC_OFF:
                assert e["keep"].all()
            else:
                log["disc_dropped"][turn] += len(e["keep"]) - int(e["keep0"].sum())
                log["disc_recovered"][turn] += e["recovered"]
            log["repair_reattached"] += e["reattached"]
        row["repaired"] = [int(v) for v in st1["off"][1:] - st1["off"][:-1]]
    # 7. extend
    st0 = st1
    fxy, bound, skipped = b.focus_state()
    b.extend(loop.STEP)
    st1 = _valid(b.export_forest())
    _same(st0, st1, ("seeds", "focus_xy", "focus_bound"))
    n = b.state()[0]
    for q in range(Q):
        r = loop.continued(osc, _tree(st0, q), _rows(st0, q, "edge_cost"), st0["seeds"][q],
                           st0["iterations"][q], st0["skipped"][q], fxy[q], bound[q], loop.STEP,
                           k, eta)
        a = r.arrays()
        _assert_same(b.tree(q, n[q]), a)
        assert np.allclose(_rows(st1, q, "edge_cost"), a[5], rtol=COST_RTOL, atol=0.0), q
        assert st1["iterations"][q] == r.it and st1["skipped"][q] == r.skipped, q
        assert st1["rewires"][q] - st0["rewires"][q] == r.rewires, q
    assert np.array_equal(b.focus_state()[2], st1["skipped"])
    row["extended"] = [int(v) for v in n]
    log["turns"].append(row)
    return raw_cur


# ------------------------------------------------------ B1. the loop, operation by operation
@pytest.mark.parametrize("k,eta", loop.CASES)
def test_the_loop_operation_by_operation(pkg, ctx, oracle_mod, k, eta):
    from pathplanning_amd import scenes

    t0 = time.perf_counter()
    raw = scenes.bench6_open()
    b = _batch(pkg, raw, loop.starts(raw), loop.SEEDS, loop.MAX_ITER, k, eta, ctx=ctx)
    b.extend(loop.N0)
    log = loop.new_log()
    raw_cur = raw
    for turn in range(loop.TURNS):
        raw_cur = _turn(oracle_mod, b, raw, raw_cur, turn, k, eta, log)
        print(log["turns"][-1])
    print({key: v for key, v in log.items() if key != "turns"})
    loop.assert_not_vacuous(log, k)
    assert (b.state()[1] == loop.MAX_ITER).all()
    # queries of one batch in different states in the same call
    assert any(min(row["plan"]) < 0 <= max(row["plan"]) for row in log["turns"])
    print("B1 (%d, %g) wall %.2f s" % (k, eta, time.perf_counter() - t0))


# ------------------------------------------------------------- B3. a twin from an export
def _plain_turn(b, raw, turn):
    """one turn without checks: [(operation, every array it returned and every array of the forest
    exported after it)] and the scene the turn changed to (None: it stays)"""
    goal = raw["goal"]
    goals = np.tile(np.asarray(goal, dtype=np.float64), (Q, 1))
    out = []

    def done(name, *arrays):
        out.append((name, [np.asarray(v) for v in arrays] + list(b.export_forest().values())))

    node, cost = b.plan(goals)
    done("plan", node, cost)
    node, cost, nrw = b.shortcut_commit(goals, node, loop.SPAN)
    done("commit", node, cost, nrw)
    b.focus(goals, cost)
    done("focus", *b.focus_state())
    n_old = b.state()[0]
    n_new, new_index = b.prune(node, n_old)
    done("prune", n_new, new_index)
    node = _remap(node, new_index, np.concatenate([[0], np.cumsum(n_old)]))
    n_old = n_new
    n_new, new_index = b.advance(node, hops=1, rounds=loop.ROUNDS)
    done("advance", n_new, new_index, [b.last_dropped, b.last_reattached, b.last_recovered])
    node = _remap(node, new_index, np.concatenate([[0], np.cumsum(n_old)]))
    scene = None
    if turn in (loop.DISC_FIRST, loop.DISC_ON, loop.DISC_OFF):
        trees = _trees(b)
        disc = (loop.disc_in_largest(trees) if turn == loop.DISC_FIRST else
                loop.disc_for(trees[0], int(node[0]), goal) if turn == loop.DISC_ON else None)
        scene = loop.scene_with(raw, disc)
        n_new, new_index = b.set_space(_space(scene), repair_rounds=loop.ROUNDS)
        done("set_space", n_new, new_index, [b.last_dropped, b.last_reattached, b.last_recovered])
    done("extend", b.extend(loop.STEP))
    return out, scene


def test_twin_from_an_export_mid_loop(pkg, ctx):
    from pathplanning_amd import scenes

    t0 = time.perf_counter()
    k, eta = loop.CASES[1]
    raw = scenes.bench6_open()
    a = _batch(pkg, raw, loop.starts(raw), loop.SEEDS, loop.MAX_ITER, k, eta, ctx=ctx)
    a.extend(loop.N0)
    scene = raw
    for turn in range(4):
        _, changed = _plain_turn(a, raw, turn)
        scene = scene if changed is None else changed
    assert scene is not raw  # turn 2's disc is still there
    st = _valid(a.export_forest())
    c2 = pkg.Context(0)
    try:
        # other starts and seeds: everything has to come from the state
        twin = _batch(pkg, scene, loop.starts(raw)[::-1], [101, 102, 103, 104], loop.MAX_ITER, k,
                      eta, ctx=c2)
        twin.import_forest(st)
        _same(st, twin.export_forest(), st.keys())
        for turn in (4, 5):
            ops_a, _ = _plain_turn(a, raw, turn)
            ops_t, _ = _plain_turn(twin, raw, turn)
            assert [name for name, _ in ops_a] == [name for name, _ in ops_t]
            for (name, got_a), (_, got_t) in zip(ops_a, ops_t):
                assert len(got_a) == len(got_t)
                for va, vt in zip(got_a, got_t):
                    assert np.array_equal(va, vt), (turn, name)
        sa, stw = a.export_forest(), twin.export_forest()
        _same(sa, stw, sa.keys())
        assert (sa["iterations"] == loop.MAX_ITER).all()
    finally:
        c2.close()
    print("B3 wall %.2f s" % (time.perf_counter() - t0))

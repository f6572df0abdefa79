"""bench.py's plain run, `--full` and `--dump-outputs`.

CPU: the arrays `--dump-outputs` writes are float64 `.npy` files capped at 64 MB, and the options
parse as documented.  GPU: a plain run of config 2 at a small size prints the headline keys and
none of what `--full` adds, `--steps` sets the timed steps, and the tree it dumps is the tree of
the same command with `--full` and the sequential oracle's tree of as many iterations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
             "warmup", "n_gpus")


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def _refuse(tok):
    raise ValueError(tok)


def test_dump_outputs_writes_float64_npy(tmp_path):
    bench = _bench()
    d = tmp_path / "a" / "b"  # created on demand
    par = np.array([-1, 0, 0, 2], dtype=np.int32)
    x = np.array([0.1, 0.2, 0.30000000000000004, 1e300])
    bench.dump_outputs(str(d), {"x": x, "parent": par})
    assert sorted(os.listdir(d)) == ["parent.npy", "x.npy"]
    gx, gp = np.load(d / "x.npy"), np.load(d / "parent.npy")
    assert gx.dtype == np.float64 and gp.dtype == np.float64
    assert np.array_equal(gx, x) and np.array_equal(gp, par)  # bit for bit; indices exact


def test_dump_outputs_refuses_more_than_the_cap(tmp_path, monkeypatch):
    bench = _bench()
    assert bench.DUMP_MAX_BYTES == 64 << 20
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64)
    bench.dump_outputs(str(tmp_path), {"a": np.zeros(8)})
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), {"a": np.zeros(8), "b": np.zeros(1)})


def test_options_parse():
    bench = _bench()
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse(["--workload", "plan", "--dump-outputs", "out"])


SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--nodes", "3000", "--window", "256"]


def _run(tmp, name, *extra):
    out, detail = os.path.join(tmp, name), os.path.join(tmp, name + ".json")
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra,
                        "--dump-outputs", out, "--detail", detail],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    with open(detail) as f:
        full = json.load(f)
    tree = {k: np.load(os.path.join(out, k + ".npy")) for k in ("x", "y", "yaw", "parent")}
    assert sorted(os.listdir(out)) == ["parent.npy", "x.npy", "y.npy", "yaw.npy"]
    return json.loads(lines[0], parse_constant=_refuse), full, tree


@pytest.fixture(scope="module")
def plain(built, tmp_path_factory):
    """One plain run, shared by the tests below and left unchanged."""
    return _run(str(tmp_path_factory.mktemp("plain")), "plain")


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_tree(plain, oracle_mod):
    from pathplanning_amd import scenes

    line, rec, tree = plain
    for k in HEAD_KEYS:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["unit"] == "iterations/s"
    assert rec["stats"]["iterations"] == 3 * 256  # --steps sets the timed steps
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(256 / (line["ms_per_step"] * 1e-3), rel=1e-2)
    # nothing beside the headline figure ran
    assert "sub" not in line and line["cpu_baseline"] is None and line["roofline"] is None
    assert set(rec["sizes"]) == {"3000"} and rec["window_chain_us"] is None
    for k in ("config3", "config5", "config4", "polygons", "config1", "plan", "example_rrt"):
        assert k not in rec, k

    # the dumped tree: float64, root first, as long as the line says, and the sequential
    # oracle's tree after the same iterations (growth + warmup + timed steps)
    n = len(tree["x"])
    assert all(a.dtype == np.float64 and a.shape == (n,) for a in tree.values())
    assert n == line["config"]["tree_nodes_at_start"] + rec["stats"]["accepted"]
    assert tree["parent"][0] == -1
    raw = scenes.field512()
    sc = oracle_mod.OracleScene.from_raw(raw)
    ot = oracle_mod.OracleTree(raw["start"], n + 16 * 256)
    done, marks = 0, [1000, 10000]
    while ot.n < 3000:  # run_tree's growth: whole windows, five more at each size mark
        k = 256
        if marks and ot.n >= marks[0]:
            marks.pop(0)
            k += 5 * 256
        oracle_mod.rrt_extend(sc, ot, 42, done, k)
        done += k
    oracle_mod.rrt_extend(sc, ot, 42, done, (1 + 3) * 256)  # the warmup window, the timed steps
    ox, oy, oyaw, opar = ot.arrays()
    assert len(ox) == n
    assert np.array_equal(tree["x"], ox) and np.array_equal(tree["y"], oy)
    assert np.array_equal(tree["parent"], opar)
    assert np.max(np.abs(tree["yaw"] - oyaw)) <= 1e-9


@pytest.mark.gpu
def test_full_adds_the_rest_and_leaves_the_timed_outputs(plain, tmp_path):
    line, _, tree = plain
    fline, frec, ftree = _run(str(tmp_path), "full", "--full", "--no-sub", "--cpu-seconds", "0.3")
    for k in tree:
        assert np.array_equal(tree[k], ftree[k]), k
    assert fline["roofline"]["frac"] > 0 and fline["cpu_baseline"]["value"] > 0
    assert set(frec["sizes"]) == {"1000", "3000"} and frec["window_chain_us"]["windows"] >= 3
    for k in HEAD_KEYS:
        assert k in fline, k
    assert (fline["metric"], fline["unit"], fline["steps"]) == (line["metric"], line["unit"], 3)

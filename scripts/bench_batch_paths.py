"""Time of the batched path export (pp_batch_paths / pp_star_paths) on the two query batches:
config 3's (the 512-field, 8192 queries x 2000 extend iterations: plan() then paths(best)) and
config 5's (the config-5 field, RRT*: plan(goals) then paths(goals, best)).  The trees are grown
first (untimed).

  python scripts/bench_batch_paths.py [--queries 8192] [--iters 2000] [--runs 7]
                                      [--baseline-queries 64] [--config 3|5|both]

Prints one JSON line (record: profiles/batch_paths.json).  Per config: the median wall time of
the paths call of `runs` calls after a warm-up, the device-to-host copy included (the C call with
buffers sized beforehand: from the plan's n_points for config 3, from a sizes-only call for
config 5 — that call is timed too and reported beside it), the total points and bytes, points/s,
and that run's plan time (config 3: bench.py's check_finish_ms is this wall time).  The baseline
is what a caller has to do without the batched call, measured here on the first
--baseline-queries queries that have a path, per query: config 3 pp_batch_tree_export ->
pp_rrt_new + pp_rrt_tree_import -> pp_rrt_check_finish; config 5 pp_star_path.  ratio =
baseline ms per query / batched ms per query (over the queries with a path).

Kernel trace of the calls (a run of its own, no counters):
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python scripts/bench_batch_paths.py --runs 1 --baseline-queries 0"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rs-pathplanning_amd"), os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)


def med(ms):
    return {"ms": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3), "runs": len(ms)}


def timed(fn, runs):
    """wall ms of `runs` calls of fn after one warm-up; the last result"""
    ms, out = [], None
    for i in range(runs + 1):
        t0 = time.perf_counter()
        out = fn()
        if i > 0:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def report(ms, n_points, n_paths, plan_ms, base_ms, base_n):
    m = statistics.median(ms)
    r = dict(med(ms))
    r.update({"points": int(n_points), "bytes": int(16 * n_points), "queries_with_path": int(n_paths),
              "points_per_s": round(n_points / (m * 1e-3)) if m > 0 else None,
              "us_per_query": round(1e3 * m / max(n_paths, 1), 3)})
    r["plan"] = med(plan_ms)
    if base_n > 0:
        per = statistics.median(base_ms)
        r["baseline_loop"] = {"queries": base_n, "ms_per_query": round(per, 3),
                              "extrapolated_batch_ms": round(per * n_paths, 1)}
        r["ratio_baseline_over_batched_per_query"] = round(per / (m / max(n_paths, 1)), 1)
    return r


def config3(args):
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.field512()
    space = rrt.Space.from_raw(raw)
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    b = rrt.RRTBatch(starts, goals, args.iters, raw["step_size"], space, seeds)
    b.extend(args.iters)
    plan_ms, plan = timed(b.plan, args.runs)
    best = np.ascontiguousarray(plan["best_node"], dtype=np.int32)
    total = int(plan["n_points"].sum(dtype=np.int64))
    L = _ffi.lib()
    ip, dp, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    off = np.zeros(b.q + 1, dtype=np.int64)
    x, y = np.zeros(max(total, 1)), np.zeros(max(total, 1))
    tot = C.c_int64(0)

    def call():
        _ffi.check(L.pp_batch_paths(b.ctx.handle, best.ctypes.data_as(ip), off.ctypes.data_as(i64),
                                    x.ctypes.data_as(dp), y.ctypes.data_as(dp), total,
                                    C.byref(tot), None))
        return tot.value

    ms, got = timed(call, args.runs)
    assert got == total and np.array_equal(np.diff(off), plan["n_points"])
    # the loop a caller needs without the batched call, per query
    fin = [int(q) for q in np.flatnonzero(best >= 0)[:args.baseline_queries]]
    st = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    gl = np.asarray(goals, dtype=np.float64).reshape(-1, 3)
    ctx1 = _ffi.Context(0)
    base = []
    for i, q in enumerate(fin[:1] + fin):  # (the first once more: the warm-up)
        t0 = time.perf_counter()
        tree = b.tree(q)
        t = rrt.RRT(st[q][:2], st[q][2], gl[q][:2], gl[q][2], args.iters, raw["step_size"], space,
                    ctx=ctx1)
        t.tree_import(*tree)
        line = t.check_finish(int(best[q]))
        dt = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(line, np.stack([x, y], axis=1)[off[q]:off[q + 1]]), q
        if i > 0:
            base.append(dt)
    ctx1.close()
    r = report(ms, total, int((best >= 0).sum()), plan_ms, base, len(fin))
    r["workload"] = (f"pp_batch_plan then pp_batch_paths(best_node): {args.queries} queries x "
                     f"{args.iters} iterations, the config-3 field")
    r["baseline_what"] = ("per query: pp_batch_tree_export -> pp_rrt_new + pp_rrt_tree_import -> "
                          "pp_rrt_check_finish (RRTBatch.tree, RRT, tree_import, check_finish)")
    b.close()
    return r


def config5(args):
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    goals = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
    b = rrt.RRTStarBatch(starts, args.iters, raw["step_size"], rrt.Space.from_raw(raw), seeds,
                         k=0, eta=scenes.CONFIG5_ETA)
    b.extend(args.iters)
    plan_ms, (node, _) = timed(lambda: b.plan(goals), args.runs)
    best = np.ascontiguousarray(node, dtype=np.int32)
    L = _ffi.lib()
    ip, dp, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    off = np.zeros(b.q + 1, dtype=np.int64)
    length = np.zeros(b.q)
    tot = C.c_int64(0)
    G, N, O = goals.ctypes.data_as(dp), best.ctypes.data_as(ip), off.ctypes.data_as(i64)

    def sizes():
        _ffi.check(L.pp_star_paths(b.ctx.handle, G, N, O, None, None, 0, C.byref(tot), None, None))
        return tot.value

    size_ms, total = timed(sizes, args.runs)
    x, y = np.zeros(max(total, 1)), np.zeros(max(total, 1))

    def call():
        _ffi.check(L.pp_star_paths(b.ctx.handle, G, N, O, x.ctypes.data_as(dp),
                                   y.ctypes.data_as(dp), total, C.byref(tot),
                                   length.ctypes.data_as(dp), None))
        return tot.value

    ms, got = timed(call, args.runs)
    assert got == total
    fin = [int(q) for q in np.flatnonzero(best >= 0)[:args.baseline_queries]]
    base = []
    for i, q in enumerate(fin[:1] + fin):
        t0 = time.perf_counter()
        xy, ln = b.path(q, goals[q], int(best[q]))
        dt = (time.perf_counter() - t0) * 1e3
        row = np.stack([x, y], axis=1)[off[q]:off[q + 1]]
        assert row.shape == xy.shape and np.max(np.abs(row - xy)) <= 1e-9, q
        assert abs(ln - length[q]) <= 1e-9 * ln, q
        if i > 0:
            base.append(dt)
    r = report(ms, total, int((best >= 0).sum()), plan_ms, base, len(fin))
    r["sizes_only_call"] = med(size_ms)
    r["workload"] = (f"pp_star_plan then pp_star_paths(goals, best_node): {args.queries} queries x "
                     f"{args.iters} RRT* iterations, the config-5 field, eta {scenes.CONFIG5_ETA}")
    r["baseline_what"] = "per query: pp_star_path (RRTStarBatch.path: its sizes call and its points call)"
    b.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--baseline-queries", type=int, default=64)
    ap.add_argument("--config", default="both", choices=["3", "5", "both"])
    args = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    line = {"what": "batched path export: wall ms around the call, device-to-host copy included",
            "queries": args.queries, "iters": args.iters}
    if args.config in ("3", "both"):
        line["config3"] = config3(args)
    if args.config in ("5", "both"):
        line["config5"] = config5(args)
    print(json.dumps(line))


if __name__ == "__main__":
    main()

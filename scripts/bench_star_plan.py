"""Time of the RRT* goal connection (pp_star_plan) on config 5's batch: the config-5 field,
CONFIG5_ETA, config3_queries' starts, goals and seeds; the trees are grown first (untimed).

  python scripts/bench_star_plan.py [--queries 8192] [--iters 2000] [--runs 7] [--cpu-queries 16]

Prints one JSON line: the median wall time of plan(goals) around pp_synchronize, the (query,
node) pairs considered and pairs/s, the tasks actually steered (hence the cull rate), the share
of reachable goals, the same figures with pruning off (the internal launch's debug switch, not
part of the ABI), and the CPU restatement (oracle.dubins + verify_line per pair, one core) on the
first --cpu-queries queries, extrapolated to the batch as pairs/s.

Kernel trace of one plan (a run of its own, no counters):
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python scripts/bench_star_plan.py --plans 2
  python scripts/bench_star_plan.py --trace-summary DIR"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rs-pathplanning_amd"), os.path.join(ROOT, "oracle"),
          os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)


def timed_plan(batch, goals, prune, runs):
    """median ms of `runs` plans after one warm-up; (ms list, best_node, cost, checked, steered)"""
    from pathplanning_amd import _ffi

    L = _ffi.lib()
    fn = L.ppamd_star_plan_debug
    dp, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    fn.argtypes = [C.c_void_p, dp, C.c_int, C.POINTER(C.c_int32), dp, i64p, i64p]
    fn.restype = C.c_int
    node = np.zeros(batch.q, dtype=np.int32)
    cost = np.zeros(batch.q)
    chk, steered = C.c_int64(0), C.c_int64(0)
    ms = []
    for i in range(runs + 1):
        _ffi.check(L.pp_synchronize(batch.ctx.handle))
        t0 = time.perf_counter()
        _ffi.check(fn(batch.ctx.handle, goals.ctypes.data_as(dp), int(prune),
                      node.ctypes.data_as(C.POINTER(C.c_int32)), cost.ctypes.data_as(dp),
                      C.byref(chk), C.byref(steered)))
        _ffi.check(L.pp_synchronize(batch.ctx.handle))
        if i > 0:  # (run 0: the warm-up)
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, node.copy(), cost.copy(), chk.value, steered.value


def figures(ms, checked, steered):
    med = statistics.median(ms)
    return {"ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "runs": len(ms), "pairs_per_s": round(checked / (med * 1e-3)),
            "tasks_steered": steered, "cull_rate": round(1.0 - steered / max(checked, 1), 4)}


def trace_summary(d):
    """the last plan of a `rocprofv3 --kernel-trace` run of `--plans N` under directory d (its
    dispatches from the last star_goal_init_kernel on), per kernel: one JSON line"""
    import csv
    import glob

    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    first = max(i for i, r in enumerate(rows) if "star_goal_init_kernel" in r["Kernel_Name"])
    seg = rows[first:]
    per = {}
    for r in seg:
        name = r["Kernel_Name"].rsplit("(", 1)[0].replace("void ", "").replace("ppamd::", "")
        name = name.split("<")[0]
        k = per.setdefault(name, {"calls": 0, "us": 0.0})
        k["calls"] += 1
        k["us"] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
    span = (int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) * 1e-3
    for k in per.values():
        k["us"] = round(k["us"], 1)
    print(json.dumps({"what": "one pp_star_plan, rocprofv3 --kernel-trace (no counters)",
                      "dispatches": len(seg), "span_us": round(span, 1),
                      "busy_us": round(sum(k["us"] for k in per.values()), 1), "kernels": per}))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--trace-summary":
        return trace_summary(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--cpu-queries", type=int, default=16)
    ap.add_argument("--plans", type=int, default=0,
                    help="profiling: only this many pruned plans after the extend, no timing")
    args = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    from pathplanning_amd import rrt, scenes

    raw = scenes.config5_field()
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    goals = np.ascontiguousarray(goals, dtype=np.float64)
    batch = rrt.RRTStarBatch(starts, args.iters, raw["step_size"], rrt.Space.from_raw(raw), seeds,
                             k=0, eta=scenes.CONFIG5_ETA)
    batch.extend(args.iters)
    if args.plans > 0:
        for _ in range(args.plans):
            batch.plan(goals)
        return
    ms, node, cost, checked, steered = timed_plan(batch, goals, 1, args.runs)
    ms0, node0, cost0, checked0, steered0 = timed_plan(batch, goals, 0, args.runs)
    assert np.array_equal(node, node0) and np.array_equal(cost, cost0), "pruned != un-pruned"
    line = {"workload": f"pp_star_plan: {args.queries} queries x {args.iters} RRT* iterations, "
                        f"config-5 field, eta {scenes.CONFIG5_ETA}",
            "queries": args.queries, "iters": args.iters, "n_checked": checked,
            "reachable_share": round(float((node >= 0).mean()), 4)}
    line.update(figures(ms, checked, steered))
    line["unpruned"] = figures(ms0, checked0, steered0)
    if args.cpu_queries > 0:
        import oracle
        import star_goal_ref as ref

        osc = oracle.OracleScene.from_raw(raw)
        nq = min(args.cpu_queries, args.queries)
        trees = [batch.tree(q) for q in range(nq)]
        t0 = time.perf_counter()
        pairs = 0
        for q in range(nq):
            b, c, _ = ref.plan(osc, trees[q], goals[q])
            assert b == node[q], (q, b, node[q])
            pairs += len(trees[q][0])
        dt = time.perf_counter() - t0
        line["cpu_restatement"] = {
            "note": f"oracle.dubins + verify_line per pair on one core, queries 0..{nq - 1} only "
                    f"(a subset extrapolation)",
            "pairs": pairs, "s": round(dt, 3), "pairs_per_s": round(pairs / dt),
            "extrapolated_batch_s": round(checked / (pairs / dt), 1)}
    print(json.dumps(line))
    batch.close()


if __name__ == "__main__":
    main()

"""Time and effect of the shortcuts along the chain (pp_star_shortcut) on config 5's batch: the
config-5 field, CONFIG5_ETA, config3_queries' starts, goals and seeds; the trees are grown and
planned first (untimed), then every reachable query's path is shortened at span 8 and span 63.

  python scripts/bench_star_shortcut.py [--queries 8192] [--iters 2000] [--runs 7]
                                        [--out profiles/star_shortcut.json]

Per span: the median wall time of shortcut(goals, plan's nodes, span) around pp_synchronize (of
--runs calls after a warm-up), the pairs tested, the steer rounds, the per-kernel split of one
call by stream events (the internal launch's debug entry, not part of the ABI) and the
distribution of shortcut cost / plan cost over the reachable queries.  plan's own time is measured
beside it for scale.  Prints the JSON and writes it to --out."""
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

STAGES = ("chain_and_sizes", "emit", "steer_prep", "steer_walk", "settle", "dp", "pack_and_copy")


def timed(batch, fn, runs):
    """ms of `runs` calls of fn() after one warm-up, each between two pp_synchronize"""
    from pathplanning_amd import _ffi

    L = _ffi.lib()
    ms, out = [], None
    for i in range(runs + 1):
        _ffi.check(L.pp_synchronize(batch.ctx.handle))
        t0 = time.perf_counter()
        out = fn()
        _ffi.check(L.pp_synchronize(batch.ctx.handle))
        if i > 0:  # (run 0: the warm-up)
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def stage_split(batch, goals, nodes, span):
    """one call through the debug entry: ({stage: ms}, steer rounds)"""
    from pathplanning_amd import _ffi

    fn = _ffi.lib().ppamd_star_shortcut_debug
    dp, ip, i64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    fn.argtypes = [C.c_void_p, dp, ip, C.c_int, i64, ip, C.c_int64, i64, dp,
                   C.POINTER(C.c_uint8), i64, dp, i64]
    fn.restype = C.c_int
    off = np.zeros(batch.q + 1, dtype=np.int64)
    cap = int(np.sum(batch.state()[0], dtype=np.int64))
    chain = np.zeros(cap, dtype=np.int32)
    ms = np.zeros(len(STAGES))
    tot, tested, rounds = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _ffi.check(fn(batch.ctx.handle, goals.ctypes.data_as(dp), nodes.ctypes.data_as(ip), int(span),
                  off.ctypes.data_as(i64), chain.ctypes.data_as(ip), cap, C.byref(tot), None, None,
                  C.byref(tested), ms.ctypes.data_as(dp), C.byref(rounds)))
    return {k: round(float(v), 3) for k, v in zip(STAGES, ms)}, rounds.value


def summary(ms):
    return {"ms": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_shortcut.json"))
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
    plan_ms, (node, cost) = timed(batch, lambda: batch.plan(goals), args.runs)
    reach = node >= 0
    line = {"workload": f"pp_star_shortcut after pp_star_plan: {args.queries} queries x "
                        f"{args.iters} RRT* iterations, config-5 field, eta {scenes.CONFIG5_ETA}",
            "queries": args.queries, "iters": args.iters,
            "reachable": int(reach.sum()), "plan": summary(plan_ms), "spans": {}}
    depth = None
    for span in (8, 63):
        ms, (off, chain, scost, ok) = timed(batch, lambda: batch.shortcut(goals, node, span),
                                            args.runs)
        assert np.array_equal(ok, reach), "a reachable query lost its route"
        ratio = scost[reach] / cost[reach]
        stages, rounds = stage_split(batch, goals, node, span)
        rec = summary(ms)
        rec.update({
            "pairs_tested": batch.n_tested, "steer_rounds": rounds,
            "pairs_per_s": round(batch.n_tested / (rec["ms"] * 1e-3)),
            "stages_ms_one_call": stages,
            "nodes_per_path_mean": round(float(np.diff(off)[reach].mean()), 2),
            "cost_ratio": {"mean": round(float(ratio.mean()), 4),
                           "median": round(float(np.median(ratio)), 4),
                           "p10": round(float(np.percentile(ratio, 10)), 4),
                           "p90": round(float(np.percentile(ratio, 90)), 4),
                           "min": round(float(ratio.min()), 4), "max": round(float(ratio.max()), 6),
                           "share_shorter": round(float((ratio < 1.0).mean()), 4)}})
        line["spans"][str(span)] = rec
        if depth is None:  # the tree chains' own depth: span 1's rows
            o1 = batch.shortcut(goals, node, 1)[0]
            depth = np.diff(o1)[reach]
            line["chain_depth"] = {"mean": round(float(depth.mean()), 2), "max": int(depth.max())}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
    batch.close()


if __name__ == "__main__":
    main()

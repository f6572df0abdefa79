"""Time and effect of committing chain shortcuts into the trees (pp_star_shortcut_commit, DESIGN.md
§3.7 "Committing shortcuts") on config 5's batch: the config-5 field, CONFIG5_ETA,
config3_queries' starts, goals and seeds.

  python scripts/bench_star_shortcut_commit.py [--queries 8192] [--iters 2000] [--first 1000]
                                               [--more 1000] [--span 8] [--runs 5]
                                               [--out profiles/star_shortcut_commit.json]

Two measurements, not thresholds:
  time    the trees are grown --iters steps and planned (untimed); shortcut_commit(goals, plan's
          nodes, span) and pp_star_shortcut on the same batch, goals, nodes and span, in the same
          run: median wall time around pp_synchronize of --runs calls after a warm-up.  A commit
          changes the trees, so the forest exported before the first one is imported again
          (untimed) ahead of every commit; one more call goes through the debug entries for the
          stages' event times (not part of the ABI).
  effect  --first steps, then plan(goals, focus=True) (arm A) or plan(goals, focus=True,
          commit=span) (arm B), --more focused steps, then plan(goals): B's cost over A's over the
          queries reachable at the first plan, as scripts/bench_star_focus.py reports B over A.
Prints the JSON and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rs-pathplanning_amd"), os.path.join(ROOT, "oracle"), ROOT,
          os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import bench_star_shortcut as short  # noqa: E402  (timed, summary, stage_split)

STAGES = ("chain_and_sizes", "steer_rounds", "commit_kernel", "copies")


def commit_stages(batch, goals, nodes, span):
    """one commit through the debug entry: {stage: ms}"""
    from pathplanning_amd import _ffi

    fn = _ffi.lib().ppamd_star_shortcut_commit_debug
    dp, ip, i64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    fn.argtypes = [C.c_void_p, dp, ip, C.c_int, ip, dp, ip, i64, i64, dp]
    fn.restype = C.c_int
    ms = np.zeros(len(STAGES))
    _ffi.check(fn(batch.ctx.handle, goals.ctypes.data_as(dp), nodes.ctypes.data_as(ip), int(span),
                  None, None, None, None, None, ms.ctypes.data_as(dp)))
    return {k: round(float(v), 3) for k, v in zip(STAGES, ms)}


def measure_time(args, rrt, scenes, _ffi):
    raw = scenes.config5_field()
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    goals = np.ascontiguousarray(goals, dtype=np.float64)
    batch = rrt.RRTStarBatch(starts, args.iters, raw["step_size"], rrt.Space.from_raw(raw), seeds,
                             k=0, eta=scenes.CONFIG5_ETA)
    batch.extend(args.iters)
    node, cost = batch.plan(goals)
    reach = node >= 0
    sync = _ffi.lib().pp_synchronize
    short_ms, (_, _, scost, _) = short.timed(batch, lambda: batch.shortcut(goals, node, args.span),
                                             args.runs)
    short_pairs = batch.n_tested
    short_stages, rounds = short.stage_split(batch, goals, node, args.span)
    snap = batch.export_forest()
    ms, out = [], None
    for i in range(args.runs + 1):
        if i > 0:
            batch.import_forest(snap)
        _ffi.check(sync(batch.ctx.handle))
        t0 = time.perf_counter()
        out = batch.shortcut_commit(goals, node, args.span)
        _ffi.check(sync(batch.ctx.handle))
        if i > 0:  # (run 0: the warm-up)
            ms.append((time.perf_counter() - t0) * 1e3)
    cnode, ccost, nrw = out
    assert batch.n_tested == short_pairs
    rec = {"reachable": int(reach.sum()), "span": args.span, "pairs_tested": short_pairs,
           "steer_rounds": rounds,
           "shortcut": dict(short.summary(short_ms), stages_ms_one_call=short_stages),
           "commit": short.summary(ms),
           "rewires": int(nrw.sum()), "queries_rewired": int((nrw > 0).sum()),
           "costs_changed": int(batch.n_changed),
           # (the ocml steer is the same code in both calls: the costs agree to the last bit where
           # every own edge steers to its stored cost)
           "cost_equals_shortcut_share": round(float((ccost[reach] == scost[reach]).mean()), 4)}
    after_node, after = batch.plan(goals)
    rec["plan_cost_after_over_before"] = {
        "median": round(float(np.median(after[reach] / cost[reach])), 4),
        "min": round(float((after[reach] / cost[reach]).min()), 4),
        "strictly_cheaper_share": round(float((after[reach] < cost[reach]).mean()), 4),
        "dearer": int((after[reach] > cost[reach]).sum())}
    batch.import_forest(snap)
    rec["commit"]["stages_ms_one_call"] = commit_stages(batch, goals, node, args.span)
    batch.close()
    return rec


def measure_effect(args, rrt, scenes, _ffi):
    raw = scenes.config5_field()
    space = rrt.Space.from_raw(raw)
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    goals = np.ascontiguousarray(goals, dtype=np.float64)
    sync = _ffi.lib().pp_synchronize

    def arm(commit):
        b = rrt.RRTStarBatch(starts, args.first + args.more, raw["step_size"], space, seeds, k=0,
                             eta=scenes.CONFIG5_ETA)
        b.extend(args.first)
        _, cost0 = b.plan(goals, focus=True, commit=commit)
        _ffi.check(sync(b.ctx.handle))
        t0 = time.perf_counter()
        b.extend(args.more)
        _ffi.check(sync(b.ctx.handle))
        ms = (time.perf_counter() - t0) * 1e3 / args.more
        _, cost1 = b.plan(goals)
        n, _, _, rw = b.state()
        b.close()
        return {"cost0": cost0, "cost1": cost1, "ms_per_step": ms, "nodes": int(n.sum()),
                "rewires": int(rw.sum())}

    arm(None)  # warm-up: module load, allocations
    A, B = arm(None), arm(args.span)
    reach0 = np.isfinite(A["cost0"])
    assert np.array_equal(reach0, np.isfinite(B["cost0"]))
    ratio = B["cost1"][reach0] / A["cost1"][reach0]
    q1, q2, q3 = (float(v) for v in np.percentile(ratio, [25, 50, 75]))
    r0 = B["cost0"][reach0] / A["cost0"][reach0]
    return {
        "first": args.first, "more": args.more, "span": args.span,
        "reachable_at_first": int(reach0.sum()),
        "A_focus": {"ms_per_step": round(A["ms_per_step"], 4), "nodes": A["nodes"],
                    "rewires": A["rewires"]},
        "B_focus_commit": {"ms_per_step": round(B["ms_per_step"], 4), "nodes": B["nodes"],
                           "rewires": B["rewires"]},
        "cost_at_first_B_over_A": {"median": round(float(np.median(r0)), 4),
                                   "B_strictly_cheaper_share": round(float((r0 < 1.0).mean()), 4)},
        "cost_B_over_cost_A": {"over": "queries reachable at the first plan", "q1": round(q1, 4),
                               "median": round(q2, 4), "q3": round(q3, 4),
                               "min": round(float(ratio.min()), 4),
                               "max": round(float(ratio.max()), 4),
                               "B_strictly_cheaper_share": round(float((ratio < 1.0).mean()), 4),
                               "A_strictly_cheaper_share": round(float((ratio > 1.0).mean()), 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--first", type=int, default=1000)
    ap.add_argument("--more", type=int, default=1000)
    ap.add_argument("--span", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_shortcut_commit.json"))
    args = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    from pathplanning_amd import _ffi, rrt, scenes

    line = {"workload": f"pp_star_shortcut_commit on config 5's batch: {args.queries} queries, "
                        f"config-5 field, eta {scenes.CONFIG5_ETA}, span {args.span}",
            "queries": args.queries, "iters": args.iters,
            "time": measure_time(args, rrt, scenes, _ffi),
            "effect": measure_effect(args, rrt, scenes, _ffi)}
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

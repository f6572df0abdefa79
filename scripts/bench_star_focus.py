"""Focused sampling (Informed RRT* as a rejection filter) on config 5's batch: what
a focus buys the returned paths and what its draw rounds cost a step.

  python scripts/bench_star_focus.py [--queries 8192] [--first 1000] [--more 1000]
                                     [--out profiles/star_focus.json]

The batch is built several times (the runs are deterministic, so no snapshot is needed).  Both
arms start with --first steps and a plan(goals):
  arm A   --more further steps unfocused, then plan(goals)
  arm B   plan(goals, focus=True), --more further steps, then plan(goals)
Each arm runs three times: timed (wall time of the second extend around pp_synchronize, profiling
off), profiled (HIP events around star_sample and the walks: star_sample's share of the streams'
time) and, arm B only, stepwise (one step per call: the draws skipped and the full-miss
iterations, an iteration whose node_evals did not grow).  Prints one JSON line and writes it to
--out.  These are measurements, not thresholds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rs-pathplanning_amd"), ROOT):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--first", type=int, default=1000)
    ap.add_argument("--more", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_focus.json"))
    args = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    space = rrt.Space.from_raw(raw)
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    goals = np.ascontiguousarray(goals, dtype=np.float64)
    sync = _ffi.lib().pp_synchronize

    def arm(focused, mode):
        b = rrt.RRTStarBatch(starts, args.first + args.more, raw["step_size"], space, seeds, k=0,
                             eta=scenes.CONFIG5_ETA)
        b.extend(args.first)
        _, cost0 = b.plan(goals, focus=focused)
        out = {"cost0": cost0}
        b.set_profiling(mode == "profiled")
        s0 = b.stats()
        _ffi.check(sync(b.ctx.handle))
        t0 = time.perf_counter()
        if mode == "stepwise":
            ev = b.state()[2]
            miss = 0
            for _ in range(args.more):
                b.extend(1)
                ev1 = b.state()[2]
                miss += int((ev1 == ev).sum())
                ev = ev1
            out["full_miss_iterations"] = miss
        else:
            b.extend(args.more)
        _ffi.check(sync(b.ctx.handle))
        out["ms_per_step"] = (time.perf_counter() - t0) * 1e3 / args.more
        s1 = b.stats()
        out["sample_ms_per_step"] = (s1["nn_scan_ms"] - s0["nn_scan_ms"]) / args.more
        out["walk_ms_per_step"] = (s1["steer_ms"] - s0["steer_ms"]) / args.more
        out["launches_per_step"] = (s1["nn_scan_launches"] - s0["nn_scan_launches"]) / args.more
        b.set_profiling(False)
        _, out["cost1"] = b.plan(goals)
        n, it, _, rw = b.state()
        out["nodes"], out["rewires"] = int(n.sum()), int(rw.sum())
        assert (it == args.first + args.more).all()
        out["skipped"] = b.focus_state()[2]
        b.close()
        return out

    arm(False, "timed")  # warm-up: module load, allocations
    runs = {(f, m): arm(f, m) for f in (False, True) for m in ("timed", "profiled")}
    step = arm(True, "stepwise")
    A, B = runs[(False, "timed")], runs[(True, "timed")]
    for (f, m), r in runs.items():  # the runs of one arm are the same run
        ref = B if f else A
        assert np.array_equal(r["cost1"], ref["cost1"]) and r["nodes"] == ref["nodes"], (f, m)
    assert np.array_equal(step["cost1"], B["cost1"]) and np.array_equal(step["skipped"], B["skipped"])
    assert np.array_equal(A["cost0"], B["cost0"])

    reach0 = np.isfinite(A["cost0"])
    ratio = B["cost1"][reach0] / A["cost1"][reach0]
    q1, q2, q3 = (float(v) for v in np.percentile(ratio, [25, 50, 75]))
    focused_iters = int(reach0.sum()) * args.more

    def side(focused):
        t, p = runs[(focused, "timed")], runs[(focused, "profiled")]
        nsub = p["launches_per_step"]
        return {
            "ms_per_step": round(t["ms_per_step"], 4),
            "profiled_ms_per_step": round(p["ms_per_step"], 4),
            "star_sample_ms_per_step": round(p["sample_ms_per_step"], 4),
            "walk_ms_per_step": round(p["walk_ms_per_step"], 4),
            "sub_batch_streams": nsub,
            # the sub-batches' star_sample event spans over the streams' time of the profiled run
            "star_sample_share": round(p["sample_ms_per_step"] / (nsub * p["ms_per_step"]), 4),
            "nodes": t["nodes"], "rewires": t["rewires"],
            "reachable_after": int(np.isfinite(t["cost1"]).sum()),
            "newly_reachable": int((np.isfinite(t["cost1"]) & ~reach0).sum()),
            "improved_share_of_reachable": round(float((t["cost1"][reach0] < t["cost0"][reach0]).mean()), 4),
        }

    line = {
        "workload": f"config 5's batch: {args.queries} queries, config-5 field, eta "
                    f"{scenes.CONFIG5_ETA}; {args.first} steps + plan, then {args.more} steps "
                    f"unfocused (A) or after plan(focus=True) (B), then plan",
        "queries": args.queries, "first": args.first, "more": args.more,
        "reachable_at_first": int(reach0.sum()),
        "A_unfocused": side(False), "B_focused": side(True),
        "cost_B_over_cost_A": {"over": "queries reachable at the first plan", "q1": round(q1, 4),
                               "median": round(q2, 4), "q3": round(q3, 4),
                               "min": round(float(ratio.min()), 4),
                               "max": round(float(ratio.max()), 4),
                               "B_strictly_cheaper_share": round(float((ratio < 1.0).mean()), 4),
                               "A_strictly_cheaper_share": round(float((ratio > 1.0).mean()), 4)},
        "draws_skipped": {"focused_queries": int(reach0.sum()),
                          "mean_per_focused_iteration": round(float(B["skipped"].sum()) / max(focused_iters, 1), 3),
                          "max_per_query": int(B["skipped"].max()),
                          "full_miss_iterations": step["full_miss_iterations"],
                          "full_miss_share": round(step["full_miss_iterations"] / max(focused_iters, 1), 6),
                          "stepwise_ms_per_step": round(step["ms_per_step"], 4)},
    }
    txt = json.dumps(line)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()

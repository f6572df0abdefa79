"""Pruning by the focus bound (pp_star_prune) on config 5's batch: what the call
costs, what it takes out of the trees, and what the later steps and the paths gain or lose.

  python scripts/bench_star_prune.py [--queries 8192] [--first 1000] [--more 1000] [--reps 7]
                                     [--out profiles/star_prune.json]

The batch is built several times (the runs are deterministic, so no snapshot is needed).  Both
arms run --first steps and plan(goals, focus=True):
  arm A   --more further focused steps, then plan(goals)
  arm B   prune(keep=best_node), the same --more steps, then plan(goals)
The prune is timed on 1 + --reps freshly built batches (the first is the warm-up): wall time around
pp_synchronize of pp_star_revalidate (the unchanged scene: it keeps every node) and then of
pp_star_prune as RRTStarBatch.prune calls it (n_nodes and new_index copied to the host).  Three
more batches time pp_star_prune with every output NULL; the last of them goes on as arm B.  Prints
one JSON line and writes it to --out.
These are measurements, not thresholds."""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_prune.json"))
    args = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    space = rrt.Space.from_raw(raw)
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    goals = np.ascontiguousarray(goals, dtype=np.float64)
    sync = _ffi.lib().pp_synchronize

    def timed(b, fn):
        _ffi.check(sync(b.ctx.handle))
        t0 = time.perf_counter()
        r = fn()
        _ffi.check(sync(b.ctx.handle))
        return (time.perf_counter() - t0) * 1e3, r

    def start():
        b = rrt.RRTStarBatch(starts, args.first + args.more, raw["step_size"], space, seeds, k=0,
                             eta=scenes.CONFIG5_ETA)
        b.extend(args.first)
        node, cost0 = b.plan(goals, focus=True)
        return b, node, cost0

    def finish(b, out):
        ev0 = b.state()[2]
        ms, _ = timed(b, lambda: b.extend(args.more))
        out["ms_per_step"] = ms / args.more
        n, it, ev, rw = b.state()
        assert (it == args.first + args.more).all()
        out["node_evals"] = int((ev - ev0).sum())
        out["plan_ms"], (_, out["cost1"]) = timed(b, lambda: b.plan(goals))
        out["nodes"], out["rewires"] = int(n.sum()), int(rw.sum())
        b.close()
        return out

    b, _, _ = start()  # warm-up: module load, allocations
    finish(b, {})
    b, _, cost0 = start()
    A = finish(b, {"cost0": cost0})

    # --reps prunes as RRTStarBatch.prune makes them (new_index copied to the host), then three
    # with every output NULL: the device work and the one synchronise alone
    reval_ms, prune_ms, bare_ms = [], [], []
    bare = 3
    for rep in range(1 + args.reps + bare):
        b, node, cost0_b = start()
        n_before = b.state()[0]
        ms, _ = timed(b, lambda: b.revalidate(n_before))
        assert b.last_dropped == 0
        if rep <= args.reps:
            reval_ms.append(ms)
            ms, (n_after, _) = timed(b, lambda: b.prune(node, n_before))
            prune_ms.append(ms)
        else:
            keep = np.ascontiguousarray(node, dtype=np.int32)
            ms, rc = timed(b, lambda: _ffi.lib().pp_star_prune(
                b.ctx.handle, keep.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None))
            _ffi.check(rc)
            bare_ms.append(ms)
            assert np.array_equal(b.state()[0], n_after)
        if rep < args.reps + bare:
            b.close()
    assert np.array_equal(cost0_b, A["cost0"])
    B = finish(b, {"cost0": cost0_b})
    reval_ms, prune_ms = reval_ms[1:], prune_ms[1:]

    reach0 = np.isfinite(A["cost0"])
    ratio = B["cost1"][reach0] / A["cost1"][reach0]
    q1, q2, q3 = (float(v) for v in np.percentile(ratio, [25, 50, 75]))

    def side(r):
        return {"ms_per_step": round(r["ms_per_step"], 4), "node_evals": r["node_evals"],
                "final_plan_ms": round(r["plan_ms"], 3), "nodes": r["nodes"],
                "rewires": r["rewires"], "reachable_after": int(np.isfinite(r["cost1"]).sum())}

    line = {
        "workload": f"config 5's batch: {args.queries} queries, config-5 field, eta "
                    f"{scenes.CONFIG5_ETA}; {args.first} steps + plan(focus=True), then "
                    f"{args.more} focused steps (A) or prune(keep=best_node) and the same steps "
                    f"(B), then plan",
        "queries": args.queries, "first": args.first, "more": args.more,
        "reachable_at_first": int(reach0.sum()),
        "prune": {"nodes_before": int(n_before.sum()), "nodes_after": int(n_after.sum()),
                  "queries_pruned": int((n_after < n_before).sum()),
                  "reps": args.reps,
                  "prune_ms_median": round(float(np.median(prune_ms)), 4),
                  "prune_ms_min": round(min(prune_ms), 4), "prune_ms_max": round(max(prune_ms), 4),
                  "prune_null_outputs_ms": [round(v, 4) for v in bare_ms],
                  "revalidate_ms_median": round(float(np.median(reval_ms)), 4),
                  "revalidate_ms_min": round(min(reval_ms), 4),
                  "revalidate_ms_max": round(max(reval_ms), 4)},
        "A_focused": side(A), "B_pruned": side(B),
        "cost_B_over_cost_A": {"over": "queries reachable at the first plan", "q1": round(q1, 4),
                               "median": round(q2, 4), "q3": round(q3, 4),
                               "min": round(float(ratio.min()), 4),
                               "max": round(float(ratio.max()), 4),
                               "B_strictly_worse_share": round(float((ratio > 1.0).mean()), 4),
                               "B_strictly_cheaper_share": round(float((ratio < 1.0).mean()), 4)},
    }
    txt = json.dumps(line)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()

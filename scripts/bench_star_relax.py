"""Time and value of relaxing every RRT* tree (pp_star_relax, DESIGN.md §3.8 "Relaxing the trees")
on scripts/bench_star_repair.py's batch: config 5's (config3_queries on config5_field, --queries x
--iters, Steer eta 16), in two settings — the batch as grown, and the batch after
advance(best_node, hops=1, rounds=3).

  python scripts/bench_star_relax.py [--queries 8192] [--iters 2000] [--runs 7] [--extra 400]
                                     [--out profiles/star_relax.json]

Timed in one invocation, medians of --runs after a warm-up, wall time around pp_synchronize:
relax(1), relax(3) and relax(16), alternated, each on the setting's state restored (untimed) by
import_forest of one export.  Then, untimed and with profiling on, the rounds one by one
(relax(1) until a round re-parents nothing): nodes, candidates before and after each cull, edges
walked, re-parentings, costs changed, launches.  Then the value: pp_star_plan with the queries' own
goals before and after relax(16) — queries with a plan, median cost, plans that got cheaper or
dearer — and the same for a twin that spends the same wall time in pp_star_extend steps instead.
The call's device reservations are read as the drop of free device memory over the first call.
Prints one JSON line and writes it to --out.

Kernel trace of one call (a run of its own, no counters):
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python scripts/bench_star_relax.py --calls 2 --rounds 1"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_star_revalidate import med, sync  # noqa: E402  (sets up the import paths)
from bench_star_repair import grown  # noqa: E402

LAUNCHES_PER_SLICE = 5  # the task counter's memset, knn, prep, walk, choose


def relax(b, rounds):
    """(ms, n_rewired)"""
    sync(b.ctx)
    t0 = time.perf_counter()
    nrw = b.relax(rounds)
    sync(b.ctx)
    return (time.perf_counter() - t0) * 1e3, nrw


def free_bytes():
    try:
        import torch

        return int(torch.cuda.mem_get_info(0)[0])
    except Exception:  # noqa: BLE001  (no torch: the figure is left out)
        return None


def plan_figures(c0, c1):
    both = np.isfinite(c0) & np.isfinite(c1)
    fin = np.isfinite(c1)
    return {"queries_with_plan": int(fin.sum()),
            "plan_cost_median": round(float(np.median(c1[fin])), 6) if fin.any() else None,
            "plans_cheaper": int((c1[both] < c0[both]).sum()) + int((fin & ~np.isfinite(c0)).sum()),
            "plans_dearer": int((c1[both] > c0[both]).sum()) + int((~fin & np.isfinite(c0)).sum())}


def setting(name, b, st, goals, args, out):
    """the timings, the rounds and the value of one setting whose state is the export `st`"""
    if args.calls > 0:  # profiling: only the calls
        for _ in range(args.calls):
            b.import_forest(st)
            relax(b, args.rounds)
        return
    modes = [1, 3, 16]
    ms = {r: [] for r in modes}
    run = {r: 0 for r in modes}
    free0 = free_bytes()
    for i in range(args.runs + 1):  # (run 0: the warm-up)
        for r in modes:
            b.import_forest(st)
            t, _ = relax(b, r)
            run[r] = b.last_rounds
            if i == 0 and r == modes[0] and free0 is not None and "reserved_bytes" not in out:
                out["reserved_bytes"] = free0 - free_bytes()
            if i > 0:
                ms[r].append(t)
    for r in modes:
        out[f"{name}_relax{r}_ms"] = med(ms[r])
        out[f"{name}_relax{r}_ms_min"] = round(min(ms[r]), 3)
        out[f"{name}_relax{r}_ms_max"] = round(max(ms[r]), 3)
        out[f"{name}_relax{r}_rounds_run"] = run[r]
        out[f"{name}_relax{r}_ms_per_round"] = round(med(ms[r]) / max(run[r], 1), 3)
    # the rounds one by one, counted
    b.import_forest(st)
    b.set_profiling(True)
    rounds = []
    for _ in range(16):
        t, nrw = relax(b, 1)
        c = b.relax_counts()
        rounds.append({"ms_profiled": round(t, 3), "rewired": int(nrw.sum(dtype=np.int64)),
                       "changed": int(b.last_changed), "nodes": c["nodes"],
                       "candidates": c["candidates"], "after_parent_skip": c["not_parent"],
                       "after_cost_skip": c["cheaper"], "after_chord_bound_tasks": c["tasks"],
                       "edges_walked": c["walked"], "slices": c["slices"],
                       "launches": c["slices"] * LAUNCHES_PER_SLICE + 1})
        if rounds[-1]["rewired"] == 0:
            break
    b.set_profiling(False)
    out[f"{name}_rounds"] = rounds
    # the value: plans before and after, against the same wall time spent extending
    b.import_forest(st)
    _, c0 = b.plan(goals)
    sum0 = float(b.export_forest()["cost"].sum())
    t16, _ = relax(b, 16)
    _, c1 = b.plan(goals)
    out[f"{name}_cost_sum_before"] = round(sum0, 3)
    out[f"{name}_cost_sum_after_relax16"] = round(float(b.export_forest()["cost"].sum()), 3)
    out[f"{name}_before"] = plan_figures(c0, c0)
    out[f"{name}_after_relax16"] = plan_figures(c0, c1)
    b.import_forest(st)
    sync(b.ctx)
    t0 = time.perf_counter()
    b.extend(args.probe)
    sync(b.ctx)
    step_ms = (time.perf_counter() - t0) * 1e3 / args.probe
    steps = min(max(int(t16 / step_ms) - args.probe, 0), args.extra - args.probe)
    if steps > 0:
        b.extend(steps)
    _, c2 = b.plan(goals)
    out[f"{name}_extend_instead"] = dict(plan_figures(c0, c2), steps=steps + args.probe,
                                         step_ms=round(step_ms, 4), wall_ms_matched=round(t16, 3))


def run(args):
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    space = rrt.Space.from_raw(raw)
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    ctx = _ffi.Context(0)
    b = grown(args, raw, space, starts, seeds, ctx)
    n_old = b.state()[0]
    total = int(n_old.sum(dtype=np.int64))
    out = {"what": "pp_star_relax on config 5's batch: median wall ms around pp_synchronize, "
                   "1 x MI355X; the kNN is the one-wave-per-node self-join from global memory",
           "workload": f"config 5's batch: {args.queries} queries x {args.iters} iterations on "
                       f"{raw['name']}, eta {scenes.CONFIG5_ETA}",
           "queries": args.queries, "iters": args.iters, "runs": args.runs, "nodes": total}
    st = b.export_forest()
    setting("grown", b, st, goals, args, out)
    b.import_forest(st)
    node, _ = b.plan(goals)
    b.advance(node, hops=1, rounds=3, n_old=n_old)
    out["advanced_nodes"] = int(b.state()[0].sum(dtype=np.int64))
    setting("advanced", b, b.export_forest(), goals, args, out)
    ctx.close()
    return None if args.calls > 0 else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--extra", type=int, default=400, help="room for the twin's extend steps")
    ap.add_argument("--probe", type=int, default=20, help="extend steps timed for the twin's rate")
    ap.add_argument("--calls", type=int, default=0,
                    help="profiling: only this many calls per setting, no timing")
    ap.add_argument("--rounds", type=int, default=1, help="--calls: the rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_relax.json"))
    args = ap.parse_args()
    out = run(args)
    if out is None:
        return
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

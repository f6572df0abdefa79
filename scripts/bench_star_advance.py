"""Time and value of moving every RRT* tree's root one edge along its plan (pp_star_advance,
DESIGN.md §3.8 "Advancing the root") on scripts/bench_star_repair.py's batch: config 5's
(config3_queries on config5_field, --queries x --iters, Steer eta 16), after a plan.

  python scripts/bench_star_advance.py [--queries 8192] [--iters 2000] [--runs 7] [--extra 400]
                                       [--out profiles/star_advance.json]

Timed in one invocation, medians of --runs after a warm-up, wall time around pp_synchronize, the
batch grown again (untimed) before every call, alternated: advance(best_node, hops=1) at rounds
0, 1 and 3, and — the parent's call on the same batch, bench_star_repair.py's measurement —
pp_star_repair(rounds 1 and 3) under config5_field plus the 8 scaled discs.  A query without a
plan is left alone (node -1).  With each advance: the kept share, round 1's tops (one per advanced
query: one hop leaves the old root alone above the new one), the old roots that found no parent,
round 2's tops (the other children of those old roots that are not already kept), the re-attached
and recovered counts.  Then, untimed, the value: after the advance and --extra more steps, the
queries with a plan and their median cost for the rounds = 0 batch, the rounds = 3 batch and a
fresh batch planted at the new roots' poses with the same seeds and the same steps (what
reset_queries gives).  Prints one JSON line and writes it to --out.

Kernel trace of one call (a run of its own, no counters):
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python scripts/bench_star_advance.py --calls 2 --rounds 1"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_star_revalidate import discs_2048, med, sync  # noqa: E402  (sets up the import paths)
from bench_star_repair import change, grown  # noqa: E402


def advance(b, node, n_old, rounds):
    """(ms, n_nodes after, new_index)"""
    sync(b.ctx)
    t0 = time.perf_counter()
    n_new, idx = b.advance(node, hops=1, rounds=rounds, n_old=n_old)
    sync(b.ctx)
    return (time.perf_counter() - t0) * 1e3, n_new, idx


def plan_share(b, goals):
    _, c = b.plan(goals)
    fin = np.isfinite(c)
    return int(fin.sum()), round(float(np.median(c[fin])), 6) if fin.any() else None


def run(args):
    import revalidate_ref as ref
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    space = rrt.Space.from_raw(raw)
    space2 = rrt.Space.from_raw(ref.with_discs(raw, discs_2048(raw)))
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    ctx = _ffi.Context(0)
    b = grown(args, raw, space, starts, seeds, ctx)
    n_old = b.state()[0]
    node, cost0 = b.plan(goals)  # (every regrown batch holds the same trees)
    if args.calls > 0:  # profiling: only the calls
        for _ in range(args.calls):
            b = grown(args, raw, space, starts, seeds, ctx)
            advance(b, node, n_old, args.rounds)
        ctx.close()
        return None
    modes = [("advance0", 0), ("advance1", 1), ("advance3", 3), ("repair1", 1), ("repair3", 3)]
    ms = {name: [] for name, _ in modes}
    for i in range(args.runs + 1):  # (run 0: the warm-up)
        for name, rounds in modes:
            b = grown(args, raw, space, starts, seeds, ctx)
            if name.startswith("advance"):
                t = advance(b, node, n_old, rounds)[0]
            else:
                t = change(b, space2, n_old, rounds)[0]
                space._upload(ctx)
            if i > 0:
                ms[name].append(t)
    total = int(n_old.sum(dtype=np.int64))
    out = {"what": "pp_star_advance(best_node, hops = 1) against pp_star_repair on the same batch: "
                   "median wall ms around pp_synchronize, 1 x MI355X",
           "workload": f"config 5's batch: {args.queries} queries x {args.iters} iterations on "
                       f"{raw['name']}, eta {scenes.CONFIG5_ETA}; the repair under +8 discs",
           "queries": args.queries, "iters": args.iters, "runs": args.runs, "nodes": total,
           "queries_with_plan_before": int((node >= 0).sum()),
           "plan_cost_median_before": round(float(np.median(cost0[node >= 0])), 6)}
    for name, _ in modes:
        out[name + "_ms"] = med(ms[name])
        out[name + "_ms_min"] = round(min(ms[name]), 3)
        out[name + "_ms_max"] = round(max(ms[name]), 3)
    # what each advance keeps, and what grows from it
    off = np.concatenate([[0], np.cumsum(n_old, dtype=np.int64)])
    roots = None
    for name, rounds in modes[:3]:
        b = grown(args, raw, space, starts, seeds, ctx)
        par = b.export_forest()["parent"] if rounds == 1 else None
        _, n_new, idx = advance(b, node, n_old, rounds)
        moved = idx[off[:-1]] != 0  # the old root is no longer row 0
        out[name + "_advanced_queries"] = int(moved.sum())
        out[name + "_kept"] = int(n_new.sum(dtype=np.int64))
        out[name + "_kept_share"] = round(float(n_new.sum(dtype=np.int64)) / total, 6)
        out[name + "_kept_share_advanced"] = round(
            float(n_new[moved].sum(dtype=np.int64)) / max(int(n_old[moved].sum(dtype=np.int64)), 1), 6)
        out[name + "_tops_round1"] = int(moved.sum()) if rounds else 0
        out[name + "_reattached"] = b.last_reattached
        out[name + "_recovered"] = b.last_recovered
        if rounds:
            failed = moved & (idx[off[:-1]] < 0)
            out[name + "_old_roots_without_parent"] = int(failed.sum())
        if rounds == 1:  # round 2's tops: the dropped children of a failed old root
            tree_of = np.repeat(np.arange(args.queries), n_old)
            child = (par == 0) & failed[tree_of] & (idx < 0)
            out["tops_round2"] = int(child.sum())
        if rounds == 0:
            st = b.export_forest()
            o = st["off"][:-1]
            roots = np.stack([st["x"][o], st["y"][o], st["yaw"][o]], axis=1)
        if rounds in (0, 3):
            b.extend(args.extra)
            out[name + "_then_queries_with_plan"], out[name + "_then_plan_cost_median"] = \
                plan_share(b, goals)
            out[name + "_then_nodes"] = int(b.state()[0].sum(dtype=np.int64))
    f = rrt.RRTStarBatch(roots, args.iters + args.extra, raw["step_size"], space, seeds, k=0,
                         eta=scenes.CONFIG5_ETA, ctx=ctx)
    f.extend(args.extra)
    out["fresh_then_queries_with_plan"], out["fresh_then_plan_cost_median"] = plan_share(f, goals)
    out["fresh_then_nodes"] = int(f.state()[0].sum(dtype=np.int64))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--extra", type=int, default=400, help="the steps after the advance")
    ap.add_argument("--calls", type=int, default=0,
                    help="profiling: only this many calls, no timing")
    ap.add_argument("--rounds", type=int, default=1, help="--calls: the rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_advance.json"))
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

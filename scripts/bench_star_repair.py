"""Time and value of re-attaching dropped subtrees after a scene change (pp_star_repair, DESIGN.md
§3.8 "Re-attaching orphaned subtrees") on scripts/bench_star_revalidate.py's workload: config 5's
batch (config3_queries on config5_field, --queries x --iters, Steer eta 16) under config5_field
plus the 8 scaled discs.

  python scripts/bench_star_repair.py [--queries 8192] [--iters 2000] [--runs 7] [--extra 400]
                                      [--out profiles/star_repair.json]

Timed in one invocation, medians of --runs after a warm-up, wall time around pp_synchronize, the
batch grown again (untimed) before every call: pp_star_revalidate (the parent's call),
pp_star_repair(rounds = 1) and pp_star_repair(rounds = 3), alternated.  Then, untimed:
  - the nodes each keeps, the tops re-attached and the nodes recovered;
  - pp_star_plan for the queries' goals after each: the queries with a plan and their costs;
  - the pp_star_extend steps the pruned batch needs to hold as many nodes as the repaired one
    (the batches are made with --extra iterations of room for this).
Prints one JSON line and writes it to --out.

Kernel trace of one call (a run of its own, no counters):
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python scripts/bench_star_repair.py --calls 2 --rounds 1
  python scripts/bench_star_repair.py --trace-summary DIR rounds1 [profiles/star_repair.json]
(with a file: the summary is also stored in it under "kernel_trace_<label>")"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_star_revalidate import discs_2048, med, sync  # noqa: E402  (sets up the import paths)


def grown(args, raw, space, starts, seeds, ctx):
    from pathplanning_amd import rrt, scenes

    b = rrt.RRTStarBatch(starts, args.iters + args.extra, raw["step_size"], space, seeds, k=0,
                         eta=scenes.CONFIG5_ETA, ctx=ctx)
    b.extend(args.iters)
    return b


def change(b, space2, n_old, rounds):
    """the scene upload (untimed), then the call: (ms, n_nodes after); rounds None: revalidate"""
    space2._upload(b.ctx)
    sync(b.ctx)
    t0 = time.perf_counter()
    n_new, _ = b.revalidate(n_old) if rounds is None else b.repair(rounds, n_old)
    sync(b.ctx)
    return (time.perf_counter() - t0) * 1e3, n_new


def run(args):
    import revalidate_ref as ref
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    raw2 = ref.with_discs(raw, discs_2048(raw))
    space, space2 = rrt.Space.from_raw(raw), rrt.Space.from_raw(raw2)
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    ctx = _ffi.Context(0)
    if args.calls > 0:  # profiling: only the calls
        for _ in range(args.calls):
            b = grown(args, raw, space, starts, seeds, ctx)
            change(b, space2, b.state()[0], args.rounds)
        ctx.close()
        return None
    modes = [("revalidate", None), ("repair1", 1), ("repair3", 3)]
    ms = {name: [] for name, _ in modes}
    n_old = None
    for i in range(args.runs + 1):  # (run 0: the warm-up)
        for name, rounds in modes:
            b = grown(args, raw, space, starts, seeds, ctx)
            n_old = b.state()[0] if n_old is None else n_old
            t, _ = change(b, space2, n_old, rounds)
            if i > 0:
                ms[name].append(t)
    total = int(n_old.sum(dtype=np.int64))
    out = {"what": "pp_star_repair against pp_star_revalidate: median wall ms around "
                   "pp_synchronize, 1 x MI355X",
           "workload": f"config 5's batch: {args.queries} queries x {args.iters} iterations on "
                       f"{raw['name']}, eta {scenes.CONFIG5_ETA}, under +8 discs",
           "queries": args.queries, "iters": args.iters, "runs": args.runs, "nodes": total}
    for name, _ in modes:
        out[name + "_ms"] = med(ms[name])
        out[name + "_ms_min"] = round(min(ms[name]), 3)
        out[name + "_ms_max"] = round(max(ms[name]), 3)
    # value: what each keeps and what the goal connection finds on it
    cost, kept = {}, {}
    for name, rounds in modes:
        b = grown(args, raw, space, starts, seeds, ctx)
        b.set_profiling(True)
        _, n_new = change(b, space2, n_old, rounds)
        st = b.stats()
        b.set_profiling(False)
        kept[name] = int(n_new.sum(dtype=np.int64))
        out[name + "_kept"] = kept[name]
        out[name + "_walk_tasks"] = st["walk_tasks"]
        out[name + "_walk_points"] = st["walk_points"]
        if rounds is not None:
            out[name + "_reattached"] = b.last_reattached
            out[name + "_recovered"] = b.last_recovered
            extra_ms = out[name + "_ms"] - out["revalidate_ms"]
            out[name + "_extra_ms"] = round(extra_ms, 3)
            edges = st["walk_tasks"] - out["revalidate_walk_tasks"]
            out[name + "_candidate_edges"] = edges
            out[name + "_extra_us_per_reattached_top"] = round(extra_ms * 1e3 / max(b.last_reattached, 1), 3)
            out[name + "_extra_ns_per_candidate_edge"] = round(extra_ms * 1e6 / max(edges, 1), 2)
        _, c = b.plan(goals)
        cost[name] = c
        fin = np.isfinite(c)
        out[name + "_queries_with_plan"] = int(fin.sum())
        out[name + "_plan_cost_min"] = round(float(c[fin].min()), 6) if fin.any() else None
        out[name + "_plan_cost_median"] = round(float(np.median(c[fin])), 6) if fin.any() else None
    # plan costs, repair against revalidate, over the queries both plan for
    for name in ("repair1", "repair3"):
        both = np.isfinite(cost[name]) & np.isfinite(cost["revalidate"])
        out[name + "_plan_cheaper_queries"] = int((cost[name][both] < cost["revalidate"][both]).sum())
        out[name + "_plan_dearer_queries"] = int((cost[name][both] > cost["revalidate"][both]).sum())
        out[name + "_plan_cost_sum_both"] = round(float(cost[name][both].sum()), 3)
        out["revalidate_plan_cost_sum_both_" + name] = round(float(cost["revalidate"][both].sum()), 3)
    # the extend steps the pruned batch needs to hold the repaired batch's node count
    b = grown(args, raw, space, starts, seeds, ctx)
    change(b, space2, n_old, None)
    # (counted from the pruned batch for both: repair3's target lies past repair1's)
    sync(ctx)
    steps, t0 = 0, time.perf_counter()
    for name in ("repair1", "repair3"):
        target = kept[name]
        while steps < args.extra and int(b.state()[0].sum(dtype=np.int64)) < target:
            b.extend(args.chunk)
            steps += args.chunk
        sync(ctx)
        have = int(b.state()[0].sum(dtype=np.int64))
        out["extend_steps_to_" + name] = steps if have >= target else None
        out["extend_ms_to_" + name] = round((time.perf_counter() - t0) * 1e3, 3)
    ctx.close()
    return out


def trace_summary(d, label, out_path=None):
    """the last call of a `rocprofv3 --kernel-trace` run of `--calls N` under directory d (its
    dispatches from its first reval_emit_kernel to its reval_write_kernel), per kernel"""
    import csv
    import glob

    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(rows) if "reval_write_kernel" in r["Kernel_Name"]]
    e = ends[-1]
    prev = max([i for i in ends if i < e], default=-1)
    first = min(i for i in range(prev + 1, e + 1) if "reval_emit_kernel" in rows[i]["Kernel_Name"])
    seg = rows[first:e + 1]
    per = {}
    in_repair = False
    for r in seg:
        name = r["Kernel_Name"].rsplit("(", 1)[0].replace("void ", "").replace("ppamd::", "")
        name = name.split("<")[0]
        in_repair = in_repair or "repair_init_kernel" in name
        if in_repair and name.startswith("steer_"):  # the repair rounds' share of prep and walk
            name = "repair:" + name
        k = per.setdefault(name, {"calls": 0, "us": 0.0})
        k["calls"] += 1
        k["us"] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
    span = (int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) * 1e-3
    for k in per.values():
        k["us"] = round(k["us"], 1)
    out = {"what": f"one call ({label}), rocprofv3 --kernel-trace (no counters)",
           "dispatches": len(seg), "span_us": round(span, 1),
           "busy_us": round(sum(k["us"] for k in per.values()), 1), "kernels": per}
    print(json.dumps(out))
    if out_path:
        with open(out_path) as f:
            line = json.load(f)
        line["kernel_trace_" + label] = out
        with open(out_path, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


def main():
    if len(sys.argv) in (4, 5) and sys.argv[1] == "--trace-summary":
        return trace_summary(*sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--extra", type=int, default=400,
                    help="iterations of room past --iters (the pruned batch's catch-up)")
    ap.add_argument("--chunk", type=int, default=5, help="extend steps between two node counts")
    ap.add_argument("--calls", type=int, default=0,
                    help="profiling: only this many calls, no timing")
    ap.add_argument("--rounds", type=int, default=1, help="--calls: the rounds (-1: revalidate)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_repair.json"))
    args = ap.parse_args()
    if args.rounds < 0:
        args.rounds = None

    import __graft_entry__ as g
    g.build()
    line = run(args)
    if line is None:
        return
    print(json.dumps(line))
    with open(args.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

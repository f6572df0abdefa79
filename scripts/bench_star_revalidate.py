"""Time of keeping an RRT* batch's trees across a scene change (pp_star_revalidate, DESIGN.md §3.8
"RRT* trees"): config 5's batch (config3_queries on config5_field, --queries x --iters, Steer eta
16) under config5_field plus 8 discs (tests/revalidate_ref.extra_discs's draw, scaled from 512² to
the field's 2048²: centres U(0, 2048), r U(8, 32)).

  python scripts/bench_star_revalidate.py [--queries 8192] [--iters 2000] [--runs 7]
                                          [--out profiles/star_revalidate.json]

Medians of --runs after a warm-up, wall time around pp_synchronize:
  (a) pp_star_revalidate on the unchanged scene (nothing is dropped, so it repeats as it stands);
  (b) one pruning call: the scene upload, then pp_star_revalidate.  The batch has no import, so it
      is grown again before every call (untimed).  Walked points come from pp_stats in a profiled
      call of its own;
  (c) what a caller had before the call existed, timed in the same invocation: pp_star_new +
      pp_star_extend of the same iterations in the new scene.  The regrown trees are not the pruned
      trees (they hold the nodes --iters iterations insert in the new scene, the pruned batch holds
      what survives and goes on from its iteration counter), so both node counts are reported.
Prints one JSON line and writes it to --out.

Kernel trace of one pruning call (a run of its own, no counters):
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python scripts/bench_star_revalidate.py --calls 2
  python scripts/bench_star_revalidate.py --trace-summary DIR [profiles/star_revalidate.json]
(with a file: the summary is also stored in it under "kernel_trace")"""
import argparse
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


def med(v):
    return round(statistics.median(v), 3)


def discs_2048(raw, count=8, seed=77):
    """extra_discs's draw with the field's size and radii scaled by 4 (2048 / 512)"""
    import revalidate_ref as ref

    return [(cx, cy, 4.0 * r) for cx, cy, r in
            ref.extra_discs(raw, count, seed=seed, size=2048.0)]


def sync(ctx):
    from pathplanning_amd import _ffi

    _ffi.check(_ffi.lib().pp_synchronize(ctx.handle))


def grown(args, raw, space, starts, seeds, ctx):
    from pathplanning_amd import rrt, scenes

    b = rrt.RRTStarBatch(starts, args.iters, raw["step_size"], space, seeds, k=0,
                         eta=scenes.CONFIG5_ETA, ctx=ctx)
    b.extend(args.iters)
    return b


def prune(b, space2, n_old):
    """(upload ms, revalidate ms, n_nodes after)"""
    sync(b.ctx)
    t0 = time.perf_counter()
    space2._upload(b.ctx)
    t1 = time.perf_counter()
    n_new, _ = b.revalidate(n_old)
    sync(b.ctx)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, n_new


def run(args):
    import revalidate_ref as ref
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    raw2 = ref.with_discs(raw, discs_2048(raw))
    space, space2 = rrt.Space.from_raw(raw), rrt.Space.from_raw(raw2)
    starts, _, seeds = scenes.config3_queries(raw, 0, args.queries)
    ctx = _ffi.Context(0)
    if args.calls > 0:  # profiling: only the pruning calls
        for _ in range(args.calls):
            b = grown(args, raw, space, starts, seeds, ctx)
            prune(b, space2, b.state()[0])
        ctx.close()
        return None
    # (a) the unchanged scene
    b = grown(args, raw, space, starts, seeds, ctx)
    n_old = b.state()[0]
    total = int(n_old.sum(dtype=np.int64))
    same = []
    for i in range(args.runs + 1):  # (run 0: the warm-up)
        sync(ctx)
        t0 = time.perf_counter()
        n_same, _ = b.revalidate(n_old)
        sync(ctx)
        if i > 0:
            same.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(n_same, n_old) and b.last_dropped == 0
    # (b) one pruning call and (c) the regrowth in the new scene, alternated
    up, rv, regrow = [], [], []
    for i in range(args.runs + 1):
        b = grown(args, raw, space, starts, seeds, ctx)
        a, r, n_new = prune(b, space2, n_old)
        sync(ctx)
        t0 = time.perf_counter()
        g = grown(args, raw2, space2, starts, seeds, ctx)  # (its scene upload included)
        sync(ctx)
        t1 = time.perf_counter()
        if i > 0:
            up.append(a)
            rv.append(r)
            regrow.append((t1 - t0) * 1e3)
    n_regrown = g.state()[0]
    # walked points: a profiled call of its own
    b = grown(args, raw, space, starts, seeds, ctx)
    b.set_profiling(True)
    prune(b, space2, n_old)
    st = b.stats()
    b.set_profiling(False)
    call = med([x + y for x, y in zip(up, rv)])
    out = {"what": "pp_star_revalidate: median wall ms around pp_synchronize, 1 x MI355X",
           "workload": f"config 5's batch: {args.queries} queries x {args.iters} iterations on "
                       f"{raw['name']}, eta {scenes.CONFIG5_ETA}, under +8 discs",
           "queries": args.queries, "iters": args.iters, "runs": args.runs, "nodes": total,
           "unchanged_scene_ms": med(same), "unchanged_scene_ms_min": round(min(same), 3),
           "unchanged_scene_ms_max": round(max(same), 3),
           "unchanged_scene_nodes_per_s": round(total / (med(same) * 1e-3)),
           "kept": int(n_new.sum(dtype=np.int64)),
           "dropped": total - int(n_new.sum(dtype=np.int64)),
           "queries_pruned": int((n_new < n_old).sum()),
           "queries_root_only": int((n_new == 1).sum()),
           "space_new_ms": med(up), "revalidate_ms": med(rv),
           "revalidate_ms_min": round(min(rv), 3), "revalidate_ms_max": round(max(rv), 3),
           "nodes_per_s": round(total / (med(rv) * 1e-3)), "set_space_ms": call,
           "walk_points": st["walk_points"], "walk_tasks": st["walk_tasks"],
           "regrow_ms": med(regrow), "regrow_ms_min": round(min(regrow), 3),
           "regrow_ms_max": round(max(regrow), 3),
           "regrown_nodes": int(n_regrown.sum(dtype=np.int64)),
           "regrow_over_set_space": round(med(regrow) / call, 2)}
    ctx.close()
    return out


def trace_summary(d, out_path=None):
    """the last pruning call of a `rocprofv3 --kernel-trace` run of `--calls N` under directory d
    (its dispatches from its first reval_emit_kernel to its reval_write_kernel), per kernel"""
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
    for r in seg:
        name = r["Kernel_Name"].rsplit("(", 1)[0].replace("void ", "").replace("ppamd::", "")
        name = name.split("<")[0]
        k = per.setdefault(name, {"calls": 0, "us": 0.0})
        k["calls"] += 1
        k["us"] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
    span = (int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) * 1e-3
    for k in per.values():
        k["us"] = round(k["us"], 1)
    out = {"what": "one pruning pp_star_revalidate call, rocprofv3 --kernel-trace (no counters)",
           "dispatches": len(seg), "span_us": round(span, 1),
           "busy_us": round(sum(k["us"] for k in per.values()), 1), "kernels": per}
    print(json.dumps(out))
    if out_path:
        with open(out_path) as f:
            line = json.load(f)
        line["kernel_trace"] = out
        with open(out_path, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


def main():
    if len(sys.argv) in (3, 4) and sys.argv[1] == "--trace-summary":
        return trace_summary(*sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=0,
                    help="profiling: only this many pruning calls, no timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "star_revalidate.json"))
    args = ap.parse_args()

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

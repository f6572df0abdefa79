"""Time of keeping a tree across a scene change (pp_rrt_revalidate / pp_batch_revalidate, DESIGN.md
§3.8): config 2's tree (field512, seed 42, grown to --nodes) and config 3's query batch
(config3_queries on field512, --queries x --iters), each under field512 plus 8 discs
(tests/revalidate_ref.extra_discs).

  python scripts/bench_revalidate.py [--nodes 100000] [--queries 8192] [--iters 2000] [--runs 7]
                                     [--out profiles/revalidate.json]

One tree: the median wall time around pp_synchronize of the in-place call (the scene upload
pp_space_new, then pp_rrt_revalidate with new_index), alternated in the same invocation with the
host route a caller without the call has: pp_rrt_tree_export, pp_space_new, pp_rrt_new,
pp_rrt_tree_import, pp_rrt_verify_node_batch over every node, the propagation to descendants and
the compaction on the host (numpy, pointer doubling), pp_rrt_tree_import of the result.  The tree is
restored by pp_rrt_tree_import before every call and both routes must give the same tree.  The
batch has no import: it is grown again before every call (untimed), and has no host route.
Walked points come from pp_stats in a profiled call of its own.  Prints one JSON line and writes
it to --out.

Kernel trace of one call (a run of its own, no counters):
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python scripts/bench_revalidate.py --calls 2
  python scripts/bench_revalidate.py --trace-summary DIR [profiles/revalidate.json]
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


def planner(raw, ctx, seed=42, window=4096, capacity=1 << 18):
    from pathplanning_amd import rrt

    sx, sy, syaw = raw["start"]
    gx, gy, gyaw = raw["goal"]
    return rrt.RRT((sx, sy), syaw, (gx, gy), gyaw, raw["max_iter"], raw["step_size"],
                   rrt.Space.from_raw(raw), seed=seed, window=window, capacity=capacity, ctx=ctx)


def in_place(p, space2, n_old):
    """(upload ms, revalidate ms, n_kept, new_index)"""
    p.synchronize()
    t0 = time.perf_counter()
    space2._upload(p.ctx)
    t1 = time.perf_counter()
    kept, new_index = p.revalidate(n_old)
    p.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, kept, new_index


def host_route(p, raw2, ctx):
    """the same result through the calls a caller had before; (ms by stage, planner, new_index)"""
    ms = {}
    p.synchronize()
    t = [time.perf_counter()]

    def lap(name):
        t.append(time.perf_counter())
        ms[name] = round((t[-1] - t[-2]) * 1e3, 3)

    x, y, yaw, par = p.tree()
    lap("export")
    q = planner(raw2, ctx)  # pp_space_new + pp_rrt_new
    lap("space_new_rrt_new")
    q.tree_import(x, y, yaw, par)
    lap("import")
    ok, _ = q.verify_node_batch(x[1:], y[1:], par[1:])
    lap("verify_node_batch")
    n = len(x)
    bad = np.concatenate([[False], ~ok])
    anc = np.concatenate([[0], par[1:]]).astype(np.int64)
    while True:  # pointer doubling: parents precede children
        nb = bad | bad[anc]
        na = anc[anc]
        if np.array_equal(na, anc) and np.array_equal(nb, bad):
            break
        bad, anc = nb, na
    keep = ~bad
    keep[0] = True
    new_index = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    npar = par[keep].astype(np.int32)
    npar[1:] = new_index[npar[1:]]
    lap("host_propagate_compact")
    q.tree_import(x[keep], y[keep], yaw[keep], npar)
    q.synchronize()
    lap("reimport")
    ms["total"] = round((t[-1] - t[0]) * 1e3, 3)
    assert n == len(new_index)
    return ms, q, new_index


def med(v):
    return round(statistics.median(v), 3)


def one_tree(args, raw, raw2):
    from pathplanning_amd import _ffi, rrt

    ctx = _ffi.Context(0)
    p = planner(raw, ctx)
    while p.tree_size() < args.nodes:
        p.extend(4096)
    tree0 = p.tree()
    n = len(tree0[0])
    space2 = rrt.Space.from_raw(raw2)
    if args.calls > 0:  # profiling: only the in-place calls
        for _ in range(args.calls):
            p = planner(raw, ctx)
            p.tree_import(*tree0)
            in_place(p, space2, n)
        return None
    up, rv, host = [], [], []
    stages = {}
    for i in range(args.runs + 1):  # (run 0: the warm-up)
        p = planner(raw, ctx)
        p.tree_import(*tree0)
        a, b, kept, new_index = in_place(p, space2, n)
        got = p.tree()
        p = planner(raw, ctx)
        p.tree_import(*tree0)
        ms, q, new_index_h = host_route(p, raw2, ctx)
        assert np.array_equal(new_index, new_index_h), "host route != in-place call"
        for u, v in zip(got, q.tree()):
            assert np.array_equal(u, v), "host route != in-place call"
        if i > 0:
            up.append(a)
            rv.append(b)
            host.append(ms["total"])
            for k, v in ms.items():
                stages.setdefault(k, []).append(v)
    # walked points: a profiled call of its own
    p = planner(raw, ctx)
    p.tree_import(*tree0)
    p.set_profiling(True)
    p.reset_stats()
    in_place(p, space2, n)
    st = p.stats()
    p.set_profiling(False)
    call = med([a + b for a, b in zip(up, rv)])
    out = {"workload": f"config 2's tree ({raw['name']}, seed 42) at {n} nodes under +8 discs",
           "nodes": n, "kept": int(kept), "runs": args.runs,
           "in_place_ms": call, "space_new_ms": med(up), "revalidate_ms": med(rv),
           "revalidate_ms_min": round(min(rv), 3), "revalidate_ms_max": round(max(rv), 3),
           "nodes_per_s": round(n / (med(rv) * 1e-3)),
           "walk_points": st["walk_points"], "walk_tasks": st["walk_tasks"],
           "host_route_ms": med(host), "host_route_stages_ms": {k: med(v) for k, v in stages.items()},
           "host_route_over_in_place": round(med(host) / call, 2)}
    ctx.close()
    return out


def batch(args, raw, raw2):
    from pathplanning_amd import _ffi, rrt, scenes

    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    space, space2 = rrt.Space.from_raw(raw), rrt.Space.from_raw(raw2)
    ctx = _ffi.Context(0)
    up, rv = [], []
    runs = args.calls if args.calls > 0 else args.runs + 1
    for i in range(runs):
        b = rrt.RRTBatch(starts, goals, args.iters, raw["step_size"], space, seeds, ctx=ctx)
        b.extend(args.iters)
        n_old = b.state()[0]
        _ffi.check(_ffi.lib().pp_synchronize(ctx.handle))
        t0 = time.perf_counter()
        space2._upload(ctx)
        t1 = time.perf_counter()
        n_new, _ = b.revalidate(n_old)
        _ffi.check(_ffi.lib().pp_synchronize(ctx.handle))
        t2 = time.perf_counter()
        if i > 0:
            up.append((t1 - t0) * 1e3)
            rv.append((t2 - t1) * 1e3)
    if args.calls > 0:
        return None
    b = rrt.RRTBatch(starts, goals, args.iters, raw["step_size"], space, seeds, ctx=ctx)
    b.extend(args.iters)
    n_old = b.state()[0]
    b.set_profiling(True)
    space2._upload(ctx)
    b.revalidate(n_old)
    st = b.stats()
    total = int(n_old.sum(dtype=np.int64))
    out = {"workload": f"config 3's batch: {args.queries} queries x {args.iters} iterations on "
                       f"{raw['name']} under +8 discs",
           "queries": args.queries, "iters": args.iters, "nodes": total,
           "kept": int(n_new.sum(dtype=np.int64)),
           "queries_pruned": int((n_new < n_old).sum()), "runs": args.runs,
           "space_new_ms": med(up), "revalidate_ms": med(rv),
           "revalidate_ms_min": round(min(rv), 3), "revalidate_ms_max": round(max(rv), 3),
           "nodes_per_s": round(total / (med(rv) * 1e-3)),
           "walk_points": st["walk_points"], "walk_tasks": st["walk_tasks"]}
    ctx.close()
    return out


def trace_summary(d, out_path=None):
    """the last revalidate call of a `rocprofv3 --kernel-trace` run of `--calls N` under directory
    d (its dispatches from its first reval_emit_kernel to its reval_write_kernel), per kernel"""
    import csv
    import glob

    rows = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ends = [i for i, r in enumerate(rows) if "reval_write_kernel" in r["Kernel_Name"]]
    out = []
    for which, e in (("one tree", ends[len(ends) // 2 - 1]), ("batch", ends[-1])):
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
        out.append({"what": f"one revalidate call ({which}), rocprofv3 --kernel-trace (no counters)",
                    "dispatches": len(seg), "span_us": round(span, 1),
                    "busy_us": round(sum(k["us"] for k in per.values()), 1), "kernels": per})
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
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=0,
                    help="profiling: only this many in-place calls per workload, no timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "revalidate.json"))
    args = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    import revalidate_ref as ref
    from pathplanning_amd import scenes

    raw = scenes.field512()
    raw2 = ref.with_discs(raw, ref.extra_discs(raw, 8))
    tree = one_tree(args, raw, raw2)
    forest = batch(args, raw, raw2)
    if args.calls > 0:
        return
    line = {"what": "pp_rrt_revalidate / pp_batch_revalidate: median wall ms around "
                    "pp_synchronize, 1 x MI355X", "one_tree": tree, "batch": forest}
    print(json.dumps(line))
    with open(args.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

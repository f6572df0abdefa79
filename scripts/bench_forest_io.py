"""Packed forest export / import (pp_star_forest_export / pp_star_forest_import) on
config 5's batch: what a checkpoint, a restore and a recycling of slots cost, against the only
route there was before — a pp_star_tree_export loop, one copy set and one synchronisation per
query.

  python scripts/bench_forest_io.py [--queries 8192] [--iters 2000] [--reps 7] [--loop 256]
                                    [--parent-root DIR] [--out profiles/forest_io.json]

One batch is grown --iters steps.  Every figure is the median of --reps calls after one warm-up
call, wall time around the call (the calls synchronise themselves); all copies go to or come from
pageable host memory (numpy arrays), as pp_star_paths' do:
  sizes_only_ms     pp_star_forest_export with no row array: off, the per-slot arrays, n_total
  export_ms         the same call with every array, into arrays allocated and touched before
  export_method_ms  RRTStarBatch.export_forest(): both calls and the allocation of the arrays
  import_ms         RRTStarBatch.import_forest(state) of the whole exported state (with cost: checked)
  reset_ms          RRTStarBatch.reset_queries of every 8th slot
  loop_ms           RRTStarBatch.tree(q, n) (pp_star_tree_export; no edge costs, counters or focus)
                    over the first --loop queries, scaled to the batch: an extrapolation
--parent-root: a built checkout of the parent commit; pp_star_extend's rate is then measured in
child processes, parent and change alternating, three pairs (--rate-only --root DIR is the child's
mode: the package and library of that checkout, as built).
These are measurements, not thresholds."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop", type=int, default=256)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--rate-only", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_io.json"))
    args = ap.parse_args()

    root = os.path.abspath(args.root) if args.root else ROOT
    for p in (os.path.join(root, "rs-pathplanning_amd"), root):
        sys.path.insert(0, p)
    if not args.root:
        import __graft_entry__ as g
        g.build()
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    space = rrt.Space.from_raw(raw)
    starts, _, seeds = scenes.config3_queries(raw, 0, args.queries)
    b = rrt.RRTStarBatch(starts, args.iters, raw["step_size"], space, seeds, k=0,
                         eta=scenes.CONFIG5_ETA)
    t0 = time.perf_counter()
    it, _, _ = b.extend(args.iters)
    rate = it / (time.perf_counter() - t0)
    if args.rate_only:
        print(json.dumps({"extend_it_per_s": rate}))
        b.close()
        return

    def med(fn, reps=args.reps):
        fn()  # the warm-up: allocations, first-touch
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3),
                "max": round(max(ms), 3)}

    L = _ffi.lib()
    Q = args.queries
    state = b.export_forest()
    total = int(state["off"][Q])
    tot = C.c_int64(0)
    sizes = {k: np.zeros_like(v) for k, v in state.items() if len(v) in (Q, Q + 1)}
    sizes["focus_xy"] = np.zeros(2 * Q)
    st_sizes = rrt._forest_struct("s", sizes)
    full = {k: np.zeros_like(v).reshape(-1) for k, v in state.items()}
    st_full = rrt._forest_struct("s", full)

    def call(st, cap):
        _ffi.check(L.pp_star_forest_export(b.ctx.handle, None, Q, C.byref(st), cap, C.byref(tot)))

    out = {"sizes_only_ms": med(lambda: call(st_sizes, 0)),
           "export_ms": med(lambda: call(st_full, total))}
    assert all(np.array_equal(full[k], state[k].reshape(-1)) for k in state)
    out["export_method_ms"] = med(lambda: b.export_forest())
    out["import_ms"] = med(lambda: b.import_forest(state))
    again = b.export_forest()
    assert all(np.array_equal(again[k], state[k]) for k in state)
    n = state["off"][1:] - state["off"][:-1]
    loop = min(args.loop, Q)

    def tree_loop():
        for q in range(loop):
            b.tree(q, int(n[q]))

    lm = med(tree_loop, 3)
    out["loop_ms"] = {"queries": loop, "measured_median": lm["median"],
                      "extrapolated_to_batch": round(lm["median"] * Q / loop, 1),
                      "note": "extrapolation: the loop over the first queries, scaled by "
                              "queries / loop"}
    slots = np.arange(0, Q, 8, dtype=np.int32)
    out["reset_ms"] = dict(med(lambda: b.reset_queries(slots, starts[slots], seeds[slots])),
                           slots=len(slots))
    b.close()

    rates = None
    if args.parent_root:
        rates = {"parent": [], "change": []}
        for _ in range(3):
            for side in ("parent", "change"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rate-only",
                                    "--root", args.parent_root if side == "parent" else ROOT,
                                    "--queries", str(Q), "--iters", str(args.iters)],
                                   capture_output=True, text=True, check=True, timeout=300)
                rates[side].append(round(json.loads(r.stdout.strip().splitlines()[-1])
                                         ["extend_it_per_s"] / 1e6, 3))
    line = {
        "workload": f"config 5's batch: {Q} queries x {args.iters} iterations, config-5 field, "
                    f"eta {scenes.CONFIG5_ETA}; median of {args.reps} calls after a warm-up, wall "
                    f"time around each call, pageable host memory",
        "queries": Q, "iterations": args.iters, "nodes": total,
        "bytes_per_node": 44, "extend_it_per_s_this_process_M": round(rate / 1e6, 3),
        **out,
        "export_over_loop": round(out["loop_ms"]["extrapolated_to_batch"]
                                  / out["export_ms"]["median"], 1),
        "extend_M_it_per_s_alternated": rates,
    }
    txt = json.dumps(line)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()

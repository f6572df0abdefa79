"""Time of the segment export and the sampler on config 5's batch (the config-5 field, RRT*, 8192
queries x 2000 iterations: plan(goals), then the best nodes' paths), beside the point export of the
same paths in the same process.  The trees are grown first (untimed).

  python scripts/bench_path_segments.py [--queries 8192] [--iters 2000] [--runs 7]
                                        [--out profiles/path_segments.json]

Prints one JSON line and writes it to --out.  Per call: the median wall time of `runs` calls after
a warm-up (the C call with buffers sized beforehand, the device-to-host copies included; every call
ends in a stream synchronise) and the bytes it returns:
  sizes_only       pp_star_path_segments without arrays (off, ok, n_total)
  path_segments    pp_star_path_segments(goals, best): five arrays, off, length, ok
  sample_segments  pp_segments_sample at ds = step_size (step_size x R, the polyline's own
                   spacing, when that would pass one call's 2^26 samples): the five segment arrays
                   go up, five sample arrays come back (its sizes-only call is timed beside it)
  paths            pp_star_paths(goals, best): x, y, off, length — for comparison
It also checks that both exports describe the same paths: equal ok flags, and every polyline's
length within the chord bound of its row's arc length."""
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


def med(ms):
    return {"ms": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
            "ms_max": round(max(ms), 3), "runs": len(ms)}


def timed(fn, runs):
    """wall ms of `runs` calls of fn after one warm-up; the last result"""
    ms, out = [], None
    for i in range(runs + 1):
        t0 = time.perf_counter()
        out = fn()
        if i > 0:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_segments.json"))
    args = ap.parse_args()

    import __graft_entry__ as g
    g.build()
    from pathplanning_amd import _ffi, rrt, scenes

    raw = scenes.config5_field()
    step = float(raw["step_size"])
    starts, goals, seeds = scenes.config3_queries(raw, 0, args.queries)
    goals = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 3)
    space = rrt.Space.from_raw(raw)
    R = float(space.get_steer())
    b = rrt.RRTStarBatch(starts, args.iters, step, space, seeds, k=0, eta=scenes.CONFIG5_ETA)
    b.extend(args.iters)
    plan_ms, (node, _) = timed(lambda: b.plan(goals), args.runs)
    best = np.ascontiguousarray(node, dtype=np.int32)
    Q = b.q
    L = _ffi.lib()
    ip, dp, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    u8 = C.POINTER(C.c_uint8)
    h = b.ctx.handle
    G, N = goals.ctypes.data_as(dp), best.ctypes.data_as(ip)
    off = np.zeros(Q + 1, dtype=np.int64)
    ok = np.zeros(Q, dtype=np.uint8)
    length = np.zeros(Q)
    tot = C.c_int64(0)
    O, K = off.ctypes.data_as(i64), ok.ctypes.data_as(u8)

    def seg_sizes():
        _ffi.check(L.pp_star_path_segments(h, G, N, 1, O, None, 0, C.byref(tot), None, K))
        return tot.value

    size_ms, nseg = timed(seg_sizes, args.runs)
    seg = {f: np.zeros(max(nseg, 1)) for f in _ffi.SEGMENT_FIELDS}
    st, _keep = rrt._segments_struct(seg)

    def seg_call():
        _ffi.check(L.pp_star_path_segments(h, G, N, 1, O, C.byref(st), nseg, C.byref(tot),
                                           length.ctypes.data_as(dp), K))
        return tot.value

    seg_ms, got = timed(seg_call, args.runs)
    assert got == nseg
    seg_off, seg_len, seg_ok = off.copy(), length.copy(), ok.copy()

    # the sampler at the polyline's own spacing
    poff = np.zeros(Q + 1, dtype=np.int64)
    SO, PO = seg_off.ctypes.data_as(i64), poff.ctypes.data_as(i64)

    ds = step

    def samp_sizes():
        _ffi.check(L.pp_segments_sample(h, Q, SO, C.byref(st), ds, PO, None, None, None, None,
                                        None, 0, C.byref(tot)))
        return tot.value

    try:
        ssize_ms, nsamp = timed(samp_sizes, args.runs)
    except _ffi.PPError as e:  # more than one call's 2^26 samples: the polyline's own spacing
        if e.code != _ffi.PP_ERR_CAPACITY:
            raise
        ds = step * R
        ssize_ms, nsamp = timed(samp_sizes, args.runs)
    outs = [np.zeros(max(nsamp, 1)) for _ in range(5)]
    optr = [a.ctypes.data_as(dp) for a in outs]

    def samp_call():
        _ffi.check(L.pp_segments_sample(h, Q, SO, C.byref(st), ds, PO, *optr, nsamp,
                                        C.byref(tot)))
        return tot.value

    samp_ms, got = timed(samp_call, args.runs)
    assert got == nsamp

    # the point export of the same paths
    def pts_sizes():
        _ffi.check(L.pp_star_paths(h, G, N, O, None, None, 0, C.byref(tot), None, None))
        return tot.value

    npts = pts_sizes()
    x, y = np.zeros(max(npts, 1)), np.zeros(max(npts, 1))
    plen = np.zeros(Q)
    pok = np.zeros(Q, dtype=np.uint8)

    def pts_call():
        _ffi.check(L.pp_star_paths(h, G, N, O, x.ctypes.data_as(dp), y.ctypes.data_as(dp), npts,
                                   C.byref(tot), plen.ctypes.data_as(dp), pok.ctypes.data_as(u8)))
        return tot.value

    pts_ms, got = timed(pts_call, args.runs)
    assert got == npts
    # the two exports describe the same paths: equal flags, the polyline's length within the
    # chord bound of the arc length (the points are step R of arc apart: 1 - step^2 / 24)
    assert np.array_equal(pok, seg_ok)
    has = seg_ok.astype(bool)
    assert np.all(plen[has] <= seg_len[has] + 1e-9)
    assert np.all(seg_len[has] * (1.0 - step * step / 24.0) - 1e-9 <= plen[has])
    n_paths = int(has.sum())
    line = {
        "what": "segment export and sampling vs the point export: wall ms around the call, copies included",
        "workload": (f"pp_star_plan, then the best nodes' paths: {args.queries} queries x "
                     f"{args.iters} RRT* iterations, the config-5 field, eta {scenes.CONFIG5_ETA}, "
                     f"R {R}, step {step}"),
        "queries": args.queries, "iters": args.iters, "queries_with_path": n_paths,
        "plan": med(plan_ms),
        "sizes_only": dict(med(size_ms), bytes=int(8 * (Q + 1) + Q + 8)),
        "path_segments": dict(med(seg_ms), segments=int(nseg),
                              segments_per_path=round(nseg / max(n_paths, 1), 1),
                              bytes=int(40 * nseg + 8 * (Q + 1) + 8 * Q + Q)),
        "sample_segments": dict(med(samp_ms), ds=ds, samples=int(nsamp),
                                bytes=int(40 * nsamp + 8 * (Q + 1)),
                                bytes_uploaded=int(40 * nseg + 8 * (Q + 1)),
                                sizes_only=med(ssize_ms)),
        "paths": dict(med(pts_ms), points=int(npts), points_per_path=round(npts / max(n_paths, 1), 1),
                      bytes=int(16 * npts + 8 * (Q + 1) + 8 * Q + Q)),
    }
    line["ratio_paths_over_segments_ms"] = round(line["paths"]["ms"] / line["path_segments"]["ms"], 2)
    line["ratio_paths_over_segments_bytes"] = round(line["paths"]["bytes"] / line["path_segments"]["bytes"], 1)
    print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
    b.close()


if __name__ == "__main__":
    main()

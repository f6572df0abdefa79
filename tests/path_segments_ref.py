"""CPU restatement of the segment export and the sampler (pp_star_path_segments,
pp_batch_path_segments, pp_segments_sample; DESIGN.md §3.7 "Segment export and sampling"), plain
Python over dubins_py's word functions and WORD_MODES.  A helper module (no fixtures).

An edge a -> b: the local coordinates of dubins_path_planning (dubins.rs:401-411), the word
selection of dubins_path_planning_from_origin (dubins.rs:333-363), then three segments — start
pose, signed curvature (+1/R L, 0 S, -1/R R), length (t | p | q) * R — each starting at the
closed-form end of the one before.  A row is the edges of a chain of poses, three segments each;
`reverse` is the same curve from its other end.  The sampler walks a row by arc position.
"""
import math

import numpy as np

import dubins_py as dpy
import oracle

FIELDS = ("x", "y", "yaw", "kappa", "len")


def edge_word(a, b, R, step=None):
    """(word, (t, p, q)) of the edge a -> b (poses (x, y, yaw)), or None.  step: also assert that
    oracle.dubins chooses the same word for it."""
    (ax, ay, ayaw), (bx, by, byaw) = a, b
    exr = bx - ax
    eyr = by - ay
    c = 1.0 / R
    lex = math.cos(ayaw) * exr + math.sin(ayaw) * eyr
    ley = -(math.sin(ayaw)) * exr + math.cos(ayaw) * eyr
    leyaw = byaw - ayaw
    d = dpy.libm_hypot(lex, ley) * c
    theta = dpy.mod2pi(math.atan2(ley, lex))
    alpha = dpy.mod2pi(-theta)
    beta = dpy.mod2pi(leyaw - theta)
    best, bcost = None, math.inf
    for i, f in enumerate(dpy.ALL_PLANNERS):
        r = f(alpha, beta, d)
        if r is not None:
            cost = abs(r[0]) + abs(r[1]) + abs(r[2])
            if bcost > cost:
                best, bcost = (i, r), cost
    if step is not None:
        od = oracle.dubins(ax, ay, ayaw, bx, by, byaw, R, step)
        assert (od is None) == (best is None)
        assert od is None or od[3] == best[0], (a, b, od[3], best[0])
    return best


def seg_end(x, y, yaw, k, u):
    """the pose u along a segment of signed curvature k from (x, y, yaw)"""
    if k == 0.0:
        return x + u * math.cos(yaw), y + u * math.sin(yaw), yaw
    yaw1 = yaw + k * u
    return (x + (math.sin(yaw1) - math.sin(yaw)) / k, y - (math.cos(yaw1) - math.cos(yaw)) / k,
            yaw1)


def edge_segments(a, b, R, step=None):
    """(word, [(x, y, yaw, kappa, len)] * 3) of the edge a -> b, or None"""
    w = edge_word(a, b, R, step)
    if w is None:
        return None
    word, tpq = w
    x, y, yaw = (float(v) for v in a)
    segs = []
    for j in range(3):
        m = dpy.WORD_MODES[word][j]
        k = 0.0 if m == dpy.S else (1.0 / R if m == dpy.L else -(1.0 / R))
        ln = tpq[j] * R
        segs.append((x, y, yaw, k, ln))
        x, y, yaw = seg_end(x, y, yaw, k, ln)
    return word, segs


def row_end(row):
    """the end pose of a row's last segment"""
    return seg_end(*(row[f][-1] for f in FIELDS))


def chain_row(poses, R, step=None):
    """(row, words): the segments of the edges poses[e] -> poses[e + 1], every edge from its own
    pose; None when the first edge has no word (an empty row); a later edge without one raises"""
    segs, words = [], []
    for e in range(len(poses) - 1):
        r = edge_segments(poses[e], poses[e + 1], R, step)
        if r is None:
            if e == 0:
                return None
            raise RuntimeError("an edge of the chain has no Dubins word")
        words.append(r[0])
        segs.extend(r[1])
    a = np.array(segs, dtype=np.float64).reshape(-1, 5)
    return {f: a[:, i].copy() for i, f in enumerate(FIELDS)}, words


def star_poses(tree, goal, node):
    """pp_star_paths' chain: the goal, then the stored poses of node, its parent, ..., the root"""
    x, y, yaw, par = tree[:4]
    poses = [tuple(float(v) for v in goal)]
    v = int(node)
    while v >= 0:
        poses.append((float(x[v]), float(y[v]), float(yaw[v])))
        v = int(par[v])
    return poses


def finalize_poses(tree, goal, node, chain):
    """finalize's chain (rrt.rs:503-540) of check_finish(node): the goal, optimize's copies (at
    the node / the chosen ancestors, yaw by compute_yaw toward the next one; `chain` =
    oracle.check_finish's), then the stored poses of the last chosen ancestor (or the node) down
    to the root"""
    x, y, yaw, par = tree[:4]
    poses = [tuple(float(v) for v in goal)]
    here = int(node)
    for to in chain:
        poses.append((float(x[here]), float(y[here]),
                      math.atan2(float(y[to]) - float(y[here]), float(x[to]) - float(x[here]))))
        here = int(to)
    v = here
    while v >= 0:
        poses.append((float(x[v]), float(y[v]), float(yaw[v])))
        v = int(par[v])
    return poses


def reverse_row(row):
    """the same curve from its other end: the segments in reverse order, each starting at its own
    end pose with yaw + pi (unwrapped), kappa negated, len unchanged"""
    n = len(row["x"])
    out = {f: np.zeros(n) for f in FIELDS}
    for j in range(n):
        ex, ey, eyaw = seg_end(*(row[f][j] for f in FIELDS))
        i = n - 1 - j
        k = row["kappa"][j]
        out["x"][i], out["y"][i], out["yaw"][i] = ex, ey, eyaw + math.pi
        out["kappa"][i] = 0.0 if k == 0.0 else -k
        out["len"][i] = row["len"][j]
    return out


def row_length(row):
    s = 0.0
    for v in row["len"]:
        s += float(v)
    return s


def sample_row(row, ds):
    """(x, y, yaw, kappa, s) arrays of the samples of one row every ds"""
    n = len(row["x"])
    if n == 0:
        return tuple(np.zeros(0) for _ in range(5))
    P = [0.0]
    for v in row["len"]:
        P.append(P[-1] + float(v))
    L = P[-1]
    nf = int(math.floor(L / ds))
    ss = [i * ds for i in range(nf + 1)]
    if L > ss[-1]:
        ss.append(L)
    out = []
    for s in ss:
        j = next((j for j in range(n) if s < P[j + 1]), None)
        if j is None:
            j, u = n - 1, float(row["len"][n - 1])
        else:
            u = s - P[j]
        k = float(row["kappa"][j])
        px, py, pyaw = seg_end(float(row["x"][j]), float(row["y"][j]), float(row["yaw"][j]), k, u)
        out.append((px, py, pyaw, k, s))
    a = np.array(out, dtype=np.float64).reshape(-1, 5)
    return tuple(a[:, i].copy() for i in range(5))


def pack(rows):
    """(off, seg): rows (None: empty) packed as the C ABI packs them"""
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    for i, r in enumerate(rows):
        off[i + 1] = off[i] + (0 if r is None else len(r["x"]))
    seg = {f: np.concatenate([np.zeros(0)] + [r[f] for r in rows if r is not None])
           for f in FIELDS}
    return off, seg


def unpack(off, seg):
    return [{f: np.asarray(seg[f][off[i]:off[i + 1]]) for f in FIELDS}
            for i in range(len(off) - 1)]


def words_of(row):
    """the word index of every edge from its three curvature signs"""
    sg = np.sign(row["kappa"]).astype(int).reshape(-1, 3)
    code = {dpy.L: 1, dpy.S: 0, dpy.R: -1}
    table = {tuple(code[m] for m in modes): w for w, modes in enumerate(dpy.WORD_MODES)}
    return [table[tuple(s)] for s in sg]


def curve_distance(row, px, py):
    """the distance of every point (px, py) from the row's curve (arcs and straights, exact)"""
    px = np.asarray(px, dtype=np.float64)
    py = np.asarray(py, dtype=np.float64)
    best = np.full(len(px), np.inf)
    for j in range(len(row["x"])):
        x, y, yaw, k, ln = (float(row[f][j]) for f in FIELDS)
        ex, ey, _ = seg_end(x, y, yaw, k, ln)
        d = np.minimum(np.hypot(px - x, py - y), np.hypot(px - ex, py - ey))
        if k == 0.0:
            ux, uy = math.cos(yaw), math.sin(yaw)
            t = (px - x) * ux + (py - y) * uy
            on = (t >= 0.0) & (t <= ln)
            perp = np.abs((px - x) * uy - (py - y) * ux)
            d = np.where(on, np.minimum(d, perp), d)
        else:
            r = 1.0 / abs(k)
            cx, cy = x - math.sin(yaw) / k, y + math.cos(yaw) / k
            phi0 = math.atan2(y - cy, x - cx)
            delta = np.mod((np.arctan2(py - cy, px - cx) - phi0) * (1.0 if k > 0.0 else -1.0),
                           2.0 * math.pi)
            on = delta <= abs(k) * ln
            d = np.where(on, np.minimum(d, np.abs(np.hypot(px - cx, py - cy) - r)), d)
        best = np.minimum(best, d)
    return best

"""CPU restatement of the tree revalidation (pp_rrt_revalidate / pp_batch_revalidate, DESIGN.md
§3.8), composed only from what the oracle exports: oracle.dubins and OracleScene.verify_line.  A
plain helper module (no fixtures): the tests import it.

Node i > 0 of a tree with stored poses (x, y, yaw) and parents:
  edge_ok[i] = Space::verify of the Dubins points from node i's stored pose to its parent's stored
               pose, followed by the parent's point; a None steer gives [(x_i, y_i), (x_p, y_p)]
               (line_to_origin, rrt.rs:291-321, with the stored yaw)
  keep[0]    = 1 (RRT::new inserts the root unverified); root_ok = False (polygon mode: the root
               fails verify as a point) drops every other node
  keep[i]    = edge_ok[i] and keep[parent[i]] — verify(line_to_origin(i)) by DESIGN.md §2
Kept nodes keep their order; parents are remapped; poses are untouched.
"""
import numpy as np

import oracle


def edge_ok(osc, tree):
    """edge_ok[i] for every node (edge_ok[0] = True)"""
    x, y, yaw, par = tree[:4]
    ok = np.ones(len(x), dtype=bool)
    for i in range(1, len(x)):
        p = int(par[i])
        d = oracle.dubins(x[i], y[i], yaw[i], x[p], y[p], yaw[p], osc.turn_radius, osc.step_size)
        if d is None:
            lx, ly = np.array([x[i], x[p]]), np.array([y[i], y[p]])
        else:
            lx, ly = np.append(d[0], x[p]), np.append(d[1], y[p])
        ok[i] = osc.verify_line(lx, ly)
    return ok


def root_ok(osc, tree):
    """polygon mode: Space::verify of the root as a one-point line (else True: the root is never
    verified, and a covered root fails the depth-1 edges through the appended parent point)"""
    if osc.polygons is None:
        return True
    return osc.verify_line(np.array([tree[0][0]]), np.array([tree[1][0]]))


def keep_mask(eok, par, rok=True):
    """the sequential loop: parents precede children"""
    keep = np.zeros(len(eok), dtype=bool)
    keep[0] = True
    for i in range(1, len(eok)):
        keep[i] = rok and eok[i] and keep[int(par[i])]
    return keep


def compact(tree, keep):
    """((x, y, yaw, parent) of the kept nodes in order, new_index int32[n] with -1 dropped)"""
    x, y, yaw, par = tree[:4]
    new_index = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    npar = np.asarray(par)[keep].astype(np.int32)
    npar[1:] = new_index[npar[1:]]
    assert (npar[1:] >= 0).all() and (npar[1:] < np.arange(1, len(npar))).all()
    return (np.asarray(x)[keep], np.asarray(y)[keep], np.asarray(yaw)[keep], npar), new_index


def revalidate(osc, tree):
    """dict: edge_ok, keep, tree (compacted), new_index, kept, failed (edges), orphans (edge_ok
    but a failed ancestor)"""
    eok = edge_ok(osc, tree)
    rok = root_ok(osc, tree)
    keep = keep_mask(eok, tree[3], rok)
    new_tree, new_index = compact(tree, keep)
    return {"edge_ok": eok, "keep": keep, "tree": new_tree, "new_index": new_index,
            "kept": int(keep.sum()), "failed": int((~eok).sum()),
            "orphans": int((eok & ~keep).sum())}


def depth(par):
    d = np.zeros(len(par), dtype=np.int64)
    for i in range(1, len(par)):
        d[i] = d[int(par[i])] + 1
    return d


def descendants(par):
    """descendant count of every node (itself excluded)"""
    c = np.zeros(len(par), dtype=np.int64)
    for i in range(len(par) - 1, 0, -1):
        c[int(par[i])] += c[i] + 1
    return c


def with_discs(raw, discs):
    """the disc scene `raw` plus extra (cx, cy, r) discs"""
    out = dict(raw)
    out["circles"] = [tuple(c) for c in raw["circles"]] + [tuple(float(v) for v in d) for d in discs]
    return out


def extra_discs(raw, count, seed=77, size=512.0):
    """`count` discs (cx, cy ~ U(0, size), r ~ U(2, 8)) from default_rng(seed), rejecting a disc
    when hypot(c - start) <= r + 4"""
    rng = np.random.default_rng(seed)
    sx, sy = raw["start"][:2]
    out = []
    while len(out) < count:
        cx, cy = rng.uniform(0.0, size, 2)
        r = rng.uniform(2.0, 8.0)
        if np.hypot(cx - sx, cy - sy) <= r + 4.0:
            continue
        out.append((cx, cy, r))
    return out

"""CPU restatement, in plain numpy, of what pp_star_forest_import / pp_batch_forest_import check
on a packed forest state and of the cost rebuild, plus the hand-built trees the
CPU and the GPU tests share.

A state is the dict ``RRTStarBatch.export_forest`` returns: ``off`` (m + 1), the rows ``x``,
``y``, ``yaw``, ``parent`` (-1 for a tree's row 0), ``cost``, ``edge_cost`` and per slot
``iterations``, ``seeds``, ``node_evals``, ``rewires``, ``focus_xy``, ``focus_bound``, ``skipped``
(the extend batch: no cost / edge_cost / rewires / focus, but ``goals``).

The rebuild is level-synchronous from the root, as the device does it: pass s gives every node
whose parent sits on level s the cost ``cost[parent] + edge_cost`` — one f64 addition — and level
s + 1.  Index order plays no part (a rewired node's parent may be a later node), and a pass that
reaches nobody ends the loop: the nodes still on level 0 then hang on a cycle or an island."""
import numpy as np

OK, INVALID, CAPACITY = "ok", "invalid", "capacity"
COORD_MAX = 2.0 ** 61


def rebuild_costs(parent, edge_cost):
    """(cost, level) of one tree: level 1 the root, 0 a node no chain from the root reaches"""
    parent = np.asarray(parent, dtype=np.int64)
    edge_cost = np.asarray(edge_cost, dtype=np.float64)
    n = len(parent)
    lvl = np.zeros(n, dtype=np.int64)
    cost = np.zeros(n)
    lvl[0] = 1
    for s in range(1, n + 1):
        todo = np.nonzero(lvl == 0)[0]
        hit = todo[lvl[parent[todo]] == s]
        if len(hit) == 0:
            break
        cost[hit] = cost[parent[hit]] + edge_cost[hit]
        lvl[hit] = s + 1
    return cost, lvl


def check_tree(parent, edge_cost=None, cost=None, ordered=False):
    """(verdict, rebuilt cost or None) of one tree's rows"""
    parent = np.asarray(parent, dtype=np.int64)
    n = len(parent)
    if parent[0] != -1:
        return INVALID, None  # a root with a parent
    p = parent[1:]
    idx = np.arange(1, n)
    if ((p < 0) | (p >= n) | (p == idx)).any():
        return INVALID, None  # a parent out of range, a self-parent
    if ordered:
        return (INVALID if (p >= idx).any() else OK), None
    rebuilt, lvl = rebuild_costs(parent, edge_cost)
    if (lvl == 0).any():
        return INVALID, None  # a cycle or an island
    if cost is not None and not np.array_equal(np.asarray(cost, dtype=np.float64).view(np.uint64),
                                               rebuilt.view(np.uint64)):
        return INVALID, None  # a damaged checkpoint
    return OK, rebuilt


def check_state(state, max_iter, queries=None, star=True):
    """(verdict, the first offending slot or None, the rebuilt costs or None) of a state, in the
    import's order: the host's checks slot by slot, then the device's"""
    off = np.asarray(state["off"], dtype=np.int64)
    m = len(off) - 1
    slot = (lambda i: i) if queries is None else (lambda i: int(queries[i]))
    for i in range(m):
        g0, g1 = int(off[i]), int(off[i + 1])
        n, it = g1 - g0, int(state["iterations"][i])
        if n < 1 or it < 0 or it > max_iter:
            return INVALID, slot(i), None
        if n > it + 1:
            return CAPACITY, slot(i), None
        for key in ("x", "y"):
            if not (np.abs(np.asarray(state[key][g0:g1])) <= COORD_MAX).all():
                return INVALID, slot(i), None
        if not np.isfinite(state["yaw"][g0:g1]).all() or state["node_evals"][i] < 0:
            return INVALID, slot(i), None
        if star:
            e = np.asarray(state["edge_cost"][g0:g1])
            if not (np.isfinite(e) & (e >= 0.0)).all():
                return INVALID, slot(i), None
            if state["rewires"][i] < 0 or state["skipped"][i] < 0:
                return INVALID, slot(i), None
            if not state["focus_bound"][i] > 0.0:
                return INVALID, slot(i), None
            if not (np.abs(np.asarray(state["focus_xy"]).reshape(m, 2)[i]) <= COORD_MAX).all():
                return INVALID, slot(i), None
        elif not np.isfinite(np.asarray(state["goals"]).reshape(m, 3)[i]).all():
            return INVALID, slot(i), None
    out = np.zeros(int(off[m]))
    for i in range(m):
        g0, g1 = int(off[i]), int(off[i + 1])
        given = state.get("cost") if star else None
        v, rebuilt = check_tree(state["parent"][g0:g1], state["edge_cost"][g0:g1] if star else None,
                                None if given is None else given[g0:g1], ordered=not star)
        if v != OK:
            return v, slot(i), None
        if star:
            out[g0:g1] = rebuilt
    return OK, None, out if star else None


# ---- trees: one dict per tree, packed into a state by pack()

def star_tree(x, y, yaw, parent, edge_cost, cost=None, iterations=None, seed=1, node_evals=0,
              rewires=0, focus_xy=(0.0, 0.0), focus_bound=np.inf, skipped=0):
    n = len(x)
    return {"x": np.asarray(x, dtype=np.float64), "y": np.asarray(y, dtype=np.float64),
            "yaw": np.asarray(yaw, dtype=np.float64), "parent": np.asarray(parent, dtype=np.int32),
            "edge_cost": np.asarray(edge_cost, dtype=np.float64),
            "cost": None if cost is None else np.asarray(cost, dtype=np.float64),
            "iterations": n - 1 if iterations is None else iterations, "seed": seed,
            "node_evals": node_evals, "rewires": rewires, "focus_xy": tuple(focus_xy),
            "focus_bound": focus_bound, "skipped": skipped}


def pack(trees):
    """the state dict of a list of star_tree dicts; ``cost`` is None unless every tree has one"""
    cat = lambda key, dt: np.concatenate([np.asarray(t[key], dtype=dt) for t in trees])  # noqa: E731
    per = lambda key, dt: np.array([t[key] for t in trees], dtype=dt)  # noqa: E731
    st = {"off": np.concatenate(([0], np.cumsum([len(t["x"]) for t in trees]))).astype(np.int64),
          "x": cat("x", np.float64), "y": cat("y", np.float64), "yaw": cat("yaw", np.float64),
          "parent": cat("parent", np.int32), "edge_cost": cat("edge_cost", np.float64),
          "cost": None if any(t["cost"] is None for t in trees) else cat("cost", np.float64),
          "iterations": per("iterations", np.int64), "seeds": per("seed", np.uint64),
          "node_evals": per("node_evals", np.int64), "rewires": per("rewires", np.int64),
          "focus_xy": per("focus_xy", np.float64).reshape(len(trees), 2),
          "focus_bound": per("focus_bound", np.float64), "skipped": per("skipped", np.int64)}
    return st


def chain_tree(n, reverse=False, x0=-4.0, y0=-4.0):
    """a hand-built tree of n nodes on a short line inside bench6_open's free corner.  Forward:
    node i hangs under i - 1.  Reverse (n >= 3): the parent of node i is i + 1 and the last node
    hangs under the root — depth n - 1 with every parent after its child, the worst case for a
    sweep that assumes index order.  Edge costs are distinct inexact fractions, so a rebuild in
    the wrong order would round differently."""
    i = np.arange(n)
    par = i - 1
    if reverse and n >= 3:
        par = i + 1
        par[n - 1] = 0
    par[0] = -1
    e = np.where(i == 0, 0.0, 0.1 + i / 7.0)
    return star_tree(x0 + 0.01 * i, y0 + 0.003 * i, 0.001 * i, par, e)


def bad_variants(tree):
    """(name, tree, expected verdict) for every defect the import must refuse, each built from a
    valid tree of at least 6 nodes that carries its costs"""
    n = len(tree["x"])
    assert n >= 6 and tree["cost"] is not None

    def variant(**kw):
        t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tree.items()}
        for k, (j, v) in kw.items():
            t[k][j] = v
        return t

    j = n // 2
    out = [("self-parent", variant(parent=(j, j)), INVALID),
           ("parent out of range", variant(parent=(j, n)), INVALID),
           ("negative parent", variant(parent=(j, -1)), INVALID),
           ("root with a parent", variant(parent=(0, 1)), INVALID)]
    cyc = variant()
    a, b, c = n - 3, n - 2, n - 1  # a 3-cycle that avoids the root
    cyc["parent"][[a, b, c]] = [b, c, a]
    out.append(("3-cycle", cyc, INVALID))
    isl = variant()  # an island: c hangs on a, whose chain ends in b and never in row 0
    isl["parent"][[a, b, c]] = [b, a, a]
    out.append(("island", isl, INVALID))
    out.append(("edge cost NaN", variant(edge_cost=(j, np.nan)), INVALID))
    out.append(("edge cost -1", variant(edge_cost=(j, -1.0)), INVALID))
    big = variant()
    big["iterations"] = n - 2  # n > iterations + 1
    out.append(("n > iterations + 1", big, CAPACITY))
    out.append(("cost off by one ulp",
                variant(cost=(j, np.nextafter(tree["cost"][j], np.inf))), INVALID))
    return out

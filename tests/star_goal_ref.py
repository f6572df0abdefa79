"""CPU restatement of the RRT* goal connection (pp_star_plan / pp_star_goal_costs / pp_star_path,
DESIGN.md §3.7 "Goal connection"), composed only from what the oracle exports: oracle.dubins,
OracleScene.verify_line and oracle.line_length.  A plain helper module (no fixtures): the tests
and tests/golden/gen_star_goal.py import it.

Goal edge of node m: the goal is the child and keeps its yaw, node m is the parent —
dubins(goal pose -> node pose, R, step); feasible when the word is Some and verify accepts the
edge's points followed by the node's point; total[m] = cost[m] + Dubins cost, else +inf.  The best
node is the first strict minimum of total in node-index order (-1, +inf when none is feasible).
"""
import numpy as np

import oracle

SCENES = ("bench6_open", "field512", "config5_field", "field512_grid", "bench6_polygons_open")


def scene(name):
    from pathplanning_amd import scenes

    assert name in SCENES, name
    return getattr(scenes, name)()


def grow(raw, start, seed, n_iter, k, eta, osc=None):
    """the oracle's RRT* tree after n_iter iterations: (x, y, yaw, parent, cost)"""
    osc = osc or oracle.OracleScene.from_raw(raw)
    tr = oracle.OracleStarTree(tuple(start), n_iter + 1)
    oracle.star_extend(osc, tr, int(seed), 0, n_iter, k, eta)
    return tr.star_arrays()[:5]


def goal_costs(osc, tree, goal):
    """total[m] = cost[m] + e[m], +inf where the goal edge of node m is infeasible"""
    x, y, yaw, _, cost = tree[:5]
    gx, gy, gyaw = (float(v) for v in goal)
    total = np.full(len(x), np.inf)
    for m in range(len(x)):
        d = oracle.dubins(gx, gy, gyaw, x[m], y[m], yaw[m], osc.turn_radius, osc.step_size)
        if d is None:
            continue
        px, py, _, _, e = d
        if osc.verify_line(np.append(px, x[m]), np.append(py, y[m])):
            total[m] = cost[m] + e
    return total


def first_min(total):
    """(best node, cost): the first strict minimum in index order; (-1, inf) when none is finite"""
    total = np.asarray(total)
    if len(total) == 0 or not np.isfinite(total).any():
        return -1, np.inf
    b = int(np.argmin(total))  # (the first occurrence of the minimum)
    return b, float(total[b])


def runner_up_gap(total):
    """relative gap between the best and the second-best total (inf when there is no second)"""
    f = np.sort(np.asarray(total)[np.isfinite(total)])
    if len(f) < 2:
        return np.inf
    return float((f[1] - f[0]) / f[0]) if f[0] > 0.0 else float(f[1] - f[0])


def plan(osc, tree, goal):
    """(best node, cost, total)"""
    total = goal_costs(osc, tree, goal)
    return first_min(total) + (total,)


def path(osc, tree, goal, node):
    """E(goal -> node) ++ E(node -> parent) ++ ... ++ E(. -> 0) ++ [root], reversed (root first),
    E = the kept Dubins points of an edge from the child's stored pose to the parent's stored
    pose.  Returns (xy[n, 2], euclidean length)."""
    x, y, yaw, par = tree[:4]
    R, step = osc.turn_radius, osc.step_size
    gx, gy, gyaw = (float(v) for v in goal)
    xs, ys = [], []

    def edge(cx, cy, cyaw, p):
        d = oracle.dubins(cx, cy, cyaw, x[p], y[p], yaw[p], R, step)
        if d is None:
            raise RuntimeError("an edge of the chain has no Dubins word")
        xs.append(d[0])
        ys.append(d[1])

    edge(gx, gy, gyaw, node)
    v = int(node)
    while par[v] >= 0:
        edge(x[v], y[v], yaw[v], int(par[v]))
        v = int(par[v])
    assert v == 0
    xs.append(np.array([x[0]]))
    ys.append(np.array([y[0]]))
    lx, ly = np.concatenate(xs)[::-1], np.concatenate(ys)[::-1]
    return np.stack([lx, ly], axis=1), oracle.line_length(lx, ly)


# ---- the golden cases (tests/golden/star_goal.json): one record per (tree, goal)
def golden_specs():
    from pathplanning_amd import scenes

    specs = []
    raw = scenes.bench6_open()
    for seed, k, eta in ((5, 0, 0.0), (11, 4, 2.0)):
        for n_iter in (100, 200, 400):
            specs.append(dict(scene="bench6_open", start=list(raw["start"]), seed=seed,
                              n_iter=n_iter, k=k, eta=eta, goal=list(raw["goal"])))
    for name, eta, n_iter in (("field512", 12.0, 1500), ("config5_field", scenes.CONFIG5_ETA, 300)):
        raw = getattr(scenes, name)()
        starts, goals, seeds = scenes.config3_queries(raw, 0, 2)
        for q in range(2):
            specs.append(dict(scene=name, start=[float(v) for v in starts[q]], seed=int(seeds[q]),
                              n_iter=n_iter, k=0, eta=eta, goal=[float(v) for v in goals[q]]))
    return specs


def golden_record(spec):
    raw = scene(spec["scene"])
    osc = oracle.OracleScene.from_raw(raw)
    tree = grow(raw, spec["start"], spec["seed"], spec["n_iter"], spec["k"], spec["eta"], osc)
    b, c, total = plan(osc, tree, spec["goal"])
    rec = dict(spec)
    rec["n_nodes"] = len(tree[0])
    rec["best_node"] = b
    rec["cost"] = c if b >= 0 else None
    gap = runner_up_gap(total)
    rec["gap"] = gap if np.isfinite(gap) else None
    rec["feasible"] = [int(i) for i in np.flatnonzero(np.isfinite(total))]
    if b >= 0:
        xy, length = path(osc, tree, spec["goal"], b)
        rec["path_points"] = len(xy)
        rec["path_length"] = length
    else:
        rec["path_points"] = 0
        rec["path_length"] = None
    return rec

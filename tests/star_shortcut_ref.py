"""CPU restatement of the shortcuts along the chain (pp_star_shortcut / pp_star_shortcut_edges,
DESIGN.md §3.7 "Shortcuts along the chain"), composed only from oracle.dubins,
OracleScene.verify_line and star_goal_ref.  A plain helper module (no fixtures): the tests and
tests/golden/gen_star_shortcut.py import it.

Positions of (tree, goal, node): c_0 = the goal with its own yaw, c_1 = the node, c_2 = its parent,
..., c_D = the root, each with its stored pose.  Edge (i -> j), i < j <= i + span: dubins(c_i's pose
-> c_j's pose, R, step), feasible when the word is Some and verify accepts the edge's points
followed by c_j's point; w(i, j) its Dubins cost, else +inf.  best[D] = 0; best[i] = the first
strict minimum in increasing j of best[j] + w(i, j); next[i] that j; the path follows next from 0.
"""
import itertools

import numpy as np

import oracle
import star_goal_ref as goal_ref

SCENES = goal_ref.SCENES
scene = goal_ref.scene
grow = goal_ref.grow


def chain_nodes(tree, node):
    """[node, parent[node], ..., 0]: the tree nodes of positions 1 .. D"""
    par = tree[3]
    out = []
    v = int(node)
    while v >= 0:
        assert len(out) <= len(par), "parent cycle"
        out.append(v)
        v = int(par[v])
    assert out[-1] == 0
    return out


def poses(tree, goal, node):
    """(cnode[D], pose[D + 1]): pose[0] the goal, pose[i] the stored pose of cnode[i - 1]"""
    x, y, yaw = tree[:3]
    cnode = chain_nodes(tree, node)
    ps = [tuple(float(v) for v in goal)] + [(float(x[m]), float(y[m]), float(yaw[m])) for m in cnode]
    return cnode, ps


def edge_cost(osc, a, b):
    """w of the feasible edge from pose a (own yaw) to pose b, +inf when infeasible"""
    d = oracle.dubins(a[0], a[1], a[2], b[0], b[1], b[2], osc.turn_radius, osc.step_size)
    if d is None:
        return np.inf
    px, py, _, _, e = d
    return float(e) if osc.verify_line(np.append(px, b[0]), np.append(py, b[1])) else np.inf


def band(osc, tree, goal, node, span):
    """(cnode int[D], w float64[D, span]): w[i, j - i - 1] = w(i, j), +inf where infeasible or
    j > D; and the number of pairs tested"""
    cnode, ps = poses(tree, goal, node)
    D = len(cnode)
    w = np.full((D, span), np.inf)
    pairs = 0
    for i in range(D):
        for j in range(i + 1, min(i + span, D) + 1):
            w[i, j - i - 1] = edge_cost(osc, ps[i], ps[j])
            pairs += 1
    return np.array(cnode, dtype=np.int32), w, pairs


def dp(w):
    """The DP over a band w[D, span]: (cost, positions, gap) — positions = [0, ..., D] along next
    ([] when nothing reaches the root, cost inf); gap = the smallest relative distance between the
    minimum and the runner-up over the rows with a finite best (inf when no row has a runner-up).
    Each sum best[j] + w(i, j) is one f64 addition."""
    D, span = w.shape
    best = np.full(D + 1, np.inf)
    nxt = np.full(D + 1, -1, dtype=np.int64)
    best[D] = 0.0
    gap = np.inf
    for i in range(D - 1, -1, -1):
        cands = []
        for j in range(i + 1, min(i + span, D) + 1):
            v = np.float64(best[j]) + np.float64(w[i, j - i - 1])
            cands.append(v)
            if v < best[i]:  # the first strict minimum in increasing j
                best[i] = v
                nxt[i] = j
        fin = sorted(v for v in cands if np.isfinite(v))
        if len(fin) >= 2:
            gap = min(gap, (fin[1] - fin[0]) / fin[0] if fin[0] > 0.0 else fin[1] - fin[0])
    if not np.isfinite(best[0]):
        return np.inf, [], gap
    pos = [0]
    while pos[-1] != D:
        pos.append(int(nxt[pos[-1]]))
    return float(best[0]), pos, float(gap)


def shortcut(osc, tree, goal, node, span):
    """dict(D, cnode, w, pairs, cost, positions, chain, gap): chain = the tree nodes of the
    shortened path after the goal (the root last), [] when no route exists within the span"""
    cnode, w, pairs = band(osc, tree, goal, node, span)
    cost, pos, gap = dp(w)
    return dict(D=len(cnode), cnode=cnode, w=w, pairs=pairs, cost=cost, positions=pos,
                chain=[int(cnode[p - 1]) for p in pos[1:]], gap=gap)


def brute(w):
    """the cheapest route 0 -> D over all subsets of the positions between (hops <= span), every
    route's cost accumulated from the root's end like the DP: the minimum cost (inf: none)"""
    D, span = w.shape
    bestc = np.inf
    for r in range(D):
        for mid in itertools.combinations(range(1, D), r):
            pos = (0,) + mid + (D,)
            if any(b - a > span for a, b in zip(pos, pos[1:])):
                continue
            c = np.float64(0.0)
            for a, b in zip(reversed(pos[:-1]), reversed(pos[1:])):
                c = c + np.float64(w[a, b - a - 1])
            if c < bestc:
                bestc = float(c)
    return bestc


def deepest_reaching_node(osc, tree, goal):
    """the node with the deepest chain among those with a feasible goal edge (the lowest index on
    a tie), -1 when none"""
    total = goal_ref.goal_costs(osc, tree, goal)
    par = tree[3]
    depth = np.zeros(len(par), dtype=np.int64)
    for m in range(len(par)):  # (a rewired node's parent may be a later node)
        d, v = 0, m
        while par[v] >= 0:
            v = int(par[v])
            d += 1
        depth[m] = d
    fin = np.flatnonzero(np.isfinite(total))
    if len(fin) == 0:
        return -1
    return int(fin[np.argmax(depth[fin])])


# ---- the recorded cases of the issue (bench6_open, the scene's start and goal)
RECORDED = (
    dict(seed=7, n_iter=3000, k=6, eta=0.25, node=1292, n_nodes=1556, D=25,
         tree_cost=71.7636392913853,
         spans={8: dict(cost=41.756682774076026, edges=6, pairs=172, feasible=165,
                        positions=[0, 1, 2, 10, 13, 21, 25]),
                63: dict(cost=39.786111241426696, edges=2, pairs=325, feasible=301)}),
    dict(seed=9, n_iter=6000, k=6, eta=0.1, node=1785, D=49, tree_cost=134.16,
         spans={8: dict(cost=41.7613), 63: dict(cost=39.1985)}),
)


# ---- the golden cases (tests/golden/star_shortcut.json): one record per (tree, goal, node, span)
def golden_specs():
    from pathplanning_amd import scenes

    specs = []
    raw = scenes.bench6_open()
    for span in (1, 8, 63):
        specs.append(dict(scene="bench6_open", start=list(raw["start"]), seed=7, n_iter=3000, k=6,
                          eta=0.25, goal=list(raw["goal"]), node=1292, span=span))
    specs.append(dict(scene="bench6_open", start=list(raw["start"]), seed=11, n_iter=400, k=4,
                      eta=2.0, goal=list(raw["goal"]), node=None, span=4))
    for name, eta, n_iter in (("field512", 12.0, 1500), ("config5_field", scenes.CONFIG5_ETA, 300)):
        r = getattr(scenes, name)()
        starts, goals, seeds = scenes.config3_queries(r, 0, 2)
        for q in range(2):
            specs.append(dict(scene=name, start=[float(v) for v in starts[q]], seed=int(seeds[q]),
                              n_iter=n_iter, k=0, eta=eta, goal=None, node=None, span=8))
    for name, eta in (("field512_grid", 10.0), ("bench6_polygons_open", 0.5)):
        r = getattr(scenes, name)()
        specs.append(dict(scene=name, start=list(r["start"]), seed=3, n_iter=300, k=0, eta=eta,
                          goal=None, node=None, span=6))
    return specs


def near_goal(tree):
    """a goal a short Dubins edge away from the deepest node, facing back (reachable in an open
    scene whatever the scene's own goal is)"""
    x, y, yaw, par = tree[:4]
    depth = [len(chain_nodes(tree, m)) for m in range(len(x))]
    m = int(np.argmax(depth))
    return [float(x[m] + 3.0 * np.cos(yaw[m])), float(y[m] + 3.0 * np.sin(yaw[m])),
            float(yaw[m] + np.pi)]


def golden_record(spec):
    raw = scene(spec["scene"])
    osc = oracle.OracleScene.from_raw(raw)
    tree = grow(raw, spec["start"], spec["seed"], spec["n_iter"], spec["k"], spec["eta"], osc)
    rec = dict(spec)
    if rec["goal"] is None:
        rec["goal"] = near_goal(tree)
    if rec["node"] is None:
        rec["node"] = deepest_reaching_node(osc, tree, rec["goal"])
    rec["n_nodes"] = len(tree[0])
    if rec["node"] < 0:
        rec.update(D=0, chain=[], cost=None, gap=None, feasible=[], pairs=0)
        return rec
    s = shortcut(osc, tree, rec["goal"], rec["node"], rec["span"])
    rec["D"] = s["D"]
    rec["chain"] = s["chain"]
    rec["cost"] = s["cost"] if s["chain"] else None
    rec["gap"] = s["gap"] if np.isfinite(s["gap"]) else None
    rec["pairs"] = s["pairs"]
    rec["feasible"] = [[int(i), int(i + 1 + l)] for i, l in zip(*np.nonzero(np.isfinite(s["w"])))]
    return rec

"""CPU restatement of relaxing the trees of an RRT* batch (pp_star_relax, DESIGN.md §3.8 "Relaxing
the trees"), built on what the oracle exports: oracle.dubins, OracleScene.verify_line and
oracle.star_k.  A plain helper module (no fixtures): the tests import it.

For a batch of trees with stored x, y, yaw, parent, cost and edge costs elen, the scene, the
batch's k and up to R rounds.  An inactive tree, a tree of one node and a root-blocked tree stay bit
for bit.  A round reads parent, cost and elen as they stood when it began:
  candidates  of node i > 0: the star_k(k, n - 1) nearest nodes j != i of its tree by exact f64
              (dx * dx + dy * dy, index), the root like any other; the candidate equal to parent[i]
              keeps its place in the order and is never evaluated
  edge        i -> p keeps i's stored pose, yaw included, and runs to p's stored pose; feasible by
              star_edge (the word is Some, Space::verify accepts the points followed by p's point);
              total = cost[p] + e, one rounded f64 add
  choice      the first strict minimum of total in candidate order among the feasible candidates,
              accepted only when total < cost[i]; the node stages parent = p, elen = e and reads no
              other node's staged values
  apply       after every node has chosen: the staged rows, then cost rebuilt from the root level
              by level, cost[i] = cost[parent[i]] + elen[i], parents final before children
  early stop  a round that re-parents nothing in any active tree ends the call; rounds_run counts
              it
The restatement does not cull: `cull=True` adds the device's exact skip of a candidate with
cost[p] >= cost[i] so that a test can show it changes nothing.  Every node reads the start-of-round
state alone, so the order in which nodes are taken cannot matter (`order` permutes it).
"""
import numpy as np

import oracle


class Edges:
    """the feasible-edge evaluations i -> p of one tree's fixed poses in one scene, memoised: the
    poses never change, so a round asks again what an earlier one asked"""

    def __init__(self, osc, x, y, yaw):
        self.osc, self.x, self.y, self.yaw = osc, x, y, yaw
        self.memo = {}
        self.none = 0

    def __call__(self, i, p):
        key = (i, p)
        if key not in self.memo:
            x, y, yaw, osc = self.x, self.y, self.yaw, self.osc
            d = oracle.dubins(x[i], y[i], yaw[i], x[p], y[p], yaw[p], osc.turn_radius,
                              osc.step_size)
            if d is None:
                self.none += 1
                self.memo[key] = None
            elif not osc.verify_line(np.append(d[0], x[p]), np.append(d[1], y[p])):
                self.memo[key] = None
            else:
                self.memo[key] = float(d[4])
        return self.memo[key]


def candidates(x, y, i, kk):
    """the kk nearest nodes j != i by (d2, index)"""
    dx, dy = x[i] - x, y[i] - y
    d2 = dx * dx + dy * dy
    idx = np.arange(len(x))
    o = np.lexsort((idx, d2))
    o = o[o != i]
    return o[:kk]


def rebuild_costs(par, elen):
    """cost from the root level by level, one add per edge; raises on a node the root does not
    reach"""
    n = len(par)
    cost = np.zeros(n)
    done = np.zeros(n, dtype=bool)
    done[0] = True
    front = np.array([0])
    while len(front):
        mark = np.zeros(n, dtype=bool)
        mark[front] = True
        front = np.array([i for i in range(1, n) if not done[i] and mark[par[i]]], dtype=np.int64)
        for i in front:
            cost[i] = cost[par[i]] + elen[i]
            done[i] = True
    assert done.all(), "a chain that does not end in the root"
    return cost


class _Tree:
    def __init__(self, osc, tree, elen):
        self.x, self.y, self.yaw = (np.asarray(a, dtype=np.float64) for a in tree[:3])
        self.par = np.array(tree[3], dtype=np.int64)
        self.cost = np.array(tree[4], dtype=np.float64)
        self.elen = np.array(elen, dtype=np.float64)
        self.cost0 = self.cost.copy()
        self.edges = Edges(osc, self.x, self.y, self.yaw)
        self.n = len(self.x)
        self.rewired = 0
        self.moved = np.zeros(self.n, dtype=bool)  # re-parented in some round
        self.per_round = []
        self.margin = np.inf  # least |total - cost[i]| / cost[i] over the evaluated feasible
        self.gap = np.inf     # least (runner-up - winner) / winner over the winners
        self.evaluated = 0
        self.culled = 0

    def round(self, kk, order, cull):
        """one round: the staged (node, parent, elen) rows, applied; returns their count"""
        nodes = np.arange(1, self.n)
        if order is not None:
            nodes = order(nodes)
        staged = []
        for i in nodes:
            i = int(i)
            ci = self.cost[i]
            best, be, bt, second = -1, np.inf, np.inf, np.inf
            for p in candidates(self.x, self.y, i, kk):
                p = int(p)
                if p == self.par[i]:
                    continue
                if cull and self.cost[p] >= ci:
                    self.culled += 1
                    continue
                e = self.edges(i, p)
                if e is None:
                    continue
                self.evaluated += 1
                total = self.cost[p] + e
                self.margin = min(self.margin, abs(total - ci) / ci)
                if total < bt:
                    second = bt
                    best, be, bt = p, e, total
                elif total < second:
                    second = total
            if best >= 0 and bt < ci:
                staged.append((i, best, be))
                # the runner-up that matters: the next total, or the node's own cost
                self.gap = min(self.gap, (min(second, ci) - bt) / bt if bt > 0 else np.inf)
        for i, p, e in staged:  # (the start-of-round state has been read by every node)
            self.par[i], self.elen[i] = p, e
            self.moved[i] = True
        if staged:
            self.cost = rebuild_costs(self.par, self.elen)
        self.rewired += len(staged)
        self.per_round.append(len(staged))
        return len(staged)


def relax(osc, trees, elens, k, rounds, active=None, blocked=None, order=None, cull=False):
    """The call over a batch: trees[q] = (x, y, yaw, parent, cost), elens[q] its edge costs.
    dict: rounds_run, n_changed, n_rewired [q], per_round [q][r], parent / cost / elen [q] after
    the call, moved [q] (bool per node: re-parented in some round, wherever it hangs in the end),
    margin / gap [q] (see _Tree), evaluated / culled [q], none_edges.
    order: None, or a function (nodes 1 .. n - 1) -> the nodes in the order to take them"""
    assert 1 <= rounds <= 16
    Q = len(trees)
    ts = [_Tree(osc, t, e) for t, e in zip(trees, elens)]
    live = [q for q in range(Q)
            if (active is None or active[q]) and ts[q].n > 1 and not (blocked is not None and blocked[q])]
    run = 0
    for _ in range(rounds):
        run += 1
        got = 0
        for q in live:
            t = ts[q]
            got += t.round(oracle.star_k(k, t.n - 1), order, cull)
        if got == 0:
            break
    return {"rounds_run": run,
            "n_changed": int(sum((t.cost.view(np.uint64) != t.cost0.view(np.uint64)).sum() for t in ts)),
            "n_rewired": np.array([t.rewired for t in ts], dtype=np.int32),
            "per_round": [t.per_round for t in ts],
            "parent": [t.par.astype(np.int32) for t in ts], "cost": [t.cost for t in ts],
            "elen": [t.elen for t in ts], "moved": [t.moved for t in ts], "margin": [min(t.margin, t.gap) for t in ts],
            "cost_margin": [t.margin for t in ts], "gap": [t.gap for t in ts],
            "evaluated": [t.evaluated for t in ts], "culled": [t.culled for t in ts],
            "none_edges": sum(t.edges.none for t in ts)}


def relax_one(osc, tree, elen, k, rounds, **kw):
    """relax of a batch of one tree, unwrapped"""
    r = relax(osc, [tree], [elen], k, rounds, **kw)
    return {key: (v[0] if isinstance(v, (list, np.ndarray)) else v) for key, v in r.items()}


def chains_end_in_root(par):
    """every node's chain reaches node 0 within n steps"""
    n = len(par)
    for i in range(1, n):
        v, steps = i, 0
        while v != 0:
            v = int(par[v])
            steps += 1
            if v < 0 or steps > n:
                return False
    return int(par[0]) == -1


def touched(par0, par1):
    """bool[n]: the node or one of its ancestors (in the new tree) was re-parented"""
    n = len(par0)
    chg = np.asarray(par0) != np.asarray(par1)
    out = np.zeros(n, dtype=bool)
    for i in range(1, n):
        v = i
        while v != 0:
            if chg[v]:
                out[i] = True
                break
            v = int(par1[v])
    return out

"""CPU restatement of moving an RRT* tree's root to one of its nodes (pp_star_advance, DESIGN.md
§3.8 "Advancing the root"), built on star_repair_ref's choice of a parent, on
forest_state_ref.rebuild_costs' order of additions and on what the oracle exports.  A plain helper
module (no fixtures): the tests import it.

For one tree with stored x, y, yaw, parent, cost and edge costs elen, a node and hops:
  r         = node (hops None), or the node min(hops, depth(node)) edges from the root on the
              chain root -> ... -> node; node -1 or r = 0: the tree stays bit for bit
  A         = the proper ancestors of r (parent[r], ..., 0): their edges point the wrong way
  K0        = the nodes whose chain to the old root passes through r; r becomes the root (parent
              -1, elen 0, cost 0), the others keep pose, parent and elen, and cost'[i] =
              cost'[parent[i]] + elen[i], one f64 add per edge, parents first
  rounds    star_repair_ref's rounds with K = K0, the costs cost' and A as round 1's tops (the
              old root among them); later rounds: the dropped nodes, never a top, whose parent is
              a failed top.  The scene is consulted for the new edges alone: stored edges are not
              re-verified
  compact   r to index 0, the other kept nodes behind it in old index order
"""
import numpy as np

import oracle
from star_repair_ref import ATTACHED, FAILED, _choose


def chain(par, node):
    """[node, parent[node], ..., 0]"""
    out, v = [int(node)], int(node)
    while v != 0:
        v = int(par[v])
        out.append(v)
        assert len(out) <= len(par), "a cycle in the parent array"
    return out


def pick_root(par, node, hops=None):
    """the new root's old index (0: the tree stays)"""
    if node < 0:
        return 0
    ch = chain(par, node)  # depth = len(ch) - 1
    if hops is None:
        return int(node)
    return ch[len(ch) - 1 - min(int(hops), len(ch) - 1)]


def descendants_brute(par, r):
    """K0 by the definition, node by node: r lies on the chain i -> ... -> 0"""
    return np.array([r in chain(par, i) for i in range(len(par))], dtype=bool)


def compact(x, y, yaw, par, cost, elen, keep, r):
    """((x, y, yaw, parent, cost), elen, new_index): r first, the rest in old order"""
    order = np.concatenate([[r], [i for i in np.flatnonzero(keep) if i != r]]).astype(np.int64)
    new_index = np.full(len(x), -1, dtype=np.int32)
    new_index[order] = np.arange(len(order), dtype=np.int32)
    npar = np.asarray(par)[order].astype(np.int32)
    assert npar[0] == -1
    npar[1:] = new_index[npar[1:]]
    assert (npar[1:] >= 0).all()
    return (x[order], y[order], yaw[order], npar, cost[order]), elen[order], new_index


def advance(osc, tree, elen, k, node, hops=None, rounds=0, order=None):
    """dict: r, anc (A, nearest first), keep0, keep, tree (compacted, with cost), elen (of the
    compacted tree), new_index, rounds (one dict per round that had tops: tops, reattached,
    recovered), reattached, recovered, failed_tops, gap (old index of a re-attached top -> its
    runner-up gap), kept, below (kept nodes with a lower old index than r), identity.
    order: None, or a function (round, tops array) -> the tops in the order to take them"""
    x, y, yaw = (np.array(a, dtype=np.float64) for a in tree[:3])
    par = np.array(tree[3], dtype=np.int64)
    cost = np.array(tree[4], dtype=np.float64)
    elen = np.array(elen, dtype=np.float64)
    n = len(x)
    r = pick_root(par, node, hops)
    if r == 0:
        return {"r": 0, "anc": [], "keep0": np.ones(n, dtype=bool), "keep": np.ones(n, dtype=bool),
                "tree": (x, y, yaw, par.astype(np.int32), cost), "elen": elen,
                "new_index": np.arange(n, dtype=np.int32), "rounds": [], "reattached": 0,
                "recovered": 0, "failed_tops": 0, "gap": {}, "kept": n, "below": 0,
                "identity": True}
    anc = chain(par, r)[1:]
    # K0 level by level from r, and its costs in that order
    keep0 = np.zeros(n, dtype=bool)
    keep0[r] = True
    par[r], elen[r], cost[r] = -1, 0.0, 0.0
    front = np.array([r])
    while len(front):
        mark = np.zeros(n, dtype=bool)
        mark[front] = True
        front = np.array([i for i in range(n) if not keep0[i] and par[i] >= 0 and mark[par[i]]],
                         dtype=np.int64)
        for i in front:
            cost[i] = cost[par[i]] + elen[i]
            keep0[i] = True
    keep = keep0.copy()
    state = np.zeros(n, dtype=np.int8)  # 0 never a top, ATTACHED, FAILED
    log, gap = [], {}
    for rnd in range(1, rounds + 1):
        if rnd == 1:
            tops = np.array(sorted(anc), dtype=np.int64)
        else:
            tops = np.array([i for i in range(n) if not keep[i] and state[i] == 0 and par[i] >= 0
                             and state[par[i]] == FAILED], dtype=np.int64)
        if len(tops) == 0:
            break
        kidx = np.flatnonzero(keep)
        kk = oracle.star_k(k, len(kidx))
        staged = []
        for t in (tops if order is None else order(rnd, tops)):
            t = int(t)
            dx, dy = x[t] - x[kidx], y[t] - y[kidx]
            d2 = dx * dx + dy * dy
            cand = kidx[np.lexsort((kidx, d2))[:kk]]
            staged.append((t,) + _choose(osc, x, y, yaw, cost, t, cand))
        got, front = 0, []
        for t, p, e, total, g in staged:  # (the start-of-round state has been read by every top)
            if p < 0:
                state[t] = FAILED
                continue
            state[t] = ATTACHED
            par[t], elen[t], cost[t] = p, e, total
            keep[t] = True
            gap[t] = g
            front.append(t)
            got += 1
        rec = got
        while front:
            mark = np.zeros(n, dtype=bool)
            mark[front] = True
            front = [i for i in range(n)
                     if not keep[i] and state[i] == 0 and par[i] >= 0 and mark[par[i]]]
            for i in front:
                cost[i] = cost[par[i]] + elen[i]
                keep[i] = True
            rec += len(front)
        log.append({"tops": int(len(tops)), "reattached": got, "recovered": rec})
    new_tree, new_elen, new_index = compact(x, y, yaw, par, cost, elen, keep, r)
    return {"r": r, "anc": anc, "keep0": keep0, "keep": keep, "tree": new_tree, "elen": new_elen,
            "new_index": new_index, "rounds": log, "gap": gap, "kept": int(keep.sum()),
            "below": int(keep[:r].sum()), "identity": False,
            "reattached": sum(d["reattached"] for d in log),
            "recovered": sum(d["recovered"] for d in log),
            "failed_tops": int((state == FAILED).sum())}


def min_gap(res):
    """the smallest runner-up gap over the re-attached tops (inf: none had a second candidate)"""
    return min(res["gap"].values(), default=np.inf)

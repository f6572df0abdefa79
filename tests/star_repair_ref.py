"""CPU restatement of the RRT* batch's repair (pp_star_repair, DESIGN.md §3.8 "Re-attaching
orphaned subtrees"), built on star_revalidate_ref (edges, keep_mask, compact) and on what the
oracle exports: oracle.dubins, OracleScene.verify_line and oracle.star_k.  A plain helper module
(no fixtures): the tests import it.

For one tree with stored x, y, yaw, parent, cost, the new scene, the batch's k and R rounds:
  K0        = star_revalidate_ref's kept set (rounds = 0 is revalidate, result for result; a
              blocked root re-attaches nothing)
  round r   tops = dropped nodes that were no top before and whose own edge is not ok (r = 1) or
            whose parent was a top of an earlier round that found no parent (r > 1)
            candidates of top t = the star_k(k, |K|) nearest nodes of (x_t, y_t) by (d2, index)
            among K as it stood at the start of the round; the edge t -> p keeps t's stored pose
            and is feasible by star_edge; total = cost[p] + e; the choice is the first strict
            minimum of total in candidate order
            a top with a choice takes parent, elen, cost; every dropped node whose chain of ok
            edges reaches it is kept again with cost = cost[parent] + elen, parents first
Every top reads the start-of-round state alone, so the order in which tops are taken cannot
matter (`order` permutes it: the tests run it reversed and shuffled).
"""
import numpy as np

import oracle
import star_revalidate_ref as ref
from star_revalidate_ref import root_ok

FAILED, ATTACHED = 3, 2


def _choose(osc, x, y, yaw, cost, t, cand):
    """(parent, elen, total, gap): the first strict minimum of total over the candidates in their
    order (parent -1: no feasible candidate); gap = second-best total - best (inf: no second)"""
    best, be, bt, second = -1, np.inf, np.inf, np.inf
    for p in cand:
        p = int(p)
        d = oracle.dubins(x[t], y[t], yaw[t], x[p], y[p], yaw[p], osc.turn_radius, osc.step_size)
        if d is None:
            continue
        if not osc.verify_line(np.append(d[0], x[p]), np.append(d[1], y[p])):
            continue
        total = cost[p] + d[4]
        if total < bt:
            second = bt
            best, be, bt = p, d[4], total
        elif total < second:
            second = total
    return best, be, bt, second - bt


def repair(osc, tree, k, rounds, order=None):
    """dict: keep0 (K0), keep, tree (compacted, with cost), new_index, elen (per old node: the
    restated edge cost, a re-attached top's new one), parent / cost (per old node, after the
    call), rounds (one dict per round that had tops: tops, reattached, recovered, tasks),
    reattached, recovered (sums; recovered counts the re-attached tops too), failed_tops, gap
    (old index of a re-attached top -> its runner-up gap), none_edges.
    order: None, or a function (round, tops array) -> the tops in the order to take them"""
    x, y, yaw = (np.asarray(a, dtype=np.float64) for a in tree[:3])
    par = np.array(tree[3], dtype=np.int64)
    cost = np.array(tree[4], dtype=np.float64)
    n = len(x)
    eok, elen, none = ref.edges(osc, tree)
    rok = root_ok(osc, tree)
    keep0 = ref.keep_mask(eok, par, rok)
    keep = keep0.copy()
    state = np.zeros(n, dtype=np.int8)  # 0 never a top, ATTACHED, FAILED
    log, gap = [], {}
    for r in range(1, (rounds if rok else 0) + 1):
        if r == 1:
            tops = np.flatnonzero(~keep & ~eok)
        else:
            tops = np.array([i for i in range(1, n)
                             if not keep[i] and state[i] == 0 and state[par[i]] == FAILED],
                            dtype=np.int64)
        tops = tops[tops > 0]
        if len(tops) == 0:
            break
        kidx = np.flatnonzero(keep)
        kk = oracle.star_k(k, len(kidx))
        staged = []
        for t in (tops if order is None else order(r, tops)):
            t = int(t)
            dx, dy = x[t] - x[kidx], y[t] - y[kidx]
            d2 = dx * dx + dy * dy
            cand = kidx[np.lexsort((kidx, d2))[:kk]]
            staged.append((t,) + _choose(osc, x, y, yaw, cost, t, cand))
        got = 0
        front = []
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
        # the subtrees under the re-attached tops, level by level: parents final before children
        while front:
            mark = np.zeros(n, dtype=bool)
            mark[front] = True
            front = [i for i in range(1, n) if not keep[i] and state[i] == 0 and mark[par[i]]]
            for i in front:
                assert eok[i]
                cost[i] = cost[par[i]] + elen[i]
                keep[i] = True
            rec += len(front)
        log.append({"tops": int(len(tops)), "reattached": got, "recovered": rec,
                    "tasks": int(len(tops)) * kk})
    new_tree, new_index = ref.compact((x, y, yaw, par, cost), keep)
    return {"keep0": keep0, "keep": keep, "tree": new_tree, "new_index": new_index, "elen": elen,
            "parent": par, "cost": cost, "rounds": log, "gap": gap, "none_edges": none,
            "edge_ok": eok, "kept": int(keep.sum()),
            "reattached": sum(d["reattached"] for d in log),
            "recovered": sum(d["recovered"] for d in log),
            "failed_tops": int((state == FAILED).sum())}


def min_gap(res):
    """the smallest runner-up gap over the re-attached tops (inf: none had a second candidate)"""
    return min(res["gap"].values(), default=np.inf)

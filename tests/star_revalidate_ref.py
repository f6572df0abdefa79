"""CPU restatement of the RRT* batch's revalidation (pp_star_revalidate, DESIGN.md §3.8 "RRT*
trees"), composed only from what the oracle exports: oracle.dubins and OracleScene.verify_line.  A
plain helper module (no fixtures): the tests import it.

Node i > 0 of a tree with stored poses (x, y, yaw), parents and costs:
  edge_ok[i] = RRT*'s feasible edge (§3.7 item 3, star_edge of oracle/rrtstar_py.py) from node i's
               stored pose to its parent's stored pose: the Dubins steer is Some and Space::verify
               accepts its points followed by the parent's point.  A None steer is infeasible (and
               counted: a tree the library grew has none)
  elen[i]    = that edge's Dubins cost
  keep[0]    = 1; root_ok = False (polygon mode: the root fails verify as a point) drops every
               other node
  keep[i]    = every edge on the chain i -> parent -> ... -> root is ok.  The chain is NOT
               index-ordered: a rewired node's parent is the later node that rewired it
Kept nodes keep their order, poses and costs; parents are remapped (and may exceed their child).
"""
import numpy as np

import oracle
from revalidate_ref import root_ok, with_discs  # noqa: F401  (re-exported for the tests)


def edges(osc, tree):
    """(edge_ok bool[n], elen f64[n], none_edges): edge_ok[0] = True, elen[0] = 0"""
    x, y, yaw, par = tree[:4]
    ok = np.ones(len(x), dtype=bool)
    elen = np.zeros(len(x))
    none = 0
    for i in range(1, len(x)):
        p = int(par[i])
        d = oracle.dubins(x[i], y[i], yaw[i], x[p], y[p], yaw[p], osc.turn_radius, osc.step_size)
        if d is None:
            ok[i] = False
            elen[i] = np.inf
            none += 1
            continue
        ok[i] = osc.verify_line(np.append(d[0], x[p]), np.append(d[1], y[p]))
        elen[i] = d[4]
    return ok, elen, none


def keep_mask(eok, par, rok=True):
    """keep by walking every node's chain to the root, memoised (no index order assumed)"""
    n = len(eok)
    state = np.full(n, -1, dtype=np.int8)  # -1 unknown, 0 dropped, 1 kept
    state[0] = 1
    for i in range(1, n):
        chain = []
        v = i
        while state[v] < 0:
            chain.append(v)
            assert len(chain) < n, "a cycle in the parent array"
            v = int(par[v])
        s = state[v]
        for u in reversed(chain):  # from the known ancestor down
            s = 1 if (s and rok and eok[u]) else 0
            state[u] = s
    return state.astype(bool)


def keep_brute(eok, par, rok=True):
    """the definition, node by node: every edge of the chain to the root"""
    n = len(eok)
    keep = np.zeros(n, dtype=bool)
    keep[0] = True
    for i in range(1, n):
        v, good, steps = i, bool(rok), 0
        while v != 0:
            good = good and bool(eok[v])
            v = int(par[v])
            steps += 1
            assert steps < n, "a cycle in the parent array"
        keep[i] = good
    return keep


def compact(tree, keep):
    """((x, y, yaw, parent, cost) of the kept nodes in order, new_index int32[n] with -1 dropped);
    a remapped parent is a kept node but not necessarily an earlier one"""
    x, y, yaw, par, cost = tree[:5]
    new_index = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    npar = np.asarray(par)[keep].astype(np.int32)
    npar[1:] = new_index[npar[1:]]
    assert npar[0] == -1 and (npar[1:] >= 0).all()
    assert (npar[1:] != np.arange(1, len(npar))).all()
    return (np.asarray(x)[keep], np.asarray(y)[keep], np.asarray(yaw)[keep], npar,
            np.asarray(cost)[keep]), new_index


def revalidate(osc, tree):
    """dict: edge_ok, elen, none_edges, keep, tree (compacted, with cost), new_index, kept, failed
    (edges), orphans (edge ok, yet dropped), kept_back (kept nodes whose parent index exceeds their
    own), orphans_via_later (dropped nodes whose own edge is ok and whose parent index is
    higher)"""
    par = np.asarray(tree[3])
    eok, elen, none = edges(osc, tree)
    keep = keep_mask(eok, par, root_ok(osc, tree))
    new_tree, new_index = compact(tree, keep)
    back = par > np.arange(len(par))
    return {"edge_ok": eok, "elen": elen, "none_edges": none, "keep": keep, "tree": new_tree,
            "new_index": new_index, "kept": int(keep.sum()), "failed": int((~eok).sum()),
            "orphans": int((eok & ~keep).sum()), "kept_back": int((keep & back).sum()),
            "orphans_via_later": int((eok & ~keep & back).sum())}


def depth(par):
    """edges to the root of every node, by walking chains (no index order assumed)"""
    n = len(par)
    d = np.full(n, -1, dtype=np.int64)
    d[0] = 0
    for i in range(1, n):
        chain, v = [], i
        while d[v] < 0:
            chain.append(v)
            v = int(par[v])
        for k, u in enumerate(reversed(chain)):
            d[u] = d[v] + 1 + k
    return d


def descendants(par):
    """descendant count of every node (itself excluded), children before parents by depth"""
    c = np.zeros(len(par), dtype=np.int64)
    for i in np.argsort(-depth(par), kind="stable"):
        if i != 0:
            c[int(par[i])] += c[i] + 1
    return c


def quarter_subtree_node(tree):
    """the node whose descendant count is closest to n / 4"""
    cnt = descendants(tree[3])
    return 1 + int(np.argmin(np.abs(cnt[1:] - len(tree[0]) / 4.0)))


def oracle_tree(start, tree, elen, extra):
    """an OracleStarTree holding `tree` (x, y, yaw, parent, cost) with edge costs `elen` and room
    for `extra` more nodes"""
    n = len(tree[0])
    tr = oracle.OracleStarTree(tuple(start), n + extra + 1)
    tr.x[:n], tr.y[:n], tr.yaw[:n], tr.parent[:n], tr.cost[:n] = tree[:5]
    tr.elen[:n] = elen
    tr._c.n = n
    return tr

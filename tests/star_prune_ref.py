"""CPU restatement of the RRT* batch's prune by the focus bound (pp_star_prune, DESIGN.md §3.7
"Pruning by the focus bound").  A plain helper module (no fixtures): the tests import it.

Node i > 0 of a tree with stored points (x, y), parents and costs, against the focus (fx, fy), the
bound L and the scene's turn radius R:
  fails[i]   = cost[i] * R + sqrt((x[i]-fx)*(x[i]-fx) + (y[i]-fy)*(y[i]-fy)) > L   (numpy f64:
               every product and sum rounded on its own, a correctly rounded square root; strict)
  protected  = the nodes on the chain keep_node -> parent -> ... -> root (keep_node -1: none): they
               pass whatever the test says
  keep       = star_revalidate_ref.keep_mask of the verdicts: the root stays, node i stays iff it
               and every node on its chain to the root pass.  The chain is NOT index-ordered
Kept nodes keep their order, poses and costs; parents are remapped (star_revalidate_ref.compact).
"""
import numpy as np

import star_revalidate_ref as reval_ref


def node_value(tree, R, fxy):
    """cost * R + |node - focus| of every node, in the order of operations of the spec"""
    x, y, cost = np.asarray(tree[0]), np.asarray(tree[1]), np.asarray(tree[4])
    dx, dy = x - np.float64(fxy[0]), y - np.float64(fxy[1])
    return cost * np.float64(R) + np.sqrt(dx * dx + dy * dy)


def chain(par, node):
    """node -> parent -> ... -> root as a list (empty for node -1)"""
    out = []
    v = int(node)
    while v >= 0:
        out.append(v)
        assert len(out) <= len(par), "a cycle in the parent array"
        v = int(par[v])
    assert not out or out[-1] == 0
    return out


def verdicts(tree, R, fxy, L, keep_node=-1):
    """passes bool[n]: the node test with the protected chain; passes[0] = True"""
    par = np.asarray(tree[3])
    assert -1 <= int(keep_node) < len(par)
    ok = ~(node_value(tree, R, fxy) > np.float64(L))
    ok[0] = True
    ok[chain(par, keep_node)] = True
    return ok


def prune(tree, R, fxy, L, keep_node=-1):
    """dict: passes (own verdicts), keep, tree (compacted, with cost), new_index, kept, elen (of
    the kept nodes, when `tree` carries a sixth array, else None), via_ancestor (nodes that pass
    their own test yet are dropped through an ancestor), kept_back (kept nodes whose parent index
    exceeds their own)"""
    par = np.asarray(tree[3])
    ok = verdicts(tree, R, fxy, L, keep_node)
    keep = reval_ref.keep_mask(ok, par)
    new_tree, new_index = reval_ref.compact(tree, keep)
    back = par > np.arange(len(par))
    elen = np.asarray(tree[5])[keep] if len(tree) > 5 else None
    return {"passes": ok, "keep": keep, "tree": new_tree, "new_index": new_index,
            "kept": int(keep.sum()), "elen": elen, "via_ancestor": int((ok & ~keep).sum()),
            "kept_back": int((keep & back).sum())}


def margin(tree, R, fxy, L, keep_node=-1):
    """min over the unprotected nodes i > 0 of |cost*R + d - L| / L (inf: none, or L = +inf): how
    far the nearest verdict is from flipping"""
    if not np.isfinite(L):
        return np.inf
    free = np.ones(len(tree[0]), dtype=bool)
    free[0] = False
    free[chain(np.asarray(tree[3]), keep_node)] = False
    if not free.any():
        return np.inf
    return float(np.min(np.abs(node_value(tree, R, fxy)[free] - L)) / L)

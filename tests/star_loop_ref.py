"""The replanning loop of DESIGN.md §9 on the CPU, composed from the restatements alone: every step
is one that some restatement already states (star_goal_ref.plan, star_shortcut_commit_ref,
star_focus_ref.Query, star_prune_ref, star_advance_ref, star_repair_ref, revalidate_ref.with_discs).
A plain helper module (no fixtures): tests/test_star_loop_ref.py runs it on the oracle alone and
tests/test_gpu_star_loop.py takes its shapes, its disc and its continuation from here.

The run: bench6_open, the four starts and seeds 0 / 5 / 11 / 12 of tests/test_gpu_star_advance.py,
N0 = 300 iterations, then TURNS = 6 turns in rows of N0 + TURNS * STEP + 1 nodes.  One turn:
  1. plan(goal)                                    best node and cost, -1 and inf without one
  2. shortcut_commit(goal, node, span = SPAN)      a query without a plan is skipped
  3. focus(goal, cost)                             an infinite cost leaves the query unfocused
  4. prune(keep = node)
  5. advance(node, hops = 1, rounds = ROUNDS)      node -1: the tree stays
  6. turn DISC_ON (2): the scene becomes the first one plus one disc across query 0's next edge
     (disc_for), with repair(ROUNDS); turn DISC_OFF (4): back to the first scene, with
     repair(ROUNDS).  By turn 2 the pruned and advanced trees hold 1 to 12 nodes (one unplanned
     tree aside) and a top sees at most a handful of kept nodes, all behind the disc: this disc
     drops nodes and the repair recovers none.  So turn DISC_FIRST (0), where the trees still
     hold a hundred nodes, has a scene change of its own: the first scene plus one disc in the
     largest tree (disc_in_largest), with repair(ROUNDS), which recovers most of what it drops
  7. extend(STEP)
A query's state between the steps is what the batch exports: the tree (x, y, yaw, parent, cost),
its edge costs, `iterations`, `skipped`, the focus and the rewire counter.
"""
import math

import numpy as np

import forest_state_ref as fs
import oracle
import star_advance_ref as adv
import star_focus_ref
import star_goal_ref
import star_prune_ref
import star_repair_ref as rep
import star_revalidate_ref as ref
import star_shortcut_commit_ref as commit_ref

SEEDS = [0, 5, 11, 12]
CASES = [(0, 0.0), (8, 0.75)]
N0, TURNS, STEP, SPAN, ROUNDS = 300, 6, 100, 6, 2
MAX_ITER = N0 + TURNS * STEP
DISC_FIRST, DISC_ON, DISC_OFF, DISC_R = 0, 2, 4, 0.3


def starts(raw):
    return [raw["start"], (-4.0, -4.5, 0.3), (-3.0, -3.0, 0.785), (2.0, -4.0, 1.2)]


def disc_for(tree, node, goal):
    """(x, y, r) of a disc on the middle of the edge the vehicle would drive next: the first edge
    of the chain root -> node, or the goal edge when node is the root or -1"""
    x, y = tree[0], tree[1]
    tx, ty = float(goal[0]), float(goal[1])
    if node > 0:
        c = adv.chain(np.asarray(tree[3]), node)[-2]
        tx, ty = float(x[c]), float(y[c])
    return (0.5 * (float(x[0]) + tx), 0.5 * (float(y[0]) + ty), DISC_R)


def disc_in_largest(trees):
    """(x, y, r) of tests/test_gpu_star_repair.py's disc in the batch's largest tree (the first of
    them): on the node whose subtree is closest to a quarter of the tree"""
    t = trees[int(np.argmax([len(t[0]) for t in trees]))]
    v = ref.quarter_subtree_node(t)
    return (float(t[0][v]), float(t[1][v]), DISC_R)


def scene_with(raw, disc):
    """the first scene with one more disc (None: without)"""
    return raw if disc is None else ref.with_discs(raw, [disc])


def continued(osc, tree, elen, seed, it, skipped, fxy, bound, n_steps, k, eta):
    """the star_focus_ref.Query that holds (tree, elen) with the given counters and focus, after
    n_steps more iterations"""
    root = (float(tree[0][0]), float(tree[1][0]), float(tree[2][0]))
    q = star_focus_ref.Query(osc, root, int(seed), MAX_ITER, k, eta)
    q.tr = ref.oracle_tree(root, tree, elen, n_steps)
    q.it, q.skipped = int(it), int(skipped)
    q.set_focus(fxy, bound)
    return q.extend(n_steps)


def repaired_elen(elen, e):
    """the edge costs after star_repair_ref.repair's result e of a tree with stored edge costs
    elen: a re-attached top takes its new edge's, every other kept node keeps its stored one"""
    out = np.array(elen, dtype=np.float64)
    for t in e["gap"]:
        out[t] = e["elen"][t]
    return out[e["keep"]]


def check(tree, elen):
    verdict, _ = fs.check_tree(tree[3], elen, tree[4])
    assert verdict == fs.OK, verdict


class Slot:
    """one query between the steps"""

    def __init__(self, osc, start, seed, k, eta):
        q = star_focus_ref.Query(osc, start, seed, MAX_ITER, k, eta).extend(N0)
        a = q.arrays()
        self.tree, self.elen = tuple(a[:5]), a[5]
        self.seed, self.it, self.skipped, self.rewires = int(seed), q.it, q.skipped, q.rewires
        self.fxy, self.bound = (0.0, 0.0), math.inf


def new_log():
    return dict(commit_rewired=0, prune_dropped=0, advance_below=0, advance_reattached=0,
                repair_reattached=0, no_plan=0, disc_dropped={t: 0 for t in (DISC_FIRST, DISC_ON)},
                disc_recovered={t: 0 for t in (DISC_FIRST, DISC_ON)}, root_best=[],
                turns=[])


def note_advance(log, turn, nodes, exp):
    """what a turn's advance adds to the log; a root_best entry is (turn, the queries whose best
    node is the root, the queries that moved)"""
    log["advance_below"] += sum(e["below"] for e in exp)
    log["advance_reattached"] += sum(e["reattached"] for e in exp)
    at_root = [q for q, m in enumerate(nodes) if m == 0]
    moved = [q for q, e in enumerate(exp) if not e["identity"]]
    if at_root and moved:
        assert all(exp[q]["identity"] for q in at_root)
        log["root_best"].append((turn, at_root, moved))


def assert_not_vacuous(log, k):
    assert log["commit_rewired"] > 0, log
    assert log["prune_dropped"] > 0, log
    assert log["advance_below"] > 0, log
    assert log["advance_reattached"] + log["repair_reattached"] > 0, log
    assert log["no_plan"] > 0, log
    assert all(v > 0 for v in log["disc_dropped"].values()), log
    assert sum(log["disc_recovered"].values()) > 0, log
    if k == 0:
        assert log["root_best"], log


def run(raw, k, eta, turns=TURNS):
    """the loop on the oracle alone: (slots, log)"""
    goal = raw["goal"]
    R = raw["robot"][2]
    osc = oracle.OracleScene.from_raw(raw)
    slots = [Slot(osc, s, seed, k, eta) for s, seed in zip(starts(raw), SEEDS)]
    log = new_log()
    for turn in range(turns):
        row = {"turn": turn, "n0": [len(s.tree[0]) for s in slots]}
        nodes = []
        for s in slots:  # 1 to 4
            node, cost, _ = star_goal_ref.plan(osc, s.tree, goal)
            if node >= 0:
                res = commit_ref.commit_oracle(osc, s.tree, s.elen, goal, node, SPAN)[0]
                s.tree, s.elen = commit_ref.committed_tree(s.tree, res), res["edge_cost"]
                s.rewires += res["n_rewired"]
                log["commit_rewired"] += res["n_rewired"]
                node, cost = res["node"], res["cost_out"]
                check(s.tree, s.elen)
            else:
                log["no_plan"] += 1
            s.fxy, s.bound = (float(goal[0]), float(goal[1])), cost * R
            e = star_prune_ref.prune(s.tree + (s.elen,), R, s.fxy, s.bound, node)
            log["prune_dropped"] += len(s.tree[0]) - e["kept"]
            node = int(e["new_index"][node]) if node >= 0 else -1
            s.tree, s.elen = e["tree"], e["elen"]
            check(s.tree, s.elen)
            nodes.append(node)
        row["plan"], row["pruned"] = list(nodes), [len(s.tree[0]) for s in slots]
        exp = [adv.advance(osc, s.tree, s.elen, k, nodes[q], 1, ROUNDS)  # 5
               for q, s in enumerate(slots)]
        note_advance(log, turn, nodes, exp)
        for q, (s, e) in enumerate(zip(slots, exp)):
            nodes[q] = int(e["new_index"][nodes[q]]) if nodes[q] >= 0 else -1
            s.tree, s.elen = e["tree"], e["elen"]
            check(s.tree, s.elen)
        row["advanced"] = [len(s.tree[0]) for s in slots]
        row["reattached"] = [e["reattached"] for e in exp]
        if turn in (DISC_FIRST, DISC_ON, DISC_OFF):  # 6
            disc = (disc_in_largest([s.tree for s in slots]) if turn == DISC_FIRST else
                    disc_for(slots[0].tree, nodes[0], goal) if turn == DISC_ON else None)
            osc = oracle.OracleScene.from_raw(scene_with(raw, disc))
            for q, s in enumerate(slots):
                e = rep.repair(osc, s.tree, k, ROUNDS)
                assert e["none_edges"] == 0
                if turn != DISC_OFF:
                    log["disc_dropped"][turn] += len(s.tree[0]) - int(e["keep0"].sum())
                    log["disc_recovered"][turn] += e["recovered"]
                else:
                    assert e["keep"].all()  # nothing is in the way any more
                log["repair_reattached"] += e["reattached"]
                s.elen = repaired_elen(s.elen, e)
                s.tree = e["tree"]
                check(s.tree, s.elen)
            row["repaired"] = [len(s.tree[0]) for s in slots]
        for s in slots:  # 7
            q = continued(osc, s.tree, s.elen, s.seed, s.it, s.skipped, s.fxy, s.bound, STEP, k,
                          eta)
            a = q.arrays()
            s.tree, s.elen = tuple(a[:5]), a[5]
            s.it, s.skipped, s.rewires = q.it, q.skipped, s.rewires + q.rewires
            check(s.tree, s.elen)
        row["extended"] = [len(s.tree[0]) for s in slots]
        log["turns"].append(row)
    return slots, log

"""The replanning loop on the oracle alone (tests/star_loop_ref.py): the inputs of
tests/test_gpu_star_loop.py are known not to be vacuous before they reach a GPU, and every tree
between two steps is a valid one whose stored costs are their own rebuild (star_loop_ref.check,
asserted after every step inside run)."""
import numpy as np
import pytest

import star_loop_ref as loop


@pytest.mark.parametrize("k,eta", loop.CASES)
def test_the_loop_is_not_vacuous(oracle_mod, k, eta):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    slots, log = loop.run(raw, k, eta)
    for row in log["turns"]:
        print(row)
    print({key: v for key, v in log.items() if key != "turns"})
    loop.assert_not_vacuous(log, k)
    assert all(s.it == loop.MAX_ITER for s in slots)
    assert all(len(s.tree[0]) <= loop.MAX_ITER + 1 for s in slots)
    # queries of one batch in different states in the same call: some turn has a query without a
    # plan next to one with a plan
    assert any(min(row["plan"]) < 0 <= max(row["plan"]) for row in log["turns"])
    if k == 0:  # the vehicle has arrived: the advance leaves that query and moves another
        turn, at_root, moved = log["root_best"][0]
        assert set(at_root).isdisjoint(moved)


def test_disc_lies_on_the_next_edge():
    x = np.array([0.0, 2.0, 4.0, 1.0])
    y = np.array([0.0, 0.0, 2.0, 5.0])
    par = np.array([-1, 0, 1, 0])
    tree = (x, y, np.zeros(4), par, np.zeros(4))
    goal = (6.0, 8.0, 0.0)
    assert loop.disc_for(tree, 2, goal) == (1.0, 0.0, loop.DISC_R)
    assert loop.disc_for(tree, 3, goal) == (0.5, 2.5, loop.DISC_R)
    assert loop.disc_for(tree, 0, goal) == (3.0, 4.0, loop.DISC_R)  # the goal edge
    assert loop.disc_for(tree, -1, goal) == (3.0, 4.0, loop.DISC_R)

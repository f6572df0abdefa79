"""CPU: the focused-sampling restatement tests/star_focus_ref.py (DESIGN.md §3.7 "Focused
sampling") against oracle.star_extend, and the inputs of tests/test_gpu_star_focus.py: each class
of iteration a GPU case relies on (no skip, a skip inside the first wave round, a skip in a later
round, a full miss) occurs in the reference run of that case.

Scene bench6_open, queries 0-2 of config3_queries, k = 0, eta = 0, 150 + 150 iterations; the bounds
are the plan's cost x turn radius, 1.002 x and 0.5 x the distance between root and goal."""
import math

import numpy as np
import pytest

import star_focus_ref as ref
import star_goal_ref

N1 = N2 = 150
# the second 150 iterations by skip: (j = 0, 1 <= j < 64, 64 <= j < 1024, full miss) per query
EXPECTED = {
    "plan": [(17, 133, 0, 0), (30, 120, 0, 0), (43, 107, 0, 0)],
    "tight": [(1, 43, 105, 1), (2, 97, 51, 0), (2, 65, 83, 0)],
    "empty": [(0, 0, 0, 150)] * 3,
}


@pytest.fixture(scope="module")
def case(oracle_mod):
    from pathplanning_amd import scenes

    raw = scenes.bench6_open()
    starts, goals, seeds = scenes.config3_queries(raw, 0, 3)
    osc = oracle_mod.OracleScene.from_raw(raw)
    return raw, osc, starts, goals, seeds


def _grown(case, q, max_iter=N1 + N2):
    _, osc, starts, _, seeds = case
    return ref.Query(osc, starts[q], seeds[q], max_iter, 0, 0.0).extend(N1)


def _bound(case, kind, q, query):
    _, osc, starts, goals, _ = case
    if kind == "plan":
        _, cost, _ = star_goal_ref.plan(osc, query.arrays(), goals[q])
        assert math.isfinite(cost)
        return cost * osc.turn_radius
    return {"tight": 1.002, "empty": 0.5}[kind] * ref.foci_distance(starts[q], goals[q])


def test_unfocused_reference_is_the_oracle(oracle_mod, case):
    """every bound +inf (never set, set to +inf, and cleared): one straight oracle.star_extend
    run, bit for bit, rewires included"""
    _, osc, starts, goals, seeds = case
    for q in range(3):
        tr = oracle_mod.OracleStarTree(tuple(starts[q]), N1 + N2 + 1)
        _, erw, _, _ = oracle_mod.star_extend(osc, tr, int(seeds[q]), 0, N1 + N2, 0, 0.0)
        exp = tr.star_arrays()
        a = ref.Query(osc, starts[q], seeds[q], N1 + N2, 0, 0.0)
        a.extend(1).extend(36)
        a.set_focus(goals[q][:2], math.inf)
        a.extend(113)
        a.set_focus()
        a.extend(10 ** 6)  # capped at max_iter
        assert a.it == N1 + N2 and a.skipped == 0 and a.js == [0] * (N1 + N2)
        assert a.rewires == erw
        for g, e in zip(a.arrays(), exp):
            assert np.array_equal(g, e)


@pytest.mark.parametrize("kind", ["plan", "tight", "empty"])
def test_gpu_case_inputs_are_not_vacuous(case, kind):
    for q in range(3):
        a = _grown(case, q)
        n_before = a.tr.n
        a.set_focus(case[3][q][:2], _bound(case, kind, q, a))
        a.extend(N2)
        got = ref.classes(a.js[N1:])
        print(kind, q, got, "skipped", a.skipped)
        assert got == EXPECTED[kind][q], (kind, q, got)
        assert a.it == N1 + N2
        js = np.asarray(a.js[N1:])
        assert a.skipped == int(np.where(js == ref.MISS, ref.DRAWS - 1, js).sum())
        if kind == "empty":
            assert a.tr.n == n_before and a.skipped == N2 * (ref.DRAWS - 1)
    # the classes each GPU case uses
    for kind_, q_, cls in (("plan", 0, (0, 1)), ("tight", 1, (0, 1, 2)), ("tight", 0, (3,)),
                           ("empty", 2, (3,))):
        assert all(EXPECTED[kind_][q_][c] > 0 for c in cls)


def test_full_miss_advances_skipped_by_1023_and_it_by_1(case):
    a = _grown(case, 0)
    a.set_focus(case[3][0][:2], _bound(case, "empty", 0, a))
    before = a.arrays()
    for step in range(1, 4):
        a.extend(1)
        assert a.js[-1] == ref.MISS
        assert a.it == N1 + step and a.skipped == step * (ref.DRAWS - 1) == step * 1023
    for g, e in zip(a.arrays(), before):  # no insert, no rewire
        assert np.array_equal(g, e)
    # clearing keeps the skip: the next sample is draw it + skipped
    a.set_focus()
    a.extend(1)
    assert a.js[-1] == 0 and a.skipped == 3 * 1023


def test_best_cost_does_not_get_worse(case):
    """for a fixed goal the best cost after a focused extension is <= the best cost before it
    (RRT* only ever lowers a node's cost, and the goal edge of a node does not change)"""
    _, osc, _, goals, _ = case
    for q in range(3):
        a = _grown(case, q)
        _, before, _ = star_goal_ref.plan(osc, a.arrays(), goals[q])
        a.set_focus(goals[q][:2], before * osc.turn_radius)
        a.extend(N2)
        _, after, _ = star_goal_ref.plan(osc, a.arrays(), goals[q])
        print(q, before, after)
        assert after <= before

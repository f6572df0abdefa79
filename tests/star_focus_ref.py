"""CPU restatement of the RRT* batch's focused sampling (pp_star_set_focus, DESIGN.md §3.7 "Focused
sampling"), composed only from what the oracle exports: oracle.gen_range and oracle.star_extend.
A plain helper module (no fixtures): the tests import it.

A query carries a focus point (fx, fy), a bound L (finite and > 0, or +inf: no focus) and a counter
`skipped`; draw d is the point (gen_range(seed, 2d, minx, maxx), gen_range(seed, 2d + 1, miny,
maxy)), and (x0, y0) is the root's stored point.  Iteration `it`:
  L = +inf:  the sample is draw it + skipped
  L finite:  the first j in [0, DRAWS) whose draw it + skipped + j has
             sqrt((x-x0)^2 + (y-y0)^2) + sqrt((x-fx)^2 + (y-fy)^2) < L (f64, the raw sample);
             skipped += j.  With none: skipped += DRAWS - 1 and the iteration ends without a
             nearest node, an insert or a rewire
and it += 1 either way.  An iteration with sample draw d is one oracle.star_extend(sc, tr, seed, d,
1, k, eta): the oracle uses its `it0` only as the RNG counter.
"""
import math

import numpy as np

import oracle

DRAWS = 1024  # PP_STAR_FOCUS_DRAWS
MISS = -1     # an iteration's entry in `js` when none of its draws is in the set


def in_set(x, y, x0, y0, fx, fy, bound):
    ax, ay, bx, by = x - x0, y - y0, x - fx, y - fy
    return math.sqrt(ax * ax + ay * ay) + math.sqrt(bx * bx + by * by) < bound


def foci_distance(start, goal):
    dx, dy = float(goal[0]) - float(start[0]), float(goal[1]) - float(start[1])
    return math.sqrt(dx * dx + dy * dy)


def classes(js):
    """an iteration list's counts by skip: (j = 0, 1 <= j < 64, 64 <= j < DRAWS, full miss)"""
    js = np.asarray(js)
    return (int((js == 0).sum()), int(((js >= 1) & (js < 64)).sum()),
            int(((js >= 64) & (js < DRAWS)).sum()), int((js == MISS).sum()))


class Query:
    """One query of the batch: the oracle's tree plus the iteration, focus and skip state.
    ``osc`` and ``tr`` may be replaced between extends (a scene change with its revalidation)."""

    def __init__(self, osc, start, seed, max_iter, k, eta):
        self.osc = osc
        self.tr = oracle.OracleStarTree(tuple(float(v) for v in start), int(max_iter) + 1)
        self.seed = int(seed)
        self.max_iter = int(max_iter)
        self.k = int(k)
        self.eta = float(eta)
        self.it = 0
        self.skipped = 0
        self.rewires = 0
        self.fxy = (0.0, 0.0)
        self.bound = math.inf
        self.js = []  # per iteration: the draws skipped, MISS for a full miss

    def set_focus(self, fxy=None, bound=math.inf):
        """fxy None clears (the bound becomes +inf, skipped stays)"""
        if fxy is None:
            self.bound = math.inf
            return
        assert bound > 0.0
        self.fxy = (float(fxy[0]), float(fxy[1]))
        self.bound = float(bound)

    def _draw(self, d):
        sc = self.osc
        return (oracle.gen_range(self.seed, 2 * d, sc.minx, sc.maxx),
                oracle.gen_range(self.seed, 2 * d + 1, sc.miny, sc.maxy))

    def extend(self, n_steps):
        """n_steps iterations, to max_iter at most"""
        x0, y0 = float(self.tr.x[0]), float(self.tr.y[0])
        for _ in range(min(int(n_steps), self.max_iter - self.it)):
            j = 0
            if self.bound < math.inf:
                j = MISS
                for t in range(DRAWS):
                    x, y = self._draw(self.it + self.skipped + t)
                    if in_set(x, y, x0, y0, self.fxy[0], self.fxy[1], self.bound):
                        j = t
                        break
            self.js.append(j)
            if j == MISS:
                self.skipped += DRAWS - 1
            else:
                self.skipped += j
                _, rw, _, _ = oracle.star_extend(self.osc, self.tr, self.seed,
                                                 self.it + self.skipped, 1, self.k, self.eta)
                self.rewires += rw
            self.it += 1
        return self

    def arrays(self):
        """(x, y, yaw, parent, cost, elen)"""
        return self.tr.star_arrays()

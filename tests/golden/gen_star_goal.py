"""Writes tests/golden/star_goal.json: the RRT* goal-connection cases of tests/star_goal_ref.py
(the CPU restatement over the C oracle).  Run from the repository root after
__graft_entry__.build():  python tests/golden/gen_star_goal.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "rs-pathplanning_amd"), os.path.join(ROOT, "oracle"),
          os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import star_goal_ref as ref  # noqa: E402


def main():
    recs = [ref.golden_record(s) for s in ref.golden_specs()]
    with open(os.path.join(HERE, "star_goal.json"), "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")
    for r in recs:
        print(r["scene"], r["seed"], r["n_iter"], r["n_nodes"], len(r["feasible"]), r["best_node"],
              r["cost"], r["gap"], r["path_points"], r["path_length"])


if __name__ == "__main__":
    main()

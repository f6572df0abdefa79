"""Writes tests/golden/star_shortcut_commit.json: the commit cases of
tests/star_shortcut_commit_ref.py (the CPU restatement over the C oracle).  Run from the repository
root after __graft_entry__.build(): python tests/golden/gen_star_shortcut_commit.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "rs-pathplanning_amd"), os.path.join(ROOT, "oracle"),
          os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import star_shortcut_commit_ref as ref  # noqa: E402


def main():
    recs = [ref.golden_record(s) for s in ref.specs()]
    with open(os.path.join(HERE, "star_shortcut_commit.json"), "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")
    for r in recs:
        print(r["scene"], r["seed"], r["n_iter"], r["n_nodes"], r["node"], r["span"], r["D"],
              r["pairs"], r["rewired"], r["n_changed"], r["cost"], r["gap"], r["plan_before"],
              r["plan_after"])


if __name__ == "__main__":
    main()

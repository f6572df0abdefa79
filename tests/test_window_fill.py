"""CPU: which iterations a window takes (csrc/pp_window_fill.h), swept on the host by a
stand-alone C++ program (tests/window_fill/check.cpp, plain and under ASan + UBSan).

K bounds the samples a window screens; the draws in an obstacle take no sample id, so a window
spans up to 2 K iterations.  The sweep: Kw in {1, 2, 7, 64, 4096}; Kw - 1, Kw, Kw + 1, 2 Kw - 1,
2 Kw, 2 Kw + 1 and 5 Kw + 3 iterations; no draw blocked, all, alternating, one blocked run of
Kw - 1, Kw, Kw + 1 at the start, middle and end, the (Kw + 1)-th live draw on the last drawable
draw and one past it, a run straddling the cap, seeded random at 10/32/50/90 %; three round
sizes.  Every case is cut into consecutive windows; for each, against a count one draw at a time:
W <= Kw, span <= cap, W = the live draws inside the span, the span maximal, iter_off strictly
increasing and naming exactly the live iterations in order (so the windows tile the iterations),
the draws made whole rounds that stop once the span is decided."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "rs-pathplanning_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "window_fill", "check.cpp")


def _sweep(tmp_path_factory, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler on PATH")
    exe = str(tmp_path_factory.mktemp("fill") / "check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", CSRC, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_span_rule_holds_for_every_pattern(tmp_path_factory):
    got = _sweep(tmp_path_factory, [])
    print(got)
    assert got["cases"] > 1000 and got["windows"] > got["cases"]
    # the draws stop with the round that decides the span: a K = 4096 window draws 2 K only when
    # it has to (the all-blocked patterns do)
    assert got["max_draws4096"] == 8192


def test_span_rule_sweep_under_sanitizers(tmp_path_factory):
    got = _sweep(tmp_path_factory, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert got["cases"] > 1000

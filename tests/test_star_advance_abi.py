"""CPU: the ABI surface of advancing the root — pp_star_advance is declared in the header, exported
by the library, bound by the ctypes layer, listed in INTEGRATION.md, rejects a NULL context, and
RRTStarBatch has the method.  (The behaviour is tests/test_gpu_star_advance.py.)"""
import inspect
import os
import re
import subprocess

NAME = "pp_star_advance"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_advance_declared_exported_bound(built, pkg):
    from pathplanning_amd import _ffi

    with open(os.path.join(ROOT, "include", "pathplanning_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", built.LIB], check=True,
                        capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert NAME in exported
    assert NAME in _ffi.EXPORTED
    assert len(getattr(_ffi.lib(), NAME).argtypes) == 9
    assert re.search(r"pub fn %s\(" % NAME, integration)
    # the ABI version is unchanged: the function is an addition ("5 (+)")
    assert _ffi.lib().pp_abi_version() == 5
    assert re.search(r"#define PP_ABI_VERSION 5\b", header)
    assert re.search(r"5 \(\+\): pp_star_advance added", header)


def test_advance_rejects_null_context(pkg):
    from pathplanning_amd import _ffi

    assert _ffi.lib().pp_star_advance(None, None, None, 0, None, None, None, None,
                                      None) == _ffi.PP_ERR_INVALID_ARGUMENT


def test_advance_method(pkg):
    from pathplanning_amd import rrt

    assert callable(getattr(rrt.RRTStarBatch, "advance", None))
    sig = inspect.signature(rrt.RRTStarBatch.advance)
    assert list(sig.parameters)[1:] == ["nodes", "hops", "rounds", "n_old"]
    assert sig.parameters["hops"].default is None
    assert sig.parameters["rounds"].default == 0
    assert sig.parameters["n_old"].default is None
    # plan's signature is pinned by tests/test_star_shortcut_commit_abi.py: no new parameters
    plan = inspect.signature(rrt.RRTStarBatch.plan)
    assert list(plan.parameters)[1:] == ["goals", "focus", "prune", "commit"]

"""CPU: the ABI surface of relaxing the trees — pp_star_relax is declared in the header, exported by
the library, bound by the ctypes layer, listed in INTEGRATION.md, rejects a NULL context, and
RRTStarBatch has the method.  (The behaviour is tests/test_gpu_star_relax.py.)"""
import inspect
import os
import re
import subprocess

NAME = "pp_star_relax"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relax_declared_exported_bound(built, pkg):
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
    assert len(getattr(_ffi.lib(), NAME).argtypes) == 6
    assert re.search(r"pub fn %s\(" % NAME, integration)
    # the ABI version is unchanged: the function is an addition ("5 (+)")
    assert _ffi.lib().pp_abi_version() == 5
    assert re.search(r"#define PP_ABI_VERSION 5\b", header)
    assert re.search(r"5 \(\+\): pp_star_relax added, nothing else changed", header)
    # the kernels are a unit of their own, built with the rest
    assert "pp_k_relax.hip" in built.SOURCES and "pp_relax.cpp" in built.SOURCES


def test_relax_rejects_null_context(pkg):
    from pathplanning_amd import _ffi

    L = _ffi.lib()
    assert L.pp_star_relax(None, 1, None, None, None, None) == _ffi.PP_ERR_INVALID_ARGUMENT
    assert L.pp_star_relax_counts(None, None) == _ffi.PP_ERR_INVALID_ARGUMENT


def test_relax_method(pkg):
    from pathplanning_amd import rrt

    assert callable(getattr(rrt.RRTStarBatch, "relax", None))
    sig = inspect.signature(rrt.RRTStarBatch.relax)
    assert list(sig.parameters)[1:] == ["rounds", "active"]
    assert sig.parameters["rounds"].default == 1
    assert sig.parameters["active"].default is None
    # the signatures other ABI tests pin stay as they are: no new parameters
    plan = inspect.signature(rrt.RRTStarBatch.plan)
    assert list(plan.parameters)[1:] == ["goals", "focus", "prune", "commit"]
    advance = inspect.signature(rrt.RRTStarBatch.advance)
    assert list(advance.parameters)[1:] == ["nodes", "hops", "rounds", "n_old"]
    repair = inspect.signature(rrt.RRTStarBatch.repair)
    assert list(repair.parameters)[1:] == ["rounds", "n_old"]
    set_space = inspect.signature(rrt.RRTStarBatch.set_space)
    assert list(set_space.parameters)[1:] == ["space", "repair_rounds"]

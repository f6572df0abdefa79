"""CPU: the ABI surface of the shortcuts along the chain — pp_star_shortcut,
pp_star_shortcut_edges and pp_star_chain_segments are declared in the header, exported by the
library, bound by the ctypes layer, listed in INTEGRATION.md, reject a NULL context, and
RRTStarBatch has the methods.  (The behaviour is tests/test_gpu_star_shortcut.py.)"""
import os
import re
import subprocess

NAMES = ("pp_star_shortcut", "pp_star_shortcut_edges", "pp_star_chain_segments")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shortcut_declared_exported_bound(built, pkg):
    from pathplanning_amd import _ffi

    with open(os.path.join(ROOT, "include", "pathplanning_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        integration = f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", built.LIB], check=True,
                        capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _ffi.EXPORTED, name
        assert getattr(_ffi.lib(), name).argtypes is not None
        assert re.search(r"pub fn %s\(" % name, integration), name
    # the ABI version is unchanged: the functions are additions ("5 (+)")
    assert _ffi.lib().pp_abi_version() == 5
    assert re.search(r"5 \(\+\): pp_star_shortcut, pp_star_shortcut_edges and "
                     r"pp_star_chain_segments added", header)


def test_shortcut_reject_null_context(pkg):
    from pathplanning_amd import _ffi

    L = _ffi.lib()
    assert L.pp_star_shortcut(None, None, None, 8, None, None, 0, None, None, None,
                              None) == _ffi.PP_ERR_INVALID_ARGUMENT
    assert L.pp_star_shortcut_edges(None, 0, None, 0, 8, None, None, 0,
                                    None) == _ffi.PP_ERR_INVALID_ARGUMENT
    assert L.pp_star_chain_segments(None, None, None, None, 0, None, None, 0, None, None,
                                    None) == _ffi.PP_ERR_INVALID_ARGUMENT


def test_shortcut_methods_exist(pkg):
    from pathplanning_amd import rrt

    for name in ("shortcut", "shortcut_edges", "chain_segments", "shortcut_trajectories"):
        assert callable(getattr(rrt.RRTStarBatch, name, None)), name


def test_shortcut_unit_is_built(built):
    """the kernels are their own unit, compiled into the library"""
    assert "pp_k_shortcut.hip" in built.SOURCES and "pp_shortcut.cpp" in built.SOURCES
    for f in ("pp_k_shortcut.hip", "pp_shortcut.cpp"):
        assert os.path.exists(os.path.join(built.CSRC, f))


def test_every_source_file_is_listed(built):
    """csrc/ and the build's lists name the same files, in both directions: a file missing from
    SOURCES is not compiled, one missing from HEADERS does not make the library stale"""
    files = os.listdir(built.CSRC)
    assert len(set(built.SOURCES)) == len(built.SOURCES)
    assert len(set(built.HEADERS)) == len(built.HEADERS)
    assert sorted(built.SOURCES) == sorted(f for f in files if f.endswith((".hip", ".cpp")))
    assert sorted(built.HEADERS) == sorted(f for f in files if f.endswith(".h"))
    # the kernel split is complete: every kernel unit is named after its subsystem
    assert "pp_kernels.hip" not in files

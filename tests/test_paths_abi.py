"""CPU: the batched path export's ABI surface — pp_batch_paths / pp_star_paths are declared in
the header, exported by the library, bound by the ctypes layer, reject a NULL context, and the
Python batches have their ``paths`` methods.  (The behaviour is tests/test_gpu_batch_paths.py and
tests/test_gpu_star_paths.py.)"""
import os
import re
import subprocess

NAMES = ("pp_batch_paths", "pp_star_paths")


def test_paths_declared_exported_bound(built, pkg):
    from pathplanning_amd import _ffi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pathplanning_amd.h")) as f:
        header = f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", built.LIB], check=True,
                        capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _ffi.EXPORTED, name
        assert getattr(_ffi.lib(), name).argtypes is not None
    # the ABI version is unchanged: the functions are additions ("5 (+)")
    assert _ffi.lib().pp_abi_version() == 5
    assert re.search(r"5 \(\+\): pp_batch_paths / pp_star_paths added", header)


def test_paths_reject_null_context(pkg):
    from pathplanning_amd import _ffi

    L = _ffi.lib()
    assert L.pp_batch_paths(None, None, None, None, None, 0, None,
                            None) == _ffi.PP_ERR_INVALID_ARGUMENT
    assert L.pp_star_paths(None, None, None, None, None, None, 0, None, None,
                           None) == _ffi.PP_ERR_INVALID_ARGUMENT


def test_paths_methods_exist(pkg):
    from pathplanning_amd import rrt

    assert callable(getattr(rrt.RRTBatch, "paths", None))
    assert callable(getattr(rrt.RRTStarBatch, "paths", None))

"""CPU: the segment export's ABI surface — pp_star_path_segments / pp_batch_path_segments /
pp_segments_sample are declared in the header, exported by the library, bound by the ctypes layer,
reject a NULL context, and the Python layer has its methods.  (The behaviour is
tests/test_gpu_path_segments.py.)"""
import ctypes as C
import os
import re
import subprocess

NAMES = ("pp_star_path_segments", "pp_batch_path_segments", "pp_segments_sample")


def test_segments_declared_exported_bound(built, pkg):
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
    assert re.search(r"typedef struct pp_path_segments \{", header)


def test_segments_struct_layout(pkg):
    """size first, then five pointers in the header's order"""
    from pathplanning_amd import _ffi

    st = _ffi.PathSegmentsC
    assert [n for n, _ in st._fields_] == ["size", "x", "y", "yaw", "kappa", "len"]
    assert C.sizeof(st) == 8 + 5 * C.sizeof(C.c_void_p)
    assert [getattr(st, n).offset for n in _ffi.SEGMENT_FIELDS] == [8, 16, 24, 32, 40]


def test_segments_reject_null_context(pkg):
    from pathplanning_amd import _ffi

    L = _ffi.lib()
    inv = _ffi.PP_ERR_INVALID_ARGUMENT
    assert L.pp_star_path_segments(None, None, None, 0, None, None, 0, None, None, None) == inv
    assert L.pp_batch_path_segments(None, None, 0, None, None, 0, None, None, None) == inv
    assert L.pp_segments_sample(None, 0, None, None, 1.0, None, None, None, None, None, None, 0,
                                None) == inv


def test_segments_methods_exist(pkg):
    from pathplanning_amd import rrt

    for cls in (rrt.RRTBatch, rrt.RRTStarBatch):
        assert callable(getattr(cls, "path_segments", None))
        assert callable(getattr(cls, "trajectories", None))
    assert callable(getattr(rrt, "sample_segments", None))

"""CPU: the NN screen's tiling (csrc/pp_screen_geom.h) swept on the host by a stand-alone C++
program (tests/screen_geom/check.cpp, plain and under ASan + UBSan), and the window kernel's
resources read from the code object's metadata.

The sweep is every Ws in 0..4096 x 13 tree sizes: every (row, node) pair in exactly one workgroup,
<= 255 workgroups, <= kMaxChunks chunks and 1..8 rows per block, chunk lengths whole blocks and at
least one block per wave, workgroup -> (block, chunk) a bijection with one contiguous range of the
work list per XCD, and — for Ws >= 2048, ns >= 65 536 — the largest workgroup within 1.05 of the
even split ceil(Ws/64) ns / 255 (the tiling before: 1.16 at Ws = 2797, 1.29 at Ws = 2049)."""
import json
import os
import re
import shutil
import struct
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "rs-pathplanning_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "screen_geom", "check.cpp")


def _sweep(tmp_path_factory, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler on PATH")
    exe = str(tmp_path_factory.mktemp("geom") / "check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", CSRC, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    return _sweep(tmp_path_factory, [])


def test_tiling_properties_hold_for_every_window(sweep):
    assert sweep["pairs"] == 4097 * 13
    assert sweep["worst"] <= 1.05, sweep


def test_tiling_of_the_benched_window(sweep):
    # Ws = 2797: 44 rows as 8, 8, 7, 7, 7, 7; the largest workgroup is 7 rows x ns / 40
    assert sweep["rows2797"] == [8, 8, 7, 7, 7, 7]
    assert 248 <= sweep["g2797"] <= 255 and sweep["g4096"] == 255
    rows, chunks = sweep["rows2797"], sweep["chunks2797"]
    assert max(r / c for r, c in zip(rows, chunks)) <= 7 / 40


def test_tiling_sweep_under_sanitizers(tmp_path_factory):
    got = _sweep(tmp_path_factory, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert got["pairs"] == 4097 * 13


def _code_objects(blob):
    """the gfx950 ELF images of every offload bundle in the library"""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = []
    at = blob.find(magic)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(magic))
        p = at + len(magic) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", blob, p)
            tid = blob[p + 24:p + 24 + idlen]
            p += 24 + idlen
            if b"gfx950" in tid and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(magic, at + len(magic))
    return out


def test_window_kernel_resources(pkg, tmp_path):
    readelf = None
    for d in (os.path.join(os.path.dirname(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), "..",
                           "llvm", "bin"), "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, "llvm-readelf")):
            readelf = os.path.join(d, "llvm-readelf")
            break
    readelf = readelf or shutil.which("llvm-readelf")
    if readelf is None:
        pytest.skip("llvm-readelf not found")
    with open(pkg._ffi.LIB_PATH, "rb") as f:
        blob = f.read()
    found = None
    for i, co in enumerate(_code_objects(blob)):
        if not co.startswith(b"\x7fELF"):
            continue
        path = str(tmp_path / f"co{i}.elf")
        with open(path, "wb") as f:
            f.write(co)
        notes = subprocess.run([readelf, "--notes", path], capture_output=True, text=True,
                               check=True).stdout
        m = re.search(r"\.name:\s+_ZN5ppamd13window_kernelE", notes)
        if m:  # a kernel's keys are sorted: the LDS size stands before its name, the rest after
            found = {"group_segment_fixed_size": int(re.findall(
                r"\.group_segment_fixed_size:\s+(\d+)", notes[:m.start()])[-1])}
            for k in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count"):
                found[k] = int(re.search(r"\.%s:\s+(\d+)" % k, notes[m.end():]).group(1))
    assert found, "window_kernel's metadata not found in the library's code objects"
    print("window_kernel:", found)
    assert found["vgpr_count"] <= 256 and found["vgpr_spill_count"] == 0
    assert found["group_segment_fixed_size"] <= 152608  # no more LDS than before the tiling
    assert found["private_segment_fixed_size"] == 0  # no scratch

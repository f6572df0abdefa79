"""Register / scratch / LDS / occupancy of every kernel of the kernel units (the .hip files of
__graft_entry__.SOURCES) for gfx950, from the compiler's kernel-resource-usage remarks (no GPU
needed): the spill check behind DESIGN.md §3.2.

  python scripts/kernel_resources.py [name-substring ...]     the table, unit by unit
  python scripts/kernel_resources.py --dump [name-substring ...]
      one line per kernel sorted by name, without the unit: the same kernels built from another
      split of the sources give the same dump, so
          python scripts/kernel_resources.py --dump | diff saved_table.txt -
      compares a tree against a saved table."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import CSRC, SOURCES  # noqa: E402

UNITS = [f for f in SOURCES if f.endswith(".hip")]
KEYS = (("VGPRs", "vgpr"), ("SGPRs", "sgpr"), (r"ScratchSize \[bytes/lane\]", "scratch"),
        (r"LDS Size \[bytes/block\]", "lds"), (r"Occupancy \[waves/SIMD\]", "occupancy"))


def resources(unit):
    """The kernels of one unit (a file name in csrc/, or a path), in the compiler's order."""
    src = unit if os.path.isabs(unit) else os.path.join(CSRC, unit)
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                            "-ffp-contract=off", "-c", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", src, "-o",
                            os.path.join(d, "k.o")], capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1), "unit": os.path.basename(src)}
            rows.append(cur)
            continue
        for key, tag in KEYS:
            m = re.search(key + r": (\d+)", line)
            if m and cur is not None:
                cur[tag] = int(m.group(1))
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows),
                           capture_output=True, text=True).stdout.splitlines()
    for r, n in zip(rows, names):
        r["name"] = n.replace("ppamd::", "").split("(")[0].replace("void ", "")
    return rows


def all_resources(units=UNITS):
    with ThreadPoolExecutor(max_workers=len(units)) as ex:
        return [r for rows in ex.map(resources, units) for r in rows]


def fmt(r):
    return (f"{r.get('vgpr', 0):4d} v {r.get('sgpr', 0):4d} s {r.get('scratch', 0):4d} B "
            f"{r.get('lds', 0):6d} lds occ {r.get('occupancy', 0)}  {r['name']}")


if __name__ == "__main__":
    args = sys.argv[1:]
    dump = "--dump" in args
    pats = [a for a in args if a != "--dump"]
    rows = [r for r in all_resources() if not pats or any(p in r["name"] for p in pats)]
    if dump:
        for r in sorted(rows, key=lambda r: r["name"]):
            print(fmt(r))
    else:
        for r in rows:
            print(f"{r['unit']:16s} {fmt(r)}")

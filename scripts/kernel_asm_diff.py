"""Device assembly of two csrc trees compared symbol by symbol (no GPU needed): the table of
DESIGN.md Appendix A for a cut that moves kernels from one unit into another.

  python scripts/kernel_asm_diff.py PARENT_CSRC NEW_CSRC [new_unit=parent_unit ...]

Every .hip file of NEW_CSRC is compiled (HIPCC_FLAGS plus -S --cuda-device-only) and each of its
functions is compared with the function of the same name in the parent's unit of the same file
name, or in the unit a mapping names (pp_k_star.hip=pp_kernels.hip).  Local labels are numbered in
order of first appearance before the comparison; "differing" counts the lines that still differ
with label numbers dropped altogether.  Resources come from kernel_resources.resources()."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import resources  # noqa: E402
from __graft_entry__ import HIPCC_FLAGS  # noqa: E402

LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def display(mangled):
    names = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True,
                           text=True).stdout.splitlines()
    # (a function template's name comes with its return type)
    return [re.sub(r"^\w+ (?=[\w:]+<)", "", n.split("(")[0]).replace("ppamd::", "") for n in names]


def functions(src):
    """{display name: instruction and label lines} of one unit's device assembly."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", *[f for f in HIPCC_FLAGS if f != "-shared"], "-S",
                        "--cuda-device-only", src, "-o", out], capture_output=True, check=True)
        text = open(out).read().splitlines()
    funcs, cur = {}, None
    for line in text:
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif re.match(r"\.Lfunc_end\d+:", line):
            cur = None
        elif cur is not None:
            line = line.split(";")[0].strip()
            if line:
                cur.append(line)
    return dict(zip(display(list(funcs)), funcs.values()))


def renumbered(lines):
    seen = {}
    return [LABEL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), l) for l in lines]


def differing(a, b):
    a, b = [LABEL.sub(".L", l) for l in a], [LABEL.sub(".L", l) for l in b]
    ops = difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes()
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != "equal")


def res_text(r):
    return " / ".join(str(r.get(k, 0)) for k in ("vgpr", "sgpr", "scratch", "lds", "occupancy"))


def main(parent, new, pairs):
    unit_of = dict(p.split("=") for p in pairs)
    units = sorted(f for f in os.listdir(new) if f.endswith(".hip"))
    paths = {os.path.join(new, u) for u in units}
    paths |= {os.path.join(parent, unit_of.get(u, u)) for u in units}
    paths = sorted(p for p in paths if os.path.exists(p))
    with ThreadPoolExecutor(max_workers=16) as ex:
        asm = dict(zip(paths, ex.map(functions, paths)))
        res = {p: {r["name"]: r for r in rows} for p, rows in zip(paths, ex.map(resources, paths))}
    print("| unit | symbol | code | lines parent / new | differing | "
          "VGPR / SGPR / scratch B / LDS B / occupancy |\n|---|---|---|---|---|---|")
    for kernels in (True, False):
        for u in units:
            pn, pp = os.path.join(new, u), os.path.join(parent, unit_of.get(u, u))
            for name, b in sorted(asm[pn].items()):
                if (name in res[pn]) != kernels:
                    continue
                a = asm.get(pp, {}).get(name)
                if a is None:
                    print(f"| {u[:-4]} | `{name}` | **new** | - / {len(b)} | - | |")
                    continue
                same = renumbered(a) == renumbered(b)
                rp, rn = res[pp].get(name), res[pn].get(name)
                col = "(device function)" if rn is None else (
                    f"{res_text(rn)} (both)" if rp == dict(rn, unit=rp["unit"])
                    else f"**{res_text(rp)} -> {res_text(rn)}**")
                print(f"| {u[:-4]} | `{name}` | {'identical' if same else '**differs**'} | "
                      f"{len(a)} / {len(b)} | {0 if same else differing(a, b)} | {col} |")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2]), sys.argv[3:])

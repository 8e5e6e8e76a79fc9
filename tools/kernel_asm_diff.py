"""Compares the device code of two csrc trees kernel by kernel, so that a move of kernels between translation units can
show that no kernel's code changed.  Whole-unit hashes (tools/device_code_hash.py) cannot: the units differ.

    python tools/kernel_asm_diff.py PARENT_CSRC HEAD_CSRC [--units A.hip,B.hip ...] [--scratch DIR]

Every .hip of each tree (or only the named units; a name missing from one tree is skipped there) is compiled with
build.FLAGS plus `-S --cuda-device-only`.  Each .s is cut into functions, from the line that carries `; -- Begin function SYM`
through `; -- End function` and the `.set SYM.num_vgpr ...` lines behind it; the .amdhsa_kernel descriptor lies inside
that range.  Within a
function the unit-local ordinal is rewritten (.LBB<k>_ -> .LBB_, .Lfunc_end<k> -> .Lfunc_end), comments (whole lines, and the
trailing ones, which repeat the ordinal as "Header=BB<k>_6") and lines with .ident, .file or __hip_cuid_ are dropped, and the rest is compared as text, keyed by symbol.  Prints one row
per kernel: symbol, unit(s), lines compared, diff lines, and vgpr / sgpr / scratch / LDS of both sides; then the symbols
that exist on one side only or more than once.  Exit status 1 if anything differs.  Needs no GPU.
"""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
import build  # noqa: E402

BEGIN = re.compile(r"; -- Begin function (\S+)")
END = re.compile(r"^\s*; -- End function")
DROP = re.compile(r"\.ident|\.file|__hip_cuid_")
ORDINAL = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_end\d+"), ".Lfunc_end")]
RESOURCES = [("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
             ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size")]


def compile_unit(csrc: str, unit: str, out: str) -> str:
    asm = os.path.join(out, unit.replace(".hip", ".s"))
    subprocess.run([build.HIPCC, *build.FLAGS, "-S", "--cuda-device-only", os.path.join(csrc, unit), "-o", asm], check=True,
                   capture_output=True)
    return asm


def functions(asm: str):
    """{symbol: filtered lines} of one .s file."""
    found, name, body, ended = {}, None, [], False
    for line in open(asm):
        m = BEGIN.search(line)
        if m:
            name, body, ended = m.group(1), [], False
            found[name] = body
        elif name and END.match(line):
            ended = True
            continue
        elif name and ended and not line.lstrip().startswith(".set " + name + "."):
            name = None  # past the function's resource symbols
        if name and not line.lstrip().startswith(";") and line.strip() and not DROP.search(line):
            if '"' not in line:
                line = line.split(";", 1)[0]  # trailing comment: "in Loop: Header=BB<k>_6", padded to a column
            for pat, to in ORDINAL:
                line = pat.sub(to, line)
            body.append(line.rstrip())
    return found


def resources(body) -> str:
    vals = []
    for label, key in RESOURCES:
        hit = [ln.split()[-1] for ln in body if ln.split()[0] == key]
        vals.append(f"{label}={hit[0] if hit else '?'}")
    return " ".join(vals)


def kernels(csrc: str, units, out: str):
    """{symbol: [(unit, lines), ...]} of the kernels (functions with an .amdhsa_kernel block) of a tree."""
    units = [u for u in units if os.path.exists(os.path.join(csrc, u))]
    os.makedirs(out, exist_ok=True)
    with ThreadPoolExecutor(max_workers=6) as ex:
        asms = list(ex.map(lambda u: compile_unit(csrc, u, out), units))
    table = {}
    for unit, asm in zip(units, asms):
        for sym, body in functions(asm).items():
            if any(ln.lstrip().startswith(".amdhsa_kernel") for ln in body):
                table.setdefault(sym, []).append((unit, body))
    return table


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_csrc")
    ap.add_argument("head_csrc")
    ap.add_argument("--units", default="", help="comma-separated unit names; default: every .hip of either tree")
    ap.add_argument("--scratch", default=None)
    ap.add_argument("--show", action="store_true", help="print the differing lines of every kernel that differs")
    args = ap.parse_args()
    units = [u for u in args.units.split(",") if u] or sorted(
        {os.path.basename(p) for d in (args.parent_csrc, args.head_csrc) for p in glob.glob(os.path.join(d, "*.hip"))})
    scratch = args.scratch or tempfile.mkdtemp(prefix="kernel_asm_diff_")
    parent = kernels(args.parent_csrc, units, os.path.join(scratch, "parent"))
    head = kernels(args.head_csrc, units, os.path.join(scratch, "head"))

    bad = 0
    print(f"{'symbol':<100} {'parent unit':<18} {'head unit':<18} {'lines':>6} {'diff':>5}  parent resources | head resources")
    for sym in sorted(set(parent) & set(head)):
        (pu, pb), (hu, hb) = parent[sym][0], head[sym][0]
        ndiff = sum(1 for ln in difflib.unified_diff(pb, hb, lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---"))
        bad += ndiff != 0
        print(f"{sym:<100} {pu:<18} {hu:<18} {len(pb):>6} {ndiff:>5}  {resources(pb)} | {resources(hb)}")
        if ndiff and args.show:
            print("\n".join(difflib.unified_diff(pb, hb, "parent", "head", lineterm="", n=1)))
    for label, a, b in (("parent", parent, head), ("head", head, parent)):
        for sym in sorted(set(a) - set(b)):
            bad += 1
            print(f"only in {label}: {sym} ({a[sym][0][0]})")
        for sym, where in sorted(a.items()):
            if len(where) > 1:
                bad += 1
                print(f"more than once in {label}: {sym} ({', '.join(u for u, _ in where)})")
    print(f"kernels: parent {len(parent)}, head {len(head)}, common {len(set(parent) & set(head))}; "
          f"{'all identical' if not bad else str(bad) + ' problem(s)'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

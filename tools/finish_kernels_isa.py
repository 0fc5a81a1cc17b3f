#!/usr/bin/env python3
"""The checked finishes' kernels of two trees, compared on their gfx950 code - no GPU needed.

    tools/finish_kernels_isa.py --parent-csrc <parent checkout>/sda_amd/csrc [--out profiles/r21/finish_kernels_isa.txt]

Compiles sda_kernels.hip of the parent tree and of this tree to assembly (device side only, the flags of __graft_entry__.build) and
records, per kernel, the instruction count, VGPRs, SGPRs, LDS and scratch bytes from the compiler's resource report, and whether the
instruction streams are the same text.  The three existing finish kernels and the erasure setup kernel must be identical in both
trees (exit status 1 otherwise); the unmasking kernels exist in this tree only and must use no scratch."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

EXISTING = ("reveal_check_finish_kernel", "reveal_decode_finish_kernel", "reveal_erasure_setup_kernel", "reveal_erasure_finish_kernel")
NEW = ("reveal_check_unmask_kernel", "reveal_decode_unmask_kernel")
FIELDS = (("VGPRs", ".vgpr_count"), ("SGPRs", ".sgpr_count"), ("LDS bytes", ".group_segment_fixed_size"),
          ("scratch bytes", ".private_segment_fixed_size"), ("spilled VGPRs", ".vgpr_spill_count"), ("spilled SGPRs", ".sgpr_spill_count"))


def assembly(csrc):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "sda_kernels.s")
        subprocess.run([ge.HIPCC] + ge.FLAGS + ["-S", "--cuda-device-only", "-I", os.path.join(os.path.dirname(os.path.dirname(csrc)), "include"),
                        "-o", out, os.path.join(csrc, "sda_kernels.hip")], check=True, cwd=tmp, timeout=1800)
        return open(out).read().split("\n")


def kernels(lines, names):
    """mangled symbol -> (instructions as text, resource fields) of every kernel whose name contains one of `names`"""
    found = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if not m or not any(n in m.group(1) for n in names):
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        # a label carries the number of its function in the file, which moves when a kernel is added above: not part of the code
        body = [re.sub(r"\.(LBB|LJTI|LCPI|Ltmp)\d+_", r".\1_", x.split(";")[0].strip()) for x in lines[i + 1:end]]
        found[m.group(1)] = [x for x in body if x and not x.startswith(".") and not x.endswith(":")]
    meta = {}
    for i, l in enumerate(lines):                                  # the amdhsa.kernels metadata: one block per kernel, .name inside
        m = re.match(r"^\s+\.name:\s+(\S+)", l)
        if m and m.group(1) in found:
            lo = max(j for j in range(i, -1, -1) if lines[j].lstrip().startswith("- .agpr_count") or lines[j].lstrip().startswith("- .args"))
            hi = next(j for j in range(i + 1, len(lines)) if lines[j].lstrip().startswith("- .") or lines[j].startswith("amdhsa."))
            block = "\n".join(lines[lo:hi])
            meta[m.group(1)] = {key: int(re.search(re.escape(key) + r":\s+(\d+)", block).group(1)) for _, key in FIELDS}
    return {sym: (found[sym], meta[sym]) for sym in found}


def row(sym, code, res):
    return f"  {sym}\n      instructions {len(code)}, " + ", ".join(f"{title} {res[key]}" for title, key in FIELDS)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-csrc", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "finish_kernels_isa.txt"))
    a = ap.parse_args()
    parent = kernels(assembly(os.path.abspath(a.parent_csrc)), EXISTING)
    asm = assembly(ge.CSRC)
    mine, new = kernels(asm, EXISTING), kernels(asm, NEW)
    text = ["The kernels of the checked finishes, parent commit against this tree: gfx950 code from hipcc " + " ".join(ge.FLAGS) +
            " -S --cuda-device-only, sda_kernels.hip;", "the figures are the compiler's resource report (amdhsa.kernels), the instructions "
            "are counted and compared as text.", ""]
    ok = set(parent) == set(mine) and len(mine) == len(EXISTING)
    for sym in sorted(parent):
        same = sym in mine and parent[sym] == mine[sym]
        ok = ok and same
        text += ["parent " + row(sym, *parent[sym]).strip(), "tree   " + (row(sym, *mine[sym]).strip() if sym in mine else "MISSING"),
                 "  -> " + ("identical: every instruction and every figure" if same else "DIFFERENT"), ""]
    text += ["The unmasking kernels (this tree only):"]
    for sym in sorted(new):
        text.append(row(sym, *new[sym]))
        ok = ok and new[sym][1][".private_segment_fixed_size"] == 0 and new[sym][1][".vgpr_spill_count"] == 0
    ok = ok and len(new) == 3
    text += ["", "existing kernels identical and no scratch in the new ones: " + ("yes" if ok else "NO")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The checked finishes' kernels of two trees, compared on their gfx950 code - no GPU needed.

    tools/finish_kernels_isa.py --parent-csrc <parent checkout>/sda_amd/csrc [--out profiles/r22/finish_kernels_isa.txt] [--dump DIR]

Compiles sda_kernels.hip of the parent tree and of this tree to assembly (device side only, the flags of __graft_entry__.build) and
records, per kernel and side, the instruction count, VGPRs, SGPRs, LDS and scratch bytes from the compiler's resource report, and
whether the instruction streams are the same text.  Kernels are matched by name, whatever their argument types.  Exit status 0
when the tree keeps the parent's footing: reveal_erasure_setup_kernel identical, and each of the six finish kernels with no
scratch, no spilled VGPR, no more spilled SGPRs than the parent, the parent's LDS bytes and no more VGPRs than the parent once
both are rounded up to the allocation granule of 8 (= the parent's waves per SIMD).  Instruction counts are recorded, not
bounded.  --dump DIR leaves <kernel>.{parent,tree}.s there, the instruction text to diff when a leg of
tools/bench_checked_ends_parent_vs_tree.py misses."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

SETUP = "reveal_erasure_setup_kernel"
FINISHES = ("reveal_check_finish_kernel", "reveal_decode_finish_kernel", "reveal_erasure_finish_kernel", "reveal_check_unmask_kernel",
            "reveal_decode_unmask_kernel<false>", "reveal_decode_unmask_kernel<true>")
FIELDS = (("VGPRs", ".vgpr_count"), ("SGPRs", ".sgpr_count"), ("LDS bytes", ".group_segment_fixed_size"),
          ("scratch bytes", ".private_segment_fixed_size"), ("spilled VGPRs", ".vgpr_spill_count"), ("spilled SGPRs", ".sgpr_spill_count"))
GRANULE = 8                                                        # VGPRs are allocated in eights on gfx950 (512 per SIMD lane)


def assembly(csrc):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "sda_kernels.s")
        subprocess.run([ge.HIPCC] + ge.FLAGS + ["-S", "--cuda-device-only", "-I", os.path.join(os.path.dirname(os.path.dirname(csrc)), "include"),
                        "-o", out, os.path.join(csrc, "sda_kernels.hip")], check=True, cwd=tmp, timeout=1800)
        return open(out).read().split("\n")


def kernel_name(symbol):
    """reveal_check_finish_kernel, reveal_decode_unmask_kernel<true> ... of a mangled symbol, None for any other"""
    m = re.match(r"^_ZN3sda\d+(reveal_\w+?_kernel)(?:ILb([01])EE)?", symbol)
    if not m:
        return None
    name = m.group(1) + ({"0": "<false>", "1": "<true>"}[m.group(2)] if m.group(2) else "")
    return name if name == SETUP or name in FINISHES else None


def kernels(lines):
    """kernel name -> (instructions as text, resource fields) of the family's kernels"""
    found, symbol_of = {}, {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        name = kernel_name(m.group(1)) if m else None
        if not name:
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        # a label carries the number of its function in the file, which moves when a kernel is added above: not part of the code
        body = [re.sub(r"\.(LBB|LJTI|LCPI|Ltmp)\d+_", r".\1_", x.split(";")[0].strip()) for x in lines[i + 1:end]]
        found[name] = [x for x in body if x and not x.startswith(".") and not x.endswith(":")]
        symbol_of[m.group(1)] = name
    meta = {}
    for i, l in enumerate(lines):                                  # the amdhsa.kernels metadata: one block per kernel, .name inside
        m = re.match(r"^\s+\.name:\s+(\S+)", l)
        if m and m.group(1) in symbol_of:
            lo = max(j for j in range(i, -1, -1) if lines[j].lstrip().startswith("- .agpr_count") or lines[j].lstrip().startswith("- .args"))
            hi = next(j for j in range(i + 1, len(lines)) if lines[j].lstrip().startswith("- .") or lines[j].startswith("amdhsa."))
            block = "\n".join(lines[lo:hi])
            meta[symbol_of[m.group(1)]] = {key: int(re.search(re.escape(key) + r":\s+(\d+)", block).group(1)) for _, key in FIELDS}
    return {name: (found[name], meta[name]) for name in found}


def row(side, code, res):
    return f"  {side:6} instructions {len(code)}, " + ", ".join(f"{title} {res[key]}" for title, key in FIELDS)


def granules(n):
    return (n + GRANULE - 1) // GRANULE * GRANULE


def misses(parent, tree):
    """the structural conditions a finish kernel of the tree fails against the parent's, as text (empty: none)"""
    bad = []
    if tree[".private_segment_fixed_size"] != 0:
        bad.append("scratch")
    if tree[".vgpr_spill_count"] != 0:
        bad.append("spilled VGPRs")
    if tree[".sgpr_spill_count"] > parent[".sgpr_spill_count"]:
        bad.append("more spilled SGPRs")
    if tree[".group_segment_fixed_size"] != parent[".group_segment_fixed_size"]:
        bad.append("other LDS bytes")
    if granules(tree[".vgpr_count"]) > granules(parent[".vgpr_count"]):
        bad.append(f"VGPRs {granules(tree['.vgpr_count'])} > {granules(parent['.vgpr_count'])} allocated")
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-csrc", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "finish_kernels_isa.txt"))
    ap.add_argument("--dump", help="directory for the kernels' instruction text, <kernel>.{parent,tree}.s")
    a = ap.parse_args()
    parent, tree = kernels(assembly(os.path.abspath(a.parent_csrc))), kernels(assembly(ge.CSRC))
    text = ["The kernels of the checked finishes, parent commit against this tree: gfx950 code from hipcc " + " ".join(ge.FLAGS) +
            " -S --cuda-device-only, sda_kernels.hip;", "the figures are the compiler's resource report (amdhsa.kernels), the instructions "
            "are counted and compared as text.", ""]
    ok = True
    for name in (SETUP,) + FINISHES:
        if name not in parent or name not in tree:
            text += [name, "  MISSING in " + ("the parent" if name not in parent else "the tree"), ""]
            ok = False
            continue
        same = parent[name][0] == tree[name][0]
        bad = ([] if same else ["not identical"]) if name == SETUP else misses(parent[name][1], tree[name][1])
        ok = ok and not bad
        text += [name, row("parent", *parent[name]), row("tree", *tree[name]),
                 "  -> instructions " + ("identical" if same else "differ") + "; " + ("MISSES: " + ", ".join(bad) if bad else "conditions met"), ""]
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            for side, k in (("parent", parent), ("tree", tree)):
                with open(os.path.join(a.dump, re.sub(r"\W", "_", name) + f".{side}.s"), "w") as f:
                    f.write("\n".join(k[name][0]) + "\n")
    text += ["setup kernel identical; finishes without scratch or spilled VGPRs, SGPR spills and allocated VGPRs not above the parent's, "
             "LDS bytes the parent's: " + ("yes" if ok else "NO")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

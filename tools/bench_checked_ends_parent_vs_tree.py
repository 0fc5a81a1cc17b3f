#!/usr/bin/env python3
"""The three ends of the checked reveal, the parent commit's library against this tree's: the same entry points on both, since the
tree only rebuilds the five finish kernels from shared pieces and the four launchers as one.  Per end (locate, decode, erasures),
SDA_CHECK_CORRECT, max_errors = 0:
    F/parent, F/tree  the named finish alone (finish_checked_dev, finish_decoded_dev, finish_erasures_dev)
    U/parent, U/tree  sda_secret_unmasker_unmask_checked_jobs_dev
Shapes, dimension 1 Mi over the 62-bit prime: config3 (k = 3, t = 1, n = 8, 4 checks) and config4 (k = 8, t = 2, n = 26, 16 checks)
with a Full mask (4 participants), and config3 with no mask (a None unmasker, NULL combiner: the kernels' own path).  Row sets per
end: clean rows; one faulty row; for the erasure end also one refused row (zeros, flagged in d_ok).  Both jobs are filled by
plaintext update_dev calls OUTSIDE the timed region; timed: the host clock around the call and a device synchronise.  The four legs
are interleaved in one process (both libraries sit on the one HIP runtime), the order rotates, 3 warm-up rounds, REPS >= 20 timed;
median with (min - max), spread = max - min.  Every tree leg's output and report must equal the parent leg's word for word.
The criterion is bench_recipient_unmask_checked.compare: a tree leg's median is not above the parent leg's by more than the larger
of the two legs' spreads.  Exit status 1 when a leg misses it or differs.  Every shape is a child process under its own time
limit; a child that fails or runs out of time ends the whole measurement.
Writes checked_ends_parent_vs_tree.json / .txt into --out-dir (default profiles/r22).  DIMENSION / REPS override the shape."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_recipient_unmask_checked import CONFIGS, compare  # noqa: E402

SHAPES = ["config3-full", "config4-full", "config3-none"]
ROWS = [("locate", "clean"), ("locate", "faulty1"), ("decode", "clean"), ("decode", "faulty1"), ("erasures", "clean"), ("erasures", "faulty1"),
        ("erasures", "refused1")]
LEGS = ["F/parent", "F/tree", "U/parent", "U/tree"]
NAME = "checked_ends_parent_vs_tree"


def child(shape, parent_path):
    import numpy as np
    from bench_recipient_reveal_erasures import ParentLibrary
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    config, masking = shape.split("-")
    (p, k, t, n, w2, w3), checks = CONFIGS[config]
    dim, reps = int(os.environ.get("DIMENSION", str(1 << 20))), max(20, int(os.environ.get("REPS", "20")))
    lib = capi.load()
    parent = ParentLibrary(parent_path)
    assert parent.lib.sda_build_id() != lib.sda_build_id(), "--parent-lib is this tree's library"
    B = -(-dim // k)
    indices = list(range(n))
    sharing = crypto.PackedShamir(k, n, t, p, w2, w3)
    msch = crypto.Full(p) if masking == "full" else crypto.NoMask()
    gen = crypto.ShareGenerator(sharing)
    gen.set_drbg_key(bytes(range(32)))
    rng = np.random.default_rng(n)
    sums = None
    for q in range(2):                                            # the clerk sums of two participants' shares
        sh = np.asarray(gen.generate(rng.integers(0, p, size=dim, dtype=np.int64)), dtype=np.int64)
        sums = sh if sums is None else ((sums.astype(np.uint64) + sh.astype(np.uint64)) % np.uint64(p)).astype(np.int64)
    liar, refused = int(rng.integers(0, n)), int(rng.integers(0, n))
    rows = {"clean": sums, "faulty1": sums.copy(), "refused1": sums.copy()}
    rows["faulty1"][liar] = ((sums[liar].astype(np.uint64) + np.uint64(12345)) % np.uint64(p)).astype(np.int64)
    rows["refused1"][refused] = 0                                 # a refused box adds nothing
    ok = np.ones(n, dtype="<u4")
    d_ones = DeviceBytes.from_bytes(ok.tobytes())
    ok[refused] = 0
    d_flags = DeviceBytes.from_bytes(ok.tobytes())
    d_rows = {which: DeviceBuffer.from_numpy(v) for which, v in rows.items()}
    if masking == "full":
        d_masks = DeviceBuffer(4 * dim)
        capi.check(lib.sda_fill_synthetic_dev(d_masks.ptr, 4, dim, dim, 100, 18, p, None))
    synchronize()

    def objects(made):                                            # unmasker, mask combiner (None without a mask), reconstructor
        return (made(lambda: crypto.SecretUnmasker(msch)), made(lambda: crypto.MaskCombiner(msch)) if masking == "full" else None,
                made(lambda: crypto.SecretReconstructor(sharing, dim)))
    sides = {"tree": objects(lambda make: make()), "parent": objects(parent.made)}
    d_out = {leg: DeviceBuffer(dim).zero() for leg in LEGS}
    d_report = {leg: DeviceBuffer(16 + n).zero() for leg in LEGS}
    ends = {"locate": capi.CHECKED_END_LOCATE, "decode": capi.CHECKED_END_DECODE, "erasures": capi.CHECKED_END_ERASURES}
    kernels = {}

    def run(leg, end, which):
        """-> the milliseconds of the leg's timed call"""
        form, side = leg.split("/")
        unm, comb, rec = sides[side]
        d_ok = (d_flags if which == "refused1" else d_ones).ptr
        rec.begin_checked_dev(indices, n, B, checks)
        rec.update_dev(0, d_rows[which].ptr, n, B)
        if form == "U" and comb is not None:
            comb.begin_dev(dim)
            comb.update_dev(d_masks.ptr, 4, dim, dim)
        synchronize()
        parent.synchronize()
        out, report = d_out[leg].ptr, d_report[leg].ptr
        t0 = time.perf_counter()
        if form == "U":
            unm.unmask_checked_jobs_dev(comb, rec, ends[end], out, dim, report, d_ok if end == "erasures" else 0, 0, True)
        elif end == "locate":
            rec.finish_checked_dev(out, dim, report, True)
        elif end == "decode":
            rec.finish_decoded_dev(out, dim, report, 0, True)
        else:
            rec.finish_erasures_dev(d_ok, out, dim, report, 0, True)
        synchronize()
        parent.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if side == "tree":
            kernels[form] = lib.sda_debug_last_kernel().decode()
        return ms
    res = {"shape": shape, "masking": masking, "rows": n, "k": k, "t": t, "checks": checks, "dimension": dim, "batches": B, "reps": reps,
           "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(),
           "parent_version": parent.lib.sda_version().decode(), "parent_kernel_id": parent.lib.sda_kernel_id().decode(),
           "faulty_position": liar, "refused_position": refused, "sets": {}}
    for end, which in ROWS:
        ms = {leg: [] for leg in LEGS}
        for rep in range(-3, reps):                               # three warm-up rounds
            for leg in LEGS[rep % len(LEGS):] + LEGS[:rep % len(LEGS)]:       # the legs are interleaved, the order rotates
                v = run(leg, end, which)
                if rep >= 0:
                    ms[leg].append(v)
        got = {leg: (d_out[leg].to_numpy(), d_report[leg].to_numpy()[:(4 if end == "locate" else 16) + n]) for leg in LEGS}
        entry = {"kernels": dict(kernels), "report_head": [int(x) for x in got["F/tree"][1].view(np.uint64)[:8]], "legs": {}}
        for form in ("F", "U"):
            a, b = got[form + "/parent"], got[form + "/tree"]
            entry[form + "_tree_equals_parent"] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
        entry["in_range_and_not_constant"] = all(bool(((got[leg][0] >= 0) & (got[leg][0] < p)).all()) and len(set(got[leg][0][:64].tolist())) > 32
                                                 for leg in LEGS)
        for leg in LEGS:
            v = sorted(ms[leg])
            entry["legs"][leg] = {"median_ms": (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, "min_ms": v[0], "max_ms": v[-1]}
        res["sets"][f"{end}/{which}"] = entry
    for obj in sides["parent"]:
        if obj is not None:
            obj.close()
    print("RESULT " + json.dumps(res))


def run_child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        raise SystemExit(f"child {args} ended with status {r.returncode}: nothing more is started")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def report(res):
    """-> (the text, the legs that miss the criterion or differ from the parent's)"""
    lines = ["the ends of the checked reveal, parent commit's library against this tree's; dimension 1 Mi unless DIMENSION says otherwise; host",
             "clock around the call + synchronise, jobs filled outside the timed region, legs interleaved in one process (rotating order), 3",
             "warm-up rounds; SDA_CHECK_CORRECT, max_errors = 0; median ms (min - max)",
             "F = the named finish alone; U = sda_secret_unmasker_unmask_checked_jobs_dev",
             "criterion: a tree leg's median is not above the parent leg's by more than the larger of the two legs' spreads (max - min)", ""]
    missed = []
    for shape, r in res.items():
        lines.append(f"[{shape}] {r['rows']} rows, k = {r['k']}, t = {r['t']}, checks = {r['checks']}, {r['masking']} mask, dimension {r['dimension']} "
                     f"({r['batches']} batches), {r['reps']} repetitions; {r['version']} kernel id {r['kernel_id']}; parent {r['parent_version']} "
                     f"kernel id {r['parent_kernel_id']}")
        for name, e in r["sets"].items():
            L = e["legs"]
            lines.append(f"  {name:20s} " + "  ".join(f"{leg} {L[leg]['median_ms']:.3f} ({L[leg]['min_ms']:.3f} - {L[leg]['max_ms']:.3f})" for leg in LEGS))
            for form in ("F", "U"):
                ok, text = compare(L[form + "/parent"], L[form + "/tree"])
                same = e[form + "_tree_equals_parent"] and e["in_range_and_not_constant"]
                lines.append(f"  {'':20s} {form} tree / parent = {text}{'' if ok else '  MISSES THE CRITERION'}; tree = parent word for word: "
                             f"{same}; ran {e['kernels'][form]}")
                if not (ok and same):
                    missed.append(f"{shape} {name} {form}")
            lines.append(f"  {'':20s} report {e['report_head']}")
        lines.append("")
    lines.append("legs on which the tree's median is above the parent's by more than the larger spread, or whose words differ: " +
                 (", ".join(missed) or "none"))
    return "\n".join(lines), missed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default=None, choices=SHAPES)
    ap.add_argument("--parent-lib", required=True, help="libsda_hip.so built from the parent commit")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r22"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.shape, a.parent_lib)
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, NAME + (f".{a.shape}" if a.shape else ""))   # a single shape (a second run of it) gets its own files
    res = {}
    for shape in ([a.shape] if a.shape else SHAPES):
        res[shape] = run_child(["--shape", shape, "--parent-lib", os.path.abspath(a.parent_lib)], a.limit)
        text, missed = report(res)
        with open(path + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(path + ".txt", "w") as f:
            f.write(text + "\n")
    print(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())

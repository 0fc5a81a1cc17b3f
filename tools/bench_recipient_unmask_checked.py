#!/usr/bin/env python3
"""The last step of the CHECKED reveal from the two device jobs' sums: the mask combiner's job and a checked reconstructor job are
filled, then, per end (locate = finish_checked_dev, decode = finish_decoded_dev, erasures = finish_erasures_dev), SDA_CHECK_CORRECT:
    A         the named finish -> d_masked, sda_mask_combiner_finish_dev -> d_mask, sda_secret_unmasker_unmask_dev -> d_out
              (the three-call chain with its two intermediate buffers, on the PARENT commit's library, --parent-lib)
    B         sda_secret_unmasker_unmask_checked_jobs_dev                                   (the one call, this tree)
    F/parent  the named finish alone on the parent commit's library
    F/tree    the named finish alone on this tree: the three existing kernels compile to the same code (profiles/r21/
              finish_kernels_isa.txt), so these two must not differ beyond their spread
Shapes, dimension 1 Mi over the 62-bit prime: config3 (k = 3, t = 1, n = 8, 4 checks) and config4 (k = 8, t = 2, n = 26, 16 checks),
each with a Full mask (4 participants) and a ChaCha mask (4 seeds).  Row sets per end: clean rows; one faulty row; for the erasure end
also one and `checks` refused rows (zeros, flagged in d_ok).  Both jobs are filled by plaintext update_dev calls OUTSIDE the timed
region; timed: the host clock around the call(s) and a device synchronise.  The legs are interleaved in one process (both libraries
sit on the one HIP runtime), the order rotates, 3 warm-up rounds, REPS >= 20 timed; median with (min - max), spread = max - min.
B's output and report are compared with A's, word for word.  Every shape is a child process under its own time limit; a child that
fails or runs out of time ends the whole measurement.
Writes recipient_unmask_checked.json / .txt into --out-dir (default profiles/r21).  DIMENSION / REPS override the shape."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
P62 = 4611686006577364993
CONFIGS = {"config3": ((P62, 3, 1, 8, 631229665360524489, 3451275676410824977), 4),
           "config4": ((P62, 8, 2, 26, 2589100645267092065, 365137883145458390), 16)}
SHAPES = [f"{c}-{m}" for c in CONFIGS for m in ("full", "chacha")]
ROWS = [("locate", "clean"), ("locate", "faulty1"), ("decode", "clean"), ("decode", "faulty1"), ("erasures", "clean"), ("erasures", "faulty1"),
        ("erasures", "refused1"), ("erasures", "refused-checks")]
LEGS = ["A", "B", "F/parent", "F/tree"]
NEW = "sda_secret_unmasker_unmask_checked_jobs_dev"


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
    assert not hasattr(parent.lib, NEW), "--parent-lib is not the parent's library"
    B = -(-dim // k)
    indices = list(range(n))
    sharing = crypto.PackedShamir(k, n, t, p, w2, w3)
    msch = crypto.Full(p) if masking == "full" else crypto.ChaCha(p, dim, 128)
    gen = crypto.ShareGenerator(sharing)
    gen.set_drbg_key(bytes(range(32)))
    rng = np.random.default_rng(n)
    sums = None
    for q in range(2):                                            # the clerk sums of two participants' shares
        sh = np.asarray(gen.generate(rng.integers(0, p, size=dim, dtype=np.int64)), dtype=np.int64)
        sums = sh if sums is None else ((sums.astype(np.uint64) + sh.astype(np.uint64)) % np.uint64(p)).astype(np.int64)
    liar = int(rng.integers(0, n))
    refused = {"refused1": [int(rng.integers(0, n))], "refused-checks": sorted(int(i) for i in rng.permutation(n)[:checks])}
    rows, flags = {"clean": sums}, {"clean": None, "faulty1": None}
    rows["faulty1"] = sums.copy()
    rows["faulty1"][liar] = ((sums[liar].astype(np.uint64) + np.uint64(12345)) % np.uint64(p)).astype(np.int64)
    for which, erased in refused.items():
        rows[which] = sums.copy()
        rows[which][erased] = 0                                   # a refused box adds nothing
        ok = np.ones(n, dtype="<u4")
        ok[erased] = 0
        flags[which] = DeviceBytes.from_bytes(ok.tobytes())
    d_ones = DeviceBytes.from_bytes(np.ones(n, dtype="<u4").tobytes())
    d_rows = {which: DeviceBuffer.from_numpy(v) for which, v in rows.items()}
    if masking == "full":
        mask_rows, mask_width = 4, dim
        d_masks = DeviceBuffer(mask_rows * dim)
        capi.check(lib.sda_fill_synthetic_dev(d_masks.ptr, mask_rows, dim, dim, 100, 18, p, None))
    else:
        mask_rows, mask_width = 4, 4
        d_masks = DeviceBuffer.from_numpy(np.random.default_rng(19).integers(0, 1 << 32, size=(4, 4), dtype=np.int64))
    synchronize()

    new = (crypto.SecretUnmasker(msch), crypto.MaskCombiner(msch), crypto.SecretReconstructor(sharing, dim))
    old = (parent.made(lambda: crypto.SecretUnmasker(msch)), parent.made(lambda: crypto.MaskCombiner(msch)),
           parent.made(lambda: crypto.SecretReconstructor(sharing, dim)))
    words = 16 + n
    d_masked, d_mask = DeviceBuffer(dim), DeviceBuffer(dim)       # leg A's two intermediate buffers
    d_out = {leg: DeviceBuffer(dim).zero() for leg in LEGS}
    d_report = {leg: DeviceBuffer(words).zero() for leg in LEGS}
    ends = {"locate": capi.CHECKED_END_LOCATE, "decode": capi.CHECKED_END_DECODE, "erasures": capi.CHECKED_END_ERASURES}
    kernels = {}

    def ok_ptr(which):
        return (flags[which] if flags[which] is not None else d_ones).ptr

    def finish(rec, end, which, out, report):
        if end == "locate":
            rec.finish_checked_dev(out, dim, report, True)
        elif end == "decode":
            rec.finish_decoded_dev(out, dim, report, 0, True)
        else:
            rec.finish_erasures_dev(ok_ptr(which), out, dim, report, 0, True)

    def run(leg, end, which):
        """-> the milliseconds of the leg's timed unit"""
        unm, comb, rec = old if leg in ("A", "F/parent") else new
        rec.begin_checked_dev(indices, n, B, checks)
        rec.update_dev(0, d_rows[which].ptr, n, B)
        if leg in ("A", "B"):
            comb.begin_dev(dim)
            comb.update_dev(d_masks.ptr, mask_rows, mask_width, mask_width)
        synchronize()
        parent.synchronize()
        out, report = d_out[leg].ptr, d_report[leg].ptr
        t0 = time.perf_counter()
        if leg == "A":
            finish(rec, end, which, d_masked.ptr, report)
            comb.finish_dev(d_mask.ptr, dim)
            unm.unmask_dev(d_mask.ptr, d_masked.ptr, dim, out)
        elif leg == "B":
            unm.unmask_checked_jobs_dev(comb, rec, ends[end], out, dim, report, ok_ptr(which) if end == "erasures" else 0, 0, True)
        else:
            finish(rec, end, which, out, report)
        synchronize()
        parent.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if leg == "B":
            kernels[end] = lib.sda_debug_last_kernel().decode()
        return ms
    res = {"shape": shape, "masking": masking, "rows": n, "k": k, "t": t, "checks": checks, "dimension": dim, "batches": B, "reps": reps,
           "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(),
           "parent_version": parent.lib.sda_version().decode(), "parent_kernel_id": parent.lib.sda_kernel_id().decode(),
           "faulty_position": liar, "refused_positions": refused, "sets": {}}
    for end, which in ROWS:
        ms = {leg: [] for leg in LEGS}
        for rep in range(-3, reps):                               # three warm-up rounds
            order = LEGS[rep % len(LEGS):] + LEGS[:rep % len(LEGS)]           # the legs are interleaved, the order rotates
            for leg in order:
                v = run(leg, end, which)
                if rep >= 0:
                    ms[leg].append(v)
        got = {leg: (d_out[leg].to_numpy(), d_report[leg].to_numpy()[:(4 if end == "locate" else 16) + n]) for leg in LEGS}
        entry = {"kernels_B": kernels[end], "report_head": [int(x) for x in got["B"][1].view(np.uint64)[:8]],
                 "B_equals_A": bool(np.array_equal(got["A"][0], got["B"][0]) and np.array_equal(got["A"][1], got["B"][1])),
                 "finish_tree_equals_parent": bool(np.array_equal(got["F/parent"][0], got["F/tree"][0]) and
                                                   np.array_equal(got["F/parent"][1], got["F/tree"][1])),
                 "B_in_range_and_not_constant": bool(((got["B"][0] >= 0) & (got["B"][0] < p)).all()) and len(set(got["B"][0][:64].tolist())) > 32,
                 "legs": {}}
        for leg in LEGS:
            v = sorted(ms[leg])
            entry["legs"][leg] = {"median_ms": (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, "min_ms": v[0], "max_ms": v[-1]}
        res["sets"][f"{end}/{which}"] = entry
    for obj in old:
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


def spread(v):
    return v["max_ms"] - v["min_ms"]


def compare(a, b):
    """the routing criterion: b's median is not above a's by more than the larger of the two spreads"""
    over, room = b["median_ms"] - a["median_ms"], max(spread(a), spread(b))
    return over <= room, f"{b['median_ms'] / a['median_ms']:.3f} (median {over:+.3f} ms, larger spread {room:.3f} ms)"


def report(res):
    lines = ["the last step of the checked reveal from the two device jobs' sums; dimension 1 Mi unless DIMENSION says otherwise; host clock around",
             "the call(s) + synchronise, jobs filled outside the timed region, legs interleaved in one process (rotating order), 3 warm-up",
             "rounds; SDA_CHECK_CORRECT, max_errors = 0; median ms (min - max)",
             "A = the named finish + mask combiner finish_dev + unmask_dev with two buffers of 8 L bytes, on the parent commit's library",
             "B = sda_secret_unmasker_unmask_checked_jobs_dev, this tree",
             "F = the named finish alone, parent commit's library / this tree", ""]
    slower, moved = [], []
    for shape, r in res.items():
        lines.append(f"[{shape}] {r['rows']} rows, k = {r['k']}, t = {r['t']}, checks = {r['checks']}, {r['masking']} mask, dimension {r['dimension']} "
                     f"({r['batches']} batches), {r['reps']} repetitions; {r['version']} kernel id {r['kernel_id']}; parent {r['parent_version']} "
                     f"kernel id {r['parent_kernel_id']}")
        for name, e in r["sets"].items():
            L = e["legs"]
            cells = "  ".join(f"{leg} {L[leg]['median_ms']:.3f} ({L[leg]['min_ms']:.3f} - {L[leg]['max_ms']:.3f})" for leg in LEGS)
            ok_b, text_b = compare(L["A"], L["B"])
            ok_f, text_f = compare(L["F/parent"], L["F/tree"])
            ok_g, _ = compare(L["F/tree"], L["F/parent"])
            lines.append(f"  {name:24s} {cells}")
            lines.append(f"  {'':24s} B / A = {text_b}{'' if ok_b else '  B IS SLOWER'};  F tree / parent = {text_f}"
                         f"{'' if ok_f and ok_g else '  BEYOND THE SPREAD'};  B = A word for word: {e['B_equals_A']}; F tree = parent: "
                         f"{e['finish_tree_equals_parent']}; report {e['report_head']}; B ran {e['kernels_B']}")
            if not ok_b:
                slower.append(f"{shape} {name}")
            if not (ok_f and ok_g):
                moved.append(f"{shape} {name}")
        lines.append("")
    lines.append("rows on which B's median is above A's by more than the larger spread: " + (", ".join(slower) or "none"))
    lines.append("rows on which the existing finish differs between the trees by more than the larger spread: " + (", ".join(moved) or "none"))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default=None, choices=SHAPES)
    ap.add_argument("--parent-lib", required=True, help="libsda_hip.so built from the parent commit: legs A and F/parent run on it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r21"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.shape, a.parent_lib)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {}
    for shape in ([a.shape] if a.shape else SHAPES):
        res[shape] = run_child(["--shape", shape, "--parent-lib", os.path.abspath(a.parent_lib)], a.limit)
        with open(os.path.join(a.out_dir, "recipient_unmask_checked.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "recipient_unmask_checked.txt"), "w") as f:
            f.write(report(res) + "\n")
    print(report(res))


if __name__ == "__main__":
    main()

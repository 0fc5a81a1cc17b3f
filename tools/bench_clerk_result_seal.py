#!/usr/bin/env python3
"""The clerk's last step (clerk.rs:84-100), device resident: the sums of a finished clerking job reduced, varint encoded and
sealed to the recipient.  JOBS jobs of VALUES columns (4 synthetic share rows each, uniform residues of the 62-bit prime) sit
in a combiner's 128-bit accumulators; three legs are timed with sda_event_*, ALTERNATED repetition by repetition in one process
(3 warm-up rounds, REPS >= 20 timed), OS-entropy ephemeral keys:
    A  sda_share_combiner_finish_dev + sda_sealedbox_seal_share_rows_dev (rows = jobs: one WAVE encodes and encrypts a result)
    B  sda_share_combiner_finish_dev + sda_varint_encode_dev (scan form) + sda_sealedbox_seal_rows_dev: parallel, through a
       plaintext result buffer and a plaintext wire buffer; with more than one job the scan form's contiguous rows do not fit
       seal_rows_dev's slots, so the encode and the seal run once per job
    C  sda_share_combiner_finish_sealed_rows_dev (every row split over the chip, no result buffer, no wire buffer)
After the timed rounds every leg runs once more into a wiped box buffer and the box of job 0 is opened with the Python oracle
(oracle/sealedbox_oracle.py), decoded and compared with finish_dev's sums.
Shapes: 1 x 349,526 (config 3's row), 1 x 5,592,406 (config 5's), 8 x 349,526; --shapes JOBSxVALUES,... overrides them.
Every shape is a child process under its own time limit; a child that fails or runs out of time ends the whole measurement.
Writes clerk_result_seal.json / .txt into --out-dir (default profiles/r12)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P62 = 4611686006577364993
SHAPES = "1x349526,1x5592406,8x349526"
FEED_ROWS = 4


def child(jobs, L, reps):
    import numpy as np
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    lib = capi.load()
    rows = DeviceBuffer(jobs * FEED_ROWS * L)
    capi.check(lib.sda_fill_synthetic_dev(rows.ptr, jobs * FEED_ROWS, L, L, 0, 0x5DA5DA5DA5DA5DA5, P62, None))
    comb = crypto.ShareCombiner(crypto.Additive(3, P62))
    comb.begin_dev(jobs, L)
    comb.update_dev(rows.ptr, FEED_ROWS * L, FEED_ROWS, L)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    vslot = codec.slot_size(L)
    bslot = vslot + 48
    sums = DeviceBuffer(jobs * L)
    wire, offs = DeviceBytes(jobs * vslot), DeviceBytes(jobs * 16).zero()
    boxes, blen = DeviceBytes(jobs * bslot), DeviceBytes(jobs * 8).zero()
    sk = bytes(range(1, 33))
    pk = box.public_key(sk)
    synchronize()

    def leg_a():
        comb.finish_dev(sums.ptr)
        box.seal_share_rows_dev(codec, [pk], jobs, sums.ptr, jobs, L, L, boxes.ptr, bslot, blen.ptr)

    def leg_b():
        comb.finish_dev(sums.ptr)
        for j in range(jobs):            # row j: offsets pair at offs + 16 j, its second word is the row's byte count
            codec.encode_dev(sums.at(j * L), 1, L, L, wire.ptr + j * vslot, vslot, offs.ptr + 16 * j)
            box.seal_rows_dev([pk], 1, wire.ptr + j * vslot, vslot, offs.ptr + 16 * j + 8, 1, vslot, boxes.ptr + j * bslot, bslot, blen.ptr + 8 * j)

    def leg_c():
        comb.finish_sealed_rows_dev(codec, box, pk, boxes.ptr, bslot, blen.ptr)

    fns = {"A": leg_a, "B": leg_b, "C": leg_c}

    def ev():
        e = C.c_void_p()
        capi.check(lib.sda_event_create(C.byref(e)))
        return e
    a, b = ev(), ev()
    ms = {k: [] for k in fns}
    for rep in range(-3, reps):                              # three warm-up rounds
        for k in fns:
            capi.check(lib.sda_event_record(a, None))
            fns[k]()
            capi.check(lib.sda_event_record(b, None))
            t = C.c_float()
            capi.check(lib.sda_event_elapsed_ms(a, b, C.byref(t)))
            if rep >= 0:
                ms[k].append(t.value)
    # every leg once more into a wiped box buffer: job 0's box must open to job 0's sums
    comb.finish_dev(sums.ptr)
    want = sums.to_numpy(L, 0)
    host = rows.to_numpy(FEED_ROWS * L, 0).reshape(FEED_ROWS, L)
    sums_ok = bool(np.array_equal(want, coracle.combine(P62, host)))
    verified, box_bytes, kernels = {}, 0, {}
    for k in fns:
        boxes.zero(); blen.zero()
        fns[k]()
        kernels[k] = lib.sda_debug_last_kernel().decode()
        lens = np.frombuffer(blen.to_bytes(), dtype="<u8")
        box_bytes = int(lens.sum())
        got = coracle.varint_decode(so.seal_open(boxes.to_bytes(int(lens[0]), 0), pk, sk))
        verified[k] = sums_ok and bool((lens > 48).all()) and bool(np.array_equal(got, want))
    out = {"library": os.path.relpath(capi.active_path(), ROOT), "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(),
           "jobs": jobs, "values": L, "reps": reps, "box_bytes_total": box_bytes, "kernels_of_C": kernels["C"], "legs": {}}
    for k in fns:
        v = sorted(ms[k])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        out["legs"][k] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "verified": verified[k]}
    print("RESULT " + json.dumps(out))


def run_child(shape, reps, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        raise SystemExit(f"child {shape} ended with status {r.returncode}: nothing more is started")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def verdict(r):
    """C against A: C's median below A's by more than the two legs' own min-to-max spreads together"""
    a, c = r["legs"]["A"], r["legs"]["C"]
    spread = (a["max_ms"] - a["min_ms"]) + (c["max_ms"] - c["min_ms"])
    return a["median_ms"] - c["median_ms"] > spread, spread


def report(res):
    lines = ["the clerk's last step: finish + encode + seal of a job's sums, legs alternated in one process, job 0's box of every leg opened with the oracle",
             "leg A = finish_dev + seal_share_rows_dev (one wave per result); B = finish_dev + varint_encode_dev + seal_rows_dev (per job); "
             "C = finish_sealed_rows_dev", ""]
    for shape, r in res.items():
        lines.append(f"[{r['jobs']} job(s) x {r['values']} values] {r['box_bytes_total'] / 1e6:.2f} MB of boxes, {r['reps']} timed repetitions per leg, "
                     f"{r['version']} kernel id {r['kernel_id']}")
        for k, v in r["legs"].items():
            lines.append(f"  {k}: median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  verified {v['verified']}")
        L = r["legs"]
        lines.append(f"  C ran: {r['kernels_of_C']}")
        lines.append(f"  C / A = {L['C']['median_ms'] / L['A']['median_ms']:.4f}   C / B = {L['C']['median_ms'] / L['B']['median_ms']:.4f}")
        if r["jobs"] == 1:
            ok, spread = verdict(r)
            lines.append(f"  criterion (one job): A - C = {L['A']['median_ms'] - L['C']['median_ms']:.3f} ms against the two legs' min-to-max spreads, {spread:.3f} ms together: "
                         f"{'met' if ok else 'NOT MET'}")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, metavar="JOBSxVALUES")
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r12"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        jobs, L = a.child.split("x")
        return child(int(jobs), int(L), max(20, a.reps))
    os.makedirs(a.out_dir, exist_ok=True)
    res = {}
    for shape in a.shapes.split(","):
        res[shape] = run_child(shape, a.reps, a.limit)
        with open(os.path.join(a.out_dir, "clerk_result_seal.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "clerk_result_seal.txt"), "w") as f:
            f.write(report(res))
    print(report(res))
    if not all(all(v["verified"] for v in r["legs"].values()) for r in res.values()):
        raise SystemExit("a leg's box did not open to the sums")


if __name__ == "__main__":
    main()

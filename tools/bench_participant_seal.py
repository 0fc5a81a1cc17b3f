#!/usr/bin/env python3
"""A participation's share rows into sealed boxes (participate.rs:82-101), device resident: the two-call sequence with its wire
buffer against the one-call form that has none.  ROWS share vectors of VALUES uniform residues of the 62-bit prime (default:
2000 x 349,526, config 3's row, about 6.3 GB of boxes) are sealed to one clerk key with OS-entropy ephemeral keys; four legs
are timed with sda_event_*, ALTERNATED repetition by repetition in one process (3 warm-up rounds, REPS >= 20 timed):
    A  sda_varint_encode_rows_dev + sda_sealedbox_seal_rows_dev
    B  sda_sealedbox_seal_share_rows_dev
    C  sda_sealedbox_seal_rows_dev alone, on the wire rows
    D  sda_varint_encode_rows_dev alone
After the timed rounds every leg that writes boxes runs once more and a sample of its boxes is opened (host form of
sda_sealedbox_open + varint decode) and compared with the share rows.
Every run is a child process under its own time limit; a child that fails or runs out of time ends the whole measurement.
    this tree, release library: A B C D         --parent-lib PATH: A, C and D again on a library built from the parent commit
Writes participant_seal_fused.json / .txt into --out-dir (default profiles/r08).  ROWS / VALUES / REPS override the job."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P62 = 4611686006577364993
NEW = "sda_sealedbox_seal_share_rows_dev"


def child(legs):
    import numpy as np
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    if "B" not in legs:
        capi.SIGNATURES.pop(NEW, None)                       # a library built from the parent commit does not have it
    lib = capi.load()
    P, L, reps = int(os.environ.get("ROWS", "2000")), int(os.environ.get("VALUES", "349526")), max(20, int(os.environ.get("REPS", "20")))
    shares = DeviceBuffer(P * L)
    capi.check(lib.sda_fill_synthetic_dev(shares.ptr, P, L, L, 0, 0x5DA5DA5DA5DA5DA5, P62, None))
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    vslot = codec.slot_size(L)
    bslot = vslot + 48
    wire, wlen = DeviceBytes(P * vslot), DeviceBytes(P * 8).zero()
    boxes, blen = DeviceBytes(P * bslot), DeviceBytes(P * 8).zero()
    sk = bytes(range(1, 33))
    pk = box.public_key(sk)
    codec.encode_rows_dev(shares.ptr, P, L, L, wire.ptr, vslot, wlen.ptr)          # legs C and D start from (and rewrite) these rows
    synchronize()

    def leg_a():
        codec.encode_rows_dev(shares.ptr, P, L, L, wire.ptr, vslot, wlen.ptr)
        box.seal_rows_dev([pk], P, wire.ptr, vslot, wlen.ptr, P, vslot, boxes.ptr, bslot, blen.ptr)

    def leg_b():
        box.seal_share_rows_dev(codec, [pk], P, shares.ptr, P, L, L, boxes.ptr, bslot, blen.ptr)

    def leg_c():
        box.seal_rows_dev([pk], P, wire.ptr, vslot, wlen.ptr, P, vslot, boxes.ptr, bslot, blen.ptr)

    def leg_d():
        codec.encode_rows_dev(shares.ptr, P, L, L, wire.ptr, vslot, wlen.ptr)

    fns = {"A": leg_a, "B": leg_b, "C": leg_c, "D": leg_d}

    def ev():
        e = C.c_void_p()
        capi.check(lib.sda_event_create(C.byref(e)))
        return e
    a, b = ev(), ev()
    ms = {k: [] for k in legs}
    for rep in range(-3, reps):                              # three warm-up rounds
        for k in legs:
            capi.check(lib.sda_event_record(a, None))
            fns[k]()
            capi.check(lib.sda_event_record(b, None))
            t = C.c_float()
            capi.check(lib.sda_event_elapsed_ms(a, b, C.byref(t)))
            if rep >= 0:
                ms[k].append(t.value)
    # every leg that seals, once more into a wiped box buffer: a sample of its boxes must open to the share rows
    sample = sorted({0, P // 3, P - 1})
    dec = crypto.ShareDecryptor(pk, sk)
    verified, box_bytes = {}, 0
    for k in legs:
        if k == "D":
            want = np.frombuffer(wlen.to_bytes(), dtype="<u8")
            fns[k]()
            verified[k] = bool(np.array_equal(np.frombuffer(wlen.to_bytes(), dtype="<u8"), want)) and all(
                np.array_equal(codec.decode(wire.to_bytes(int(want[r]), r * vslot)), shares.to_numpy(L, r * L)) for r in sample)
            continue
        boxes.zero(); blen.zero()
        fns[k]()
        lens = np.frombuffer(blen.to_bytes(), dtype="<u8")
        box_bytes = int(lens.sum())
        verified[k] = bool((lens > 48).all()) and all(
            np.array_equal(dec.decrypt(boxes.to_bytes(int(lens[r]), r * bslot)), shares.to_numpy(L, r * L)) for r in sample)
    out = {"library": os.path.basename(capi.active_path()) + " given with --parent-lib" if os.environ.get("SDA_HIP_LIBRARY") else os.path.relpath(capi.active_path(), ROOT), "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(),
           "rows": P, "values": L, "reps": reps, "box_bytes_total": box_bytes, "boxes_opened_per_leg": len(sample), "legs": {}}
    for k in legs:
        v = sorted(ms[k])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        out["legs"][k] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "box_GBps_at_median": box_bytes / (med * 1e-3) / 1e9,
                          "verified": verified[k]}
    if "B" in legs:
        fns["B"]()
        out["kernels_of_B"] = lib.sda_debug_last_kernel().decode()
    print("RESULT " + json.dumps(out))


def run_child(args, env_extra, limit):
    env = dict(os.environ, **env_extra)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        raise SystemExit(f"child {args} ended with status {r.returncode}: nothing more is started")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--legs", default="ABCD")
    ap.add_argument("--parent-lib", default=None, help="libsda_hip.so built from the parent commit: legs A, C and D on it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r08"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.legs)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"this_tree": run_child(["--legs", "ABCD"], {}, a.limit)}

    def save():
        with open(os.path.join(a.out_dir, "participant_seal_fused.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "participant_seal_fused.txt"), "w") as f:
            f.write(report(res))
    save()
    if a.parent_lib:
        res["parent_commit"] = run_child(["--legs", "ACD"], {"SDA_HIP_LIBRARY": os.path.abspath(a.parent_lib)}, a.limit)
        save()
    print(report(res))


def report(res):
    t = res["this_tree"]
    lines = [f"participation: {t['rows']} share rows x {t['values']} values, {t['box_bytes_total'] / 1e9:.2f} GB of boxes, {t['reps']} timed repetitions per leg (legs alternated), "
             f"{t['boxes_opened_per_leg']} boxes of every leg opened and compared",
             "leg A = encode_rows_dev + seal_rows_dev; B = seal_share_rows_dev; C = seal_rows_dev alone; D = encode_rows_dev alone", ""]
    for name, r in res.items():
        lines.append(f"[{name}] {r['version']} kernel id {r['kernel_id']}")
        for k, v in r["legs"].items():
            lines.append(f"  {k}: median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  {v['box_GBps_at_median']:.0f} GB/s of box bytes  verified {v['verified']}")
        if r.get("kernels_of_B"):
            lines.append(f"  B ran: {r['kernels_of_B']}")
    if "parent_commit" in res:
        p = res["parent_commit"]["legs"]
        lines += ["", f"B (this tree) / A (parent commit) = {t['legs']['B']['median_ms'] / p['A']['median_ms']:.3f}",
                  f"A (this tree) / A (parent commit) = {t['legs']['A']['median_ms'] / p['A']['median_ms']:.3f}",
                  f"C (this tree) / C (parent commit) = {t['legs']['C']['median_ms'] / p['C']['median_ms']:.3f}",
                  f"D (this tree) / D (parent commit) = {t['legs']['D']['median_ms'] / p['D']['median_ms']:.3f}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()

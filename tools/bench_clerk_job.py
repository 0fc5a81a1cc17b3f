#!/usr/bin/env python3
"""A clerk's whole job from its sealed boxes (clerk.rs:78-86), device resident: the two-call sequence against the one-call
form that keeps no plaintext.  P participants' share vectors for ONE clerk (default: 2000 boxes of 349,526 62-bit shares,
the shape of profiles/r02/sealedbox_bench.json) are encoded and sealed on the device, then three legs are timed with
sda_event_*, ALTERNATED repetition by repetition in one process (3 warm-up rounds, REPS >= 20 timed):
    A  begin_dev + sda_sealedbox_open_rows_dev + sda_share_combiner_update_varint_rows_dev + finish_dev
    B  begin_dev + sda_share_combiner_update_sealed_rows_dev + finish_dev
    C  sda_share_combiner_update_varint_rows_dev alone, on the plaintext rows
Every run is a child process under its own time limit; a child that fails or runs out of time ends the whole measurement.
    this tree, release library: A B C           --parent-lib PATH: A and C again on a library built from the parent commit
    --waves-ab: B once more on the library with the test hooks, kernel pinned to 16 and to 8 rows per workgroup
Writes clerk_job_fused.json / .txt into --out-dir (default profiles/r07).  ROWS / VALUES / REPS override the job."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P62 = 4611686006577364993
NEW = "sda_share_combiner_update_sealed_rows_dev"


def child(legs, waves):
    import numpy as np
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    if "B" not in legs:
        capi.SIGNATURES.pop(NEW, None)                       # a library built from the parent commit does not have it
    if waves:
        capi.use_test_hooks()
        capi.check(capi.load().sda_debug_set_knob(b"SDA_SEALED_WAVES", waves))
    lib = capi.load()
    P, L, reps = int(os.environ.get("ROWS", "2000")), int(os.environ.get("VALUES", "349526")), max(20, int(os.environ.get("REPS", "20")))
    shares = DeviceBuffer(P * L)
    capi.check(lib.sda_fill_synthetic_dev(shares.ptr, P, L, L, 0, 0x5DA5DA5DA5DA5DA5, P62, None))
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    vslot = codec.slot_size(L)
    bslot = vslot + 48
    wire, wlen = DeviceBytes(P * vslot), DeviceBytes(P * 8)
    boxes, blen = DeviceBytes(P * bslot), DeviceBytes(P * 8)
    status = DeviceBytes(4).zero()
    sk = bytes(range(1, 33))
    pk = box.public_key(sk)
    codec.encode_rows_dev(shares.ptr, P, L, L, wire.ptr, vslot, wlen.ptr)
    box.seal_rows_dev([pk], P, wire.ptr, vslot, wlen.ptr, P, vslot, boxes.ptr, bslot, blen.ptr)
    synchronize()
    box_bytes = int(np.frombuffer(blen.to_bytes(), dtype="<u8").sum())
    plain, plen = (DeviceBytes(P * vslot), DeviceBytes(P * 8)) if "A" in legs else (None, None)
    comb = crypto.ShareCombiner(crypto.Additive(3, P62))
    sums = DeviceBuffer(L)

    def leg_a():
        comb.begin_dev(1, L)
        box.open_rows_dev(pk, sk, boxes.ptr, bslot, blen.ptr, P, bslot, plain.ptr, vslot, plen.ptr, status.ptr)
        comb.update_encoded_rows_dev(codec, plain.ptr, vslot, plen.ptr, P, status.ptr)
        comb.finish_dev(sums.ptr)

    def leg_b():
        comb.begin_dev(1, L)
        comb.update_sealed_rows_dev(codec, box, pk, sk, boxes.ptr, bslot, blen.ptr, P, bslot, status.ptr)
        comb.finish_dev(sums.ptr)

    def leg_c():
        comb.update_encoded_rows_dev(codec, wire.ptr, vslot, wlen.ptr, P, status.ptr)

    fns = {"A": leg_a, "B": leg_b, "C": leg_c}

    def ev():
        e = C.c_void_p()
        capi.check(lib.sda_event_create(C.byref(e)))
        return e
    a, b = ev(), ev()
    ms = {k: [] for k in legs}
    for rep in range(-3, reps):                              # three warm-up rounds
        for k in legs:
            if k == "C":
                comb.begin_dev(1, L)
            capi.check(lib.sda_event_record(a, None))
            fns[k]()
            capi.check(lib.sda_event_record(b, None))
            t = C.c_float()
            capi.check(lib.sda_event_elapsed_ms(a, b, C.byref(t)))
            if rep >= 0:
                ms[k].append(t.value)
    # the last timed leg's sums against the direct clerk sum of the plaintext shares
    direct = crypto.ShareCombiner(crypto.Additive(3, P62))
    direct.begin_dev(1, L)
    direct.update_dev(shares.ptr, 0, P, L)
    want = DeviceBuffer(L)
    direct.finish_dev(want.ptr)
    verified = {}
    for k in legs:
        if k == "C":
            comb.begin_dev(1, L)
        fns[k]()
        if k == "C":
            comb.finish_dev(sums.ptr)
        verified[k] = bool(np.array_equal(sums.to_numpy(), want.to_numpy())) and status.to_bytes() == bytes(4)
    out = {"library": os.path.basename(capi.active_path()) + " given with --parent-lib" if os.environ.get("SDA_HIP_LIBRARY") else os.path.relpath(capi.active_path(), ROOT), "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(),
           "rows": P, "values": L, "reps": reps, "box_bytes_total": box_bytes, "pinned_waves": waves or None, "legs": {}}
    for k in legs:
        v = sorted(ms[k])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        out["legs"][k] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "box_GBps_at_median": box_bytes / (med * 1e-3) / 1e9,
                          "verified": verified[k]}
    if "B" in legs:
        out["kernels_of_B"] = lib.sda_debug_last_kernel().decode() if verified.get("B") is not None else None
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
    ap.add_argument("--legs", default="ABC")
    ap.add_argument("--waves", type=int, default=0)
    ap.add_argument("--parent-lib", default=None, help="libsda_hip.so built from the parent commit: legs A and C on it")
    ap.add_argument("--waves-ab", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r07"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.legs, a.waves)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"this_tree": run_child(["--legs", "ABC"], {}, a.limit)}

    def save():
        with open(os.path.join(a.out_dir, "clerk_job_fused.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "clerk_job_fused.txt"), "w") as f:
            f.write(report(res))
    save()
    if a.parent_lib:
        res["parent_commit"] = run_child(["--legs", "AC"], {"SDA_HIP_LIBRARY": os.path.abspath(a.parent_lib)}, a.limit)
        save()
    if a.waves_ab:
        for w in (16, 8):
            res[f"this_tree_waves_{w}"] = run_child(["--legs", "B", "--waves", str(w)], {}, a.limit)
            save()
    print(report(res))


def report(res):
    t = res["this_tree"]
    lines = [f"clerk job: {t['rows']} sealed boxes x {t['values']} values, {t['box_bytes_total'] / 1e9:.2f} GB of boxes, {t['reps']} timed repetitions per leg (legs alternated)",
             "leg A = open_rows_dev + update_varint_rows_dev + finish_dev; B = update_sealed_rows_dev + finish_dev; C = update_varint_rows_dev on plaintext", ""]
    for name, r in res.items():
        lines.append(f"[{name}] {r['version']} kernel id {r['kernel_id']}" + (f", pinned to {r['pinned_waves']} rows per workgroup" if r.get("pinned_waves") else ""))
        for k, v in r["legs"].items():
            lines.append(f"  {k}: median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  {v['box_GBps_at_median']:.0f} GB/s of box bytes  verified {v['verified']}")
        if r.get("kernels_of_B"):
            lines.append(f"  B ran: {r['kernels_of_B']}")
    if "parent_commit" in res:
        p = res["parent_commit"]["legs"]
        lines += ["", f"B (this tree) / A (parent commit) = {t['legs']['B']['median_ms'] / p['A']['median_ms']:.3f}",
                  f"C (this tree) / C (parent commit) = {t['legs']['C']['median_ms'] / p['C']['median_ms']:.3f}"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()

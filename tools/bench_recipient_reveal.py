#!/usr/bin/env python3
"""The second half of the recipient's reveal (receive.rs:120-146): n sealed clerking results -> the reconstructed secrets.
Two shapes, each with all n rows, dimension 1 Mi:
    config3   k = 3, t = 1, n = 8 over the 62-bit prime          (8 rows of about 3 MB: ONE wave per row, the known limit)
    pss155    tss's PSS_155_728_100 over 746497                  (728 rows of about 31 KB)
Legs, timed with the host clock around the call(s) and a device synchronise (3 warm-up rounds, REPS >= 20 timed):
    C  sda_sealedbox_open_rows_dev + sda_varint_decode_rows_dev + sda_secret_reconstructor_reconstruct_dev   (the chain)
    S  sda_secret_reconstructor_begin_dev + update_sealed_rows_dev + finish_dev                              (the streaming job)
Every run is a child process under its own time limit; a child that fails or runs out of time ends the whole measurement.
    this tree: C and S alternated      --parent-lib PATH: C again on a library built from the parent commit
Writes recipient_reveal.json / .txt into --out-dir (default profiles/r10).  DIMENSION / REPS override the shape."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P62 = 4611686006577364993
SHAPES = {"config3": (P62, 3, 1, 8, 631229665360524489, 3451275676410824977),
          "pss155": (746497, 100, 155, 728, 95660, 610121)}
NEW = ["sda_secret_reconstructor_begin_dev", "sda_secret_reconstructor_update_dev", "sda_secret_reconstructor_update_sealed_rows_dev",
       "sda_secret_reconstructor_finish_dev"]


def child(shape, legs):
    import numpy as np
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    if "S" not in legs:
        for name in NEW:
            capi.SIGNATURES.pop(name, None)                  # a library built from the parent commit does not have them
    lib = capi.load()
    p, k, t, n, w2, w3 = SHAPES[shape]
    dim, reps = int(os.environ.get("DIMENSION", str(1 << 20))), max(20, int(os.environ.get("REPS", "20")))
    B = -(-dim // k)
    stride = B + (B & 1)
    rows = np.random.default_rng(n).integers(0, p, size=(n, stride), dtype=np.int64)      # clerk sums are uniform residues
    indices = list(range(n))
    rec = crypto.SecretReconstructor(crypto.PackedShamir(k, n, t, p, w2, w3), dim)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    sk = bytes(range(1, 33))
    pk = box.public_key(sk)
    d_rows = DeviceBuffer.from_numpy(rows)
    slot = max(codec.slot_size(B), 16) + 48
    boxes, blen = DeviceBytes(n * slot).zero(), DeviceBytes(n * 8).zero()
    box.seal_share_rows_dev(codec, [pk], n, d_rows.ptr, n, B, stride, boxes.ptr, slot, blen.ptr)
    synchronize()
    box_bytes = int(np.frombuffer(blen.to_bytes(), dtype="<u8").sum())
    status = DeviceBytes(4).zero()
    d_out = DeviceBuffer(dim)
    held = {}
    if "C" in legs:
        plain, plen = DeviceBytes(n * slot), DeviceBytes(n * 8).zero()
        decoded = DeviceBuffer(n * stride)
        held["C"] = n * slot + n * stride * 8 + dim * 8
    held["S"] = B * k * 16 + n * k * 8 + dim * 8             # 128-bit accumulators, the transposed matrix, the output

    def leg_c():
        box.open_rows_dev(pk, sk, boxes.ptr, slot, blen.ptr, n, slot, plain.ptr, slot, plen.ptr, status.ptr)
        codec.decode_rows_dev(plain.ptr, slot, plen.ptr, n, B, decoded.ptr, stride, status.ptr)
        rec.reconstruct_dev(indices, decoded.ptr, B, stride, d_out.ptr, dim)

    def leg_s():
        rec.begin_dev(indices, n, B)
        rec.update_sealed_rows_dev(codec, box, pk, sk, 0, boxes.ptr, slot, blen.ptr, n, slot, status.ptr)
        rec.finish_dev(d_out.ptr, dim)

    fns = {"C": leg_c, "S": leg_s}
    ms = {x: [] for x in legs}
    for rep in range(-3, reps):                              # three warm-up rounds
        for x in legs:
            synchronize()
            t0 = time.perf_counter()
            fns[x]()
            synchronize()
            if rep >= 0:
                ms[x].append((time.perf_counter() - t0) * 1e3)
    want = DeviceBuffer(dim)
    rec.reconstruct_dev(indices, d_rows.ptr, B, stride, want.ptr, dim)
    want = want.to_numpy()
    verified = {}
    for x in legs:
        d_out.zero()
        fns[x]()
        verified[x] = bool(np.array_equal(d_out.to_numpy(), want)) and status.to_bytes() == bytes(4)
    out = {"library": "given with --parent-lib" if os.environ.get("SDA_HIP_LIBRARY") else os.path.relpath(capi.active_path(), ROOT),
           "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(), "shape": shape, "rows": n, "k": k,
           "dimension": dim, "reps": reps, "sealed_bytes": box_bytes, "legs": {}}
    for x in legs:
        v = sorted(ms[x])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        out["legs"][x] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "device_bytes_held": held[x], "verified": verified[x]}
    if "S" in legs:
        out["kernels_of_S"] = lib.sda_debug_last_kernel().decode()
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


def report(res):
    lines = ["recipient reveal from sealed clerking results, dimension 1 Mi unless DIMENSION says otherwise; host clock around call(s) + synchronise,",
             "legs alternated; C = open_rows_dev + decode_rows_dev + reconstruct_dev, S = begin_dev + update_sealed_rows_dev + finish_dev",
             "device bytes held = what the form keeps for the job besides the sealed boxes themselves", ""]
    for shape, r in res.items():
        t = r["this_tree"]
        lines.append(f"[{shape}] {t['rows']} rows, k = {t['k']}, dimension {t['dimension']}, {t['sealed_bytes']} sealed bytes, {t['reps']} repetitions; "
                     f"{t['version']} kernel id {t['kernel_id']}")
        for x, v in t["legs"].items():
            lines.append(f"  this tree {x}: median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  "
                         f"device bytes held {v['device_bytes_held']}  verified {v['verified']}")
        if t.get("kernels_of_S"):
            lines.append(f"  S ran: {t['kernels_of_S']}")
        base, who = t["legs"]["C"]["median_ms"], "this tree"
        if "parent_commit" in r:
            v = r["parent_commit"]["legs"]["C"]
            lines.append(f"  parent commit C: median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  verified {v['verified']}")
            base, who = v["median_ms"], "parent commit"
        lines += [f"  S (this tree) / C ({who}) = {t['legs']['S']['median_ms'] / base:.3f}", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--legs", default="CS")
    ap.add_argument("--parent-lib", default=None, help="libsda_hip.so built from the parent commit: leg C on it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r10"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.shape, a.legs)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {}

    def save():
        with open(os.path.join(a.out_dir, "recipient_reveal.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "recipient_reveal.txt"), "w") as f:
            f.write(report(res))
    for shape in ([a.shape] if a.shape else list(SHAPES)):
        res[shape] = {"this_tree": run_child(["--shape", shape, "--legs", "CS"], {}, a.limit)}
        save()
        if a.parent_lib:
            res[shape]["parent_commit"] = run_child(["--shape", shape, "--legs", "C"], {"SDA_HIP_LIBRARY": os.path.abspath(a.parent_lib)}, a.limit)
            save()
    print(report(res))


if __name__ == "__main__":
    main()

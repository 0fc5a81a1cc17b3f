#!/usr/bin/env python3
"""The recipient's mask combine (receive.rs:101-118, chacha.rs:56-77): P ChaCha seeds expanded to `dimension` masks each and
summed.  Default shape: P = 4096 seeds x dimension 1 Mi over the 62-bit prime (VERDICT.md "Next round" item 2).  Legs, timed
with the host clock around the call(s) and a device synchronise, ALTERNATED repetition by repetition in one process (3 warm-up
rounds, REPS >= 20 timed):
    H  sda_mask_combiner_combine          host form: seeds from host pointers, the combined mask back to the host
    D  begin_dev + update_dev + finish_dev            seeds [P][4] resident in HBM, the combined mask stays there
    S  begin_dev + update_sealed_rows_dev + finish_dev   the same seeds as P sealed boxes resident in HBM
Every run is a child process under its own time limit; a child that fails or runs out of time ends the whole measurement.
    this tree: H D S            --parent-lib PATH: the same three legs on a library built from the parent commit, this tree / parent
Writes mask_combine_dev.json / .txt into --out-dir (default profiles/r09).  SEEDS / DIMENSION / REPS override the shape."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P62 = 4611686006577364993


def child(legs):
    import numpy as np
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    lib = capi.load()
    P, dim, reps = int(os.environ.get("SEEDS", "4096")), int(os.environ.get("DIMENSION", str(1 << 20))), max(20, int(os.environ.get("REPS", "20")))
    S = np.random.default_rng(P).integers(0, 1 << 32, size=(P, 4), dtype=np.int64)
    comb = crypto.MaskCombiner(crypto.ChaCha(P62, dim, 128))
    rows = (C.POINTER(C.c_int64) * P)(*[S[r].ctypes.data_as(C.POINTER(C.c_int64)) for r in range(P)])
    lens = (C.c_size_t * P)(*([4] * P))
    host_out, n_out = np.empty(dim, dtype=np.int64), C.c_size_t()
    d_S, d_out = DeviceBuffer.from_numpy(S), DeviceBuffer(dim)
    status = DeviceBytes(4).zero()
    if "S" in legs:
        codec, box = crypto.VarintCodec(), crypto.SealedBox()
        sk = bytes(range(1, 33))
        pk = box.public_key(sk)
        slot = max(codec.slot_size(4), 16) + 48
        boxes, blen = DeviceBytes(P * slot).zero(), DeviceBytes(P * 8).zero()
        box.seal_share_rows_dev(codec, [pk], P, d_S.ptr, P, 4, 4, boxes.ptr, slot, blen.ptr)
        synchronize()

    def leg_h():
        capi.check(lib.sda_mask_combiner_combine(comb._h, rows, lens, P, host_out.ctypes.data_as(C.POINTER(C.c_int64)), dim, C.byref(n_out)))

    def leg_d():
        comb.begin_dev(dim)
        comb.update_dev(d_S.ptr, P, 4, 4)
        comb.finish_dev(d_out.ptr, dim)

    def leg_s():
        comb.begin_dev(dim)
        comb.update_sealed_rows_dev(codec, box, pk, sk, boxes.ptr, slot, blen.ptr, P, slot, status.ptr)
        comb.finish_dev(d_out.ptr, dim)

    fns = {"H": leg_h, "D": leg_d, "S": leg_s}
    ms = {k: [] for k in legs}
    for rep in range(-3, reps):                              # three warm-up rounds
        for k in legs:
            synchronize()
            t0 = time.perf_counter()
            fns[k]()
            synchronize()
            if rep >= 0:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    leg_h()
    want = host_out.copy()
    verified = {}
    for k in legs:
        fns[k]()
        verified[k] = bool(np.array_equal(host_out if k == "H" else d_out.to_numpy(), want)) and status.to_bytes() == bytes(4)
    out = {"library": "given with --parent-lib" if os.environ.get("SDA_HIP_LIBRARY") else os.path.relpath(capi.active_path(), ROOT),
           "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(), "seeds": P, "dimension": dim, "reps": reps,
           "chacha_blocks": P * ((dim + 7) // 8), "legs": {}}
    for k in legs:
        v = sorted(ms[k])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        out["legs"][k] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "blocks_per_s_at_median": out["chacha_blocks"] / (med * 1e-3),
                          "verified": verified[k]}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--legs", default="HDS")
    ap.add_argument("--parent-lib", default=None, help="libsda_hip.so built from the parent commit: the same legs on it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r09"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.legs)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {"this_tree": run_child(["--legs", "HDS"], {}, a.limit)}

    def save():
        with open(os.path.join(a.out_dir, "mask_combine_dev.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "mask_combine_dev.txt"), "w") as f:
            f.write(report(res))
    save()
    if a.parent_lib:
        res["parent_commit"] = run_child(["--legs", "HDS"], {"SDA_HIP_LIBRARY": os.path.abspath(a.parent_lib)}, a.limit)
        save()
    print(report(res))


def report(res):
    t = res["this_tree"]
    lines = [f"mask combine: {t['seeds']} ChaCha seeds x dimension {t['dimension']} over the 62-bit prime = {t['chacha_blocks']:.3e} ChaCha blocks, "
             f"{t['reps']} timed repetitions per leg (legs alternated, host clock around call + synchronise)",
             "leg H = sda_mask_combiner_combine (host form); D = begin_dev + update_dev + finish_dev; S = begin_dev + update_sealed_rows_dev + finish_dev", ""]
    for name, r in res.items():
        lines.append(f"[{name}] {r['version']} kernel id {r['kernel_id']}")
        for k, v in r["legs"].items():
            lines.append(f"  {k}: median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  {v['blocks_per_s_at_median']:.3e} blocks/s  verified {v['verified']}")
        if r.get("kernels_of_S"):
            lines.append(f"  S ran: {r['kernels_of_S']}")
    if "parent_commit" in res:
        lines.append("")
        for k, v in res["parent_commit"]["legs"].items():
            lines.append(f"{k}: this tree / parent commit = {t['legs'][k]['median_ms'] / v['median_ms']:.3f}")
        lines.append("required: every ratio <= 1.04, or the parent-vs-parent spread of the day where that is larger")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()

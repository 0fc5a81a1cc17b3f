#!/usr/bin/env python3
"""The head of a participation (participate.rs:75-101), device resident: share the secrets and seal every clerk's vector - the
two-call chain with its share buffer against the one call that has none.  Config 3 (packed Shamir k=3, t=1, n=8 over the 62-bit
prime, dimension 1 Mi, PARTICIPANTS = 250: 2000 share rows of 349,526 values) is sealed to 8 clerk keys with OS-entropy
ephemeral keys; the generators run in deterministic mode on one CSPRNG key, so every leg seals the same shares.  The legs are
timed with sda_event_*, ALTERNATED repetition by repetition in one process (3 warm-up rounds, REPS >= 20 timed):
    A   generate_batch_dev + seal_share_rows_dev on a library BUILT FROM THE PARENT COMMIT (--parent-lib, required)
    A2  the same chain on this tree's release library (the encode loop both of its kernels share was templated)
    B   sda_share_generator_generate_sealed_rows_dev, this tree's release library
    R   the same call with a workgroup on consecutive rows instead of the clerks of one participant (knob SDA_GENSEAL_BY_ROWS,
        this tree's library with the test hooks)
After the timed rounds every leg runs once more into a wiped box buffer; three of its boxes are opened with the clerk's secret
key and compared with the C oracle's shares of that (clerk, participant) (oracle/: drbg_fill -> packed_generate_csprng).  For
every leg the device bytes it holds BESIDES the secrets and the boxes are measured (free device memory before its handles and
buffers exist against after its first call).
The measurement runs in a child process under its own time limit.
Writes participant_generate_seal.json / .txt into --out-dir (default profiles/r11).  PARTICIPANTS / DIM / REPS override the job,
ORDER=A2,A,R,B the order of the legs inside a repetition, --suffix the file names."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P62 = 4611686006577364993
NEW = "sda_share_generator_generate_sealed_rows_dev"
KEY = bytes((i * 7 + 1) & 0xFF for i in range(32))
K, T, N = 3, 1, 8


def child(parent_lib):
    import numpy as np
    from oracle import coracle, pyoracle as po
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    sig = capi.SIGNATURES.pop(NEW)                            # a library built from the parent commit does not have it
    capi._load_path(parent_lib)
    capi.SIGNATURES[NEW] = sig
    paths = {"A": parent_lib, "A2": None, "B": None, "R": capi.TEST_LIB_PATH}
    order = os.environ.get("ORDER", "A,A2,B,R").split(",")   # the order inside a repetition (a leg's time depends on what ran before it)
    assert sorted(order) == sorted(paths)
    paths = {k: paths[k] for k in order}
    hooks = capi.hooks_library()

    class on:                                                 # the library a leg's handles live in is the active one while it runs
        def __init__(self, leg): self.path = paths[leg]
        def __enter__(self): capi._active_path = self.path
        def __exit__(self, *a): capi._active_path = None

    lib = capi.load()
    P, dim, reps = int(os.environ.get("PARTICIPANTS", "250")), int(os.environ.get("DIM", str(1 << 20))), max(20, int(os.environ.get("REPS", "20")))
    B = (dim + K - 1) // K
    rows = N * P
    w2, w3 = po.P62_OMEGA[8], po.P62_OMEGA[9]
    sch = crypto.PackedShamir(K, N, T, P62, w2, w3)
    secrets = DeviceBuffer(P * dim)
    capi.check(lib.sda_fill_synthetic_dev(secrets.ptr, P, dim, dim, 0, 0x5DA5DA5DA5DA5DA5, P62, None))
    slot = crypto.VarintCodec().slot_size(B) + 48
    boxes, blen = DeviceBytes(rows * slot), DeviceBytes(rows * 8).zero()
    sks = [bytes([c + 1]) * 32 for c in range(N)]
    pks = [crypto.SealedBox().public_key(sk) for sk in sks]
    synchronize()

    def free_now():
        synchronize()
        f, t = C.c_size_t(), C.c_size_t()
        capi.check(hooks.sda_debug_mem_info(C.byref(f), C.byref(t)))
        return f.value

    fns, held, keep = {}, {}, []
    for leg in paths:
        before = free_now()
        with on(leg):
            gen, codec, box = crypto.ShareGenerator(sch), crypto.VarintCodec(), crypto.SealedBox()
            gen.set_drbg_key(KEY)
            if leg == "R":
                capi.check(capi._load_path(capi.TEST_LIB_PATH).sda_debug_set_knob(b"SDA_GENSEAL_BY_ROWS", 1))
            if leg in ("A", "A2"):
                shares = DeviceBuffer(rows * B)

                def fn(gen=gen, codec=codec, box=box, shares=shares):
                    gen.generate_batch_dev(secrets.ptr, P, dim, dim, shares.ptr, B, P * B)
                    box.seal_share_rows_dev(codec, pks, P, shares.ptr, rows, B, B, boxes.ptr, slot, blen.ptr)
            else:
                def fn(gen=gen, codec=codec, box=box):
                    gen.generate_sealed_rows_dev(codec, box, pks, secrets.ptr, P, dim, dim, boxes.ptr, slot, blen.ptr)
            fn()
        held[leg] = before - free_now()
        fns[leg] = fn
        keep.append((leg, gen, codec, box))

    def ev():
        e = C.c_void_p()
        capi.check(lib.sda_event_create(C.byref(e)))
        return e
    a, b = ev(), ev()
    ms = {k: [] for k in paths}
    for rep in range(-3, reps):                              # three warm-up rounds
        for k in paths:
            capi.check(lib.sda_event_record(a, None))
            with on(k):
                fns[k]()
            capi.check(lib.sda_event_record(b, None))
            t = C.c_float()
            capi.check(lib.sda_event_elapsed_ms(a, b, C.byref(t)))
            if rep >= 0:
                ms[k].append(t.value)
    # every leg once more into a wiped box buffer: three of its boxes must open to the oracle's shares
    sample = sorted({0, rows // 3, rows - 1})
    want = {}
    for r in sample:
        c, q = divmod(r, P)
        sec = secrets.to_numpy(dim, q * dim)
        want[r] = coracle.packed_generate_csprng(P62, K, T, N, w2, w3, sec, coracle.drbg_fill(KEY, q, B, T, P62), 1)[c]
    verified, box_bytes, kernels = {}, 0, {}
    for k in paths:
        boxes.zero(); blen.zero()
        with on(k):
            fns[k]()
            kernels[k] = lib.sda_debug_last_kernel().decode()
        lens = np.frombuffer(blen.to_bytes(), dtype="<u8")
        box_bytes = int(lens.sum())
        ok = bool((lens > 48).all())
        for r in sample:
            dec = crypto.ShareDecryptor(pks[r // P], sks[r // P])
            ok = ok and bool(np.array_equal(dec.decrypt(boxes.to_bytes(int(lens[r]), r * slot)), want[r]))
        verified[k] = ok
    with on("A"):
        parent = {"version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode()}
    out = {"this_tree": {"version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode()}, "parent_commit": parent,
           "participants": P, "dimension": dim, "rows": rows, "values_per_row": B, "reps": reps, "box_bytes_total": box_bytes,
           "secret_bytes": P * dim * 8, "share_buffer_bytes": rows * B * 8, "boxes_opened_per_leg": len(sample), "legs": {}}
    for k in paths:
        v = sorted(ms[k])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        out["legs"][k] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "box_GBps_at_median": box_bytes / (med * 1e-3) / 1e9,
                          "held_bytes_besides_secrets_and_boxes": held[k], "verified": verified[k], "last_kernels": kernels[k]}
    for leg, gen, codec, box in keep:                         # a handle is freed by the library that made it
        with on(leg):
            gen.close(); codec.close(); box.close()
    print("RESULT " + json.dumps(out))


LEGS = {"A": "generate_batch_dev + seal_share_rows_dev, library built from the parent commit",
        "A2": "generate_batch_dev + seal_share_rows_dev, this tree",
        "B": "generate_sealed_rows_dev, this tree (a workgroup = the clerks of one participant)",
        "R": "generate_sealed_rows_dev, this tree, knob SDA_GENSEAL_BY_ROWS (a workgroup = consecutive rows of one clerk)"}


def report(r):
    lines = [f"participation: {r['participants']} participants x dimension {r['dimension']}, packed Shamir k={K} t={T} n={N} over the 62-bit prime: "
             f"{r['rows']} share rows x {r['values_per_row']} values, {r['box_bytes_total'] / 1e9:.2f} GB of boxes, {r['secret_bytes'] / 1e9:.2f} GB of secrets; "
             f"{r['reps']} timed repetitions per leg (legs alternated in one process), {r['boxes_opened_per_leg']} boxes of every leg opened and compared with the oracle's shares",
             "order of the legs inside a repetition: " + " ".join(r["legs"]),
             f"this tree: {r['this_tree']['version']} kernel id {r['this_tree']['kernel_id']}; parent commit: {r['parent_commit']['version']} build {r['parent_commit']['kernel_id']}", ""]
    for k, v in r["legs"].items():
        lines.append(f"  {k:2s} {LEGS[k]}")
        lines.append(f"     median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  {v['box_GBps_at_median']:.0f} GB/s of box bytes  verified {v['verified']}")
        lines.append(f"     device bytes held besides the secrets and the boxes: {v['held_bytes_besides_secrets_and_boxes']} ({v['held_bytes_besides_secrets_and_boxes'] / 1e9:.3f} GB)   ran: {v['last_kernels']}")
    L = r["legs"]
    lines += ["", f"B / A  (new call / parent's chain)            = {L['B']['median_ms'] / L['A']['median_ms']:.3f}",
              f"A2 / A (this tree's chain / parent's chain)   = {L['A2']['median_ms'] / L['A']['median_ms']:.3f}",
              f"R / B  (rows mapping / participant mapping)   = {L['R']['median_ms'] / L['B']['median_ms']:.3f}",
              f"held by B / held by A                         = {L['B']['held_bytes_besides_secrets_and_boxes'] / max(L['A']['held_bytes_besides_secrets_and_boxes'], 1):.4f}"
              f"   (the chain's share buffer alone: {r['share_buffer_bytes'] / 1e9:.2f} GB)"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", required=True, help="libsda_hip.so built from the parent commit: leg A runs on it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r11"))
    ap.add_argument("--limit", type=int, default=400, help="seconds for the measuring child process")
    ap.add_argument("--suffix", default="", help="appended to the output file names (a second run in another leg order)")
    a = ap.parse_args()
    if a.child:
        return child(os.path.abspath(a.parent_lib))
    os.makedirs(a.out_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--parent-lib", a.parent_lib]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    sys.stderr.write(r.stderr[-3000:])
    if r.returncode != 0:
        raise SystemExit(f"the measuring child ended with status {r.returncode}: nothing more is started")
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    with open(os.path.join(a.out_dir, f"participant_generate_seal{a.suffix}.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out_dir, f"participant_generate_seal{a.suffix}.txt"), "w") as f:
        f.write(report(res))
    print(report(res))


if __name__ == "__main__":
    main()

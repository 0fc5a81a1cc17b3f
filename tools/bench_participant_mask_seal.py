#!/usr/bin/env python3
"""The masking step of a participation (participate.rs:52-72), device resident: mask the secrets and seal every participant's mask
to the recipient - the two-call chain with its mask buffer against the one call that has none.
    A   sda_secret_masker_mask_batch_dev + sda_sealedbox_seal_share_rows_dev on a library BUILT FROM THE PARENT COMMIT
        (--parent-lib, required), with their participants x mask_len buffer of plaintext masks
    B   sda_secret_masker_mask_sealed_rows_dev, this tree's release library
Shapes: Full over the 62-bit prime at 2000 participants x 349,526 values and at 64 x 1 Mi (mask_seal_stream_kernel: one wave per
participant), and ChaCha at (62-bit prime, dimension 4099, 9 participants) of tests/mask_combiner_cases.CHACHA_SHAPES (no new
kernel: the expansion driver, then the seed rows sealed).  The Full maskers run in deterministic mode on one CSPRNG key, so both
legs seal the same masks; ChaCha seeds and all ephemeral keys come from the OS.  The legs are timed with sda_event_*, ALTERNATED
repetition by repetition in one process (3 warm-up rounds, REPS >= 10 timed); reported: median, min and max per leg.  After the
timed rounds each Full leg runs once more into a wiped box buffer; three of its boxes are opened with the recipient's secret key
and compared with the C oracle's draws (oracle/: drbg_fill), and the masked secrets of those rows with (secret + mask) mod q.
The measurement runs in a child process under its own time limit and writes participant_mask_seal.json / .txt into --out-dir
(default profiles/r15).

--resources (needs hipcc, no GPU): compiles varint_kernels.hip for gfx950 to assembly with the compiler's resource report and
appends to the .txt the VGPR / SGPR / LDS / scratch figures of mask_seal_stream_kernel<20 | 12 | 8> and the instruction counts of
the three kernels that share encode_row with it - of this tree and, with --parent-src DIR (a checkout of the parent commit), of
the parent."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P62 = 4611686006577364993
NEW = "sda_secret_masker_mask_sealed_rows_dev"
KEY = bytes((i * 7 + 1) & 0xFF for i in range(32))
SHAPES = [("full", P62, 2000, 349_526), ("full", P62, 64, 1 << 20), ("chacha", P62, 9, 4099)]
SHARED = ["varint_stream_encode_kernel", "varint_seal_stream_kernel", "share_seal_stream_kernel"]


def measure(kind, q, P, L, parent_lib, reps):
    import numpy as np
    from oracle import coracle
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    paths = {"A": parent_lib, "B": None}

    class on:                                                 # the library a leg's handles live in is the active one while it runs
        def __init__(self, leg): self.path = paths[leg]
        def __enter__(self): capi._active_path = self.path
        def __exit__(self, *a): capi._active_path = None

    lib = capi.load()
    scheme = crypto.Full(q) if kind == "full" else crypto.ChaCha(q, L, 128)
    mask_len = L if kind == "full" else 4
    secrets, masked = DeviceBuffer(P * L), DeviceBuffer(P * L)
    capi.check(lib.sda_fill_synthetic_dev(secrets.ptr, P, L, L, 0, 0x5DA5DA5DA5DA5DA5, q, None))
    slot = crypto.VarintCodec().slot_size(mask_len) + 48
    boxes, blen = DeviceBytes(P * slot), DeviceBytes(P * 8).zero()
    sk = bytes(range(1, 33))
    pk = crypto.SealedBox().public_key(sk)
    synchronize()
    fns, keep = {}, []
    for leg in paths:
        with on(leg):
            masker, codec, box = crypto.SecretMasker(scheme), crypto.VarintCodec(), crypto.SealedBox()
            if kind == "full":
                masker.set_drbg_key(KEY)
            if leg == "A":
                masks = DeviceBuffer(P * mask_len)

                def fn(masker=masker, codec=codec, box=box, masks=masks):
                    masker.mask_batch_dev(secrets.ptr, P, L, L, masks.ptr, mask_len, masked.ptr, L)
                    box.seal_share_rows_dev(codec, [pk], P, masks.ptr, P, mask_len, mask_len, boxes.ptr, slot, blen.ptr)
            else:
                def fn(masker=masker, codec=codec, box=box):
                    masker.mask_sealed_rows_dev(codec, box, pk, secrets.ptr, P, L, L, masked.ptr, L, boxes.ptr, slot, blen.ptr)
        fns[leg] = fn
        keep.append((leg, masker, codec, box))

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
            synchronize()
            t = C.c_float()
            capi.check(lib.sda_event_elapsed_ms(a, b, C.byref(t)))
            if rep >= 0:
                ms[k].append(t.value)
    verified, box_bytes, kernels = {}, 0, {}
    sample = sorted({0, P // 3, P - 1})
    for k in paths:
        boxes.zero(); blen.zero()
        with on(k):
            fns[k]()
            kernels[k] = lib.sda_debug_last_kernel().decode()
        lens = np.frombuffer(blen.to_bytes(), dtype="<u8")
        box_bytes = int(lens.sum())
        ok = bool((lens > 48).all())
        if kind == "full":                                   # ChaCha seeds are the OS's: the GPU tests compare that kind with the oracle
            for p in sample:
                want = coracle.drbg_fill(KEY, p, L, 1, q)
                got = crypto.ShareDecryptor(pk, sk).decrypt(boxes.to_bytes(int(lens[p]), p * slot))
                sec = secrets.to_numpy(L, p * L)
                sums = ((sec.astype(object) % q + want.astype(object)) % q).astype(np.int64)
                ok = ok and bool(np.array_equal(got, want)) and bool(np.array_equal(masked.to_numpy(L, p * L), sums))
        verified[k] = ok
    out = {"kind": kind, "modulus": q, "participants": P, "len": L, "mask_len": mask_len, "reps": reps, "box_bytes_total": box_bytes,
           "mask_buffer_bytes": P * mask_len * 8, "legs": {}}
    for k in paths:
        v = sorted(ms[k])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        out["legs"][k] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "verified": verified[k], "last_kernels": kernels[k]}
    for leg, masker, codec, box in keep:                      # a handle is freed by the library that made it
        with on(leg):
            masker.close(); codec.close(); box.close()
    return out


def child(parent_lib):
    from sda_amd import capi
    sig = capi.SIGNATURES.pop(NEW)                            # a library built from the parent commit does not have it
    capi._load_path(parent_lib)
    capi.SIGNATURES[NEW] = sig
    lib = capi.load()
    reps = max(10, int(os.environ.get("REPS", "12")))
    capi._active_path = parent_lib
    parent = {"version": capi.load().sda_version().decode(), "kernel_id": capi.load().sda_kernel_id().decode()}
    capi._active_path = None
    out = {"this_tree": {"version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode()}, "parent_commit": parent,
           "shapes": [measure(kind, q, P, L, parent_lib, reps) for kind, q, P, L in SHAPES]}
    print("RESULT " + json.dumps(out))


def report(r):
    lines = ["the masking step of a participation: A = mask_batch_dev + seal_share_rows_dev with their mask buffer, library built from the parent commit;",
             "B = sda_secret_masker_mask_sealed_rows_dev, this tree.  Legs alternated in one process, 3 warm-up rounds.",
             f"this tree: {r['this_tree']['version']} kernel id {r['this_tree']['kernel_id']}; parent commit: {r['parent_commit']['version']} kernel id {r['parent_commit']['kernel_id']}", ""]
    for s in r["shapes"]:
        A, B = s["legs"]["A"], s["legs"]["B"]
        lines.append(f"{s['kind']}  modulus {s['modulus']}  {s['participants']} participants x {s['len']} values  ({s['reps']} timed repetitions per leg; "
                     f"{s['box_bytes_total'] / 1e6:.1f} MB of boxes, the chain's mask buffer {s['mask_buffer_bytes'] / 1e6:.1f} MB)")
        for k, v in (("A", A), ("B", B)):
            lines.append(f"  {k}  median {v['median_ms']:.3f} ms  (min {v['min_ms']:.3f}, max {v['max_ms']:.3f})  verified {v['verified']}  ran: {v['last_kernels']}")
        spread = (A["max_ms"] - A["min_ms"]) + (B["max_ms"] - B["min_ms"])
        gain = A["median_ms"] - B["median_ms"]
        lines.append(f"  B / A = {B['median_ms'] / A['median_ms']:.3f};  A - B = {gain:.3f} ms against the two spreads together {spread:.3f} ms: "
                     + ("B's median beats A's by more than that" if gain > spread else "B's median does NOT beat A's by more than that"))
        lines.append("")
    return "\n".join(lines)


# ---- the compiler's figures (no GPU) -------------------------------------------------------------------------------------------
def compile_report(src_root):
    """varint_kernels.hip of a tree -> ({kernel: {figure: value}}, {kernel: instruction count})"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "varint.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                            "-Rpass-analysis=kernel-resource-usage", "-o", asm, os.path.join(src_root, "sda_amd", "csrc", "varint_kernels.hip")],
                           check=True, capture_output=True, text=True, cwd=tmp)
        text = open(asm).read().split("\n")
    figures, name = {}, None
    for line in r.stderr.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            figures[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:\[]*?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and name:
            figures[name][m.group(1).strip()] = m.group(2)
    counts, name, n = {}, None, 0
    for line in text:
        m = re.match(r"^(_ZN3sda\w+):", line)
        if m:
            name, n = m.group(1), 0
        elif line.startswith(".Lfunc_end") and name:
            counts[name], name = n, None
        elif name:
            t = line.split(";")[0].strip()
            if t and not t.startswith(".") and not t.endswith(":"):
                n += 1
    return figures, counts


def resources(out_dir, parent_src):
    figures, counts = compile_report(ROOT)
    before = compile_report(parent_src)[1] if parent_src else {}
    lines = ["", "the compiler's resource report (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage), this tree:"]
    for k in sorted(figures):
        if "mask_seal_stream_kernel" in k:
            f = figures[k]
            lines.append(f"  {k}: VGPRs {f.get('VGPRs')}  AGPRs {f.get('AGPRs')}  SGPRs {f.get('TotalSGPRs')}  LDS {f.get('LDS Size')} B/workgroup  "
                         f"scratch {f.get('ScratchSize')} B/lane  VGPR spill {f.get('VGPRs Spill')}  occupancy {f.get('Occupancy')} waves/SIMD  "
                         f"{counts.get(k)} instructions")
    lines.append("instruction counts of the kernels that share encode_row / EncXSalsa with it (parent commit -> this tree):")
    for k in sorted(counts):
        if any(s in k for s in SHARED):
            lines.append(f"  {k}: {before.get(k, 'not compiled')} -> {counts[k]}")
    path = os.path.join(out_dir, "participant_mask_seal.txt")
    old = open(path).read() if os.path.exists(path) else ""
    old = old.split("\nthe compiler's resource report")[0].rstrip("\n")
    with open(path, "w") as f:
        f.write(old + "\n" + "\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", help="libsda_hip.so built from the parent commit: leg A runs on it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r15"))
    ap.add_argument("--limit", type=int, default=400, help="seconds for the measuring child process")
    ap.add_argument("--resources", action="store_true", help="append the compiler's figures to the report (needs hipcc, no GPU)")
    ap.add_argument("--parent-src", help="--resources: a checkout of the parent commit, for the instruction counts before the change")
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    if a.resources:
        return resources(a.out_dir, a.parent_src)
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    if a.child:
        return child(os.path.abspath(a.parent_lib))
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--parent-lib", a.parent_lib]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    sys.stderr.write(r.stderr[-3000:])
    if r.returncode != 0:
        raise SystemExit(f"the measuring child ended with status {r.returncode}: nothing more is started")
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    with open(os.path.join(a.out_dir, "participant_mask_seal.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out_dir, "participant_mask_seal.txt"), "w") as f:
        f.write(report(res))
    print(report(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The recipient's reconstruction from sealed clerking results (receive.rs:120-146) with and without the parity checks riding along:
    A   sda_secret_reconstructor_begin_dev + update_sealed_rows_dev + finish_dev          on a library built from the parent commit
    B   the same three calls                                                              on this tree (must not have moved)
    C1, C2, C4   begin_checked_dev (checks = 1, 2, 4) + update_sealed_rows_dev + finish_checked_dev (SDA_CHECK_CORRECT)   this tree
Shapes, dimension 1 Mi, clean rows (the finish of a clean job is its cheapest: nothing to locate):
    config3   k = 3, t = 1, n = 8 over the 62-bit prime, all 8 rows           (r = 4)
    pss155    tss's PSS_155_728_100 over 746497, 260 scattered rows           (r = 5; job width k + checks = 101 .. 104)
Timed with the host clock around the calls and a device synchronise; the legs alternate in one process (both libraries sit on the
one HIP runtime), 3 warm-up rounds, REPS >= 20 timed; median with (min - max).  Every leg's output is compared with
reconstruct_dev on the decoded rows, the checked legs' reports must be clean.
Every shape is a child process under its own time limit; a child that fails or runs out of time ends the whole measurement.
    --parent-lib PATH   libsda_hip.so built from the parent commit (leg A); without it leg A runs on this tree's library and says so
Writes recipient_reveal_checked.json / .txt into --out-dir (default profiles/r18).  DIMENSION / REPS override the shape."""
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
SHAPES = {"config3": ((P62, 3, 1, 8, 631229665360524489, 3451275676410824977), tuple(range(8))),
          "pss155": ((746497, 100, 155, 728, 95660, 610121), tuple((37 * i + 5) % 728 for i in range(260)))}
CHECKS = (1, 2, 4)
NEW = ["sda_secret_reconstructor_begin_checked_dev", "sda_secret_reconstructor_finish_checked_dev"]
USED = ["sda_version", "sda_kernel_id", "sda_last_error", "sda_debug_last_kernel", "sda_secret_reconstructor_new", "sda_secret_reconstructor_free",
        "sda_secret_reconstructor_begin_dev", "sda_secret_reconstructor_update_sealed_rows_dev", "sda_secret_reconstructor_finish_dev",
        "sda_varint_codec_new", "sda_varint_codec_free", "sda_sealedbox_new", "sda_sealedbox_free"]


def open_library(path, with_new):
    """a library by path with the signatures of the calls this tool makes (a parent-commit build lacks the new ones)"""
    from sda_amd import capi
    lib = C.CDLL(path)
    for name in USED + (NEW if with_new else []):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = capi.SIGNATURES[name]
    return lib


class Job:
    """the handles of one library and the sealed rows they stream"""

    def __init__(self, lib, scheme, indices, dim, boxes, slot, lens, pk, sk, d_status):
        from sda_amd import capi
        p, k, t, n, w2, w3 = scheme
        self.lib, self.dim, self.rows, self.B = lib, dim, len(indices), -(-dim // k)
        self.boxes, self.slot, self.lens, self.pk, self.sk, self.d_status = boxes, slot, lens, pk, sk, d_status
        ss = capi.SharingScheme(capi.SHARING_PACKED_SHAMIR, n, p, k, t, w2, w3)
        self.r, self.codec, self.box = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ok(lib.sda_secret_reconstructor_new(C.byref(ss), dim, C.byref(self.r)))
        self.ok(lib.sda_varint_codec_new(C.byref(self.codec)))
        self.ok(lib.sda_sealedbox_new(C.byref(self.box)))
        self.indices = (C.c_size_t * self.rows)(*indices)

    def ok(self, status):
        if status != 0:
            raise SystemExit(f"status {status}: {self.lib.sda_last_error().decode()}")

    def feed(self):
        self.ok(self.lib.sda_secret_reconstructor_update_sealed_rows_dev(self.r, self.codec, self.box, self.pk, self.sk, 0, self.boxes, self.slot,
                                                                         self.lens, self.rows, self.slot, None, self.d_status, None))

    def plain(self, d_out):
        self.ok(self.lib.sda_secret_reconstructor_begin_dev(self.r, self.indices, self.rows, self.B, None))
        self.feed()
        self.ok(self.lib.sda_secret_reconstructor_finish_dev(self.r, d_out, self.dim, None))

    def checked(self, checks, d_out, d_report):
        self.ok(self.lib.sda_secret_reconstructor_begin_checked_dev(self.r, self.indices, self.rows, self.B, checks, None))
        self.feed()
        self.kernels = self.lib.sda_debug_last_kernel().decode()
        self.ok(self.lib.sda_secret_reconstructor_finish_checked_dev(self.r, 1, d_out, self.dim, d_report, None))

    def free(self):
        self.lib.sda_secret_reconstructor_free(self.r)
        self.lib.sda_varint_codec_free(self.codec)
        self.lib.sda_sealedbox_free(self.box)


def child(shape, parent_lib):
    import numpy as np
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    scheme, indices = SHAPES[shape]
    p, k, t, n, w2, w3 = scheme
    dim, reps = int(os.environ.get("DIMENSION", str(1 << 20))), max(20, int(os.environ.get("REPS", "20")))
    capi.load()
    lib_b = open_library(capi.RELEASE_LIB_PATH, True)
    lib_a = open_library(parent_lib, False) if parent_lib else lib_b
    B = -(-dim // k)
    rows = len(indices)
    # clean rows: clerk sums of two participants' shares of random secrets (the generator of this tree), the job's positions only
    sharing = crypto.PackedShamir(k, n, t, p, w2, w3)
    gen = crypto.ShareGenerator(sharing)
    gen.set_drbg_key(bytes(range(32)))
    secrets = np.random.default_rng(rows).integers(0, p, size=(2, dim), dtype=np.int64)
    sums = None
    for q in range(2):
        sh = np.asarray(gen.generate(secrets[q]), dtype=np.int64)[list(indices)]
        sums = sh if sums is None else ((sums.astype(np.uint64) + sh.astype(np.uint64)) % np.uint64(p)).astype(np.int64)
    d_rows = DeviceBuffer.from_numpy(sums)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    sk = bytes(range(1, 33))
    pk = box.public_key(sk)
    slot = max(codec.slot_size(B), 16) + 48
    boxes, blen = DeviceBytes(rows * slot).zero(), DeviceBytes(rows * 8).zero()
    box.seal_share_rows_dev(codec, [pk], rows, d_rows.ptr, rows, B, B, boxes.ptr, slot, blen.ptr)
    synchronize()
    box_bytes = int(np.frombuffer(blen.to_bytes(), dtype="<u8").sum())
    status = DeviceBytes(4).zero()
    a = Job(lib_a, scheme, indices, dim, boxes.ptr, slot, blen.ptr, pk, sk, status.ptr)
    b = Job(lib_b, scheme, indices, dim, boxes.ptr, slot, blen.ptr, pk, sk, status.ptr)
    d_out, d_report = DeviceBuffer(dim).zero(), DeviceBuffer(4 + rows).zero()
    legs = {"A": lambda: a.plain(d_out.ptr), "B": lambda: b.plain(d_out.ptr)}
    for c in CHECKS:
        legs[f"C{c}"] = (lambda c=c: b.checked(c, d_out.ptr, d_report.ptr))
    names = list(legs)
    ms = {x: [] for x in names}
    for rep in range(-3, reps):                                  # three warm-up rounds
        order = names[rep % len(names):] + names[:rep % len(names)]      # the legs alternate, the order rotates
        for x in order:
            synchronize()
            t0 = time.perf_counter()
            legs[x]()
            synchronize()
            if rep >= 0:
                ms[x].append((time.perf_counter() - t0) * 1e3)
    want = DeviceBuffer(dim)
    crypto.SecretReconstructor(sharing, dim).reconstruct_dev(list(indices), d_rows.ptr, B, B, want.ptr, dim)
    want = want.to_numpy()
    truth = ((secrets[0].astype(np.uint64) + secrets[1].astype(np.uint64)) % np.uint64(p)).astype(np.int64)
    res = {"shape": shape, "rows": rows, "k": k, "t": t, "dimension": dim, "reps": reps, "sealed_bytes": box_bytes,
           "library_A": "built from the parent commit (--parent-lib)" if parent_lib else "this tree (no --parent-lib given)",
           "version_A": lib_a.sda_version().decode(), "kernel_id_A": lib_a.sda_kernel_id().decode(),
           "version_B": lib_b.sda_version().decode(), "kernel_id_B": lib_b.sda_kernel_id().decode(),
           "rows_reconstruct_to_the_secrets": bool(np.array_equal(want, truth)), "legs": {}}
    for x in names:
        d_out.zero()
        d_report.zero()
        legs[x]()
        v = sorted(ms[x])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        leg = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "verified": bool(np.array_equal(d_out.to_numpy(), want))}
        if x.startswith("C"):
            leg["report_clean"] = d_report.to_numpy()[:3].tolist() == [0, 0, 0] and not d_report.to_numpy()[4:].any()
            leg["kernels"] = b.kernels + " + reveal_check_finish_kernel"
        res["legs"][x] = leg
    res["status_word"] = int(np.frombuffer(status.to_bytes(), dtype="<u4")[0])
    a.free(); b.free()
    print("RESULT " + json.dumps(res))


def run_child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        raise SystemExit(f"child {args} ended with status {r.returncode}: nothing more is started")
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def verdict(a, b):
    if b["max_ms"] < a["min_ms"]:
        return "faster, beyond both spreads"
    if b["min_ms"] > a["max_ms"]:
        return "SLOWER, beyond both spreads"
    return "the spreads overlap: no difference shown"


def report(res):
    lines = ["recipient reconstruction from sealed clerking results, with and without parity checks; dimension 1 Mi unless DIMENSION says otherwise;",
             "host clock around the calls + synchronise, legs alternated in one process (rotating order), 3 warm-up rounds, clean rows",
             "A = begin_dev + update_sealed_rows_dev + finish_dev (parent commit's library), B = the same on this tree,",
             "Cn = begin_checked_dev(checks = n) + update_sealed_rows_dev + finish_checked_dev(SDA_CHECK_CORRECT) on this tree", ""]
    for shape, r in res.items():
        lines.append(f"[{shape}] {r['rows']} rows, k = {r['k']}, t = {r['t']}, dimension {r['dimension']}, {r['sealed_bytes']} sealed bytes, "
                     f"{r['reps']} repetitions; status word {r['status_word']}; rows reconstruct to the secrets: {r['rows_reconstruct_to_the_secrets']}")
        lines.append(f"  A on {r['library_A']}: {r['version_A']} kernel id {r['kernel_id_A']}")
        lines.append(f"  B, C on this tree: {r['version_B']} kernel id {r['kernel_id_B']}")
        a = r["legs"]["A"]
        for x, v in r["legs"].items():
            extra = f"  report clean {v['report_clean']}  ran {v['kernels']}" if x.startswith("C") else ""
            lines.append(f"  {x}: median {v['median_ms']:.3f} ms  ({v['min_ms']:.3f} - {v['max_ms']:.3f})  verified {v['verified']}{extra}")
        for x, v in r["legs"].items():
            if x != "A":
                lines.append(f"  {x} / A = {v['median_ms'] / a['median_ms']:.3f}; {verdict(a, v)}")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--parent-lib", default=None, help="libsda_hip.so built from the parent commit: leg A runs on it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r18"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.shape, os.path.abspath(a.parent_lib) if a.parent_lib else None)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {}
    for shape in ([a.shape] if a.shape else list(SHAPES)):
        res[shape] = run_child(["--shape", shape] + (["--parent-lib", a.parent_lib] if a.parent_lib else []), a.limit)
        with open(os.path.join(a.out_dir, "recipient_reveal_checked.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "recipient_reveal_checked.txt"), "w") as f:
            f.write(report(res))
    print(report(res))


if __name__ == "__main__":
    main()

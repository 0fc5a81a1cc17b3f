#!/usr/bin/env python3
"""The last step of the recipient's reveal (receive.rs:148-156) from the two device jobs' sums: the mask combiner's job and the
reconstructor's job are filled, then
    A  sda_secret_reconstructor_finish_dev + sda_mask_combiner_finish_dev + sda_secret_unmasker_unmask_dev, with the two
       intermediate buffers of 8 L bytes                                     (the chain, on a library built from the parent commit)
    B  sda_secret_unmasker_unmask_jobs_dev                                   (the one call, this tree)
Sharing k = 3, t = 1, n = 8 over the 62-bit prime, all 8 clerking results; shapes: a Full mask (4 participants) at dimension 1 Mi and
16 Mi, ChaCha (4 seeds) at 1 Mi.  Both jobs are filled once per repetition by plaintext update_dev calls OUTSIDE the timed region;
timed: the host clock around the call(s) and a device synchronise.  The legs alternate in one process (both libraries sit on the one
HIP runtime), 3 warm-up rounds, REPS >= 20 timed; median with (min - max).  The outputs of the two legs are compared at the timed
size, and the device bytes each leg newly holds after its first run are read from the allocator.
Every shape is a child process under its own time limit; a child that fails or runs out of time ends the whole measurement.
    --parent-lib PATH   libsda_hip.so built from the parent commit (leg A); without it leg A runs on this tree's library and says so
Writes recipient_unmask.json / .txt into --out-dir (default profiles/r17).  REPS overrides the repetitions."""
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
SHARING = (P62, 3, 1, 8, 631229665360524489, 3451275676410824977)
SHAPES = {"full-1Mi": ("full", 1 << 20), "full-16Mi": ("full", 1 << 24), "chacha-1Mi": ("chacha", 1 << 20)}
NEW = "sda_secret_unmasker_unmask_jobs_dev"
USED = ["sda_version", "sda_kernel_id", "sda_last_error", "sda_secret_unmasker_new", "sda_secret_unmasker_free", "sda_mask_combiner_new",
        "sda_mask_combiner_free", "sda_mask_combiner_begin_dev", "sda_mask_combiner_update_dev", "sda_mask_combiner_finish_dev",
        "sda_secret_reconstructor_new", "sda_secret_reconstructor_free", "sda_secret_reconstructor_begin_dev",
        "sda_secret_reconstructor_update_dev", "sda_secret_reconstructor_finish_dev", "sda_secret_unmasker_unmask_dev"]


def open_library(path, with_new):
    """a library by path with the signatures of the calls this tool makes (a parent-commit build lacks the new one)"""
    from sda_amd import capi
    lib = C.CDLL(path)
    for name in USED + ([NEW] if with_new else []):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = capi.SIGNATURES[name]
    return lib


class Jobs:
    """the three handles of one library and what fills their two jobs"""

    def __init__(self, lib, kind, dim, d_rows, stride, d_masks, mask_rows, mask_width):
        from sda_amd import capi
        self.lib, self.dim = lib, dim
        p, k, t, n, w2, w3 = SHARING
        self.n, self.B, self.stride = n, -(-dim // k), stride
        self.d_rows, self.d_masks, self.mask_rows, self.mask_width = d_rows, d_masks, mask_rows, mask_width
        ss = capi.SharingScheme(capi.SHARING_PACKED_SHAMIR, n, p, k, t, w2, w3)
        ms = capi.MaskingScheme(capi.MASKING_FULL, p, 0, 0) if kind == "full" else capi.MaskingScheme(capi.MASKING_CHACHA, p, dim, 128)
        self.u, self.c, self.r = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ok(lib.sda_secret_unmasker_new(C.byref(ms), C.byref(self.u)))
        self.ok(lib.sda_mask_combiner_new(C.byref(ms), C.byref(self.c)))
        self.ok(lib.sda_secret_reconstructor_new(C.byref(ss), dim, C.byref(self.r)))
        self.indices = (C.c_size_t * n)(*range(n))

    def ok(self, status):
        if status != 0:
            raise SystemExit(f"status {status}: {self.lib.sda_last_error().decode()}")

    def fill(self):
        lib = self.lib
        self.ok(lib.sda_secret_reconstructor_begin_dev(self.r, self.indices, self.n, self.B, None))
        self.ok(lib.sda_secret_reconstructor_update_dev(self.r, 0, self.d_rows, self.n, self.stride, None))
        self.ok(lib.sda_mask_combiner_begin_dev(self.c, self.dim, None))
        self.ok(lib.sda_mask_combiner_update_dev(self.c, self.d_masks, self.mask_rows, self.mask_width, self.mask_width, None))

    def chain(self, d_masked, d_mask, d_out):
        lib = self.lib
        self.ok(lib.sda_secret_reconstructor_finish_dev(self.r, d_masked, self.dim, None))
        self.ok(lib.sda_mask_combiner_finish_dev(self.c, d_mask, self.dim, None))
        self.ok(lib.sda_secret_unmasker_unmask_dev(self.u, d_mask, d_masked, self.dim, d_out, None))

    def one_call(self, d_out):
        self.ok(getattr(self.lib, NEW)(self.u, self.c, self.r, None, None, d_out, self.dim, None))

    def free(self):
        self.lib.sda_secret_unmasker_free(self.u)
        self.lib.sda_mask_combiner_free(self.c)
        self.lib.sda_secret_reconstructor_free(self.r)


def child(shape, parent_lib):
    import numpy as np
    from sda_amd import capi
    from sda_amd.device import DeviceBuffer, synchronize
    kind, dim = SHAPES[shape]
    reps = max(20, int(os.environ.get("REPS", "20")))
    this = capi.load()
    hooks = capi.hooks_library()                                 # sda_debug_mem_info
    lib_b = open_library(capi.RELEASE_LIB_PATH, True)
    lib_a = open_library(parent_lib, False) if parent_lib else lib_b
    p, k, t, n, w2, w3 = SHARING
    B = -(-dim // k)
    stride = B + (B & 1)
    d_rows = DeviceBuffer(n * stride)                            # clerking results: uniform residues, made on the device
    capi.check(this.sda_fill_synthetic_dev(d_rows.ptr, n, stride, stride, 0, 17, p, None))
    if kind == "full":
        mask_rows, mask_width = 4, dim
        d_masks = DeviceBuffer(mask_rows * dim)
        capi.check(this.sda_fill_synthetic_dev(d_masks.ptr, mask_rows, dim, dim, 100, 18, p, None))
    else:
        mask_rows, mask_width = 4, 4
        d_masks = DeviceBuffer.from_numpy(np.random.default_rng(19).integers(0, 1 << 32, size=(4, 4), dtype=np.int64))
    synchronize()
    a = Jobs(lib_a, kind, dim, d_rows.ptr, stride, d_masks.ptr, mask_rows, mask_width)
    b = Jobs(lib_b, kind, dim, d_rows.ptr, stride, d_masks.ptr, mask_rows, mask_width)
    out_a, out_b = DeviceBuffer(dim).zero(), DeviceBuffer(dim).zero()

    def free_now():
        synchronize()
        f, tot = C.c_size_t(), C.c_size_t()
        capi.check(hooks.sda_debug_mem_info(C.byref(f), C.byref(tot)))
        return f.value

    # what each leg newly holds: the jobs are filled first (their accumulators exist in both legs alike)
    a.fill(); b.fill()
    before = free_now()
    d_masked, d_mask = DeviceBuffer(dim), DeviceBuffer(dim)      # leg A's two intermediate buffers
    a.chain(d_masked.ptr, d_mask.ptr, out_a.ptr)
    held_a = before - free_now()
    before = free_now()
    b.one_call(out_b.ptr)
    held_b = before - free_now()
    legs = {"A": lambda: a.chain(d_masked.ptr, d_mask.ptr, out_a.ptr), "B": lambda: b.one_call(out_b.ptr)}
    fills = {"A": a.fill, "B": b.fill}
    ms = {"A": [], "B": []}
    for rep in range(-3, reps):                                  # three warm-up rounds
        for x in ("A", "B") if rep % 2 == 0 else ("B", "A"):
            fills[x]()
            synchronize()
            t0 = time.perf_counter()
            legs[x]()
            synchronize()
            if rep >= 0:
                ms[x].append((time.perf_counter() - t0) * 1e3)
    got_a, got_b = out_a.to_numpy(), out_b.to_numpy()
    same = bool(np.array_equal(got_a, got_b))
    sane = bool(((got_b >= 0) & (got_b < p)).all()) and len(set(got_b[:64].tolist())) > 32
    res = {"shape": shape, "masking": kind, "dimension": dim, "rows": n, "k": k, "reps": reps, "outputs_equal": same, "outputs_sane": sane,
           "library_A": "built from the parent commit (--parent-lib)" if parent_lib else "this tree (no --parent-lib given)",
           "version_A": lib_a.sda_version().decode(), "kernel_id_A": lib_a.sda_kernel_id().decode(),
           "version_B": lib_b.sda_version().decode(), "kernel_id_B": lib_b.sda_kernel_id().decode(), "legs": {}}
    for x, held in (("A", held_a), ("B", held_b)):
        v = sorted(ms[x])
        med = (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2
        res["legs"][x] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "device_bytes_newly_held": held}
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
        return "B is faster, beyond both spreads"
    if b["min_ms"] > a["max_ms"]:
        return "B is SLOWER, beyond both spreads"
    return "the spreads overlap: no difference shown"


def report(res):
    lines = ["recipient's last step from the two device jobs' sums; sharing k = 3, t = 1, n = 8 over the 62-bit prime; host clock around the call(s) +",
             "synchronise, jobs filled outside the timed region, legs alternated in one process, 3 warm-up rounds",
             "A = reconstructor finish_dev + mask combiner finish_dev + unmask_dev with two buffers of 8 L bytes; B = unmask_jobs_dev", ""]
    for shape, r in res.items():
        lines.append(f"[{shape}] {r['masking']} mask, dimension {r['dimension']}, {r['reps']} repetitions")
        lines.append(f"  A on {r['library_A']}: {r['version_A']} kernel id {r['kernel_id_A']}")
        lines.append(f"  B on this tree: {r['version_B']} kernel id {r['kernel_id_B']}")
        for x in ("A", "B"):
            v = r["legs"][x]
            lines.append(f"  {x}: median {v['median_ms']:.3f} ms  ({v['min_ms']:.3f} - {v['max_ms']:.3f})  device bytes newly held {v['device_bytes_newly_held']}")
        a, b = r["legs"]["A"], r["legs"]["B"]
        lines.append(f"  B / A = {b['median_ms'] / a['median_ms']:.3f}; {verdict(a, b)}")
        lines += [f"  outputs of A and B equal: {r['outputs_equal']}; in [0, q) and not constant: {r['outputs_sane']}", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--parent-lib", default=None, help="libsda_hip.so built from the parent commit: leg A runs on it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r17"))
    ap.add_argument("--limit", type=int, default=180, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.shape, a.parent_lib)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {}
    for shape in ([a.shape] if a.shape else list(SHAPES)):
        res[shape] = run_child(["--shape", shape] + (["--parent-lib", os.path.abspath(a.parent_lib)] if a.parent_lib else []), a.limit)
        with open(os.path.join(a.out_dir, "recipient_unmask.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "recipient_unmask.txt"), "w") as f:
            f.write(report(res) + "\n")
    print(report(res))


if __name__ == "__main__":
    main()

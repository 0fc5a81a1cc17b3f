#!/usr/bin/env python3
"""The erasure finish of a checked reconstruction job against what a caller had before it:
    A   clean rows.  A/parent = sda_secret_reconstructor_finish_decoded_dev of the PARENT commit's library (--parent-lib),
        A/new = sda_secret_reconstructor_finish_erasures_dev of this tree with d_ok all ones.  The timed unit is the finish call alone
        (job begun and fed by update_dev outside the timed region).
    B   one refused box (its tag byte flipped; update_sealed_rows_dev writes d_ok[r] = 0 and sets status bit 16).
        B/new    = finish_erasures_dev with the update's own d_ok, the finish call alone - the job is already fed;
        B/parent = what the parent's caller must do once the job is fed: download d_ok, begin_checked_dev without the row (checks - 1:
                   the surplus shrank by one), stream the remaining sealed rows again, finish_decoded_dev - all of it timed, on the
                   parent's library.
    C   f = checks refused boxes, which the parent cannot repair at all: finish_erasures_dev alone, the time only.
Shapes, dimension 1 Mi:
    config3   k = 3, t = 1, n = 8 over the 62-bit prime, all 8 rows, checks = 4
    config4   k = 8, t = 2, n = 26 over the 62-bit prime, all 26 rows, checks = 16
The legs alternate in one process, the order rotates, 3 warm-up rounds, REPS >= 20 timed; median with (min - max); host clock around the
calls + synchronise.  Every leg's output is compared with the secrets.  Every shape is a child process under its own time limit; a
child that fails or runs out of time ends the whole measurement.
Writes recipient_reveal_erasures.json / .txt into --out-dir (default profiles/r20).  DIMENSION / REPS override the shape."""
import argparse
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P62 = 4611686006577364993
SHAPES = {"config3": ((P62, 3, 1, 8, 631229665360524489, 3451275676410824977), 4),
          "config4": ((P62, 8, 2, 26, 2589100645267092065, 365137883145458390), 16)}


class ParentLibrary:
    """the parent commit's libsda_hip.so next to this tree's in one process: objects made inside made() belong to it for good"""

    def __init__(self, path):
        from sda_amd import capi
        self.capi, self.path = capi, os.path.abspath(path)
        self.lib = C.CDLL(self.path)
        for name, (res, args) in capi.SIGNATURES.items():
            fn = getattr(self.lib, name, None)                    # it lacks this tree's new entry points
            if fn is not None:
                fn.restype, fn.argtypes = res, args
        capi._loaded[self.path] = self.lib

    @contextlib.contextmanager
    def _active(self):
        before, self.capi._active_path = self.capi._active_path, self.path
        try:
            yield
        finally:
            self.capi._active_path = before

    def made(self, make):
        with self._active():
            obj = make()
        obj._lib = self.lib
        return obj

    def synchronize(self):
        assert self.lib.sda_dev_synchronize() == 0


def child(shape, parent_path):
    import numpy as np
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    (p, k, t, n, w2, w3), checks = SHAPES[shape]
    dim, reps = int(os.environ.get("DIMENSION", str(1 << 20))), max(20, int(os.environ.get("REPS", "20")))
    lib = capi.load()
    parent = ParentLibrary(parent_path)
    assert not hasattr(parent.lib, "sda_secret_reconstructor_finish_erasures_dev"), "--parent-lib is not the parent's library"
    B = -(-dim // k)
    indices = list(range(n))
    sharing = crypto.PackedShamir(k, n, t, p, w2, w3)
    gen = crypto.ShareGenerator(sharing)
    gen.set_drbg_key(bytes(range(32)))
    rng = np.random.default_rng(n)
    secrets = rng.integers(0, p, size=(2, dim), dtype=np.int64)
    sums = None
    for q in range(2):
        sh = np.asarray(gen.generate(secrets[q]), dtype=np.int64)
        sums = sh if sums is None else ((sums.astype(np.uint64) + sh.astype(np.uint64)) % np.uint64(p)).astype(np.int64)
    truth = ((secrets[0].astype(np.uint64) + secrets[1].astype(np.uint64)) % np.uint64(p)).astype(np.int64)
    d_rows = DeviceBuffer.from_numpy(sums)

    # the sealed clerking results, and copies with one / `checks` boxes whose tag byte is flipped
    sk = bytes(np.random.default_rng(7).integers(0, 256, 32, dtype=np.uint8))
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    pk = box.public_key(sk)
    slot = max(codec.slot_size(B), 16) + 48
    d_boxes, d_lens = DeviceBytes(n * slot).zero(), DeviceBytes(n * 8).zero()
    box.seal_share_rows_dev(codec, [pk], n, d_rows.ptr, n, B, B, d_boxes.ptr, slot, d_lens.ptr)
    synchronize()
    raw = bytearray(d_boxes.to_bytes())
    refused = {"one": [int(rng.integers(0, n))], "all": sorted(int(i) for i in rng.permutation(n)[:checks])}
    tampered = {}
    for which, liars in refused.items():
        bad = bytearray(raw)
        for r in liars:
            bad[r * slot + 37] ^= 0x40
        tampered[which] = DeviceBytes.from_bytes(bytes(bad))
    del raw

    rec = crypto.SecretReconstructor(sharing, dim)
    old = parent.made(lambda: crypto.SecretReconstructor(sharing, dim))
    old_codec, old_box = parent.made(crypto.VarintCodec), parent.made(crypto.SealedBox)
    d_out, d_report = DeviceBuffer(dim).zero(), DeviceBuffer(16 + n).zero()
    d_status, d_ok, d_ones = DeviceBytes(4).zero(), DeviceBytes(4 * n).zero(), DeviceBytes.from_bytes(b"\x01\x00\x00\x00" * n)
    legs = ["A/parent", "A/new", "B/parent", "B/new", "C/new"]
    kernels = {}

    def sealed_update(r, cdc, bx, d_b, first_pos, first_row, rows, ok):
        r.update_sealed_rows_dev(cdc, bx, pk, sk, first_pos, d_b.ptr + first_row * slot, slot, d_lens.ptr + 8 * first_row, rows, slot,
                                 d_status.ptr, ok)

    def feed_tampered(which):
        d_status.zero()
        d_ok.zero()
        rec.begin_checked_dev(indices, n, B, checks)
        sealed_update(rec, codec, box, tampered[which], 0, 0, n, d_ok.ptr)
        synchronize()

    def run(leg):
        """-> the milliseconds of the leg's timed unit"""
        if leg.startswith("A"):
            r = old if leg == "A/parent" else rec
            r.begin_checked_dev(indices, n, B, checks)
            r.update_dev(0, d_rows.ptr, n, B)
            synchronize()
            parent.synchronize()
            t0 = time.perf_counter()
            if leg == "A/parent":
                old.finish_decoded_dev(d_out.ptr, dim, d_report.ptr, 0, True)
                parent.synchronize()
            else:
                rec.finish_erasures_dev(d_ones.ptr, d_out.ptr, dim, d_report.ptr, 0, True)
                synchronize()
        elif leg == "B/parent":
            feed_tampered("one")                                  # the job the caller had streamed when the box was refused
            t0 = time.perf_counter()
            ok = np.frombuffer(d_ok.to_bytes(), dtype="<u4")      # the round trip
            keep = [i for i in range(n) if ok[i]]
            old.begin_checked_dev(keep, len(keep), B, checks - 1)
            start = 0
            while start < len(keep):                              # the remaining rows, one call per run of neighbours
                stop = start
                while stop + 1 < len(keep) and keep[stop + 1] == keep[stop] + 1:
                    stop += 1
                sealed_update(old, old_codec, old_box, tampered["one"], start, keep[start], stop - start + 1, 0)
                start = stop + 1
            old.finish_decoded_dev(d_out.ptr, dim, d_report.ptr, 0, True)
            parent.synchronize()
        else:
            feed_tampered("one" if leg == "B/new" else "all")
            t0 = time.perf_counter()
            rec.finish_erasures_dev(d_ok.ptr, d_out.ptr, dim, d_report.ptr, 0, True)
            synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if leg.endswith("new"):
            kernels[leg] = lib.sda_debug_last_kernel().decode()
        return ms
    ms = {leg: [] for leg in legs}
    for rep in range(-3, reps):                                  # three warm-up rounds
        order = legs[rep % len(legs):] + legs[:rep % len(legs)]          # the legs alternate, the order rotates
        for leg in order:
            v = run(leg)
            if rep >= 0:
                ms[leg].append(v)
    res = {"shape": shape, "rows": n, "k": k, "t": t, "checks": checks, "dimension": dim, "batches": B, "reps": reps,
           "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(),
           "parent_version": parent.lib.sda_version().decode(), "parent_kernel_id": parent.lib.sda_kernel_id().decode(),
           "refused_positions": refused, "legs": {}}
    for leg in legs:
        d_out.zero()
        d_report.zero()
        run(leg)
        words = [int(x) for x in d_report.to_numpy().view(np.uint64)]
        v = sorted(ms[leg])
        res["legs"][leg] = {"median_ms": (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, "min_ms": v[0], "max_ms": v[-1],
                            "verified": bool(np.array_equal(d_out.to_numpy(), truth)), "report_head": words[:8],
                            "status": int(np.frombuffer(d_status.to_bytes(), dtype="<u4")[0]) if leg[0] != "A" else 0,
                            "kernel": kernels.get(leg, "(the parent's library keeps no note here)")}
    for obj in (old, old_codec, old_box):
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


def verdict(a, b):
    if b["median_ms"] < a["min_ms"]:
        return "new's median lies BELOW the parent's spread (faster)"
    if b["median_ms"] > a["max_ms"]:
        return "new's median lies ABOVE the parent's spread (slower)"
    return "new's median lies inside the parent's spread: no difference shown"


def report(res):
    lines = ["the erasure finish of a checked reconstruction job; dimension 1 Mi unless DIMENSION says otherwise; host clock around the calls +",
             "synchronise, legs alternated in one process (rotating order), 3 warm-up rounds; SDA_CHECK_CORRECT, max_errors = 0",
             "A: clean rows, the finish alone - parent = finish_decoded_dev of the parent commit's library, new = finish_erasures_dev, d_ok all ones",
             "B: one refused box - new = finish_erasures_dev alone on the fed job; parent = download d_ok + begin_checked_dev without the row +",
             "   the remaining sealed rows streamed again + finish_decoded_dev, on the parent commit's library",
             "C: f = checks refused boxes - finish_erasures_dev alone (the parent cannot repair them)", ""]
    for shape, r in res.items():
        lines.append(f"[{shape}] {r['rows']} rows, k = {r['k']}, t = {r['t']}, checks = {r['checks']}, dimension {r['dimension']} ({r['batches']} batches), "
                     f"{r['reps']} repetitions; {r['version']} kernel id {r['kernel_id']}; parent {r['parent_version']} kernel id {r['parent_kernel_id']}")
        for x, v in r["legs"].items():
            lines.append(f"  {x:9s}: median {v['median_ms']:.3f} ms  ({v['min_ms']:.3f} - {v['max_ms']:.3f})  output = the secrets {v['verified']}  "
                         f"status {v['status']}  report {v['report_head']}  ran {v['kernel']}")
        for leg in ("A", "B"):
            a, b = r["legs"][leg + "/parent"], r["legs"][leg + "/new"]
            lines.append(f"  {leg}: new / parent = {b['median_ms'] / a['median_ms']:.4f}; {verdict(a, b)}")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--parent-lib", required=True, help="libsda_hip.so built from the parent commit")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r20"))
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.shape, a.parent_lib)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {}
    for shape in ([a.shape] if a.shape else list(SHAPES)):
        res[shape] = run_child(["--shape", shape, "--parent-lib", os.path.abspath(a.parent_lib)], a.limit)
        with open(os.path.join(a.out_dir, "recipient_reveal_erasures.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "recipient_reveal_erasures.txt"), "w") as f:
            f.write(report(res))
    print(report(res))


if __name__ == "__main__":
    main()

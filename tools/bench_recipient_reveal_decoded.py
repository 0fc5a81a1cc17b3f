#!/usr/bin/env python3
"""The finish of a checked reconstruction job, locating one position or decoding up to floor(checks / 2):
    A   sda_secret_reconstructor_finish_checked_dev (SDA_CHECK_CORRECT)   reveal_check_finish_kernel, unchanged by the decoder
    B   sda_secret_reconstructor_finish_decoded_dev (SDA_CHECK_CORRECT, max_errors = 0)   reveal_decode_finish_kernel
The timed unit is the finish call ALONE: every repetition begins a job (begin_checked_dev) and feeds it (update_dev, decoded rows in
HBM) outside the timed region, synchronises, then times the finish with the host clock up to the next synchronise.
Shapes, dimension 1 Mi:
    config3   k = 3, t = 1, n = 8 over the 62-bit prime, all 8 rows, checks = 4      (decodes up to 2)
    config4   k = 8, t = 2, n = 26 over the 62-bit prime, all 26 rows, checks = 16   (decodes up to 8)
Rows: clean (A, B), one whole faulty row (A, B), floor(checks / 2) whole faulty rows (B only: A cannot attribute them).
The legs alternate in one process, the order rotates, 3 warm-up rounds, REPS >= 20 timed; median with (min - max).  Every leg's
output is compared with the secrets, its report with what the planted rows imply.
Every shape is a child process under its own time limit; a child that fails or runs out of time ends the whole measurement.
Writes recipient_reveal_decoded.json / .txt into --out-dir (default profiles/r19).  DIMENSION / REPS override the shape."""
import argparse
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


def child(shape):
    import numpy as np
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, synchronize
    (p, k, t, n, w2, w3), checks = SHAPES[shape]
    dim, reps = int(os.environ.get("DIMENSION", str(1 << 20))), max(20, int(os.environ.get("REPS", "20")))
    lib = capi.load()
    B = -(-dim // k)
    indices = list(range(n))
    half = checks // 2
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
    liars = [int(i) for i in rng.permutation(n)[:half]]

    def spoiled(count):
        rows = sums.copy()
        for i in liars[:count]:
            err = rng.integers(1, p, size=B, dtype=np.int64)
            rows[i] = ((rows[i].astype(np.uint64) + err.astype(np.uint64)) % np.uint64(p)).astype(np.int64)
        return DeviceBuffer.from_numpy(rows)
    d_rows = {"clean": spoiled(0), "one": spoiled(1), "half": spoiled(half)}
    faulty = {"clean": 0, "one": 1, "half": half}
    rec = crypto.SecretReconstructor(sharing, dim)
    d_out, d_report = DeviceBuffer(dim).zero(), DeviceBuffer(16 + n).zero()
    legs = [("clean", "A"), ("clean", "B"), ("one", "A"), ("one", "B"), ("half", "B")]
    kernels = {}

    def run(rows, which):
        """-> the milliseconds of the finish alone"""
        rec.begin_checked_dev(indices, n, B, checks)
        rec.update_dev(0, d_rows[rows].ptr, n, B)
        synchronize()
        t0 = time.perf_counter()
        if which == "A":
            rec.finish_checked_dev(d_out.ptr, dim, d_report.ptr, True)
        else:
            rec.finish_decoded_dev(d_out.ptr, dim, d_report.ptr, 0, True)
        synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        kernels[which] = lib.sda_debug_last_kernel().decode()
        return ms
    ms = {leg: [] for leg in legs}
    for rep in range(-3, reps):                                  # three warm-up rounds
        order = legs[rep % len(legs):] + legs[:rep % len(legs)]          # the legs alternate, the order rotates
        for leg in order:
            v = run(*leg)
            if rep >= 0:
                ms[leg].append(v)
    res = {"shape": shape, "rows": n, "k": k, "t": t, "checks": checks, "dimension": dim, "batches": B, "reps": reps,
           "version": lib.sda_version().decode(), "kernel_id": lib.sda_kernel_id().decode(), "faulty_positions": liars, "legs": {}}
    for rows, which in legs:
        d_out.zero()
        d_report.zero()
        run(rows, which)
        words = [int(x) for x in d_report.to_numpy().view(np.uint64)]
        head, blame = (words[:4], words[4:4 + n]) if which == "A" else (words[:6], words[16:16 + n])
        want_blame = [B if i in liars[:faulty[rows]] else 0 for i in range(n)]
        fixed = 0 if rows == "clean" else B
        v = sorted(ms[(rows, which)])
        res["legs"][f"{rows}/{which}"] = {
            "median_ms": (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, "min_ms": v[0], "max_ms": v[-1],
            "verified": bool(np.array_equal(d_out.to_numpy(), truth)),
            "report_as_planted": head[:3] == [fixed, fixed, fixed] and blame == want_blame and (which == "A" or head[5] == faulty[rows]),
            "kernel": kernels[which]}
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
        return "B's median lies BELOW A's spread (faster)"
    if b["median_ms"] > a["max_ms"]:
        return "B's median lies ABOVE A's spread (slower)"
    return "B's median lies inside A's spread: no difference shown"


def report(res):
    lines = ["the finish of a checked reconstruction job alone (the job is begun and fed outside the timed region); dimension 1 Mi unless",
             "DIMENSION says otherwise; host clock around the call + synchronise, legs alternated in one process (rotating order), 3 warm-up rounds",
             "A = finish_checked_dev(SDA_CHECK_CORRECT), B = finish_decoded_dev(max_errors = 0, SDA_CHECK_CORRECT);",
             "rows: clean | one whole faulty row | half = floor(checks / 2) whole faulty rows (B only)", ""]
    for shape, r in res.items():
        lines.append(f"[{shape}] {r['rows']} rows, k = {r['k']}, t = {r['t']}, checks = {r['checks']}, dimension {r['dimension']} ({r['batches']} batches), "
                     f"{r['reps']} repetitions; {r['version']} kernel id {r['kernel_id']}")
        for x, v in r["legs"].items():
            lines.append(f"  {x:8s}: median {v['median_ms']:.3f} ms  ({v['min_ms']:.3f} - {v['max_ms']:.3f})  output = the secrets {v['verified']}  "
                         f"report as planted {v['report_as_planted']}  ran {v['kernel']}")
        for rows in ("clean", "one"):
            a, b = r["legs"][f"{rows}/A"], r["legs"][f"{rows}/B"]
            lines.append(f"  {rows}: B / A = {b['median_ms'] / a['median_ms']:.3f}; {verdict(a, b)}")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r19"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.shape)
    os.makedirs(a.out_dir, exist_ok=True)
    res = {}
    for shape in ([a.shape] if a.shape else list(SHAPES)):
        res[shape] = run_child(["--shape", shape], a.limit)
        with open(os.path.join(a.out_dir, "recipient_reveal_decoded.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out_dir, "recipient_reveal_decoded.txt"), "w") as f:
            f.write(report(res))
    print(report(res))


if __name__ == "__main__":
    main()

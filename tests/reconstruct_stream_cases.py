"""Cases of the reconstructor's streaming device job (sda_secret_reconstructor_begin_dev / update_dev / update_sealed_rows_dev /
finish_dev), shared by tests/test_reconstruct_stream_cpu.py (which reconstructs every case with the C oracle and proves, from a
model of the kernel's lockstep, which cases reach the global fallback) and tests/test_reconstruct_stream_gpu.py.

A case is a scheme, a dimension, the clerk index of every position, how the rows are made and how they are fed.  build(case)
makes its rows once (deterministic) and is cached; nothing here needs a device."""
import collections
import functools
import zlib

import numpy as np

P62 = 4611686006577364993
W62 = {8: 631229665360524489, 9: 3451275676410824977, 16: 2589100645267092065, 27: 365137883145458390}   # tests/test_parity_gpu.py
P31 = 2147482801                                                   # tests/test_path_select.py, tests/test_narrow_gpu.py
TSS_P, TSS_W2, TSS_W3 = 746497, 95660, 610121                      # tss's PSS_155_728_100, tests/test_parity_gpu.py:267

# name -> (p, k, t, n, omega_secrets, omega_shares); Additive: (q, 1, 0, n, 0, 0)
SCHEMES = {
    "k3_62": (P62, 3, 1, 8, W62[8], W62[9]),
    "k3_31": (P31, 3, 4, 8, 495332030, 1761729792),                 # tss-valid (3, 4, 8), tests/test_path_select.py:62
    "k8_62": (P62, 8, 2, 26, W62[16], W62[27]),
    "pss155": (TSS_P, 100, 155, 728, TSS_W2, TSS_W3),
    # a wide committee over the 62-bit prime: extremes.omegas(P62, 3, 1, 300) - any distinct nodes, all the library asks for
    # (tests/test_reveal_erasure_reach.py recomputes the two literals)
    "k3_wide": (P62, 3, 1, 300, 2177342806168468507, 4354685612336937012),
    "additive": (P62, 1, 0, 3, 0, 0),
}

KWINDOW = 2048          # output columns the kernel's LDS window holds (kCombWindow)
GROUP_BYTES = 4096      # a lockstep group: kStreamDepth = 4 chunks of 1 KiB
WG_ROWS = 8             # rows per workgroup of sealed_stream_weighted_kernel

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

# values: "sums" = clerk sums of 3 participants' shares; "crafted" = any-int64 rows; "drift" = one-byte rows next to ten-byte rows
# feed: "one" = one sealed call; "descending" = one position per sealed call, last first; "mixed" = sealed for the second half of
#       the positions, then plaintext update_dev for the first half; surplus = values every row holds past ceil(dimension / k)
Case = collections.namedtuple("Case", "name scheme dim indices values feed surplus")

ALL8 = tuple(range(8))
SCATTERED = (7, 0, 3, 5)                                            # exactly t + k rows of k3_62
PERMUTED = (3, 7, 5, 0)                                             # the same rows in another order
SEVEN = (7, 0, 3, 5, 1, 6, 2)                                       # exactly t + k rows of k3_31
PSS_255 = tuple((37 * i + 5) % 728 for i in range(255))             # exactly t + k rows of pss155, scattered (gcd(37, 728) = 1)


def _cases():
    out = []
    for dim in (1, 3, 4, 1000, 6301):
        out.append(Case(f"k3_62-all-d{dim}", "k3_62", dim, ALL8, "sums", "one", 0))
    out.append(Case("k3_62-scattered-d4", "k3_62", 4, SCATTERED, "sums", "one", 0))
    out.append(Case("k3_62-scattered-d1000", "k3_62", 1000, SCATTERED, "sums", "one", 0))
    out.append(Case("k3_62-permuted-d1000", "k3_62", 1000, PERMUTED, "sums", "one", 0))
    out.append(Case("k3_62-descending-d1000", "k3_62", 1000, ALL8, "sums", "descending", 0))
    out.append(Case("k3_62-mixed-d1000", "k3_62", 1000, SCATTERED, "sums", "mixed", 0))
    out.append(Case("k3_62-surplus-d1000", "k3_62", 1000, ALL8, "sums", "one", 29))
    out.append(Case("k3_62-surplus-mixed-d4", "k3_62", 4, PERMUTED, "sums", "mixed", 3))
    out.append(Case("k3_62-crafted-d1000", "k3_62", 1000, SCATTERED, "crafted", "one", 0))
    out.append(Case("k3_62-drift-d6301", "k3_62", 6301, SCATTERED, "drift", "one", 0))
    for dim in (1, 4, 1000):
        out.append(Case(f"k3_31-all-d{dim}", "k3_31", dim, ALL8, "sums", "one", 0))
    out.append(Case("k3_31-seven-d1000", "k3_31", 1000, SEVEN, "sums", "descending", 0))
    out.append(Case("k3_31-crafted-d4", "k3_31", 4, SEVEN, "crafted", "mixed", 0))
    out.append(Case("k8_62-all-d805", "k8_62", 805, tuple(range(26)), "sums", "one", 0))
    out.append(Case("k8_62-ten-d805", "k8_62", 805, (25, 0, 13, 7, 1, 19, 4, 22, 10, 16), "sums", "mixed", 2))
    out.append(Case("pss155-255rows-d250", "pss155", 250, PSS_255, "sums", "one", 0))
    out.append(Case("pss155-255rows-d1", "pss155", 1, PSS_255, "sums", "mixed", 0))
    # 30 batches = 3000 outputs: the k = 100 instance past its 2048-column window, 32 workgroups adding to the same outputs
    out.append(Case("pss155-255rows-d3000", "pss155", 3000, PSS_255, "sums", "one", 0))
    out.append(Case("additive-d1000", "additive", 1000, (0, 1, 2), "sums", "one", 0))
    out.append(Case("additive-mixed-d5", "additive", 5, (0, 1, 2), "sums", "mixed", 0))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
WIDE = "pss155-255rows-d3000"
DRIFT, LONG, PERMUTED_CASE, CRAFTED_CASE = "k3_62-drift-d6301", "k3_62-all-d6301", "k3_62-permuted-d1000", "k3_62-crafted-d1000"


def batches(case):
    p, k, t, n, w2, w3 = SCHEMES[case.scheme]
    return case.dim if case.scheme == "additive" else -(-case.dim // k)


def lagrange_matrix(p, k, w2, w3, indices):
    """R[e][i] of tss reconstruct in Python integers: nodes {1} U {w3^(idx + 1)}, the value at node 1 is 0, evaluated at w2^(e+1)"""
    nodes = [1] + [pow(w3, i + 1, p) for i in indices]
    R = []
    for e in range(k):
        x = pow(w2, e + 1, p)
        row = []
        for i in range(1, len(nodes)):
            num = den = 1
            for j in range(len(nodes)):
                if j != i:
                    num = num * (x - nodes[j]) % p
                    den = den * (nodes[i] - nodes[j]) % p
            row.append(num * pow(den, -1, p) % p)
        R.append(row)
    return R


def reconstruct_python(case, rows):
    """what the job must return for any-int64 rows, in Python integers mod q"""
    p, k, t, n, w2, w3 = SCHEMES[case.scheme]
    B = batches(case)
    if case.scheme == "additive":
        return np.array([sum(int(r[b]) for r in rows) % p for b in range(B)], dtype=np.int64)
    R = lagrange_matrix(p, k, w2, w3, case.indices)
    out = [sum(R[e][i] * (int(rows[i][b]) % p) for i in range(len(rows))) % p for b in range(B) for e in range(k)]
    return np.array(out[:case.dim], dtype=np.int64)


Built = collections.namedtuple("Built", "rows want row_len batches secrets_sum")


@functools.lru_cache(maxsize=None)
def build(name):
    """rows [positions][row_len] int64 (position i belongs to clerk indices[i]) and the secrets they reconstruct to"""
    from oracle import coracle
    case = BY_NAME[name]
    p, k, t, n, w2, w3 = SCHEMES[case.scheme]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    B = batches(case)
    row_len = B + case.surplus
    pos = len(case.indices)
    if case.values == "sums":
        parts = 3
        secrets = rng.integers(0, p, size=(parts, case.dim), dtype=np.int64)
        if case.scheme == "additive":
            shares = [coracle.additive_generate(p, n, secrets[q], rng.integers(0, p, size=case.dim * (n - 1), dtype=np.int64))
                      for q in range(parts)]
        else:
            shares = [coracle.packed_generate_systematic(p, k, t, n, w2, w3, secrets[q], rng.integers(0, p, size=B * t, dtype=np.int64))
                      for q in range(parts)]
        sums = np.stack([coracle.combine(p, np.stack([shares[q][c] for q in range(parts)])) for c in range(n)])   # clerk.rs:78-86
        rows = np.empty((pos, row_len), dtype=np.int64)
        rows[:, :B] = sums[list(case.indices)]
        rows[:, B:] = rng.integers(0, p, size=(pos, case.surplus), dtype=np.int64)       # decoded for validity, otherwise ignored
        want = (secrets.astype(object).sum(axis=0) % p).astype(np.int64)
        return Built(rows, want, row_len, B, want)
    if case.values == "crafted":
        special = np.array([I64_MIN, I64_MAX, -1, -p, p - 1, 0, p, 1, I64_MIN + 1, -p - 1], dtype=np.int64)
        rows = special[rng.integers(0, special.size, size=(pos, row_len))]
        rows[:, :special.size] = np.stack([np.roll(special, i) for i in range(pos)])[:, :min(special.size, row_len)]
    else:                                                            # drift: even positions all one-byte, odd all ten-byte values
        rows = np.empty((pos, row_len), dtype=np.int64)
        for i in range(pos):
            if i % 2 == 0:
                rows[i] = rng.integers(-64, 64, size=row_len, dtype=np.int64)
            else:
                big = rng.integers(1 << 62, I64_MAX, size=row_len, dtype=np.int64)
                rows[i] = np.where(rng.integers(0, 2, size=row_len) == 1, big, -big - 2)
    return Built(rows, reconstruct_python(case, rows), row_len, B, None)


# ---- model of the kernel's lockstep -------------------------------------------------------------------------------------------
def value_ends(payload):
    """byte offsets (exclusive) at which the values of a varint payload end"""
    b = np.frombuffer(payload, dtype=np.uint8)
    return np.flatnonzero(b < 0x80) + 1


def reach(case, payloads):
    """One sealed call over all positions.  A box's ciphertext starts 16-byte aligned, so chunk j of a row is its bytes
    [1024 j, 1024 j + 1024) and after g groups the row's column is the number of values that end inside its first 4096 g bytes.
    The 8 rows of a workgroup advance one group at a time; after each group the window base moves to the smallest output column
    any live row may still touch.  A product lands in the LDS window iff its output column is less than 2048 past the base, else
    it takes the direct global atomic.  -> counts of both, and what the rows crossed."""
    p, k, t, n, w2, w3 = SCHEMES[case.scheme]
    B = batches(case)
    total = B * k
    res = dict(window=0, beyond=0, wrapped=0, chunks=0, groups=0)
    for w0 in range(0, len(payloads), WG_ROWS):
        ends = [value_ends(pl) for pl in payloads[w0:w0 + WG_ROWS]]
        sizes = [len(pl) for pl in payloads[w0:w0 + WG_ROWS]]
        res["chunks"] = max(res["chunks"], max(-(-s // 1024) for s in sizes))
        res["groups"] = max(res["groups"], max(-(-s // GROUP_BYTES) for s in sizes))
        base, g = 0, 0
        cols = [0] * len(ends)
        while any(g * GROUP_BYTES < s for s in sizes):
            nxt = [int(np.searchsorted(e, (g + 1) * GROUP_BYTES, side="right")) for e in ends]
            for r in range(len(ends)):
                for b in range(cols[r], min(nxt[r], B)):
                    lo, hi = b * k, b * k + k                      # the k outputs of this value
                    inside = max(0, min(hi, base + KWINDOW) - lo)
                    res["window"] += inside
                    res["beyond"] += k - inside
                    if inside and hi - 1 >= KWINDOW:
                        res["wrapped"] += 1
            cols = nxt
            g += 1
            live = [g * GROUP_BYTES < s for s in sizes]
            base = min([min(c, B) * k if lv and c < B else total for c, lv in zip(cols, live)] + [total])
    return res

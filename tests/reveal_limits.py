"""The one-shot reveal (sda_secret_reconstructor_reconstruct_dev) over its shape space and at its sum limits - a helper module, not a
conftest, shared by tests/test_reveal_limits_reach.py (CPU) and tests/test_reveal_limits_gpu.py.

The reveal is three kernels behind a routing rule (sda_capi.cpp, sda_kernels.hip: packed_reconstruct_n31_available,
launch_packed_reconstruct_n31, launch_packed_reconstruct):
  * packed_reconstruct_n31_kernel<NMAX, GROUP> (narrow_gen.inc.hpp): p < 2^31, rows <= 16, k <= 16, both pointers 16-byte aligned,
    even row stride.  One signed 32-bit limb per residue, GROUP (16 below 2^29, else 4) products per signed 64-bit sum S, and
    n31_redc, which needs |S| < p 2^31 for its quotient t to lie in (-p, p).
  * packed_reconstruct_vec_kernel<NMAX> (sda_kernels.hip): the same layout conditions over any prime; 128-bit sums of canonical
    products, a conditional subtraction of p 2^64 every four terms.
  * packed_reconstruct_kernel: everything else, the k secrets of a batch split into `groups` of `e_per_group`.

This module holds
  * route(): the routing rule restated, giving the name sda_debug_last_reveal_kernel() reports and the dynamic LDS of the launch;
  * an integer model of each kernel in Python integers, every register checked against its width (model_n31, model_wide, and the
    lane / store / partition branches in coverage()), equal to the plain Python-integer Lagrange reconstruction (reference());
  * crafted rows, one kind per batch (KINDS), the target output row cycling so that every output row gets its worst batch;
  * CASES / REUSE: the instance grid, the batch and store edges, the grouped kernel's partition forms, the layout fallbacks and
    the handle-reuse sequences;
  * REACH: what the model records for every case - the largest |S| / (p 2^31) and |t| / p of the n31 kernel, the largest
    128-bit accumulator / (2 p 2^64) of the 64-bit kernels.  No test claims more than that table.

How far valid inputs stay below the proven bounds.  The n31 kernel: |constant|, |value| <= (p - 1) / 2, so |S| <= GROUP p^2 / 4 <
p 2^31 exactly because GROUP p < 2^33; sign-aligned rows reach 0.68 - 0.89 of p 2^31 at 2^31 - 1 with 7 or more rows and 0.51 - 0.67 just below
2^29 with 15 or 16 (16 terms), 0.13 - 0.23 just above (4 terms); the p - 1 / 0 / 1 rows of tests/test_extremes_gpu.py reach 2^-28 of it.  The
64-bit kernels: an accumulator below p 2^64 plus four products below p^2 stays below 2 p 2^64 exactly because p < 2^62 (the fraction
is at most 0.5 + 2 p / 2^64), with acc.hi < 2 p < 2^63; rows of p - 1 and the aligned rows reach up to 0.88 of 2 p 2^64 at the
62-bit moduli, while over a narrow prime the accumulator never gets near p 2^64 (0.0 at six places).  The model's width assertions are the proof that those bounds suffice."""
import functools
import random
import zlib

import numpy as np

import extremes as X
from reconstruct_stream_cases import I64_MAX, I64_MIN, lagrange_matrix

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
KTHREADS = 256                                   # kThreads: one workgroup of the register/LDS kernels covers 512 batches
P62 = X.P62
P31_ABOVE = 2147483659                           # the first prime above 2^31: must not take the narrow kernel
GRID_PRIMES = (X.PMAX, P62, X.P31MAX, P31_ABOVE, X.P29_ABOVE, X.P29_BELOW, X.NGEMM_PMAX, 433)
POISON = 0x5A5A5A5A5A5A5A5A                      # padding columns and the words around the rows: never read
CANARY = -0x0123456789ABCDEF                     # the words of `out` a reveal must not touch


def ceil_div(a, b):
    return -(-a // b)


# ---- routing ------------------------------------------------------------------------------------------------------------------------
def n31_group(p):
    return 16 if p < (1 << 29) else 4


def nmax_for(rows):
    return 4 if rows <= 4 else 8 if rows <= 8 else 16


def partition(k, batches):
    """launch_packed_reconstruct's split of a batch's k secrets: (blocks, groups, e_per_group)"""
    blocks = ceil_div(batches, KTHREADS)
    groups = min(ceil_div(2048, blocks) if blocks < 2048 else 1, k)
    e_per_group = ceil_div(k, groups)
    return blocks, ceil_div(k, e_per_group), e_per_group


def route(p, k, rows, shares_aligned, out_aligned, stride, batches, no_narrow=False):
    """(kernel name as sda_debug_last_reveal_kernel() reports it, dynamic LDS bytes of the launch)"""
    layout = rows <= 16 and k <= 16 and shares_aligned and out_aligned and stride % 2 == 0
    lds = 2 * KTHREADS * k * 8
    if p < (1 << 31) and not no_narrow and layout:
        return f"packed_reconstruct_n31_kernel<{nmax_for(rows)}, {n31_group(p)}>", lds
    if layout:
        return f"packed_reconstruct_vec_kernel<{nmax_for(rows)}>", lds
    _, groups, e_per_group = partition(k, batches)
    return f"packed_reconstruct_kernel groups={groups} e_per_group={e_per_group}", 0


# ---- the constants the host prepares (prepare_R, sda_capi.cpp) ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def roots(p, k, t, n):
    return X.omegas(p, k, t, n)


@functools.lru_cache(maxsize=None)
def matrix(p, k, t, n, indices):
    w2, w3 = roots(p, k, t, n)
    return lagrange_matrix(p, k, w2, w3, indices)


def r31(M, p):
    """R31: the centred representatives of M 2^32 mod p - int32 for a narrow prime (over a wide one only their signs are used, to
    give the crafted rows a pattern)"""
    out = [[X.centred(m * (1 << 32) % p, p) for m in row] for row in M]
    assert p >= (1 << 31) or all(-(1 << 31) <= c < (1 << 31) for row in out for c in row)
    return out


def rmont(M, p):
    """the Montgomery form (R = 2^64) of the 64-bit kernels, canonical"""
    return [[m * (1 << 64) % p for m in row] for row in M]


# ---- the device arithmetic, register by register ------------------------------------------------------------------------------------
def canon_i64(x, m):
    """canon_i64 / barrett_mod64 (modarith.hpp): any int64 -> [0, m)"""
    assert I64_MIN <= x <= I64_MAX and 2 <= m < (1 << 62)
    mu = (1 << 64) // m
    if 0 <= x < m:
        return x

    def barrett(v):
        assert 0 <= v <= 1 << 63
        qhat = (v * mu) >> 64
        r = v - qhat * m
        assert 0 <= r < 3 * m and r <= M64                  # the true quotient is qhat + 0, 1 or 2
        for _ in range(2):
            if r >= m:
                r -= m
        assert r == v % m
        return r
    if x >= 0:
        return barrett(x)
    r = barrett(-x)
    return 0 if r == 0 else m - r


def n31_centre(v, p):
    h = (p + 1) // 2
    x = v & M32
    assert x == v
    c = X.s32(x - p if x >= h else x)
    assert c == (v - p if v >= h else v) and abs(c) <= (p - 1) // 2
    return c


def n31_redc(S, p, pinv, stats):
    assert -(1 << 63) <= S < (1 << 63)
    assert abs(S) < p << 31                                 # what puts t into (-p, p)
    sl = S & M32
    sh = S >> 32
    assert -(1 << 31) <= sh < (1 << 31)
    q = X.s32(sl * pinv)                                    # a signed 32-bit value
    assert (S + q * p) & M32 == 0
    mulhi = (q * p) >> 32                                   # __mulhi: the floor
    assert -(1 << 31) <= mulhi < (1 << 31)
    t = sh + mulhi + (1 if sl != 0 else 0)
    assert -(1 << 31) <= t < (1 << 31) and t << 32 == S + q * p and -p < t < p
    stats["S"] = max(stats["S"], abs(S))
    stats["t"] = max(stats["t"], abs(t))
    t += p if t < 0 else 0                                  # the masked add
    assert 0 <= t < p
    return t


def model_n31(p, C31, values, stats):
    """one batch through packed_reconstruct_n31_kernel: C31 = R31 [k][rows], values = the batch's any-int64 column -> k secrets"""
    rows, G, NMAX = len(values), n31_group(p), nmax_for(len(values))
    pinv = (-pow(p, -1, 1 << 32)) & M32
    v = [n31_centre(canon_i64(x, p), p) for x in values] + [0] * (NMAX - rows)
    out = []
    for row in C31:
        r = 0
        for g0 in range(0, NMAX, G):
            if g0 >= rows:
                continue
            S = 0
            for c in range(g0, min(g0 + G, NMAX)):
                if c < rows:
                    S += row[c] * v[c]
                    assert -(1 << 63) <= S < (1 << 63)
            tq = n31_redc(S, p, pinv, stats)
            s = r + tq
            assert s <= M32
            d = (s - p) & M32
            nr = d if d < s else s
            assert nr == (r + tq) % p
            r = nr
        out.append(r)
    return out


def model_wide(p, Cm, values, stats):
    """one batch through the dot product of packed_reconstruct_vec_kernel / packed_reconstruct_kernel: Cm = Montgomery-form
    constants [k][rows]; mac128 of four products, mont_acc_condsub, mont_redc"""
    pinv = (-pow(p, -1, 1 << 64)) & M64
    v = [canon_i64(x, p) for x in values]
    out = []

    def condsub(lo, hi):
        acc = (hi << 64) | lo
        assert acc < (2 * p) << 64                          # below 2 p 2^64 before
        stats["acc"] = max(stats["acc"], acc)
        if hi >= p:
            hi -= p
        assert ((hi << 64) | lo) < p << 64                  # below p 2^64 after
        return hi
    for row in Cm:
        lo = hi = 0
        since = 0
        for m, x in zip(row, v):
            assert 0 <= m < p and 0 <= x < p
            prod = m * x
            nlo = (lo + (prod & M64)) & M64
            hi = hi + (prod >> 64) + (1 if nlo < lo else 0)
            assert hi <= M64                                # acc.hi inside 64 bits
            lo = nlo
            since += 1
            if since == 4:
                hi, since = condsub(lo, hi), 0
        hi = condsub(lo, hi)
        mq = (lo * pinv) & M64
        tq = hi + ((mq * p) >> 64) + (1 if lo != 0 else 0)
        assert tq <= M64 and tq << 64 == ((hi << 64) | lo) + mq * p and tq < 2 * p
        out.append(tq - p if tq >= p else tq)
    return out


# ---- crafted rows -------------------------------------------------------------------------------------------------------------------
KINDS = ("aligned", "opposed", "half_below", "half_above", "p_minus_1", "specials", "any_i64", "canonical")


def specials(p):
    return [I64_MIN, I64_MAX, -1, -p, p - 1, 0, p, 1, I64_MIN + 1, -p - 1]       # reconstruct_stream_cases' crafted values


@functools.lru_cache(maxsize=24)
def make_rows(name):
    """[rows][B] int64.  Batch b is of kind KINDS[b % 8] with target output row e = (b // 8) % k:
      aligned      row c holds the canonical form of sign(R31[e][c]) (p - 1) / 2: every group sum of output row e at its largest;
      opposed      the same with all signs flipped;
      half_below / half_above / p_minus_1   every row (p - 1) / 2, (p + 1) / 2, p - 1 (the last: the unsigned worst case);
      specials     the any-int64 specials, rolled per row;  any_i64 / canonical   random, seeded by the case's name.
    A case with `sample` keeps its any-int64 values in the first and last `sample` batches only (canonical elsewhere)."""
    case = BY_NAME[name]
    if case["rows_of"]:                                     # another case's rows, permuted like its indices
        src, perm = case["rows_of"]
        return make_rows(src)[list(perm)]
    p, k, B, idx = case["p"], case["k"], case["B"], case["indices"]
    rows = len(idx)
    C31 = r31(matrix(p, k, case["t"], case["n"], idx), p)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    h = (p - 1) // 2
    b = np.arange(B)
    kind, e = b % 8, (b // 8) % k
    aligned = np.array([[h if c >= 0 else p - h for c in row] for row in C31], dtype=np.int64)      # [k][rows]
    sp = np.array(specials(p), dtype=np.int64)
    out = np.empty((rows, B), dtype=np.int64)
    for c in range(rows):
        a = aligned[e, c]
        out[c] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6],
                           [a, p - a, h, p - h, p - 1, sp[(b // 8 + c) % sp.size],
                            rng.integers(I64_MIN, I64_MAX, size=B, dtype=np.int64, endpoint=True)],
                           rng.integers(0, p, size=B, dtype=np.int64))
    if case.get("sample") and B > 2 * case["sample"]:
        mid = slice(case["sample"], B - case["sample"])
        out[:, mid] = np.mod(out[:, mid], p)
    out.setflags(write=False)
    return out


def python_reconstruct(case, rows, batches=None):
    """the plain Lagrange reconstruction in Python integers, any-int64 inputs reduced with Python's %: [len(batches)][k]"""
    p, k = case["p"], case["k"]
    M = np.array(matrix(p, k, case["t"], case["n"], case["indices"]), dtype=object)
    cols = rows if batches is None else rows[:, batches]
    return (M.dot(cols.astype(object) % p) % p).T


@functools.lru_cache(maxsize=24)
def reference(name):
    """what the reveal must return, [dim] int64: Python integers for every batch; the large cases (`sample`) take the C oracle on
    the canonical form of the rows, and Python integers check their first and last `sample` batches, where the any-int64 rows are"""
    case = BY_NAME[name]
    p, k, B, dim = case["p"], case["k"], case["B"], case["dim"]
    rows = make_rows(name)
    if not case.get("sample"):
        return python_reconstruct(case, rows).reshape(-1)[:dim].astype(np.int64)
    from oracle import coracle
    w2, w3 = roots(p, k, case["t"], case["n"])
    want = coracle.packed_reconstruct(p, k, case["t"], w2, w3, dim, list(case["indices"]), np.mod(rows, p))
    s = case["sample"]
    sel = np.concatenate([np.arange(min(s, B)), np.arange(max(B - s, s), B)])
    py = python_reconstruct(case, rows, sel)
    full = np.zeros(B * k, dtype=np.int64)
    full[:dim] = want
    inside = sel[:, None] * k + np.arange(k) < dim
    assert np.array_equal(full.reshape(B, k)[sel][inside], py.astype(np.int64)[inside]), name
    return want


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def narrow_route(case):
    return case["kernel"].startswith("packed_reconstruct_n31")


def floor_for(p, rows):
    """the |S| / (p 2^31) the sign-aligned batches of a narrow case must reach (tests/test_reveal_limits_reach.py)"""
    if p == X.P31MAX and rows >= 7:
        return 0.6
    if p == X.P29_BELOW and rows >= 15:
        return 0.5
    return 0.0


def aligned_reach(p, C31):
    """|S| / (p 2^31) of the best sign-aligned group: values +-(p - 1) / 2 with the signs of one output row's constants"""
    G, h = n31_group(p), (p - 1) // 2
    return max(sum(abs(c) for c in row[g0:g0 + G]) * h for row in C31 for g0 in range(0, len(row), G)) / (p << 31)


@functools.lru_cache(maxsize=None)
def choose_indices(p, k, t, n, rows, salt=0):
    """a scattered, unsorted subset of `rows` clerk indices, drawn from a fixed sequence; where the case has an |S| floor the
    sequence is searched (on the CPU, against the host's constants - never against the device) until the floor holds"""
    floor = floor_for(p, rows) if p < (1 << 31) and rows <= 16 and k <= 16 else 0.0
    for attempt in range(400):
        idx = tuple(random.Random(f"{p}-{k}-{t}-{n}-{rows}-{salt}-{attempt}").sample(range(n), rows))
        if rows > 2 and list(idx) == sorted(idx):
            continue
        if floor == 0.0 or aligned_reach(p, r31(matrix(p, k, t, n, idx), p)) >= floor:
            return idx
    raise ValueError(f"no index subset reaches {floor} of the bound for p = {p}, ({k}, {t}), {rows} rows")


def _case(name, p, k, t, n, rows, B, dim, stride=None, shares_off=0, out_off=0, pad=0, sample=0, twin=False, indices=None, rows_of=None):
    stride = B + (B & 1) + pad if stride is None else stride
    idx = indices or choose_indices(p, k, t, n, rows)
    kernel, lds = route(p, k, rows, shares_off == 0, out_off == 0, stride, B)
    return dict(name=name, p=p, k=k, t=t, n=n, indices=idx, B=B, dim=dim, stride=stride, shares_off=shares_off, out_off=out_off,
                sample=sample, twin=twin and p < (1 << 31), kernel=kernel, lds=lds, rows_of=rows_of)


GRID_SHAPES = [(1, 1, 0, 5), (3, 1, 2, 7), (4, 1, 3, 8), (4, 3, 1, 8), (4, 4, 0, 8), (5, 2, 3, 9), (7, 3, 4, 11), (8, 3, 5, 12),
               (8, 8, 0, 12), (8, 3, 1, 8), (9, 4, 5, 13), (15, 8, 7, 19), (16, 8, 8, 20), (16, 1, 15, 20), (16, 15, 1, 20),
               (16, 16, 0, 20), (17, 16, 1, 21), (17, 17, 0, 21)]                     # (rows, k, t, n); (8, 3, 1, 8): surplus rows


def _cases():
    out = []
    B = 1030                                                                         # two whole workgroups and a ragged one
    for p in GRID_PRIMES:
        for rows, k, t, n in GRID_SHAPES:
            out.append(_case(f"grid-p{p}-k{k}t{t}-r{rows}", p, k, t, n, rows, B, B * k - (k - 1), twin=True))
    for p in (P62, X.P31MAX):
        for rows, k, t, n in ((4, 3, 1, 8), (7, 3, 4, 11), (16, 16, 0, 20)):
            for B in (1, 2, 3, 511, 512, 513):
                for dim in sorted({B * k, B * k - 1, B * k - (k - 1)}):
                    out.append(_case(f"edge-p{p}-k{k}t{t}-r{rows}-B{B}-d{dim}", p, k, t, n, rows, B, dim))
        # the grouped kernel's partition of the k secrets: 9 groups of 2 (the last holds one secret), 2 groups of 2 (the last holds
        # one), a single group (blocks >= 2048), 7 groups of 3 (the last holds two)
        out.append(_case(f"part-p{p}-k17t0-B32763", p, 17, 0, 21, 17, 32763, 32763 * 17 - 16, sample=1000))
        out.append(_case(f"part-p{p}-k3t1-odd-B262100", p, 3, 1, 8, 4, 262100, 262100 * 3 - 2, stride=262101, sample=1000))
        out.append(_case(f"part-p{p}-k3t1-odd-B524289", p, 3, 1, 8, 4, 524289, 524289 * 3 - 2, stride=524289, sample=1000))
        out.append(_case(f"part-p{p}-k20t13-B76600", p, 20, 13, 37, 33, 76600, 76600 * 20 - 19, sample=1000))
        # layouts the register/LDS kernels cannot take (-> grouped), and one they can: an even stride with poisoned padding
        Bl = 1030
        for tag, kw in (("shares8", dict(shares_off=1)), ("out8", dict(out_off=1)), ("odd", dict(stride=Bl | 1)), ("padded", dict(pad=6))):
            out.append(_case(f"layout-p{p}-k8t7-{tag}", p, 8, 7, 19, 15, Bl, Bl * 8 - 7, **kw))
    return out


def _reuse():
    """one handle, five calls: index set A, another set of the same length, A again, A with one more row, A permuted (rows alike)"""
    out = {}
    for p in (P62, X.P31MAX):
        k, t, n, B = 3, 4, 12, 300
        dim = B * k - 1
        A = choose_indices(p, k, t, n, 7)
        other = choose_indices(p, k, t, n, 7, salt=1)
        assert set(other) != set(A)
        reach = lambda idx: p >= (1 << 31) or aligned_reach(p, r31(matrix(p, k, t, n, idx), p)) >= floor_for(p, len(idx))
        more = next(A + (i,) for i in range(n) if i not in A and reach(A + (i,)))       # searched like choose_indices
        order = (3, 6, 0, 5, 1, 4, 2)
        perm = tuple(A[i] for i in order)
        assert reach(perm)
        out[p] = [_case(f"reuse-p{p}-{tag}", p, k, t, n, len(idx), B, dim, indices=idx, rows_of=(f"reuse-p{p}-A", order) if tag == "A-permuted" else None)
                  for tag, idx in (("A", A), ("other", other), ("A-again", A), ("A-plus-one", more), ("A-permuted", perm))]
    return out


CASES = _cases()
REUSE = _reuse()
BY_NAME = {c["name"]: c for c in CASES + [c for steps in REUSE.values() for c in steps]}
assert len(BY_NAME) == len(CASES) + sum(len(s) for s in REUSE.values())


# ---- what a case runs ---------------------------------------------------------------------------------------------------------------
def model_batches(case):
    """the batches the CPU model runs: every sign-aligned and sign-opposed batch of the first cycle over the output rows, one
    batch of every kind, and the last two"""
    B, k = case["B"], case["k"]
    want = {b for b in range(min(B, 8 * k)) if b % 8 < 2} | set(range(min(B, 16))) | {B - 1, max(B - 2, 0)}
    return sorted(want)


def run_model(case):
    """({batch: [k secrets]}, maxima) - the kernel the route names"""
    p, k = case["p"], case["k"]
    M = matrix(p, k, case["t"], case["n"], case["indices"])
    rows = make_rows(case["name"])
    stats = dict(S=0, t=0, acc=0)
    narrow = narrow_route(case)
    C = r31(M, p) if narrow else rmont(M, p)
    out = {}
    for b in model_batches(case):
        col = [int(x) for x in rows[:, b]]
        out[b] = (model_n31 if narrow else model_wide)(p, C, col, stats)
    return out, stats


def coverage(case):
    """the branches of the launcher and the kernel this case runs, by name"""
    p, k, B, dim, rows = case["p"], case["k"], case["B"], case["dim"], len(case["indices"])
    got = {case["kernel"]}
    if case["kernel"].startswith("packed_reconstruct_kernel"):
        _, groups, epg = partition(k, B)
        got.add("groups=1" if groups == 1 else "e_per_group=1" if epg == 1 else "e_per_group>1")
        if epg > 1 and k % epg:
            got.add("short last group")
        if dim < B * k:
            got.add("truncated batch")
        return got
    lanes = ceil_div(B, 2)
    vblocks = ceil_div(lanes, KTHREADS)
    got.add(f"lds={case['lds']}")
    if B >= 2:
        got.add("load pair")
    if B & 1:
        got.add("load single")
    if vblocks * KTHREADS > lanes:
        got.add("idle lane")
    slots = vblocks * KTHREADS * k                          # two-element store slots of the grid
    if dim >= 2:
        got.add("store pair")
    if dim & 1:
        got.add("store single")
    if slots > ceil_div(dim, 2):
        got.add("store nothing")
    if vblocks > 1:
        got.add("more than one workgroup")
    return got


def fractions(case, stats):
    """the maxima as fractions of their bounds, cut to six places (never rounded up)"""
    p = case["p"]
    cut = lambda num, den: (num * 10 ** 6 // den) / 10 ** 6
    if narrow_route(case):
        return (cut(stats["S"], p << 31), cut(stats["t"], p))
    return (cut(stats["acc"], (2 * p) << 64),)


def print_reach():
    for c in CASES + [c for steps in REUSE.values() for c in steps]:
        print(f'    "{c["name"]}": {fractions(c, run_model(c)[1])},')


# ---- recorded reach -----------------------------------------------------------------------------------------------------------------
# Per case, over its modelled batches: n31 cases (|S| / (p 2^31), |t| / p); 64-bit cases (accumulator / (2 p 2^64),).
# tests/test_reveal_limits_reach.py asserts the table exactly (seeded inputs, integer arithmetic); print_reach() regenerates it.
REACH = {
    "grid-p4611686018427387847-k1t0-r1": (0.091254,),
    "grid-p4611686018427387847-k1t2-r3": (0.223156,),
    "grid-p4611686018427387847-k1t3-r4": (0.248385,),
    "grid-p4611686018427387847-k3t1-r4": (0.28067,),
    "grid-p4611686018427387847-k4t0-r4": (0.411778,),
    "grid-p4611686018427387847-k2t3-r5": (0.332307,),
    "grid-p4611686018427387847-k3t4-r7": (0.541296,),
    "grid-p4611686018427387847-k3t5-r8": (0.437815,),
    "grid-p4611686018427387847-k8t0-r8": (0.691463,),
    "grid-p4611686018427387847-k3t1-r8": (0.559885,),
    "grid-p4611686018427387847-k4t5-r9": (0.654308,),
    "grid-p4611686018427387847-k8t7-r15": (0.806245,),
    "grid-p4611686018427387847-k8t8-r16": (0.724535,),
    "grid-p4611686018427387847-k1t15-r16": (0.545354,),
    "grid-p4611686018427387847-k15t1-r16": (0.853775,),
    "grid-p4611686018427387847-k16t0-r16": (0.773435,),
    "grid-p4611686018427387847-k16t1-r17": (0.794167,),
    "grid-p4611686018427387847-k17t0-r17": (0.828777,),
    "grid-p4611686006577364993-k1t0-r1": (0.006475,),
    "grid-p4611686006577364993-k1t2-r3": (0.205901,),
    "grid-p4611686006577364993-k1t3-r4": (0.20436,),
    "grid-p4611686006577364993-k3t1-r4": (0.363243,),
    "grid-p4611686006577364993-k4t0-r4": (0.259613,),
    "grid-p4611686006577364993-k2t3-r5": (0.401721,),
    "grid-p4611686006577364993-k3t4-r7": (0.580207,),
    "grid-p4611686006577364993-k3t5-r8": (0.587311,),
    "grid-p4611686006577364993-k8t0-r8": (0.63697,),
    "grid-p4611686006577364993-k3t1-r8": (0.554813,),
    "grid-p4611686006577364993-k4t5-r9": (0.749929,),
    "grid-p4611686006577364993-k8t7-r15": (0.872614,),
    "grid-p4611686006577364993-k8t8-r16": (0.753538,),
    "grid-p4611686006577364993-k1t15-r16": (0.803367,),
    "grid-p4611686006577364993-k15t1-r16": (0.765285,),
    "grid-p4611686006577364993-k16t0-r16": (0.773056,),
    "grid-p4611686006577364993-k16t1-r17": (0.80823,),
    "grid-p4611686006577364993-k17t0-r17": (0.793475,),
    "grid-p2147483647-k1t0-r1": (0.189262, 0.442119),
    "grid-p2147483647-k1t2-r3": (0.417485, 0.438557),
    "grid-p2147483647-k1t3-r4": (0.483286, 0.484813),
    "grid-p2147483647-k3t1-r4": (0.747655, 0.715209),
    "grid-p2147483647-k4t0-r4": (0.717437, 0.614501),
    "grid-p2147483647-k2t3-r5": (0.668056, 0.415971),
    "grid-p2147483647-k3t4-r7": (0.697263, 0.743634),
    "grid-p2147483647-k3t5-r8": (0.783734, 0.608132),
    "grid-p2147483647-k8t0-r8": (0.738, 0.749163),
    "grid-p2147483647-k3t1-r8": (0.761907, 0.600038),
    "grid-p2147483647-k4t5-r9": (0.692494, 0.682876),
    "grid-p2147483647-k8t7-r15": (0.886188, 0.85338),
    "grid-p2147483647-k8t8-r16": (0.801425, 0.743976),
    "grid-p2147483647-k1t15-r16": (0.685669, 0.626446),
    "grid-p2147483647-k15t1-r16": (0.859703, 0.748406),
    "grid-p2147483647-k16t0-r16": (0.869442, 0.815278),
    "grid-p2147483647-k16t1-r17": (0.0,),
    "grid-p2147483647-k17t0-r17": (0.0,),
    "grid-p2147483659-k1t0-r1": (0.0,),
    "grid-p2147483659-k1t2-r3": (0.0,),
    "grid-p2147483659-k1t3-r4": (0.0,),
    "grid-p2147483659-k3t1-r4": (0.0,),
    "grid-p2147483659-k4t0-r4": (0.0,),
    "grid-p2147483659-k2t3-r5": (0.0,),
    "grid-p2147483659-k3t4-r7": (0.0,),
    "grid-p2147483659-k3t5-r8": (0.0,),
    "grid-p2147483659-k8t0-r8": (0.0,),
    "grid-p2147483659-k3t1-r8": (0.0,),
    "grid-p2147483659-k4t5-r9": (0.0,),
    "grid-p2147483659-k8t7-r15": (0.0,),
    "grid-p2147483659-k8t8-r16": (0.0,),
    "grid-p2147483659-k1t15-r16": (0.0,),
    "grid-p2147483659-k15t1-r16": (0.0,),
    "grid-p2147483659-k16t0-r16": (0.0,),
    "grid-p2147483659-k16t1-r17": (0.0,),
    "grid-p2147483659-k17t0-r17": (0.0,),
    "grid-p536870923-k1t0-r1": (0.032001, 0.439063),
    "grid-p536870923-k1t2-r3": (0.075774, 0.332741),
    "grid-p536870923-k1t3-r4": (0.147359, 0.520324),
    "grid-p536870923-k3t1-r4": (0.144601, 0.520109),
    "grid-p536870923-k4t0-r4": (0.149647, 0.491679),
    "grid-p536870923-k2t3-r5": (0.175419, 0.492901),
    "grid-p536870923-k3t4-r7": (0.15159, 0.493658),
    "grid-p536870923-k3t5-r8": (0.160758, 0.494716),
    "grid-p536870923-k8t0-r8": (0.173605, 0.543783),
    "grid-p536870923-k3t1-r8": (0.157026, 0.504157),
    "grid-p536870923-k4t5-r9": (0.177802, 0.513763),
    "grid-p536870923-k8t7-r15": (0.224163, 0.550149),
    "grid-p536870923-k8t8-r16": (0.192001, 0.514713),
    "grid-p536870923-k1t15-r16": (0.132905, 0.523086),
    "grid-p536870923-k15t1-r16": (0.216033, 0.569884),
    "grid-p536870923-k16t0-r16": (0.218452, 0.550097),
    "grid-p536870923-k16t1-r17": (0.0,),
    "grid-p536870923-k17t0-r17": (0.0,),
    "grid-p536870909-k1t0-r1": (0.033541, 0.457133),
    "grid-p536870909-k1t2-r3": (0.12413, 0.418114),
    "grid-p536870909-k1t3-r4": (0.167038, 0.34716),
    "grid-p536870909-k3t1-r4": (0.097507, 0.434754),
    "grid-p536870909-k4t0-r4": (0.097507, 0.46523),
    "grid-p536870909-k2t3-r5": (0.196446, 0.446425),
    "grid-p536870909-k3t4-r7": (0.260105, 0.514405),
    "grid-p536870909-k3t5-r8": (0.32233, 0.612944),
    "grid-p536870909-k8t0-r8": (0.332226, 0.588836),
    "grid-p536870909-k3t1-r8": (0.303268, 0.431969),
    "grid-p536870909-k4t5-r9": (0.32036, 0.592439),
    "grid-p536870909-k8t7-r15": (0.627823, 0.713294),
    "grid-p536870909-k8t8-r16": (0.663436, 0.806665),
    "grid-p536870909-k1t15-r16": (0.516577, 0.410485),
    "grid-p536870909-k15t1-r16": (0.659279, 0.625871),
    "grid-p536870909-k16t0-r16": (0.591649, 0.747698),
    "grid-p536870909-k16t1-r17": (0.0,),
    "grid-p536870909-k17t0-r17": (0.0,),
    "grid-p8355691-k1t0-r1": (0.000532, 0.494961),
    "grid-p8355691-k1t2-r3": (0.001783, 0.466582),
    "grid-p8355691-k1t3-r4": (0.002042, 0.42512),
    "grid-p8355691-k3t1-r4": (0.002195, 0.500388),
    "grid-p8355691-k4t0-r4": (0.002319, 0.47431),
    "grid-p8355691-k2t3-r5": (0.002707, 0.428418),
    "grid-p8355691-k3t4-r7": (0.003982, 0.498636),
    "grid-p8355691-k3t5-r8": (0.003097, 0.488107),
    "grid-p8355691-k8t0-r8": (0.006413, 0.49354),
    "grid-p8355691-k3t1-r8": (0.004651, 0.490467),
    "grid-p8355691-k4t5-r9": (0.005506, 0.48893),
    "grid-p8355691-k8t7-r15": (0.009332, 0.499146),
    "grid-p8355691-k8t8-r16": (0.008644, 0.49473),
    "grid-p8355691-k1t15-r16": (0.008972, 0.474327),
    "grid-p8355691-k15t1-r16": (0.00974, 0.498172),
    "grid-p8355691-k16t0-r16": (0.009865, 0.501039),
    "grid-p8355691-k16t1-r17": (0.0,),
    "grid-p8355691-k17t0-r17": (0.0,),
    "grid-p433-k1t0-r1": (0.0, 0.47806),
    "grid-p433-k1t2-r3": (0.0, 0.443418),
    "grid-p433-k1t3-r4": (0.0, 0.459584),
    "grid-p433-k3t1-r4": (0.0, 0.480369),
    "grid-p433-k4t0-r4": (0.0, 0.496535),
    "grid-p433-k2t3-r5": (0.0, 0.471131),
    "grid-p433-k3t4-r7": (0.0, 0.489607),
    "grid-p433-k3t5-r8": (0.0, 0.496535),
    "grid-p433-k8t0-r8": (0.0, 0.491916),
    "grid-p433-k3t1-r8": (0.0, 0.498845),
    "grid-p433-k4t5-r9": (0.0, 0.482678),
    "grid-p433-k8t7-r15": (0.0, 0.498845),
    "grid-p433-k8t8-r16": (0.0, 0.496535),
    "grid-p433-k1t15-r16": (0.0, 0.43187),
    "grid-p433-k15t1-r16": (0.0, 0.496535),
    "grid-p433-k16t0-r16": (0.0, 0.498845),
    "grid-p433-k16t1-r17": (0.0,),
    "grid-p433-k17t0-r17": (0.0,),
    "edge-p4611686006577364993-k3t1-r4-B1-d1": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B1-d2": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B1-d3": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B2-d4": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B2-d5": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B2-d6": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B3-d7": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B3-d8": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B3-d9": (0.181621,),
    "edge-p4611686006577364993-k3t1-r4-B511-d1531": (0.363243,),
    "edge-p4611686006577364993-k3t1-r4-B511-d1532": (0.363243,),
    "edge-p4611686006577364993-k3t1-r4-B511-d1533": (0.363243,),
    "edge-p4611686006577364993-k3t1-r4-B512-d1534": (0.363243,),
    "edge-p4611686006577364993-k3t1-r4-B512-d1535": (0.363243,),
    "edge-p4611686006577364993-k3t1-r4-B512-d1536": (0.363243,),
    "edge-p4611686006577364993-k3t1-r4-B513-d1537": (0.363243,),
    "edge-p4611686006577364993-k3t1-r4-B513-d1538": (0.363243,),
    "edge-p4611686006577364993-k3t1-r4-B513-d1539": (0.363243,),
    "edge-p4611686006577364993-k3t4-r7-B1-d1": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B1-d2": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B1-d3": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B2-d4": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B2-d5": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B2-d6": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B3-d7": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B3-d8": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B3-d9": (0.290103,),
    "edge-p4611686006577364993-k3t4-r7-B511-d1531": (0.580207,),
    "edge-p4611686006577364993-k3t4-r7-B511-d1532": (0.580207,),
    "edge-p4611686006577364993-k3t4-r7-B511-d1533": (0.580207,),
    "edge-p4611686006577364993-k3t4-r7-B512-d1534": (0.580207,),
    "edge-p4611686006577364993-k3t4-r7-B512-d1535": (0.580207,),
    "edge-p4611686006577364993-k3t4-r7-B512-d1536": (0.580207,),
    "edge-p4611686006577364993-k3t4-r7-B513-d1537": (0.580207,),
    "edge-p4611686006577364993-k3t4-r7-B513-d1538": (0.580207,),
    "edge-p4611686006577364993-k3t4-r7-B513-d1539": (0.580207,),
    "edge-p4611686006577364993-k16t0-r16-B1-d1": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B1-d15": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B1-d16": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B2-d17": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B2-d31": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B2-d32": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B3-d33": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B3-d47": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B3-d48": (0.577606,),
    "edge-p4611686006577364993-k16t0-r16-B511-d8161": (0.773056,),
    "edge-p4611686006577364993-k16t0-r16-B511-d8175": (0.773056,),
    "edge-p4611686006577364993-k16t0-r16-B511-d8176": (0.773056,),
    "edge-p4611686006577364993-k16t0-r16-B512-d8177": (0.773056,),
    "edge-p4611686006577364993-k16t0-r16-B512-d8191": (0.773056,),
    "edge-p4611686006577364993-k16t0-r16-B512-d8192": (0.773056,),
    "edge-p4611686006577364993-k16t0-r16-B513-d8193": (0.792811,),
    "edge-p4611686006577364993-k16t0-r16-B513-d8207": (0.773056,),
    "edge-p4611686006577364993-k16t0-r16-B513-d8208": (0.773056,),
    "part-p4611686006577364993-k17t0-B32763": (0.793475,),
    "part-p4611686006577364993-k3t1-odd-B262100": (0.363243,),
    "part-p4611686006577364993-k3t1-odd-B524289": (0.363243,),
    "part-p4611686006577364993-k20t13-B76600": (0.867007,),
    "layout-p4611686006577364993-k8t7-shares8": (0.872614,),
    "layout-p4611686006577364993-k8t7-out8": (0.872614,),
    "layout-p4611686006577364993-k8t7-odd": (0.872614,),
    "layout-p4611686006577364993-k8t7-padded": (0.872614,),
    "edge-p2147483647-k3t1-r4-B1-d1": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B1-d2": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B1-d3": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B2-d4": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B2-d5": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B2-d6": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B3-d7": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B3-d8": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B3-d9": (0.747655, 0.626172),
    "edge-p2147483647-k3t1-r4-B511-d1531": (0.747655, 0.715209),
    "edge-p2147483647-k3t1-r4-B511-d1532": (0.747655, 0.73243),
    "edge-p2147483647-k3t1-r4-B511-d1533": (0.747655, 0.715209),
    "edge-p2147483647-k3t1-r4-B512-d1534": (0.747655, 0.715209),
    "edge-p2147483647-k3t1-r4-B512-d1535": (0.747655, 0.715209),
    "edge-p2147483647-k3t1-r4-B512-d1536": (0.747655, 0.715209),
    "edge-p2147483647-k3t1-r4-B513-d1537": (0.747655, 0.715209),
    "edge-p2147483647-k3t1-r4-B513-d1538": (0.747655, 0.715209),
    "edge-p2147483647-k3t1-r4-B513-d1539": (0.747655, 0.715209),
    "edge-p2147483647-k3t4-r7-B1-d1": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B1-d2": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B1-d3": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B2-d4": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B2-d5": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B2-d6": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B3-d7": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B3-d8": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B3-d9": (0.697263, 0.651368),
    "edge-p2147483647-k3t4-r7-B511-d1531": (0.697263, 0.743634),
    "edge-p2147483647-k3t4-r7-B511-d1532": (0.697263, 0.743634),
    "edge-p2147483647-k3t4-r7-B511-d1533": (0.697263, 0.743634),
    "edge-p2147483647-k3t4-r7-B512-d1534": (0.697263, 0.743634),
    "edge-p2147483647-k3t4-r7-B512-d1535": (0.697263, 0.743634),
    "edge-p2147483647-k3t4-r7-B512-d1536": (0.697263, 0.743634),
    "edge-p2147483647-k3t4-r7-B513-d1537": (0.697263, 0.743634),
    "edge-p2147483647-k3t4-r7-B513-d1538": (0.697263, 0.743634),
    "edge-p2147483647-k3t4-r7-B513-d1539": (0.697263, 0.743634),
    "edge-p2147483647-k16t0-r16-B1-d1": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B1-d15": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B1-d16": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B2-d17": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B2-d31": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B2-d32": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B3-d33": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B3-d47": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B3-d48": (0.622485, 0.688757),
    "edge-p2147483647-k16t0-r16-B511-d8161": (0.869442, 0.815278),
    "edge-p2147483647-k16t0-r16-B511-d8175": (0.869442, 0.815278),
    "edge-p2147483647-k16t0-r16-B511-d8176": (0.869442, 0.815278),
    "edge-p2147483647-k16t0-r16-B512-d8177": (0.869442, 0.815278),
    "edge-p2147483647-k16t0-r16-B512-d8191": (0.869442, 0.815278),
    "edge-p2147483647-k16t0-r16-B512-d8192": (0.869442, 0.815278),
    "edge-p2147483647-k16t0-r16-B513-d8193": (0.869442, 0.815278),
    "edge-p2147483647-k16t0-r16-B513-d8207": (0.869442, 0.815278),
    "edge-p2147483647-k16t0-r16-B513-d8208": (0.869442, 0.815278),
    "part-p2147483647-k17t0-B32763": (0.0,),
    "part-p2147483647-k3t1-odd-B262100": (0.0,),
    "part-p2147483647-k3t1-odd-B524289": (0.0,),
    "part-p2147483647-k20t13-B76600": (0.0,),
    "layout-p2147483647-k8t7-shares8": (0.0,),
    "layout-p2147483647-k8t7-out8": (0.0,),
    "layout-p2147483647-k8t7-odd": (0.0,),
    "layout-p2147483647-k8t7-padded": (0.886188, 0.85338),
    "reuse-p4611686006577364993-A": (0.530487,),
    "reuse-p4611686006577364993-other": (0.461121,),
    "reuse-p4611686006577364993-A-again": (0.530487,),
    "reuse-p4611686006577364993-A-plus-one": (0.544768,),
    "reuse-p4611686006577364993-A-permuted": (0.530487,),
    "reuse-p2147483647-A": (0.683935, 0.658032),
    "reuse-p2147483647-other": (0.754122, 0.741313),
    "reuse-p2147483647-A-again": (0.683935, 0.658032),
    "reuse-p2147483647-A-plus-one": (0.689413, 0.621104),
    "reuse-p2147483647-A-permuted": (0.628357, 0.711977),
}

"""Cases of the reconstructor's CHECKED streaming job (sda_secret_reconstructor_begin_checked_dev / finish_checked_dev /
reconstruct_checked) and a Python-integer model of its whole finish - weights, syndromes, locate rule, correction, report - shared
by tests/test_reveal_check_reach.py (which proves on the CPU, against the C oracle, that the model is right and that the cases
reach every verdict) and tests/test_reveal_check_gpu.py.  Nothing here needs a device.

The mathematics.  Position i of a job evaluates the sharing polynomial (degree <= t + k) at x_i = w3^(idx_i + 1); node 0 is the
point 1, whose value is 0.  With u_i = 1 / prod_{l != i} (x_i - x_l) over all n' + 1 nodes, every batch of clean rows has
    S_d = sum_i u_i x_i^d share_i = 0 (mod p)     for d = 0 .. n' - (t + k) - 1.
One faulty position c with error e gives S_d = u_c x_c^d e: S_0 != 0 and S_{d+1} = x_c S_d, and the all-rows reconstruction is
off by R[s][c] e = (R[s][c] / u_c) S_0."""
import collections
import functools
import zlib

import numpy as np

import reconstruct_stream_cases as rc

SCHEMES = rc.SCHEMES
I64_MIN, I64_MAX = rc.I64_MIN, rc.I64_MAX
REPORT, CORRECT = 0, 1                       # SDA_CHECK_REPORT / SDA_CHECK_CORRECT
NONE64 = (1 << 64) - 1                       # report[3] when no batch is bad
KCOEF_LDS = 16                               # kCoefLds: the job's width k + checks up to which a wave keeps its coefficients in LDS
MAX_CHECKS = 16                              # SDA_RECONSTRUCT_MAX_CHECKS

# values: "sums" = clerk sums of 3 participants' oracle shares; "crafted" = any-int64 rows (no polynomial at all); "crafted-one" =
#         sums with one position replaced by any-int64 specials; "congruent" = sums with every value moved by a multiple of p
# fault : none | row (one whole faulty row) | first (one value, first batch) | last (one value, last batch) | surplus (values past
#         ceil(dim / k) only) | two (two whole faulty rows) | disjoint (two rows, one wrong at even batches, one at odd) |
#         p (one row moved by exactly p)
# feed  : how the SEALED run is fed ("one" call / "descending", one position per call); every case also runs all-plaintext and mixed
# expect: the verdict the case is there for - clean | located | unlocated | None (whatever the model says)
# pin   : the faulty positions, where the case fixes them (None: drawn from the case's seeded generator, as ever)
#
# fault "steered" (reveal_decode_cases.steer): batch b gets errors on `checks` pinned positions whose syndromes are a geometric
# sequence a r^d - r = the first pinned point (one error there: located), a value that is no point (unlocated), the node 1 that is
# no row (unlocated) for b mod 3 = 0, 1, 2
Case = collections.namedtuple("Case", "name scheme dim indices checks values fault feed surplus expect pin", defaults=(None,))

ALL8 = tuple(range(8))
FIVE = (7, 0, 3, 5, 1)                                                  # k3_62: r = 1
K8_ALL = tuple(range(26))                                              # k8_62: r = 16
K8_TWELVE = (25, 0, 13, 7, 1, 19, 4, 22, 10, 16, 2, 11)                # k8_62: r = 2
WIDE_300, WIDE_257 = tuple(range(300)), tuple(range(257))              # k3_wide: r = 296 and 253, positions past a byte
PSS_260 = tuple((37 * i + 5) % 728 for i in range(260))                # pss155: r = 5, scattered (gcd(37, 728) = 1)
# The finishes store a group of up to four secrets at a time, element j of it when j < have, the elements of the group below the
# dimension.  k8_62 folds 4 + 4: dimension mod 8 = 1 .. 4 leaves the second group of the last batch with have = 0 and the first with
# have = 1, 2, 3, 4; 6 and 7 leave the second with 2 and 3 (5 is d805's); one batch of dimension 1.  33 batches
GUARD_DIMS = (257, 258, 259, 260, 262, 263, 1)


def _cases():
    out = []

    def add(name, scheme, dim, indices, checks, values="sums", fault="none", feed="one", surplus=0, expect=None, pin=None):
        out.append(Case(name, scheme, dim, indices, checks, values, fault, feed, surplus, expect, pin))
    # config 3's committee, all 8 rows: 1, 2 and 4 checks at every dimension at which the finish takes another path - one batch, no
    # padding, padding, 334 batches (two workgroups; at k + checks = 7 past the 2048-column window of the sealed kernel), 2101
    for dim in (1, 3, 4, 1000, 6301):
        for checks in (1, 2, 4):
            add(f"k3_62-c{checks}-d{dim}-clean", "k3_62", dim, ALL8, checks, expect="clean")
            add(f"k3_62-c{checks}-d{dim}-row", "k3_62", dim, ALL8, checks, fault="row", feed="descending" if dim == 1000 else "one",
                expect="located" if checks >= 2 else "unlocated")
    for checks in (2, 4):
        add(f"k3_62-c{checks}-d1000-first", "k3_62", 1000, ALL8, checks, fault="first", expect="located")
        add(f"k3_62-c{checks}-d1000-last", "k3_62", 1000, ALL8, checks, fault="last", expect="located")
        add(f"k3_62-c{checks}-d1000-surplus", "k3_62", 1000, ALL8, checks, fault="surplus", surplus=5, expect="clean")
        add(f"k3_62-c{checks}-d1000-two", "k3_62", 1000, ALL8, checks, fault="two", expect="unlocated")
        add(f"k3_62-c{checks}-d1000-disjoint", "k3_62", 1000, ALL8, checks, fault="disjoint", feed="descending", expect="located")
        add(f"k3_62-c{checks}-d1000-p", "k3_62", 1000, ALL8, checks, fault="p", expect="clean")
        add(f"k3_62-c{checks}-d1000-congruent", "k3_62", 1000, ALL8, checks, values="congruent", expect="clean")
        add(f"k3_62-c{checks}-d1000-crafted", "k3_62", 1000, ALL8, checks, values="crafted")
        add(f"k3_62-c{checks}-d1000-crafted-one", "k3_62", 1000, ALL8, checks, values="crafted-one")
    add("k3_62-c3-d1000-two", "k3_62", 1000, ALL8, 3, fault="two", expect="unlocated")
    add("k3_62-c1-d1000-two", "k3_62", 1000, ALL8, 1, fault="two", expect="unlocated")
    add("k3_62-c1-d1000-last", "k3_62", 1000, ALL8, 1, fault="last", expect="unlocated")
    add("k3_62-c2-d4-last", "k3_62", 4, ALL8, 2, fault="last", expect="located")
    add("k3_62-c2-d4-surplus", "k3_62", 4, ALL8, 2, fault="surplus", surplus=3, expect="clean")
    # r = 1: one check is all there is
    add("k3_62-five-c1-d1000-clean", "k3_62", 1000, FIVE, 1, expect="clean")
    add("k3_62-five-c1-d1000-row", "k3_62", 1000, FIVE, 1, fault="row", expect="unlocated")
    add("k3_31-c1-d1000-clean", "k3_31", 1000, ALL8, 1, expect="clean")
    add("k3_31-c1-d1000-row", "k3_31", 1000, ALL8, 1, fault="row", feed="descending", expect="unlocated")
    add("k3_31-c1-d4-crafted-one", "k3_31", 4, ALL8, 1, values="crafted-one")
    # k + checks = 16 and 17: either side of kCoefLds
    for checks in (8, 9):
        add(f"k8_62-c{checks}-d805-clean", "k8_62", 805, K8_ALL, checks, expect="clean")
        add(f"k8_62-c{checks}-d805-row", "k8_62", 805, K8_ALL, checks, fault="row", expect="located")
        add(f"k8_62-c{checks}-d805-two", "k8_62", 805, K8_ALL, checks, fault="two", surplus=2, expect="unlocated")
    add("k8_62-twelve-c2-d805-clean", "k8_62", 805, K8_TWELVE, 2, expect="clean")
    add("k8_62-twelve-c2-d805-row", "k8_62", 805, K8_TWELVE, 2, fault="row", expect="located")
    add("k8_62-twelve-c2-d805-two", "k8_62", 805, K8_TWELVE, 2, fault="two", expect="unlocated")
    # many clerks: k + checks = 105, coefficients from memory
    for dim in (1, 250):
        add(f"pss155-c5-d{dim}-clean", "pss155", dim, PSS_260, 5, expect="clean")
        add(f"pss155-c5-d{dim}-row", "pss155", dim, PSS_260, 5, fault="row", expect="located")
    add("pss155-c5-d250-two", "pss155", 250, PSS_260, 5, fault="two", expect="unlocated")
    add("pss155-c5-d250-first", "pss155", 250, PSS_260, 5, fault="first", feed="descending", expect="located")
    add("pss155-c2-d250-two", "pss155", 250, PSS_260, 2, fault="two", expect="unlocated")
    # a wide committee over the 62-bit prime (300 rows, k = 3, t = 1): k + checks = 5, 16 (LDS coefficients) and 19 (global); 257
    # batches (two workgroups, a store tail).  The faulty positions are pinned at and past 256 - the blame word report[4 + pos], the
    # column of corr - and at the last row
    for checks, row, two in ((2, (299,), (255, 256)), (13, (256,), (64, 299)), (16, (257,), (256, 299))):
        add(f"k3_wide-c{checks}-d769-clean", "k3_wide", 769, WIDE_300, checks, expect="clean")
        add(f"k3_wide-c{checks}-d769-row", "k3_wide", 769, WIDE_300, checks, fault="row", expect="located", pin=row,
            feed="descending" if checks == 13 else "one")
        add(f"k3_wide-c{checks}-d769-two", "k3_wide", 769, WIDE_300, checks, fault="two", expect="unlocated", pin=two)
    add("k3_wide-257-c2-d769-row", "k3_wide", 769, WIDE_257, 2, fault="row", expect="located", pin=(256,))
    add("k3_wide-c16-d1-row", "k3_wide", 1, WIDE_300, 16, fault="row", expect="located", pin=(299,))
    # steered syndromes: the locate rule on geometric sequences whose ratio is a point, no point, and the node 1
    add("k3_62-c4-d769-steered", "k3_62", 769, ALL8, 4, fault="steered", pin=(7, 0, 3, 5))
    # the guard of the store's partial group (GUARD_DIMS below): one faulty row at each
    for dim in GUARD_DIMS:
        add(f"k8_62-c8-d{dim}-row", "k8_62", dim, K8_ALL, 8, fault="row", expect="located")
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
SINGLE_FAULTS = ("row", "first", "last")      # exactly one faulty position: the correction is the other rows' reconstruction
E2E = "k3_62-c4-d1000-row"
GUARD = tuple(f"k8_62-c8-d{dim}-row" for dim in GUARD_DIMS)
assert set(GUARD) <= set(BY_NAME)


def batches(case):
    return -(-case.dim // SCHEMES[case.scheme][1])


def width(case):
    return SCHEMES[case.scheme][1] + case.checks


def coef_path(case):
    """which instance of the sealed kernel serves the job: its run-time width is k + checks"""
    return "lds" if width(case) <= KCOEF_LDS else "global"


def redundancy(case):
    p, k, t = SCHEMES[case.scheme][:3]
    return len(case.indices) - (t + k)


# ---- the tables the host builds at begin_checked_dev ------------------------------------------------------------------------------
Tables = collections.namedtuple("Tables", "p k x u R H corr")


@functools.lru_cache(maxsize=None)
def tables(scheme, indices, checks, plant=None):
    p, k, t, n, w2, w3 = SCHEMES[scheme]
    x = [pow(w3, i + 1, p) for i in indices]
    nodes = ([] if plant == "no_node1" else [1]) + x
    u = []
    for xi in x:
        den = 1
        for xl in nodes:
            if xl != xi:
                den = den * (xi - xl) % p
        u.append(pow(den, -1, p))
    R = rc.lagrange_matrix(p, k, w2, w3, indices)
    H = [[u[i] * pow(x[i], d, p) % p for i in range(len(x))] for d in range(checks)]
    if plant == "weight":
        H[0][len(x) // 2] = (H[0][len(x) // 2] + 1) % p
    corr = [[R[s][i] * pow(u[i], -1, p) % p for i in range(len(x))] for s in range(k)]
    return Tables(p, k, x, u, R, H, corr)


Finish = collections.namedtuple("Finish", "out report verdicts")


def model_finish(case, rows, policy, plant=None):
    """what finish_checked_dev must store and report for any-int64 rows.  plant: a fault planted in the MODEL (tests only):
    "weight" (one wrong syndrome weight), "no_node1" (node 1 left out of u_i), "locate" (the locate loop stops one syndrome early),
    "sign" (the correction added), "position_mod_256" (the located position loses its high byte in blame and correction)"""
    T = tables(case.scheme, case.indices, case.checks, plant if plant in ("weight", "no_node1") else None)
    p, k, n_rows, checks = T.p, T.k, len(case.indices), case.checks
    B = batches(case)
    out, blame = [], [0] * n_rows
    bad = located = corrected = 0
    first_bad = NONE64
    verdicts = []                             # per batch: "clean" | "located" | "unlocated"
    pairs = checks - 1 - (1 if plant == "locate" else 0)
    for b in range(B):
        sh = [int(rows[i][b]) % p for i in range(n_rows)]
        sec = [sum(T.R[s][i] * sh[i] for i in range(n_rows)) % p for s in range(k)]
        S = [sum(T.H[d][i] * sh[i] for i in range(n_rows)) % p for d in range(checks)]
        verdict = "clean"
        if any(S):
            bad += 1
            first_bad = min(first_bad, b)
            verdict = "unlocated"
            if checks >= 2 and S[0] != 0:
                fits = [i for i in range(n_rows) if all(S[d + 1] == T.x[i] * S[d] % p for d in range(pairs))]
                if len(fits) == 1:
                    verdict = "located"
                    c = fits[0] % 256 if plant == "position_mod_256" else fits[0]
                    located += 1
                    blame[c] += 1
                    if policy == CORRECT:
                        corrected += 1
                        sign = 1 if plant == "sign" else -1
                        sec = [(sec[s] + sign * T.corr[s][c] * S[0]) % p for s in range(k)]
        verdicts.append(verdict)
        out.extend(sec)
    return Finish(np.array(out[:case.dim], dtype=np.int64), [bad, located, corrected, first_bad] + blame, verdicts)


def unchecked_python(case, rows, keep=None):
    """the plain reconstruction of positions `keep` (default: all) in Python integers"""
    p, k, t, n, w2, w3 = SCHEMES[case.scheme]
    keep = list(range(len(case.indices))) if keep is None else list(keep)
    R = rc.lagrange_matrix(p, k, w2, w3, tuple(case.indices[i] for i in keep))
    out = [sum(R[e][j] * (int(rows[i][b]) % p) for j, i in enumerate(keep)) % p for b in range(batches(case)) for e in range(k)]
    return np.array(out[:case.dim], dtype=np.int64)


# ---- the store of a plain finish, shared by the three finish tables -------------------------------------------------------------
SENTINEL = 0x5A5A5A5A5A5A5A5A                # what the GPU runners fill the output buffer with, dim + TAIL words
TAIL = 8
STORE_PLANTS = ("last_element_dropped", "second_group_unguarded")


def last_batch_groups(case):
    """(n, have) of every group of four of the LAST batch (every other batch has full groups): its secrets, and those of them below
    the dimension"""
    k = SCHEMES[case.scheme][1]
    e = (batches(case) - 1) * k
    return tuple((min(4, k - s0), max(0, min(min(4, k - s0), case.dim - (e + s0)))) for s0 in range(0, k, 4))


def framed(model, case, rows, policy, plant=None):
    """What a plain finish leaves in a SENTINEL-filled buffer of dim + TAIL words, by the table's `model` (its model_finish) - what the
    GPU runners compare, tail included.  plant, a fault of STORE_PLANTS in the store: "last_element_dropped" (`have` one short in a
    partial group: the last element stays), "second_group_unguarded" (the second group of the last batch of k = 8 is stored though it
    is all padding: behind the output)"""
    k = SCHEMES[case.scheme][1]
    buf = [int(x) for x in model(case, rows, policy).out] + [SENTINEL] * TAIL
    groups = last_batch_groups(case)
    if plant == "last_element_dropped" and any(0 < have < n for n, have in groups):
        buf[case.dim - 1] = SENTINEL
    if plant == "second_group_unguarded" and k == 8 and groups[1][1] == 0:
        padded = model(case._replace(dim=batches(case) * k), rows, policy).out
        e0 = (batches(case) - 1) * k + 4
        for j in range(4):
            buf[e0 + j] = int(padded[e0 + j])
    return buf


# ---- rows -----------------------------------------------------------------------------------------------------------------------
Built = collections.namedtuple("Built", "rows clean_rows want row_len batches faulty")


def _errors(rng, p, n):
    return rng.integers(1, p, size=n, dtype=np.int64)


def _add(v, e, p):
    return ((v.astype(object) + e.astype(object)) % p).astype(np.int64)


@functools.lru_cache(maxsize=None)
def build(name):
    """rows [positions][row_len] int64 with the case's faults planted, the clean rows, the true secrets, the faulty positions"""
    from oracle import coracle
    case = BY_NAME[name]
    p, k, t, n, w2, w3 = SCHEMES[case.scheme]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    B = batches(case)
    row_len = B + case.surplus
    pos = len(case.indices)
    parts = 3
    secrets = rng.integers(0, p, size=(parts, case.dim), dtype=np.int64)
    shares = [coracle.packed_generate_systematic(p, k, t, n, w2, w3, secrets[q], rng.integers(0, p, size=B * t, dtype=np.int64))
              for q in range(parts)]
    sums = np.stack([coracle.combine(p, np.stack([shares[q][c] for q in range(parts)])) for c in case.indices])   # clerk.rs:78-86
    clean = np.empty((pos, row_len), dtype=np.int64)
    clean[:, :B] = sums
    clean[:, B:] = rng.integers(0, p, size=(pos, case.surplus), dtype=np.int64)
    want = (secrets.astype(object).sum(axis=0) % p).astype(np.int64)
    rows = clean.copy()
    c1, c2 = int(rng.integers(0, pos)), 0
    c2 = (c1 + 1 + int(rng.integers(0, pos - 1))) % pos
    if case.pin is not None and case.fault != "steered":
        c1 = case.pin[0]
        c2 = case.pin[1] if len(case.pin) > 1 else (c1 + 1) % pos
    faulty = ()
    special = np.array([I64_MIN, I64_MAX, -1, -p, p - 1, 0, p, 1, I64_MIN + 1, -p - 1], dtype=np.int64)
    if case.values == "crafted":
        rows = special[rng.integers(0, special.size, size=(pos, row_len))]
        rows[:, :special.size] = np.stack([np.roll(special, i) for i in range(pos)])[:, :min(special.size, row_len)]
        faulty = None                                            # no polynomial: the model alone says what comes out
    elif case.values == "crafted-one":
        rows[c1] = np.resize(special, row_len)
        faulty = (c1,)
    elif case.values == "congruent":                             # the same residues, other int64 values: +p, -p, -2p in turn
        shift = np.array([p, -p, -2 * p], dtype=object)[(np.arange(row_len)[None, :] + np.arange(pos)[:, None]) % 3]
        rows = (rows.astype(object) + shift).astype(np.int64)
    if case.fault == "row":
        rows[c1, :B] = _add(rows[c1, :B], _errors(rng, p, B), p)
        faulty = (c1,)
    elif case.fault == "first":
        rows[c1, 0] = _add(rows[c1, :1], _errors(rng, p, 1), p)[0]
        faulty = (c1,)
    elif case.fault == "last":
        rows[c1, B - 1] = _add(rows[c1, B - 1:B], _errors(rng, p, 1), p)[0]
        faulty = (c1,)
    elif case.fault == "surplus":
        assert case.surplus > 0
        rows[c1, B:] = _add(rows[c1, B:], _errors(rng, p, case.surplus), p)
    elif case.fault == "two":
        for c in (c1, c2):
            rows[c, :B] = _add(rows[c, :B], _errors(rng, p, B), p)
        faulty = (c1, c2)
    elif case.fault == "disjoint":
        rows[c1, 0:B:2] = _add(rows[c1, 0:B:2], _errors(rng, p, len(range(0, B, 2))), p)
        rows[c2, 1:B:2] = _add(rows[c2, 1:B:2], _errors(rng, p, len(range(1, B, 2))), p)
        faulty = (c1, c2)
    elif case.fault == "p":
        rows[c1, :B] += p                                        # below 2^62 + 2^62: no overflow
        assert not np.array_equal(rows[c1], clean[c1])
    elif case.fault == "steered":
        import reveal_decode_cases as dc                         # (it imports this module: only at the call)
        T = tables(case.scheme, case.indices, case.checks)
        z = dc.no_point(T, rng)
        for b in range(B):
            a = int(rng.integers(1, p))
            ratio = (T.x[case.pin[0]], z, 1)[b % 3]
            dc.steer(rows, T, case.pin, b, [a * pow(ratio, d, p) % p for d in range(case.checks)])
        faulty = None                                            # the model alone says what comes out
    else:
        assert case.fault == "none"
    return Built(rows, clean, want, row_len, B, faulty)

"""Cases of the reconstructor's DECODING finish (sda_secret_reconstructor_finish_decoded_dev / reconstruct_decoded) and a
Python-integer model of the whole finish - verdict, nu, positions, magnitudes, correction, every report word - shared by
tests/test_reveal_decode_reach.py (which proves on the CPU that the model is the definition and that the cases reach every verdict)
and tests/test_reveal_decode_gpu.py.  Nothing here needs a device.

The definition.  Batch b of a checked job holds S_d = sum_i u_i x_i^d share_i[b], d < c; with errors e_i on a set E of positions
S_d = sum_{i in E} Y_i x_i^d, Y_i = u_i e_i.  With a cap e <= floor(c / 2) the batch is DECODED WITH nu POSITIONS (1 <= nu <= e)
when nu distinct positions and non-zero Y exist that reproduce all c syndromes; the solution is unique when it exists.

The model does NOT walk the kernel's route (Berlekamp-Massey, Horner, Forney): it is Peterson-Gorenstein-Zierler - for nu from the
cap downwards, Gaussian elimination on the nu x nu Hankel system for the locator, its roots among the job's points by powers, a
Vandermonde solve for Y - and then CHECKS the definition: nu roots, every Y non-zero, all c syndromes reproduced.  A solution it
returns therefore satisfies the definition; and a solution that exists with nu' positions makes the nu' x nu' Hankel matrix
V diag(Y) V^T regular, so the loop finds it.  brute_force() is the definition itself, over all subsets, for the 8-row shapes."""
import collections
import functools
import itertools
import zlib

import numpy as np

import reveal_check_cases as vc

SCHEMES = vc.SCHEMES
REPORT, CORRECT = vc.REPORT, vc.CORRECT
NONE64 = vc.NONE64
MAX_ERRORS = 8
HEAD = 16                                    # report words before the blame

# fault : none | ("rows", nu) nu whole faulty rows | stair (batch b has b mod (e + 2) faulty rows at rotating positions) | first |
#         last (one value in the first / last batch) | s0zero (two faulty rows with Y_1 = -Y_2 in every batch: S_0 = 0) |
#         surplus | p (as in reveal_check_cases: clean) | steered (batch b holds errors on `checks` pinned positions whose
#         syndromes are EXACTLY those of family b mod F of families(): the degenerate walks of the decoder, side by side in a wave)
# values: sums | congruent | crafted (any-int64 rows: the model alone says what comes out)
# cap   : max_errors as passed (0 = floor(checks / 2))
# pin   : positions that come first in the order the faulty rows are taken from (None: the seeded permutation alone, as ever);
#         steered: the `checks` positions the errors are planted on
Case = collections.namedtuple("Case", "name scheme dim indices checks cap values fault feed surplus pin", defaults=(None,))

ALL8, K8_ALL, K8_TWELVE, PSS_260 = vc.ALL8, vc.K8_ALL, vc.K8_TWELVE, vc.PSS_260
WIDE_300, WIDE_257 = vc.WIDE_300, vc.WIDE_257
STEER8 = (0, 3, 5, 7)                                                   # the four positions a steered batch of the 8-row shape uses


def cap_of(case):
    return case.cap or case.checks // 2


def _cases():
    out = []

    def add(tag, scheme, dim, indices, checks, fault="none", cap=0, values="sums", feed="one", surplus=0, pin=None):
        fname = fault if isinstance(fault, str) else f"rows{fault[1]}"
        out.append(Case(f"{tag}-c{checks}-d{dim}-{fname}" + (f"-cap{cap}" if cap else "") + ("" if values == "sums" else "-" + values),
                        scheme, dim, indices, checks, cap, values, fault, feed, surplus, pin))
    # config 3's committee on all 8 rows: c = 4 (e = 2) and c = 3 (e = 1; two faulty rows are the guaranteed-undecoded band); one
    # batch, padding, 334 batches (two workgroups)
    for checks in (4, 3):
        e = checks // 2
        for dim in (1, 4, 1000):
            add("k3_62", "k3_62", dim, ALL8, checks)
            for nu in range(1, e + 3):
                add("k3_62", "k3_62", dim, ALL8, checks, ("rows", nu), feed="descending" if dim == 1000 and nu == 2 else "one")
            add("k3_62", "k3_62", dim, ALL8, checks, "stair")
            add("k3_62", "k3_62", dim, ALL8, checks, "last")
        add("k3_62", "k3_62", 1000, ALL8, checks, "first")
        add("k3_62", "k3_62", 1000, ALL8, checks, "surplus", surplus=5)
        add("k3_62", "k3_62", 1000, ALL8, checks, "p")
        add("k3_62", "k3_62", 1000, ALL8, checks, values="congruent")
        add("k3_62", "k3_62", 1000, ALL8, checks, "s0zero")
        add("k3_62", "k3_62", 1000, ALL8, checks, values="crafted")
    add("k3_62", "k3_62", 1000, ALL8, 4, ("rows", 2), cap=1)
    add("k3_62", "k3_62", 1000, ALL8, 4, "stair", cap=1)
    # config 4's committee: k + c = 24, 17, 16 - either side of kCoefLds for the sealed feed - and twelve rows with c = 2
    for checks in (16, 9, 8):
        e = checks // 2
        add("k8_62", "k8_62", 805, K8_ALL, checks)
        for nu in range(1, e + 3):
            add("k8_62", "k8_62", 805, K8_ALL, checks, ("rows", nu), feed="descending" if nu == e else "one", surplus=2 if nu == 2 else 0)
        add("k8_62", "k8_62", 805, K8_ALL, checks, "stair")
    add("k8_62", "k8_62", 805, K8_ALL, 16, "s0zero")
    add("k8_62", "k8_62", 805, K8_ALL, 16, "first")
    add("k8_62", "k8_62", 805, K8_ALL, 16, "last")
    add("k8_62", "k8_62", 805, K8_ALL, 16, ("rows", 2), cap=1)           # a lowered cap: two faulty rows are refused, not decoded
    add("k8_62", "k8_62", 805, K8_ALL, 16, "stair", cap=3)
    add("k8_62", "k8_62", 805, K8_ALL, 16, values="congruent")
    add("k8_62", "k8_62", 805, K8_ALL, 16, values="crafted")
    add("k8_62-twelve", "k8_62", 805, K8_TWELVE, 2)
    for nu in (1, 2, 3):
        add("k8_62-twelve", "k8_62", 805, K8_TWELVE, 2, ("rows", nu))
    add("k8_62-twelve", "k8_62", 805, K8_TWELVE, 2, "stair")
    # many clerks, a 20-bit prime
    for checks in (5, 4):
        for dim in (1, 250):
            add("pss155", "pss155", dim, PSS_260, checks)
            for nu in range(1, 5):
                add("pss155", "pss155", dim, PSS_260, checks, ("rows", nu), feed="descending" if (dim, nu) == (250, 2) else "one")
            add("pss155", "pss155", dim, PSS_260, checks, "last")
        add("pss155", "pss155", 250, PSS_260, checks, "stair")
    parent = len(out)                                              # the table up to here is older than the wide committee
    # a wide committee over the 62-bit prime (300 rows, k = 3, t = 1; 257 batches: two workgroups, a store tail): positions past a
    # byte in dec_pos, in the blame words and in the columns of corr.  The pins put faulty rows at and past 256 and at the last row
    pins = {1: (299,), 2: (256, 0), 3: (257,), 5: (255, 256), 8: (299, 256, 64)}
    for nu in range(1, 11):
        add("k3_wide", "k3_wide", 769, WIDE_300, 16, ("rows", nu), pin=pins.get(nu), feed="descending" if nu == 8 else "one")
    for fault in ("stair", "first", "last", "s0zero"):
        add("k3_wide", "k3_wide", 769, WIDE_300, 16, fault, pin=(256, 299) if fault == "s0zero" else (258,) if fault == "last" else None)
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, values="crafted")
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, values="congruent")
    for nu in range(1, 9):                                               # k + c = 16: the sealed feed's LDS coefficients
        add("k3_wide", "k3_wide", 769, WIDE_300, 13, ("rows", nu), pin={1: (256,), 6: (299, 63)}.get(nu))
    for nu in range(1, 5):
        add("k3_wide-257", "k3_wide", 769, WIDE_257, 4, ("rows", nu), pin={1: (256,), 2: (0, 256)}.get(nu))
    add("k3_wide", "k3_wide", 1, WIDE_300, 16, ("rows", 8), pin=(299, 256))
    add("k3_wide-257", "k3_wide", 1, WIDE_257, 4, ("rows", 2), pin=(256,))
    # steered syndromes: every family of families() in every wave
    add("k3_62", "k3_62", 769, ALL8, 4, "steered", pin=STEER8)
    add("k8_62", "k8_62", 805, K8_ALL, 16, "steered", pin=tuple(range(1, 26, 2)) + (0, 2, 24))
    add("k8_62", "k8_62", 805, K8_ALL, 16, "steered", cap=2, pin=tuple(range(1, 26, 2)) + (0, 2, 24))
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, "steered", pin=(0, 63, 64, 127, 128, 191, 192, 255, 256, 257, 270, 280, 290, 297, 298, 299))
    wide = len(out)
    # the guard of the store's partial group (reveal_check_cases.GUARD_DIMS): one faulty row at each
    for dim in vc.GUARD_DIMS:
        add("k8_62", "k8_62", dim, K8_ALL, 16, ("rows", 1))
    return out, parent, wide


CASES, PARENT_CASES, WIDE_CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NEW = tuple(c.name for c in CASES[PARENT_CASES:WIDE_CASES])              # ... and these came with it
GUARD = tuple(c.name for c in CASES[WIDE_CASES:])                        # ... and these with the store the finishes share
E2E = "k3_62-c4-d1000-rows2"


def batches(case):
    return vc.batches(case)


def coef_path(case):
    return vc.coef_path(case)


def tables(case):
    return vc.tables(case.scheme, case.indices, case.checks)


# ---- linear algebra mod p ----------------------------------------------------------------------------------------------------------
def solve(M, rhs, p):
    """the solution of the square system M y = rhs mod p; None when M is singular"""
    n = len(M)
    A = [list(r) + [v] for r, v in zip(M, rhs)]
    for col in range(n):
        piv = next((r for r in range(col, n) if A[r][col] % p), None)
        if piv is None:
            return None
        A[col], A[piv] = A[piv], A[col]
        inv = pow(A[col][col], -1, p)
        A[col] = [v * inv % p for v in A[col]]
        for r in range(n):
            if r != col and A[r][col]:
                f = A[r][col]
                A[r] = [(a - f * b) % p for a, b in zip(A[r], A[col])]
    return [A[r][n] for r in range(n)]


def magnitudes(S, xs, p):
    """Y with sum_j Y_j xs_j^d = S_d for d < len(xs) (a Vandermonde system: regular for distinct points)"""
    return solve([[pow(x, d, p) for x in xs] for d in range(len(xs))], S[:len(xs)], p)


def reproduces(S, xs, Y, p):
    return all(sum(y * pow(x, d, p) for x, y in zip(xs, Y)) % p == S[d] for d in range(len(S)))


# ---- steered syndromes ---------------------------------------------------------------------------------------------------------------
def no_point(T, rng):
    """a value that is no point of the job, not 0 and not the node 1"""
    while True:
        z = int(rng.integers(2, T.p))
        if z not in T.x:
            return z


def steer(rows, T, positions, b, target, weight=None):
    """plant errors on `positions` (as many as `target` is long) of batch b so that  sum_i Y_i x_i^d = target_d  over them: Y from
    the Vandermonde system, err_i = Y_i / u_i.  On clean rows the batch's syndromes ARE `target`.  weight[i] (erasures): the system
    is solved for Z_i = Y_i weight[i], so `target` is met by the MODIFIED syndromes.  -> the positions whose error is not zero"""
    p = T.p
    assert len(positions) == len(target) == len(set(positions))
    Y = magnitudes(list(target), [T.x[i] for i in positions], p)
    hit = []
    for i, y in zip(positions, Y):
        if weight is not None:
            y = y * pow(weight[i], -1, p) % p
        if y:
            rows[i, b] = (int(rows[i, b]) + y * pow(T.u[i], -1, p)) % p
            hit.append(i)
    return tuple(sorted(hit))


# x: a point among the steered positions P (in their order), z: a value that is no point, a, b: random non-zero
FAMILIES = ("ratio_z",              # a z^d: a locator whose root is no point of the job
            "ratio_one",            # a: a root at the node 1, which is no row
            "ratio_zero",           # (a, 0, .., 0): a root at 0
            "late_jump",            # (0, .., 0, a): L jumps from 0 to n at the last syndrome
            "zero_half",            # zeros, then non-zero from n // 2 on: zero discrepancies, then L > n / 2
            "double_root",          # a d x^(d-1): the locator (z - x)^2
            "point_and_z",          # a x^d + b z^d: L = 2 with one root among the points
            "all_pm1",              # p - 1 in every place
            "one_point_pm1",        # (p - 1) x^d at x = the last of P: decoded
            "two_points_cancel",    # a x1^d - a x2^d at the first and the last of P: decoded with S_0 = 0
            "s0_zero_two_points",   # the same at the second and third of P
            "s0_forced_zero")       # 0, then a x1^d + b x2^d for d >= 1 with a + b != 0: L jumps by two after a zero discrepancy
CAP_FAMILIES = ("cap_points",           # exactly e points
                "cap_plus_one",         # e + 1 points
                "cap_minus_one_and_z",  # e - 1 points and a value that is no point: L = e with e - 1 roots
                "three_points")         # decoded - unless max_errors is lowered below three


def families(n):
    """the families of a steered case with n (modified) syndromes"""
    return FAMILIES + (CAP_FAMILIES if n >= 8 else ())


def family_syndromes(fam, n, pts, z, e, p, rng):
    """the n syndromes of one batch of family `fam`; pts: the points of the steered positions, e: the cap"""
    a, b = (int(v) for v in rng.integers(1, p, size=2))

    def sums(pairs):
        return [sum(y * pow(x, d, p) for y, x in pairs) % p for d in range(n)]

    def some(m):
        return [int(v) for v in rng.integers(1, p, size=m)]
    if fam == "ratio_z":
        return sums([(a, z)])
    if fam == "ratio_one":
        return [a] * n
    if fam == "ratio_zero":
        return [a] + [0] * (n - 1)
    if fam == "late_jump":
        return [0] * (n - 1) + [a]
    if fam == "zero_half":
        return [0] * (n // 2) + some(n - n // 2)
    if fam == "double_root":
        return [a * d * pow(pts[0], max(d - 1, 0), p) % p for d in range(n)]
    if fam == "point_and_z":
        return sums([(a, pts[0]), (b, z)])
    if fam == "all_pm1":
        return [p - 1] * n
    if fam == "one_point_pm1":
        return sums([(p - 1, pts[-1])])
    if fam == "two_points_cancel":
        return sums([(a, pts[0]), (p - a, pts[-1])])
    if fam == "s0_zero_two_points":
        return sums([(a, pts[1]), (p - a, pts[2])])
    if fam == "s0_forced_zero":
        if (a + b) % p == 0:
            b = b % (p - 1) + 1
        return [0] + sums([(a, pts[1]), (b, pts[2])])[1:]
    if fam == "cap_points":
        return sums(list(zip(some(e), pts[:e])))
    if fam == "cap_plus_one":
        return sums(list(zip(some(e + 1), pts[:e + 1])))
    if fam == "cap_minus_one_and_z":
        return sums(list(zip(some(e), list(pts[:e - 1]) + [z])))
    assert fam == "three_points", fam
    return sums(list(zip(some(3), pts[:3])))


def family_verdict(fam, n, e, P):
    """what a batch of family `fam` must come back as, known from its construction: (nu, positions) | (-1, ()) | None where the
    definition promises nothing and the model is asked.  n >= 3 syndromes, cap e, P: the steered positions in their order"""
    if e == 0:
        return -1, ()
    decoded = {"one_point_pm1": P[-1:], "two_points_cancel": (P[0], P[-1]), "s0_zero_two_points": P[1:3], "cap_points": P[:e],
               "three_points": P[:3]}
    if fam in decoded:
        at = tuple(sorted(decoded[fam]))
        return (len(at), at) if len(at) <= e else (-1, ()) if len(at) <= n - e else None     # e < nu <= n - e: always detected
    if fam == "cap_plus_one":
        return (-1, ()) if e + 1 <= n - e else None
    if fam in ("cap_minus_one_and_z", "s0_forced_zero"):
        return None
    # one or two nodes outside the job (with multiplicity): a solution on nu <= e points would be a vanishing combination of at
    # most e + 2 <= n distinct nodes (confluent for the double root); zeros up to n // 2 >= e force Y = 0
    return -1, ()


def pgz(S, x, e, p):
    """-> [(position, Y), ...] ascending by position when the syndromes S are decoded with 1 .. e positions of x, else None"""
    if not any(S):
        return None
    for nu in range(min(e, len(S) // 2), 0, -1):
        # x^nu + L_1 x^(nu-1) + .. + L_nu vanishes at the error points: sum_j L_j S_{i+nu-j} = -S_{i+nu}, i < nu
        L = solve([[S[i + nu - j] for j in range(1, nu + 1)] for i in range(nu)], [-S[i + nu] % p for i in range(nu)], p)
        if L is None:
            continue
        pos = [i for i, xi in enumerate(x) if (pow(xi, nu, p) + sum(L[j - 1] * pow(xi, nu - j, p) for j in range(1, nu + 1))) % p == 0]
        if len(pos) != nu:
            continue
        Y = magnitudes(S, [x[i] for i in pos], p)
        if Y is None or not all(Y) or not reproduces(S, [x[i] for i in pos], Y, p):
            continue
        return list(zip(pos, Y))
    return None


def brute_force(S, x, e, p):
    """the definition: every subset of 1 .. e positions with non-zero Y that reproduces all syndromes (small committees only)"""
    assert len(x) <= 8
    if not any(S):
        return []
    found = []
    for nu in range(1, e + 1):
        if nu > len(S):
            break
        for pos in itertools.combinations(range(len(x)), nu):
            Y = magnitudes(S, [x[i] for i in pos], p)
            if Y is not None and all(Y) and reproduces(S, [x[i] for i in pos], Y, p):
                found.append(list(zip(pos, Y)))
    return found


# ---- the model of the whole finish -----------------------------------------------------------------------------------------------
Finish = collections.namedtuple("Finish", "out report verdicts errors")
PLANTS = ("cap_ge", "roots", "denominator", "sign", "blame_per_error", "histogram", "first_undecoded", "odd_ceil")
# ... and three more that only a wide committee or a steered syndrome can notice (tests/test_reveal_decode_reach.py says which):
# a located position loses its high byte in blame and correction; the root search also tries the node 1 / the value 0 and counts
# the root it finds there
GAP_PLANTS = ("position_mod_256", "root_at_node_one", "root_at_zero")


def _decode(S, T, e, checks, p, plant):
    x = T.x
    if plant == "odd_ceil" and checks % 2:                               # the cap of an odd c taken as ceil(c / 2)
        found = [f for f in brute_force(S, x, (checks + 1) // 2, p)]
        return min(found, key=len) if found else None
    if plant == "roots":                                                 # the root count not checked: whatever roots there are
        for nu in range(e, 0, -1):
            L = solve([[S[i + nu - j] for j in range(1, nu + 1)] for i in range(nu)], [-S[i + nu] % p for i in range(nu)], p)
            if L is None:
                continue
            pos = [i for i, xi in enumerate(x) if (pow(xi, nu, p) + sum(L[j - 1] * pow(xi, nu - j, p) for j in range(1, nu + 1))) % p == 0]
            if not pos:
                return None
            return list(zip(pos, magnitudes(S, [x[i] for i in pos], p)))
        return None
    if plant in ("root_at_node_one", "root_at_zero"):                    # one more candidate behind the rows (position n_rows)
        return pgz(S, list(x) + [1 if plant == "root_at_node_one" else 0], e, p)
    got = pgz(S, x, e, p)
    if got is not None and plant == "cap_ge" and len(got) >= e:          # the cap compared with >= instead of >
        return None
    if got is not None and plant == "denominator" and len(got) > 1:      # sigma_j taken at the next root instead of its own
        pos = [i for i, _ in got]

        def sigma(j, at):
            v = 1
            for l, i in enumerate(pos):
                if l != j:
                    v = v * (at - x[i]) % p
            return v
        got = [(i, y * sigma(j, x[i]) * pow(sigma(j, x[pos[(j + 1) % len(pos)]]) or 1, -1, p) % p) for j, (i, y) in enumerate(got)]
    return got


@functools.lru_cache(maxsize=None)
def _decoded(S, scheme, indices, checks, e, plant):
    """_decode, remembered: both policies, and every test that asks again, decode a batch once"""
    T = vc.tables(scheme, indices, checks)
    return _decode(list(S), T, e, checks, T.p, plant)


def model_finish(case, rows, policy, plant=None):
    """what finish_decoded_dev must store and report for any-int64 rows.  verdicts: per batch 0 (clean), nu (decoded) or -1
    (undecoded); errors: per batch the decoded [(position, Y)].  plant: one of PLANTS, a fault planted in the MODEL (tests only)"""
    T = tables(case)
    p, k, n_rows, checks, e = T.p, T.k, len(case.indices), case.checks, cap_of(case)
    B = batches(case)
    out, blame, hist = [], [0] * n_rows, [0] * MAX_ERRORS
    bad = decoded = corrected = most = 0
    first_bad = first_undecoded = NONE64
    verdicts, errors = [], []
    for b in range(B):
        sh = [int(rows[i][b]) % p for i in range(n_rows)]
        sec = [sum(T.R[s][i] * sh[i] for i in range(n_rows)) % p for s in range(k)]
        S = [sum(T.H[d][i] * sh[i] for i in range(n_rows)) % p for d in range(checks)]
        verdict, got = 0, None
        if any(S):
            bad += 1
            first_bad = min(first_bad, b)
            got = _decoded(tuple(S), case.scheme, case.indices, checks, e, plant)
            if got is None:
                verdict = -1
                first_undecoded = min(first_undecoded, b)
            else:
                verdict = nu = len(got)
                decoded += 1
                most = max(most, nu)
                hist[(nu if plant == "histogram" else nu - 1) % MAX_ERRORS] += 1
                at = [(i % 256 if plant == "position_mod_256" else i, y) for i, y in got if i < n_rows]   # i = n_rows: a planted root
                for i, _ in at:
                    blame[i] += nu if plant == "blame_per_error" else 1
                if policy == CORRECT:
                    corrected += 1
                    sign = 1 if plant == "sign" else -1
                    sec = [(sec[s] + sign * sum(T.corr[s][i] * y for i, y in at)) % p for s in range(k)]
        verdicts.append(verdict)
        errors.append(got)
        out.extend(sec)
    if plant == "first_undecoded":
        first_undecoded = first_bad
    report = [bad, decoded, corrected, first_bad, first_undecoded, most, 0, 0] + hist + blame
    return Finish(np.array(out[:case.dim], dtype=np.int64), report, verdicts, errors)


# ---- rows ------------------------------------------------------------------------------------------------------------------------
Built = collections.namedtuple("Built", "rows clean_rows want row_len batches faulty")


def _base(case):
    """the clean rows of reveal_check_cases' builder (its value kinds and its clean faults), under a name of this table"""
    fault = case.fault if case.fault in ("surplus", "p") else "none"
    base = vc.Case("decode/" + case.name, case.scheme, case.dim, case.indices, case.checks, case.values, fault, case.feed, case.surplus, None)
    vc.BY_NAME.setdefault(base.name, base)                               # BY_NAME only: vc.CASES, what its own tests walk, stays
    return vc.build(base.name)


@functools.lru_cache(maxsize=None)
def build(name):
    """rows [positions][row_len] int64 with the case's faults planted, the clean rows, the true secrets and, per batch, the tuple of
    faulty positions (None: crafted rows, no polynomial at all)"""
    case = BY_NAME[name]
    base = _base(case)
    T = tables(case)
    p, pos, B, e = T.p, len(case.indices), base.batches, case.checks // 2
    rng = np.random.default_rng(zlib.crc32(("decode/" + name).encode()))
    rows = base.rows.copy()
    faulty = [()] * B
    if case.values == "crafted":
        return Built(rows, base.clean_rows, base.want, base.row_len, B, None)
    order = [int(i) for i in rng.permutation(pos)]
    if case.pin is not None:
        order = list(case.pin) + [i for i in order if i not in case.pin]

    def spoil(i, bs):
        bs = np.asarray(bs)
        rows[i, bs] = vc._add(rows[i, bs], vc._errors(rng, p, len(bs)), p)
    if isinstance(case.fault, tuple):
        chosen = sorted(order[:case.fault[1]])
        for i in chosen:
            spoil(i, np.arange(B))
        faulty = [tuple(chosen)] * B
    elif case.fault == "stair":
        per = [tuple(sorted((b + 3 * j) % pos for j in range(b % (e + 2)))) for b in range(B)]
        for i in range(pos):
            bs = [b for b in range(B) if i in per[b]]
            if bs:
                spoil(i, bs)
        faulty = per
    elif case.fault in ("first", "last"):
        b = 0 if case.fault == "first" else B - 1
        spoil(order[0], [b])
        faulty[b] = (order[0],)
    elif case.fault == "s0zero":
        i1, i2 = sorted(order[:2])
        e1 = vc._errors(rng, p, B)
        ratio = T.u[i1] * pow(T.u[i2], -1, p) % p                        # u_2 e_2 = -u_1 e_1
        e2 = np.array([(-int(v) * ratio) % p for v in e1], dtype=np.int64)
        rows[i1, :B] = vc._add(rows[i1, :B], e1, p)
        rows[i2, :B] = vc._add(rows[i2, :B], e2, p)
        faulty = [(i1, i2)] * B
    elif case.fault == "steered":
        assert len(case.pin) == case.checks
        z, fams = no_point(T, rng), families(case.checks)
        pts = [T.x[i] for i in case.pin]
        faulty = [steer(rows, T, case.pin, b, family_syndromes(fams[b % len(fams)], case.checks, pts, z, cap_of(case), p, rng)) for b in range(B)]
    else:
        assert case.fault in ("none", "surplus", "p"), case.fault
    return Built(rows, base.clean_rows, base.want, base.row_len, B, faulty)


def expected_verdicts(case, built):
    """what the GUARANTEES say per batch from the planted faults alone: 0, nu, -1, or None where they promise nothing"""
    if built.faulty is None:
        return None
    e, c = cap_of(case), case.checks
    return [0 if not f else len(f) if len(f) <= e else -1 if len(f) <= c - e else None for f in built.faulty]

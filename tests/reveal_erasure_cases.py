"""Cases of the reconstructor's ERASURE finish (sda_secret_reconstructor_finish_erasures_dev / reconstruct_erasures) and a
Python-integer model of the whole finish - verdict, positions, magnitudes of errors and erasures, correction, every report word -
shared by tests/test_reveal_erasure_reach.py (which proves on the CPU that the model is the definition and that the cases reach
every (f, nu) class) and tests/test_reveal_erasure_gpu.py.  Nothing here needs a device.

The definition (include/sda_hip.h).  F = the f erased positions, Gamma(z) = prod_{j in F} (z - x_j) = sum_m gamma_m z^m.  The
modified syndromes T_j = sum_m gamma_m S_{j+m}, j < c - f, do not see F.  With e' = min(cap, floor((c - f) / 2)): a batch is
consistent when T = 0, else bad; a bad batch is decoded with nu <= e' non-erased positions E when non-zero Z reproduce T, and
Y_i = Z_i / Gamma(x_i); the erased magnitudes solve sum_{j in F} Y_j x_j^d = S_d - sum_{i in E} Y_i x_i^d, d < f.

The model does NOT walk the kernel's route.  It is Gaussian elimination throughout: T from the definition, then reveal_decode_cases'
Peterson-Gorenstein-Zierler (from the cap downwards) on T over the non-erased points, a Vandermonde solve for the erased
magnitudes, and then it CHECKS that E u F with those magnitudes reproduce all c ORIGINAL syndromes.  brute_force() never forms T:
it tries every subset E of the non-erased positions and solves the c equations in the |E| + f unknowns directly."""
import collections
import functools
import itertools
import zlib

import numpy as np

import reveal_check_cases as vc
import reveal_decode_cases as dc

SCHEMES = vc.SCHEMES
REPORT, CORRECT = vc.REPORT, vc.CORRECT
NONE64 = vc.NONE64
HEAD = dc.HEAD
MAX_ERRORS = dc.MAX_ERRORS
ALL8, K8_ALL = vc.ALL8, vc.K8_ALL

# erased: the erased positions F
# errors: how many NON-erased rows are faulty in every batch, or "mixed": batch b is clean (erased rows hold their true values) /
#         erasure-only / erasure + e' errors / erasure + e' + 1 errors (undecoded) for b mod 4 = 0 .. 3 - side by side in one wave
#         or "aimed": c - f faulty rows whose modified syndromes are those of ONE error on an erased position - a root the
#         search must not accept
#         or "steered": batch b holds errors on c - f pinned non-erased positions whose MODIFIED syndromes are exactly those of
#         family b mod F of reveal_decode_cases.families(c - f)
# fill  : what the erased rows hold - zero (a refused row adds nothing) | random | clean (their true values) | spoiled (true + error)
# ok    : how the flags reach the call - flags (n_rows words) | ones (all non-zero) | null
# cap   : max_errors as passed (0 = unlimited)
# pin   : non-erased positions that come first in the order the faulty rows are taken from (None: the seeded permutation alone, as
#         ever); steered: the c - f positions the errors are planted on
Case = collections.namedtuple("Case", "name scheme dim indices checks cap erased errors fill ok pin", defaults=(None,))
WIDE_300, WIDE_257 = vc.WIDE_300, vc.WIDE_257
STEP = 256                                   # positions reveal_erasure_setup_kernel compacts per step (kThreads), four waves of 64
KEPT = 16                                    # erased positions it keeps (kEraseMax); f is counted in full


def _cases():
    out = []

    def add(tag, scheme, dim, indices, checks, erased=(), errors=0, fill="zero", ok="flags", cap=0, note="", pin=None):
        name = f"{tag}-c{checks}-d{dim}-f{len(erased)}-e{errors}-{fill}" + (f"-cap{cap}" if cap else "") + ("" if ok == "flags" else "-" + ok) + note
        out.append(Case(name, scheme, dim, tuple(indices), checks, cap, tuple(sorted(erased)), errors, fill, ok, pin))
    # config 3's committee (8 rows, k = 3, t = 1), c = 4: every (f, errors) pair, at one batch, 255 and 257 batches (one workgroup
    # - 1 / + 1) with the three store tails (dim mod 3 = 1, 2, 0); the padding batch is decoded and not stored
    pairs = [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (4, 0), (0, 1), (0, 2), (1, 2), (3, 1), (5, 0)]
    sets = {0: (), 1: (5,), 2: (2, 6), 3: (1, 4, 6), 4: (1, 2, 4, 6), 5: (1, 2, 3, 5, 6)}
    for f, errors in pairs:
        for dim in (1, 764, 769):
            add("k3_62", "k3_62", dim, ALL8, 4, sets[f], errors)
    add("k3_62", "k3_62", 768, ALL8, 4, (2, 6), 1)                           # 256 batches: no tail
    add("k3_62", "k3_62", 764, ALL8, 4, (0,), 1, note="-first")              # the first and the last position erased
    add("k3_62", "k3_62", 764, ALL8, 4, (7,), 1, note="-last")
    add("k3_62", "k3_62", 764, ALL8, 4, (0, 7), 1, note="-both")
    add("k3_62", "k3_62", 769, ALL8, 4, (2, 6), "mixed")                     # one wave with all four kinds of lane
    add("k3_62", "k3_62", 769, ALL8, 4, (5,), "mixed")
    add("k3_62", "k3_62", 764, ALL8, 4, (2, 6), "aimed")
    for fill in ("random", "clean", "spoiled"):                              # whatever the erased rows added: the same result
        add("k3_62", "k3_62", 764, ALL8, 4, (2, 6), 1, fill=fill)
    add("k3_62", "k3_62", 764, ALL8, 4, (), 0, ok="ones")
    add("k3_62", "k3_62", 764, ALL8, 4, (), 2, ok="ones")
    add("k3_62", "k3_62", 764, ALL8, 4, (), 2, ok="null")
    add("k3_62", "k3_62", 764, ALL8, 4, (), 3, ok="null")
    add("k3_62", "k3_62", 764, ALL8, 4, (5,), 1, cap=1)
    add("k3_62", "k3_62", 764, ALL8, 4, (), 2, cap=1)
    # one check: one erasure is repaired, an error is only detected
    add("k3_62", "k3_62", 764, ALL8, 1, (3,), 0)
    add("k3_62", "k3_62", 764, ALL8, 1, (3,), 0, fill="random")
    add("k3_62", "k3_62", 764, ALL8, 1, (), 1)
    add("k3_62", "k3_62", 764, ALL8, 1, (), 0, ok="null")
    add("k3_62", "k3_62", 764, ALL8, 1, (3, 4), 0)                           # f > c
    add("k3_31", "k3_31", 764, ALL8, 1, (6,), 0)                             # a 31-bit prime, t + k = 7: one check is all there is
    # config 4's committee (26 rows, k = 8, t = 2), c = 16; 101 batches, dim mod 8 = 5
    rng = np.random.default_rng(20)

    def some(f):
        return tuple(sorted(int(i) for i in rng.permutation(26)[:f]))
    for f, errors in ((1, 7), (6, 5), (8, 4), (15, 0), (16, 0), (15, 1), (17, 0), (0, 8), (3, 6), (3, 7)):
        add("k8_62", "k8_62", 805, K8_ALL, 16, some(f), errors)
    add("k8_62", "k8_62", 805, K8_ALL, 16, (0, 25), 7, note="-both")
    add("k8_62", "k8_62", 805, K8_ALL, 16, (4, 9), 2, cap=1)                 # a lowered cap: two errors are refused
    add("k8_62", "k8_62", 805, K8_ALL, 16, (4, 9), 1, cap=1)
    add("k8_62", "k8_62", 805, K8_ALL, 16, some(6), "mixed")
    add("k8_62", "k8_62", 805, K8_ALL, 16, some(8), 4, fill="random")
    add("k8_62", "k8_62", 805, K8_ALL, 16, some(8), 4, fill="spoiled")
    add("k8_62", "k8_62", 2053, K8_ALL, 16, some(6), 5)                      # 257 batches
    add("k8_62", "k8_62", 805, K8_ALL, 16, (), 8, ok="null")
    add("k8_62", "k8_62", 805, K8_ALL, 16, (), 3, ok="ones")
    parent = len(out)                                                  # the table up to here is older than the wide committee
    # a wide committee over the 62-bit prime (300 rows, k = 3, t = 1; 257 batches): the setup kernel's second step (positions from
    # 256), every wave of a step (64 positions each), the count carried from step to step, positions it counts and does not keep,
    # 1 / Gamma for more rows than the workgroup has lanes; errors at and past 256 and at the last row
    edge = (63, 64, 255, 256, 299)
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, edge, 5, pin=(257, 298, 0))
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, range(256, 272), 0, note="-second")     # sixteen, all in the second step
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, range(0, 300, 19), 0, note="-spread")   # sixteen, in every wave of both steps
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, range(0, 300, 43), 4, pin=(299, 256))
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, range(0, 300, 43), 5)                   # e' = 4: undecoded
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, (64, 256), "mixed")
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, (256, 64), "aimed")
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, tuple(range(3, 256, 16)) + (290,), 0)   # seventeen: over, the last one not kept
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, range(50, 250), 0)                      # two hundred
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, edge, 5, fill="random", pin=(257, 298, 0))
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, edge, 5, fill="spoiled", pin=(257, 298, 0))
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, (), 8, ok="ones", pin=(256, 299))
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, (), 8, ok="null", pin=(256, 299))
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, edge, 3, cap=2)                         # a lowered cap: three errors are refused
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, edge, 2, cap=2, pin=(257,))
    add("k3_wide", "k3_wide", 769, WIDE_300, 13, (63, 256), 5, pin=(299, 257))           # k + c = 16: the sealed feed's LDS coefficients
    add("k3_wide-257", "k3_wide", 769, WIDE_257, 4, (0, 256), 1, pin=(255,))
    add("k3_wide-257", "k3_wide", 769, WIDE_257, 4, (256,), 1, pin=(0,))
    add("k3_wide-256", "k3_wide", 769, tuple(range(256)), 4, (255,), 1, pin=(254,))      # exactly one step
    add("k3_wide-65", "k3_wide", 769, tuple(range(65)), 4, (63, 64), 1, pin=(62,))       # the first position of the second wave
    add("k3_wide-64", "k3_wide", 769, tuple(range(64)), 4, (63,), 1, pin=(0,))           # exactly one wave
    add("k3_wide", "k3_wide", 1, WIDE_300, 16, edge, 5, pin=(257, 298, 0))
    add("k3_wide-257", "k3_wide", 1, WIDE_257, 4, (0, 256), 1, pin=(255,))
    # steered modified syndromes: every family of reveal_decode_cases.families() in every wave
    add("k3_62", "k3_62", 769, ALL8, 4, (2,), "steered", pin=(0, 3, 7))
    add("k8_62", "k8_62", 805, K8_ALL, 16, (4, 8, 20), "steered", pin=tuple(range(1, 26, 2)))
    add("k3_wide", "k3_wide", 769, WIDE_300, 16, (64, 256), "steered", pin=(0, 63, 65, 127, 128, 191, 192, 255, 257, 270, 280, 290, 298, 299))
    wide = len(out)
    # the guard of the store's partial group (reveal_check_cases.GUARD_DIMS): one refused and one faulty row at each
    for dim in vc.GUARD_DIMS:
        add("k8_62", "k8_62", dim, K8_ALL, 16, (12,), 1)
    return out, parent, wide


CASES, PARENT_CASES, WIDE_CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NEW = tuple(c.name for c in CASES[PARENT_CASES:WIDE_CASES])                  # ... and these came with it
GUARD = tuple(c.name for c in CASES[WIDE_CASES:])                            # ... and these with the store the finishes share
E2E = "k3_62-c4-d764-f2-e1-zero"


def batches(case):
    return vc.batches(case)


def cap_of(case):
    """e': what the finish decodes with at most"""
    f = len(case.erased)
    if f > case.checks:
        return 0
    room = (case.checks - f) // 2
    return min(case.cap, room) if case.cap else room


def tables(case):
    return vc.tables(case.scheme, case.indices, case.checks)


def ok_words(case):
    """the d_ok array of the case (None: NULL)"""
    if case.ok == "null":
        return None
    ok = np.ones(len(case.indices), dtype=np.uint32)
    ok[list(case.erased)] = 0
    if case.ok == "ones":
        ok[:] = np.arange(1, len(ok) + 1, dtype=np.uint32) * 0x01010101      # any non-zero word
    return ok


# ---- the definition, piece by piece ------------------------------------------------------------------------------------------------
def gamma_of(xF, p):
    """the coefficients of prod (z - x), ascending"""
    g = [1]
    for x in xF:
        g = [((g[m - 1] if m else 0) - x * (g[m] if m < len(g) else 0)) % p for m in range(len(g) + 1)]
    return g


def modified(S, g, p):
    f = len(g) - 1
    return [sum(g[m] * S[j + m] for m in range(f + 1)) % p for j in range(len(S) - f)]


def solve_batch(S, x, F, e, p, plant=None):
    """-> ("clean" | "consistent" | "decoded" | "undecoded", [(position, Y) of E], [(position, Y) of F])"""
    f, c = len(F), len(S)
    if not any(S):
        return "clean", [], [(j, 0) for j in F]
    g = gamma_of([x[j] for j in F], p)
    if plant == "gamma_reversed":
        g = g[::-1]
    T = modified(S, g, p)
    live = [i for i in range(len(x)) if i not in F or plant == "root_on_erased"]
    E = []
    if any(T):
        got = dc.pgz(T, [x[i] for i in live], e, p)
        if got is None and plant == "cap_from_c" and len(x) <= 8:           # a cap past floor((c - f) / 2): the first subset that fits
            for nu in range(1, min(e, len(T)) + 1):
                for at in itertools.combinations(range(len(live)), nu):
                    Z = dc.magnitudes(T, [x[live[a]] for a in at], p)
                    if got is None and Z is not None and all(Z) and dc.reproduces(T, [x[live[a]] for a in at], Z, p):
                        got = list(zip(at, Z))
        if got is None:
            return "undecoded", [], []
        for at, Z in got:
            i = live[at]
            G = sum(g[m] * pow(x[i], m, p) for m in range(f + 1)) % p
            if plant == "z_not_divided":
                G = 1
            if G == 0:                                                       # only a planted fault gets here
                G = 1
            E.append((i, Z * pow(G, -1, p) % p))
    rhs = [(S[d] - (0 if plant == "errors_not_removed" else sum(y * pow(x[i], d, p) for i, y in E))) % p for d in range(f)]
    YF = dc.solve([[pow(x[j], d, p) for j in F] for d in range(f)], rhs, p) if f else []
    assert YF is not None
    both = E + list(zip(F, YF))
    if plant is None:                                                        # the definition, checked on the ORIGINAL syndromes
        assert all(sum(y * pow(x[i], d, p) for i, y in both) % p == S[d] for d in range(c)), "the model's solution does not reproduce S"
        assert all(y for _, y in E) and len({i for i, _ in E}) == len(E) and not set(F) & {i for i, _ in E}
    return ("decoded" if E else "consistent"), E, list(zip(F, YF))


@functools.lru_cache(maxsize=None)
def _solved(S, scheme, indices, checks, F, e, plant):
    """solve_batch, remembered: both policies, and every test that asks again, solve a batch once"""
    T = vc.tables(scheme, indices, checks)
    return solve_batch(list(S), T.x, list(F), e, T.p, plant)


def brute_force(S, x, F, e, p):
    """the definition without T: every subset E of 0 .. e non-erased positions for which Y on E u F (non-zero on E) reproduces all
    c syndromes -> [(E as [(position, Y)], F as [(position, Y)])]  (small committees only)"""
    assert len(x) <= 8
    f, c = len(F), len(S)
    found = []
    others = [i for i in range(len(x)) if i not in F]
    for nu in range(0, e + 1):
        if nu + f > c:
            break
        for E in itertools.combinations(others, nu):
            pos = list(E) + list(F)
            Y = dc.solve([[pow(x[i], d, p) for i in pos] for d in range(len(pos))], S[:len(pos)], p) if pos else []
            if Y is None or not all(Y[:nu]):
                continue
            if all(sum(y * pow(x[i], d, p) for i, y in zip(pos, Y)) % p == S[d] for d in range(c)):
                found.append((list(zip(E, Y[:nu])), list(zip(F, Y[nu:]))))
    return found


# ---- the model of the whole finish -------------------------------------------------------------------------------------------------
Finish = collections.namedtuple("Finish", "out report verdicts errors erasures")
PLANTS = ("gamma_reversed", "root_on_erased", "z_not_divided", "errors_not_removed", "one_erasure_skipped", "cap_from_c", "f_over_swapped",
          "padding_stored")
# ... and faults of the setup kernel's compaction and of a position's width, which only a wide committee can notice
# (tests/test_reveal_erasure_reach.py says which cases do):
#   compaction_restarts  the erased positions of a later 256-step are numbered from the step's own start
#   keeps_last_16        the kept list is filled from its first slot again in every step: a later step's positions overwrite
#                        the earlier ones (f itself is counted right)
#   position_mod_256     a located or erased position loses its high byte in blame and correction
#   counts_kept_only     f is reported, and compared with the checks, as min(f, 16)
GAP_PLANTS = ("compaction_restarts", "keeps_last_16", "position_mod_256", "counts_kept_only")


def planted_erasures(F, checks, plant):
    """-> (the erased positions the finish works with, f as reported, the overflow word) under a fault of GAP_PLANTS"""
    F, f = list(F), len(F)
    if plant == "compaction_restarts":
        F = sorted({j % STEP for j in F})
        f = len(F)
    elif plant == "keeps_last_16":
        kept = []
        for step in sorted({j // STEP for j in F}):
            here = [j for j in F if j // STEP == step]
            kept = here + kept[len(here):]
        F = sorted(kept)
    elif plant == "counts_kept_only":
        f = min(f, KEPT)
        F = F[:f]
    return F, f, f > checks


def model_finish(case, rows, policy, plant=None):
    """what finish_erasures_dev must store and report for any-int64 rows.  verdicts: per batch "clean", "consistent" (T = 0, S != 0:
    repaired by its erasures alone), nu (decoded) or -1 (undecoded); plant: one of PLANTS, a fault planted in the MODEL (tests only)"""
    T = tables(case)
    p, k, n_rows, c = T.p, T.k, len(case.indices), case.checks
    F = list(case.erased) if case.ok == "flags" else []
    f = len(F)
    over = f > c
    if plant in GAP_PLANTS:
        F, f, over = planted_erasures(F, c, plant)
    low = (lambda i: i % 256) if plant == "position_mod_256" else (lambda i: i)
    e = cap_of(case)
    if plant in GAP_PLANTS and not over:
        e = min(case.cap, (c - len(F)) // 2) if case.cap else (c - len(F)) // 2
    if plant == "cap_from_c" and not over:
        e = min(case.cap, c // 2) if case.cap else c // 2
    B = batches(case)
    out, blame, hist = [], [0] * n_rows, [0] * MAX_ERRORS
    bad = decoded = corrected = most = 0
    first_bad = first_undecoded = NONE64
    verdicts, errors, erasures = [], [], []
    for b in range(B):
        sh = [int(rows[i][b]) % p for i in range(n_rows)]
        sec = [sum(T.R[s][i] * sh[i] for i in range(n_rows)) % p for s in range(k)]
        S = [sum(T.H[d][i] * sh[i] for i in range(n_rows)) % p for d in range(c)]
        verdict, E, YF = "clean", [], []
        if not over:
            kind, E, YF = _solved(tuple(S), case.scheme, case.indices, c, tuple(F), e, plant)
            verdict = {"clean": "clean", "consistent": "consistent", "decoded": len(E), "undecoded": -1}[kind]
            if kind in ("decoded", "undecoded"):
                bad += 1
                first_bad = min(first_bad, b)
            if kind == "undecoded":
                first_undecoded = min(first_undecoded, b)
            if kind == "decoded":
                nu = len(E)
                decoded += 1
                most = max(most, nu)
                hist[nu - 1] += 1
                for i, _ in E:
                    blame[low(i)] += 1
                if policy == CORRECT:
                    corrected += 1
            if policy == CORRECT and kind in ("consistent", "decoded"):
                fix = E + (YF[:-1] if plant == "one_erasure_skipped" else YF)
                sec = [(sec[s] - sum(T.corr[s][low(i)] * y for i, y in fix)) % p for s in range(k)]
        verdicts.append(verdict)
        errors.append(E)
        erasures.append(YF)
        out.extend(sec)
    tail = [int(over), f] if plant == "f_over_swapped" else [f, int(over)]
    report = [bad, decoded, corrected, first_bad, first_undecoded, most] + tail + hist + blame
    return Finish(np.array(out if plant == "padding_stored" else out[:case.dim], dtype=np.int64), report, verdicts, errors, erasures)


# ---- rows --------------------------------------------------------------------------------------------------------------------------
Built = collections.namedtuple("Built", "rows clean_rows want row_len batches faulty")


def _base(case):
    """the clean rows of reveal_check_cases' builder under a name of this table"""
    base = vc.Case("erasure/" + case.name, case.scheme, case.dim, case.indices, case.checks, "sums", "none", "one", 0, None)
    vc.BY_NAME.setdefault(base.name, base)                                   # BY_NAME only: vc.CASES, what its own tests walk, stays
    return vc.build(base.name)


@functools.lru_cache(maxsize=None)
def build(name):
    """rows [positions][row_len] int64 with the erased rows filled and the errors planted, the clean rows, the true secrets and, per
    batch, the tuple of faulty NON-erased positions"""
    case = BY_NAME[name]
    base = _base(case)
    p = tables(case).p
    pos, B = len(case.indices), base.batches
    rng = np.random.default_rng(zlib.crc32(("erasure/" + name).encode()))
    rows = base.rows.copy()
    others = [i for i in range(pos) if i not in case.erased]
    order = [others[int(i)] for i in rng.permutation(len(others))]
    if case.pin is not None:
        assert not set(case.pin) & set(case.erased)
        order = list(case.pin) + [i for i in order if i not in case.pin]
    e = cap_of(case)
    if case.errors == "steered":
        per = _steer(case, rows, B, rng)
    elif case.errors == "mixed":
        per = [tuple(sorted(order[(b + j) % len(order)] for j in range({0: 0, 1: 0, 2: e, 3: e + 1}[b % 4]))) for b in range(B)]
    elif case.errors == "aimed":
        per = [tuple(sorted(order[:case.checks - len(case.erased)]))] * B
        _aim(case, rows, per[0], B, rng)
    else:
        per = [tuple(sorted(order[:case.errors]))] * B
    for i in others if case.errors not in ("aimed", "steered") else ():
        bs = np.array([b for b in range(B) if i in per[b]], dtype=np.int64)
        if bs.size:
            rows[i, bs] = vc._add(rows[i, bs], vc._errors(rng, p, bs.size), p)
    for j in case.erased:
        if case.fill == "zero":
            rows[j, :] = 0
        elif case.fill == "random":
            rows[j, :] = rng.integers(0, p, size=rows.shape[1], dtype=np.int64)
        elif case.fill == "spoiled":
            rows[j, :B] = vc._add(rows[j, :B], vc._errors(rng, p, B), p)
        else:
            assert case.fill == "clean"
        if case.errors == "mixed":                                           # b mod 4 = 0: a clean lane
            rows[j, 0:B:4] = base.rows[j, 0:B:4]
    return Built(rows, base.clean_rows, base.want, base.row_len, B, per)


def _aim(case, rows, at, B, rng):
    """errors on the c - f positions `at` whose modified syndromes are W x_j^d, d < c - f - those of ONE error on the erased position
    j: the first erased one (on a committee wider than one step of the setup kernel the last one, so that the refused root sits
    past position 255)"""
    T = tables(case)
    p, x = T.p, T.x
    j = case.erased[0] if len(case.indices) <= STEP else case.erased[-1]
    g = gamma_of([x[q] for q in case.erased], p)
    weight = {i: sum(g[m] * pow(x[i], m, p) for m in range(len(g))) % p for i in at}
    for batch in range(B):
        W = int(rng.integers(1, p))
        dc.steer(rows, T, at, batch, [W * pow(x[j], d, p) % p for d in range(len(at))], weight)


def _steer(case, rows, B, rng):
    """errors on the c - f pinned positions so that batch b's MODIFIED syndromes are those of family b mod F: the Vandermonde
    system gives Z, the error is Z_i / (Gamma(x_i) u_i).  -> per batch, the positions whose error is not zero"""
    T = tables(case)
    p, n = T.p, case.checks - len(case.erased)
    assert len(case.pin) == n >= 3
    g = gamma_of([T.x[q] for q in case.erased], p)
    weight = {i: sum(g[m] * pow(T.x[i], m, p) for m in range(len(g))) % p for i in case.pin}
    z, fams = dc.no_point(T, rng), dc.families(n)
    pts = [T.x[i] for i in case.pin]
    return [dc.steer(rows, T, case.pin, b, dc.family_syndromes(fams[b % len(fams)], n, pts, z, cap_of(case), p, rng), weight) for b in range(B)]


def refilled(name, fill):
    """the case's rows with its erased rows filled another way (the same errors): the finish must not tell the difference"""
    case, b = BY_NAME[name], build(name)
    rows = b.rows.copy()
    rng = np.random.default_rng(zlib.crc32(("refill/" + name + fill).encode()))
    for j in case.erased:
        rows[j, :] = 0 if fill == "zero" else rng.integers(0, tables(case).p, size=rows.shape[1], dtype=np.int64)
    return rows


def expected_verdicts(case, built):
    """what the GUARANTEES say per batch from the planted faults alone: "ok" (clean or consistent), nu, -1, or None where they
    promise nothing"""
    f, c, e = len(case.erased) if case.ok == "flags" else 0, case.checks, cap_of(case)
    if f > c:
        return ["clean"] * built.batches
    return ["ok" if not q else len(q) if len(q) <= e else -1 if len(q) <= c - f - e else None for q in built.faulty]

"""Operands, boundary points, case tables and Python-integer models for the reference-representative kernels
(SDA_VALUES_RUST_SIGNED: sda_amd/csrc/signed_rem.hpp, signed_kernels.hip, signed_additive_gen_drbg_kernel of sda_kernels.hip).

The header's contract: the sum or difference of two int64 is formed EXACTLY (128 bits), then reduced with Rust's truncated `%`
(sign of the dividend).  trunc_rem128 has four branches,
    near  |x| < q            -> x            high  q <= x < 2q      -> x - q
    low   -2q < x <= -q      -> x + q        far   everything else  -> x % q
and the values at which they meet, x = +-q, +-2q, +-(2q - 1), are the places where an off-by-one compare would go unseen by
random operands.  Everything here is Python integers; numpy appears only where a table is handed to the device.
tests/test_signed_limits_reach.py proves on the CPU what the tables reach, tests/test_signed_limits_gpu.py runs them."""
import functools
import random

MIN, MAX = -(1 << 63), (1 << 63) - 1
MODULI = (2, 3, 433, 1 << 61, (1 << 62) - 57, (1 << 62) - 1)          # the last one is the largest make_mod admits
BRANCHES = ("near", "high", "low", "far")
FIXED_POINTS = ("-2q", "-2q+1", "-q-1", "-q", "-q+1", "q-1", "q", "q+1", "2q-1", "2q", "-2^64", "-2^64+1", "2^64-1")
POINTS = FIXED_POINTS + ("positive multiple beyond 2q", "negative multiple beyond 2q")
# a difference of two int64 is at least MIN - MAX = -2^64 + 1: only a SUM reaches -2^64 (and only a difference 2^64 - 1)
POINTS_OF_A_DIFFERENCE = tuple(p for p in POINTS if p != "-2^64")
COMBINE_BOUNDARIES = ("q", "-q", "2q", "-2q", "2q-1", "-2q+1")


def fits(v):
    return MIN <= v <= MAX


def specials(q):
    """the int64 values at and around every boundary of trunc_rem128 for the modulus q, and at the ends of int64"""
    K = MAX // q * q                                                   # the largest multiple of q in int64
    cand = [0, 1, -1]
    for v in (q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1):
        cand += [v, -v]
    cand += [MIN, MIN + 1, MAX, MAX - 1]
    for v in (1 << 62, (1 << 62) - 1, K, K - 1):
        cand += [v, -v]
    cand.append(-((1 << 63) // q) * q)                                 # the multiple of q nearest above INT64_MIN
    out = []
    for v in cand:
        if fits(v) and v not in out:
            out.append(v)
    return out


def branch(x, q):
    """which of trunc_rem128's four returns x takes, in the header's order"""
    if -q < x < q:
        return "near"
    if q <= x < 2 * q:
        return "high"
    if -2 * q < x <= -q:
        return "low"
    return "far"


def point_values(q):
    return {"-2q": -2 * q, "-2q+1": -2 * q + 1, "-q-1": -q - 1, "-q": -q, "-q+1": -q + 1, "q-1": q - 1, "q": q, "q+1": q + 1,
            "2q-1": 2 * q - 1, "2q": 2 * q, "-2^64": -(1 << 64), "-2^64+1": -(1 << 64) + 1, "2^64-1": (1 << 64) - 1}


def points_hit(x, q):
    """the names of POINTS that x is (several for a small q, where e.g. -2q + 1 == -q - 1).  The two multiples are taken
    strictly beyond 2q, so that they are other values than the points 2q and -2q"""
    hit = {name for name, v in point_values(q).items() if v == x}
    if x % q == 0 and x > 2 * q:
        hit.add("positive multiple beyond 2q")
    if x % q == 0 and x < -2 * q:
        hit.add("negative multiple beyond 2q")
    return hit


class Reach:
    """the branches and points a list of dividends x takes"""

    def __init__(self, q):
        self.q, self.branches, self.points = q, set(), set()

    def add(self, x):
        assert -(1 << 64) <= x <= (1 << 64) - 1, x                     # what a sum or difference of two int64 can be
        self.branches.add(branch(x, self.q))
        self.points |= points_hit(x, self.q)
        return x


# ---- the kernels, restated from their text on Python integers -------------------------------------------------------------------------
def trem(x, q):
    """trunc_rem128, branch for branch; the last one is C's `%` on __int128 (quotient rounded towards zero)"""
    if -q < x < q:
        return x
    if q <= x < 2 * q:
        return x - q
    if -2 * q < x <= -q:
        return x + q
    return x - q * (abs(x) // q) * (1 if x > 0 else -1)


def model_generate(secrets, rand, n, q, reach=None):
    """signed_additive_gen_kernel: out[j][i] = rand[i (n - 1) + j], out[n - 1][i] = the fold acc = (acc - r) % q from the raw secret"""
    out = [[0] * len(secrets) for _ in range(n)]
    for i, s in enumerate(secrets):
        acc = s
        for j in range(n - 1):
            r = rand[i * (n - 1) + j]
            out[j][i] = r
            x = acc - r
            if reach is not None:
                reach.add(x)
            acc = trem(x, q)
        out[n - 1][i] = acc
    return out


def model_combine(rows, q, state=None, reach=None, step_reach=None):
    """signed_combine_update_kernel: state[col] = (state[col] + row[col]) % q, row after row; the state starts at 0 (begin)"""
    state = [0] * len(rows[0]) if state is None else list(state)
    for k, row in enumerate(rows):
        for c, v in enumerate(row):
            x = state[c] + v
            if reach is not None:
                reach.add(x)
            if step_reach is not None and k in step_reach:
                step_reach[k].add(x)
            state[c] = trem(x, q)
    return state


def model_addsub(a, b, subtract, q, reach=None):
    """signed_addsub_kernel: (a - b) % q or (a + b) % q"""
    out = []
    for u, v in zip(a, b):
        x = u - v if subtract else u + v
        if reach is not None:
            reach.add(x)
        out.append(trem(x, q))
    return out


# ---- the case tables --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_table(q):
    """specials(q)^2 laid out as two vectors (at most 729 elements: two full 256-thread workgroups and a ragged third)"""
    sp = specials(q)
    return [a for a in sp for _ in sp], [b for _ in sp for b in sp]


GEN_N = (1, 2, 3, 5)


@functools.lru_cache(maxsize=None)
def generate_table(q, n):
    """(secrets, rand): secret x first draw run through specials(q)^2, draw j > 0 of element i is specials[(5 i + j) mod len] -
    rand[i (n - 1) + j], the layout the reference's draw order gives (batched.rs:46-48)"""
    sp = specials(q)
    secrets, first = pair_table(q)
    rand = []
    for i in range(len(secrets)):
        for j in range(n - 1):
            rand.append(first[i] if j == 0 else sp[(5 * i + j) % len(sp)])
    return list(secrets), rand


def generate_rolled(q, n, roll):
    """generate_table(q, n) with its elements rotated by `roll`: another participant of a device call"""
    secrets, rand = generate_table(q, n)
    r = roll % len(secrets)
    return secrets[r:] + secrets[:r], rand[r * (n - 1):] + rand[:r * (n - 1)]


def cycle(q, elements, start=MIN):
    """`elements` values cycling through specials(q), the first one `start` (INT64_MIN: a sum with a draw in [0, q) stays negative)"""
    sp = specials(q)
    k = sp.index(start)
    return [sp[(k + i) % len(sp)] for i in range(elements)]


def grid_pairs(q, elements):
    """element i pairs specials[i mod L] with specials[(i div L) mod L]: L^2 elements run through specials(q)^2 once"""
    sp = specials(q)
    L = len(sp)
    return [sp[i % L] for i in range(elements)], [sp[i // L % L] for i in range(elements)]


BIG_JOB = (65535 + 2, 3, 2)                                            # participants, dimension, n: blockIdx.y is sliced at 65535
BIG_JOB_MODULI = (433, (1 << 62) - 1)
CHACHA_DIMS = (1, 256, 257)
CHACHA_SEED = (1, 2, 3, 0xFFFFFFFF)
DRBG_DIMS = (1, 2, 511, 512, 513)                                      # one workgroup serves 512 elements, two per lane
DRBG_N = (2, 5)
DRBG_CANDIDATES = MODULI + ((1 << 31) - 1,)                            # one modulus per sda_drbg_draw_rule among these, and 2^62 - 1
DRBG_MODULI = (2, 433, (1 << 31) - 1, 1 << 61, (1 << 62) - 1)          # (two per rule; the GPU test asks the library for the rules)
DRBG_FIRST = (1 << 56) - 2                                             # two participants end at the last stream id (2^56 - 1)
DRBG_KEY = bytes(range(11, 43))


def drbg_secrets(q, dim):
    """the two participants' secrets: both cycles start below zero, so that a draw in [0, q) leaves the fold's dividend negative"""
    return [cycle(q, dim), cycle(q, dim, MIN + 1)]


COMBINE_DIMS = (1, 255, 256, 257)
COMBINE_RANDOM_ROWS = 37


def combine_firsts(q):
    out = []
    for v in (0, 1, -1, q - 1, -(q - 1)):
        if v not in out:
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def combine_table(q, dim, shift=0):
    """[2 + 37][dim] rows: column c holds pair (c + shift) of combine_firsts(q) x specials(q) in rows 0 and 1 - the first row sets the
    running value, the second lands on the boundaries - then 37 rows drawn from specials(q) with a fixed seed, so the sign of every
    later running value depends on its history.  `shift` gives the jobs of a device call different columns"""
    sp = specials(q)
    pairs = [(f, s) for s in sp for f in combine_firsts(q)]
    cols = [pairs[(c + shift) % len(pairs)] for c in range(dim)]
    head = [[f for f, _ in cols], [s for _, s in cols]]
    for attempt in range(64):                                          # (a single column may end non-negative: the next seed then)
        rng = random.Random(q % 1000003 + 7919 * dim + shift + 104729 * attempt)
        rows = head + [[sp[rng.randrange(len(sp))] for _ in range(dim)] for _ in range(COMBINE_RANDOM_ROWS)]
        if any(v < 0 for v in model_combine(rows, q)):
            return tuple(tuple(r) for r in rows)
    raise AssertionError("no seed gives a negative sum")


def canonical(values, q):
    return [v % q for v in values]


def tells_signed_from_canonical(values, q):
    """the expectation has negative values, so it differs from the residues in [0, q): a route that fell back to the canonical kernel fails"""
    return any(v < 0 for v in values) and list(values) != canonical(values, q)

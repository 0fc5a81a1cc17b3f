"""Crafted share rows for the clerk sums at the carry limits of their 128-bit accumulators (shared by
tests/test_clerk_limits_reach.py and tests/test_clerk_limits_gpu.py - a helper module, not a conftest).

The clerk sum adds ANY i64 rows into exact column accumulators (an unsigned low word, a signed high word: acc_add /
acc_atomic_add in modarith.hpp) that mod_i128 reduces once at finish.  This module holds
  * column_patterns / crafted_matrix / crafted_jobs: columns that make the low word wrap, the high word grow, cancel or sit at
    -1, and totals that are negative multiples of the modulus;
  * want: the reference - Python integer column sums, nothing from the library or the C oracle;
  * the split geometry of the launchers, restated (combine_split: launch_combine_update; fuse_split: fuse_plan and the clerk
    workgroups of ngemm_launch_fused; window_rows: launch_varint_stream_combine);
  * a plain Python model of the three accumulation schemes (acc_add over a row range with acc_atomic_add of the per-split
    partials, the read-modify-write ending, the two-plane LDS window with its fold) that records which special cases a given
    input reaches.  The model produces NO expected values: tests/test_clerk_limits_reach.py uses it to prove that the crafted
    inputs of every GPU case reach the carries they are meant to reach, so the GPU test cannot pass vacuously;
  * the case tables both test modules run."""
import numpy as np

MIN, MAX = -(1 << 63), (1 << 63) - 1
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
P62 = 4611686006577364993
PMAX = (1 << 62) - 57
P31MAX = (1 << 31) - 1
NGEMM_PMAX = 8355691
MODULI = (PMAX, P62, P31MAX, NGEMM_PMAX, 433, 2)

PATTERNS = ("all MIN", "all MAX", "all -1", "MIN / MAX", "+1 / -1", "MIN every 16", "all m - 1", "all -m", "-1 then -m", "all 0",
            "uniform")
NPAT = len(PATTERNS)
STRIDE = 3                       # pattern of column c: (first + 3 c) mod 11 - coprime, so even and odd columns each meet all 11


def column_patterns(rows, m, seed=0):
    """name -> int64 column of `rows` values.  "+1 / -1" sums to 0 when `rows` is even."""
    r = np.arange(rows)
    neg_m = np.full(rows, -m, dtype=np.int64)
    first_neg1 = neg_m.copy()
    first_neg1[0] = -1
    cols = {
        "all MIN": np.full(rows, MIN, dtype=np.int64),
        "all MAX": np.full(rows, MAX, dtype=np.int64),
        "all -1": np.full(rows, -1, dtype=np.int64),
        "MIN / MAX": np.where(r % 2 == 0, MIN, MAX).astype(np.int64),
        "+1 / -1": np.where(r % 2 == 0, 1, -1).astype(np.int64),
        "MIN every 16": np.where(r % 16 == 0, MIN, 0).astype(np.int64),
        "all m - 1": np.full(rows, m - 1, dtype=np.int64),
        "all -m": neg_m,
        "-1 then -m": first_neg1,
        "all 0": np.zeros(rows, dtype=np.int64),
        "uniform": np.random.default_rng(1000003 * seed + rows).integers(MIN, MAX, size=rows, dtype=np.int64, endpoint=True),
    }
    assert tuple(cols) == PATTERNS
    return cols


def pattern_of(c, first=0):
    return PATTERNS[(first + STRIDE * c) % NPAT]


def crafted_matrix(rows, dim, m, first=0):
    """[rows][dim]: the patterns cycle over the columns, column c holds pattern (first + 3 c) mod 11.  From 22 columns on every
    pattern lands on an even and on an odd column; the last column of an odd `dim` holds ONE pattern per matrix, so callers vary
    `first` (crafted_jobs: per job; the case tables: per modulus as well) until every pattern has been there."""
    pats = column_patterns(rows, m, seed=first)
    out = np.empty((rows, dim), dtype=np.int64)
    for c in range(dim):
        out[:, c] = pats[pattern_of(c, first)]
    return out


def crafted_jobs(jobs, rows, dim, m, first=0):
    """[jobs][rows][dim]: job j is crafted_matrix(rows, dim, m, first + j)"""
    return np.stack([crafted_matrix(rows, dim, m, first + j) for j in range(jobs)])


def want(matrix, m):
    """the reference: per column sum(int(x) for x in column) % m in Python integers.  [rows][dim] -> int64 [dim];
    [jobs][rows][dim] -> [jobs][dim]"""
    a = np.asarray(matrix)
    if a.ndim == 3:
        return np.stack([want(j, m) for j in a])
    return np.array([sum(int(x) for x in a[:, c].tolist()) % m for c in range(a.shape[1])], dtype=np.int64)


def first_difference(got, expect, first=0):
    """None, or "(job, column, pattern name)" of the first differing sum of [jobs][dim] arrays"""
    got, expect = np.asarray(got), np.asarray(expect)
    if np.array_equal(got, expect):
        return None
    j, c = (int(x) for x in np.argwhere(got != expect)[0])
    return f"job {j}, column {c}, pattern {pattern_of(c, first + j)!r}: got {int(got[j, c])}, want {int(expect[j, c])}"


# ---- the launchers' geometry, restated ------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def combine_split(n_rows, dimension, jobs):
    """launch_combine_update: (splits, rows_per_split).  Enough workgroups for 256 CUs 16 times over, at least 16 rows per split;
    one split = the plain read-modify-write ending, more = atomics"""
    col_blocks = _ceil(_ceil(dimension, 2), 256)
    split = 1
    if col_blocks * jobs < 4096:
        split = _ceil(4096, col_blocks * jobs)
    split = max(1, min(split, _ceil(n_rows, 16), 65535))
    rps = _ceil(n_rows, split)
    return _ceil(n_rows, rps), rps


def fuse_split(prev_rows):
    """fuse_plan (and the clerk workgroups of ngemm_launch_fused): clerk items of up to 512 rows, at most 64 of them"""
    splits = min(_ceil(prev_rows, 512), 64)
    rps = _ceil(prev_rows, splits)
    return _ceil(prev_rows, rps), rps


def window_rows(rows_per_job, jobs):
    """launch_varint_stream_combine: rows of one job per workgroup (the 16-row or the 8-row instance)"""
    return 16 if _ceil(rows_per_job, 16) * jobs >= 512 else 8


# ---- the model -------------------------------------------------------------------------------------------------------------------
WRAP_NEG = "acc_add: low word wraps, v < 0"
WRAP_POS = "acc_add: low word wraps, v >= 0"
RMW_CARRY = "read-modify-write: carry into the stored high word"
RMW_HIGH = "read-modify-write: stored high word already non-zero"
LOW_ZERO = "atomic: partial low word 0, high word non-zero"
ZERO_ZERO = "atomic: partial (0, 0)"
CANCEL = "atomic: the low word's carry cancels a high word of -1"
ATOMIC_CARRY = "atomic: carry out of the low word"
FOLD_CARRY = "window: cell with Bq < 0 whose fold carries"
CELL_8 = "window: cell with 8 adds"
CELL_16 = "window: cell with 16 adds"
DIRECT = "window: add beyond the window goes straight to the accumulator"
NEG_MULTIPLE = "mod_i128: negative total, exact multiple of the modulus"
HIGH_GE_M = "mod_i128: |high word| >= modulus"


def _s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def acc_add(lo, hi, v, ev):
    """modarith.hpp acc_add: (lo, hi) += v"""
    nl = (lo + (v & M64)) & M64
    carry = 1 if nl < lo else 0
    if carry:
        ev.add(WRAP_NEG if v < 0 else WRAP_POS)
    return nl, _s64(hi + (v >> 63) + carry)


def acc_range(values, ev):
    lo = hi = 0
    for v in values:
        lo, hi = acc_add(lo, hi, int(v), ev)
    return lo, hi


def acc_atomic_add(cell, lo, hi, ev):
    """modarith.hpp acc_atomic_add on cell = [low word, high word]"""
    if lo == 0:
        ev.add(LOW_ZERO if hi != 0 else ZERO_ZERO)
    else:
        old = cell[0]
        cell[0] = (old + lo) & M64
        if cell[0] < old:
            ev.add(ATOMIC_CARRY)
            if hi == -1:
                ev.add(CANCEL)
            hi += 1
    if hi != 0:
        cell[1] = _s64(cell[1] + hi)


def rmw_add(cell, lo, hi, ev):
    """the plain ending of combine_pair, flush of ng_clerk_wave, the ending of ngemm_clerk_rest_kernel"""
    if cell[1] != 0:
        ev.add(RMW_HIGH)
    nl = (cell[0] + lo) & M64
    carry = 1 if nl < cell[0] else 0
    if carry:
        ev.add(RMW_CARRY)
    cell[0], cell[1] = nl, _s64(cell[1] + hi + carry)


def split_sum(cell, column, splits, rps, ev, order=None):
    """one update of one column: acc_add over each split's rows, then the read-modify-write ending (one split) or
    acc_atomic_add of the partials in `order` (a permutation of the splits; None: ascending)"""
    parts = [acc_range(column[z * rps:(z + 1) * rps], ev) for z in range(splits)]
    if splits == 1:
        rmw_add(cell, *parts[0], ev)
        return
    for z in (range(splits) if order is None else order):
        acc_atomic_add(cell, *parts[z], ev)


def window_sum(cell, column, W, ev, direct=()):
    """one update of one column through the LDS window: per workgroup of W rows a cell of two planes (sum of the low 32 bits,
    sum of the arithmetic high 32 bits), folded as A + (Bq << 32) with a carry and added with acc_atomic_add; rows listed in
    `direct` have run ahead of the window and add (v, v >> 63) straight to the accumulator"""
    for g0 in range(0, len(column), W):
        A = Bq = adds = 0
        for r in range(g0, min(g0 + W, len(column))):
            v = int(column[r])
            if r in direct:
                ev.add(DIRECT)
                acc_atomic_add(cell, v & M64, v >> 63, ev)
                continue
            A += v & M32
            Bq += v >> 32
            adds += 1
        assert A < 1 << 64 and -(1 << 63) <= Bq < 1 << 63
        if adds == 8:
            ev.add(CELL_8)
        if adds == 16:
            ev.add(CELL_16)
        if A == 0 and Bq == 0:
            continue
        lo = (A + ((Bq << 32) & M64)) & M64
        carry = 1 if lo < A else 0
        if carry and Bq < 0:
            ev.add(FOLD_CARRY)
        acc_atomic_add(cell, lo, (Bq >> 32) + carry, ev)


def finish(cell, m, total, ev):
    """mod_i128's branches, and the model's own proof: the accumulator IS the Python sum"""
    value = (cell[1] << 64) + cell[0]
    assert value == total, (value, total)
    if total < 0 and total % m == 0:
        ev.add(NEG_MULTIPLE)
    if (abs(total) >> 64) >= m:
        ev.add(HIGH_GE_M)


def orders(splits):
    """split orders the atomics are tried in: ascending, descending, a seeded shuffle"""
    return (None, list(range(splits - 1, -1, -1)), [int(x) for x in np.random.default_rng(splits).permutation(splits)])


# ---- the case tables of tests/test_clerk_limits_gpu.py ---------------------------------------------------------------------------
def first_for(m):
    """the pattern offset of a modulus: with three jobs (offsets first .. first + 2) the six moduli put every pattern on every
    column, the last one of an odd dimension included"""
    return 3 * MODULI.index(m)


# plain ending: one begin, then update_dev with 16, 9 and 1 rows, five rounds (each <= 16 rows: one split)
PLAIN_ROWS = (16, 9, 1) * 5
PLAIN_DIMS = (1023, 1)
PLAIN_JOBS = 3
# atomic ending: (jobs, dimension, n_rows, what): 65 splits of 16 rows; 64 of 16 with a last split of 15; an odd rows_per_split
# (41 splits of 25: only a launch whose columns x jobs come near the workgroup target gets more than 16 rows per split)
ATOMIC_CASES = ((3, 37, 1030), (3, 37, 1023), (100, 23, 1023))
# side-stream walk kernel, dual-role launches, narrow limb GEMM: previous tiles of these many crafted rows, in this order
WALK_PREV = (40, 1030)
DUAL_PREV = (3, 40, 1030)
NGEMM_PREV = (5, 40, 1030)
# wire-fed sums: (name, jobs, rows per job, L)
WIRE_CASES = (("8 rows", 1, 24, 300), ("16 rows", 512, 16, 40))
DRIFT_ROWS, DRIFT_L = 32, 5000


def drift_matrix(long_value):
    """half the rows all -1 (one byte on the wire), half all `long_value` (MIN or MAX: ten bytes): the short rows run more than
    2048 columns ahead of the long ones"""
    a = np.empty((DRIFT_ROWS, DRIFT_L), dtype=np.int64)
    a[0::2] = -1
    a[1::2] = long_value
    return a


def drift_direct(L=DRIFT_L):
    """the columns of drift_matrix in which the short (even) rows bypass the window: the streams advance a group of four 1 KiB chunks per
    step in lockstep, a one-byte row ~4096 columns and a ten-byte row ~409; the window starts at the slowest row's column and is
    2048 columns wide, so the short (even) rows are beyond it in the columns below"""
    step_bytes = 4 * 1024
    out = set()
    base, short_col, long_col = 0, 0, 0
    while long_col < L:
        nxt_short = min(L, short_col + step_bytes)
        for c in range(short_col, nxt_short):
            if c - base >= 2048:
                out.add(c)
        short_col = nxt_short
        long_col = min(L, long_col + step_bytes // 10)
        base = min(short_col, long_col)
    return out

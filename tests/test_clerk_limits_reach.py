"""Reach checks for the crafted rows of tests/test_clerk_limits_gpu.py (CPU): every case of the GPU tables is run through the plain
Python model of tests/clerk_limits.py with the split geometry the launchers use, and per form every special case the
accumulator code branches on must occur in at least one column - asserted by name - so that a later edit which makes the inputs
benign, or changes the row counts so that a carry no longer happens, fails here and not silently on the GPU box.  The model's
final 128-bit value must equal the Python sum in every column (clerk_limits.finish).

Which events a form can reach at all:
  * the low word wrapping inside acc_add (once with v < 0, once with v >= 0) and a negative total that is an exact multiple of the
    modulus: every form;
  * the read-modify-write carry and a stored high word that is already non-zero: every form with a one-split ending (the plain
    ending, dual-role items of up to 512 rows, the limb GEMM's clerk waves and follow-up kernel);
  * a partial of (0, non-zero), of (0, 0), and a carry that cancels a high word of -1: every form that ends in acc_atomic_add;
  * |high word| >= modulus: only where the modulus is small (433, 2) - the dual-role shapes' moduli are far above any high word
    that 1030 rows can build;
  * the window's fold with Bq < 0 and a carry, cells with 8 and with 16 adds, adds beyond the window: the wire-fed and sealed sums."""
import numpy as np
import pytest

import clerk_limits as CL

COMMON = (CL.WRAP_NEG, CL.WRAP_POS, CL.NEG_MULTIPLE)
RMW = (CL.RMW_CARRY, CL.RMW_HIGH)
ATOMIC = (CL.LOW_ZERO, CL.ZERO_ZERO, CL.CANCEL, CL.ATOMIC_CARRY)
WINDOW = (CL.FOLD_CARRY,)


def _require(events, names, form):
    for name in names:
        assert name in events, f"{form}: no column reaches `{name}`"


def _columns(calls):
    """calls: list of [jobs][rows][dim] -> per (job, column) the list of per-call columns"""
    jobs, _, dim = calls[0].shape
    for j in range(jobs):
        for c in range(dim):
            yield j, c, [t[j, :, c] for t in calls]


def _split_form(calls, splits_of, m, ev, order_index=0):
    """every column of every job through split_sum, call after call; splits_of(rows) -> (splits, rows_per_split)"""
    for j, c, cols in _columns(calls):
        cell = [0, 0]
        for col in cols:
            splits, rps = splits_of(len(col))
            CL.split_sum(cell, col, splits, rps, ev, CL.orders(splits)[order_index])
        CL.finish(cell, m, sum(int(x) for col in cols for x in col.tolist()), ev)


def test_patterns_and_reference():
    """the patterns are what their names say, every pattern lands on an even and an odd column, and - over the jobs and moduli
    of the plain-ending table - on the last column of an odd dimension"""
    for m in CL.MODULI:
        pats = CL.column_patterns(32, m)
        assert set(pats["all MIN"]) == {CL.MIN} and set(pats["all MAX"]) == {CL.MAX} and set(pats["all -1"]) == {-1}
        assert sum(int(x) for x in pats["+1 / -1"]) == 0 and list(pats["MIN / MAX"][:2]) == [CL.MIN, CL.MAX]
        assert [int(x) for x in np.flatnonzero(pats["MIN every 16"])] == [0, 16] and pats["MIN every 16"][16] == CL.MIN
        assert sum(int(x) for x in pats["all -m"]) % m == 0 and sum(int(x) for x in pats["-1 then -m"]) % m == m - 1
        assert sum(int(x) for x in pats["all m - 1"]) == 32 * (m - 1) and not pats["all 0"].any()
        assert pats["uniform"].min() < -(1 << 61) and pats["uniform"].max() > 1 << 61
    for dim in (22, 23, 37, 48, 49, 300, 1023):
        for first in range(CL.NPAT):
            assert {CL.pattern_of(c, first) for c in range(0, dim, 2)} == set(CL.PATTERNS)
            assert {CL.pattern_of(c, first) for c in range(1, dim, 2)} == set(CL.PATTERNS)
    for dim in CL.PLAIN_DIMS:
        assert dim % 2 == 1
        last = {CL.pattern_of(dim - 1, CL.first_for(m) + j) for m in CL.MODULI for j in range(CL.PLAIN_JOBS)}
        assert last == set(CL.PATTERNS), set(CL.PATTERNS) - last
    # the walk kernel's 6 columns: the 242 jobs carry every pattern to an even and to an odd column
    assert {CL.pattern_of(c, j) for j in range(242) for c in (0, 2, 4)} == {CL.pattern_of(c, j) for j in range(242) for c in (1, 3, 5)} == set(CL.PATTERNS)
    a = np.array([[CL.MIN, 5], [CL.MIN, -7], [CL.MAX, 0]], dtype=np.int64)
    assert CL.want(a, 433).tolist() == [(2 * CL.MIN + CL.MAX) % 433, 431]


def test_geometry_restated():
    assert CL.combine_split(16, 1023, 3) == (1, 16) and CL.combine_split(1, 1, 3) == (1, 1)
    assert CL.combine_split(1030, 37, 3) == (65, 16) and CL.combine_split(1023, 37, 3) == (64, 16)
    assert CL.combine_split(1023, 23, 100) == (41, 25)
    assert CL.combine_split(40, 6, 242) == (3, 14) and CL.combine_split(1030, 6, 242) == (17, 61)
    assert [CL.fuse_split(r) for r in (3, 5, 40, 512, 513, 1030, 40000)] == [(1, 3), (1, 5), (1, 40), (1, 512), (2, 257), (3, 344), (64, 625)]
    assert CL.window_rows(24, 1) == 8 and CL.window_rows(16, 512) == 16 and CL.window_rows(32, 1) == 8


def test_plain_ending_reaches_its_carries():
    ev = set()
    for m in CL.MODULI:
        for dim in CL.PLAIN_DIMS:            # the patterns of 1023 columns repeat every 11: 23 columns hold them all, on both parities
            calls = [CL.crafted_jobs(CL.PLAIN_JOBS, rows, min(dim, 23), m, CL.first_for(m)) for rows in CL.PLAIN_ROWS]
            _split_form(calls, lambda rows: CL.combine_split(rows, dim, CL.PLAIN_JOBS), m, ev)
    _require(ev, COMMON + RMW + (CL.HIGH_GE_M,), "plain ending")
    assert not ev & set(ATOMIC)              # one split per call: the atomic ending never runs


@pytest.mark.parametrize("order", [0, 1, 2], ids=["ascending", "descending", "shuffled"])
def test_atomic_ending_reaches_its_special_cases(order):
    ev = set()
    for jobs, dim, rows in CL.ATOMIC_CASES:
        per_case = set()
        for m in (CL.MODULI if jobs == 3 else (CL.PMAX, 433)):
            calls = [CL.crafted_jobs(min(jobs, CL.NPAT), rows, min(dim, 23), m, CL.first_for(m))]
            _split_form(calls, lambda r: CL.combine_split(r, dim, jobs), m, per_case, order)
        _require(per_case, COMMON + ATOMIC + (CL.HIGH_GE_M,), f"atomic ending, {rows} rows, {jobs} jobs")
        ev |= per_case
    assert not ev & set(RMW)


def test_walk_kernel_reaches_its_special_cases():
    ev = set()
    m, B, n = CL.P62, 6, 242
    calls = [CL.crafted_jobs(CL.NPAT, rows, B, m, 0) for rows in CL.WALK_PREV + (40,)]     # jobs 11 .. 241 repeat jobs 0 .. 10
    for order in range(3):
        _split_form(calls, lambda r: CL.combine_split(r, B, n), m, ev, order)
    _require(ev, COMMON + ATOMIC, "side-stream walk kernel")


@pytest.mark.parametrize("m", [CL.PMAX, CL.P62, CL.P31MAX], ids=["l31", "mfma + additive", "n31"])
def test_dual_role_clerk_items_reach_their_special_cases(m):
    ev = set()
    calls = [CL.crafted_jobs(3, rows, 48, m, 0) for rows in CL.DUAL_PREV + (40,)]          # every clerk (3, 8 or 26) holds these patterns
    for order in range(3):
        _split_form(calls, CL.fuse_split, m, ev, order)
    _require(ev, COMMON + RMW + ATOMIC, "dual-role clerk items")


@pytest.mark.parametrize("B", [48, 49])
def test_narrow_limb_gemm_forms_reach_their_carries(B):
    m = CL.NGEMM_PMAX
    calls = [CL.crafted_jobs(3, rows, B, m, 0) for rows in CL.NGEMM_PREV]
    # clerk waves + follow-up kernel: per call one read-modify-write of the whole tile, or two (the waves flush the rows they got to,
    # ngemm_clerk_rest_kernel resumes from the recorded row - here after the first quantum of ten)
    for cut in (None, 10):
        ev = set()
        for j, c, cols in _columns(calls):
            cell = [0, 0]
            for col in cols:
                for part in ([col] if cut is None or len(col) <= cut else [col[:cut], col[cut:]]):
                    CL.rmw_add(cell, *CL.acc_range(part, ev), ev)
            CL.finish(cell, m, sum(int(x) for col in cols for x in col.tolist()), ev)
        _require(ev, COMMON + RMW, "limb GEMM clerk waves / follow-up kernel")
    # clerk workgroup items (odd B, the knob) and the clerk-only calls' combine_update_kernel
    # (clerk-only: the one-split call is the first, on sums that are still zero - its read-modify-write has nothing to carry)
    for splits_of, form, names in ((CL.fuse_split, "limb GEMM clerk workgroups", COMMON + RMW + ATOMIC),
                                   (lambda r: CL.combine_split(r, B, 50), "clerk-only calls", COMMON + ATOMIC)):
        ev = set()
        for order in range(3):
            _split_form(calls, splits_of, m, ev, order)
        _require(ev, names, form)


def _window_form(mat, W, m, ev, direct_columns=()):
    jobs, rows, L = mat.shape
    for j in range(jobs):
        for c in range(L):
            cell = [0, 0]
            col = mat[j, :, c]
            CL.window_sum(cell, col, W, ev, direct=set(range(0, rows, 2)) if c in direct_columns else ())
            CL.finish(cell, m, sum(int(x) for x in col.tolist()), ev)


def test_wire_fed_sums_reach_the_window_cases():
    ev = set()
    for name, jobs, rpj, L in CL.WIRE_CASES:
        W = CL.window_rows(rpj, jobs)
        per_case = set()
        for m in CL.MODULI:
            _window_form(CL.crafted_jobs(min(jobs, CL.NPAT), rpj, min(L, 23), m, CL.first_for(m)), W, m, per_case)
        _require(per_case, (CL.CELL_8 if W == 8 else CL.CELL_16, CL.FOLD_CARRY, CL.LOW_ZERO, CL.ZERO_ZERO, CL.NEG_MULTIPLE, CL.HIGH_GE_M), f"wire-fed sums, {name}")
        ev |= per_case
    _require(ev, (CL.CELL_8, CL.CELL_16, CL.FOLD_CARRY, CL.CANCEL, CL.ATOMIC_CARRY, CL.LOW_ZERO, CL.ZERO_ZERO, CL.NEG_MULTIPLE, CL.HIGH_GE_M), "wire-fed sums")


@pytest.mark.parametrize("long_value", [CL.MIN, CL.MAX], ids=["MIN", "MAX"])
def test_drift_rows_leave_the_window(long_value):
    direct = CL.drift_direct()
    assert min(direct) == 2048 and max(direct) == CL.DRIFT_L - 1 and len(direct) == CL.DRIFT_L - 2048
    mat = CL.drift_matrix(long_value)
    ev = set()
    cols = (0, 2047, 2048, CL.DRIFT_L - 1)                        # the columns are all alike on either side of the window's edge
    _window_form(mat[None][:, :, cols], 8, 2, ev, direct_columns={i for i, c in enumerate(cols) if c in direct})
    _require(ev, (CL.DIRECT, CL.CANCEL, CL.ATOMIC_CARRY, CL.CELL_8, CL.HIGH_GE_M), "wire-fed sums beyond the window")


@pytest.mark.parametrize("W", [8, 16])
def test_sealed_sums_reach_the_window_cases(W):
    ev = set()
    for m in (CL.PMAX, 433):
        _window_form(CL.crafted_matrix(24, 23, m, CL.first_for(m))[None], W, m, ev)
    _require(ev, (CL.CELL_8, CL.FOLD_CARRY, CL.LOW_ZERO, CL.ZERO_ZERO, CL.CANCEL, CL.NEG_MULTIPLE) + ((CL.CELL_16,) if W == 16 else ()),
             f"sealed sums, {W} rows per workgroup")


def test_modsum_parts_reaches_its_carries():
    ev = set()
    for m in (433, CL.PMAX):
        mat = CL.crafted_matrix(64, 23, m, CL.first_for(m))
        for c in range(mat.shape[1]):
            lo, hi = CL.acc_range(mat[:, c], ev)
            CL.finish([lo, hi], m, sum(int(x) for x in mat[:, c].tolist()), ev)
    _require(ev, COMMON, "modsum_parts_kernel")

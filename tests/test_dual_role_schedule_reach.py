"""Reach checks for tests/test_dual_role_schedule_gpu.py (CPU): the model of tests/dual_role_schedule.py - fuse_plan, fuse_role,
fuse_combine and split_item restated in Python integers - is walked over every block index of every grid.

  * The schedule is a bijection: for every 0 <= n_gen, n_comb < 200, and for every call of the case table, every clerk item and
    every share-gen chunk runs exactly once, every (job, column pair, row) of the previous tile is summed exactly once and nothing
    beside it.
  * The table reaches every named class of the schedule space (each period class in two families), and under each planted fault
    some case of the table shows an item or chunk that did not run once or a cell that was not summed once - so the GPU test, which
    runs the same table, cannot pass on a library with that slip.  Both tables (class -> first case, fault -> first case that
    notices it) are printed (pytest -s) and asserted to have no empty row.
  * What the table does not reach is dual_role_schedule.REACH.
The comparison of the model's plan with the plan the library made needs a launch: it is in the GPU file."""
import ctypes as C
import threading

import numpy as np
import pytest

import dual_role_schedule as S

IDS = [c.name for c in S.CASES]


def test_the_rules_restated():
    """the shapes the table is built from, by hand: l31 (3, 1, 8) with B = 520 has two chunks and two column blocks, 9 previous rows
    make 16 clerk items, and the participant counts walk the period classes"""
    ladder = {7: S.P1, 8: S.P23_IDLE, 15: S.P23_FULL, 16: S.P3, 24: S.P43, 32: S.P5, 40: S.P65, 48: S.P7}
    for P, name in ladder.items():
        pl = S.plan("l31", 3, 8, 3 * 520 - 1, P, 9)
        assert pl[:6] == (2, 2, 1, 9, 2 * P, 16), pl
        assert name in S.classes("l31", 3, 8, 3 * 520 - 1, P, 9), (P, name)
    assert S.plan("l31", 3, 8, 3 * 520 - 1, 8, 9)[6:10] == (2, 3, 46, 14)            # raw period, period, grid, idle positions
    assert S.plan("l31", 3, 8, 3 * 520 - 1, 15, 9)[6:10] == (2, 3, 46, 0)
    assert S.plan("l31", 3, 8, 3 * 520 - 1, 48, 9)[6:10] == (7, 7, 112, 0)
    assert [S.plan("additive", 1, 3, 2, 2, r)[2:4] for r in (513, 1025, 32769)] == [(2, 257), (3, 342), (64, 513)]
    for fam, k in (("l31", 8), ("n31", 8)):
        pl = S.plan(fam, k, 26, 8 * 520 - 1, 130, 26)
        assert (pl.n_gen, pl.n_comb, pl.raw_period, pl.period) == (260, 52, 6, 5)
    assert S.gen_chunks("mfma", 12, 12 * 520 - 1) == 2 and S.gen_chunks("mfma", 9, 9 * 40) == 1 and S.gen_chunks("additive", 1, 520) == 2
    assert S.hook_fields(S.plan("l31", 3, 8, 3 * 520 - 1, 8, 9)) == (1, 16, 16, 3, 46, 1, 9, 2)
    assert set(S.EQUIVALENT) <= set(S.FAULTS) and len(set(S.CLASSES)) == len(S.CLASSES) == 30


def test_schedule_is_a_bijection_for_every_pair_of_counts_below_200():
    """n_gen share-gen chunks beside n_comb clerk items, every pair (one chunk per participant, one item per job): the role map
    sends the grid's positions onto every item once, every chunk once and the idle surplus, whatever the period"""
    for n_comb in range(200):
        for n_gen in range(200):
            pl = S.plan("additive", 1, n_comb, 2, n_gen, 1)
            assert (pl.n_gen, pl.n_comb) == (n_gen, n_comb) and pl.period % 2 == 1
            clerk, idx, idle = S.roles(np.arange(pl.grid, dtype=np.int64), pl)
            assert np.array_equal(idx[clerk], np.arange(n_comb)), (n_gen, n_comb)
            assert np.array_equal(idx[~clerk & ~idle], np.arange(n_gen)), (n_gen, n_comb)          # ascending: each exactly once
            assert int(idle.sum()) == pl.idle == pl.grid - n_gen - n_comb
    # ... and through the whole of check(), items and chunks by name, on a coarser net
    for n_comb in range(0, 200, 7):
        for n_gen in range(0, 200, 3):
            assert S.check("additive", 1, n_comb, 2, n_gen, 1) == [], (n_gen, n_comb)


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_every_call_of_the_table_is_a_bijection(case):
    assert S.findings(case) == []
    assert len(S.calls_of(case)) >= 1 and case.Bs >= case.B and case.family in S.FAMILIES


def test_pipelines_hold_a_short_tile_the_tile_after_it_and_both_end_calls():
    for case in S.CASES:
        if case.kind != "pipeline":
            continue
        calls = S.calls_of(case)
        assert calls[0][1] == 0 and calls[-1][0] == 0, case.name
        assert {S.FIRST, S.DRAIN, "prev rows < participants"} <= S.coverage(case), case.name
    assert sum("prev rows > participants" in S.coverage(c) for c in S.CASES if c.kind == "pipeline") >= 4


def test_the_table_reaches_every_class():
    first, families = {}, {}
    for case in S.CASES:
        for name in S.coverage(case):
            assert name in S.CLASSES, name
            first.setdefault(name, case.name)
            families.setdefault(name, set()).add(case.family)
    print("\nclass -> first case that reaches it")
    for name in S.CLASSES:
        print(f"  {name:48s} {first.get(name, '-')}   [{', '.join(sorted(families.get(name, ())))}]")
    missing = [name for name in S.CLASSES if name not in first]
    assert not missing, f"no case reaches: {missing}"
    thin = [name for name in S.PERIOD_CLASSES if len(families[name]) < 2]
    assert not thin, f"period classes reached by fewer than two families: {thin}"
    # the crafted rows carry the split classes: a row summed twice or skipped there changes the sum whatever its value
    for name in S.SPLIT_CLASSES:
        assert any(name in S.coverage(c) for c in S.CASES if c.kind == "crafted prev"), name
    # every fused kernel instance of the table is there in a case that is not a fallback
    assert {c.kernel for c in S.CASES if c.layout is None} == {c.kernel for c in S.CASES} and len({c.kernel for c in S.CASES}) == 9


def test_every_planted_fault_is_noticed_by_some_case():
    noticed = {}
    for fault in S.FAULTS:
        if fault in S.EQUIVALENT:
            continue
        for case in S.CASES:
            bad = S.findings(case, fault)
            if bad:
                noticed[fault] = (case.name, bad[0])
                break
    print("\nfault -> first case that notices it")
    for fault in S.FAULTS:
        print(f"  {fault:76s} " + (" :: ".join(noticed[fault]) if fault in noticed else "changes no plan: " + S.EQUIVALENT.get(fault, "-")))
    unnoticed = [f for f in S.FAULTS if f not in noticed and f not in S.EQUIVALENT]
    assert not unnoticed, f"no case notices: {unnoticed} - add a case"


def test_a_fault_listed_as_equivalent_changes_no_plan():
    """the recomputation of `splits` gives back what it started from for every row count (dual_role_schedule.EQUIVALENT): no
    case can notice its loss.  If the 512-row items or the cap of 64 ever change so that it matters, this fails and a case is due"""
    assert list(S.EQUIVALENT) == [S.F_SPLITS_STALE]
    for prev in list(range(1, 1 << 17)) + [1 << 20, (1 << 20) + 1, (1 << 31) - 1, 1 << 31, (1 << 40) + 12345]:
        assert S.plan("additive", 1, 3, 2, 2, prev, S.F_SPLITS_STALE) == S.plan("additive", 1, 3, 2, 2, prev), prev


def test_what_the_table_does_not_reach():
    assert len(S.REACH) == 2
    for case in S.CASES:
        assert case.n <= 65535
        for pl in S.plans_of(case):
            assert 0 < pl.grid <= 1024 < S.MAX_BLOCKS, (case.name, pl.grid)       # a few hundred workgroups, never near the size refusal
    # ... and the tiles stay small: the largest buffer of a case (clerk stride = the most rows of any call + 1)
    for case in S.CASES:
        rows = max(max(P, prev) for P, prev in S.calls_of(case)) + 1
        assert case.n * rows * case.Bs * 8 <= 24 << 20, case.name


def test_the_hook_answers_a_state_error_before_the_first_plan(built):
    """sda_debug_last_fuse_plan is host-only and exists in the test library alone: on a thread that has planned nothing it says so"""
    from sda_amd import capi
    lib = capi.hooks_library()
    got = []

    def ask():
        out = (C.c_ulonglong * 8)()
        got.append((lib.sda_debug_last_fuse_plan(C.byref(out)), lib.sda_debug_last_fuse_plan(None)))
    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert got == [(capi.ERR_STATE, capi.ERR_INVALID_ARGUMENT)]

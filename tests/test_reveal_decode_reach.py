"""What tests/reveal_decode_cases.py contains, proven on the CPU: its Peterson-Gorenstein-Zierler model IS the definition (it
equals brute force over all subsets on every 8-row case), planted faults within the cap come back as exactly the planted positions
with the other rows' reconstruction and the true secrets as output, the guaranteed band e + 1 .. c - e is undecoded in every batch,
nu = 1 is reveal_check_cases' locate rule, the table reaches every nu, the S_0 = 0 branch, a Berlekamp-Massey length change at the
last syndrome and a mixed wave, and every one of eight faults planted in the model is noticed by a case of the table."""
import numpy as np
import pytest

import reveal_check_cases as vc
import reveal_decode_cases as dc

EIGHT_ROWS = [c.name for c in dc.CASES if len(c.indices) == 8]


@pytest.fixture(scope="module")
def finishes(built):
    """every case's model finish under SDA_CHECK_CORRECT, computed once"""
    return {c.name: dc.model_finish(c, dc.build(c.name).rows, dc.CORRECT) for c in dc.CASES}


def _syndromes(case, rows, b):
    T = dc.tables(case)
    sh = [int(rows[i][b]) % T.p for i in range(len(case.indices))]
    return [sum(T.H[d][i] * sh[i] for i in range(len(sh))) % T.p for d in range(case.checks)]


@pytest.mark.parametrize("name", EIGHT_ROWS)
def test_the_model_is_the_definition(built, finishes, name):
    case, b = dc.BY_NAME[name], dc.build(name)
    T = dc.tables(case)
    seen = set()
    for batch in range(b.batches):
        S = _syndromes(case, b.rows, batch)
        found = dc.brute_force(S, T.x, dc.cap_of(case), T.p)
        assert len(found) <= 1, "the definition is not unique"
        got = finishes[name].errors[batch]
        assert (found[0] if found else None) == got, (batch, found, got)
        seen.add(finishes[name].verdicts[batch])
    print(name, "verdicts", sorted(seen))


@pytest.mark.parametrize("name", [c.name for c in dc.CASES])
def test_planted_faults_come_back_as_the_guarantees_say(built, finishes, name):
    case, b = dc.BY_NAME[name], dc.build(name)
    want = dc.expected_verdicts(case, b)
    fin = finishes[name]
    if want is None:
        return                                                            # crafted rows: the model alone says what comes out
    e = dc.cap_of(case)
    for batch, (w, got) in enumerate(zip(want, fin.verdicts)):
        if w is not None:
            assert got == w, (batch, b.faulty[batch], got)
        if w is not None and w > 0:
            assert tuple(i for i, _ in fin.errors[batch]) == b.faulty[batch]
    if all(len(f) <= e for f in b.faulty):
        assert np.array_equal(fin.out, b.want), "corrected output is not the true secrets"
        assert fin.report[1] == fin.report[2] == fin.report[0] and fin.report[4] == dc.NONE64
        if len(set(b.faulty)) == 1:                                       # the same faulty rows in every batch
            keep = [i for i in range(len(case.indices)) if i not in b.faulty[0]]
            assert np.array_equal(fin.out, vc.unchecked_python(case, b.rows, keep=keep))
    rep = dc.model_finish(case, b.rows, dc.REPORT)
    assert np.array_equal(rep.out, vc.unchecked_python(case, b.rows)), "SDA_CHECK_REPORT changes the output"
    assert rep.report[2] == 0 and rep.report[:2] == fin.report[:2] and rep.report[3:] == fin.report[3:]


def test_one_position_is_the_checked_finish(built, finishes):
    """nu = 1: verdict, position and output equal reveal_check_cases.model_finish on the same rows"""
    n = 0
    for case in dc.CASES:
        if dc.cap_of(case) != 1:
            continue
        b = dc.build(case.name)
        old = vc.model_finish(case, b.rows, vc.CORRECT)
        new = finishes[case.name]
        assert [v == 1 for v in new.verdicts] == [v == "located" for v in old.verdicts], case.name
        assert [v == 0 for v in new.verdicts] == [v == "clean" for v in old.verdicts], case.name
        assert new.report[:4] == old.report[:4] and new.report[dc.HEAD:] == old.report[4:], case.name
        assert np.array_equal(new.out, old.out), case.name
        n += 1
    assert n >= 10


def _bm_changes(S, p):
    """the steps at which Berlekamp-Massey's length changes (plain textbook form, used only to measure what the table reaches)"""
    C, B, L, m, bb, changes = [1], [1], 0, 1, 1, []
    for n in range(len(S)):
        d = sum(C[i] * S[n - i] for i in range(min(L, len(C) - 1) + 1)) % p
        if d == 0:
            m += 1
            continue
        T = list(C)
        coef = d * pow(bb, -1, p) % p
        C = C + [0] * (len(B) + m - len(C))
        for i, v in enumerate(B):
            C[i + m] = (C[i + m] - coef * v) % p
        if 2 * L <= n:
            L, B, bb, m = n + 1 - L, T, d, 1
            changes.append(n)
        else:
            m += 1
    return changes


def test_the_table_reaches_every_branch(built, finishes):
    nus, s0_zero, last_change, mixed_wave = set(), False, False, False
    for case in dc.CASES:
        fin, b = finishes[case.name], dc.build(case.name)
        nus.update(fin.verdicts)
        for w in range(0, len(fin.verdicts), 64):
            if len({v for v in fin.verdicts[w:w + 64] if v > 0}) >= 3 and -1 in fin.verdicts[w:w + 64] and 0 in fin.verdicts[w:w + 64]:
                mixed_wave = True
        if case.fault == "s0zero":
            for batch in range(min(b.batches, 4)):
                S = _syndromes(case, b.rows, batch)
                assert S[0] == 0 and any(S)
                s0_zero = s0_zero or fin.verdicts[batch] == 2
        if case.checks % 2 and isinstance(case.fault, tuple) and case.fault[1] == case.checks // 2 + 1:
            S = _syndromes(case, b.rows, 0)
            last_change = last_change or _bm_changes(S, dc.tables(case).p)[-1] == case.checks - 1
    assert nus >= set(range(0, 9)) | {-1}, nus
    assert s0_zero, "no decoded batch with S_0 = 0"
    assert last_change, "no batch whose Berlekamp-Massey length changes at the last syndrome"
    assert mixed_wave, "no wave with three different nu, a clean and an undecoded lane side by side"
    assert any(c.cap for c in dc.CASES) and any(c.values == "crafted" for c in dc.CASES)
    low = dc.BY_NAME["k8_62-c16-d805-rows2-cap1"]
    assert set(finishes[low.name].verdicts) == {-1}, "two faulty rows at max_errors = 1 must be refused"
    shapes = {(c.scheme, len(c.indices), c.checks, c.dim) for c in dc.CASES}
    for want in (("k3_62", 8, 4, 1), ("k3_62", 8, 3, 4), ("k3_62", 8, 4, 1000), ("k8_62", 26, 16, 805), ("k8_62", 26, 9, 805),
                 ("k8_62", 26, 8, 805), ("k8_62", 12, 2, 805), ("pss155", 260, 5, 1), ("pss155", 260, 4, 250)):
        assert want in shapes, want
    assert {dc.coef_path(c) for c in dc.CASES} == {"lds", "global"}


@pytest.mark.parametrize("plant", dc.PLANTS)
def test_a_planted_fault_is_noticed(built, finishes, plant):
    """each fault planted in the model changes the output or the report of some case; the first such case is named"""
    for case in dc.CASES:
        if plant == "odd_ceil" and (len(case.indices) > 8 or case.checks % 2 == 0 or case.dim > 4):
            continue
        if len(case.indices) > 26 or case.dim > 1000:
            continue
        b = dc.build(case.name)
        right, wrong = finishes[case.name], dc.model_finish(case, b.rows, dc.CORRECT, plant=plant)
        if wrong.report != right.report or not np.array_equal(wrong.out, right.out):
            what = "report" if wrong.report != right.report else "output"
            print(f"planted {plant}: first noticed by {case.name} ({what})")
            return
    pytest.fail(f"planted fault {plant} is noticed by no case")

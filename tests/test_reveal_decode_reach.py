"""What tests/reveal_decode_cases.py contains, proven on the CPU: its Peterson-Gorenstein-Zierler model IS the definition (it
equals brute force over all subsets on every 8-row case), planted faults within the cap come back as exactly the planted positions
with the other rows' reconstruction and the true secrets as output, the guaranteed band e + 1 .. c - e is undecoded in every batch,
nu = 1 is reveal_check_cases' locate rule, the table reaches every nu, the S_0 = 0 branch, a Berlekamp-Massey length change at the
last syndrome and a mixed wave, and every one of eight faults planted in the model is noticed by a case of the table.  The wide
committee's cases blame positions past a byte, every steered family comes back as its construction says, and three more planted
faults say what only those cases notice."""
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
    wide = [c for c in dc.CASES if c.scheme == "k3_wide"]
    assert {dc.coef_path(c) for c in wide} == {"lds", "global"} and {(len(c.indices), c.checks) for c in wide} == {(300, 16), (300, 13), (257, 4)}
    assert {c.dim for c in wide} == {1, 769} and any(c.feed == "descending" for c in wide)
    assert {c.fault[1] for c in wide if isinstance(c.fault, tuple) and c.checks == 16 and c.dim == 769} == set(range(1, 11))
    assert {c.fault for c in wide if isinstance(c.fault, str)} >= {"stair", "first", "last", "s0zero", "steered"}
    assert {c.values for c in wide} == {"sums", "crafted", "congruent"}


def test_wide_cases_blame_positions_past_a_byte(built, finishes):
    """from Built.faulty: at least two wide cases are decoded with a position >= 256, one with the last row of 300 and one with the
    last row of 257 - and the model blames exactly those words"""
    high, last = [], set()
    for name in dc.NEW:
        case, b, fin = dc.BY_NAME[name], dc.build(name), finishes[name]
        if case.scheme != "k3_wide" or not isinstance(case.fault, tuple) or case.fault[1] > dc.cap_of(case):
            continue
        at = b.faulty[0]
        assert set(case.pin or ()) <= set(at) or len(case.pin) > len(at)
        assert fin.report[dc.HEAD:] == [b.batches if i in at else 0 for i in range(len(case.indices))], name
        if max(at) >= 256:
            high.append(name)
        if max(at) == len(case.indices) - 1:
            last.add(len(case.indices))
    print("decoded with a position >= 256:", high)
    assert len(high) >= 2 and last == {257, 300}
    stair = finishes["k3_wide-c16-d769-stair"]
    assert any(stair.report[dc.HEAD + 256:]) and any(stair.report[dc.HEAD:dc.HEAD + 64])


STEERED = [n for n in dc.NEW if dc.BY_NAME[n].fault == "steered"]


@pytest.mark.parametrize("name", STEERED)
def test_steered_families_have_their_verdicts(built, finishes, name):
    """the planted errors give the family's syndromes back exactly, and every batch comes back as its family's construction says;
    where the definition promises nothing the model was asked, and what it said is written down here"""
    case, b, fin = dc.BY_NAME[name], dc.build(name), finishes[name]
    T, e, n = dc.tables(case), dc.cap_of(case), case.checks
    fams = dc.families(n)
    asked = {"s0_forced_zero": -1, "cap_plus_one": -1, "cap_minus_one_and_z": -1}
    seen = {}
    for batch in range(b.batches):
        fam = fams[batch % len(fams)]
        S = _syndromes(case, b.rows, batch)
        if fam == "ratio_z":
            assert S[0] and all(S[d + 1] * S[0] % T.p == S[1] * S[d] % T.p for d in range(n - 1)) and S[1] * pow(S[0], -1, T.p) % T.p not in T.x + [0, 1]
        elif fam in ("ratio_one", "all_pm1"):
            assert len(set(S)) == 1 and S[0] and (fam == "ratio_one" or S[0] == T.p - 1)
        elif fam == "ratio_zero":
            assert S[0] and not any(S[1:])
        elif fam == "late_jump":
            assert S[-1] and not any(S[:-1])
        elif fam == "zero_half":
            assert not any(S[:n // 2]) and all(S[n // 2:])
        elif fam in ("two_points_cancel", "s0_zero_two_points", "s0_forced_zero", "double_root"):
            assert S[0] == 0 and any(S)
        want = dc.family_verdict(fam, n, e, case.pin)
        got = fin.verdicts[batch]
        if want is None:
            assert got == asked[fam], (batch, fam, got)
        else:
            assert got == want[0], (batch, fam, got, want)
            if got > 0:
                assert tuple(i for i, _ in fin.errors[batch]) == want[1] == b.faulty[batch], (batch, fam)
        seen.setdefault(fam, got)
    assert set(seen) == set(fams) and b.batches >= 4 * len(fams)                   # every family, in every wave
    print(name, seen)
    if name == "k3_62-c4-d769-steered":                                            # the eleven first families on the 8-row shape
        assert [seen[f] for f in dc.FAMILIES[:8]] == [-1] * 8
        assert [fin.errors[8 + j] and [i for i, _ in fin.errors[8 + j]] for j in range(3)] == [[7], [0, 7], [3, 5]]
    if case.cap:
        assert seen["three_points"] == -1 and seen["cap_points"] == case.cap
    elif n >= 8:
        assert seen["three_points"] == 3 and seen["cap_points"] == n // 2


def _decodes(case, plant):
    """per batch, what the model's decoder says under `plant` - all a fault of GAP_PLANTS' root search can change"""
    b = dc.build(case.name)
    return [dc._decoded(tuple(S), case.scheme, case.indices, case.checks, dc.cap_of(case), plant) if any(S) else None
            for S in (_syndromes(case, b.rows, batch) for batch in range(b.batches))]


@pytest.mark.parametrize("plant", dc.GAP_PLANTS)
def test_what_only_the_new_cases_notice(built, finishes, plant):
    """position_mod_256 is noticed by wide cases and by no older case (up to 256 rows a position is its own low byte; the older
    260-row cases are asked).  A root search that also tries the node 1, or 0, is noticed by steered cases; whether an older case
    notices is found out and printed, batch by batch of the whole older table."""
    old, new = [], []
    for case in dc.CASES:
        if plant == "position_mod_256":
            if len(case.indices) <= 256:
                continue
            b = dc.build(case.name)
            wrong = dc.model_finish(case, b.rows, dc.CORRECT, plant=plant)
            hit = wrong.report != finishes[case.name].report or not np.array_equal(wrong.out, finishes[case.name].out)
        else:
            if case.name in dc.NEW and case.fault != "steered":
                continue
            hit = _decodes(case, plant) != _decodes(case, None)
        if hit:
            (new if case.name in dc.NEW else old).append(case.name)
    print(f"planted {plant}: noticed by {len(new)} new cases {new[:6]} and by {len(old)} older cases {old[:6]}")
    assert new, plant
    if plant == "position_mod_256":
        assert not old
    else:
        assert not old, "an older case notices after all: say so in the table's comment"


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


# ---- the store the plain finishes share: what the guard cases are there for ---------------------------------------------------------
@pytest.mark.parametrize("plant", vc.STORE_PLANTS)
def test_the_guard_cases_notice_a_planted_store_fault(plant):
    """the GPU runners check the output against the model and the words behind it against the sentinel - together the buffer of
    vc.framed(): a store that drops the last element of a partial
    group, or stores an all-padding second group, leaves other words there at every dimension the guard cases were chosen for"""
    assert [dc.BY_NAME[n].dim for n in dc.GUARD] == list(vc.GUARD_DIMS) and all(dc.BY_NAME[n].scheme == "k8_62" for n in dc.GUARD)
    hit = []
    for name in dc.GUARD:
        case, rows = dc.BY_NAME[name], dc.build(name).rows
        fin = dc.model_finish(case, rows, vc.CORRECT)
        assert fin.report[1] == fin.report[2] == vc.batches(case), "every batch of a guard case is corrected"
        clean = vc.framed(dc.model_finish, case, rows, vc.CORRECT)
        assert clean[case.dim:] == [vc.SENTINEL] * vc.TAIL and vc.SENTINEL not in clean[:case.dim]
        if vc.framed(dc.model_finish, case, rows, vc.CORRECT, plant) != clean:
            hit.append(case.dim % 8)
    assert sorted(hit) == ([1, 1, 2, 3, 6, 7] if plant == "last_element_dropped" else [1, 1, 2, 3, 4])

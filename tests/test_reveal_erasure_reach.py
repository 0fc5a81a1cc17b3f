"""What tests/reveal_erasure_cases.py contains, proven on the CPU: its Gaussian-elimination model IS the definition (it equals brute
force over all error subsets, with F fixed, on every 8-row case), with F empty it is reveal_decode_cases' model on that module's
whole table, corrected output within the guarantees is the C oracle's reconstruct of the surviving rows, an erased row's content
does not matter, the table reaches every (f, nu) class by name, and every one of eight faults planted in the model is noticed by a
case of the table.  The wide committee's cases reach the setup kernel's second step, every wave of a step and the positions it counts
and does not keep; every steered family comes back as its construction says; four more planted faults say what only those cases
notice."""
import numpy as np
import pytest

import reveal_check_cases as vc
import reveal_decode_cases as dc
import reveal_erasure_cases as ec

EIGHT_ROWS = [c.name for c in ec.CASES if len(c.indices) == 8]


@pytest.fixture(scope="module")
def finishes(built):
    """every case's model finish under SDA_CHECK_CORRECT, computed once"""
    return {c.name: ec.model_finish(c, ec.build(c.name).rows, ec.CORRECT) for c in ec.CASES}


def _syndromes(case, rows, b):
    T = ec.tables(case)
    sh = [int(rows[i][b]) % T.p for i in range(len(case.indices))]
    return [sum(T.H[d][i] * sh[i] for i in range(len(sh))) % T.p for d in range(case.checks)]


@pytest.mark.parametrize("name", EIGHT_ROWS)
def test_the_model_is_the_definition(built, finishes, name):
    case, b = ec.BY_NAME[name], ec.build(name)
    F = list(case.erased) if case.ok == "flags" else []
    if len(F) > case.checks:
        assert set(finishes[name].verdicts) == {"clean"} and finishes[name].report[:8] == [0, 0, 0, ec.NONE64, ec.NONE64, 0, len(F), 1]
        return
    T = ec.tables(case)
    step = max(1, b.batches // 40)                                        # every batch of the small cases, forty of the others
    for batch in list(range(0, b.batches, step)) + [b.batches - 1]:
        S = _syndromes(case, b.rows, batch)
        found = ec.brute_force(S, T.x, F, ec.cap_of(case), T.p)
        assert len(found) <= 1, "the definition is not unique"
        verdict = finishes[name].verdicts[batch]
        if verdict == -1:
            assert not found, (batch, found)
        else:
            assert found, (batch, verdict)
            E, YF = found[0]
            assert E == sorted(finishes[name].errors[batch]) and YF == finishes[name].erasures[batch], batch
            assert verdict == (len(E) if E else "consistent" if any(S) else "clean")


@pytest.mark.parametrize("name", [c.name for c in dc.CASES if len(c.indices) <= 26 and c.checks >= 2])
def test_without_erasures_it_is_the_decoding_model(built, name):
    old_case, b = dc.BY_NAME[name], dc.build(name)
    case = ec.Case("as-decode/" + name, old_case.scheme, old_case.dim, old_case.indices, old_case.checks, old_case.cap, (), 0, "zero", "null")
    for policy in (ec.REPORT, ec.CORRECT):
        old, new = dc.model_finish(old_case, b.rows, policy), ec.model_finish(case, b.rows, policy)
        assert new.report == old.report and np.array_equal(new.out, old.out), policy


@pytest.mark.parametrize("name", [c.name for c in ec.CASES])
def test_within_the_guarantees_the_output_is_the_other_rows_reconstruction(built, finishes, name):
    """... by the C oracle (reveal_check_cases.unchecked_python is proven equal to it by test_reveal_check_reach)"""
    from oracle import coracle
    case, b = ec.BY_NAME[name], ec.build(name)
    fin, want = finishes[name], ec.expected_verdicts(case, b)
    for batch, (w, got) in enumerate(zip(want, fin.verdicts)):
        if w == "ok":
            assert got in ("clean", "consistent"), (batch, got)
        elif w is not None:
            assert got == w, (batch, b.faulty[batch], got)
        if isinstance(w, int) and w > 0:
            assert tuple(sorted(i for i, _ in fin.errors[batch])) == b.faulty[batch]
    e, f = ec.cap_of(case), len(case.erased)
    rep = ec.model_finish(case, b.rows, ec.REPORT)
    assert np.array_equal(rep.out, vc.unchecked_python(case, b.rows)), "SDA_CHECK_REPORT changes the output"
    assert rep.report[2] == 0 and rep.report[:2] == fin.report[:2] and rep.report[3:] == fin.report[3:]
    assert fin.report[6:8] == [f if case.ok == "flags" else 0, int(f > case.checks)]
    assert all(fin.report[ec.HEAD + j] == 0 for j in case.erased), "an erased position is blamed"
    if f <= case.checks and all(len(q) <= e for q in b.faulty):
        assert np.array_equal(fin.out, b.want), "corrected output is not the true secrets"
        assert fin.report[1] == fin.report[2] == fin.report[0] and fin.report[4] == ec.NONE64
        if len(set(b.faulty)) == 1:                                       # the same faulty rows in every batch
            keep = [i for i in range(len(case.indices)) if i not in b.faulty[0] and i not in case.erased]
            p, k, t, n, w2, w3 = ec.SCHEMES[case.scheme]
            others = coracle.packed_reconstruct(p, k, t, w2, w3, case.dim, [case.indices[i] for i in keep],
                                                np.stack([b.rows[i][:b.batches] for i in keep]))
            assert np.array_equal(fin.out, others), "corrected output is not the oracle's reconstruct of the surviving rows"
    elif f > case.checks:
        assert np.array_equal(fin.out, rep.out)


@pytest.mark.parametrize("name", [c.name for c in ec.CASES if c.erased and len(c.indices) == 8])
def test_what_an_erased_row_added_does_not_matter(built, finishes, name):
    """a row refused (zeros), fed with garbage or fed correctly: the same report, and under SDA_CHECK_CORRECT the same output
    wherever the batch is consistent or decoded"""
    case = ec.BY_NAME[name]
    if len(case.erased) > case.checks:
        return
    right = finishes[name]
    for fill in ("zero", "random"):
        other = ec.model_finish(case, ec.refilled(name, fill), ec.CORRECT)
        assert other.report == right.report, fill
        same = [v != -1 for v in right.verdicts for _ in range(ec.tables(case).k)][:case.dim]
        assert np.array_equal(other.out[same], right.out[same]), fill


def test_the_table_reaches_every_class(built, finishes):
    def classes(scheme, checks):
        got = set()
        for c in ec.CASES:
            if c.scheme == scheme and c.checks == checks and c.ok == "flags" and isinstance(c.errors, int):
                v = set(finishes[c.name].verdicts)
                got.add((len(c.erased), c.errors, "over" if len(c.erased) > checks else "undecoded" if v == {-1} else "repaired"))
        return got
    small = classes("k3_62", 4)
    for f, errors in ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (4, 0), (0, 1), (0, 2)):
        assert (f, errors, "repaired") in small, (f, errors)
    assert (1, 2, "undecoded") in small and (3, 1, "undecoded") in small and (5, 0, "over") in small
    big = classes("k8_62", 16)
    for f, errors in ((1, 7), (6, 5), (8, 4), (15, 0), (16, 0)):
        assert (f, errors, "repaired") in big, (f, errors)
    assert (15, 1, "undecoded") in big and (17, 0, "over") in big
    low = ec.BY_NAME["k8_62-c16-d805-f2-e2-zero-cap1"]
    assert set(finishes[low.name].verdicts) == {-1}, "max_errors = 1 with f = 2 and two errors must be refused"
    assert (1, 0, "repaired") in classes("k3_62", 1) and (1, 0, "repaired") in classes("k3_31", 1)
    assert set(finishes["k3_62-c1-d764-f0-e1-zero"].verdicts) == {-1}
    # one wave with a clean, an erasure-only, an erasure + errors and an undecoded lane
    for name in ("k3_62-c4-d769-f2-emixed-zero", "k3_62-c4-d769-f1-emixed-zero"):
        v = finishes[name].verdicts[:64]
        assert {"clean", "consistent", -1} <= set(v) and any(isinstance(q, int) and q > 0 for q in v), name
    # the aimed errors: the modified syndromes are one error's on an erased position, and nothing is decoded
    for aimed, at in ((ec.BY_NAME["k3_62-c4-d764-f2-eaimed-zero"], 2), (ec.BY_NAME["k3_wide-c16-d769-f2-eaimed-zero"], 256)):
        b, T = ec.build(aimed.name), ec.tables(aimed)
        S = _syndromes(aimed, b.rows, 0)
        Tm = ec.modified(S, ec.gamma_of([T.x[j] for j in aimed.erased], T.p), T.p)
        assert at in aimed.erased and Tm[0] and all(Tm[d + 1] == Tm[d] * T.x[at] % T.p for d in range(len(Tm) - 1))
        assert set(finishes[aimed.name].verdicts) == {-1}
    # an error planted on an erased position is absorbed, not counted
    spoiled = finishes["k3_62-c4-d764-f2-e1-spoiled"]
    assert spoiled.report[:3] == finishes["k3_62-c4-d764-f2-e1-zero"].report[:3] and spoiled.report[5] == 1
    assert {c.fill for c in ec.CASES} == {"zero", "random", "clean", "spoiled"} and {c.ok for c in ec.CASES} == {"flags", "ones", "null"}
    assert any(0 in c.erased for c in ec.CASES) and any(len(c.indices) - 1 in c.erased for c in ec.CASES)
    B = {ec.batches(c) for c in ec.CASES if c.scheme == "k3_62"}
    assert {1, 255, 256, 257} <= B and {c.dim % 3 for c in ec.CASES if c.scheme == "k3_62"} == {0, 1, 2}


def test_the_wide_cases_reach_the_setup_kernels_steps_and_waves(built, finishes):
    """what reveal_erasure_setup_kernel does per 256 positions and per wave of 64, read off the tables' erased sets"""
    wide = [c for c in ec.CASES if c.scheme == "k3_wide" and c.ok == "flags"]
    steps = lambda c: {j // ec.STEP for j in c.erased}
    waves = lambda c, step: {j % ec.STEP // 64 for j in c.erased if j // ec.STEP == step}
    assert any(steps(c) == {0, 1} for c in wide) and any(steps(c) == {1} for c in wide)                    # the count is carried; a step adds nothing
    assert any(waves(c, 0) == {0, 1, 2, 3} for c in wide), "no case with erased positions in all four waves of a step"
    assert any(len(c.erased) <= ec.KEPT and max(c.erased) >= 256 and min(c.erased) < 256 for c in wide)    # a kept position >= 256 behind earlier ones
    assert any(len(c.erased) == ec.KEPT and min(c.erased) >= 256 for c in wide)                            # all sixteen slots from the second step
    over = [c for c in wide if len(c.erased) > ec.KEPT]
    assert {len(c.erased) for c in over} == {17, 200}
    seventeen = next(c for c in over if len(c.erased) == 17)
    assert sorted(seventeen.erased)[15] < 256 <= sorted(seventeen.erased)[16]                              # counted, not kept
    for c in over:
        assert finishes[c.name].report[:8] == [0, 0, 0, ec.NONE64, ec.NONE64, 0, len(c.erased), 1] and set(finishes[c.name].verdicts) == {"clean"}
    assert {len(c.indices) for c in ec.CASES if c.scheme == "k3_wide"} == {64, 65, 256, 257, 300}          # a wave, + 1, a step, + 1, > kThreads
    assert {vc.coef_path(c) for c in wide} == {"lds", "global"} and {c.dim for c in wide} == {1, 769}
    assert {c.fill for c in wide} >= {"zero", "random", "spoiled"} and any(c.cap for c in wide)
    assert {c.ok for c in ec.CASES if c.scheme == "k3_wide"} == {"flags", "ones", "null"}
    import extremes
    p, k, t, n, w2, w3 = ec.SCHEMES["k3_wide"]
    assert (w2, w3) == extremes.omegas(p, k, t, n)
    # errors past a byte: at least two wide cases are decoded with a position >= 256, one with the last row
    high, last = [], []
    for c in ec.CASES:
        b = ec.build(c.name)
        if c.scheme != "k3_wide" or not isinstance(c.errors, int) or not 0 < c.errors <= ec.cap_of(c) or len(c.erased) > c.checks:
            continue
        at = b.faulty[0]
        assert finishes[c.name].report[ec.HEAD:] == [b.batches if i in at else 0 for i in range(len(c.indices))], c.name
        high += [c.name] if max(at) >= 256 else []
        last += [c.name] if max(at) == len(c.indices) - 1 else []
    print("decoded with a position >= 256:", high, "with the last row:", last)
    assert len(high) >= 2 and last


@pytest.mark.parametrize("name", [n for n in ec.NEW if ec.BY_NAME[n].errors == "steered"])
def test_steered_families_have_their_verdicts(built, finishes, name):
    """the planted errors give the family's MODIFIED syndromes back exactly - whatever the erased rows hold - and every batch comes
    back as its family's construction says; where the definition promises nothing the model was asked"""
    case, b, fin = ec.BY_NAME[name], ec.build(name), finishes[name]
    T, e, n = ec.tables(case), ec.cap_of(case), case.checks - len(case.erased)
    fams = dc.families(n)
    g = ec.gamma_of([T.x[j] for j in case.erased], T.p)
    seen = {}
    for batch in range(b.batches):
        fam = fams[batch % len(fams)]
        Tm = ec.modified(_syndromes(case, b.rows, batch), g, T.p)
        assert len(Tm) == n and Tm == ec.modified(_syndromes(case, ec.refilled(name, "random"), batch), g, T.p)
        if fam == "ratio_one":
            assert len(set(Tm)) == 1 and Tm[0]
        elif fam == "all_pm1":
            assert Tm == [T.p - 1] * n
        elif fam == "late_jump":
            assert Tm[-1] and not any(Tm[:-1])
        elif fam == "ratio_zero":
            assert Tm[0] and not any(Tm[1:])
        want = dc.family_verdict(fam, n, e, case.pin)
        got = fin.verdicts[batch]
        if want is None:
            assert got == -1, (batch, fam, got)
        else:
            assert got == want[0], (batch, fam, got, want)
            if got != -1:
                assert tuple(sorted(i for i, _ in fin.errors[batch])) == want[1] == b.faulty[batch], (batch, fam)
        seen.setdefault(fam, got)
    assert set(seen) == set(fams) and b.batches >= 4 * len(fams)
    print(name, "n", n, "cap", e, seen)


@pytest.mark.parametrize("plant", ec.GAP_PLANTS)
def test_what_only_the_new_cases_notice(built, finishes, plant):
    """the faults of the compaction and of a position's width.  A case whose erased set the fault leaves as it is, on a committee of
    up to 256 rows, cannot tell - the model is not even asked; every other case is.  compaction_restarts, keeps_last_16 and
    position_mod_256 are noticed by wide cases and by no older case; which older cases notice counts_kept_only is printed."""
    old, new = [], []
    for case in ec.CASES:
        F = list(case.erased) if case.ok == "flags" else []
        if ec.planted_erasures(F, case.checks, plant) == (F, len(F), len(F) > case.checks) and (plant != "position_mod_256" or len(case.indices) <= 256):
            continue
        b = ec.build(case.name)
        right, wrong = finishes[case.name], ec.model_finish(case, b.rows, ec.CORRECT, plant=plant)
        if wrong.report != right.report or not np.array_equal(wrong.out, right.out):
            (new if case.name in ec.NEW else old).append(case.name)
    print(f"planted {plant}: noticed by {len(new)} new cases {new[:8]} and by {len(old)} older cases {old}")
    assert new, plant
    if plant == "counts_kept_only":
        assert old == ["k8_62-c16-d805-f17-e0-zero"]
    else:
        assert not old


@pytest.mark.parametrize("plant", ec.PLANTS)
def test_a_planted_fault_is_noticed(built, finishes, plant):
    """each fault planted in the model changes the output or the report of some case; the first such case is named"""
    for case in ec.CASES:
        b = ec.build(case.name)
        right, wrong = finishes[case.name], ec.model_finish(case, b.rows, ec.CORRECT, plant=plant)
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
    assert [ec.BY_NAME[n].dim for n in ec.GUARD] == list(vc.GUARD_DIMS) and all(ec.BY_NAME[n].scheme == "k8_62" for n in ec.GUARD)
    hit = []
    for name in ec.GUARD:
        case, rows = ec.BY_NAME[name], ec.build(name).rows
        fin = ec.model_finish(case, rows, vc.CORRECT)
        assert fin.report[1] == fin.report[2] == vc.batches(case), "every batch of a guard case is corrected"
        clean = vc.framed(ec.model_finish, case, rows, vc.CORRECT)
        assert clean[case.dim:] == [vc.SENTINEL] * vc.TAIL and vc.SENTINEL not in clean[:case.dim]
        if vc.framed(ec.model_finish, case, rows, vc.CORRECT, plant) != clean:
            hit.append(case.dim % 8)
    assert sorted(hit) == ([1, 1, 2, 3, 6, 7] if plant == "last_element_dropped" else [1, 1, 2, 3, 4])

"""The model of the checked reveal finish (tests/reveal_check_cases.py) against the C oracle, and what its cases reach - no device.
tests/test_reveal_check_gpu.py compares the device bit for bit against this model, so the model is proven here first: on clean rows
it is the oracle's reconstruction, on one faulty position its correction is the oracle's reconstruction of the other rows, and
every fault planted in the model itself is noticed by at least one case."""
import numpy as np
import pytest

import reveal_check_cases as vc


def _oracle(case, rows, keep=None):
    from oracle import coracle
    p, k, t, n, w2, w3 = vc.SCHEMES[case.scheme]
    keep = list(range(len(case.indices))) if keep is None else list(keep)
    canon = (rows[keep][:, :vc.batches(case)].astype(object) % p).astype(np.int64)
    return coracle.packed_reconstruct(p, k, t, w2, w3, case.dim, [case.indices[i] for i in keep], canon)


def _all_verdicts(case, fin):
    return set(fin.verdicts)


@pytest.mark.parametrize("name", [c.name for c in vc.CASES])
def test_model_equals_the_oracle(name):
    case, b = vc.BY_NAME[name], vc.build(name)
    rep, cor = vc.model_finish(case, b.rows, vc.REPORT), vc.model_finish(case, b.rows, vc.CORRECT)
    # SDA_CHECK_REPORT is the plain reconstruction of the rows as they are
    assert np.array_equal(rep.out, _oracle(case, b.rows))
    assert rep.report[:2] == cor.report[:2] and rep.report[3:] == cor.report[3:] and rep.report[2] == 0
    assert cor.report[2] == cor.report[1] == sum(cor.report[4:])
    assert np.array_equal(_oracle(case, b.clean_rows), b.want)
    if case.expect == "clean":
        assert rep.report == [0, 0, 0, vc.NONE64] + [0] * len(case.indices), rep.report[:4]
        assert np.array_equal(rep.out, b.want) and np.array_equal(cor.out, b.want)
    elif case.expect == "located":
        assert rep.report[0] > 0 and rep.report[1] == rep.report[0]
        assert {i for i, n in enumerate(rep.report[4:]) if n} == set(b.faulty)
        assert np.array_equal(cor.out, b.want), "a batch with one faulty position is corrected to the true secrets"
        assert not np.array_equal(rep.out, b.want)
    elif case.expect == "unlocated":
        assert rep.report[0] > 0 and rep.report[1] == 0 and not any(rep.report[4:])
        assert np.array_equal(cor.out, rep.out)
    if b.faulty is not None and len(b.faulty) == 1 and case.checks >= 2:
        keep = [i for i in range(len(case.indices)) if i != b.faulty[0]]
        assert np.array_equal(cor.out, _oracle(case, b.rows, keep)), "the correction is the reconstruction of the other rows"
        assert np.array_equal(cor.out, vc.unchecked_python(case, b.rows, keep))


def test_cases_reach_every_verdict():
    reached = set()
    for case in vc.CASES:
        b = vc.build(case.name)
        fin = vc.model_finish(case, b.rows, vc.CORRECT)
        B = vc.batches(case)
        v = set(fin.verdicts)
        if v == {"clean"}:
            reached.add("clean")
        if "located" in v:
            reached.add("bad + located")
            if fin.report[2]:
                reached.add("corrected")
        if "unlocated" in v:
            reached.add("bad + unlocated")
        padded = case.dim % vc.SCHEMES[case.scheme][1] != 0
        if case.fault == "last" and padded and B > 1 and fin.verdicts[:-1] == ["clean"] * (B - 1) and fin.verdicts[-1] != "clean":
            assert fin.report[3] == B - 1
            reached.add("last-batch-only")
        if case.fault == "surplus" and v == {"clean"} and not np.array_equal(b.rows, b.clean_rows):
            reached.add("surplus-ignored")
        if case.values == "congruent" and v == {"clean"} and not (b.rows == b.clean_rows).any():
            reached.add("congruent-but-different")
        reached.add("path " + vc.coef_path(case))
        if len({i for i, n in enumerate(fin.report[4:]) if n}) >= 2 and case.fault == "disjoint":
            reached.add("two positions blamed")
    assert reached == {"clean", "bad + located", "bad + unlocated", "corrected", "last-batch-only", "surplus-ignored",
                       "congruent-but-different", "path lds", "path global", "two positions blamed"}, reached


def test_shapes_sit_where_something_can_break():
    by = vc.BY_NAME
    assert {vc.width(c) for c in vc.CASES if c.scheme == "k8_62" and len(c.indices) == 26} == {16, 17}          # either side of kCoefLds
    assert vc.coef_path(by["k8_62-c8-d805-row"]) == "lds" and vc.coef_path(by["k8_62-c9-d805-row"]) == "global"
    assert vc.width(by["pss155-c5-d250-row"]) == 105 and vc.redundancy(by["pss155-c5-d250-row"]) == 5
    assert vc.redundancy(by["k3_62-five-c1-d1000-row"]) == 1 and vc.redundancy(by["k3_31-c1-d1000-row"]) == 1
    assert vc.redundancy(by["k8_62-twelve-c2-d805-row"]) == 2
    assert vc.batches(by["k3_62-c4-d1000-row"]) == 334 and 334 * 7 > 2048 and 334 > 256                          # window, workgroups
    assert {c.dim for c in vc.CASES if c.scheme == "k3_62" and c.indices == vc.ALL8} >= {1, 3, 4, 1000, 6301}
    assert {c.checks for c in vc.CASES if c.scheme == "k3_62" and c.dim == 6301} == {1, 2, 4}
    assert all(1 <= c.checks <= min(vc.redundancy(c), vc.MAX_CHECKS) for c in vc.CASES)
    assert {c.feed for c in vc.CASES} == {"one", "descending"}
    # the wide committee: its literals are extremes.omegas' (any distinct nodes), both coefficient paths, two workgroups and a tail
    import extremes
    p, k, t, n, w2, w3 = vc.SCHEMES["k3_wide"]
    assert (w2, w3) == extremes.omegas(p, k, t, n) and p == vc.SCHEMES["k3_62"][0] and (k, t, n) == (3, 1, 300)
    wide = [c for c in vc.CASES if c.scheme == "k3_wide"]
    assert {vc.width(c) for c in wide} == {5, 16, 19} and {vc.coef_path(c) for c in wide} == {"lds", "global"}
    assert {(len(c.indices), c.checks) for c in wide} >= {(300, 2), (300, 13), (300, 16), (257, 2)}
    assert {vc.batches(c) for c in wide} == {1, 257} and 769 % 3 == 1
    # the any-int64 rows hold the extremes
    rows = vc.build("k3_62-c4-d1000-crafted").rows
    assert vc.I64_MIN in rows and vc.I64_MAX in rows


def test_two_faulty_rows_are_located_to_nobody():
    """with >= 3 syndromes that is the Vandermonde argument; with 2 the seeds are pinned (the case names) and the model is asked"""
    seen = set()
    for case in vc.CASES:
        if case.fault != "two":
            continue
        fin = vc.model_finish(case, vc.build(case.name).rows, vc.CORRECT)
        assert fin.report[0] == vc.batches(case) and fin.report[1] == 0, case.name
        seen.add(min(case.checks, 3))
    assert seen == {1, 2, 3}


def test_wide_cases_blame_positions_past_a_byte():
    """the faulty rows of the wide cases are pinned: at least two cases blame a position >= 256, one the last row of 300 and one the
    last row of 257 - in the model's report, at the word the pinned position names"""
    high, last = [], []
    for case in vc.CASES:
        if case.scheme != "k3_wide" or case.fault != "row":
            continue
        b = vc.build(case.name)
        assert b.faulty == tuple(case.pin)
        fin = vc.model_finish(case, b.rows, vc.CORRECT)
        B = vc.batches(case)
        assert fin.report[4:] == [B if i == b.faulty[0] else 0 for i in range(len(case.indices))], case.name
        if b.faulty[0] >= 256:
            high.append(case.name)
        if b.faulty[0] == len(case.indices) - 1:
            last.append(len(case.indices))
    assert len(high) >= 2 and set(last) == {257, 300}, (high, last)
    two = [vc.build(c.name).faulty for c in vc.CASES if c.scheme == "k3_wide" and c.fault == "two"]
    assert all(max(f) >= 256 for f in two) and len(two) == 3


def test_steered_geometric_syndromes():
    """a ratio that is a point is located there; a ratio that is no point, and the ratio 1 - the node that is no row - are not"""
    case = vc.BY_NAME["k3_62-c4-d769-steered"]
    b, T = vc.build(case.name), vc.tables(case.scheme, case.indices, case.checks)
    fin = vc.model_finish(case, b.rows, vc.CORRECT)
    for batch in (0, 1, 2, 255, 256):
        sh = [int(b.rows[i][batch]) % T.p for i in range(8)]
        S = [sum(T.H[d][i] * sh[i] for i in range(8)) % T.p for d in range(4)]
        ratio = S[1] * pow(S[0], -1, T.p) % T.p
        assert all(S[d + 1] == ratio * S[d] % T.p for d in range(3)), "the planted errors do not give the syndromes back"
        assert (ratio == T.x[case.pin[0]], ratio not in T.x + [1], ratio == 1) == tuple(batch % 3 == r for r in range(3))
    assert fin.verdicts == [("located", "unlocated", "unlocated")[batch % 3] for batch in range(vc.batches(case))]
    located = len(range(0, vc.batches(case), 3))
    assert fin.report[:3] == [vc.batches(case), located, located] and fin.report[4 + case.pin[0]] == located
    out = fin.out.reshape(-1)
    want = b.want
    good = np.array([batch % 3 == 0 for batch in range(vc.batches(case)) for _ in range(3)][:case.dim])
    assert np.array_equal(out[good], want[good]) and (out[~good] != want[~good]).any()


def test_a_lost_high_byte_is_noticed_by_the_wide_cases_alone():
    """position_mod_256: a case of up to 256 rows cannot tell (a position below 256 is its own low byte: the model is not even
    asked); of the older cases with more rows none locates a position past 255; the pinned wide cases do"""
    noticed = {}
    for case in vc.CASES:
        if len(case.indices) <= 256:
            continue
        b = vc.build(case.name)
        good, off = vc.model_finish(case, b.rows, vc.CORRECT), vc.model_finish(case, b.rows, vc.CORRECT, plant="position_mod_256")
        noticed[case.name] = good.report != off.report or not np.array_equal(good.out, off.out)
    old = [n for n, hit in noticed.items() if hit and vc.BY_NAME[n].scheme != "k3_wide"]
    new = [n for n, hit in noticed.items() if hit and vc.BY_NAME[n].scheme == "k3_wide"]
    print("position_mod_256 noticed by", new, "and of the older cases by", old)
    assert not old and len(new) >= 3


PLANTS = ("weight", "no_node1", "locate", "sign")


@pytest.mark.parametrize("plant", PLANTS)
def test_a_planted_model_fault_is_noticed(plant):
    """a wrong syndrome weight, node 1 dropped from u_i, the locate loop one short, the correction's sign: some case differs"""
    probes = ["k3_62-c4-d4-clean", "k3_62-c4-d4-row", "k3_62-c2-d4-last", "k3_62-c3-d1000-two", "k8_62-twelve-c2-d805-row"]
    noticed = []
    for name in probes:
        case, b = vc.BY_NAME[name], vc.build(name)
        good, off = vc.model_finish(case, b.rows, vc.CORRECT), vc.model_finish(case, b.rows, vc.CORRECT, plant=plant)
        if good.report != off.report or not np.array_equal(good.out, off.out):
            noticed.append(name)
    print(plant, "noticed by", noticed)
    assert noticed, plant


# ---- the store the plain finishes share: what the guard cases are there for ---------------------------------------------------------
@pytest.mark.parametrize("plant", vc.STORE_PLANTS)
def test_the_guard_cases_notice_a_planted_store_fault(plant):
    """the GPU runners check the output against the model and the words behind it against the sentinel - together the buffer of
    vc.framed(): a store that drops the last element of a partial
    group, or stores an all-padding second group, leaves other words there at every dimension the guard cases were chosen for"""
    assert [vc.BY_NAME[n].dim for n in vc.GUARD] == list(vc.GUARD_DIMS) and all(vc.BY_NAME[n].scheme == "k8_62" for n in vc.GUARD)
    hit = []
    for name in vc.GUARD:
        case, rows = vc.BY_NAME[name], vc.build(name).rows
        fin = vc.model_finish(case, rows, vc.CORRECT)
        assert fin.report[1] == fin.report[2] == vc.batches(case), "every batch of a guard case is corrected"
        clean = vc.framed(vc.model_finish, case, rows, vc.CORRECT)
        assert clean[case.dim:] == [vc.SENTINEL] * vc.TAIL and vc.SENTINEL not in clean[:case.dim]
        if vc.framed(vc.model_finish, case, rows, vc.CORRECT, plant) != clean:
            hit.append(case.dim % 8)
    assert sorted(hit) == ([1, 1, 2, 3, 6, 7] if plant == "last_element_dropped" else [1, 1, 2, 3, 4])

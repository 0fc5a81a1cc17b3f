"""What the case table of tests/unmask_checked_cases.py contains, proved on the CPU from its Python-integer model alone: every
combination sda_secret_unmasker_unmask_checked_jobs_dev treats differently is there BY NAME, the model is the composition of the
existing models, and each fault planted in the model is noticed - the test names the case that notices it first - so a green
tests/test_unmask_checked_gpu.py says something about each of them.  For the cases that came with the wide committees: the older
cases' rows are what they were (by digest), every wide and steered case of the three finish tables is borrowed with its rows and
its fields, the finish tables' gap plants reach the UNMASKED output of a named new case, five faults of the glue around the decoder
walks and one of the mask sum's high word are noticed by the case that is there for them, and the reach table - workgroups, blame
past position 255, `have` per group, steered families per wave, the setup kernel's steps, the high words - is printed and asserted."""
import numpy as np
import pytest

import chacha_repair as cr
import reconstruct_stream_cases as rc
import reveal_check_cases as vc
import reveal_decode_cases as dc
import reveal_erasure_cases as ec
import unmask_checked_cases as kc
import unmask_jobs_cases as uc

LANES = 256                                # sda_kernels.hip kThreads; a lane takes one batch
WAVE = 64
OLD = [c.name for c in kc.CASES[:kc.PARENT_CASES]]                                    # the table before the wide committees
SHUT_WIDE = ("locate-correct-from-k3_wide-c16-d769-row-shut-masks", "decode-correct-from-k3_wide-c16-d769-rows2-shut-results",
             "erasures-correct-from-k3_wide-c16-d769-f5-e5-zero-shut-equal")
SPARSE = [c.name for c in kc.CASES if c.values == "sparse"]


@pytest.fixture(autouse=True)
def _the_entry_point_exists(built):
    """the table is about one entry point: without it in the ctypes table no statement below means anything (built: the borrowed
    cases' rows are the finish tables', whose clean rows are the C oracle's shares)"""
    from sda_amd import capi
    assert "sda_secret_unmasker_unmask_checked_jobs_dev" in capi.SIGNATURES


def _open(c):
    return not kc.gate_shut(c)


def test_every_end_with_both_policies_by_name():
    names = set(kc.BY_NAME)
    for tag in ("report", "correct"):
        assert {f"k3_62-locate-{tag}-d769-row1", f"k3_62-decode-{tag}-d766-rows2", f"k3_62-erasures-{tag}-d764-f1-e1"} <= names
    assert {(c.end, c.policy) for c in kc.CASES if _open(c)} == {(e, p) for e in kc.ENDS for p in (kc.REPORT, kc.CORRECT)}


def test_every_masking_kind_modulus_relation_padding_and_gate_form():
    cases = [c for c in kc.CASES if _open(c)]
    for end in kc.ENDS:
        mine = [c for c in cases if c.end == end]
        assert {c.masking.split("-")[0] for c in mine} == {"full", "chacha", "none"}, kc.ENDS[end]
        assert {kc.modulus_relation(c) for c in mine} >= {"equal", "below", "none"}, kc.ENDS[end]
        assert {kc.padding_form(c) for c in mine} >= {0, 1, 2}, kc.ENDS[end]          # dimension mod 3 = 0, 2, 1 on k3_62
        assert {c.offset for c in mine} == {0, 8}, kc.ENDS[end]
        assert any(kc.gate_shut(c) for c in kc.CASES if c.end == end), kc.ENDS[end]
    by = kc.BY_NAME
    assert by["k3_62-locate-correct-d764-none-combiner"].masking == "none-combiner"
    # q_mask above the sharing modulus: k3_31 has one check, which the decoding end refuses
    assert kc.modulus_relation(by["k3_31-locate-correct-d766-full62-row1"]) == "above"
    assert kc.modulus_relation(by["k3_31-erasures-correct-d766-full62-f1"]) == "above"
    assert kc.modulus_relation(by["pss155-erasures-correct-d250-f1-e1"]) == "above"
    assert {c.gates for c in cases} == {"null", "two", "equal"}
    shut = {c.name: c for c in kc.CASES if kc.gate_shut(c)}
    assert {"k3_62-locate-correct-d769-shut-masks", "k3_62-decode-correct-d766-shut-results", "k3_62-erasures-correct-d764-shut-equal",
            "k3_62-decode-correct-d4-none-null-shut-masks", "k3_62-erasures-correct-d764-word16-pass0",
            "k3_62-erasures-correct-d764-word18-pass16"} == set(shut) - set(kc.NEW)
    assert set(shut) & set(kc.NEW) == set(SHUT_WIDE)                                  # ... and the wide committee's three
    assert shut["k3_62-locate-correct-d769-shut-masks"].word_m and shut["k3_62-decode-correct-d766-shut-results"].word_r
    # the pass bits: the word 16 with pass bits 16 stores
    for name in ("k3_62-erasures-correct-d764-word16-pass16", "k3_62-locate-report-d3-word16-pass16"):
        assert by[name].word_r == 16 and by[name].pass_bits == 16 and _open(by[name])
    assert by["k3_62-erasures-correct-d764-word18-pass16"].word_r == 16 | 2


def test_the_shapes():
    by = kc.BY_NAME
    got = {kc.batches(c) for c in kc.CASES if c.scheme == "k3_62"}
    assert {1, LANES - 1, LANES, LANES + 1} <= got
    assert {c.dim % 3 for c in kc.CASES if c.scheme == "k3_62" and kc.batches(c) >= LANES - 1} == {0, 1, 2}
    # the secret groups: one of 3, 4 + 4, 25 of 4 with 50 padding sums over 3 batches
    assert rc.SCHEMES["k3_62"][1] == 3 and rc.SCHEMES["k8_62"][1] == 8 and rc.SCHEMES["pss155"][1] == 100
    pss = by["pss155-decode-correct-d250-rows2"]
    assert kc.batches(pss) == 3 and kc.padding_form(pss) == 50 and len(pss.indices) == 260
    assert kc.padding_form(by["k8_62-decode-correct-d61-rows8"]) == 3
    # the mask job holds dim sums: the padding of the last batch has none
    for c in (pss, by["k8_62-decode-correct-d61-rows8"], by["k3_62-decode-correct-d766-rows2"]):
        assert len(kc.mask_sums(c.name)) == c.dim < kc.batches(c) * rc.SCHEMES[c.scheme][1]


def test_the_row_sets_reach_their_verdicts():
    by = kc.BY_NAME
    B = kc.batches

    def verdicts(name):
        return list(kc.finish(name).verdicts)
    for name in [c.name for c in kc.CASES if c.values == "sums" and not c.faulty and not c.erased]:
        assert set(verdicts(name)) <= {"clean", 0}, name
    assert set(verdicts("k3_62-locate-correct-d769-row1")) == {"located"}
    assert set(verdicts("k3_62-locate-correct-d769-rows2")) == {"unlocated"}
    assert set(verdicts("k3_62-decode-correct-d766-rows2")) == {2}                    # floor(checks / 2)
    assert set(verdicts("k3_62-decode-correct-d771-rows3")) == {-1}                   # one more: stays undecoded
    assert set(verdicts("k8_62-decode-correct-d61-rows8")) == {8} and set(verdicts("k8_62-decode-correct-d61-rows9")) == {-1}
    assert set(verdicts("k3_62-erasures-correct-d764-f1-e1")) == {1}                  # erasures together with errors
    assert set(verdicts("k3_62-erasures-correct-d764-f2-e2")) == {-1}
    assert set(verdicts("k8_62-erasures-report-d61-f3-e6")) == {6}
    for name, f in (("k3_62-erasures-correct-d766-f1", 1), ("k3_62-erasures-correct-d766-f4", 4), ("k8_62-erasures-correct-d61-f16", 16)):
        rep = kc.finish(name).report
        assert rep[6] == f == len(by[name].erased) and rep[7] == 0 and set(verdicts(name)) == {"consistent"}, name
    for name in ("k3_62-erasures-correct-d766-f5", "k8_62-erasures-correct-d61-f17"):
        rep = kc.finish(name).report
        assert rep[6] == by[name].checks + 1 and rep[7] == 1 and rep[0] == 0, name
    # a correction happens wherever the case is there for one: the corrected output is not the plain fold
    for name in ("k3_62-locate-correct-d769-row1", "k3_62-decode-correct-d766-rows2", "k3_62-erasures-correct-d764-f1-e1",
                 "k3_62-erasures-correct-d766-f4", "k3_31-erasures-correct-d766-full62-f1", "pss155-decode-correct-d250-rows2",
                 "k3_62-locate-correct-d766-full61-row1", "k3_62-decode-correct-d766-full61-rows2", "k3_62-erasures-correct-d766-chacha61-f1-e1"):
        changed = int((kc.finish(name).out != kc.finish(name, kc.REPORT).out).sum())
        print(f"{name}: {changed} of {by[name].dim} values corrected")
        assert changed > by[name].dim // 2, name
    assert B(by["k3_62-decode-correct-d1-row1"]) == 1


@pytest.mark.parametrize("name", [c.name for c in kc.CASES if kc.modulus_relation(c) == "below" and _open(c)])
def test_masked_values_at_or_above_the_masking_modulus(name):
    c = kc.BY_NAME[name]
    v = [int(x) for x in kc.finish(name).out]
    n = sum(x >= c.q_mask for x in v)
    print(f"{name}: {n} of {len(v)} masked values >= q_mask")
    assert n > 0 or c.masks in cr.SEEDS                                               # the located seed's case has 8 values


def test_the_chacha_jobs():
    noseed = kc.BY_NAME["k3_62-locate-correct-d769-chacha-noseed"]
    assert kc.build(noseed.name).mask_rows.shape[0] == 0
    m = kc.model(noseed.name)
    assert all(s == 0 for s in kc.mask_sums(noseed.name)) and m.out == tuple(int(x) for x in kc.finish(noseed.name).out)
    rej = kc.BY_NAME["k3_62-decode-correct-d8-chacha-rejecting"]
    seed, q, dim, pins = cr.SEEDS[rej.masks]
    assert (q, dim) == (rej.q_mask, rej.dim) and uc.chacha_rejections(list(seed), q, dim) > 0
    assert kc.build("k3_62-decode-correct-d771-clean").mask_rows.shape == (5, 4)


def test_none_stores_the_finish_output():
    for name in ("k3_62-decode-correct-d766-none-null", "k3_62-locate-correct-d764-none-combiner", "k3_62-erasures-correct-d4-none-null"):
        assert kc.model(name).out == tuple(int(x) for x in kc.finish(name).out) and kc.mask_sums(name) == ()


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_the_model_is_the_composition_of_the_existing_models(name):
    """the finish model of the end (reveal_*_cases.model_finish, called here on its own), then unmask_jobs_cases' formula
    submod(canon(v, q_mask), fold(mask sums, q_mask), q_mask), element by element; the report is the finish model's"""
    c, m = kc.BY_NAME[name], kc.model(name)
    fin = {kc.LOCATE: vc.model_finish, kc.DECODE: dc.model_finish, kc.ERASURES: ec.model_finish}[c.end](c, kc.build(name).rows, c.policy)
    assert len(fin.out) == c.dim
    sums = kc.mask_sums(name)
    for i in range(c.dim):
        v = int(fin.out[i])
        if kc.has_mask(c):
            x, y = v % c.q_mask, sums[i] % c.q_mask
            v = x - y if x >= y else x + c.q_mask - y
        assert m.out[i] == v
    head = c.offset // 8
    assert m.buffer[:head] == (kc.SENTINEL,) * head and m.buffer[head + c.dim:] == (kc.SENTINEL,) * kc.TAIL
    assert m.buffer[head:head + c.dim] == ((kc.SENTINEL,) * c.dim if kc.gate_shut(c) else m.out)
    assert list(m.report_buffer) == [int(w) for w in fin.report] + [kc.SENTINEL] * kc.TAIL          # whether or not the gate is shut
    assert len(fin.report) == kc.report_words(c)
    assert np.array_equal(kc.want(name)[0], np.array(m.buffer, dtype=np.int64))


# the first case of the table, in its order, whose expected buffers change under the planted fault
FIRST_NOTICED_BY = {
    "correction_after_canonicalisation": "pss155-erasures-correct-d250-f1-e1",
    "no_canonicalisation": "k3_62-decode-correct-d8-chacha-rejecting",
    "subtraction_under_sharing_modulus": "pss155-erasures-correct-d250-f1-e1",
    "padding_stored": "k3_62-locate-report-d769-row1",
    "gate_ignored": "k3_62-locate-correct-d769-shut-masks",
    "pass_bits_ignored": "k3_62-erasures-correct-d764-word16-pass16",
    "report_suppressed": "k3_62-locate-correct-d769-shut-masks",
    # the glue faults and the mask sums' high word: test_a_glue_fault_is_noticed_by_its_named_case says more about them
    "first_bad_workgroup_local": "decode-report-from-k3_wide-c16-d769-last",
    "first_bad_from_first_lane": "decode-report-from-k3_wide-c16-d769-stair",
    "blame_once_per_wave": "k3_62-locate-report-d769-row1",
    "second_group_unguarded": "k8_62-locate-correct-d57-row1",
    "last_element_dropped": "k3_62-locate-report-d769-row1",
    "mask_hi_kept_to_4_bits": "k3_62-locate-correct-d769-full61-masks40",
}


def _noticed(name, fault):
    good, bad = kc.model(name), kc.model(name, frozenset([fault]))
    return sum(x != y for x, y in zip(good.buffer + good.report_buffer, bad.buffer + bad.report_buffer))


def test_every_fault_is_listed():
    assert set(FIRST_NOTICED_BY) == set(kc.FAULTS)


@pytest.mark.parametrize("fault", kc.FAULTS)
def test_a_planted_fault_is_noticed(fault):
    first = next((c.name for c in kc.CASES if _noticed(c.name, fault)), None)
    every = [c.name for c in kc.CASES if _noticed(c.name, fault)]
    print(f"{fault}: noticed first by {first}, by {len(every)} of {len(kc.CASES)} cases in all")
    assert first == FIRST_NOTICED_BY[fault]
    assert len(every) >= 2


@pytest.mark.parametrize("name", [c.name for c in kc.CASES if kc.gate_shut(c)])
def test_a_shut_gate_leaves_the_sentinel_and_writes_the_report(name):
    m = kc.model(name)
    assert set(m.buffer) == {kc.SENTINEL} and list(m.report) == [int(w) for w in kc.finish(name).report]
    assert m.report[0] > 0 or kc.BY_NAME[name].erased                                 # a report worth reading: bad batches, or f


# ---- what came with the wide committees: borrowed cases, sparse faults, the guards, deep mask sums -----------------------------------
def _digest(name):
    import hashlib
    h = hashlib.sha256()
    for a in kc.build(name):
        h.update(str(a.shape).encode())
        h.update(a.astype("<i8").tobytes())
    return h.hexdigest()[:32]


def test_the_older_cases_rows_are_what_they_were():
    """a digest of every older case's rows and mask rows, recorded before the table grew"""
    from unmask_checked_parent_rows import PARENT_ROWS as gold
    assert list(gold) == OLD and len(OLD) == kc.PARENT_CASES == 52
    for name in OLD:
        assert _digest(name) == gold[name], name
        c = kc.BY_NAME[name]
        assert (c.source, c.source_name, c.pin, c.fill, c.bad) == (None, None, None, "zero", None)


def test_every_wide_and_steered_case_of_the_finish_tables_is_borrowed():
    want = {("reveal_decode_cases", n, kc.DECODE) for n in dc.NEW} | {("reveal_erasure_cases", n, kc.ERASURES) for n in ec.NEW} \
        | {("reveal_check_cases", c.name, kc.LOCATE) for c in vc.CASES if c.scheme == "k3_wide"}
    assert want <= set(kc.BORROWED) and len(set(kc.BORROWED)) == len(kc.BORROWED)
    assert {"k3_62-c4-d769-steered", "k8_62-c16-d805-steered", "k8_62-c16-d805-steered-cap2"} <= set(dc.NEW)      # the older shapes' steered cases: once
    got = [(c.source, c.source_name, c.end, c.policy) for c in kc.CASES if c.source and _open(c)]
    assert sorted(got) == sorted((s, n, e, p) for s, n, e in kc.BORROWED for p in (kc.REPORT, kc.CORRECT))
    print(f"borrowed: {len(kc.BORROWED)} source cases -", {s: sum(1 for b in kc.BORROWED if b[0] == s) for s in kc.SOURCES})
    seen = set()
    for i, (source, source_name, end) in enumerate(kc.BORROWED):
        what, fields = kc.ROTATION[i % 4]
        src = kc.SOURCES[source].BY_NAME[source_name]
        twins = [kc.BY_NAME[f"{kc.ENDS[end]}-{tag}-from-{source_name}"] for tag in ("report", "correct")]
        print(f"{i:3d} {kc.ENDS[end]:8s} {source_name:44s} {what}; gates {kc.GATE_FORMS[i % 3]}; offsets {[c.offset for c in twins]}")
        for c in twins:
            assert (c.scheme, c.dim, c.indices, c.checks, c.pin) == (src.scheme, src.dim, tuple(src.indices), src.checks, src.pin)
            assert (c.masking, c.q_mask, c.masks) == (fields["masking"], fields["q_mask"], fields["masks"]) and c.gates == kc.GATE_FORMS[i % 3]
            assert c.cap == getattr(src, "cap", 0) and c.values == "borrowed" and not c.faulty
            if end == kc.ERASURES:
                assert (c.erased, c.fill, c.ok) == (src.erased, src.fill, src.ok)
                want_ok, got_ok = ec.ok_words(src), kc.ok_words(c)
                assert (want_ok is None and got_ok is None) or np.array_equal(want_ok, got_ok)
            rows = kc.build(c.name).rows
            assert np.array_equal(rows, kc.SOURCES[source].build(source_name).rows) and rows.shape[1] == kc.batches(c)
            seen.add((end, i % 4, c.offset))
        assert sorted(c.offset for c in twins) == [0, 8]
    assert seen == {(e, r, o) for e in kc.ENDS for r in range(4) for o in (0, 8)}                 # every arrangement at every end, on and off 16 bytes
    fed = [c for c in kc.CASES if c.source == "reveal_erasure_cases"]
    assert {c.ok for c in fed} == {"flags", "ones", "null"} and {c.fill for c in fed} >= {"zero", "random", "spoiled"}
    # ... and the three behind a shut gate, one per end and per way of shutting it
    shut = [kc.BY_NAME[n] for n in SHUT_WIDE]
    assert [c.end for c in shut] == [kc.LOCATE, kc.DECODE, kc.ERASURES] and all(c.scheme == "k3_wide" and kc.gate_shut(c) for c in shut)
    assert [(c.gates, bool(c.word_m), bool(c.word_r)) for c in shut] == [("two", True, False), ("two", False, True), ("equal", True, False)]
    for c in shut:
        m = kc.model(c.name)
        assert set(m.buffer) == {kc.SENTINEL} and any(m.report[kc.report_words(c) - len(c.indices) + 256:]), c.name    # blame past position 255


@pytest.mark.parametrize("name", SPARSE)
def test_sparse_faults_over_five_workgroups(name):
    c, fin = kc.BY_NAME[name], kc.finish(name)
    bad = dict(c.bad)
    wide = c.scheme == "k3_wide"
    assert kc.batches(c) == 1100 and -(-kc.batches(c) // LANES) == 5 and c.dim % 3 in (1, 2) and len(c.indices) == (300 if wide else 8)
    got = [b for b, v in enumerate(fin.verdicts) if v not in ("clean", "consistent", 0)]
    lost = [b for b, v in enumerate(fin.verdicts) if v in ("unlocated", -1)]
    assert got == sorted(bad) and lost == [700]
    assert {b // LANES for b in got} == {1, 2, 4} and min(got) == 300 and 300 % WAVE == 44 and max(got) == kc.batches(c) - 1
    assert fin.report[0] == len(bad) and fin.report[1] == len(bad) - 1 and fin.report[3] == 300
    if c.end != kc.LOCATE:
        assert fin.report[4] == 700
    at = kc.blamed(name)
    assert all(at[b] == (tuple(sorted(bad[b])) if b != 700 else ()) for b in range(kc.batches(c)) if b in bad or at[b])
    assert 300 // WAVE == 301 // WAVE == 302 // WAVE and at[300].index(2) == at[301].index(2) and not set(at[302]) & set(at[300])
    blame = fin.report[kc.report_words(c) - len(c.indices):]
    assert blame[2] == 2 and blame == [sum(i in at[b] for b in bad) for i in range(len(c.indices))]
    if wide:
        assert at[302] == (257,) and blame[257] >= 1 and blame[299] >= 1
    if c.end == kc.ERASURES:
        assert c.erased == ((256,) if wide else (3,)) and {v for b, v in enumerate(fin.verdicts) if b not in bad} == {"consistent"}
    plain = kc.finish(name, kc.REPORT).out
    k = rc.SCHEMES[c.scheme][1]
    changed = sorted({i // k for i in np.nonzero(plain != fin.out)[0]})
    if c.policy == kc.REPORT:
        assert not changed and fin.report[2] == 0
    elif c.end != kc.ERASURES:
        assert changed == [b for b in sorted(bad) if b != 700]                           # the corrections, and nothing else
    else:
        assert changed == [b for b in range(kc.batches(c)) if b != 700]                  # every batch is mended; 700 stays as it folds
    print(f"{name}: bad {got}, blamed {[at[b] for b in got]}")


def test_the_guard_geometry():
    """`have` of every group of the last batch, by unmask_group_have's rule"""
    new = [kc.BY_NAME[n] for n in kc.NEW]
    k8 = {c.dim % 8: c for c in kc.CASES if c.scheme == "k8_62" and 1 < c.dim < 100}
    assert sorted(k8) == [1, 2, 3, 4, 5, 6, 7] and [n for n, c in k8.items() if c.name in OLD] == [5]
    assert {r: kc.group_haves(c) for r, c in k8.items()} == {1: (1, 0), 2: (2, 0), 3: (3, 0), 4: (4, 0), 5: (4, 1), 6: (4, 2), 7: (4, 3)}
    assert {c.end for c in new if c.scheme == "k8_62" and not c.source} == set(kc.ENDS)
    pss = {c.dim: c for c in kc.CASES if c.scheme == "pss155" and c.dim > 1}
    assert sorted(pss) == [248, 249, 250, 251] and {pss[d].end for d in (248, 249, 251)} == set(kc.ENDS)
    for dim, partial in ((248, ()), (249, (1,)), (250, (2,)), (251, (3,))):
        c = pss[dim]
        assert kc.group_haves(c) == (4,) * 12 + partial + (0,) * (13 - len(partial)) and kc.batches(c) == 3 and kc.has_mask(c), dim
        assert c.checks == 5 and len(c.indices) == 260
    for name, haves in (("k8_62-decode-correct-d1-rows8", (1, 0)), ("pss155-locate-correct-d1-row1", (1,) + (0,) * 24)):
        assert kc.batches(kc.BY_NAME[name]) == 1 and kc.group_haves(kc.BY_NAME[name]) == haves
    for c in new:
        if not c.source and c.values != "sparse":
            print(f"{c.name}: have {kc.group_haves(c)}")
    # a correction happens in each of them: the partial group is corrected, masked and stored
    for c in [k8[r] for r in (1, 2, 3, 4, 6, 7)] + [pss[248], pss[249], pss[251]]:
        assert (kc.finish(c.name).out != kc.finish(c.name, kc.REPORT).out).all(), c.name


def test_the_mask_sums_high_words():
    """computed from the mask rows: three rows keep the high word of a sum within -2 .. 1, the forty-row cases go beyond +-8"""
    forty = [c for c in kc.CASES if c.masks == "crafted40"]
    assert [c.end for c in forty] == list(kc.ENDS) and all(c.q_mask == kc.Q61 and c.scheme == "k3_62" and c.name in kc.NEW for c in forty)
    most = 0
    for c in kc.CASES:
        hi = kc.mask_high_words(c.name) if kc.has_mask(c) else [0]
        if c in forty:
            assert kc.build(c.name).mask_rows.shape == (40, c.dim)
            print(f"{c.name}: high words {min(hi)} .. {max(hi)}")
            assert min(hi) < -8 and max(hi) > 8
            most = max(most, max(abs(h) for h in hi))
        else:
            assert -8 <= min(hi) and max(hi) < 8 and (c.masking != "full" or kc.build(c.name).mask_rows.shape[0] == 3), c.name
    print(f"the largest |hi| of a mask sum: {most}")
    assert most == 15
    by = kc.BY_NAME
    assert by["k3_62-decode-correct-d766-full2-crafted"].q_mask == 2 and set(kc.model("k3_62-decode-correct-d766-full2-crafted").out) == {0, 1}
    top = by["k3_62-locate-correct-d766-fullmax-row1"]
    assert top.q_mask == kc.Q_MAX == (1 << 62) - 1 and kc.modulus_relation(top) == "above"       # make_mod: 2 <= m < 2^62
    assert max(int(v) for v in kc.build(top.name).mask_rows.max(axis=0)) > 1 << 61


# the first new case - a correcting one - whose expected buffers change under a fault planted in the finish model (the OUTPUT
# buffer, but for the two faults of the root search), and the
# older cases that notice it too (committees of up to 256 rows cannot; pss155 has 260, and its erased row 258 is row 2 modulo 256)
FINISH_PLANT_NOTICED_BY = {
    (kc.LOCATE, "position_mod_256"): ("locate-correct-from-k3_wide-c2-d769-row", []),
    (kc.DECODE, "position_mod_256"): ("decode-correct-from-k3_wide-c16-d769-rows1", []),
    (kc.DECODE, "root_at_node_one"): ("decode-correct-from-k3_62-c4-d769-steered", []),
    (kc.DECODE, "root_at_zero"): ("decode-correct-from-k3_62-c4-d769-steered", []),
    (kc.ERASURES, "compaction_restarts"): ("erasures-correct-from-k3_wide-c16-d769-f5-e5-zero", ["pss155-erasures-correct-d250-f1-e1"]),
    (kc.ERASURES, "keeps_last_16"): ("erasures-correct-from-k3_wide-c16-d769-f5-e5-zero", []),
    (kc.ERASURES, "position_mod_256"): ("erasures-correct-from-k3_wide-c16-d769-f5-e5-zero", ["pss155-erasures-correct-d250-f1-e1"]),
    (kc.ERASURES, "counts_kept_only"): ("erasures-correct-from-k3_wide-c16-d769-f17-e0-zero", ["k8_62-erasures-correct-d61-f17"]),
}


def _changed(name, fault):
    """(words of the output buffer, words of the report buffer) that the planted fault changes"""
    good, bad = kc.model(name), kc.model(name, frozenset([fault]))
    return sum(x != y for x, y in zip(good.buffer, bad.buffer)), sum(x != y for x, y in zip(good.report_buffer, bad.report_buffer))


def test_every_finish_plant_is_listed():
    assert set(FINISH_PLANT_NOTICED_BY) == {(end, plant) for end, plants in kc.FINISH_PLANTS.items() for plant in plants}
    assert set(kc.FINISH_PLANTS[kc.DECODE]) == set(dc.GAP_PLANTS) and set(kc.FINISH_PLANTS[kc.ERASURES]) == set(ec.GAP_PLANTS)


@pytest.mark.parametrize("end, plant", list(FINISH_PLANT_NOTICED_BY))
def test_a_fault_planted_in_the_finish_model_changes_the_unmasked_output(end, plant):
    """model(name, {plant}) hands the plant to the source table's model_finish: the UNMASKED output buffer of a named new case
    changes, not the finish's alone.  No older case notices position_mod_256 on the locating and the decoding end; on the erasure
    end pss155's older case does (its erased row is 258), and the statement says so"""
    named, older = FINISH_PLANT_NOTICED_BY[end, plant]
    steered = lambda c: "steered" in (getattr(kc.SOURCES[c.source].BY_NAME[c.source_name], "fault", None),
                                      getattr(kc.SOURCES[c.source].BY_NAME[c.source_name], "errors", None))
    first = None
    for name in kc.NEW:
        c = kc.BY_NAME[name]
        if c.end != end or c.policy != kc.CORRECT or not _open(c) or (plant.startswith("root_at") and not (c.source and steered(c))):
            continue
        if any(_changed(name, plant)):
            first = name
            break
    out, rep = _changed(named, plant)
    print(f"{kc.ENDS[end]} / {plant}: {named} - {out} output words and {rep} report words change")
    assert first == named, f"{plant} is first noticed by {first}"
    if plant.startswith("root_at"):                                     # the root that is no row is counted and blamed nowhere: the report alone
        assert (out, rep) == (0, 3)
    else:
        assert out > 0 and rep > 0 and kc.model(named, frozenset([plant])).out != kc.model(named).out
    got = [n for n in OLD if kc.BY_NAME[n].end == end and any(_changed(n, plant))]
    print(f"{kc.ENDS[end]} / {plant}: older cases that notice: {got}")
    assert got == older


# fault -> the new case that is there for it, what it does to that case, and how many OLDER cases notice it.  Two of the faults
# cannot hide from the older table: all its faulty rows are wrong in every batch, so every wave blames a position from many lanes
# (blame_once_per_wave), and most of its dimensions end in a partial group (last_element_dropped); the new cases name the state
GLUE_NOTICED_BY = {
    "first_bad_workgroup_local": ("k3_62-decode-correct-d3299-sparse", 0),
    "first_bad_from_first_lane": ("k3_wide-decode-correct-d3298-sparse", 0),
    "blame_once_per_wave": ("k3_wide-locate-correct-d3298-sparse", 24),
    "second_group_unguarded": ("k8_62-locate-correct-d60-row1", 0),
    "last_element_dropped": ("k8_62-erasures-correct-d59-f3-e6", 38),
    "mask_hi_kept_to_4_bits": ("k3_62-decode-correct-d769-full61-masks40", 0),
}


@pytest.mark.parametrize("fault", list(GLUE_NOTICED_BY))
def test_a_glue_fault_is_noticed_by_its_named_case(fault):
    assert set(GLUE_NOTICED_BY) == set(kc.GLUE_FAULTS) | {"mask_hi_kept_to_4_bits"}
    named, older = GLUE_NOTICED_BY[fault]
    assert named in kc.NEW
    c, good, bad = kc.BY_NAME[named], kc.model(named), kc.model(named, frozenset([fault]))
    out, rep = _changed(named, fault)
    got = [n for n in OLD if any(_changed(n, fault))]
    print(f"{fault}: {named} - {out} output words and {rep} report words change; {len(got)} older cases notice {got[:3]}")
    assert out + rep > 0 and len(got) == older
    head, blame = c.offset // 8, kc.report_words(c) - len(c.indices)
    if fault == "first_bad_workgroup_local":
        assert good.report[3:5] == (300, 700) and bad.report[3:5] == (300 - 256, 700 - 512) and (out, rep) == (0, 2)
    elif fault == "first_bad_from_first_lane":
        assert good.report[3:5] == (300, 700) and bad.report[3:5] == (256, 640) and (out, rep) == (0, 2)
    elif fault == "blame_once_per_wave":
        assert good.report[blame + 2] == 2 and bad.report[blame + 2] == 1 and good.report[blame + 257] == bad.report[blame + 257] == 1 and (out, rep) == (0, 1)
    elif fault == "second_group_unguarded":                              # dimension 60: the second group of batch 7 is all padding
        assert kc.group_haves(c) == (4, 0) and good.buffer[head + c.dim:] == (kc.SENTINEL,) * kc.TAIL and (out, rep) == (4, 0)
        assert all(w != kc.SENTINEL for w in bad.buffer[head + c.dim:head + c.dim + 4]) and bad.buffer[head + c.dim + 4:] == (kc.SENTINEL,) * 4
    elif fault == "last_element_dropped":                                # dimension 59: the first group of batch 7 has three of four
        assert kc.group_haves(c) == (3, 0) and bad.buffer[head + c.dim - 1] == kc.SENTINEL != good.buffer[head + c.dim - 1] and (out, rep) == (1, 0)
    else:
        hi = kc.mask_high_words(named)
        assert rep == 0 and out == sum(not -8 <= h < 8 for h in hi) > c.dim // 4
    if fault in ("second_group_unguarded", "last_element_dropped"):      # every residue the guard cases are there for
        k8 = {q.dim % 8: q.name for q in kc.CASES if q.scheme == "k8_62" and 1 < q.dim < 100}
        hit = sorted(r for r, n in k8.items() if any(_changed(n, fault)))
        assert hit == ([1, 2, 3, 4] if fault == "second_group_unguarded" else [1, 2, 3, 5, 6, 7])


def test_what_the_new_cases_reach():
    """the reach table: workgroups, blame past position 255, the guards' `have`, the steered families in every wave, the setup
    kernel's two steps, the mask sums' high words"""
    new = [kc.BY_NAME[n] for n in kc.NEW]
    groups = {}
    for c in new:
        groups.setdefault(-(-kc.batches(c) // LANES), []).append(c.name)
    for wg, names in sorted(groups.items()):
        print(f"{wg} workgroup(s): {len(names)} cases, e.g. {names[0]}")
    assert sorted(groups) == [1, 2, 5] and set(groups[5]) == set(SPARSE) and len(SPARSE) == 8
    # positions blamed at and past 256, from the models' report words
    high = {e: [] for e in kc.ENDS}
    for c in new:
        if len(c.indices) > 256 and any(kc.model(c.name).report[kc.report_words(c) - len(c.indices) + 256:]):
            high[c.end].append(c.name)
    for e in kc.ENDS:
        print(f"{kc.ENDS[e]}: {len(high[e])} cases blame a position >= 256, e.g. {high[e][:2]}")
        assert len(high[e]) >= 6 and set(high[e]) & set(SPARSE) and set(high[e]) & set(SHUT_WIDE)
    # the steered families, by the source tables' bookkeeping: batch b is of family b mod F, so a wave of F or more batches holds them all
    steered = 0
    for c in new:
        src = kc.SOURCES[c.source].BY_NAME[c.source_name] if c.source else None
        if src is None or "steered" not in (getattr(src, "fault", None), getattr(src, "errors", None)) or c.policy != kc.CORRECT:
            continue
        steered += 1
        fams = ("point", "no_point", "node_one") if c.end == kc.LOCATE else dc.families(c.checks - len(c.erased))
        fin, B = kc.finish(c.name), kc.batches(c)
        waves = [range(w, min(w + WAVE, B)) for w in range(0, B, WAVE)]
        full = [w for w in waves if len(w) >= len(fams)]                      # all but a last wave of one lane
        assert len(full) >= 2 and B >= 4 * len(fams) and len(waves) - len(full) <= 1 and all({fams[b % len(fams)] for b in w} == set(fams) for w in full), c.name
        kinds = [{"decoded" if (isinstance(fin.verdicts[b], int) and fin.verdicts[b] > 0) or fin.verdicts[b] == "located" else "lost" for b in w} for w in full]
        assert all(k == {"decoded", "lost"} for k in kinds), c.name
        print(f"{c.name}: {len(fams)} families in each of {len(full)} waves, decoded and undecoded lanes side by side in each")
    assert steered == 8                                                   # 1 locating, 4 decoding (one with a lowered cap), 3 erasure cases
    # the erased positions the setup kernel compacts in its first step (positions below 256) and in its second
    both = [c.name for c in new if c.end == kc.ERASURES and c.ok == "flags" and {j // ec.STEP for j in c.erased} == {0, 1}]
    second = [c.name for c in new if c.end == kc.ERASURES and c.ok == "flags" and c.erased and {j // ec.STEP for j in c.erased} == {1}]
    print(f"erased positions in both steps: {len(both)} cases; in the second alone: {second}")
    assert len(both) >= 10 and "k3_wide-erasures-correct-d3298-sparse" in second and len(second) >= 3
    assert any(len(kc.BY_NAME[n].erased) > ec.KEPT for n in both)         # counted past the sixteen that are kept

"""What the case table of tests/unmask_checked_cases.py contains, proved on the CPU from its Python-integer model alone: every
combination sda_secret_unmasker_unmask_checked_jobs_dev treats differently is there BY NAME, the model is the composition of the
existing models, and each fault planted in the model is noticed - the test names the case that notices it first - so a green
tests/test_unmask_checked_gpu.py says something about each of them."""
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


@pytest.fixture(autouse=True)
def _the_entry_point_exists():
    """the table is about one entry point: without it in the ctypes table no statement below means anything"""
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
            "k3_62-erasures-correct-d764-word18-pass16"} == set(shut)
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

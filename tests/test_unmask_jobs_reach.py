"""What the case table of tests/unmask_jobs_cases.py contains, proved on the CPU from its Python-integer model alone: every class of
operand and of length that unmask_finish_kernel treats differently is there BY NAME, and a fault planted in the model is noticed by
a named case - so a green tests/test_unmask_jobs_gpu.py says something about each of them."""
import pytest

import chacha_repair as cr
import reconstruct_stream_cases as rc
import unmask_jobs_cases as uc



@pytest.fixture(autouse=True)
def _the_entry_point_exists():
    """the table is about one entry point: without it in the ctypes table no statement below means anything"""
    from sda_amd import capi
    assert "sda_secret_unmasker_unmask_jobs_dev" in capi.SIGNATURES


LANES = 256                                # sda_kernels.hip kThreads; a lane takes two elements
WORKGROUP = 2 * LANES


def _open(name):
    return not uc.gate_shut(uc.BY_NAME[name])


def test_the_table_is_what_the_issue_lists():
    names = set(uc.BY_NAME)
    for L in (1, 2, 3, 4, 5, 511, 512, 513, 1000, 6301):
        for off in (0, 8):
            assert f"k3_62-full-d{L}-off{off}" in names
    kinds = {c.masking for c in uc.CASES}
    assert kinds == {"full", "chacha", "none-null", "none-combiner"}
    assert {c.gates for c in uc.CASES} == {"null", "two", "equal", "closed-masks", "closed-results", "closed-equal"}
    assert {c.offset for c in uc.CASES} == {0, 8}
    pairs = {(rc.SCHEMES[c.scheme][0], c.q_mask) for c in uc.CASES if uc.has_mask(c)}
    assert {(uc.P62, uc.P62), (uc.P62, uc.Q61), (uc.P31, uc.P62)} <= pairs


@pytest.mark.parametrize("name", ["k3_62-full61-d1000", "k3_62-full61-crafted-d513", "additive-full61-crafted-d1000",
                                  "k3_62-chacha61-noseed-d4", "k3_62-chacha-rejecting-d8"])
def test_masked_values_at_or_above_the_masking_modulus(name):
    m, q = uc.model(name), uc.BY_NAME[name].q_mask
    n = sum(x >= q for x in m.masked)
    print(f"{name}: {n} of {len(m.masked)} masked values >= q_mask")
    assert n > 0 and _open(name)


@pytest.mark.parametrize("name", ["k3_62-full-d1000-off0", "k3_62-full61-d1000", "k3_62-chacha-d1000", "additive-crafted-d1000"])
def test_both_branches_of_the_subtraction(name):
    m, q = uc.model(name), uc.BY_NAME[name].q_mask
    ge = sum(x % q >= y for x, y in zip(m.masked, m.mask))
    print(f"{name}: masked >= mask in {ge} of {len(m.mask)} positions")
    assert 0 < ge < len(m.mask) and _open(name)


@pytest.mark.parametrize("name", ["additive-crafted-d1000", "additive-crafted-d5", "additive-full61-crafted-d1000"])
def test_negative_high_words_on_either_side(name):
    """a 128-bit sum below zero has a negative high word: the fold's negation branch, on the reconstructor's and on the mask's side"""
    m = uc.model(name)
    neg_r, neg_m = sum(s < 0 for s in m.recon_sums), sum(s < 0 for s in m.mask_sums)
    print(f"{name}: {neg_r} negative reconstructor sums, {neg_m} negative mask sums, of {len(m.recon_sums)}")
    assert neg_r > 0 and neg_m > 0 and _open(name)
    if len(m.recon_sums) >= 1000:                             # ... a high word below -1, and sums that are not negative, beside them
        assert any(s < -(1 << 64) for s in m.recon_sums) and any(s < -(1 << 64) for s in m.mask_sums)
        assert any(s >= 0 for s in m.recon_sums) and any(s >= 0 for s in m.mask_sums)


def test_a_packed_job_never_has_a_negative_sum():
    """the weighted sums are products of canonical values: the negative side is reached through Additive alone"""
    assert all(s >= 0 for s in uc.model("k3_62-full61-crafted-d513").recon_sums)


def test_every_length_class():
    by = uc.BY_NAME
    odd_tail = [c.name for c in uc.CASES if c.dim % 2 == 1 and _open(c.name)]
    lone = [c.name for c in uc.CASES if c.dim == 1 and _open(c.name)]
    misaligned = [c.name for c in uc.CASES if c.offset == 8 and c.dim >= 2 and _open(c.name)]
    padded = [c.name for c in uc.CASES if uc.accumulators(c) > c.dim and _open(c.name)]
    assert {"k3_62-full-d1-off0", "k3_62-full-d1-off8"} <= set(lone)
    assert {"k3_62-full-d3-off0", "k3_62-full-d513-off8", "k3_62-full-d6301-off0"} <= set(odd_tail)
    assert {"k3_62-full-d2-off8", "k3_62-full-d512-off8", "k3_62-full-d6301-off8", "pss155-full-d250"} <= set(misaligned)
    assert {"k3_62-full-d1-off0", "k3_62-full-d4-off0", "k3_62-full-d1000-off0", "k8_62-full-d805", "pss155-full-d250"} <= set(padded)
    assert uc.accumulators(by["k8_62-full-d805"]) - 805 == 3 and uc.accumulators(by["pss155-full-d250"]) - 250 == 50
    assert len(by["pss155-full-d250"].indices) == 255
    # exactly one workgroup of 256 lanes x 2 elements, one less (its last lane takes the odd tail), one more (a second workgroup of one
    # lane with one element)
    for off in (0, 8):
        assert by[f"k3_62-full-d{WORKGROUP - 1}-off{off}"].dim == WORKGROUP - 1
        assert by[f"k3_62-full-d{WORKGROUP}-off{off}"].dim == WORKGROUP
        assert by[f"k3_62-full-d{WORKGROUP + 1}-off{off}"].dim == WORKGROUP + 1
    assert -(-6301 // 2) > 12 * LANES                     # more than a dozen workgroups
    # an unpadded packed job and Additive (accumulators == L, an odd L: the pair load of the last lane would read past them)
    assert uc.accumulators(by["k3_62-full-d513-off0"]) == 513 and uc.accumulators(by["additive-crafted-d5"]) == 5


def test_the_chacha_jobs():
    noseed = uc.BY_NAME["k3_62-chacha-noseed-d1000"]
    assert uc.build(noseed.name).mask_rows.shape[0] == 0
    m = uc.model(noseed.name)
    assert all(s == 0 for s in m.mask_sums) and m.out == tuple(x % noseed.q_mask for x in m.masked) and m.out == m.masked
    m = uc.model("k3_62-chacha61-noseed-d4")                  # ... and under a smaller masking modulus the chain's canonical form
    assert m.out == tuple(x % uc.Q61 for x in m.masked)
    rej = uc.BY_NAME["k3_62-chacha-rejecting-d8"]
    seed, q, dim, pins = cr.SEEDS[rej.masks]
    assert (q, dim) == (rej.q_mask, rej.dim) and "shift_R2" in pins
    assert uc.chacha_rejections(list(seed), q, dim) == 2      # the repair moves masks: the sum read is a repaired one
    assert uc.chacha_masks(list(seed), q, dim) == list(cr.oracle_mask(seed, q, dim))      # the model's expansion is the C oracle's
    seeds = uc.build("k3_62-chacha-d1000").mask_rows
    assert seeds.shape == (5, 4)


def test_none_goes_with_and_without_a_combiner():
    for name in ("k3_62-none-null-d1000", "k3_62-none-combiner-d1000", "additive-none-combiner-d5"):
        m = uc.model(name)
        assert m.out == m.masked and m.mask == ()


NOTICED_BY = {
    "recon_under_mask_modulus": ["k3_62-full61-d1000", "k3_62-full61-crafted-d513", "additive-full61-crafted-d1000", "k3_31-full62-d1000",
                                 "k3_31-full62-d4", "k3_62-chacha-rejecting-d8"],
    "no_canonicalisation": ["k3_62-full61-d1000", "k3_62-full61-crafted-d513", "additive-full61-crafted-d1000", "k3_62-chacha61-noseed-d4"],
    "padding_stored": ["k3_62-full-d1-off0", "k3_62-full-d4-off8", "k3_62-full-d1000-off0", "k8_62-full-d805", "pss155-full-d250",
                       "k3_62-none-null-d1000", "k3_62-chacha-d1000"],
    "gate_ignored": ["k3_62-full-d1000-closed-masks", "k3_62-full-d513-closed-results", "additive-chacha-d5-closed-equal",
                     "k3_62-none-null-d4-closed-results"],
}


def test_every_fault_is_listed():
    assert set(NOTICED_BY) == set(uc.FAULTS)


@pytest.mark.parametrize("fault,name", [(f, n) for f, names in NOTICED_BY.items() for n in names])
def test_a_planted_fault_is_noticed(fault, name):
    good, bad = uc.model(name), uc.model(name, frozenset([fault]))
    differ = sum(x != y for x, y in zip(good.buffer, bad.buffer))
    print(f"{fault} / {name}: {differ} of {len(good.buffer)} buffer words differ")
    assert differ > 0


@pytest.mark.parametrize("name", [c.name for c in uc.CASES if uc.gate_shut(c)])
def test_a_shut_gate_leaves_the_sentinel(name):
    assert set(uc.model(name).buffer) == {uc.SENTINEL}


def test_the_model_is_the_formula_of_the_chain():
    """out = submod(canon_i64(mod_i128(recon sums, q_share), q_mask), mod_i128(mask sums, q_mask), q_mask), element by element"""
    for name in ("k3_62-full61-crafted-d513", "additive-crafted-d5", "k3_31-full62-d4"):
        c, m = uc.BY_NAME[name], uc.model(name)
        p, q = rc.SCHEMES[c.scheme][0], c.q_mask
        for i in range(c.dim):
            masked, mask = m.recon_sums[i] % p, m.mask_sums[i] % q
            x = masked % q
            assert m.out[i] == (x - mask if x >= mask else x + q - mask)
        head = c.offset // 8
        assert m.buffer[:head] == (uc.SENTINEL,) * head and m.buffer[head + c.dim:] == (uc.SENTINEL,) * uc.TAIL

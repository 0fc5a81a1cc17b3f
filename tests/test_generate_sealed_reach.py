"""What the case table of sda_share_generator_generate_sealed_rows_dev (tests/generate_sealed_cases.py) reaches, proved with
the oracle alone and by name: a table that stops reaching one of these fails here, not silently on the GPU.

One item of the list cannot be reached by ANY case and is asserted as such: a share is a canonical residue below 2^62, its
zig-zag image is below 2^63, so no share takes 10 varint bytes - lengths 1 to 9 are reached, length 10 is shown to be
impossible for this call (the 10-byte path of the encode loop stays covered by tests/test_participant_seal_gpu.py)."""
import numpy as np
import pytest

import drbg_retry as dr
import generate_sealed_cases as gs


def _case(name):
    return gs.BY_NAME[name]


def _streams(case):
    return [case["first"] + q for q in range(case["participants"])]


def _rejections(case):
    return dr.first_attempt(gs.KEY, _streams(case), gs.batches(case), case["t"], case["p"])[1]


def test_case_names_are_unique_and_small(built):
    assert len(gs.BY_NAME) == len(gs.CASES)
    for c in gs.CASES:
        assert gs.rows(c) <= 80 and gs.batches(c) <= 1701, c["name"]
        assert c["additive"] or c["k"] + c["t"] <= 32
        assert c["stride"] >= c["len"]


def test_batch_counts(built):
    want = {1, 2, 3, 7, 8, 9, 127, 128, 129, 257}
    assert want <= {gs.batches(c) for c in gs.CASES if c["name"].startswith("B")}


def test_a_rejected_main_candidate_in_every_retry_case(built):
    for name in ("retry-packed", "retry-additive", "retry-paired-even-t", "retry-paired-odd-t", "retry-second-attempt"):
        rej = _rejections(_case(name))
        assert rej.any(), name
    # one in five: every position of a quad's group of 8, every participant
    rej = _rejections(_case("retry-packed"))
    assert dr.covered(rej)
    rej = _rejections(_case("retry-additive"))
    assert rej.sum() >= 10 and rej[1:].any()


def test_a_second_retry_attempt(built):
    c = _case("retry-second-attempt")
    stream, b, i = next(d for d in dr.DEEP_CASES if d["name"] == "deep-additive")["hit"]
    assert c["first"] == stream and gs.batches(c) > b and (c["t"], c["p"]) == (2, dr.PM)
    assert dr.retry_depth(gs.KEY, stream, b, i, c["t"], c["p"])[0] >= 2


def test_located_rejected_pairs_under_the_paired_rule(built):
    for name, t_parity in (("retry-paired-even-t", 0), ("retry-paired-odd-t", 1)):
        c = _case(name)
        assert dr.paired(c["p"]) and c["t"] % 2 == t_parity
        rej = _rejections(c)
        assert rej.shape[2] == (c["t"] + 1) // 2 and rej.any(), name
        # the C oracle and the big-int oracle agree at the located draws
        from oracle import pyoracle as po
        q, b, j = (int(x) for x in np.argwhere(rej)[0])
        draws = gs.draws_of(c, q).reshape(gs.batches(c), c["t"])
        for i in (2 * j, 2 * j + 1):
            if i < c["t"]:
                assert int(draws[b, i]) == po.drbg_value(gs.KEY, c["first"] + q, b, c["t"], i, c["p"])


def test_both_draw_rules(built):
    rules = {dr.paired(c["p"]) for c in gs.CASES}
    assert rules == {True, False}
    paired_t = {c["t"] % 2 for c in gs.CASES if dr.paired(c["p"])}
    assert paired_t == {0, 1}


def test_a_zero_padded_batch_and_a_job_shorter_than_one_batch(built):
    assert any(c["len"] % c["k"] for c in gs.CASES if not c["additive"])
    assert any(c["len"] < c["k"] for c in gs.CASES)
    assert any(c["len"] % c["k"] == 0 for c in gs.CASES if not c["additive"])
    # every one of the batch-count cases pads its last batch
    assert all(c["len"] % c["k"] for c in gs.CASES if c["name"].startswith("B"))


def test_a_quad_partly_past_the_end_of_the_row(built):
    """lane l of a step holds batches 2 l, 2 l + 1: a quad (4 lanes, 8 batches) with some lanes past the end, and a lane whose
    second batch alone is past the end"""
    partly = [c["name"] for c in gs.CASES if 0 < (gs.batches(c) + 1) // 2 % 4]
    odd = [c["name"] for c in gs.CASES if gs.batches(c) % 2]
    assert {"B1", "B3", "B9"} <= set(partly) and {"B1", "B127", "B257"} <= set(odd)
    assert any(gs.batches(c) % 8 == 0 for c in gs.CASES)                  # ... and a row that ends with a whole quad


def test_each_step_boundary(built):
    steps = {(gs.batches(c) + gs.STEP - 1) // gs.STEP for c in gs.CASES}
    assert {1, 2, 3} <= steps
    for B in (127, 128, 129, 257):                                          # last value of a step, first of the next
        assert any(gs.batches(c) == B for c in gs.CASES)


def test_each_keystream_refill(built):
    once = gs.payloads_of(_case("refill-once"), 1)
    twice = gs.payloads_of(_case("refill-twice"), 1)
    assert all(gs.REFILLS[0] < len(m) < gs.REFILLS[1] for m in once if len(m) > 1000)
    assert sum(len(m) > gs.REFILLS[0] for m in once) >= 35                 # the 7 clerks x 5 participants of 9-byte shares
    assert any(len(m) > gs.REFILLS[1] for m in twice)
    assert gs.batches(_case("refill-once")) >= 460 and gs.batches(_case("refill-twice")) >= 920


def test_every_varint_length_a_share_can_have(built):
    from oracle import coracle
    seen = set()
    for c in gs.CASES:
        sh = gs.shares_of(c, gs.share_maps(c)[0])
        assert sh.min() >= 0 and sh.max() < c["p"] < 1 << 62                # canonical: zig-zag(v) = 2 v < 2^63
        zz = sh.astype(np.uint64) << np.uint64(1)
        for w in range(1, 11):
            lo, hi = (1 << (7 * (w - 1))) if w > 1 else 0, 1 << min(7 * w, 64)
            if ((zz >= np.uint64(lo)) & ((zz < np.uint64(hi)) if hi < 1 << 64 else True)).any():
                seen.add(w)
    assert seen == set(range(1, 10)), seen
    # length 10 needs zig-zag(v) >= 2^63, i.e. v >= 2^62 or v < 0: no canonical share
    assert len(coracle.varint_encode(np.array([(1 << 62) - 1], dtype=np.int64))) == 9


def test_secrets_layouts_and_participants(built):
    assert {c["participants"] for c in gs.CASES} >= {1, 5}
    assert any(c["first"] > 1 << 32 for c in gs.CASES) and any(0 < c["first"] < 1 << 32 for c in gs.CASES)
    anyc = [c for c in gs.CASES if c["secrets"] == "any"]
    assert anyc and all(gs.secrets_of(c).min() == gs.I64_MIN and gs.secrets_of(c).max() == gs.I64_MAX for c in anyc)
    assert any(c["stride"] > c["len"] for c in gs.CASES) and any(c["offset"] % 2 for c in gs.CASES)
    assert any((c["stride"] % 2 or c["offset"] % 2) and c["participants"] > 1 for c in gs.CASES)
    assert any(c["small_order"] is not None for c in gs.CASES)


def test_schemes(built):
    shapes = {(c["k"], c["t"], c["n"], c["p"]) for c in gs.CASES if not c["additive"]}
    assert {(3, 1, 8, gs.P62), (8, 2, 26, gs.P62), (3, 4, 8, gs.P31)} <= shapes
    assert any(c["k"] + c["t"] == 32 for c in gs.CASES if not c["additive"])
    assert {c["n"] for c in gs.CASES if c["additive"]} >= {2, 3}
    assert (1 << 30) < gs.P31 < (1 << 31) and dr.is_prime(gs.P31) and dr.is_prime(gs.P_PAIRED)

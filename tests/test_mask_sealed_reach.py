"""CPU proof, from the reference alone, of what the cases of tests/mask_sealed_cases.py reach in mask_seal_stream_kernel and in the
ChaCha driver behind sda_secret_masker_mask_sealed_rows_dev: the keystream refills, the 8-byte accesses, the CSPRNG's retry
stream, every varint length a canonical mask can have, and the repair plan of every ChaCha case."""
import numpy as np
import pytest

import drbg_retry as dr
import mask_combiner_cases as mc
import mask_sealed_cases as ms


def _full(name):
    return ms.BY_NAME[name]


def test_the_table_holds_the_cases_it_was_given():
    shapes = {(c["q"], c["participants"], c["len"]) for c in ms.FULL_CASES}
    for want in [(ms.P62, 1, 1), (ms.P62, 3, 129), (ms.P62, 2, 460), (ms.P62, 1, 1000), (433, 5, 700), (ms.P_PAIRED, 4, 300),
                 (ms.P31, 2, 257), (ms.PM, 3, 2000), (ms.P62, 3, 40), (ms.P62, 70, 40), (ms.P62, 2, 200)]:
        assert want in shapes, want
    assert _full("pm-3x2000")["first"] == dr.FIRST and _full("last-streams-3x40")["first"] + 3 == 1 << 56
    assert _full("3x129-in-place")["in_place"] and _full("small-order-2x200")["small_order"]
    assert dr.paired(ms.P_PAIRED) and dr.paired(433) and not dr.paired(ms.P31) and not dr.paired(ms.P62) and not dr.paired(ms.PM)
    chacha = {(c["q"], c["len"], c["participants"], c["bits"]) for c in ms.CHACHA_CASES}
    for shape in [(433, 1000, 5), (ms.P62, 4099, 9), (mc.Q_HEAVY, 3000, 6), mc.BOTH_LISTS]:
        assert shape in mc.CHACHA_SHAPES
        assert {shape + (128,), shape + (256,)} <= chacha
    assert any(c["bits"] == 288 and c["words"] == 9 for c in ms.CHACHA_CASES)
    assert any(c["small_order"] for c in ms.CHACHA_CASES)


def test_which_full_cases_cross_each_keystream_refill():
    """the tile holds message bytes below 4064, then 4096 more: a row longer than an edge makes the wave refill there"""
    longest = {c["name"]: max(len(p) for p in ms.payloads_of(c)) for c in ms.FULL_CASES}
    shortest = {c["name"]: min(len(p) for p in ms.payloads_of(c)) for c in ms.FULL_CASES}
    first, second = ms.REFILLS
    once = [n for n in longest if first < shortest[n] and longest[n] <= second]
    twice = [n for n in longest if shortest[n] > second]
    print("payload bytes:", {n: (shortest[n], longest[n]) for n in longest})
    assert "2x460" in once, "no case crosses the first refill only"
    assert "1x1000" in twice and "pm-3x2000" in twice, "no case crosses the second refill"
    assert longest["1x1"] <= 9 and longest["3x129-misaligned"] < first


def test_the_misaligned_case_takes_the_8_byte_accesses_and_the_odd_tail():
    """device allocations are 16-byte aligned, so row p of a buffer lies on the 16-byte grid iff offset + p * stride is even; the
    kernel takes 16-byte accesses only where both rows do.  An odd length leaves one element to the 8-byte tail either way."""
    c = _full("3x129-misaligned")
    assert c["len"] % 2 == 1 and c["len"] > ms.STEP and c["len"] - ms.STEP == 1        # a second step of one value
    vec = [(c["offset"] + p * c["s_stride"]) % 2 == 0 and (c["offset"] + p * c["m_stride"]) % 2 == 0 for p in range(c["participants"])]
    assert vec == [False, True, False], "rows on both paths"
    assert c["m_stride"] == 131 and c["offset"] == 1
    a = _full("3x129-in-place")                                          # aligned rows with an odd tail
    assert a["len"] % 2 == 1 and a["s_stride"] == a["m_stride"] and a["offset"] == 0 and a["s_stride"] % 2 == 1
    assert _full("1x1")["len"] == 1


def test_every_row_of_the_retry_case_holds_a_rejected_candidate():
    c = _full("pm-3x2000")
    _, rej = dr.first_attempt(ms.KEY, [c["first"] + p for p in range(c["participants"])], c["len"], 1, c["q"])
    per_row = rej.reshape(c["participants"], -1).sum(axis=1)
    print("rejected first attempts per row:", per_row)
    assert (per_row > 0).all()
    assert rej[:, -8:].any() or rej[:, :8].any()
    # ... and the masks the reference draws differ from the first-attempt values exactly there
    x, _ = dr.first_attempt(ms.KEY, [c["first"]], c["len"], 1, c["q"])
    naive = np.array([(int(v) * c["q"]) >> 64 for v in x[0, :, 0]], dtype=np.int64)
    assert np.array_equal(naive != ms.masks_of(c)[0], rej[0, :, 0])


def _varint_len(v):
    zz = (int(v) << 1) ^ (int(v) >> 63)
    return max(1, (zz.bit_length() + 6) // 7)


def test_value_lengths_one_to_nine_occur_and_ten_is_out_of_reach():
    from oracle import coracle
    seen = set()
    for c in ms.FULL_CASES:
        M = ms.masks_of(c)
        assert ((M >= 0) & (M < c["q"])).all(), c["name"]
        seen |= {int(x) for x in np.unique([_varint_len(v) for v in M.ravel()])}
    print("varint lengths among the masks of the Full cases:", sorted(seen))
    assert seen == set(range(1, 10))
    # a canonical mask is below 2^62 (the library admits no larger modulus): its zig-zag value is below 2^63 = nine groups of 7 bits
    top = (1 << 62) - 1
    assert _varint_len(top) == 9 and len(coracle.varint_encode(np.array([top], dtype=np.int64))) == 9
    assert len(coracle.varint_encode(np.array([-1 << 63], dtype=np.int64))) == 10      # only a value no mask can take needs ten
    for v in (0, 63, 64, 8191, 8192, top):
        assert _varint_len(v) == len(coracle.varint_encode(np.array([v], dtype=np.int64)))


@pytest.mark.parametrize("name", [c["name"] for c in ms.CHACHA_CASES])
def test_each_chacha_case_takes_the_plan_its_table_names(name):
    c = ms.BY_NAME[name]
    S = ms.seeds_of(c)
    assert S.shape == (c["participants"], c["words"]) and ((S >= 0) & (S < 1 << 32)).all()
    count, _ = mc.rejections(S, c["q"], c["len"])
    exact_for_all = mc.all_exact_order(c["q"], c["len"])
    print(name, "rejected among the first", c["len"], "candidates per seed:", np.bincount(np.minimum(count, 4), minlength=5))
    if c["plan"] == "all-exact":
        assert exact_for_all and (count > 0).all()
    elif c["plan"] == "clean":
        assert not exact_for_all and (count == 0).all()
    else:
        assert c["plan"] == "both-lists" and not exact_for_all
        assert (count == 0).any() and ((count >= 1) & (count <= 3)).any() and (count > 3).any()
    if c["words"] > 8:                                                   # the ninth word is sealed and sent, never expanded
        from oracle import coracle
        assert np.array_equal(coracle.chacha_expand(S[0], c["q"], 16), coracle.chacha_expand(S[0][:8], c["q"], 16))
        assert S[:, 8].any()

"""The sealed-box kernels' limb arithmetic in Python integers, in the DEVICE's order, with every register width asserted
(tests/sbox_model.py restates sbox_primitives.hpp and the lane / step / region order of sealedbox_kernels.hip).  Two kinds of
check: (1) the model's result equals a plain big-int reference (Poly1305 written below in five lines; the oracle's X25519) on
random and on crafted inputs, none of which may trip a width assertion; (2) the worst case of each stage is DERIVED by
interval arithmetic over the same steps - largest limb in, largest limb out - so that no assertion rests on having found the
worst input.

Poly1305 (radix 2^26), stage by stage: proven bound | reached by the crafted inputs here
  p26_from_piece      limbs 0..3 <= 2^26 - 1, limb 4 <= 2^25 - 1                  | both (all-0xFF piece)
  p26_mul operands    a_i <= 2^27 + 127, b_i <= 2^26 + 127 (the contract)         | a_i = 2^27 - 1, b_i = 2^26 - 1
  p26_mul  5 b_i      <= 5 (2^26 + 127) < 2^28.4 (uint32_t)                       | -
  p26_mul columns     <= 21 a b < 2^57.4 (uint64_t)                               | 2^56.9 (r = all clamped bits, 0xFF message)
  p26_mul result      limbs 0,2,3,4 <= 2^26 - 1, limb 1 <= 2^26 + 51              | limb 1 = 2^26 (r = 1)
  p26_carry of it     every limb <= 2^26 - 1 (case split on limb 1 >= 2^26)       | 2^26 - 1 in all five limbs of all 64 lanes
  64-lane sum         <= 64 (2^26 - 1) = 2^32 - 64 (uint32_t)                     | 2^32 - 64 exactly, all five limbs
  p26_carry of sums   limb + carry <= 2^32 - 64 + 63 = 2^32 - 1 (uint32_t)        | 2^32 - 1 exactly: margin ZERO
                      result limb 1 <= 2^26 (not < 2^26)                          | 2^26 exactly
  region Horner       acc_i <= (2^26 + 51) + 2^26 <= the p26_mul contract         | 2^27 - 1
  p26_finish          two carries -> h < 2^130; take_g iff h >= 2^130 - 5;        | h = p - 1, p, 2^130 - 1 and both verdicts,
                      h + s carries through all four words                        | carries in every word (s = 2^128 - 1)
No uint32_t or uint64_t wrap is reachable; the margin of the lane sums is exactly zero and rests on the case split above
(after p26_mul the wrap carry of p26_carry is 1 only if limb 1 overflowed, whose masked value is then <= 51).

GF(2^255 - 19) (radix 2^25.5): proven bound | largest seen over the whole ladders below
  fe_carry result     h_i in [-2^25, 2^25) even i, [-2^24, 2^24) odd i, |h_1| <= 2^24 + 1, for |columns| < 2^62
  fe_mul operands     ladder: <= 2^26 even / 2^25 + 2 odd (two carried elements)  | 2^26 - 1 even, 2^25 - 1 odd
                      contract: |g_i| <= 113,025,455 = (2^31 - 1) / 19 (19 g_i in int32_t); 2^27 does NOT fit
  fe_mul columns      < 2^61.6 at the contract, < 2^59.3 in the ladder (int64_t)  | 2^59.0
"""
import math
import random

import pytest

import sbox_model as S
from oracle import sealedbox_oracle as so

M26 = S.M26


def poly1305_plain(key, msg):
    """RFC 8439 section 2.5 on Python integers - the reference of this file"""
    r, s, h = int.from_bytes(key[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF, int.from_bytes(key[16:], "little"), 0
    for i in range(0, len(msg), 16):
        h = (h + int.from_bytes(msg[i:i + 16] + b"\x01", "little")) * r % (2**130 - 5)
    return ((h + s) % 2**128).to_bytes(16, "little")


def _agree(key, msg, stats=None, regions=None):
    tag = S.poly1305_device_order(key, msg, regions=regions, stats=stats)
    assert tag == poly1305_plain(key, msg) == so.poly1305(key, msg), (key.hex(), len(msg))
    return tag


def test_poly1305_device_order_equals_the_plain_form_on_random_inputs():
    rng = random.Random(130)
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, 16 * 1024 - 1, 16 * 1024, 16 * 1024 + 1, 2 * 16384 - 1, 2 * 16384 + 16, 3 * 16384 + 1, 40000):
        _agree(rb(32), rb(n))
    # `used` regions of `regions`: a short row in a launch sized for a long one reads only its own partial sums
    for n in (0, 5, 16384, 16385):
        _agree(rb(32), rb(n), regions=4)


@pytest.mark.parametrize("s16", [bytes(16), b"\xff" * 16])
def test_poly1305_crafted_inputs_reach_the_bounds(s16):
    """r = 1: a lane's value is the plain sum of its pieces, so limb_extreme_message() sets the limbs that enter the 64-lane
    sum; r = 0, r with all clamped bits, all-0xFF / all-0x00 messages, tails of 1 .. 15 bytes"""
    st = {}
    sizes = {"one lane": 48, "64 lanes": 3072, "one region": 16384, "three regions and a ragged head": 3 * 16384 + 5000 + 7}
    for name, n in sizes.items():
        one = {}
        _agree(S.KEY_R1(s16), S.limb_extreme_message(n), one)
        for k, v in one.items():
            S.note(st, k, v)
        if name != "one lane":
            # every lane hands 2^26 - 1 in every limb to the sum; the sums and the carry behind them sit ON their bounds
            assert one["lane_out"] == M26 and one["lane_sum"] == 64 * M26 == 2**32 - 64, (name, one)
            assert one["carry_presum"] == 2**32 - 1 and one["carry_out1"] == 2**26, (name, one)
    for tail in range(1, 16):
        for body in (0, 3072, 16384):
            _agree(S.KEY_R1(s16), S.limb_extreme_message(body + tail), st)
            _agree(S.KEY_RMAX(s16), b"\xff" * (body + tail), st)
    for key in (bytes(16) + s16, S.KEY_R1(s16), (2).to_bytes(16, "little") + s16, S.KEY_RMAX(s16)):
        for fill in (b"\xff", b"\x00"):
            for n in (16, 1024, 16384 + 16, 40000):
                _agree(key, fill * n, st)
    assert st["mul_a"] >= 2**27 - 1 and st["mul_b"] == M26 and st["mul_out1"] >= 2**26
    assert st["mul_col"] >= 2**56                                   # of the 2^57.4 proven below


def test_poly1305_finish_edges_through_the_whole_device_order():
    """h = p - 1, p, p + 4 = 2^130 - 1 before the final reduction (r = 1: h is the plain sum of the pieces), with s = 0,
    2^128 - 1 and an s that makes h + s carry through all four words"""
    p = 2**130 - 5
    st = {}
    for target in (p - 1, p, p + 1, p + 4, 4, 5):
        # three pieces summing to `target`: 2^128 + m1, 2^128 + m2, 2^128 + m3 (r = 1)
        rest = target - 3 * 2**128
        if rest < 0:
            rest += p
        m1 = min(rest, 2**128 - 1); m2 = min(rest - m1, 2**128 - 1); m3 = rest - m1 - m2
        assert 0 <= m3 < 2**128
        msg = b"".join(m.to_bytes(16, "little") for m in (m1, m2, m3))
        h = sum(int.from_bytes(msg[i:i + 16] + b"\x01", "little") for i in (0, 16, 32))
        assert h % p == target % p
        for s in (0, 2**128 - 1, 2**128 - (h % p), 2**128 - 1 - (h % p), 1 << 127):
            _agree(S.KEY_R1((s % 2**128).to_bytes(16, "little")), msg, st)
    assert st["finish_take_g"] == 1 and st["finish_take_h"] == 1            # both verdicts of the final select
    assert all(st["finish_word_carry_%d" % i] == 1 for i in range(4))


def test_p26_finish_raw_limbs():
    p = 2**130 - 5
    spell = lambda v: [(v >> (26 * i)) & M26 for i in range(5)]
    for v in (0, 1, 4, 5, p - 1, p, p + 1, p + 4):
        for s in (0, 2**128 - 1, (2**128 - (v % p)) % 2**128, 2**127 + 12345):
            h = spell(v)
            for limbs in (h, [h[0], h[1] + 2**26, h[2] - 1, h[3], h[4]] if h[2] else h):      # minimal; excess in limb 1
                tag = S.p26_finish(limbs, s.to_bytes(16, "little"))
                assert int.from_bytes(tag, "little") == (v % p + s) % 2**128, (v, s, limbs)


def test_poly1305_interval_proof_of_every_stage():
    """largest limb in -> largest limb out, stage by stage; the bounds close over themselves (an inductive invariant), so they
    hold for every key and message, not only for the inputs above"""
    A, B = [S.MUL_A_MAX] * 5, [S.MUL_B_MAX] * 5
    prod, cols = S.p26_mul_interval(A, B)                            # asserts 5 b_i in uint32_t and the 64-bit carries
    assert prod == [M26, M26 + 51, M26, M26, M26] and prod[1] <= S.MUL_OUT1_MAX and cols < 2**57.4 < 2**64
    piece = [M26, M26, M26, M26, 2**25 - 1]
    clamped_r = S.p26_clamped_r(b"\xff" * 16)
    assert all(x <= S.MUL_B_MAX for x in clamped_r)                  # r itself
    assert all(x <= S.MUL_B_MAX for x in prod)                       # every power of r is a product: a valid b
    assert all(x + y <= S.MUL_A_MAX for x, y in zip(prod, piece))    # h r^64 + c: a valid a
    # the lane's last p26_carry, applied to a product: split on whether limb 1 overflows
    lo = S.p26_carry_interval([(0, M26)] * 5)                        # limb 1 <= 2^26 - 1: no carry anywhere
    hi = S.p26_carry_interval([(0, M26), (2**26, prod[1]), (0, M26), (0, M26), (0, M26)])
    assert max(x[1] for x in lo) == M26 and lo[1] == (0, M26)
    assert hi[1][1] <= 51 + 1 and max(x[1] for x in hi) == M26       # masked limb 1 <= 51, + the wrap carry
    lane_sum = 64 * M26
    assert lane_sum == S.CARRY_IN_MAX == 2**32 - 64
    # sbox_final_kernel: p26_carry of the raw sums (asserts limb + carry in uint32_t: 2^32 - 64 + 63), then acc = t + p
    p = S.p26_carry_interval([(0, lane_sum)] * 5)
    assert [x[1] for x in p] == [M26, M26 + 1, M26, M26, M26]
    assert all(x + y[1] <= S.MUL_A_MAX for x, y in zip(prod, p))     # acc: a valid a for the next p26_mul and for p26_finish
    # one unit more in the lane sums would wrap: the margin is zero
    with pytest.raises(AssertionError):
        S.p26_carry_interval([(0, lane_sum + 1)] * 5)
    # p26_finish: acc -> first carry -> second carry (split on limb 1 = 2^26) -> below 2^130
    first = S.p26_carry_interval([(0, S.MUL_A_MAX)] * 5)
    assert [x[1] for x in first] == [M26, M26 + 1, M26, M26, M26]
    second_lo = S.p26_carry_interval([(0, M26)] * 5)
    second_hi = S.p26_carry_interval([(0, M26), (2**26, 2**26), (0, M26), (0, M26), (0, M26)])
    assert max(x[1] for x in second_lo + second_hi) == M26


def test_p26_carry_documented_counterexamples():
    """limb 1 = 2^26 after p26_carry in general, and the wrap one unit above the kernel's worst case"""
    assert S.p26_carry([2**26 - 5, M26, M26, M26, 2**26])[1] == 2**26
    assert S.p26_carry([64 * M26] * 5)[1] == 2**26
    with pytest.raises(AssertionError):
        S.p26_carry([64 * M26, 2**32 - 1, 0, 0, 0])


# ---- GF(2^255 - 19) --------------------------------------------------------------------------------------------------
def test_field_interval_proof_and_the_contract_of_fe_mul():
    carried = S.FE_CARRIED
    operand = [2 * x for x in carried]                               # a sum or difference of two carried elements
    assert operand[0] == 2**26 and operand[1] == 2**25 + 2 and operand[3] == 2**25
    cols = S.fe_mul_interval(operand, operand)                       # asserts 19 g_i, 2 f_i in int32_t, columns in int64_t
    assert max(cols) < 2**59.3
    assert S.fe_carry_interval(cols) == carried                      # ... and what comes out is carried again: closed
    assert all(S.i32(4 * x) for x in operand[1::2])                  # fe_sq's 4 f_i (odd limbs)
    # the widest operands fe_mul can take: 19 g_i in int32_t
    top = [S.FE_G_MAX] * 10
    cols = S.fe_mul_interval(top, top)
    assert max(cols) < 2**61.6 and S.fe_carry_interval(cols) == carried
    with pytest.raises(AssertionError):
        S.fe_mul_interval(top, [S.FE_G_MAX + 1] * 10)
    with pytest.raises(AssertionError):                              # the 2^27 the header used to state does not fit
        S.fe_mul_interval([2**27 - 1] * 10, [2**27 - 1] * 10)
    # fe_mul_a24 (one-lane form) and fe_carry's own limit
    assert S.fe_carry_interval([121665 * x for x in operand]) == carried
    assert S.fe_carry_interval([2**62] * 10) == carried


def test_field_primitives_on_edge_operands():
    rng = random.Random(25519)
    p = S.P25519
    ops = []
    for sign in ((1,) * 10, (-1,) * 10, (1, -1) * 5, (-1, 1) * 5):
        ops.append([s * 2 * c for s, c in zip(sign, S.FE_CARRIED)])
        ops.append([s * S.FE_G_MAX for s in sign])
    for i in range(10):
        ops.append([(2 * S.FE_CARRIED[j] if j == i else rng.randrange(-5, 6)) for j in range(10)])
        ops.append([(-S.FE_G_MAX if j == i else 0) for j in range(10)])
    ops += [[rng.randrange(-2**26, 2**26) for _ in range(10)] for _ in range(20)]
    for f in ops:
        S.fe_sq(f)                                                   # asserts widths, carried ranges and the value
        for g in ops[:12] + ops[-4:]:
            out = S.fe_mul(f, g)                                     # asserts widths, carried ranges and the value
            assert int.from_bytes(S.fe_to_bytes(out), "little") == S.fe_value(f) * S.fe_value(g) % p
    for v in (0, 1, 18, 19, p - 1, p, p + 1, 2**255 - 1, 2**255 - 20):
        assert S.fe_value(S.fe_from_bytes(v.to_bytes(32, "little"))) == v
        assert S.fe_value(S.fe_from_bytes((v | 1 << 255).to_bytes(32, "little"))) == v          # bit 255 dropped
        assert int.from_bytes(S.fe_to_bytes(S.fe_carry(S.fe_from_bytes(v.to_bytes(32, "little")))), "little") == v % p


def test_one_ladder_step_in_both_forms():
    """the one-lane schedule (fe_sq, fe_mul_a24) and the quad's three levels of fe_mul give the same point"""
    rng = random.Random(7)
    p = S.P25519
    for _ in range(6):
        x1 = S.fe_from_bytes(rng.getrandbits(255).to_bytes(32, "little"))
        state = [S.fe_carry([rng.randrange(-2**60, 2**60) for _ in range(10)]) for _ in range(4)]
        a, b = S.ladder_step_lane(x1, *state), S.ladder_step_quad(x1, *state)
        assert [S.fe_value(x) % p for x in a] == [S.fe_value(x) % p for x in b]
        x2, z2, x3, z3 = (S.fe_value(x) % p for x in state)
        A, B, C, D = x2 + z2, x2 - z2, x3 + z3, x3 - z3
        E = A * A - B * B
        want = (A * A * B * B % p, E * (A * A + 121665 * E) % p, (D * A + C * B) ** 2 % p, S.fe_value(x1) * (D * A - C * B) ** 2 % p)
        assert tuple(S.fe_value(x) % p for x in a) == want


def test_whole_ladders_on_the_edge_operands_and_the_operand_maxima():
    """every edge u-coordinate of tests/test_sealedbox_extremes_gpu.py through the quad schedule (a few through the one-lane
    form too), every edge scalar on the base point: equal to the oracle, no width assertion trips, and the per-call operand
    maxima stay inside what the interval proof allows - the real contract of fe_mul, not 2^27"""
    st = {}
    k = bytes(range(100, 132))
    pts = S.edge_points()
    for name, u in pts.items():
        assert S.x25519_model(k, u, True, st) == so.x25519(k, u), name
    for name in ("9", "p+2", "p-2", "limb9_saturated", "2^128-1", "9+2^255"):
        assert S.x25519_model(k, pts[name], False, st) == so.x25519(k, pts[name]), name
    for name, sk in S.edge_scalars().items():
        assert S.x25519_model(sk, so.BASEPOINT, True, st) == so.x25519_base(sk), name
    for u in (0, 1, S.P25519 - 1, S.P25519, S.P25519 + 1):          # small order: all-zero out, through fe_to_words' q
        assert S.x25519_model(k, u.to_bytes(32, "little"), True, st) == bytes(32)
    assert st["fe_mul_operand"] <= 2**26 and st["fe_mul_operand_odd"] <= 2**25 + 2 and st["fe_sq_operand"] <= 2**26
    assert st["fe_mul_operand"] >= 2**26 - 2**20 and st["fe_mul_operand_odd"] >= 2**25 - 2**19       # the ladders come this close
    assert st["fe_col"] < 2**59.3
    print("operand maxima", st["fe_mul_operand"], st["fe_mul_operand_odd"], "columns 2^%.2f" % math.log2(st["fe_col"]))

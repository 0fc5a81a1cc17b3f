"""Width-checked Python-integer model of sda_amd/csrc/sbox_primitives.hpp and of the order in which
sda_amd/csrc/sealedbox_kernels.hip evaluates Poly1305 and X25519 (tests/test_sbox_model.py runs it; the crafted messages are
shared with tests/test_sealedbox_extremes_gpu.py).  Every function restates one function of the header line by line; every
value that lives in a uint32_t / int32_t / uint64_t / int64_t there passes through u32 / i32 / u64 / i64 here, which assert
the width, and every range a comment of the header states is asserted where it is stated.  `stats` dictionaries keep the
largest value seen per stage."""
M26 = (1 << 26) - 1
P1305 = (1 << 130) - 5
P25519 = (1 << 255) - 19
POLY_STEPS, LANES = 16, 64
REGION_PIECES = POLY_STEPS * LANES

# the operand contract of p26_mul (header comment) and the bounds the interval proof of tests/test_sbox_model.py closes over
MUL_A_MAX = (1 << 27) + 127          # limbs of a: a product plus a piece / plus carried lane sums
MUL_B_MAX = (1 << 26) + 127          # limbs of b: a product (a power of r)
MUL_OUT1_MAX = (1 << 26) + 63        # limb 1 of a product; limbs 0, 2, 3, 4 <= M26
CARRY_IN_MAX = (1 << 32) - 64        # limbs 1 .. 4 into p26_carry
FE_G_MAX = ((1 << 31) - 1) // 19     # |g_i| of fe_mul: 19 g_i in int32_t
FE_CARRIED = [(1 << 25) if i % 2 == 0 else (1 << 24) for i in range(10)]
FE_CARRIED[1] += 1                   # limb 1 takes the last carry


def u32(x, what="uint32_t"):
    assert 0 <= x < 1 << 32, (what, x)
    return x


def u64(x, what="uint64_t"):
    assert 0 <= x < 1 << 64, (what, x)
    return x


def i32(x, what="int32_t"):
    assert -(1 << 31) <= x < 1 << 31, (what, x)
    return x


def i64(x, what="int64_t"):
    assert -(1 << 63) <= x < 1 << 63, (what, x)
    return x


def note(stats, key, value):
    if stats is not None and value > stats.get(key, -1):
        stats[key] = value


# ================================================================================================================
# Poly1305, five 26-bit limbs
# ================================================================================================================
def p26_from_piece(piece: bytes):
    """`piece`: the 1 .. 16 bytes of the piece; the pad bit goes to 2^(8 len)"""
    nbytes = len(piece)
    w = [int.from_bytes(piece[4 * i:4 * i + 4].ljust(4, b"\0"), "little") for i in range(4)]
    t = w + [0]
    if nbytes < 16:
        t[nbytes >> 2] |= 1 << (8 * (nbytes & 3))
    else:
        t[4] = 1
    h = [t[0] & M26, ((t[0] >> 26) | (t[1] << 6)) & M26, ((t[1] >> 20) | (t[2] << 12)) & M26, ((t[2] >> 14) | (t[3] << 18)) & M26,
         u32((t[3] >> 8) | (t[4] << 24))]
    assert p26_value(h) == int.from_bytes(piece, "little") + (1 << (8 * nbytes))
    assert all(x <= M26 for x in h[:4]) and h[4] < 1 << 25
    return h


def p26_clamped_r(k16: bytes):
    k = [int.from_bytes(k16[4 * i:4 * i + 4], "little") for i in range(4)]
    t0, t1, t2, t3 = k[0] & 0x0FFFFFFF, k[1] & 0x0FFFFFFC, k[2] & 0x0FFFFFFC, k[3] & 0x0FFFFFFC
    return [t0 & M26, ((t0 >> 26) | (t1 << 6)) & M26, ((t1 >> 20) | (t2 << 12)) & M26, ((t2 >> 14) | (t3 << 18)) & M26, t3 >> 8]


def p26_value(h):
    return sum(x << (26 * i) for i, x in enumerate(h))


def p26_mul(a, b, stats=None):
    for x in a:
        assert u32(x) <= MUL_A_MAX, ("p26_mul a", x)
    for x in b:
        assert u32(x) <= MUL_B_MAX, ("p26_mul b", x)
    note(stats, "mul_a", max(a)); note(stats, "mul_b", max(b))
    s = [None] + [u32(b[i] * 5, "5 b_i") for i in range(1, 5)]
    d = [a[0] * b[0] + a[1] * s[4] + a[2] * s[3] + a[3] * s[2] + a[4] * s[1],
         a[0] * b[1] + a[1] * b[0] + a[2] * s[4] + a[3] * s[3] + a[4] * s[2],
         a[0] * b[2] + a[1] * b[1] + a[2] * b[0] + a[3] * s[4] + a[4] * s[3],
         a[0] * b[3] + a[1] * b[2] + a[2] * b[1] + a[3] * b[0] + a[4] * s[4],
         a[0] * b[4] + a[1] * b[3] + a[2] * b[2] + a[3] * b[1] + a[4] * b[0]]
    for x in d:
        u64(x, "p26_mul column"); note(stats, "mul_col", x)
    for i in range(4):
        c = d[i] >> 26; d[i] &= M26; d[i + 1] = u64(d[i + 1] + c)
    c = d[4] >> 26; d[4] &= M26; d[0] = u64(d[0] + c * 5)
    c = d[0] >> 26; d[0] &= M26; d[1] = u64(d[1] + c)
    out = [u32(x) for x in d]
    assert out[1] <= MUL_OUT1_MAX and all(out[i] <= M26 for i in (0, 2, 3, 4)), out
    note(stats, "mul_out1", out[1])
    assert p26_value(out) % P1305 == p26_value(a) * p26_value(b) % P1305
    return out


def p26_add(a, b):
    return [u32(x + y, "p26_add") for x, y in zip(a, b)]


def p26_carry(h, stats=None, after_mul=False):
    h = list(h)
    for x in h[1:]:
        assert u32(x) <= CARRY_IN_MAX, ("p26_carry in", x)
    u32(h[0])
    before = p26_value(h)
    for i in range(4):
        c = h[i] >> 26; h[i] &= M26
        note(stats, "carry_presum", h[i + 1] + c)
        h[i + 1] = u32(h[i + 1] + c, "p26_carry: limb + carry")
    c = h[4] >> 26; h[4] &= M26; h[0] = u32(h[0] + c * 5)
    c = h[0] >> 26; h[0] &= M26; h[1] = u32(h[1] + c)
    assert all(h[i] <= M26 for i in (0, 2, 3, 4)) and h[1] <= M26 + 1, h
    if after_mul:
        assert h[1] <= M26, h           # the claim the 64-lane sum rests on
    note(stats, "carry_out1", h[1])
    assert p26_value(h) % P1305 == before % P1305
    return h


def p26_finish(hin, s16: bytes, stats=None):
    s = [int.from_bytes(s16[4 * i:4 * i + 4], "little") for i in range(4)]
    h = p26_carry(p26_carry(hin, stats), stats)
    assert all(x <= M26 for x in h), h             # after two carries: a number below 2^130
    g = [0] * 5
    g[0] = u32(h[0] + 5); c = g[0] >> 26; g[0] &= M26
    for i in (1, 2, 3):
        g[i] = u32(h[i] + c); c = g[i] >> 26; g[i] &= M26
    g[4] = (h[4] + c - (1 << 26)) % (1 << 32)      # wraps when h < p: that is the sign the next line reads
    take_g = ((g[4] >> 31) - 1) % (1 << 32)
    assert take_g in (0, 0xFFFFFFFF) and (take_g != 0) == (p26_value(h) >= P1305)
    note(stats, "finish_take_g", 1 if take_g else 0); note(stats, "finish_take_h", 0 if take_g else 1)
    h = [(x & ~take_g & 0xFFFFFFFF) | (y & take_g) for x, y in zip(h, g)]
    M32 = 0xFFFFFFFF
    hw = [(h[0] | (h[1] << 26)) & M32, ((h[1] >> 6) | (h[2] << 20)) & M32, ((h[2] >> 12) | (h[3] << 14)) & M32, ((h[3] >> 18) | (h[4] << 8)) & M32]
    tag, f = [], 0
    for i in range(4):
        f = u64(hw[i] + s[i] + (f >> 32)); tag.append(f & M32)
        note(stats, "finish_word_carry_%d" % i, f >> 32)
    return b"".join(x.to_bytes(4, "little") for x in tag)


def poly_state(key32: bytes, stats=None):
    """derive_poly_state: s, rpow[i] = r^(i+1), r64, rS = r^1024"""
    r = p26_clamped_r(key32[:16])
    rp, rpow = r, []
    for i in range(64):
        rpow.append(rp)
        if i < 63:
            rp = p26_mul(rp, r, stats)
    r64 = rp
    steps = POLY_STEPS
    while steps > 1:
        rp = p26_mul(rp, rp, stats); steps >>= 1
    rv = p26_value(r)
    assert all(p26_value(x) % P1305 == pow(rv, i + 1, P1305) for i, x in enumerate(rpow))
    assert p26_value(rp) % P1305 == pow(rv, REGION_PIECES, P1305)
    return {"s": key32[16:32], "rpow": rpow, "r64": r64, "rS": rp}


def sbox_regions(max_msg):
    return -(-(-(-max_msg // 16)) // REGION_PIECES) + (1 if max_msg == 0 else 0)


def poly_partials(st, msg: bytes, regions, stats=None):
    """sbox_poly_kernel: one wave per region, returns partial[region] = the 64-lane uint32_t sums"""
    mlen = len(msg)
    npieces, tail = (mlen + 15) // 16, mlen & 15
    partial = []
    for region in range(regions):
        lanes = []
        for lane in range(LANES):
            h = [0] * 5
            d0 = region * REGION_PIECES + lane + 1
            if d0 - lane <= npieces:
                for m in range(POLY_STEPS - 1, -1, -1):
                    d = d0 + 64 * m
                    h = p26_mul(h, st["r64"], stats)
                    if d <= npieces:
                        b = npieces - d
                        nb = tail if (d == 1 and tail) else 16
                        h = p26_add(h, p26_from_piece(msg[16 * b:16 * b + nb]))
                h = p26_carry(p26_mul(h, st["rpow"][lane], stats), stats, after_mul=True)
                note(stats, "lane_out", max(h))
            lanes.append(h)
        sums = [u32(sum(h[j] for h in lanes), "64-lane sum") for j in range(5)]
        note(stats, "lane_sum", max(sums))
        partial.append(sums)
    return partial


def poly_final(st, partial, mlen, stats=None):
    """sbox_final_kernel (a good row): Horner over the `used` regions with r^1024, then p26_finish"""
    used = ((mlen + 15) // 16 + REGION_PIECES - 1) // REGION_PIECES
    assert used <= len(partial)
    acc = [0] * 5
    for g in range(used - 1, -1, -1):
        t = p26_mul(acc, st["rS"], stats)
        acc = p26_add(t, p26_carry(partial[g], stats))
    return p26_finish(acc, st["s"], stats)


def poly1305_device_order(key32: bytes, msg: bytes, regions=None, stats=None):
    st = poly_state(key32, stats)
    regions = sbox_regions(len(msg)) if regions is None else regions
    return poly_final(st, poly_partials(st, msg, regions, stats), len(msg), stats)


def poly1305_bigint(key32: bytes, msg: bytes):
    r = int.from_bytes(key32[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    h = 0
    for i in range(0, len(msg), 16):
        h = (h + int.from_bytes(msg[i:i + 16] + b"\x01", "little")) * r % P1305
    return ((h + int.from_bytes(key32[16:], "little")) % (1 << 128)).to_bytes(16, "little")


KEY_R1 = lambda s16=bytes(16): (1).to_bytes(16, "little") + s16         # r = 1: every power of r is 1
KEY_RMAX = lambda s16=bytes(16): b"\xff" * 16 + s16                      # r with every clamped bit set


def limb_extreme_message(mlen):
    """A message of `mlen` bytes for a key with r = 1.  There every lane's value is the plain sum of the pieces it reads (a piece
    = its 1 .. 16 bytes + the pad bit), kept partially reduced; wherever a lane reads three pieces or more, its bytes are chosen
    so that the sum is 2^130 - 1 + k (2^130 - 5), which the lane holds as 2^130 - 1: all five limbs 2^26 - 1, the largest a lane
    can hand to the 64-lane sum.  Lanes with one or two pieces get all-0xFF bytes."""
    npieces, tail = (mlen + 15) // 16, mlen & 15
    msg = bytearray(mlen)
    for region in range(sbox_regions(mlen) if mlen else 0):
        for lane in range(LANES):
            ds = [d for d in (region * REGION_PIECES + lane + 1 + 64 * m for m in range(POLY_STEPS)) if d <= npieces]
            if not ds:
                continue
            size = {d: (tail if (d == 1 and tail) else 16) for d in ds}
            pads = sum(1 << (8 * size[d]) for d in ds)
            cap = sum((1 << (8 * size[d])) - 1 for d in ds)
            k = 0
            while (1 << 130) - 1 + k * P1305 - pads < 0:
                k += 1
            want = (1 << 130) - 1 + k * P1305 - pads
            if want > cap:
                want = cap                                           # too few pieces: all 0xFF
            for d in ds:
                take = min(want, (1 << (8 * size[d])) - 1)
                want -= take
                b = npieces - d
                msg[16 * b:16 * b + size[d]] = take.to_bytes(size[d], "little")
            assert want == 0
    return bytes(msg)


# ---- interval arithmetic over the same steps: (lo, hi) per limb ------------------------------------------------------
def p26_mul_interval(A, B):
    """largest limbs out for limbs of a <= A[i], of b <= B[i] (every term is monotone, so the maxima come from the maxima)"""
    s = [None] + [u32(B[i] * 5, "5 b_i") for i in range(1, 5)]
    d = [A[0] * B[0] + A[1] * s[4] + A[2] * s[3] + A[3] * s[2] + A[4] * s[1],
         A[0] * B[1] + A[1] * B[0] + A[2] * s[4] + A[3] * s[3] + A[4] * s[2],
         A[0] * B[2] + A[1] * B[1] + A[2] * B[0] + A[3] * s[4] + A[4] * s[3],
         A[0] * B[3] + A[1] * B[2] + A[2] * B[1] + A[3] * B[0] + A[4] * s[4],
         A[0] * B[4] + A[1] * B[3] + A[2] * B[2] + A[3] * B[1] + A[4] * B[0]]
    cols = max(d)
    for i in range(4):
        d[i + 1] = u64(d[i + 1] + (u64(d[i]) >> 26))
    top = u64(M26 + (d[4] >> 26) * 5)                     # limb 0 after its mask, plus the wrap
    return [M26, u32(M26 + (top >> 26)), M26, M26, M26], cols


def _carry_step(iv, add):
    """(lo, hi) of a limb + a carry in `add` -> (carry interval, masked interval); asserts the uint32_t sum"""
    lo, hi = iv[0] + add[0], u32(iv[1] + add[1], "limb + carry")
    c = (lo >> 26, hi >> 26)
    return c, ((lo & M26, hi & M26) if c[0] == c[1] else (0, M26))


def p26_carry_interval(H):
    """H: five (lo, hi); returns five (lo, hi) after p26_carry"""
    out, c = [None] * 5, (0, 0)
    for i in range(5):
        c, out[i] = _carry_step(H[i], c)
    c, out[0] = _carry_step(out[0], (c[0] * 5, c[1] * 5))
    out[1] = (out[1][0] + c[0], u32(out[1][1] + c[1]))
    return out


# ================================================================================================================
# GF(2^255 - 19), ten signed limbs of 26 / 25 bits
# ================================================================================================================
def fe_bits(i):
    return 25 if i & 1 else 26


FE_OFF = [sum(fe_bits(j) for j in range(i)) for i in range(10)]


def fe_value(h):
    return sum(x << FE_OFF[i] for i, x in enumerate(h))


def fe_from_bytes(u32bytes: bytes):
    v = int.from_bytes(u32bytes, "little")
    h = [(v >> FE_OFF[i]) & ((1 << fe_bits(i)) - 1) for i in range(10)]        # limb 9: bits 230 .. 254, bit 255 dropped
    assert fe_value(h) == v % (1 << 255)
    return h


def fe_add(f, g):
    return [i32(a + b, "fe_add") for a, b in zip(f, g)]


def fe_sub(f, g):
    return [i32(a - b, "fe_sub") for a, b in zip(f, g)]


def fe_carry(h, stats=None):
    h = list(h)
    before = fe_value(h)
    for x in h:
        i64(x, "fe_carry in"); note(stats, "fe_col", abs(x))
    for _ in range(2):
        for i in range(9):
            bits = fe_bits(i)
            c = i64(h[i] + (1 << (bits - 1))) >> bits
            h[i + 1] = i64(h[i + 1] + c); h[i] = i64(h[i] - c * (1 << bits))
        c9 = i64(h[9] + (1 << 24)) >> 25
        h[0] = i64(h[0] + i64(c9 * 19)); h[9] -= c9 * (1 << 25)
    c0 = i64(h[0] + (1 << 25)) >> 26
    h[1] += c0; h[0] -= c0 * (1 << 26)
    for i in range(10):
        half = 1 << (fe_bits(i) - 1)
        if i == 1:
            assert -half - 1 <= h[i] <= half, ("fe_carry out", i, h[i])
        else:
            assert -half <= h[i] < half, ("fe_carry out", i, h[i])
        i32(h[i])
    assert fe_value(h) % P25519 == before % P25519
    return h


def fe_mul(f, g, stats=None):
    for x in f + g:
        i32(x)
    note(stats, "fe_mul_operand", max(abs(x) for x in f + g))
    note(stats, "fe_mul_operand_odd", max(abs(x) for x in f[1::2] + g[1::2]))
    g19 = [i32(19 * x, "19 g_i") for x in g]
    f2 = [i32(2 * x, "2 f_i") for x in f]
    h = [0] * 10
    for i in range(10):
        for j in range(10):
            a = f2[i] if (i & 1) and (j & 1) else f[i]
            k = i + j
            if k < 10:
                h[k] = i64(h[k] + a * g[j], "fe_mul column")
            else:
                h[k - 10] = i64(h[k - 10] + a * g19[j], "fe_mul column")
    out = fe_carry(h, stats)
    assert fe_value(out) % P25519 == fe_value(f) * fe_value(g) % P25519
    return out


def fe_sq(f, stats=None):
    for x in f:
        i32(x)
    note(stats, "fe_sq_operand", max(abs(x) for x in f))
    f2 = [i32(2 * x, "2 f_i") for x in f]
    f19 = [i32(19 * x, "19 f_i") for x in f]
    h = [0] * 10
    for i in range(10):
        a = f2[i] if i & 1 else f[i]
        k = 2 * i
        if k < 10:
            h[k] = i64(h[k] + a * f[i])
        else:
            h[k - 10] = i64(h[k - 10] + a * f19[i])
        for j in range(i + 1, 10):
            a = i32(2 * f2[i], "4 f_i") if (i & 1) and (j & 1) else f2[i]
            k = i + j
            if k < 10:
                h[k] = i64(h[k] + a * f[j])
            else:
                h[k - 10] = i64(h[k - 10] + a * f19[j])
    out = fe_carry(h, stats)
    assert fe_value(out) % P25519 == fe_value(f) ** 2 % P25519
    return out


def fe_mul_a24(f, stats=None):
    return fe_carry([i64(x * 121665) for x in f], stats)


def fe_invert(z, stats=None):
    sq = lambda x, n=1: x if n == 0 else sq(fe_sq(x, stats), n - 1)
    mul = lambda a, b: fe_mul(a, b, stats)
    t0 = sq(z); t1 = sq(t0, 2); t1 = mul(z, t1); t0 = mul(t0, t1); t2 = sq(t0); t1 = mul(t1, t2)
    t2 = sq(t1, 5); t1 = mul(t2, t1)
    t2 = sq(t1, 10); t2 = mul(t2, t1)
    t3 = sq(t2, 20); t2 = mul(t3, t2)
    t2 = sq(t2, 10); t1 = mul(t2, t1)
    t2 = sq(t1, 50); t2 = mul(t2, t1)
    t3 = sq(t2, 100); t2 = mul(t3, t2)
    t2 = sq(t2, 50); t1 = mul(t2, t1)
    t1 = sq(t1, 5)
    out = mul(t1, t0)
    assert fe_value(out) % P25519 == pow(fe_value(z), P25519 - 2, P25519)
    return out


def fe_to_bytes(f):
    h = [i32(x) for x in f]
    want = fe_value(h) % P25519
    q = i32(19 * h[9] + (1 << 24), "19 h_9") >> 25
    for i in range(10):
        q = i32(h[i] + q) >> fe_bits(i)
    h[0] = i32(h[0] + i32(19 * q))
    for i in range(9):
        bits = fe_bits(i)
        c = h[i] >> bits
        h[i + 1] = i32(h[i + 1] + c); h[i] = i32(h[i] - i32(c * (1 << bits)))
    h[9] &= (1 << 25) - 1
    assert all(0 <= h[i] < 1 << fe_bits(i) for i in range(10)), h
    v = fe_value(h)
    assert v == want, ("fe_to_words", q)
    return v.to_bytes(32, "little")


def _clamp(k: bytes):
    e = bytearray(k); e[0] &= 248; e[31] = (e[31] & 127) | 64
    return int.from_bytes(e, "little")


def _cswap(a, b, bit):
    return (b, a) if bit else (a, b)


def ladder_step_lane(x1, x2, z2, x3, z3, stats=None):
    """one step of x25519() (the one-lane form: fe_sq and fe_mul_a24)"""
    A = fe_add(x2, z2); AA = fe_sq(A, stats); B = fe_sub(x2, z2); BB = fe_sq(B, stats)
    E = fe_sub(AA, BB); C = fe_add(x3, z3); D = fe_sub(x3, z3)
    DA = fe_mul(D, A, stats); CB = fe_mul(C, B, stats)
    x3 = fe_sq(fe_add(DA, CB), stats)
    z3 = fe_mul(x1, fe_sq(fe_sub(DA, CB), stats), stats)
    x2 = fe_mul(AA, BB, stats)
    z2 = fe_mul(E, fe_add(AA, fe_mul_a24(E, stats)), stats)
    return x2, z2, x3, z3


FE_A24 = [121665] + [0] * 9


def ladder_step_quad(x1, x2, z2, x3, z3, stats=None):
    """one step of x25519_quad: three levels of four fe_mul(P, Q), lane c computing the c-th product"""
    A = fe_add(x2, z2); B = fe_sub(x2, z2); C = fe_add(x3, z3); D = fe_sub(x3, z3)
    AA, BB, DA, CB = (fe_mul(P, Q, stats) for P, Q in ((A, A), (B, B), (D, A), (C, B)))
    E = fe_sub(AA, BB); S = fe_add(DA, CB); Df = fe_sub(DA, CB)
    x3, tt, x2, uu = (fe_mul(P, Q, stats) for P, Q in ((S, S), (Df, Df), (AA, BB), (E, FE_A24)))
    W = fe_add(AA, uu)
    r = [fe_mul(P, Q, stats) for P, Q in ((x1, tt), (x1, tt), (E, W), (E, W))]
    return x2, r[2], x3, r[0]


def x25519_model(k: bytes, u: bytes, quad: bool, stats=None):
    e = _clamp(k)
    x1 = fe_from_bytes(u)
    x2, z2, x3, z3 = [1] + [0] * 9, [0] * 10, list(x1), [1] + [0] * 9
    swap = 0
    step = ladder_step_quad if quad else ladder_step_lane
    for t in range(254, -1, -1):
        kt = (e >> t) & 1
        swap ^= kt
        x2, x3 = _cswap(x2, x3, swap); z2, z3 = _cswap(z2, z3, swap)
        swap = kt
        x2, z2, x3, z3 = step(x1, x2, z2, x3, z3, stats)
    x2, x3 = _cswap(x2, x3, swap); z2, z3 = _cswap(z2, z3, swap)
    return fe_to_bytes(fe_mul(x2, fe_invert(z2, stats), stats))


def fe_mul_interval(F, G):
    """largest |column| of fe_mul for |f_i| <= F[i], |g_i| <= G[i]; asserts the int32_t factors"""
    g19 = [i32(19 * x, "19 g_i") for x in G]
    f2 = [i32(2 * x, "2 f_i") for x in F]
    h = [0] * 10
    for i in range(10):
        for j in range(10):
            a = f2[i] if (i & 1) and (j & 1) else F[i]
            if i + j < 10:
                h[i + j] += a * G[j]
            else:
                h[i + j - 10] += a * g19[j]
    return [i64(x) for x in h]


def fe_carry_interval(H):
    """|h_i| <= H[i] in -> bounds of |h_i| out (fe_carry, every intermediate asserted int64_t)"""
    H = list(H)
    for _ in range(2):
        for i in range(9):
            bits = fe_bits(i)
            c = i64(H[i] + (1 << (bits - 1))) >> bits                # |carry| <= this for h_i of either sign
            i64(c << bits)
            H[i + 1] = i64(H[i + 1] + c); H[i] = 1 << (bits - 1)
        c9 = i64(H[9] + (1 << 24)) >> 25
        H[0] = i64(H[0] + i64(c9 * 19)); H[9] = 1 << 24
    c0 = i64(H[0] + (1 << 25)) >> 26
    H[1] += c0; H[0] = 1 << 25
    return H


# ---- the edge u-coordinates of tests/test_sealedbox_extremes_gpu.py (and of the whole-ladder cases here) ---------------
LIMB_BOUNDARIES = (26, 51, 77, 102, 128, 153, 179, 204, 230)


def edge_points():
    """name -> 32-byte u: canonical edges, non-canonical encodings, bit 255, saturated limbs, limb boundaries"""
    pts = {"2": 2, "9": 9, "9+2^255": 9 + (1 << 255), "p-2": P25519 - 2}
    for k in range(2, 19):
        pts["p+%d" % k] = P25519 + k
    for i in range(10):
        pts["limb%d_saturated" % i] = ((1 << fe_bits(i)) - 1) << FE_OFF[i]
    for b in LIMB_BOUNDARIES:
        for d in (-1, 0, 1):
            pts["2^%d%+d" % (b, d)] = (1 << b) + d
    return {n: v.to_bytes(32, "little") for n, v in pts.items()}


def edge_scalars():
    alt = bytes([0xAA] * 32)
    runs = bytes([0xFF] * 8 + [0x00] * 8 + [0xFF] * 8 + [0x00] * 8)
    return {"zero": bytes(32), "ones": b"\xff" * 32, "clamp_bits_only": bytes(31) + b"\x40", "alternating": alt,
            "alternating_inv": bytes([0x55] * 32), "long_runs": runs, "long_runs_inv": bytes(x ^ 0xFF for x in runs)}

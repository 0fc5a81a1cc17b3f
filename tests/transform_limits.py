"""The transform kernel (packed_gen_fft_kernel, sda_amd/csrc/fft_kernels.hip) at the range limits of its 32-bit forms and over its
shape space (shared by tests/test_fft_model.py, tests/test_transform_limits_reach.py and tests/test_transform_limits_gpu.py - a
helper module, not a conftest).

  * ONE whole-kernel integer model, Dev / share_transform, for the three instantiations: WIDE (uint64_t values, p < 2^62), NARROW
    reduced (uint32_t, p < 2^30, the conditional subtractions of the wide form) and NARROW lazy (uint32_t, (4b + 4) p < 2^32, no
    conditional subtraction in the radix-3 levels).  It follows the kernel line by line - f_redA / f_full2 per mode, the nz_mask
    shortcut v[e1][*] = in[0], f_full2 on B and C at jj = 0 of the second folded level (lazy only), the single radix-3 level when
    b - 2 is odd, the radix-9 passes, the final f_csub(f_full2(.), p) - asserts that every register value fits its register, and
    records the largest value each stage holds.
  * plan(): the host's plan restated (fft_narrow, fft_shape with the LDS arithmetic of fft_lds_bytes, fft_lazy in sda_capi.cpp).
  * PRIMES: for each (a, b) = (log2(k + t + 1), log3(n + 1)) the primes p = 1 mod 2^a 3^b on either side of the two thresholds -
    (4b + 4) p = 2^32 (lazy admission) and p = 2^30 (32-bit values at all) - as literals, recomputed by the reach test.
  * CASES: the case table the CPU reach test and the GPU test both run, with the inputs of each case (all p - 1; (p - 1)/2 against
    (p + 1)/2; the specials of test_transform_path_modulus_bound; any-i64 random; canonical random - fixed seeds, one kind per batch).
  * REACH: the per-stage maxima the model records for each case, as fractions of 2^32.  The lazy chain's proven maximum (4b + 2) p
    is 0.83 - 0.94 of 2^32 at these primes; valid inputs reach what the table says and no test claims more."""
import random

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
STAGES = ("radix2", "folded", "later", "final")


class Dev:
    """device-side arithmetic with register-width and range assertions: width 64 (WIDE), or 32 reduced / lazy (NARROW)"""

    def __init__(self, p, width=64, lazy=False):
        assert width in (64, 32) and not (lazy and width == 64)
        if width == 64:
            assert 2 <= p < (1 << 62)                            # every modulus the library takes (make_mod): 4p < 2^64
        else:
            assert 2 <= p < (1 << 30)                            # fft_narrow: 4p < 2^32
        self.p, self.p2, self.width, self.lazy = p, 2 * p, width, lazy
        self.mask = (1 << width) - 1
        self.np = (1 << width) - p
        self.one = self.pair(1)                                  # FftPlan.one_s: the companion of 1
        self.stage = "radix2"
        self.maxima = dict.fromkeys(STAGES, 0)

    def reg(self, x):
        """a value the kernel holds in a V register: it fits, and the stage's maximum sees it"""
        assert 0 <= x <= self.mask, (x, self.stage)
        if x > self.maxima[self.stage]:
            self.maxima[self.stage] = x
        return x

    def pair(self, w):
        """host side: a constant and its companion floor(w 2^width / p)"""
        w %= self.p
        return w, (w << self.width) // self.p

    def mulS(self, x, c):
        """x (ANY value of the register) times the constant c = (w, ws): congruent to x w, in [0, 2p)"""
        w, ws = c
        self.reg(x)
        q = (x * ws) >> self.width
        r = x * w - q * self.p
        assert 0 <= r < self.p2, (x, w, r)
        if self.width == 64:
            # the kernel computes the low 64 bits as x w + q (2^64 - p): one pair of accumulating 32 x 32 products plus four
            # low products into the high word
            x0, x1, q0, q1 = x & M32, x >> 32, q & M32, q >> 32
            w0, w1, n0, n1 = w & M32, w >> 32, self.np & M32, self.np >> 32
            t = (x0 * w0 + q0 * n0) & M64
            h = (x0 * w1 + x1 * w0 + q0 * n1 + q1 * n0) & M32
            assert (t + (h << 32)) & M64 == r
        else:
            # __umulhi(x, ws), then x * w - q * p in 32-bit registers: both products wrap, their difference does not
            assert q <= M32 and ws <= M32
            assert (((x * w) & M32) - ((q * self.p) & M32)) & M32 == r
        return r

    def csub(self, x, m):
        """x < 2m -> x < m.  WIDE: the borrow of the 64-bit subtraction selects.  NARROW: d = x - m wraps exactly when x < m, and
        the UNSIGNED minimum d < x ? d : x picks the right one - also for x >= 2^31"""
        self.reg(x)
        assert x < 2 * m, (x, m)
        want = x - m if x >= m else x
        if self.width == 32:
            d = (x - m) & M32
            got = d if d < x else x
            assert got == want, (x, m)
        return want

    def red2(self, x):
        return self.csub(x, self.p2)

    def redA(self, x):
        """f_redA: the A input of a level - [0, 4p) -> [0, 2p), or left to grow (lazy)"""
        return self.reg(x) if self.lazy else self.red2(x)

    def full2(self, x):
        """f_full2: any value of the lazy chain -> [0, 2p) by a Shoup product by 1; reduced forms: a conditional subtraction"""
        return self.mulS(x, self.one) if self.lazy else self.red2(x)

    def r3(self, A, Bv, Cv, om):
        """radix-3 butterfly, B and C in [0, 2p): y_d = A + w^d B + w^2d C.  Reduced: A in [0, 2p), outputs in [0, 4p).  Lazy: no
        conditional subtraction, the outputs are A + [0, 4p]"""
        p2 = self.p2
        assert Bv < p2 and Cv < p2
        w = self.mulS(self.reg(Bv + p2 - Cv), om)
        if self.lazy:
            self.reg(A)
            y0 = self.reg(self.reg(A + Bv) + Cv)
            y1 = self.reg(self.reg(A + self.reg(p2 - Cv)) + w)
            y2 = self.reg(self.reg(A + self.reg(p2 - Bv)) + self.reg(p2 - w))
            for y in (y0, y1, y2):
                assert y <= A + 2 * p2
            return y0, y1, y2
        assert A < p2
        y0 = self.reg(self.red2(self.reg(A + Bv)) + Cv)
        y1 = self.reg(self.red2(self.reg(A + p2 - Cv)) + w)
        y2 = self.reg(self.red2(self.reg(A + p2 - Bv)) + (p2 - w))
        for y in (y0, y1, y2):
            assert y < 2 * p2
        return y0, y1, y2


def bitrev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


def trirev(i, digits):
    r = 0
    for _ in range(digits):
        r = r * 3 + i % 3
        i //= 3
    return r


def structure(k, t, n):
    """(a, b): k + t + 1 = 2^a and n + 1 = 3^b"""
    m2, m3 = k + t + 1, n + 1
    a, b = m2.bit_length() - 1, 0
    while 3 ** b < m3:
        b += 1
    assert 1 << a == m2 and 3 ** b == m3 and b >= 2
    return a, b


def nz_mask(m2, m3):
    """build_fft's nz_mask as [e0][e1]: some 9-block has the coefficient r + e1 m3/9 + e0 m3/3"""
    return [[e1 * (m3 // 9) + e0 * (m3 // 3) < m2 for e1 in range(3)] for e0 in range(3)]


def share_transform(dev, k, t, n, w2, w3, secrets, draws):
    """one batch, exactly as the kernel does it; dev.maxima holds the largest register value of each stage afterwards"""
    p, p2 = dev.p, dev.p2
    m2, m3 = k + t + 1, n + 1
    a, b = structure(k, t, n)
    w2i = pow(w2, -1, p)
    tw2 = [dev.pair(pow(w2i, j, p)) for j in range(max(m2 // 2, 1))]
    tw3 = [dev.pair(pow(w3, j, p)) for j in range(m3)]
    om = dev.pair(pow(w3, m3 // 3, p))
    scale = dev.pair(pow(m2, -1, p))
    reg = dev.reg
    dev.stage = "radix2"
    x = [0] + [s % p for s in secrets] + [r % p for r in draws]            # canonical
    # ---- radix-2 inverse transform, decimation in frequency: natural order in, bit-reversed order out, values in [0, 2p)
    mblk, lg = m2, a
    if lg & 1:
        h = mblk // 2
        for jj in range(h):
            av, bv = x[jj], x[jj + h]
            x[jj] = dev.red2(reg(av + bv))
            x[jj + h] = dev.mulS(reg(av + p2 - bv), tw2[jj])
        mblk //= 2
        lg -= 1
    while lg >= 2:
        qd, step = mblk // 4, m2 // mblk
        for i in range(m2 // 4):
            blk, jj = i // qd, i % qd
            base = blk * mblk + jj
            x0, x1, x2, x3 = (x[base + e * qd] for e in range(4))
            assert max(x0, x1, x2, x3) < p2
            a0, a1 = dev.red2(reg(x0 + x2)), dev.red2(reg(x1 + x3))
            a3 = dev.mulS(reg(x1 + p2 - x3), tw2[(jj + qd) * step])
            if qd > 1:
                a2 = dev.mulS(reg(x0 + p2 - x2), tw2[jj * step])
                b1 = dev.mulS(reg(a0 + p2 - a1), tw2[2 * jj * step])
                b3 = dev.mulS(reg(a2 + p2 - a3), tw2[2 * jj * step])
            else:
                a2 = dev.red2(reg(x0 + p2 - x2))
                b1 = dev.red2(reg(a0 + p2 - a1))
                b3 = dev.red2(reg(a2 + p2 - a3))
            x[base], x[base + qd], x[base + 2 * qd], x[base + 3 * qd] = dev.red2(reg(a0 + a1)), b1, dev.red2(reg(a2 + a3)), b3
        lg -= 2
        mblk //= 4
    assert lg == 0
    # ---- scale by 1 / m2, zero-extend, first two radix-3 levels (decimation in time, digit-reversed input) ----------------
    dev.stage = "folded"
    y = [None] * m3
    ninth, S1 = m3 // 9, m3 // 3
    S2 = ninth
    nz = nz_mask(m2, m3)
    for q in range(ninth):
        r = trirev(q, b - 2)
        v = [[None] * 3 for _ in range(3)]
        for e1 in range(3):
            inp = [0, 0, 0]
            for e0 in range(3):
                ci = r + e1 * S2 + e0 * S1
                if nz[e0][e1] and ci < m2:
                    inp[e0] = dev.mulS(x[bitrev(ci, a)], scale)
                else:
                    assert ci >= m2                                        # the mask never hides a coefficient
            if nz[1][e1] or nz[2][e1]:
                v[e1] = [dev.redA(z) for z in dev.r3(inp[0], inp[1], inp[2], om)]
            else:
                v[e1] = [inp[0]] * 3                                       # two of three inputs are zero-extension zeros
        for jj in range(3):
            Bv, Cv = v[1][jj], v[2][jj]
            if jj:
                Bv = dev.mulS(Bv, tw3[jj * ninth])
                Cv = dev.mulS(Cv, tw3[2 * jj * ninth])
            elif dev.lazy:                                                 # twiddle 1: no product brings them back to [0, 2p)
                Bv, Cv = dev.full2(Bv), dev.full2(Cv)
            y[9 * q + jj], y[9 * q + jj + 3], y[9 * q + jj + 6] = dev.r3(v[0][jj], Bv, Cv, om)
    assert all(z is not None for z in y) and (dev.lazy or all(z < 2 * p2 for z in y))
    # ---- remaining levels: a single one when their number is odd, then two at a time -----------------------------------
    dev.stage = "later"
    t3, left = 9, b - 2
    if left & 1:
        step = m3 // (3 * t3)
        for q in range(S1):
            blk, jj = q // t3, q % t3
            base = blk * 3 * t3 + jj
            A = dev.redA(y[base])
            Bv, Cv = dev.mulS(y[base + t3], tw3[jj * step]), dev.mulS(y[base + 2 * t3], tw3[2 * jj * step])
            y[base], y[base + t3], y[base + 2 * t3] = dev.r3(A, Bv, Cv, om)
        t3 *= 3
        left -= 1
    while left:
        step_a, step_b = m3 // (3 * t3), m3 // (9 * t3)
        for q in range(ninth):
            blk, jj = q // t3, q % t3
            base = blk * 9 * t3 + jj
            av = [y[base + e * t3] for e in range(9)]
            v = [None] * 9
            for e1 in range(3):
                A = dev.redA(av[3 * e1])
                Bv, Cv = dev.mulS(av[3 * e1 + 1], tw3[jj * step_a]), dev.mulS(av[3 * e1 + 2], tw3[2 * jj * step_a])
                v[3 * e1:3 * e1 + 3] = dev.r3(A, Bv, Cv, om)
            for d in range(3):
                jb = jj + d * t3
                A = dev.redA(v[d])
                Bv, Cv = dev.mulS(v[3 + d], tw3[jb * step_b]), dev.mulS(v[6 + d], tw3[2 * jb * step_b])
                y[base + d * t3], y[base + (d + 3) * t3], y[base + (d + 6) * t3] = dev.r3(A, Bv, Cv, om)
        t3 *= 9
        left -= 2
    assert t3 == m3
    dev.stage = "final"
    out = [dev.csub(dev.full2(z), p) for z in y]                                   # canonical
    assert out[0] == 0                                                             # f(1) = 0 (tss asserts the same)
    return out[1:]


# ---- the host's plan (sda_capi.cpp: fft_narrow, fft_shape, fft_lazy; fft_kernels.hip: fft_lds_bytes) ---------------------------------
HALF_CU, WHOLE_CU = 80 * 1024, 160 * 1024


def lds_bytes(m2, m3, G, tw_lds, narrow):
    return (G * (m2 + m3) + (2 * (m3 + m2 // 2) if tw_lds else 0)) * (4 if narrow else 8)


def plan(p, k, t, n, knobs=()):
    """(narrow, lazy, G, tw_lds) of the transform kernel for this scheme under these knobs ((name, value) pairs)"""
    kn = dict(knobs)
    m2, m3 = k + t + 1, n + 1
    _, b = structure(k, t, n)
    narrow = p < (1 << 30) and not kn.get("SDA_NO_NARROW")
    G = tw_lds = 0
    cand = 16 if narrow else 8                      # the most batches per workgroup that leave two workgroups per CU
    while cand >= 1 and not G:
        for tw in (1, 0):
            if not G and lds_bytes(m2, m3, cand, tw, narrow) <= HALF_CU:
                G, tw_lds = cand, tw
        cand >>= 1
    if not G and lds_bytes(m2, m3, 1, 0, narrow) <= WHOLE_CU:
        G, tw_lds = 1, 0                            # a single batch may take the whole CU
    want = kn.get("SDA_FFT_G", 0)
    if want in (1, 2, 4, 8, 16):
        if lds_bytes(m2, m3, want, 1, narrow) <= HALF_CU:
            G, tw_lds = want, 1
        elif lds_bytes(m2, m3, want, 0, narrow) <= WHOLE_CU:
            G, tw_lds = want, 0
    assert G
    lazy = narrow and (4 * b + 4) * p < (1 << 32) and not kn.get("SDA_NO_LAZY")
    return bool(narrow), bool(lazy), G, tw_lds


def kernel_suffix(narrow, lazy):
    """how sda_debug_last_kernel() names the instantiation (note_kernel in fft_launch_v)"""
    return f"{'unsigned int' if narrow else 'unsigned long'}, {'true' if lazy else 'false'}>"


# ---- primes ----------------------------------------------------------------------------------------------------------------------
def is_prime(n):
    """deterministic Miller-Rabin (the first twelve prime bases decide every n < 3.3 10^24)"""
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    if n < 2:
        return False
    for q in bases:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in bases:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_below(limit, step):
    """the largest prime p = 1 mod step with p < limit"""
    p = (limit - 2) // step * step + 1
    while not is_prime(p):
        p -= step
    return p


def prime_from(limit, step):
    """the smallest prime p = 1 mod step with p >= limit"""
    p = (limit - 1 + step - 1) // step * step + 1
    while not is_prime(p):
        p += step
    return p


def threshold_primes(a, b):
    """(lazy_below, lazy_above, narrow_below, narrow_above) for p = 1 mod 2^a 3^b: (4b + 4) p < 2^32 holds exactly for
    p < ceil(2^32 / (4b + 4))"""
    step = 2 ** a * 3 ** b
    thr = -(-(1 << 32) // (4 * b + 4))
    return prime_below(thr, step), prime_from(thr, step), prime_below(1 << 30, step), prime_from(1 << 30, step)


# (a, b): (lazy_below, lazy_above, narrow_below, narrow_above) - threshold_primes(a, b), written out so that a reader sees them.
# For a large 2^a 3^b the nearest prime lies several percent under its threshold: those shapes are here for their structure, the
# small-a shapes for tightness
PRIMES = {
    (2, 2): (357913909, 357913981, 1073741689, 1073741833),
    (3, 2): (357913441, 357914377, 1073741689, 1073741833),
    (3, 3): (268433569, 268437241, 1073740537, 1073741833),
    (4, 3): (268433569, 268437457, 1073738161, 1073742913),
    (4, 4): (214738129, 214761457, 1073732113, 1073759329),
    (5, 4): (214736833, 214767937, 1073730817, 1073759329),
    (6, 4): (214736833, 214767937, 1073730817, 1073782657),
    (6, 5): (178894657, 179050177, 1073414593, 1073850049),
    (7, 5): (178661377, 179127937, 1073305729, 1073927809),
    (7, 6): (153311617, 153871489, 1071595009, 1073927809),
    (8, 6): (151911937, 155831041, 1071595009, 1074394369),
    (9, 6): (151911937, 156764161, 1071595009, 1075327489),
    (9, 7): (128770561, 145566721, 1071595009, 1080552961),
    (10, 7): (120932353, 145566721, 1045840897, 1088391169),
    (3, 5): (178954921, 178974361, 1073717857, 1073743129),
    (3, 8): (118675369, 119620153, 1073432089, 1073851993),
    (3, 9): (104713561, 108650161, 1073432089, 1075164193),
}
LAZY_BELOW, LAZY_ABOVE, NARROW_BELOW, NARROW_ABOVE = range(4)


def root(p, order):
    """an element of exactly this order (2^a or 3^b) mod p, from the smallest base that gives one"""
    assert (p - 1) % order == 0
    for g in range(2, 2000):
        w = pow(g, (p - 1) // order, p)
        if all(pow(w, order // f, p) != 1 for f in (2, 3) if order % f == 0):
            return w
    raise AssertionError("no root")


# ---- the case table --------------------------------------------------------------------------------------------------------------
# the 14 structures of test_transform_kernel_over_the_shape_space (tests/test_parity_gpu.py) with its split rule for k
SWEEP = [(2, 2, 0.5), (3, 2, 0.4), (3, 3, 0.9), (4, 3, 0.1), (4, 4, 0.5), (5, 4, 0.3), (6, 4, 0.7), (6, 5, 0.5),
         (7, 5, 0.2), (7, 6, 0.6), (8, 6, 0.39), (9, 6, 0.5), (9, 7, 0.5), (10, 7, 0.25)]
EDGES = [(2, 2), (3, 3), (3, 5), (3, 9)]


def shape(a, b, split=0.5):
    kt = (1 << a) - 1
    k = max(1, min(kt, int(round(kt * split))))
    return k, kt - k, 3 ** b - 1


def _case(kind, k, t, n, which, batches, knobs=(), agree=False, dim=None, xcd=False):
    a, b = structure(k, t, n)
    p = PRIMES[(a, b)][which]
    knobs = (("SDA_NO_NGEMM", 1),) + ((("SDA_FORCE_FFT", 1),) if k + t <= 32 else ()) + tuple(knobs)
    narrow, lazy, G, tw_lds = plan(p, k, t, n, knobs)
    tag = "+".join(f"{nm[4:]}{v if nm == 'SDA_FFT_G' else ''}" for nm, v in knobs[1:] if nm != "SDA_FORCE_FFT")
    name = f"{kind}-a{a}b{b}-k{k}t{t}n{n}-{('lazy_below', 'lazy_above', 'narrow_below', 'narrow_above')[which]}" + (f"-{tag}" if tag else "")
    return dict(name=name, kind=kind, a=a, b=b, k=k, t=t, n=n, p=p, which=which, batches=batches, knobs=knobs, agree=agree, xcd=xcd,
                dim=k * batches - k // 2 if dim is None else dim, narrow=narrow, lazy=lazy, G=G, tw_lds=tw_lds,
                kernel=kernel_suffix(narrow, lazy))


def _cases():
    out = []
    # structure sweep: every structure at its lazy_below prime, lazy and reduced, and reduced at its narrow_below prime; 35 batches
    # (G = 16: two full groups and a ragged one) where 3^b <= 729, else 3; a ragged last batch
    for a, b, split in SWEEP:
        k, t, n = shape(a, b, split)
        batches = 35 if 3 ** b <= 729 else 3
        out.append(_case("sweep", k, t, n, LAZY_BELOW, batches, agree=True))
        out.append(_case("sweep", k, t, n, LAZY_BELOW, batches, knobs=(("SDA_NO_LAZY", 1),)))
        out.append(_case("sweep", k, t, n, NARROW_BELOW, batches))
    # deep lazy chains: 8 and 9 radix-3 levels
    for n in (6560, 19682):
        out.append(_case("deep", 3, 4, n, LAZY_BELOW, 3, agree=True))
    # selection edges: the four primes around the two thresholds -> lazy, reduced, reduced, wide
    for a, b in EDGES:
        k, t, n = shape(a, b)
        for which in range(4):
            out.append(_case("edge", k, t, n, which, 35 if 3 ** b <= 729 else 3))
    # group forms: (40, 23, 242) with every batches-per-workgroup form; below 8 the batch count crosses one padding unit of
    # 8 * 16 / G groups (the XCD permutation) and ends in a ragged group where G > 1; (3, 4, 6560) plans G = 2, twiddles in global memory
    for G, batches in ((16, 35), (8, 35), (4, 4 * 33 + 1), (2, 2 * 65 + 1), (1, 129)):
        out.append(_case("group", 40, 23, 242, LAZY_BELOW, batches, knobs=(("SDA_FFT_G", G),), xcd=G < 8))
    out.append(_case("group", 3, 4, 6560, LAZY_BELOW, 130, xcd=True))
    return out


CASES = _cases()


def case_roots(case):
    return root(case["p"], case["k"] + case["t"] + 1), root(case["p"], case["n"] + 1)


def specials(p):
    """the special operands of test_transform_path_modulus_bound (tests/test_parity_gpu.py)"""
    return [0, 1, p - 1, (p - 1) // 2, (p + 1) // 2, -p, p, -(1 << 62), (1 << 62) - 1]


KINDS = ("all p-1", "halves", "specials", "any i64", "canonical")

# One batch [secrets, draws] that carries the lazy chain past 2^31 where 35 batches of random operands do not: (a, b) = (3, 3), where
# 2^a <= 3^b / 3 turns the first folded level into the in[0] shortcut and leaves the chain two levels to grow in (27 outputs a
# batch; nine seeds in ten stop at 0.46 - 0.50 of 2^32).  Found once by climb_chain() - single-operand moves from a random batch,
# kept when the model's largest intermediate does not shrink - and recorded: it stands in for batch 2 of the (3, 3) cases at that prime.
CHAIN = {(268433569, 3, 3): [167762998, 152794500, 227481261, 217140464, 132198165, 16940109, 77787651]}


def climb_chain(case, steps=4000, seed=1):
    """how CHAIN was found (not run by any test): (operands, largest intermediate of the lazy model on that one batch)"""
    p, k, t, n = case["p"], case["k"], case["t"], case["n"]
    w2, w3 = case_roots(case)
    rnd = random.Random(seed)

    def score(v):
        dev = Dev(p, 32, True)
        share_transform(dev, k, t, n, w2, w3, v[:k], v[k:])
        return max(dev.maxima.values())
    best = [rnd.randrange(p) for _ in range(k + t)]
    top = score(best)
    for _ in range(steps):
        v, i = list(best), rnd.randrange(k + t)
        v[i] = rnd.randrange(p) if rnd.random() < .5 else (v[i] + rnd.randrange(-(p >> rnd.randrange(4, 28)), (p >> rnd.randrange(4, 28)) + 1)) % p
        if score(v) >= top:
            best, top = v, score(v)
    return best, top


def batch_kind(case, b):
    """which operands batch b holds: the first two are the fixed patterns, the others take the three random kinds in turn (with
    three batches, the last one mixes them element by element); batch 2 is the recorded chain batch where the case has one"""
    if b < 2:
        return KINDS[b]
    if b == 2 and (case["p"], case["a"], case["b"]) in CHAIN:
        return "chain"
    return "mixed" if case["batches"] == 3 else KINDS[2 + (b - 2) % 3]


def inputs(case):
    """(secrets [dim], draws [batches * t]) as python ints in [-2^62, 2^62): any-i64 operands, the kernel canonicalises them"""
    p, k, t, B = case["p"], case["k"], case["t"], case["batches"]
    rnd = random.Random(f"{p}/{k}/{t}/{case['n']}/{B}")
    sp = specials(p)
    draw = {"specials": lambda: sp[rnd.getrandbits(16) % len(sp)], "any i64": lambda: rnd.getrandbits(63) - (1 << 62),
            "canonical": lambda: rnd.getrandbits(64) % p}
    sec, dr = [], []
    for b in range(B):
        kind = batch_kind(case, b)
        if kind == "chain":
            v = CHAIN[(p, case["a"], case["b"])]
            sec += v[:k]
            dr += v[k:]
            continue
        for dst, cnt, half in ((sec, k, (p - 1) // 2), (dr, t, (p + 1) // 2)):
            for i in range(cnt):
                if kind == "all p-1":
                    dst.append(p - 1)
                elif kind == "halves":
                    dst.append(half)
                else:
                    dst.append(draw[KINDS[2 + i % 3] if kind == "mixed" else kind]())
    return sec[:case["dim"]], dr


def batch_values(case, sec, dr, b):
    """the k secrets (zero padded, batched.rs:37-43) and t draws of batch b"""
    k, t = case["k"], case["t"]
    s = sec[b * k:(b + 1) * k]
    return s + [0] * (k - len(s)), dr[b * t:(b + 1) * t]


def model_batches(case):
    """the batches the CPU model runs: all of them, except for the two long group jobs (one value of the plan each, the same
    arithmetic in every batch), where the two fixed patterns, one batch of each random kind and the last batch do"""
    B = case["batches"]
    return list(range(B)) if B <= 35 else [0, 1, 2, 3, 4, B - 1]


def run_model(case):
    """(shares of the modelled batches {b: [n]}, per-stage maxima) - the instantiation the plan names"""
    dev = Dev(case["p"], 32 if case["narrow"] else 64, case["lazy"])
    w2, w3 = case_roots(case)
    sec, dr = inputs(case)
    out = {}
    for b in model_batches(case):
        s, r = batch_values(case, sec, dr, b)
        out[b] = share_transform(dev, case["k"], case["t"], case["n"], w2, w3, s, r)
    return out, dict(dev.maxima)


def coverage(case):
    """the branches of the kernel and its launcher this case runs, by name"""
    a, b, G = case["a"], case["b"], case["G"]
    m2, m3 = 1 << a, 3 ** b
    nz = nz_mask(m2, m3)
    got = {"a odd" if a & 1 else "a even", "b-2 odd" if (b - 2) & 1 else "b-2 even", f"G={G}", f"tw_lds={case['tw_lds']}",
           "lazy" if case["lazy"] else "reduced" if case["narrow"] else "wide"}
    if a - (a & 1) >= 4:
        got.add("radix-4 pass with qd > 1")
    if a >= 2:
        got.add("last radix-4 pass (qd == 1)")
    got.add("zero extension: m2 <= m3/9" if 9 * m2 <= m3 else "zero extension: m3/9 < m2 <= m3/3" if 3 * m2 <= m3 else "zero extension: m3/3 < m2")
    if any(not (nz[1][e1] or nz[2][e1]) for e1 in range(3)):
        got.add("in[0] shortcut")
    if any(nz[1][e1] or nz[2][e1] for e1 in range(3)):
        got.add("first-level butterfly")
    if b >= 6:
        got.add("non-last radix-9 pass")
    got.add("radix-9 output path" if b >= 4 else "LDS output path")
    groups = -(-case["batches"] // G)
    if G < 8 and groups > 8 * (16 // G):
        got.add("more than one padding unit")
    if case["batches"] % G:
        got.add("ragged group")
    if case["dim"] % case["k"]:
        got.add("ragged batch")
    return got


# ---- recorded reach ----------------------------------------------------------------------------------------------------------------
# The largest register value of each stage (radix-2 part, folded levels, later levels, final reduction) over the modelled batches of
# each case, as a fraction of 2^32 cut to six places (never rounded up to 1); tests/test_transform_limits_reach.py asserts the table exactly (the
# inputs are seeded, the model is integer arithmetic).  print_reach() regenerates it.
def fractions(maxima):
    return tuple((maxima[s] * 10 ** 6 >> 32) / 10 ** 6 for s in STAGES)


def print_reach():
    for c in CASES:
        if c["narrow"]:
            print(f'    "{c["name"]}": {fractions(run_model(c)[1])},')


REACH = {
    "sweep-a2b2-k2t1n8-lazy_below": (0.323267, 0.634558, 0.0, 0.634558),
    "sweep-a2b2-k2t1n8-lazy_below-NO_LAZY": (0.323267, 0.328291, 0.0, 0.31519),
    "sweep-a2b2-k2t1n8-narrow_below": (0.870689, 0.968379, 0.0, 0.82958),
    "sweep-a3b2-k3t4n8-lazy_below": (0.333332, 0.636277, 0.0, 0.636277),
    "sweep-a3b2-k3t4n8-lazy_below-NO_LAZY": (0.333332, 0.313146, 0.0, 0.31284),
    "sweep-a3b2-k3t4n8-narrow_below": (0.999999, 0.968749, 0.0, 0.907595),
    "sweep-a3b3-k6t1n26-lazy_below": (0.249998, 0.297909, 0.521204, 0.521204),
    "sweep-a3b3-k6t1n26-lazy_below-NO_LAZY": (0.249998, 0.236481, 0.241494, 0.23534),
    "sweep-a3b3-k6t1n26-narrow_below": (0.999998, 0.894826, 0.964036, 0.855073),
    "sweep-a4b3-k2t13n26-lazy_below": (0.249998, 0.469948, 0.649578, 0.649578),
    "sweep-a4b3-k2t13n26-lazy_below-NO_LAZY": (0.249998, 0.241722, 0.24743, 0.24161),
    "sweep-a4b3-k2t13n26-narrow_below": (0.999996, 0.952796, 0.939153, 0.890808),
    "sweep-a4b4-k8t7n80-lazy_below": (0.19999, 0.234445, 0.551846, 0.551846),
    "sweep-a4b4-k8t7n80-lazy_below-NO_LAZY": (0.19999, 0.19269, 0.197242, 0.193295),
    "sweep-a4b4-k8t7n80-narrow_below": (0.99999, 0.949439, 0.971252, 0.971252),
    "sweep-a5b4-k9t22n80-lazy_below": (0.199989, 0.403426, 0.725492, 0.725492),
    "sweep-a5b4-k9t22n80-lazy_below-NO_LAZY": (0.199989, 0.199584, 0.199584, 0.197051),
    "sweep-a5b4-k9t22n80-narrow_below": (0.999989, 0.990299, 0.982043, 0.963654),
    "sweep-a6b4-k44t19n80-lazy_below": (0.199989, 0.385045, 0.704103, 0.704103),
    "sweep-a6b4-k44t19n80-lazy_below-NO_LAZY": (0.199989, 0.197326, 0.197736, 0.194227),
    "sweep-a6b4-k44t19n80-narrow_below": (0.999989, 0.973388, 0.984355, 0.97545),
    "sweep-a6b5-k32t31n242-lazy_below": (0.166608, 0.201261, 0.590212, 0.590212),
    "sweep-a6b5-k32t31n242-lazy_below-NO_LAZY": (0.166608, 0.165409, 0.165409, 0.163834),
    "sweep-a6b5-k32t31n242-narrow_below": (0.999695, 0.9591, 0.993437, 0.963258),
    "sweep-a7b5-k25t102n242-lazy_below": (0.166391, 0.360699, 0.706669, 0.706669),
    "sweep-a7b5-k25t102n242-lazy_below-NO_LAZY": (0.166391, 0.165091, 0.164667, 0.162315),
    "sweep-a7b5-k25t102n242-narrow_below": (0.999593, 0.991784, 0.992344, 0.921111),
    "sweep-a7b6-k76t51n728-lazy_below": (0.142782, 0.173052, 0.62851, 0.62851),
    "sweep-a7b6-k76t51n728-lazy_below-NO_LAZY": (0.142782, 0.141892, 0.142217, 0.141482),
    "sweep-a7b6-k76t51n728-narrow_below": (0.998, 0.990646, 0.997206, 0.994469),
    "sweep-a8b6-k99t156n728-lazy_below": (0.141479, 0.30111, 0.692036, 0.692036),
    "sweep-a8b6-k99t156n728-lazy_below-NO_LAZY": (0.141479, 0.140573, 0.14054, 0.138925),
    "sweep-a8b6-k99t156n728-narrow_below": (0.998, 0.990852, 0.99446, 0.99367),
    "sweep-a9b6-k256t255n728-lazy_below": (0.141479, 0.291625, 0.698283, 0.698283),
    "sweep-a9b6-k256t255n728-lazy_below-NO_LAZY": (0.141479, 0.141202, 0.141137, 0.13887),
    "sweep-a9b6-k256t255n728-narrow_below": (0.998, 0.996667, 0.99664, 0.993624),
    "sweep-a9b7-k256t255n2186-lazy_below": (0.119926, 0.140459, 0.578521, 0.578521),
    "sweep-a9b7-k256t255n2186-lazy_below-NO_LAZY": (0.119926, 0.117081, 0.119645, 0.116355),
    "sweep-a9b7-k256t255n2186-narrow_below": (0.998, 0.988993, 0.994288, 0.983915),
    "sweep-a10b7-k256t767n2186-lazy_below": (0.112627, 0.233755, 0.593315, 0.593315),
    "sweep-a10b7-k256t767n2186-lazy_below-NO_LAZY": (0.112627, 0.112517, 0.111885, 0.111861),
    "sweep-a10b7-k256t767n2186-narrow_below": (0.974015, 0.973064, 0.958181, 0.886859),
    "deep-a3b8-k3t4n6560-lazy_below": (0.110525, 0.110535, 0.528993, 0.528993),
    "deep-a3b9-k3t4n19682-lazy_below": (0.097522, 0.096551, 0.515005, 0.515005),
    "edge-a2b2-k2t1n8-lazy_below": (0.323267, 0.634558, 0.0, 0.634558),
    "edge-a2b2-k2t1n8-lazy_above": (0.319194, 0.326831, 0.0, 0.326831),
    "edge-a2b2-k2t1n8-narrow_below": (0.870689, 0.968379, 0.0, 0.82958),
    "edge-a3b3-k4t3n26-lazy_below": (0.249998, 0.299534, 0.521204, 0.521204),
    "edge-a3b3-k4t3n26-lazy_above": (0.250001, 0.244872, 0.246958, 0.246958),
    "edge-a3b3-k4t3n26-narrow_below": (0.999998, 0.901368, 0.963195, 0.888086),
    "edge-a3b5-k4t3n242-lazy_below": (0.166664, 0.166629, 0.533214, 0.533214),
    "edge-a3b5-k4t3n242-lazy_above": (0.166682, 0.127349, 0.165079, 0.165079),
    "edge-a3b5-k4t3n242-narrow_below": (0.999977, 0.780659, 0.980558, 0.976545),
    "edge-a3b9-k4t3n19682-lazy_below": (0.097522, 0.094766, 0.516384, 0.516384),
    "edge-a3b9-k4t3n19682-lazy_above": (0.101188, 0.073142, 0.100644, 0.100552),
    "edge-a3b9-k4t3n19682-narrow_below": (0.999711, 0.718542, 0.990568, 0.93918),
    "group-a6b5-k40t23n242-lazy_below-FFT_G16": (0.166608, 0.206136, 0.596179, 0.596179),
    "group-a6b5-k40t23n242-lazy_below-FFT_G8": (0.166608, 0.206136, 0.596179, 0.596179),
    "group-a6b5-k40t23n242-lazy_below-FFT_G4": (0.166608, 0.195668, 0.590212, 0.590212),
    "group-a6b5-k40t23n242-lazy_below-FFT_G2": (0.166608, 0.200439, 0.590212, 0.590212),
    "group-a6b5-k40t23n242-lazy_below-FFT_G1": (0.166608, 0.197079, 0.590212, 0.590212),
    "group-a3b8-k3t4n6560-lazy_below": (0.110525, 0.110628, 0.534776, 0.534776),
}

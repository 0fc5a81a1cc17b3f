"""Big-int model of the transform form of packed-Shamir share generation (sda_amd/csrc/fft_kernels.hip, round 3): tss's
own algorithm - radix-2 inverse transform over the k+t+1 secret nodes, zero-extension, radix-3 forward transform over the
n+1 share points (packed_shamir.rs:42 -> tss `share`) - on lazily reduced UNSIGNED 64-bit values with
Shoup multiplications by table constants, in exactly the kernel's order: a single radix-2 level when their number is odd,
then radix-4 passes; the first two radix-3 levels folded into the zero-extending scatter; a single radix-3 level when the
rest is odd, then radix-9 passes.  Checks exactness against the oracle's FFT / matrix / Lagrange forms and that every
intermediate fits the 64-bit register (and the [0, 2p) / [0, 4p) range) the kernel keeps it in.  The model itself lives in
tests/transform_limits.py, which also runs it at register width 32 (reduced and lazy).  CPU only."""
import random

import pytest

from oracle import pyoracle as po

from transform_limits import M64, Dev, share_transform      # the ONE whole-kernel model (wide here; 32-bit: test_transform_limits_reach.py)


def _roots(p, o2, o3):
    g = next(g for g in range(2, 500) if all(pow(g, (p - 1) // f, p) != 1 for f in (2, 3)))
    return pow(g, (p - 1) // o2, p), pow(g, (p - 1) // o3, p)


@pytest.mark.parametrize("p,k,t,n", [(433, 3, 4, 8), (po.P62, 3, 4, 8), (po.P62, 8, 7, 26), (po.P62, 1, 2, 8),
                                     (po.P62, 20, 11, 80), (746497, 100, 155, 728), (po.P62, 40, 23, 242),
                                     (po.P62, 70, 57, 242), (po.P62, 2, 1, 26), (po.P62, 1, 0, 8)])
def test_transform_share_equals_the_oracle(p, k, t, n):
    """shapes cover: an odd and an even number of radix-2 levels (single level + radix-4 passes), 0 / 1 / 2 / 3 / 4 radix-3
    levels after the folded two (single level, radix-9 passes), and every zero-extension pattern of the first levels
    (m2 <= m3/9, m3/9 < m2 <= m3/3, m3/3 < m2 <= 2 m3/3 incl. tss's 256 of 729)"""
    rnd = random.Random(k * 1000 + n)
    if p == 433:
        w2, w3 = 354, 150
    elif p == 746497 and n == 728:
        w2, w3 = 95660, 610121                                                      # tss PSS_155_728_100 [recalled]
    else:
        w2, w3 = _roots(p, k + t + 1, n + 1)
    dev = Dev(p)
    pss = po.PackedSecretSharing(t, n, k, p, w2, w3)
    assert pss.is_fft_shape()
    special = [0, 1, p - 1, (p - 1) // 2, (p + 1) // 2]
    reps = (1 if n > 300 else 3) if n > 100 else 40
    Mx = pss.share_matrix() if n <= 100 else None
    for it in range(reps):
        if it == 0:
            s, r = [p - 1] * k, [p - 1] * t
        elif it == 1:
            s, r = [(p - 1) // 2] * k, [(p + 1) // 2] * t
        else:
            s = [rnd.choice(special + [rnd.randrange(p)] * 3) for _ in range(k)]
            r = [rnd.choice(special + [rnd.randrange(p)] * 3) for _ in range(t)]
        got = share_transform(dev, k, t, n, w2, w3, s, r)
        want = [v % p for v in pss.share_fft(s, r, "canonical")] if p < (1 << 31) else None
        if Mx is not None:
            mat = [sum(a * b for a, b in zip(row, s + r)) % p for row in Mx]
            assert got == mat
            if want is not None:
                assert want == mat
        elif want is not None:
            assert got == want
        else:
            # large prime, large shape: Lagrange evaluation at three share points (independent of any transform)
            lag = pss.share_lagrange(s, r)
            for j in (1, n // 2, n):
                assert got[j - 1] == lag[j - 1]


def _prime_below(x):
    x -= 1 - (x & 1)
    while not all(pow(a, x - 1, x) == 1 for a in (2, 3, 5, 7, 11, 13, 17)):
        x -= 2
    return x


@pytest.mark.parametrize("p", [_prime_below(1 << 62), po.P62, 433, 2])
def test_multiplication_and_butterfly_ranges_at_the_edges(p):
    """the Shoup product accepts ANY 64-bit operand and lands in [0, 2p); the butterfly keeps every sum inside 64 bits -
    for the largest modulus the library admits (p just below 2^62: 4p just below 2^64) and for tiny ones"""
    dev = Dev(p)
    rnd = random.Random(p & 0xFFFF)
    consts = [0, 1, p - 1, p // 2] + [rnd.randrange(p) for _ in range(40)]
    xs = [0, 1, p - 1, p, 2 * p - 1, 2 * p, 4 * p - 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1] + [rnd.getrandbits(64) for _ in range(60)]
    for w in consts:
        c = dev.pair(w)
        for x in xs:
            r = dev.mulS(x & M64, c)
            assert r % p == (x & M64) * w % p
    om = dev.pair(consts[5])                                   # range checks do not need a true cube root
    edge = [0, 1, 2 * p - 1, p, p - 1] + [rnd.randrange(2 * p) for _ in range(8)]
    for A in edge:
        for Bv in edge:
            for Cv in edge:
                y = dev.r3(A, Bv, Cv, om)
                w = om[0]
                assert y[0] % p == (A + Bv + Cv) % p
                assert y[1] % p == (A - Cv + w * (Bv - Cv)) % p
                assert y[2] % p == (A - Bv - w * (Bv - Cv)) % p

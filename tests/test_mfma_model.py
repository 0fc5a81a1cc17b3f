"""Big-int model of the 62-bit limb GEMM (packed_gen_mfma_kernel / fused_packed_mfma_kernel, sda_amd/csrc/sda_kernels.hip) in the
kernel's own order: constants in Montgomery form (R = 2^64), centred, as balanced bytes zero padded to 8 ceil((k+t)/8) terms
(mfma_place_matrix); values canon -> centred -> balanced bytes; the 15 Toeplitz columns as i8 x i8 products in i32 over KS steps
of 64 slots; the per-tile v_mad_i64_i32 chain with mul3; the 128-bit assembly of mfma_clerk_finish exactly as written; the
signed REDC.  Every register width and stated range is asserted (tests/extremes.py, mfma_share) and the result compared with
the plain modular dot product, for both share maps, every compiled shape and the run-time shapes, random and extreme operands."""
import random

import pytest

import extremes as X

PRIMES = [3, 433, X.P31MAX, X.P62, X.PMAX]
COMPILED = [(8, 7), (8, 2), (3, 4), (3, 1), (12, 3), (10, 5), (4, 11)]
RUNTIME = [(9, 0), (5, 4), (2, 9), (9, 6), (13, 2), (1, 14), (16, 0), (7, 9), (11, 5)]        # k + t from 9 to 16


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    from oracle import coracle
    coracle.build()


def _rows(p, k, t, n, systematic):
    if p == 3:                      # no distinct nodes at p = 3: a synthetic matrix (the model does not care where rows come from)
        rng = random.Random(k * 100 + t)
        return [[rng.randrange(p) for _ in range(k + t)] for _ in range(4)]
    w2, w3 = X.omegas(p, k, t, n)
    return X.share_matrix(p, k, t, n, w2, w3, systematic)


def _check(p, rows, batches, rng):
    C = X.family_constants("mfma", rows, p)
    kt = len(rows[0])
    vals = X.crafted_rows("mfma", C, p, batches)
    h = (p - 1) // 2
    vals += [[rng.randrange(p) for _ in range(kt)] for _ in range(batches // 2)]
    vals += [[rng.choice([0, 1, h, h + 1, p - 1]) for _ in range(kt)] for _ in range(batches // 4)]
    for b, v in enumerate(vals):
        r = b % len(rows) if b >= batches else X.target("mfma", b, len(rows))[1]
        X.mfma_share(rows[r], [x % p for x in v], p)


@pytest.mark.parametrize("p", PRIMES)
@pytest.mark.parametrize("k,t", COMPILED + RUNTIME)
@pytest.mark.parametrize("systematic", [False, True])
def test_limb_gemm_model_exact(p, k, t, systematic):
    if p < k + t + 2 and p != 3:
        pytest.skip("fewer residues than interpolation nodes")
    if systematic and t == 0:
        return                     # no systematic map without draws: tss's map is the only one (covered by systematic=False)
    n = 26 if k + t > 8 else 8
    if p == 433 and n + k + t + 1 > 432:
        n = 8
    rows = _rows(p, k, t, n, systematic and p != 3)
    _check(p, rows, X.NPAT * len(rows) * (2 if p > 3 else 1), random.Random(p ^ (k << 8) ^ (t << 16)))


@pytest.mark.parametrize("p", [X.P62, X.PMAX])
def test_limb_gemm_model_242_clerks(p):
    """the largest constant table (n = 242): one sign-aligned batch per row and every row's digit-extreme batch for one column"""
    k, t, n = 8, 7, 242
    w2, w3 = X.omegas(p, k, t, n)
    for systematic in (False, True):
        rows = X.share_matrix(p, k, t, n, w2, w3, systematic)
        C = X.family_constants("mfma", rows, p)
        vals = X.crafted_rows("mfma", C, p, X.NPAT * len(rows))
        for b, v in enumerate(vals):
            X.mfma_share(rows[X.target("mfma", b, len(rows))[1]], [x % p for x in v], p)


def test_column_bounds_of_the_digit_ranges():
    # centred residues of p < 2^62 have |x| <= 2^61 - 1: their top digit lies in [-32, 32], so no column reaches 2^21
    assert X.digit_range(X.PMAX) == [128] * 7 + [32]
    assert X.column_bound(16, X.PMAX) == 16 * 7 * 128 * 128 < 1 << 21
    assert X.digit_range(433) == [128, 1, 0, 0, 0, 0, 0, 0]
    rng = random.Random(1)
    for p in PRIMES:
        r = X.digit_range(p)
        for v in [0, 1, p - 1, p // 2, p // 2 + 1] + [rng.randrange(p) for _ in range(5000)]:
            d = X.balanced_digits(X.centred(v, p))
            assert all(abs(a) <= b for a, b in zip(d, r)), (p, v, d)
            assert sum(a << (8 * i) for i, a in enumerate(d)) == X.centred(v, p)

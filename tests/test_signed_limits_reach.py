"""Reach checks for the case tables of tests/test_signed_limits_gpu.py (CPU, no device).

For every case: which of trunc_rem128's four branches and which of the fifteen boundary points its dividends take (written out
here, so a table that moves off a boundary fails by name); that the kernel model of tests/signed_limits.py - restated from the
kernel text - equals oracle.pyoracle in rust_signed mode; that every expected value fits int64; and that the expectation holds
negative values and differs from the canonical residues, so a route that silently fell back to a canonical kernel fails on the GPU.

One point is out of reach of one table by arithmetic and is asserted so: a difference of two int64 is at least
INT64_MIN - INT64_MAX = -2^64 + 1, so the generate fold (acc - r) and unmask (a - b) cannot form -2^64; mask (a + b) forms it, and
cannot form 2^64 - 1.  The add and the subtract table together take all fifteen."""
import pytest

import signed_limits as SL
from oracle import pyoracle as po

ids = lambda q: f"q{q}"


def _fit_and_tell(values, q):
    assert all(SL.fits(v) for v in values)
    assert SL.tells_signed_from_canonical(values, q)


@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_specials(q):
    sp = SL.specials(q)
    assert 16 <= len(sp) <= 27 and len(set(sp)) == len(sp) and all(SL.fits(v) for v in sp)
    assert len(sp) == {2: 22, 3: 26, 433: 27, 1 << 61: 23, (1 << 62) - 57: 23, (1 << 62) - 1: 16}[q]
    for v in (0, 1, -1, q, -q, q - 1, 1 - q, SL.MIN, SL.MIN + 1, SL.MAX, SL.MAX - 1, 1 << 62, -(1 << 62), SL.MAX // q * q, -(SL.MAX // q * q)):
        assert v in sp, v
    assert [SL.branch(x, q) for x in (0, q - 1, 1 - q, q, 2 * q - 1, -q, 1 - 2 * q, 2 * q, -2 * q, SL.MIN - SL.MAX)] == \
           ["near", "near", "near", "high", "high", "low", "low", "far", "far", "far"]
    assert SL.MIN - SL.MAX == -(1 << 64) + 1 and SL.MIN + SL.MIN == -(1 << 64) and SL.MAX - SL.MIN == (1 << 64) - 1


@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_add_and_subtract_table(q):
    a, b = SL.pair_table(q)
    assert len(a) == len(SL.specials(q)) ** 2 <= 729
    sub, add = SL.Reach(q), SL.Reach(q)
    diff = SL.model_addsub(a, b, True, q, sub)
    summ = SL.model_addsub(a, b, False, q, add)
    assert sub.branches == add.branches == set(SL.BRANCHES)
    assert sub.points == set(SL.POINTS) - {"-2^64"} and add.points == set(SL.POINTS) - {"2^64-1"}
    assert sub.points | add.points == set(SL.POINTS) and len(SL.POINTS) == 15
    fm = po.FullMasker(q, "rust_signed")
    assert fm.unmask(b, a) == diff                                     # unmask(mask, masked) = (masked - mask) % q
    assert fm.mask(a, b) == (b, summ)
    _fit_and_tell(diff, q)
    _fit_and_tell(summ, q)
    # the answers that separate Rust's `%` from a canonical reduction are in the expectation
    at = {(u, v): d for u, v, d in zip(a, b, diff)}
    assert at[(-q, 0)] == 0 and at[(-q, q)] == 0 and at[(0, q - 1)] == 1 - q and at[(SL.MIN, SL.MAX)] == -(((1 << 64) - 1) % q)


@pytest.mark.parametrize("n", SL.GEN_N)
@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_generate_table(q, n):
    secrets, rand = SL.generate_table(q, n)
    assert len(rand) == len(secrets) * (n - 1)
    reach = SL.Reach(q)
    out = SL.model_generate(secrets, rand, n, q, reach)
    if n == 1:                                                         # no draws: the share is the raw, unreduced secret
        assert out == [secrets] and not reach.branches
    else:
        assert reach.branches == set(SL.BRANCHES) and reach.points == set(SL.POINTS_OF_A_DIFFERENCE)
        assert len(SL.POINTS_OF_A_DIFFERENCE) == 14
    assert po.generate(po.AdditiveSecretSharing(n, q, "rust_signed"), secrets, rand) == out
    for p in (1, 2):                                                   # the other participants of the device call
        s2, r2 = SL.generate_rolled(q, n, 101 * p)
        assert sorted(s2) == sorted(secrets) and po.generate(po.AdditiveSecretSharing(n, q, "rust_signed"), s2, r2) == SL.model_generate(s2, r2, n, q)
    for row in out:
        assert all(SL.fits(v) for v in row)
    _fit_and_tell(out[n - 1], q)


@pytest.mark.parametrize("q", SL.BIG_JOB_MODULI, ids=ids)
def test_generate_job_beyond_one_grid(q):
    P, dim, n = SL.BIG_JOB
    assert P > 65535 and n == 2
    secrets, rand = SL.grid_pairs(q, P * dim)
    reach = SL.Reach(q)
    out = SL.model_generate(secrets, rand, n, q, reach)
    assert reach.branches == set(SL.BRANCHES) and reach.points == set(SL.POINTS_OF_A_DIFFERENCE)
    assert out[1] == po.FullMasker(q, "rust_signed").unmask(rand, secrets)      # one step of the fold is (s - r) % q
    tail = out[1][65535 * dim:]                                        # the second launch has its own negatives
    _fit_and_tell(tail, q)
    _fit_and_tell(out[1], q)


@pytest.mark.parametrize("shift", (0, 50, 100))
@pytest.mark.parametrize("dim", SL.COMBINE_DIMS)
@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_combine_table(q, dim, shift):
    rows = [list(r) for r in SL.combine_table(q, dim, shift)]
    assert len(rows) == 2 + SL.COMBINE_RANDOM_ROWS == 39 and all(len(r) == dim for r in rows)
    assert set(rows[0]) <= set(SL.combine_firsts(q)) and all(abs(v) < q for v in rows[0])
    reach, second = SL.Reach(q), {1: SL.Reach(q)}
    out = SL.model_combine(rows, q, None, reach, second)
    if dim >= 255:                                                     # every pair of first row x second row is a column
        assert len(SL.combine_firsts(q)) * len(SL.specials(q)) <= dim
        assert second[1].points >= set(SL.COMBINE_BOUNDARIES) and reach.branches == set(SL.BRANCHES)
    assert po.combine(rows, q, "rust_signed") == out
    assert po.FullMasker(q, "rust_signed").combine(rows) == out
    assert po.AdditiveSecretSharing(3, q, "rust_signed").reconstruct(list(enumerate(rows))) == out
    for k in range(len(rows) + 1) if (dim, shift) == (257, 0) else (): # the streaming form: the state carries over a split
        assert SL.model_combine(rows[k:], q, SL.model_combine(rows[:k], q) if k else None) == out
    _fit_and_tell(out, q)


@pytest.mark.parametrize("dim", SL.CHACHA_DIMS)
@pytest.mark.parametrize("q", [q for q in SL.MODULI if q >= 3], ids=ids)
def test_chacha_cases(q, dim):
    cm = po.ChaChaMasker(q, dim, 128, "rust_signed")
    secrets = SL.cycle(q, dim)
    mask = cm.expand(SL.CHACHA_SEED)
    assert all(0 <= m < q for m in mask)
    seed, masked = cm.mask(secrets, SL.CHACHA_SEED)
    assert seed == list(SL.CHACHA_SEED) and masked == SL.model_addsub(secrets, mask, False, q)
    _fit_and_tell(masked, q)
    a, b = SL.cycle(q, dim), SL.cycle(q, dim, SL.MAX - 1)          # (MIN - MAX is a multiple of 3)
    assert cm.unmask(b, a) == SL.model_addsub(a, b, True, q)
    _fit_and_tell(cm.unmask(b, a), q)


@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_own_draw_cases(q):
    """the library's draws are in [0, q): INT64_MIN + mask stays negative, and any mask of that range leaves the sum in int64"""
    secrets = SL.cycle(q, 600)
    assert secrets[0] == SL.MIN and set(secrets) == set(SL.specials(q))
    for mask in ([0] * 600, [q - 1] * 600):
        _fit_and_tell(SL.model_addsub(secrets, mask, False, q), q)
        _fit_and_tell(SL.model_generate(secrets, mask, 2, q)[1], q)


@pytest.mark.parametrize("n", SL.DRBG_N)
@pytest.mark.parametrize("dim", SL.DRBG_DIMS)
@pytest.mark.parametrize("q", SL.DRBG_MODULI, ids=ids)
def test_csprng_cases(q, dim, n):
    """the library's draws (sda-drbg-v1, from the C oracle; pinned against pyoracle's restatement on the first elements) leave
    negative last shares in every case, for the key and the stream ids the GPU test uses"""
    from oracle import coracle
    lasts, reach = [], SL.Reach(q)
    for p, secrets in enumerate(SL.drbg_secrets(q, dim)):
        assert len(secrets) == dim and secrets[0] < 0
        draws = [int(v) for v in coracle.drbg_fill(SL.DRBG_KEY, SL.DRBG_FIRST + p, dim, n - 1, q)]
        assert all(0 <= r < q for r in draws)
        head = min(dim, 3)
        assert draws[:head * (n - 1)] == [po.drbg_value(SL.DRBG_KEY, SL.DRBG_FIRST + p, b, n - 1, i, q) for b in range(head) for i in range(n - 1)]
        out = SL.model_generate(secrets, draws, n, q, reach)
        assert out == po.generate(po.AdditiveSecretSharing(n, q, "rust_signed"), secrets, draws)
        assert all(SL.fits(v) for v in out[n - 1])
        lasts += out[n - 1]
    assert SL.DRBG_FIRST + 2 == 1 << 56                                # the last two stream ids the library admits
    assert "far" in reach.branches and (dim < 511 or reach.branches == set(SL.BRANCHES))
    _fit_and_tell(lasts, q)

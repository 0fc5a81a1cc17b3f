"""The reference-representative kernels (SDA_VALUES_RUST_SIGNED) at the limits of int64, bit-exact against Python integers (pytest -m gpu).

signed_kernels.hip promises "inputs may be ANY i64 ... sums are formed in 128 bits"; the other tests of the mode feed operands
inside +-2^62 that land on none of trunc_rem128's branch boundaries.  Here every operand comes from tests/signed_limits.py:
specials(q) - the values at and around +-q, +-2q, +-(2q - 1), the ends of int64, the last multiples of q - for the moduli 2, 3,
433, 2^61, 2^62 - 57 and 2^62 - 1 (the largest make_mod admits), through every entry point that routes to signed_addsub_kernel,
signed_combine_update_kernel, signed_additive_gen_kernel and signed_additive_gen_drbg_kernel.  Expected values are
oracle.pyoracle's in rust_signed mode (every sum exact), the library's draws come from coracle.drbg_fill.
tests/test_signed_limits_reach.py proves on the CPU which branches and boundaries each table takes and that every expectation
holds negative values - a route that fell back to a canonical kernel fails here."""
import functools

import numpy as np
import pytest

import signed_limits as SL

pytestmark = pytest.mark.gpu

KEY = SL.DRBG_KEY
GUARD = 0x5A5A5A5A5A5A5A5A
SIGNED = "rust_signed"
ids = lambda q: f"q{q}"


def _np(values):
    return np.array(values, dtype=np.int64)


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.int64).reshape(-1), _np(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {int(bad[0])}: got {int(got[bad[0]])}, expected {int(want[bad[0]])}"


def _last_kernel():
    from sda_amd import capi
    return capi.load().sda_debug_last_kernel().decode()


def _po():
    from oracle import pyoracle as po
    return po


# ---- signed_addsub_kernel ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_expect(q):
    a, b = SL.pair_table(q)
    fm = _po().FullMasker(q, SIGNED)
    return _np(a), _np(b), fm.unmask(b, a), fm.mask(a, b)[1]


@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_unmask_on_every_pair_of_specials(gpu, q):
    """(a - b) % q over specials(q)^2: host form and unmask_dev (inputs left as they were, nothing stored behind the output)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    a, b, diff, _ = _pair_expect(q)
    um = crypto.SecretUnmasker(crypto.Full(q)).set_value_mode(SIGNED)
    _same(um.unmask((b, a)), diff, "unmask")
    d_a, d_b = DeviceBuffer.from_numpy(a), DeviceBuffer.from_numpy(b)
    d_out = DeviceBuffer.from_numpy(np.full(a.size + 8, GUARD, dtype=np.int64))
    um.unmask_dev(d_b.ptr, d_a.ptr, a.size, d_out.ptr)
    out = d_out.to_numpy()
    _same(out[:a.size], diff, "unmask_dev")
    assert (out[a.size:] == GUARD).all() and np.array_equal(d_a.to_numpy(), a) and np.array_equal(d_b.to_numpy(), b)


@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_full_mask_with_injected_draws_on_every_pair_of_specials(gpu, q):
    """(a + b) % q over specials(q)^2; the mask is returned as given (full.rs:25-30), unreduced"""
    from sda_amd import crypto
    a, b, _, summ = _pair_expect(q)
    mask, masked = crypto.SecretMasker(crypto.Full(q)).set_value_mode(SIGNED).mask(a, b)
    _same(mask, b, "mask")
    _same(masked, summ, "masked secrets")


@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_full_mask_with_the_librarys_own_draws(gpu, q):
    """sda_secret_masker_mask without rand: launch_full_mask_drbg draws the mask, the signed sum is re-added with addsub - the
    mask lies in [0, q), the masked values are trunc_rem(secret + mask) on special secrets, INT64_MIN and INT64_MAX included"""
    from sda_amd import crypto
    secrets = SL.cycle(q, 600)
    m = crypto.SecretMasker(crypto.Full(q)).set_value_mode(SIGNED)
    m.set_drbg_key(KEY)
    mask, masked = m.mask(_np(secrets))
    mask = [int(v) for v in mask]
    assert len(mask) == 600 and all(0 <= v < q for v in mask)
    want = _po().FullMasker(q, SIGNED).mask(secrets, mask)[1]
    assert SL.tells_signed_from_canonical(want, q)
    _same(masked, want, "masked secrets")


@pytest.mark.parametrize("dim", SL.CHACHA_DIMS)
@pytest.mark.parametrize("q", [q for q in SL.MODULI if q >= 3], ids=ids)
def test_chacha_mask_and_unmask(gpu, q, dim):
    from sda_amd import crypto
    cm = _po().ChaChaMasker(q, dim, 128, SIGNED)
    secrets = SL.cycle(q, dim)
    seed, masked = crypto.SecretMasker(crypto.ChaCha(q, dim, 128)).set_value_mode(SIGNED).mask(_np(secrets), list(SL.CHACHA_SEED))
    wseed, wmasked = cm.mask(secrets, list(SL.CHACHA_SEED))
    _same(seed, wseed, "seed")
    _same(masked, wmasked, "masked secrets")
    a, b = SL.cycle(q, dim), SL.cycle(q, dim, SL.MAX - 1)
    um = crypto.SecretUnmasker(crypto.ChaCha(q, dim, 128)).set_value_mode(SIGNED)
    _same(um.unmask((_np(b), _np(a))), cm.unmask(b, a), "unmask")


# ---- signed_combine_update_kernel ----------------------------------------------------------------------------------------------------------
JOBS, SPLIT = 3, 20


@functools.lru_cache(maxsize=None)
def _combine_case(q, dim, shift=0):
    rows = SL.combine_table(q, dim, shift)
    return np.array(rows, dtype=np.int64), _po().combine([list(r) for r in rows], q, SIGNED)


@pytest.mark.parametrize("dim", SL.COMBINE_DIMS)
@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_share_combiner_host_forms(gpu, q, dim):
    """combine() under an Additive and a PackedShamir scheme (the combiner's mode covers both), and begin / update / finish split
    after every row count: the running values carry their signs from one update to the next"""
    from sda_amd import crypto
    mat, want = _combine_case(q, dim)
    for sch in (crypto.Additive(3, q), crypto.PackedShamir(3, 8, 4, q, 2, 3)):
        comb = crypto.ShareCombiner(sch).set_value_mode(SIGNED)
        _same(comb.combine(list(mat)), want, type(sch).__name__)
        _same(comb.combine(mat), want, type(sch).__name__ + ", matrix")
    comb = crypto.ShareCombiner(crypto.Additive(3, q)).set_value_mode(SIGNED)
    for k in range(1, mat.shape[0]):
        comb.begin(dim)
        comb.update(mat[:k])
        comb.update(mat[k:])
        _same(comb.finish(), want, f"split after {k} rows")


FORMS = [("participant-major", 0), ("clerk-major", 0), ("participant-major", 1), ("clerk-major", 1)]


def _tile(mats, r0, r1, layout, stride, off):
    """rows r0..r1 of the JOBS matrices as one device tile starting `off` elements into its buffer -> (host array, job_stride,
    row_stride)"""
    rows, dim = r1 - r0, mats[0].shape[1]
    host = np.full(JOBS * rows * stride + 2, GUARD, dtype=np.int64)
    body = host[off:off + JOBS * rows * stride]
    view = body.reshape(rows, JOBS, stride).transpose(1, 0, 2) if layout == "participant-major" else body.reshape(JOBS, rows, stride)
    for j in range(JOBS):
        view[j, :, :dim] = mats[j][r0:r1]
    if layout == "participant-major":
        return host, stride, JOBS * stride
    return host, rows * stride, stride


@pytest.mark.parametrize("layout,off", FORMS, ids=[f"{l}-base+{8 * o}" for l, o in FORMS])
@pytest.mark.parametrize("dim", SL.COMBINE_DIMS)
@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_share_combiner_device_job(gpu, q, dim, layout, off):
    """begin_dev(3 jobs) + two update_dev calls (20 and 19 rows): job = blockIdx.y with job_stride and a padded odd row_stride,
    the tile 0 or 8 bytes off 16-byte alignment; each job against its own pyoracle.combine, the tiles left as they were"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    cases = [_combine_case(q, dim, 50 * j) for j in range(JOBS)]
    mats = [c[0] for c in cases]
    stride = dim + 2 if dim & 1 else dim + 1
    assert stride & 1 and stride > dim
    comb = crypto.ShareCombiner(crypto.Additive(JOBS, q)).set_value_mode(SIGNED)
    comb.begin_dev(JOBS, dim)
    keep = []
    for r0, r1 in ((0, SPLIT), (SPLIT, mats[0].shape[0])):
        host, job_stride, row_stride = _tile(mats, r0, r1, layout, stride, off)
        d = DeviceBuffer.from_numpy(host)
        assert d.ptr % 16 == 0 and d.at(off) % 16 == 8 * off
        comb.update_dev(d.at(off), job_stride, r1 - r0, row_stride)
        keep.append((d, host))
    d_out = DeviceBuffer.from_numpy(np.full(JOBS * dim + 4, GUARD, dtype=np.int64))
    comb.finish_dev(d_out.ptr)
    out = d_out.to_numpy()
    for j in range(JOBS):
        _same(out[j * dim:(j + 1) * dim], cases[j][1], f"job {j}")
    assert (out[JOBS * dim:] == GUARD).all()
    for d, host in keep:
        assert np.array_equal(d.to_numpy(), host)


@pytest.mark.parametrize("dim", SL.COMBINE_DIMS)
@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_full_mask_combiner_and_additive_reconstructor(gpu, q, dim):
    """the same loop behind MaskCombiner(Full) (full.rs:46-48) and the additive SecretReconstructor (additive.rs:62-69): host form
    and device job, rows fed in order in two updates with a padded odd stride"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    mat, want = _combine_case(q, dim)
    rows = mat.shape[0]
    stride = dim + 2 if dim & 1 else dim + 1
    host = np.full((rows, stride), GUARD, dtype=np.int64)
    host[:, :dim] = mat
    d = DeviceBuffer.from_numpy(host)
    mc = crypto.MaskCombiner(crypto.Full(q)).set_value_mode(SIGNED)
    _same(mc.combine(list(mat)), want, "MaskCombiner.combine")
    d_out = DeviceBuffer.from_numpy(np.full(dim + 4, GUARD, dtype=np.int64))
    mc.begin_dev(dim)
    mc.update_dev(d.ptr, SPLIT, dim, stride)
    mc.update_dev(d.at(SPLIT * stride), rows - SPLIT, dim, stride)
    mc.finish_dev(d_out.ptr, dim)
    out = d_out.to_numpy()
    _same(out[:dim], want, "MaskCombiner device job")
    assert (out[dim:] == GUARD).all()
    rec = crypto.SecretReconstructor(crypto.Additive(rows, q), dim).set_value_mode(SIGNED)
    _same(rec.reconstruct(list(enumerate(mat))), want, "SecretReconstructor.reconstruct")
    d_out = DeviceBuffer.from_numpy(np.full(dim + 4, GUARD, dtype=np.int64))
    rec.begin_dev(None, rows, dim)
    rec.update_dev(0, d.ptr, SPLIT, stride)
    rec.update_dev(SPLIT, d.at(SPLIT * stride), rows - SPLIT, stride)
    rec.finish_dev(d_out.ptr, dim)
    out = d_out.to_numpy()
    _same(out[:dim], want, "SecretReconstructor device job")
    assert (out[dim:] == GUARD).all() and np.array_equal(d.to_numpy().reshape(rows, stride), host)


# ---- signed_additive_gen_kernel (injected draws) ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _generate_case(q, n, roll=0):
    secrets, rand = SL.generate_rolled(q, n, roll)
    return _np(secrets), _np(rand), _po().generate(_po().AdditiveSecretSharing(n, q, SIGNED), secrets, rand)


@pytest.mark.parametrize("n", SL.GEN_N)
@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_generate_with_injected_draws(gpu, q, n):
    """secret x first draw over specials(q)^2, further draws cycling through specials(q); n = 1 has no draws and returns the
    raw, unreduced secret (additive.rs:42-47)"""
    from sda_amd import crypto
    secrets, rand, want = _generate_case(q, n)
    gen = crypto.ShareGenerator(crypto.Additive(n, q)).set_value_mode(SIGNED)
    got = gen.generate(secrets, rand if n > 1 else None)
    assert _last_kernel() == "signed_additive_gen_kernel", _last_kernel()
    assert got.shape == (n, secrets.size)
    for j in range(n):
        _same(got[j], want[j], f"share {j}")


@pytest.mark.parametrize("layout", ["participant-major", "clerk-major"])
@pytest.mark.parametrize("n", SL.GEN_N)
@pytest.mark.parametrize("q", SL.MODULI, ids=ids)
def test_generate_batch_dev_with_injected_draws(gpu, q, n, layout):
    """three participants, padded secrets_stride, rand_stride and output strides, both output layouts: every share against the
    oracle, nothing written outside the first len columns, the inputs left as they were"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    P = 3
    cases = [_generate_case(q, n, 101 * p) for p in range(P)]
    length = cases[0][0].size
    s_stride, r_stride, Bs = length + 5, length * (n - 1) + 3, length + 3
    sec = np.full((P, s_stride), GUARD, dtype=np.int64)
    rnd = np.full((P, r_stride), GUARD, dtype=np.int64)
    for p, (s, r, _) in enumerate(cases):
        sec[p, :length] = s
        rnd[p, :r.size] = r
    d_sec, d_rnd = DeviceBuffer.from_numpy(sec), DeviceBuffer.from_numpy(rnd)
    d_out = DeviceBuffer.from_numpy(np.full(n * P * Bs, GUARD, dtype=np.int64))
    osp, osc = (n * Bs, Bs) if layout == "participant-major" else (Bs, P * Bs)
    assert (P - 1) * osp + (n - 1) * osc + length <= n * P * Bs
    gen = crypto.ShareGenerator(crypto.Additive(n, q)).set_value_mode(SIGNED)
    gen.generate_batch_dev(d_sec.ptr, P, length, s_stride, d_out.ptr, osp, osc, d_rand=d_rnd.ptr if n > 1 else 0, rand_stride=r_stride)
    assert _last_kernel() == "signed_additive_gen_kernel", _last_kernel()
    out = d_out.to_numpy()
    out = out.reshape(P, n, Bs) if layout == "participant-major" else out.reshape(n, P, Bs).transpose(1, 0, 2)
    for p in range(P):
        for j in range(n):
            _same(out[p, j, :length], cases[p][2][j], f"participant {p}, share {j}")
    assert (out[:, :, length:] == GUARD).all()
    assert np.array_equal(d_sec.to_numpy().reshape(sec.shape), sec) and np.array_equal(d_rnd.to_numpy().reshape(rnd.shape), rnd)


@pytest.mark.parametrize("q", SL.BIG_JOB_MODULI, ids=ids)
def test_generate_job_beyond_one_grid(gpu, q):
    """65535 + 2 participants in one call: the launcher slices blockIdx.y at 65535 and offsets secrets, draws and output by the
    strides.  Dimension 3, n = 2, clerk-major with padded strides, every element compared"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    P, dim, n = SL.BIG_JOB
    secrets, rand = SL.grid_pairs(q, P * dim)
    want = _po().FullMasker(q, SIGNED).unmask(rand, secrets)          # n = 2: the last share is (s - r) % q, as the reach test shows
    s_stride, r_stride, Bs = dim + 1, dim * (n - 1) + 2, dim + 1
    sec = np.full((P, s_stride), GUARD, dtype=np.int64)
    rnd = np.full((P, r_stride), GUARD, dtype=np.int64)
    sec[:, :dim] = _np(secrets).reshape(P, dim)
    rnd[:, :dim] = _np(rand).reshape(P, dim)
    d_sec, d_rnd = DeviceBuffer.from_numpy(sec), DeviceBuffer.from_numpy(rnd)
    d_out = DeviceBuffer.from_numpy(np.full(n * P * Bs, GUARD, dtype=np.int64))
    gen = crypto.ShareGenerator(crypto.Additive(n, q)).set_value_mode(SIGNED)
    gen.generate_batch_dev(d_sec.ptr, P, dim, s_stride, d_out.ptr, Bs, P * Bs, d_rand=d_rnd.ptr, rand_stride=r_stride)
    assert _last_kernel() == "signed_additive_gen_kernel", _last_kernel()
    out = d_out.to_numpy().reshape(n, P, Bs)
    _same(out[0, :, :dim], rand, "share 0 (the draws)")
    _same(out[1, :, :dim], want, "share 1")
    assert (out[:, :, dim:] == GUARD).all()


# ---- signed_additive_gen_drbg_kernel<20> (the library's draws) ----------------------------------------------------------------------------------
DRBG_MODULI = SL.DRBG_MODULI


def test_the_drbg_moduli_cover_every_draw_rule(gpu):
    """one modulus (here: two) per distinct sda_drbg_draw_rule among MODULI and 2^31 - 1, and 2^62 - 1"""
    rule = gpu.sda_drbg_draw_rule
    assert {rule(q) for q in DRBG_MODULI} == {rule(q) for q in SL.DRBG_CANDIDATES} == {1, 2}
    assert (1 << 62) - 1 in DRBG_MODULI and set(DRBG_MODULI) <= set(SL.DRBG_CANDIDATES)


@pytest.mark.parametrize("n", SL.DRBG_N)
@pytest.mark.parametrize("dim", SL.DRBG_DIMS)
@pytest.mark.parametrize("q", DRBG_MODULI, ids=ids)
def test_generate_with_the_librarys_own_draws(gpu, q, dim, n):
    """two participants at the last stream ids, clerk-major output with padded strides, secrets cycling through specials(q):
    shares 0..n-2 are coracle.drbg_fill's draws - bit for bit the canonical mode's draw rows - and the last share is pyoracle's
    fold over those draws from the RAW secret; the padding stays zero"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    from oracle import coracle
    P, first = 2, SL.DRBG_FIRST
    secrets = SL.drbg_secrets(q, dim)
    s_stride, Bs = dim + 3, dim + 5
    sec = np.full((P, s_stride), GUARD, dtype=np.int64)
    for p in range(P):
        sec[p, :dim] = _np(secrets[p])
    d_sec = DeviceBuffer.from_numpy(sec)
    outs = {}
    for mode in ("canonical", SIGNED):
        gen = crypto.ShareGenerator(crypto.Additive(n, q)).set_value_mode(mode)
        gen.set_drbg_key(KEY)
        d_out = DeviceBuffer(n * P * Bs).zero()
        gen.generate_batch_dev(d_sec.ptr, P, dim, s_stride, d_out.ptr, Bs, P * Bs, first_participant=first)
        outs[mode] = d_out.to_numpy().reshape(n, P, Bs)
    assert _last_kernel() == "signed_additive_gen_drbg_kernel<20>", _last_kernel()
    got = outs[SIGNED]
    osch = _po().AdditiveSecretSharing(n, q, SIGNED)
    lasts = []
    for p in range(P):
        draws = coracle.drbg_fill(KEY, first + p, dim, n - 1, q)
        assert draws.min() >= 0 and draws.max() < q
        want = _po().generate(osch, secrets[p], [int(v) for v in draws])
        lasts += want[n - 1]
        for j in range(n):
            _same(got[j, p, :dim], want[j], f"participant {p}, share {j}")
        _same(got[:n - 1, p, :dim], draws.reshape(dim, n - 1).T, f"participant {p}: the draw rows")
        assert np.array_equal(outs["canonical"][:n - 1, p, :dim], got[:n - 1, p, :dim])
        _same(outs["canonical"][n - 1, p, :dim], [v % q for v in want[n - 1]], f"participant {p}: the canonical last share")
    assert (got[:, :, dim:] == 0).all()
    assert SL.tells_signed_from_canonical(lasts, q)                    # (tests/test_signed_limits_reach.py shows it for this key)

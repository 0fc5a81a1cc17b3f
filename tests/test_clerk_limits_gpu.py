"""Every form of the clerk sum at the carry limits of its 128-bit column sums, bit-exact against Python integer sums (pytest -m gpu).

The other clerk-sum tests feed uniform random rows or shares the same call generated; below 2^31 such rows never make the low word
of an accumulator wrap and never leave its high word non-zero.  Here the rows are crafted (tests/clerk_limits.py: all MIN, all
MAX, all -1, alternating signs, negative multiples of the modulus, ...) and fed to every place that holds the accumulator
arithmetic: combine_update_kernel's plain and atomic endings, the side-stream walk kernel, the clerk role of the dual-role
launches (through generate_combine_dev with a crafted d_prev), the narrow limb GEMM's clerk waves, follow-up kernel and clerk
workgroups, the LDS window of the wire-fed and sealed sums, and modsum_parts_kernel.  Every expected value is
clerk_limits.want(): sum(int(x)) % m.  tests/test_clerk_limits_reach.py proves on the CPU that these inputs reach the carries."""
import functools

import numpy as np
import pytest

import clerk_limits as CL
import extremes as X
from conftest import set_knob

pytestmark = pytest.mark.gpu

KEY = bytes(range(7, 39))


def _sums(comb, jobs, dim):
    from sda_amd.device import DeviceBuffer
    d = DeviceBuffer(jobs * dim)
    comb.finish_dev(d.ptr)
    return d.to_numpy().reshape(jobs, dim)


def _same(got, expect, first=0):
    diff = CL.first_difference(got, expect, first)
    assert diff is None, diff


def _ids(m):
    return f"m{m}"


# ---- combine_update_kernel, plain ending ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_data(m, dim):
    calls = [CL.crafted_jobs(CL.PLAIN_JOBS, rows, dim, m, CL.first_for(m)) for rows in CL.PLAIN_ROWS]
    return calls, CL.want(np.concatenate(calls, axis=1), m)


@pytest.mark.parametrize("form", ["vector", "odd row stride", "base offset of 8 bytes"])
@pytest.mark.parametrize("dim", CL.PLAIN_DIMS)
@pytest.mark.parametrize("m", CL.MODULI, ids=_ids)
def test_plain_ending_across_calls(gpu, m, dim, form):
    """one begin, then update_dev with 16, 9 and 1 rows five times over: one row split each, so every call reads, adds to and
    rewrites the stored (low, high) pair, whose high words grow from call to call"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    calls, expect = _plain_data(m, dim)
    jobs = CL.PLAIN_JOBS
    comb = crypto.ShareCombiner(crypto.Additive(3, m))
    comb.begin_dev(jobs, dim)
    keep = []
    for tile in calls:
        rows = tile.shape[1]
        assert CL.combine_split(rows, dim, jobs) == (1, rows)
        stride = dim | 1 if form == "odd row stride" else dim + (dim & 1)
        job_stride = rows * stride
        host = np.zeros(jobs * job_stride + 2, dtype=np.int64)
        off = 1 if form.startswith("base offset") else 0
        view = host[off:off + jobs * job_stride].reshape(jobs, rows, stride)
        view[:, :, :dim] = tile
        d = DeviceBuffer.from_numpy(host)
        keep.append(d)
        assert (d.at(off) % 16 == 0 and stride % 2 == 0 and job_stride % 2 == 0) == (form == "vector")
        comb.update_dev(d.at(off), job_stride, rows, stride)
    _same(_sums(comb, jobs, dim), expect, CL.first_for(m))


# ---- combine_update_kernel, atomic ending -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _atomic_data(m, jobs, dim, rows):
    mat = CL.crafted_jobs(jobs, rows, dim, m, CL.first_for(m))
    return mat, CL.want(mat, m)


ATOMIC = [(m, c, 0) for c in CL.ATOMIC_CASES[:2] for m in CL.MODULI] + [(m, CL.ATOMIC_CASES[2], 0) for m in (CL.PMAX, 433)] + \
         [(m, CL.ATOMIC_CASES[0], 2) for m in (CL.PMAX, 2)]


@pytest.mark.parametrize("m,case,residency", ATOMIC, ids=[f"m{m}-jobs{c[0]}-dim{c[1]}-rows{c[2]}" + ("-residency2" if r else "") for m, c, r in ATOMIC])
def test_atomic_ending(gpu, m, case, residency):
    """several row splits per column: the partial (low, high) pairs meet in acc_atomic_add, in whatever order the hardware runs
    them - 65 splits of 16 rows, 64 with a last split of 15, 41 splits of 25"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    jobs, dim, rows = case
    assert CL.combine_split(rows, dim, jobs) == {1030: (65, 16), 1023: (64, 16) if jobs == 3 else (41, 25)}[rows]
    mat, expect = _atomic_data(m, jobs, dim, rows)
    stride = dim + 1
    host = np.zeros((jobs, rows, stride), dtype=np.int64)
    host[:, :, :dim] = mat
    d = DeviceBuffer.from_numpy(host)
    comb = crypto.ShareCombiner(crypto.Additive(3, m))
    if residency:
        comb.set_residency(residency)
    comb.begin_dev(jobs, dim)
    comb.update_dev(d.ptr, rows * stride, rows, stride)
    _same(_sums(comb, jobs, dim), expect, CL.first_for(m))


@pytest.mark.parametrize("m", CL.MODULI, ids=_ids)
def test_host_buffer_forms(gpu, m):
    """the same 1030 x 37 matrix through combine() and through begin / update / finish (two tiles)"""
    from sda_amd import crypto
    mat, expect = _atomic_data(m, 3, 37, 1030)
    comb = crypto.ShareCombiner(crypto.Additive(3, m))
    _same(comb.combine(list(mat[0]))[None, :], expect[:1], CL.first_for(m))
    comb.begin(37)
    comb.update(mat[1][:700])
    comb.update(mat[1][700:])
    _same(comb.finish()[None, :], expect[1:2], CL.first_for(m) + 1)


# ---- generate_combine_dev with a crafted previous tile ---------------------------------------------------------------------------------
def _prev_tiles(n, prevs, B, Bs, m):
    """[n][P_prev][Bs] crafted tiles (one per entry of prevs; clerk j holds crafted_matrix(.., first = j)) and the expected sums"""
    tiles = []
    for rows in prevs:
        t = np.zeros((n, rows, Bs), dtype=np.int64)
        t[:, :, :B] = CL.crafted_jobs(n, rows, B, m, 0)
        tiles.append(t)
    return tiles, CL.want(np.concatenate([t[:, :, :B] for t in tiles], axis=1), m)


def _run_crafted_prev(gen, comb, n, B, Bs, dim, tiles, participants, on_call=None):
    """one generate_combine_dev per crafted tile: d_prev is the crafted tile, d_out another buffer with the same strides.
    participants[i] secrets vectors are shared in call i (0: clerk-only).  Returns the secrets"""
    from sda_amd.device import DeviceBuffer
    rng = np.random.default_rng(dim)
    m = gen.scheme.modulus if hasattr(gen.scheme, "modulus") else gen.scheme.prime_modulus
    sec = rng.integers(0, m, size=(2, dim + (dim & 1)), dtype=np.int64)
    d_sec = DeviceBuffer.from_numpy(sec)
    comb.begin_dev(n, B)
    for i, (tile, P) in enumerate(zip(tiles, participants)):
        rows = tile.shape[1]
        assert P <= rows
        d_prev = DeviceBuffer.from_numpy(tile)
        d_out = DeviceBuffer(n * rows * Bs).zero()
        gen.generate_combine_dev(comb, d_sec.ptr if P else 0, P, dim, sec.shape[1], d_out.ptr if P else 0, Bs, rows * Bs,
                                 d_prev=d_prev.ptr, prev_participants=rows, first_participant=2 * i)
        if on_call:
            on_call(i, P, d_out.to_numpy().reshape(n, rows, Bs)[:, :P, :B] if P else None, sec[:, :dim])
        else:
            from sda_amd.device import synchronize
            synchronize()                                  # d_prev / d_out are freed when they go out of scope
    return sec[:, :dim]


def _last_kernel():
    from sda_amd import capi
    return capi.load().sda_debug_last_kernel().decode()


@pytest.mark.parametrize("side", [True, False], ids=["side stream", "SDA_NO_SIDE_STREAM"])
def test_side_stream_walk_kernel(gpu, side):
    """the transform shape's clerk sum (combine_update_walk_kernel on the generator's side stream): 242 jobs x 6 columns, previous
    tiles of 40 rows (3 splits of 14, 14, 12) and 1030 rows (17 splits of 61) with two participants generated beside them, then
    a clerk-only call; again with the side stream switched off (combine_update_kernel, two launches)"""
    from sda_amd import crypto
    from test_parity_gpu import _root
    if not side:
        set_knob("SDA_NO_SIDE_STREAM", 1)
    k, t, n, p, B = 40, 23, 242, CL.P62, 6
    sch = crypto.PackedShamir(k, n, t, p, _root(p, 64), _root(p, 243))
    gen = crypto.ShareGenerator(sch)
    gen.set_drbg_key(KEY)
    dim = k * B - 1
    assert gen.batch_count(dim) == B
    assert CL.combine_split(40, B, n) == (3, 14) and CL.combine_split(1030, B, n) == (17, 61)
    prevs = CL.WALK_PREV + (40,)
    tiles, expect = _prev_tiles(n, prevs, B, B, p)
    names = []
    comb = crypto.ShareCombiner(sch)
    _run_crafted_prev(gen, comb, n, B, B, dim, tiles, (2, 2, 0), lambda i, P, out, sec: names.append(_last_kernel()))
    _same(_sums(comb, n, B), expect)
    tail = "combine_update_walk_kernel (side stream)" if side else "combine_update_kernel (two launches)"
    assert names[0].endswith(tail) and names[1].endswith(tail), names
    assert names[2] == "combine_update_kernel (two launches)", names


DUAL = [("l31", 3, 1, 8, CL.PMAX), ("mfma", 12, 3, 26, CL.P62), ("n31", 3, 4, 8, CL.P31MAX), ("additive", 1, 2, 3, CL.P62)]


@pytest.mark.parametrize("family,k,t,n,p", DUAL, ids=[c[0] for c in DUAL])
def test_clerk_role_of_the_dual_role_launches(gpu, family, k, t, n, p):
    """fused_packed_l31 / _mfma / _n31 / fused_additive: the clerk items beside two generated participants sum crafted previous
    tiles of 3 and 40 rows (one item: read-modify-write) and 1030 rows (three atomic items of 344, 343, 343), then a clerk-only
    call; the tile each call generates still equals the oracle's shares"""
    from sda_amd import crypto
    from oracle import coracle
    from test_extremes_gpu import expected_kernel
    B = Bs = 48
    if family == "additive":
        sch, w2, w3 = crypto.Additive(n, p), None, None
    else:
        w2, w3 = X.omegas(p, k, t, n)
        sch = crypto.PackedShamir(k, n, t, p, w2, w3)
    gen = crypto.ShareGenerator(sch)
    gen.set_drbg_key(KEY)
    dim = k * B
    assert gen.batch_count(dim) == B
    assert [CL.fuse_split(r) for r in CL.DUAL_PREV] == [(1, 3), (1, 40), (3, 344)]
    prevs = CL.DUAL_PREV + (40,)
    tiles, expect = _prev_tiles(n, prevs, B, Bs, p)
    fused = "fused_additive_kernel<20>" if family == "additive" else expected_kernel(family, k, t, p, fused=True)

    def on_call(i, P, out, sec):
        if not P:
            return
        assert fused in _last_kernel(), (_last_kernel(), fused)
        for q in range(P):
            draws = coracle.drbg_fill(KEY, 2 * i + q, B, t, p)
            sh = (coracle.additive_generate(p, n, sec[q], draws) if family == "additive" else
                  coracle.packed_generate_csprng(p, k, t, n, w2, w3, sec[q], draws, gen.csprng_share_map()))
            assert np.array_equal(out[:, q, :], sh), f"call {i}: generated shares of participant {q}"
    comb = crypto.ShareCombiner(sch)
    _run_crafted_prev(gen, comb, n, B, Bs, dim, tiles, (2, 2, 2, 0), on_call)
    _same(_sums(comb, n, B), expect)


@pytest.mark.parametrize("way", ["clerk waves", "odd B", "clerk-only", "SDA_NGEMM_CLERK_WG"])
def test_narrow_limb_gemm_clerk_sums(gpu, way):
    """(20, 13, 50) over 8355691, previous tiles of 5, 40 and 1030 crafted rows: the clerk waves inside the share-generation
    workgroups with ngemm_clerk_rest_kernel behind them (even B: 16-byte read-modify-write of the running sums), the clerk
    workgroup items (odd B, or the knob), and clerk-only calls.  From the second call on the running sums the clerk waves
    fetch are large: the carries of flush and of the follow-up kernel run with real values"""
    from sda_amd import crypto
    from oracle import coracle
    k, t, n, p = 20, 13, 50, CL.NGEMM_PMAX
    if way == "SDA_NGEMM_CLERK_WG":
        set_knob("SDA_NGEMM_CLERK_WG", 1)
    B = 49 if way == "odd B" else 48
    Bs = (B + 15) // 16 * 16
    w2, w3 = X.omegas(p, k, t, n)
    sch = crypto.PackedShamir(k, n, t, p, w2, w3)
    gen = crypto.ShareGenerator(sch)
    gen.set_drbg_key(KEY)
    dim = k * B
    assert gen.batch_count(dim) == B and gen.path_name().endswith("ngemm")
    tiles, expect = _prev_tiles(n, CL.NGEMM_PREV, B, Bs, p)
    P = 0 if way == "clerk-only" else 2

    def on_call(i, P, out, sec):
        if not P:
            assert _last_kernel() == "combine_update_kernel (two launches)", _last_kernel()
            return
        assert _last_kernel().startswith("packed_gen_ngemm_kernel<1, "), _last_kernel()
        for q in range(P):
            sh = coracle.packed_generate_csprng(p, k, t, n, w2, w3, sec[q], coracle.drbg_fill(KEY, 2 * i + q, B, t, p), gen.csprng_share_map())
            assert np.array_equal(out[:, q, :], sh), f"call {i}: generated shares of participant {q}"
    comb = crypto.ShareCombiner(sch)
    _run_crafted_prev(gen, comb, n, B, Bs, dim, tiles, (P, P, P), on_call)
    _same(_sums(comb, n, B), expect)


# ---- wire-fed sums: the LDS window ------------------------------------------------------------------------------------------------------
def _slotted(mat):
    """[rows][L] -> (device bytes, slot, device lengths): the oracle's varint encoding of every row in the slotted layout"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    from oracle import coracle
    rows, L = mat.shape
    slot = crypto.VarintCodec().slot_size(L)
    raw = bytearray(rows * slot + 64)                      # (slack behind the last slot, as the other wire tests leave)
    lens = np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        e = coracle.varint_encode(mat[r])
        raw[r * slot:r * slot + len(e)] = e
        lens[r] = len(e)
    return DeviceBytes.from_bytes(raw), slot, DeviceBuffer.from_numpy(lens)


def _wire_sums(m, jobs, L, d_bytes, slot, d_lens, rows):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    comb = crypto.ShareCombiner(crypto.Additive(3, m))
    st = DeviceBuffer(1).zero()
    comb.begin_dev(jobs, L)
    comb.update_encoded_rows_dev(crypto.VarintCodec(), d_bytes.ptr, slot, d_lens.ptr, rows, st.ptr)
    got = _sums(comb, jobs, L)
    assert int(st.to_numpy()[0]) == 0
    return got


@pytest.mark.parametrize("name,jobs,rpj,L", CL.WIRE_CASES, ids=[c[0] for c in CL.WIRE_CASES])
@pytest.mark.parametrize("m", CL.MODULI, ids=_ids)
def test_wire_fed_sums_through_the_window(gpu, m, name, jobs, rpj, L):
    """varint_stream_combine_kernel<8> (1 job of 24 rows) and <16> (512 jobs of 16 rows): every window cell collects 8 / 16 values
    in two 32-bit planes and is folded as A + (Bq << 32) with a carry"""
    assert CL.window_rows(rpj, jobs) == (8 if name == "8 rows" else 16)
    mat = CL.crafted_jobs(jobs, rpj, L, m, CL.first_for(m))
    d_bytes, slot, d_lens = _slotted(mat.reshape(jobs * rpj, L))
    _same(_wire_sums(m, jobs, L, d_bytes, slot, d_lens, jobs * rpj), CL.want(mat, m), CL.first_for(m))


DRIFT = [(CL.PMAX, CL.MIN), (433, CL.MAX), (2, CL.MIN)]


@pytest.mark.parametrize("m,long_value", DRIFT, ids=[f"m{m}-{'MIN' if v < 0 else 'MAX'}" for m, v in DRIFT])
def test_wire_fed_sums_beyond_the_window(gpu, m, long_value):
    """rows of one-byte values (-1) beside rows of ten-byte values (MIN or MAX): the short rows run more than 2048 columns ahead,
    so their values go straight to acc_atomic_add(v, v >> 63)"""
    mat = CL.drift_matrix(long_value)
    assert len(CL.drift_direct()) > 2000
    d_bytes, slot, d_lens = _slotted(mat)
    got = _wire_sums(m, 1, CL.DRIFT_L, d_bytes, slot, d_lens, CL.DRIFT_ROWS)
    assert np.array_equal(got[0], CL.want(mat, m)), int(np.flatnonzero(got[0] != CL.want(mat, m))[0])


@pytest.mark.parametrize("path", ["stream", "scan"])
def test_wire_fed_sums_offsets_form(gpu, path):
    """update_encoded_dev (rows back to back, an offsets array) on the 24 x 300 matrix: the window kernel, and the decode +
    combine_update_kernel form"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    from oracle import coracle
    set_knob("SDA_VARINT_PATH", path)
    m, (_, jobs, rpj, L) = CL.PMAX, CL.WIRE_CASES[0]
    mat = CL.crafted_matrix(rpj, L, m, 5)
    enc = [coracle.varint_encode(r) for r in mat]
    raw = b"".join(enc)
    offs = np.cumsum([0] + [len(e) for e in enc]).astype(np.int64)
    d_bytes = DeviceBuffer.from_numpy(np.frombuffer(raw + b"\0" * (-len(raw) % 8 or 8), dtype=np.int64))
    d_off = DeviceBuffer.from_numpy(offs)
    comb = crypto.ShareCombiner(crypto.Additive(3, m))
    st = DeviceBuffer(1).zero()
    comb.begin_dev(1, L)
    comb.update_encoded_dev(crypto.VarintCodec(), d_bytes.ptr, len(raw), d_off.ptr, rpj, st.ptr)
    got = _sums(comb, 1, L)
    assert int(st.to_numpy()[0]) == 0
    _same(got, CL.want(mat, m)[None, :], 5)


# ---- sealed sums ---------------------------------------------------------------------------------------------------------------------------
SEALED = [(CL.PMAX, "24 x 300"), (433, "24 x 300"), (CL.PMAX, "drift MIN"), (2, "drift MAX")]


@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("m,what", SEALED, ids=[f"m{m}-{w}" for m, w in SEALED])
def test_sealed_sums(gpu, m, what, waves):
    """sealed_stream_combine_kernel<8 | 16> over boxes sealed from the crafted 24 x 300 matrix and from the drift matrix"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    from test_clerk_sealed_gpu import _keys, seal_matrix, u32
    set_knob("SDA_SEALED_WAVES", waves)
    if what == "24 x 300":
        mat = CL.crafted_matrix(24, 300, m, CL.first_for(m))
    else:
        mat = CL.drift_matrix(CL.MIN if what.endswith("MIN") else CL.MAX)
    rows, L = mat.shape
    pk, sk = _keys(300 + waves)
    job = seal_matrix(mat, pk)
    comb = crypto.ShareCombiner(crypto.Additive(3, m))
    d_status, d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * rows).zero()
    comb.begin_dev(1, L)
    comb.update_sealed_rows_dev(crypto.VarintCodec(), crypto.SealedBox(), pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, rows, job.slot,
                                d_status.ptr, d_ok.ptr)
    got = _sums(comb, 1, L)
    assert _last_kernel() == f"sbox_poly_kernel + sealed_stream_combine_kernel<{waves}>"
    assert int(u32(d_status)[0]) == 0 and u32(d_ok, rows).all()
    _same(got, CL.want(mat, m)[None, :], CL.first_for(m) if what == "24 x 300" else 0)


# ---- modsum_parts_kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [433, CL.PMAX], ids=_ids)
def test_modsum_parts(gpu, m):
    """64 parts of any i64 through sda_modsum_parts_dev: acc_add in registers, mod_i128 at once"""
    from sda_amd.capi import check
    from sda_amd.device import DeviceBuffer
    mat = CL.crafted_matrix(64, 1023, m, CL.first_for(m))
    d = DeviceBuffer.from_numpy(mat)
    out = DeviceBuffer(1023)
    check(gpu.sda_modsum_parts_dev(m, d.ptr, 64, 1023, 1023, out.ptr, None))
    _same(out.to_numpy()[None, :], CL.want(mat, m)[None, :], CL.first_for(m))

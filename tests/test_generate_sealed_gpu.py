"""sda_share_generator_generate_sealed_rows_dev: a participation from the secrets to the sealed rows of every clerking job in
one call (participate.rs:75-101) - the setup pass, then ONE kernel whose waves compute a clerk's shares of one participant from
the secrets and the sda-drbg-v1 draws, varint-encode them and xor the XSalsa20 keystream in before anything is stored, then
the Poly1305 pass.  No share reaches device memory and there is no share buffer.

The oracle of every case (tests/generate_sealed_cases.py; what the table reaches is proved in
tests/test_generate_sealed_reach.py) is coracle.drbg_fill -> packed_generate_csprng / additive_generate -> varint_encode ->
sealedbox_oracle.seal with injected ephemeral secrets; the "two-call chain" is sda_share_generator_generate_batch_dev +
sda_sealedbox_seal_share_rows_dev on a handle with the same settings.  The box buffer is prefilled with 0xA5, so a byte written
past a row's length shows (check_against of tests/test_participant_seal_gpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import generate_sealed_cases as gs
from conftest import use_test_hooks
from test_participant_seal_gpu import PATTERN, _pattern_buffer, check_against

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in gs.CASES]


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def scheme_of(case):
    from sda_amd import crypto
    if case["additive"]:
        return crypto.Additive(case["n"], case["p"])
    w2, w3 = gs.omegas(case)
    return crypto.PackedShamir(case["k"], case["n"], case["t"], case["p"], w2, w3)


def generator_of(case, share_map=None, key=gs.KEY):
    """a generator in deterministic mode on the given share map; None when the handle does not offer that map"""
    from sda_amd import crypto
    gen = crypto.ShareGenerator(scheme_of(case))
    if key is not None:
        gen.set_drbg_key(key)
    if share_map is not None:
        if share_map == 1 and gen.csprng_share_map() != 1:
            return None
        gen.set_csprng_share_map(share_map)
        assert gen.csprng_share_map() == share_map
    return gen


class Secrets:
    """the secrets of a case resident in HBM with the case's stride and element offset; junk between and around the rows"""

    def __init__(self, case, secrets=None):
        from sda_amd.device import DeviceBuffer
        sec = gs.secrets_of(case) if secrets is None else secrets
        self.participants, self.len = sec.shape
        self.stride, off = max(case["stride"], self.len), case["offset"]
        host = np.random.default_rng(7).integers(gs.I64_MIN, gs.I64_MAX, size=off + self.participants * self.stride + 2, dtype=np.int64)
        for q in range(self.participants):
            host[off + q * self.stride:off + q * self.stride + self.len] = sec[q]
        self.buf = DeviceBuffer.from_numpy(host)
        self.ptr = self.buf.at(off)


def slot_of(case):
    from sda_amd import crypto
    return crypto.VarintCodec().slot_size(gs.batches(case)) + 48


def _lens(d_lens, rows):
    return np.frombuffer(d_lens.to_bytes(rows * 8), dtype="<u8").copy()


def run_new(case, gen, S, esk, pks=None):
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    rows, slot = gs.rows(case), slot_of(case)
    d_boxes, d_lens = _pattern_buffer(rows * slot), DeviceBytes(rows * 8).zero()
    pks = [k[0] for k in gs.clerk_keys(case)] if pks is None else pks
    gen.generate_sealed_rows_dev(codec, box, pks, S.ptr, S.participants, S.len, S.stride, d_boxes.ptr, slot, d_lens.ptr,
                                 first_participant=case["first"], esk=esk)
    return d_boxes.to_bytes(rows * slot), _lens(d_lens, rows), slot


def run_chain(case, gen, S, esk):
    """generate_batch_dev into a share buffer [n][participants][B], then seal_share_rows_dev over its n * participants rows"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    rows, slot, B, P = gs.rows(case), slot_of(case), gs.batches(case), case["participants"]
    d_shares = DeviceBuffer(max(rows * B, 2)).zero()
    gen.generate_batch_dev(S.ptr, P, S.len, S.stride, d_shares.ptr, B, P * B, first_participant=case["first"])
    d_boxes, d_lens = _pattern_buffer(rows * slot), DeviceBytes(rows * 8).zero()
    box.seal_share_rows_dev(codec, [k[0] for k in gs.clerk_keys(case)], P, d_shares.ptr, rows, B, B, d_boxes.ptr, slot, d_lens.ptr, esk)
    return d_boxes.to_bytes(rows * slot), _lens(d_lens, rows)


@functools.lru_cache(maxsize=None)
def oracle_boxes(name, share_map):
    return tuple(gs.oracle_boxes(gs.BY_NAME[name], share_map))


def maps_offered(case):
    if case["additive"]:
        return [None]
    return [m for m in (1, 0) if generator_of(case, m) is not None]


# ---- 1. byte-exact against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_boxes_equal_the_oracles(gpu, name):
    from sda_amd import capi
    case = gs.BY_NAME[name]
    S, esk = Secrets(case), gs.esk_of(case)
    maps = maps_offered(case)
    assert maps
    for m in maps:
        raw, lens, slot = run_new(case, generator_of(case, m), S, esk)
        assert b"share_seal_stream_kernel<20> + sbox_poly_kernel" == capi.load().sda_debug_last_kernel()
        want = oracle_boxes(name, m)
        print(f"{name} map {m}: rows {len(want)} batches {gs.batches(case)} lengths {lens.min()}..{lens.max()} slot {slot}")
        check_against(raw, lens, slot, want, esk, f"{name}, share map {m}")
        if case["small_order"] is not None:
            P, c = case["participants"], case["small_order"]
            assert [w is None for w in want] == [r // P == c for r in range(len(want))]
            assert (lens[c * P:(c + 1) * P] == 0).all() and (np.delete(lens, range(c * P, (c + 1) * P)) > 48).all()


# ---- 2. byte-exact against the two-call chain ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_boxes_equal_the_two_call_chain(gpu, name):
    case = gs.BY_NAME[name]
    S, esk = Secrets(case), gs.esk_of(case)
    for m in maps_offered(case):
        raw, lens, slot = run_new(case, generator_of(case, m), S, esk)
        raw2, lens2 = run_chain(case, generator_of(case, m), S, esk)
        assert np.array_equal(lens, lens2), f"{name}, share map {m}: lengths differ from generate_batch_dev + seal_share_rows_dev"
        assert raw == raw2, f"{name}, share map {m}: boxes (or the bytes around them) differ from generate_batch_dev + seal_share_rows_dev"


def test_chacha12_and_chacha8_handles_equal_the_chain_too(gpu):
    case = gs.BY_NAME["retry-packed"]
    S, esk = Secrets(case), gs.esk_of(case)
    for rounds in (12, 8):
        a, b = generator_of(case), generator_of(case)
        a.set_drbg_rounds(rounds); b.set_drbg_rounds(rounds)
        raw, lens, slot = run_new(case, a, S, esk)
        raw2, lens2 = run_chain(case, b, S, esk)
        assert np.array_equal(lens, lens2) and raw == raw2, rounds


def test_len_zero_gives_boxes_of_the_empty_message(gpu):
    from oracle import sealedbox_oracle as so
    case = dict(gs.BY_NAME["B1"], len=0, stride=0)
    keys, esk = gs.clerk_keys(case), gs.esk_of(case)
    S = Secrets(case, np.zeros((1, 0), dtype=np.int64))
    raw, lens, slot = run_new(case, generator_of(case), S, esk)
    assert slot == 48 and list(lens) == [48] * 8
    assert all(raw[48 * r:48 * r + 48] == so.seal(b"", keys[r][0], esk[32 * r:32 * r + 32]) for r in range(8))


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBytes
    import extremes
    lib = capi.load()
    case = gs.BY_NAME["B9"]
    S, esk = Secrets(case), gs.esk_of(case)
    rows, slot = gs.rows(case), slot_of(case)
    assert slot % 16 == 0
    gen, codec, box = generator_of(case), crypto.VarintCodec(), crypto.SealedBox()
    pks = b"".join(k[0] for k in gs.clerk_keys(case))
    d_boxes, d_lens = _pattern_buffer(rows * slot + 64), DeviceBytes(rows * 8).zero()
    good = dict(g=gen._h, codec=codec._h, b=box._h, pks=pks, esk=esk, d_secrets=S.ptr, participants=1, len=S.len, secrets_stride=S.stride,
                first_participant=0, d_boxes=d_boxes.ptr, slot_bytes=slot, d_row_bytes=d_lens.ptr, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sda_share_generator_generate_sealed_rows_dev(*[a[k] for k in good])

    untouched = bytes([PATTERN]) * (rows * slot + 64)
    signed = crypto.ShareGenerator(crypto.Additive(8, gs.P62))
    signed.set_value_mode("rust_signed")
    big = crypto.ShareGenerator(crypto.PackedShamir(20, 40, 13, gs.P62, *extremes.omegas(gs.P62, 20, 13, 40)))
    pks40 = pks * 5
    bad, unsupported = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    cases = {"NULL generator": (dict(g=None), bad), "NULL codec": (dict(codec=None), bad), "NULL box handle": (dict(b=None), bad),
             "NULL pks": (dict(pks=None), bad), "NULL d_secrets": (dict(d_secrets=None), bad), "NULL d_boxes": (dict(d_boxes=None), bad),
             "NULL d_row_bytes": (dict(d_row_bytes=None), bad), "secrets_stride < len": (dict(secrets_stride=S.len - 1), bad),
             "slot_bytes not a multiple of 16": (dict(slot_bytes=slot + 8), bad), "slot_bytes too small": (dict(slot_bytes=slot - 16), bad),
             "d_boxes misaligned": (dict(d_boxes=d_boxes.ptr + 8), bad), "stream ids past 2^56": (dict(first_participant=1 << 56), bad),
             "SDA_VALUES_RUST_SIGNED": (dict(g=signed._h, len=9), unsupported), "k + t > 32": (dict(g=big._h, pks=pks40, slot_bytes=slot), unsupported)}
    for what, (kw, status) in cases.items():
        assert call(**kw) == status, what
        assert d_boxes.to_bytes() == untouched, what + ": the box buffer was written"
    assert call(g=big._h, pks=pks40) == unsupported and b"generate_batch_dev" in lib.sda_last_error() and b"seal_share_rows_dev" in lib.sda_last_error()
    if lib.sda_device_count() > 1:                                       # handles on different devices
        capi.check(lib.sda_set_device(1))
        try:
            other_box, other_codec = crypto.SealedBox(), crypto.VarintCodec()
        finally:
            capi.check(lib.sda_set_device(0))
        for kw in (dict(b=other_box._h), dict(codec=other_codec._h), dict(b=other_box._h, codec=other_codec._h)):
            assert call(**kw) == bad
            assert d_boxes.to_bytes() == untouched
    assert call(participants=0) == capi.OK
    assert d_boxes.to_bytes() == untouched
    # ... and after all the refusals the handles still work
    assert call() == capi.OK
    check_against(d_boxes.to_bytes(rows * slot), _lens(d_lens, rows), slot, oracle_boxes("B9", 1), esk, "after the refusals")


# ---- 4. the protocol loop in production mode -----------------------------------------------------------------------------------
def _production_job(case, gen, codec, box, S, keys):
    from sda_amd.device import DeviceBytes
    rows, slot = gs.rows(case), slot_of(case)
    d_boxes, d_lens = _pattern_buffer(rows * slot), DeviceBytes(rows * 8).zero()
    gen.generate_sealed_rows_dev(codec, box, [k[0] for k in keys], S.ptr, S.participants, S.len, S.stride, d_boxes.ptr, slot, d_lens.ptr)
    return d_boxes, d_lens, slot


@pytest.mark.parametrize("kind", ["packed", "additive"])
def test_protocol_loop_in_production_mode(gpu, kind):
    """OS entropy, no injected key or ephemeral secrets: 24 participations, every clerk sums ITS slice of the rows straight from
    the boxes, the recipient reconstructs from t + k clerks - the first and the last ones"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    case = dict(gs.BY_NAME["B129"] if kind == "packed" else gs.BY_NAME["additive-n3"], participants=24, first=0)
    P, n, B, p = 24, case["n"], gs.batches(case), case["p"]
    sch = scheme_of(case)
    gen, codec, box = crypto.ShareGenerator(sch), crypto.VarintCodec(), crypto.SealedBox()
    sec = gs.secrets_of(case)
    S, keys = Secrets(case, sec), gs.clerk_keys(case)
    d_boxes, d_lens, slot = _production_job(case, gen, codec, box, S, keys)
    assert (_lens(d_lens, n * P) > 48).all()
    sums = []
    for c in range(n):
        comb, d_status, d_sum = crypto.ShareCombiner(sch), DeviceBytes(4).zero(), DeviceBuffer(max(B, 2))
        comb.begin_dev(1, B)
        comb.update_sealed_rows_dev(codec, box, keys[c][0], keys[c][1], d_boxes.ptr + c * P * slot, slot, d_lens.ptr + c * P * 8, P, slot, d_status.ptr)
        comb.finish_dev(d_sum.ptr)
        assert d_status.to_bytes(4) == bytes(4), f"clerk {c}"
        sums.append(d_sum.to_numpy()[:B].copy())
    truth = np.array([sum(int(x) for x in sec[:, i]) % p for i in range(case["len"])], dtype=np.int64)
    need = n if case["additive"] else case["t"] + case["k"]
    rec = crypto.SecretReconstructor(sch, case["len"])
    for subset in (list(range(need)), list(range(n - need, n))):
        assert np.array_equal(rec.reconstruct([(c, sums[c]) for c in subset]), truth), subset


# ---- 5. two production calls on the same inputs --------------------------------------------------------------------------------
def test_two_production_calls_give_different_boxes_and_shares(gpu):
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import crypto
    case = dict(gs.BY_NAME["B9"], participants=3)
    P, n, B, p = 3, case["n"], gs.batches(case), case["p"]
    sch = scheme_of(case)
    gen, codec, box = crypto.ShareGenerator(sch), crypto.VarintCodec(), crypto.SealedBox()
    sec = gs.secrets_of(case)
    S, keys = Secrets(case, sec), gs.clerk_keys(case)
    truth = np.array([sum(int(x) for x in sec[:, i]) % p for i in range(case["len"])], dtype=np.int64)
    rec = crypto.SecretReconstructor(sch, case["len"])
    opened = []
    for _ in range(2):
        d_boxes, d_lens, slot = _production_job(case, gen, codec, box, S, keys)
        raw, lens = d_boxes.to_bytes(n * P * slot), _lens(d_lens, n * P)
        shares = np.stack([coracle.varint_decode(so.seal_open(raw[r * slot:r * slot + int(lens[r])], *keys[r // P])) for r in range(n * P)])
        opened.append((raw, shares.reshape(n, P, B)))
        sums = [coracle.combine(p, opened[-1][1][c]) for c in range(n)]
        assert np.array_equal(rec.reconstruct([(c, sums[c]) for c in (7, 2, 4, 1)]), truth)
    (raw1, sh1), (raw2, sh2) = opened
    assert all(raw1[r * slot:r * slot + 32] != raw2[r * slot:r * slot + 32] for r in range(n * P))      # fresh ephemeral keys
    assert all(not np.array_equal(sh1[c, q], sh2[c, q]) for c in range(n) for q in range(P)), "the call key did not advance"


# ---- 6. the kernels that share the encode loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,L,stride,offset", [(17, 333, None, 0), (6, 1300, 1303, 1)])
def test_existing_encode_and_seal_kernels_are_unchanged(gpu, rows, L, stride, offset):
    """varint_seal_stream_kernel (seal_share_rows_dev) against the oracle, varint_stream_encode_kernel (encode_rows_dev, then
    seal_rows_dev) against it: the encode loop they share with the new kernel now takes its values from a template argument"""
    from test_participant_seal_gpu import _keys, check
    pk, _ = _keys(rows * 131 + L)
    shares = np.random.default_rng(rows + L).integers(0, gs.P62, size=(rows, L), dtype=np.int64)
    check(shares, [pk], stride=stride, offset=offset)


# ---- 7. footprint --------------------------------------------------------------------------------------------------------------
def test_footprint_no_share_buffer(gpu):
    """32 participants x 8 clerks x 25,000 batches: the chain's share buffer is participants * n * B * 8 = 51.2 MB.  The chain
    needs the whole buffer, the new call none of it, so what the three handles newly hold after the call must stay below half
    that figure (it is the per-row key state, the Poly1305 partials, the staged keys, the lengths and the share matrix)."""
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    lib = use_test_hooks()                                       # sda_debug_mem_info lives in the library with the test hooks
    case = dict(gs.BY_NAME["B9"], participants=32, len=3 * 25_000, stride=3 * 25_000)
    P, n, B = 32, 8, gs.batches(case)
    share_bytes = P * n * B * 8
    assert 40e6 < share_bytes < 100e6
    S, keys, esk = Secrets(case), gs.clerk_keys(case), gs.esk_of(case)
    gen, codec, box = generator_of(case), crypto.VarintCodec(), crypto.SealedBox()
    slot = slot_of(case)
    d_boxes, d_lens = DeviceBytes(n * P * slot), DeviceBytes(n * P * 8).zero()

    def free_now():
        synchronize()
        f, t = C.c_size_t(), C.c_size_t()
        capi.check(lib.sda_debug_mem_info(C.byref(f), C.byref(t)))
        return f.value

    before = free_now()
    gen.generate_sealed_rows_dev(codec, box, [k[0] for k in keys], S.ptr, P, S.len, S.stride, d_boxes.ptr, slot, d_lens.ptr, esk=esk)
    grown = before - free_now()
    lens = _lens(d_lens, n * P)
    want = gs.shares_of(case, 1)
    for r in (0, 3 * P + 17, n * P - 1):
        got = d_boxes.to_bytes(int(lens[r]), r * slot)
        assert got == so.seal(coracle.varint_encode(want[r // P, r % P]), keys[r // P][0], esk[32 * r:32 * r + 32]), f"row {r}"
    # the chain on fresh handles: its share buffer alone is that figure
    gen2, codec2, box2 = generator_of(case), crypto.VarintCodec(), crypto.SealedBox()
    mid = free_now()
    d_shares = DeviceBuffer(n * P * B)
    gen2.generate_batch_dev(S.ptr, P, S.len, S.stride, d_shares.ptr, B, P * B)
    box2.seal_share_rows_dev(codec2, [k[0] for k in keys], P, d_shares.ptr, n * P, B, B, d_boxes.ptr, slot, d_lens.ptr, esk)
    chain = mid - free_now()
    print(f"share buffer {share_bytes} B; newly held by the new call {grown} B ({100.0 * grown / share_bytes:.2f} %), by the chain {chain} B")
    assert np.array_equal(lens, _lens(d_lens, n * P))
    assert chain >= share_bytes
    assert grown < share_bytes / 2

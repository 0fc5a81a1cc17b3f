"""sda_secret_masker_mask_sealed_rows_dev: a participation's masking step and recipient encryption in one call
(participate.rs:52-72).  Full: the setup pass, then ONE kernel whose waves draw a participant's masks (sda-drbg-v1), add them onto
the secrets, store the masked secrets, varint-encode the masks and xor the XSalsa20 keystream in before anything is stored, then
the Poly1305 pass - no mask reaches device memory.  ChaCha: the expansion driver of mask_batch_dev, then the seed rows sealed from
scratch of the masker.

The reference of every case is tests/mask_sealed_cases.py (what the table reaches is proved in tests/test_mask_sealed_reach.py);
the "two-call chain" is sda_secret_masker_mask_batch_dev + sda_sealedbox_seal_share_rows_dev on fresh handles with the same
settings.  Box buffers are prefilled with 0xA5 and the masked rows lie among canaries, so a byte written past a row shows
(check_against of tests/test_participant_seal_gpu.py).  Integer work throughout: every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import generate_sealed_cases as gs
import mask_sealed_cases as ms
from conftest import load_golden, use_test_hooks
from test_participant_seal_gpu import PATTERN, _pattern_buffer, check_against

pytestmark = pytest.mark.gpu
CANARY = -0x0123456789ABCDEF
FULL = [c["name"] for c in ms.FULL_CASES]
CHACHA = [c["name"] for c in ms.CHACHA_CASES]


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def masker_of(case, rounds=20, key=ms.KEY):
    """a masker of the case's scheme; Full: in deterministic mode under `key` (None: production mode)"""
    from sda_amd import crypto
    if case["kind"] == "chacha":
        return crypto.SecretMasker(crypto.ChaCha(case["q"], case["len"], case["bits"]))
    m = crypto.SecretMasker(crypto.Full(case["q"]))
    if key is not None:
        m.set_drbg_key(key)
        if rounds != 20:
            m.set_drbg_rounds(rounds)
    return m


class Tile:
    """the secrets of a case resident in HBM with the case's stride and element offset, junk between and around the rows, and the
    buffer of the masked secrets, canaries everywhere (in place: the secrets' own buffer)"""

    def __init__(self, case, secrets=None):
        from sda_amd.device import DeviceBuffer
        sec = ms.secrets_of(case) if secrets is None else secrets
        self.P, self.len = sec.shape
        self.s_stride, self.m_stride, self.off = max(case["s_stride"], self.len), max(case["m_stride"], self.len), case["offset"]
        self.s_host = np.random.default_rng(7).integers(gs.I64_MIN, gs.I64_MAX, size=self.off + self.P * self.s_stride + 2, dtype=np.int64)
        for p in range(self.P):
            self.s_host[self.off + p * self.s_stride:self.off + p * self.s_stride + self.len] = sec[p]
        self.d_s = DeviceBuffer.from_numpy(self.s_host)
        self.in_place = case["in_place"]
        if self.in_place:
            assert self.s_stride == self.m_stride
            self.m_host, self.d_m = self.s_host, self.d_s
        else:
            self.m_host = np.full(self.off + self.P * self.m_stride + 2, CANARY, dtype=np.int64)
            self.d_m = DeviceBuffer.from_numpy(self.m_host)
        self.s_ptr, self.m_ptr = self.d_s.at(self.off), self.d_m.at(self.off)

    def masked(self):
        """(the masked rows [P][len], the whole buffer with those rows put back to what they were before the call)"""
        got = self.d_m.to_numpy()
        rows = np.stack([got[self.off + p * self.m_stride:self.off + p * self.m_stride + self.len] for p in range(self.P)]) if self.P else got[:0]
        rest = got.copy()
        for p in range(self.P):
            a = self.off + p * self.m_stride
            rest[a:a + self.len] = self.m_host[a:a + self.len]
        return rows, rest

    def check_masked(self, want, what):
        rows, rest = self.masked()
        assert np.array_equal(rest, self.m_host), f"{what}: an element outside the masked rows was written"
        bad = np.argwhere(rows != want)
        assert bad.size == 0, f"{what}: {len(bad)} masked secrets differ, the first at (participant, element) {tuple(bad[0])}"


def slot_of(case):
    from sda_amd import crypto
    return crypto.VarintCodec().slot_size(ms.mask_len(case)) + 48


def _lens(d_lens, rows):
    return np.frombuffer(d_lens.to_bytes(rows * 8), dtype="<u8").copy()


def _u32(words):
    return np.ascontiguousarray(words, dtype=np.uint32)


def run_new(case, masker, T, esk, pk=None):
    """the call under test (ChaCha: its seeded form, the library with the test hooks being active) -> (raw boxes, lengths, slot)"""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    slot = slot_of(case)
    d_boxes, d_lens = _pattern_buffer(T.P * slot), DeviceBytes(T.P * 8).zero()
    pk = ms.keys_of(case)[0] if pk is None else pk
    if case["kind"] == "chacha":
        words = _u32(ms.seeds_of(case))
        capi.check(capi.load().sda_debug_secret_masker_mask_sealed_rows_seeded_dev(
            masker._h, words.ctypes.data, codec._h, box._h, pk, esk, T.s_ptr, T.P, T.len, T.s_stride, 0, T.m_ptr, T.m_stride, d_boxes.ptr,
            slot, d_lens.ptr, None))
    else:
        masker.mask_sealed_rows_dev(codec, box, pk, T.s_ptr, T.P, T.len, T.s_stride, T.m_ptr, T.m_stride, d_boxes.ptr, slot, d_lens.ptr,
                                    first_participant=case["first"], esk=esk)
    return d_boxes.to_bytes(T.P * slot), _lens(d_lens, T.P), slot


def run_chain(case, masker, T, esk, pk=None):
    """mask_batch_dev into a mask buffer [P][mask_len], then seal_share_rows_dev over its rows"""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    slot, L = slot_of(case), ms.mask_len(case)
    d_masks = DeviceBuffer(max(T.P * L, 2)).zero()
    if case["kind"] == "chacha":
        words = _u32(ms.seeds_of(case))
        capi.check(capi.load().sda_debug_secret_masker_mask_batch_seeded_dev(masker._h, words.ctypes.data, T.s_ptr, T.P, T.len, T.s_stride, 0,
                                                                             d_masks.ptr, L, T.m_ptr, T.m_stride, None))
    else:
        masker.mask_batch_dev(T.s_ptr, T.P, T.len, T.s_stride, d_masks.ptr, L, T.m_ptr, T.m_stride, first_participant=case["first"])
    d_boxes, d_lens = _pattern_buffer(T.P * slot), DeviceBytes(T.P * 8).zero()
    pk = ms.keys_of(case)[0] if pk is None else pk
    box.seal_share_rows_dev(codec, [pk], T.P, d_masks.ptr, T.P, L, L, d_boxes.ptr, slot, d_lens.ptr, esk)
    return d_boxes.to_bytes(T.P * slot), _lens(d_lens, T.P)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(oracle boxes, masked secrets) of a case, computed once"""
    case = ms.BY_NAME[name]
    return tuple(ms.oracle_boxes(case)), ms.masked_of(case)


def _both(case, rounds=20):
    """the new call and the chain on fresh handles and fresh tiles -> ((raw, lens, masked rows, rest), (same of the chain), slot)"""
    esk = ms.esk_of(case)
    Ta, Tb = Tile(case), Tile(case)
    raw, lens, slot = run_new(case, masker_of(case, rounds), Ta, esk)
    raw2, lens2 = run_chain(case, masker_of(case, rounds), Tb, esk)
    return (raw, lens) + Ta.masked(), (raw2, lens2) + Tb.masked(), slot


# ---- 1. against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FULL)
def test_full_boxes_lengths_and_masked_secrets_equal_the_reference(gpu, name):
    from sda_amd import capi
    case = ms.BY_NAME[name]
    T, esk = Tile(case), ms.esk_of(case)
    raw, lens, slot = run_new(case, masker_of(case), T, esk)
    assert b"mask_seal_stream_kernel<20> + sbox_poly_kernel" == capi.load().sda_debug_last_kernel()
    boxes, masked = reference(name)
    print(f"{name} ({case['purpose']}): rows {len(boxes)} len {case['len']} lengths {lens.min()}..{lens.max()} slot {slot}")
    check_against(raw, lens, slot, boxes, esk, name)
    if case["small_order"]:                                              # refused: the masked rows exactly as passed
        assert all(b is None for b in boxes) and (lens == 0).all()
        assert np.array_equal(T.d_m.to_numpy(), T.m_host), "a refused row was masked"
    else:
        assert (lens > 48).all()
        T.check_masked(masked, name)


@pytest.mark.parametrize("name", CHACHA)
def test_chacha_boxes_lengths_and_masked_secrets_equal_the_reference(gpu, name):
    use_test_hooks()
    case = ms.BY_NAME[name]
    T, esk = Tile(case), ms.esk_of(case)
    raw, lens, slot = run_new(case, masker_of(case), T, esk)
    boxes, masked = reference(name)
    print(f"{name} (plan {case['plan']}): rows {len(boxes)} dimension {case['len']} words {case['words']} lengths {lens.min()}..{lens.max()} slot {slot}")
    check_against(raw, lens, slot, boxes, esk, name)
    assert (lens == 0).all() if case["small_order"] else (lens > 48).all()
    T.check_masked(masked, name)                                         # also under a small-order key: the expansion does not read the box state


# ---- 2. against the two-call chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FULL + CHACHA)
def test_same_bytes_as_the_two_call_chain(gpu, name):
    case = ms.BY_NAME[name]
    if case["kind"] == "chacha":
        use_test_hooks()
    (raw, lens, rows, rest), (raw2, lens2, rows2, rest2), slot = _both(case)
    assert np.array_equal(lens, lens2), f"{name}: lengths differ from mask_batch_dev + seal_share_rows_dev"
    assert raw == raw2, f"{name}: boxes (or the bytes around them) differ from mask_batch_dev + seal_share_rows_dev"
    if not case["small_order"] or case["kind"] == "chacha":             # (the chain's first call masks whatever the key is)
        assert np.array_equal(rows, rows2), f"{name}: masked secrets differ from mask_batch_dev's"
        assert np.array_equal(rest, rest2)


def test_chacha12_and_chacha8_handles_equal_the_chain_too(gpu):
    case = ms.BY_NAME["pm-3x2000"]
    for rounds in (12, 8):
        (raw, lens, rows, _), (raw2, lens2, rows2, _), slot = _both(case, rounds)
        assert np.array_equal(lens, lens2) and raw == raw2 and np.array_equal(rows, rows2), rounds
        want = ms.masked_of(case, rounds)
        assert np.array_equal(rows, want), rounds
        assert raw[:int(lens[0])] == ms.oracle_boxes(case, rounds)[0], rounds


def test_len_zero_gives_boxes_of_the_empty_message(gpu):
    from oracle import sealedbox_oracle as so
    case = dict(ms.BY_NAME["70x40"], participants=5, len=0, s_stride=0, m_stride=0)
    (pk, _), esk = ms.keys_of(case), ms.esk_of(case)
    T = Tile(case, np.zeros((5, 0), dtype=np.int64))
    raw, lens, slot = run_new(case, masker_of(case), T, esk)
    assert slot == 48 and list(lens) == [48] * 5
    assert all(raw[48 * r:48 * r + 48] == so.seal(b"", pk, esk[32 * r:32 * r + 32]) for r in range(5))
    assert np.array_equal(T.d_m.to_numpy(), T.m_host), "d_masked was written"


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBytes
    lib = capi.load()
    case = ms.BY_NAME["3x129-misaligned"]
    T, esk, (pk, _) = Tile(case), ms.esk_of(case), ms.keys_of(case)
    slot = slot_of(case)
    assert slot % 16 == 0
    masker, codec, box = masker_of(case), crypto.VarintCodec(), crypto.SealedBox()
    d_boxes, d_lens = _pattern_buffer(T.P * slot + 64), DeviceBytes(T.P * 8).zero()
    good = dict(m=masker._h, codec=codec._h, b=box._h, pk=pk, esk=esk, d_secrets=T.s_ptr, participants=T.P, len=T.len, secrets_stride=T.s_stride,
                first_participant=0, d_masked=T.m_ptr, masked_stride=T.m_stride, d_boxes=d_boxes.ptr, slot_bytes=slot, d_row_bytes=d_lens.ptr,
                stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sda_secret_masker_mask_sealed_rows_dev(*[a[k] for k in good])

    untouched = bytes([PATTERN]) * (T.P * slot + 64)

    def nothing_written(what):
        assert d_boxes.to_bytes() == untouched, what + ": the box buffer was written"
        assert np.array_equal(T.d_m.to_numpy(), T.m_host), what + ": d_masked was written"
        assert np.array_equal(T.d_s.to_numpy(), T.s_host), what + ": d_secrets was written"

    none = crypto.SecretMasker(crypto.NoMask())
    signed = crypto.SecretMasker(crypto.Full(case["q"]))
    signed.set_value_mode("rust_signed")
    chacha = crypto.SecretMasker(crypto.ChaCha(case["q"], T.len, 128))
    bad, unsupported = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    cases = {"NULL masker": (dict(m=None), bad), "NULL codec": (dict(codec=None), bad), "NULL box handle": (dict(b=None), bad),
             "NULL pk": (dict(pk=None), bad), "NULL d_secrets": (dict(d_secrets=None), bad), "NULL d_masked": (dict(d_masked=None), bad),
             "NULL d_boxes": (dict(d_boxes=None), bad), "NULL d_row_bytes": (dict(d_row_bytes=None), bad),
             "secrets_stride < len": (dict(secrets_stride=T.len - 1), bad), "masked_stride < len": (dict(masked_stride=T.len - 1), bad),
             "slot_bytes not a multiple of 16": (dict(slot_bytes=slot + 8), bad), "slot_bytes too small": (dict(slot_bytes=slot - 16), bad),
             "d_boxes misaligned": (dict(d_boxes=d_boxes.ptr + 8), bad), "stream ids at 2^56": (dict(first_participant=(1 << 56) - 2), bad),
             "first stream id past 2^56": (dict(first_participant=1 << 56), bad),
             "the None scheme": (dict(m=none._h), unsupported), "SDA_VALUES_RUST_SIGNED": (dict(m=signed._h), unsupported),
             "ChaCha: len != dimension": (dict(m=chacha._h, len=T.len - 1, slot_bytes=96), capi.ERR_ASSERTION),
             "ChaCha: slot too small for the seed": (dict(m=chacha._h, slot_bytes=80), bad),
             "ChaCha: in place": (dict(m=chacha._h, d_masked=T.s_ptr, masked_stride=T.s_stride, slot_bytes=96), bad),
             "ChaCha: overlapping by one row": (dict(m=chacha._h, d_masked=T.s_ptr + 8 * T.s_stride, masked_stride=T.s_stride, participants=2, slot_bytes=96), bad)}
    for what, (kw, status) in cases.items():
        assert call(**kw) == status, what
        nothing_written(what)
    assert call(m=none._h) == unsupported and b"mask_batch_dev" in lib.sda_last_error()
    if lib.sda_device_count() > 1:                                       # handles on different devices
        capi.check(lib.sda_set_device(1))
        try:
            other_box, other_codec, other_masker = crypto.SealedBox(), crypto.VarintCodec(), masker_of(case)
        finally:
            capi.check(lib.sda_set_device(0))
        for kw in (dict(b=other_box._h), dict(codec=other_codec._h), dict(m=other_masker._h), dict(b=other_box._h, codec=other_codec._h)):
            assert call(**kw) == bad
            nothing_written("handles on two devices")
    assert call(participants=0) == capi.OK
    nothing_written("participants == 0")
    assert call(m=chacha._h, participants=0, slot_bytes=96) == capi.OK
    nothing_written("participants == 0, ChaCha")
    # ... and after all the refusals the handles still work
    assert call() == capi.OK
    boxes, masked = reference(case["name"])
    check_against(d_boxes.to_bytes(T.P * slot), _lens(d_lens, T.P), slot, boxes, esk, "after the refusals")
    T.check_masked(masked, "after the refusals")
    from sda_amd.device import DeviceBuffer
    d_out = DeviceBuffer.from_numpy(np.full(T.P * T.len, CANARY, dtype=np.int64))
    d_cb, d_cl = _pattern_buffer(T.P * 96), DeviceBytes(T.P * 8).zero()
    assert call(m=chacha._h, d_masked=d_out.ptr, masked_stride=T.len, d_boxes=d_cb.ptr, slot_bytes=96, d_row_bytes=d_cl.ptr, esk=None) == capi.OK
    assert (_lens(d_cl, T.P) > 48).all() and (d_out.to_numpy() != CANARY).all()


# ---- 4. production mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["full", "chacha"])
def test_two_production_calls_differ_and_every_box_unmasks(gpu, kind):
    """OS entropy, no injected key, seeds or ephemeral secrets: the boxes opened by the oracle hold masks that take d_masked back to
    the secrets; a second call on the same inputs has fresh ephemeral keys and fresh masks"""
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    base = ms.BY_NAME["3x129-misaligned"] if kind == "full" else ms.BY_NAME["chacha-433-1000x5-128"]
    case = dict(base, small_order=False)
    q, P, L = case["q"], case["participants"], case["len"]
    sec = ms.secrets_of(case)
    pk, sk = ms.keys_of(case)
    masker, codec, box = masker_of(case, key=None), crypto.VarintCodec(), crypto.SealedBox()
    slot = slot_of(case)
    seen = []
    for _ in range(2):
        T = Tile(case)
        d_boxes, d_lens = _pattern_buffer(P * slot), DeviceBytes(P * 8).zero()
        masker.mask_sealed_rows_dev(codec, box, pk, T.s_ptr, P, L, T.s_stride, T.m_ptr, T.m_stride, d_boxes.ptr, slot, d_lens.ptr)
        raw, lens = d_boxes.to_bytes(P * slot), _lens(d_lens, P)
        assert (lens > 48).all()
        rows, rest = T.masked()
        assert np.array_equal(rest, T.m_host)
        sent = [coracle.varint_decode(so.seal_open(raw[p * slot:p * slot + int(lens[p])], pk, sk)) for p in range(P)]
        for p in range(P):
            assert len(sent[p]) == ms.mask_len(case)
            mask = sent[p] if kind == "full" else coracle.chacha_expand(sent[p], q, L)
            assert ((mask >= 0) & (mask < q)).all()
            assert [(int(x) - int(m)) % q for x, m in zip(rows[p], mask)] == [int(s) % q for s in sec[p]], f"participant {p} does not unmask"
        seen.append((raw, sent))
    (raw1, sent1), (raw2, sent2) = seen
    assert all(raw1[p * slot:p * slot + 32] != raw2[p * slot:p * slot + 32] for p in range(P)), "ephemeral keys repeat"
    assert all(not np.array_equal(sent1[p], sent2[p]) for p in range(P)), "masks repeat: the call key (or the seed) did not change"
    assert all(not np.array_equal(sent1[0], sent1[p]) for p in range(1, P))


# ---- 5. the protocol loop on sealed bytes ----------------------------------------------------------------------------------------
def _sealed_loop(agg, inputs, subset=None):
    """participate_sealed -> clerk_sealed_job per clerk -> reconstruct_sealed_job and combine_sealed_job -> unmask"""
    from oracle import sealedbox_oracle as so
    from sda_amd import capi, crypto
    sch, msch, dim = agg.committee_sharing_scheme, agg.masking_scheme, agg.vector_dimension
    n = sch.output_size()
    rng = np.random.default_rng(n + dim)
    sks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(n + 1)]
    pks = [so.x25519_base(s) for s in sks]
    rpk, rsk = pks[n], sks[n]
    mask_job, clerk_jobs = crypto.participate_sealed(agg, inputs, rpk, pks[:n])
    assert len(clerk_jobs) == n
    row_len = dim if isinstance(sch, crypto.Additive) else -(-dim // sch.secret_count)
    results = [crypto.ShareCombiner(sch).clerk_sealed_job(clerk_jobs[c], pks[c], sks[c], rpk, row_len) for c in range(n)]
    subset = list(range(n)) if subset is None else subset
    job = crypto.JobContainer.build(capi.JOB_SEALED, [results[c] for c in subset])
    masked_out = crypto.SecretReconstructor(sch, dim).reconstruct_sealed_job(bytes(job), subset, rpk, rsk)
    if not msch.has_mask():
        assert mask_job is None
        return masked_out
    assert crypto.JobContainer.parse(mask_job).layout.rows == len(inputs)
    mask = crypto.MaskCombiner(msch).combine_sealed_job(mask_job, rpk, rsk, dim)
    return crypto.SecretUnmasker(msch).unmask((mask, masked_out))


@pytest.mark.parametrize("kind", ["full-additive", "full-packed", "chacha-packed"])
def test_the_loop_on_sealed_bytes(gpu, kind):
    from sda_amd import crypto
    case = gs.BY_NAME["additive-n3" if kind == "full-additive" else "B129"]
    q, dim = case["p"], case["len"]
    if case["additive"]:
        sch, subset = crypto.Additive(case["n"], q), None
    else:
        sch, subset = crypto.PackedShamir(case["k"], case["n"], case["t"], q, *gs.omegas(case)), [7, 0, 3, 5, 2]
    msch = crypto.ChaCha(q, dim, 128) if kind.startswith("chacha") else crypto.Full(q)
    inputs = np.random.default_rng(24 + dim).integers(0, q, size=(24, dim), dtype=np.int64)
    out = _sealed_loop(crypto.Aggregation(dim, q, msch, sch), inputs, subset)
    truth = np.array([sum(int(x) for x in inputs[:, i]) % q for i in range(dim)], dtype=np.int64)
    assert np.array_equal(out, truth)


@pytest.mark.parametrize("name", ["F2_with_fullmask", "F3_with_chachamask", "F4c_packedshamir_fullmask"])
def test_the_loop_on_sealed_bytes_gives_the_golden_outputs(gpu, name):
    from sda_amd import crypto
    from test_parity_gpu import _mask_scheme, _scheme
    sc = {s["name"]: s for s in load_golden("full_loop.json")["scenarios"]}[name]
    a = sc["aggregation"]
    assert a["masking_scheme"]["kind"] != "None"
    agg = crypto.Aggregation(a["vector_dimension"], a["modulus"], _mask_scheme(a["masking_scheme"]), _scheme(a["committee_sharing_scheme"]))
    out = _sealed_loop(agg, np.array(sc["inputs"], dtype=np.int64), sc["clerk_subset"])
    assert list(map(int, out)) == sc["stages"]["canonical"]["output"]
    assert list(map(int, crypto.RecipientOutput(a["modulus"], out).positive().values)) == sc["expected_positive"]


def test_participate_sealed_without_a_mask_shares_the_secrets_as_they_are(gpu):
    from sda_amd import crypto
    sc = {s["name"]: s for s in load_golden("full_loop.json")["scenarios"]}["F1_simple"]
    agg = crypto.Aggregation(4, 433, crypto.NoMask(), crypto.Additive(3, 433))
    assert list(map(int, _sealed_loop(agg, np.array(sc["inputs"], dtype=np.int64)))) == sc["expected_positive"]


# ---- 6. the kernels that share the encode loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,L,stride,offset", [(17, 333, None, 0), (6, 1300, 1303, 1)])
def test_existing_encode_and_seal_kernels_are_unchanged(gpu, rows, L, stride, offset):
    """varint_seal_stream_kernel (seal_share_rows_dev) against the oracle, varint_stream_encode_kernel (encode_rows_dev, then
    seal_rows_dev) against it: they share encode_row and EncXSalsa with the new kernel"""
    from test_participant_seal_gpu import _keys, check
    pk, _ = _keys(rows * 131 + L)
    shares = np.random.default_rng(rows + L).integers(0, gs.P62, size=(rows, L), dtype=np.int64)
    check(shares, [pk], stride=stride, offset=offset)


# ---- 7. footprint --------------------------------------------------------------------------------------------------------------
def test_footprint_no_mask_buffer(gpu):
    """Full, 32 participants x 200,000 values: the chain's mask buffer is participants * len * 8 = 51.2 MB.  The chain needs the
    whole buffer, the new call none of it, so what the three handles newly hold after the call must stay below half that figure
    (it is the per-row key state, the Poly1305 partials, the staged keys and the lengths)."""
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    lib = use_test_hooks()                                       # sda_debug_mem_info lives in the library with the test hooks
    P, L = 32, 200_000
    case = dict(ms.BY_NAME["2x460"], participants=P, len=L, s_stride=L, m_stride=L)
    mask_bytes = P * L * 8
    assert mask_bytes == 51_200_000
    (pk, _), esk = ms.keys_of(case), ms.esk_of(case)
    sec = np.random.default_rng(5).integers(gs.I64_MIN, gs.I64_MAX, size=(P, L), dtype=np.int64)
    d_sec, d_masked = DeviceBuffer.from_numpy(sec), DeviceBuffer(P * L)
    masker, codec, box = masker_of(case), crypto.VarintCodec(), crypto.SealedBox()
    slot = slot_of(case)
    d_boxes, d_lens = DeviceBytes(P * slot), DeviceBytes(P * 8).zero()

    def free_now():
        synchronize()
        f, t = C.c_size_t(), C.c_size_t()
        capi.check(lib.sda_debug_mem_info(C.byref(f), C.byref(t)))
        return f.value

    before = free_now()
    masker.mask_sealed_rows_dev(codec, box, pk, d_sec.ptr, P, L, L, d_masked.ptr, L, d_boxes.ptr, slot, d_lens.ptr, esk=esk)
    grown = before - free_now()
    lens = _lens(d_lens, P)
    for p in (0, 17, P - 1):
        mask = coracle.drbg_fill(ms.KEY, p, L, 1, case["q"])
        assert d_boxes.to_bytes(int(lens[p]), p * slot) == so.seal(coracle.varint_encode(mask), pk, esk[32 * p:32 * p + 32]), f"row {p}"
        want = ((sec[p].astype(object) % case["q"] + mask.astype(object)) % case["q"]).astype(np.int64)
        assert np.array_equal(d_masked.to_numpy(L, p * L), want), f"masked row {p}"
    # the chain on fresh handles: its mask buffer alone is that figure
    masker2, codec2, box2 = masker_of(case), crypto.VarintCodec(), crypto.SealedBox()
    mid = free_now()
    d_masks = DeviceBuffer(P * L)
    masker2.mask_batch_dev(d_sec.ptr, P, L, L, d_masks.ptr, L, d_masked.ptr, L)
    box2.seal_share_rows_dev(codec2, [pk], P, d_masks.ptr, P, L, L, d_boxes.ptr, slot, d_lens.ptr, esk)
    chain = mid - free_now()
    print(f"mask buffer {mask_bytes} B; newly held by the new call {grown} B ({100.0 * grown / mask_bytes:.2f} %), by the chain {chain} B")
    assert np.array_equal(lens, _lens(d_lens, P))
    assert chain >= mask_bytes
    assert grown < mask_bytes / 2

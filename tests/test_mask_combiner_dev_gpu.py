"""The mask combiner's device form on the GPU: sda_mask_combiner_begin_dev / update_dev / update_sealed_rows_dev / finish_dev
(receive.rs:101-118 with the masks in HBM) against the C oracle and against the host form sda_mask_combiner_combine, bit for bit.
tests/test_mask_combiner_reach.py proves on the CPU that the ChaCha seeds used here reach every outcome of the repair plan."""
import functools

import numpy as np
import pytest

import mask_combiner_cases as mc

pytestmark = pytest.mark.gpu
P62 = mc.P62


def u32(buf, n=1):
    return np.frombuffer(buf.to_bytes(), dtype="<u4")[:n].copy()


def _keys(seed):
    from oracle import sealedbox_oracle as so
    sk = bytes(np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8))
    return so.x25519_base(sk), sk


class Job:
    """boxes resident in HBM in the slotted layout: box r at d_boxes + r * slot, lens[r] bytes"""

    def __init__(self, d_boxes, slot, d_lens, rows, keep=()):
        self.d_boxes, self.slot, self.d_lens, self.rows, self.keep = d_boxes, slot, d_lens, rows, keep


def seal_rows(values, pk):
    """participate.rs:82-101 on the device: every row of `values` varint-encoded and sealed in one call (OS-entropy ephemeral keys)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    P, L = values.shape
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_v = DeviceBuffer.from_numpy(values)
    slot = max(codec.slot_size(L), 16) + 48
    d_boxes, d_len = DeviceBytes(P * slot).zero(), DeviceBytes(P * 8).zero()
    box.seal_share_rows_dev(codec, [pk], P, d_v.ptr, P, L, L, d_boxes.ptr, slot, d_len.ptr)
    synchronize()
    return Job(d_boxes, slot, d_len, P)


def upload_boxes(boxes, lens=None):
    """host-made boxes (the oracle's, or tampered ones) as an SDAJOBv1 blob in HBM; `lens` overrides the length fields"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    job = crypto.JobContainer.build(0, boxes)
    L = job.layout
    blob = bytearray(bytes(job))
    if lens is not None:
        blob[L.lengths_offset:L.lengths_offset + 8 * len(boxes)] = np.array(lens, dtype="<u8").tobytes()
    d = DeviceBytes.from_bytes(blob)

    class _At:                                    # the blob owns the memory; the views are plain addresses
        def __init__(self, ptr): self.ptr = ptr
    return Job(_At(d.ptr + L.payload_offset), L.slot_bytes, _At(d.ptr + L.lengths_offset), len(boxes), keep=(d,))


def combine_sealed(scheme, job, pk, sk, dim, calls=1):
    """begin_dev, the sealed update in `calls` pieces, finish_dev -> (result, status, d_ok)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    comb = crypto.MaskCombiner(scheme)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_status, d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * job.rows).zero()
    comb.begin_dev(dim)
    per = (job.rows + calls - 1) // calls
    for r0 in range(0, job.rows, per):
        n = min(per, job.rows - r0)
        comb.update_sealed_rows_dev(codec, box, pk, sk, job.d_boxes.ptr + r0 * job.slot, job.slot, job.d_lens.ptr + 8 * r0, n,
                                    job.slot, d_status.ptr, d_ok.ptr + 4 * r0)
    d_out = DeviceBuffer(dim)
    comb.finish_dev(d_out.ptr, dim)
    return d_out.to_numpy()[:dim], int(u32(d_status)[0]), u32(d_ok, job.rows)


# ---- 1. ChaCha versus the oracle and the host form ---------------------------------------------------------------------------
@pytest.mark.parametrize("q,dim,seeds", mc.CHACHA_SHAPES)
def test_chacha_update_dev_vs_oracle_and_host_form(gpu, q, dim, seeds):
    from oracle import coracle
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    S = mc.seed_matrix(q, dim, seeds)
    want = coracle.chacha_combine(S, q, dim)
    comb = crypto.MaskCombiner(crypto.ChaCha(q, dim, 128))
    assert np.array_equal(comb.combine(list(S)), want)
    d_S, d_out = DeviceBuffer.from_numpy(S), DeviceBuffer(dim)
    first = (seeds - 1) * 2 // 5
    sizes = [first, 0, 1, seeds - 1 - first]                                  # three calls of unequal size and a rows == 0 call
    assert sum(sizes) == seeds
    comb.begin_dev(dim)
    r0 = 0
    for n in sizes:
        comb.update_dev(d_S.at(4 * r0), n, 4, 4)
        r0 += n
    comb.finish_dev(d_out.ptr, dim)
    got = d_out.to_numpy()
    print(f"q {q} dim {dim} seeds {seeds}: calls {sizes}, mismatches {int((got != want).sum())}")
    assert np.array_equal(got, want)
    # the handle serves another job, and the host form after it
    comb.begin_dev(dim)
    comb.update_dev(d_S.ptr, seeds, 4, 4)
    comb.finish_dev(d_out.ptr, dim)
    assert np.array_equal(d_out.to_numpy(), want)
    assert np.array_equal(comb.combine(list(S)), want)


def test_chacha_dimension_and_state_checks(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    comb = crypto.MaskCombiner(crypto.ChaCha(P62, 100, 128))
    d = DeviceBuffer(400).zero()
    with pytest.raises(crypto.SdaError) as e:
        comb.update_dev(d.ptr, 1, 4, 4)
    assert e.value.code == capi.ERR_STATE
    with pytest.raises(crypto.SdaError) as e:
        comb.begin_dev(99)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    pk, sk = _keys(40)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()

    def sealed(d_boxes=d.ptr, slot=64, d_lens=d.ptr + 1024, rows=4, max_box=64, status=d.ptr + 2048):
        comb.update_sealed_rows_dev(codec, box, pk, sk, d_boxes, slot, d_lens, rows, max_box, status)
    with pytest.raises(crypto.SdaError) as e:
        sealed()
    assert e.value.code == capi.ERR_STATE
    comb.begin_dev(100)
    sealed(d_boxes=0, rows=0)                                                  # rows == 0: nothing is looked at, nothing launched
    for call in (lambda: comb.update_dev(0, 1, 4, 4), lambda: comb.update_dev(d.ptr, 1, 4, 3), lambda: comb.finish_dev(d.ptr, 99),
                 lambda: comb.finish_dev(0, 100), lambda: sealed(d_boxes=0), lambda: sealed(d_lens=0), lambda: sealed(status=0),
                 lambda: sealed(d_boxes=d.ptr + 8), lambda: sealed(slot=72), lambda: sealed(max_box=80)):
        with pytest.raises(crypto.SdaError) as e:
            call()
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
    comb.finish_dev(d.ptr, 100)
    with pytest.raises(crypto.SdaError) as e:
        comb.finish_dev(d.ptr, 100)
    assert e.value.code == capi.ERR_STATE


def test_more_seeds_than_one_launch_takes(gpu):
    """2^20 seeds go into one launch: three more make a second chunk, which reuses the key, record and plan scratch of the first in
    stream order.  Short streams over the 2^-11 modulus, so that both chunks have seeds on their repair lists."""
    from oracle import coracle
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    q, dim, seeds = mc.Q_SHIFT, 3, (1 << 20) + 3
    S = np.random.default_rng(20).integers(0, 1 << 32, size=(seeds, 4), dtype=np.int64)
    S[-1] = S[int(np.nonzero(mc.rejections(S[:4096], q, dim)[0])[0][0])]      # the last chunk gets a seed that needs a repair
    assert mc.rejections(S[-1:], q, dim)[0][0] >= 1
    comb = crypto.MaskCombiner(crypto.ChaCha(q, dim, 128))
    d_S, d_out = DeviceBuffer.from_numpy(S), DeviceBuffer(dim)
    comb.begin_dev(dim)
    comb.update_dev(d_S.ptr, seeds, 4, 4)
    comb.finish_dev(d_out.ptr, dim)
    assert np.array_equal(d_out.to_numpy(), coracle.chacha_combine(S, q, dim))


# ---- 2. seed forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_len", [0, 2, 8, 10])
def test_seed_forms(gpu, row_len):
    from oracle import coracle
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    q, dim, rows = P62, 1237, 3
    special = [-1, (1 << 40) + 5, 1 << 32]
    stride = row_len + 3
    rng = np.random.default_rng(row_len)
    M = rng.integers(-(1 << 62), 1 << 62, size=(rows, stride), dtype=np.int64)      # the padding is junk that must not be read as seed
    for r in range(rows):
        for w in range(row_len):
            if (r + w) % 2 == 0:
                M[r, w] = special[(r + w // 2) % 3]
    total = np.zeros(dim, dtype=object)
    for r in range(rows):
        words = [int(x) & 0xFFFFFFFF for x in M[r, :row_len]]                      # `as u32` (chacha.rs:62-64)
        total = (total + coracle.chacha_expand(words, q, dim).astype(object)) % q
    want = np.array(total, dtype=np.int64)
    comb = crypto.MaskCombiner(crypto.ChaCha(q, dim, 128))
    assert np.array_equal(comb.combine([M[r, :row_len] for r in range(rows)]), want)
    d_M, d_out = DeviceBuffer.from_numpy(M), DeviceBuffer(dim)
    comb.begin_dev(dim)
    comb.update_dev(d_M.ptr, rows, row_len, stride)
    comb.finish_dev(d_out.ptr, dim)
    assert np.array_equal(d_out.to_numpy(), want)


@pytest.mark.parametrize("mode", ["canonical", "rust_signed"])
def test_zero_seeds_give_zeros_in_both_value_modes(gpu, mode):
    from oracle import coracle
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    q, dim = P62, 777
    comb = crypto.MaskCombiner(crypto.ChaCha(q, dim, 128))
    comb.set_value_mode(mode)
    d_out = DeviceBuffer.from_numpy(np.full(dim, 5, dtype=np.int64))
    comb.begin_dev(dim)
    comb.finish_dev(d_out.ptr, dim)
    assert np.array_equal(d_out.to_numpy(), np.zeros(dim, dtype=np.int64))             # chacha.rs:58
    S = mc.seed_matrix(q, dim, 3)
    d_S = DeviceBuffer.from_numpy(S)
    comb.begin_dev(dim)
    comb.update_dev(d_S.ptr, 3, 4, 4)
    comb.finish_dev(d_out.ptr, dim)
    assert np.array_equal(d_out.to_numpy(), coracle.chacha_combine(S, q, dim))         # both modes give the same numbers


# ---- 3. stream order: the caller's buffer is free as soon as later work on the stream overwrites it ------------------------
def test_stream_order_the_row_buffer_is_reused_between_updates(gpu):
    import ctypes as C
    from oracle import coracle
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    q, dim, n = mc.STREAM_ORDER
    A, B = mc.stream_order_seeds()
    comb = crypto.MaskCombiner(crypto.ChaCha(q, dim, 128))
    d_rows, d_out = DeviceBuffer.from_numpy(A), DeviceBuffer(dim)
    comb.begin_dev(dim)
    comb.update_dev(d_rows.ptr, n, 4, 4)
    capi.check(capi.load().sda_dev_upload(C.c_void_p(d_rows.ptr), B.ctypes.data_as(C.c_void_p), B.size * 8))   # same (null) stream
    comb.update_dev(d_rows.ptr, n, 4, 4)
    comb.finish_dev(d_out.ptr, dim)
    assert np.array_equal(d_out.to_numpy(), coracle.chacha_combine(np.vstack([A, B]), q, dim))


# ---- 4. sealed ChaCha seeds -------------------------------------------------------------------------------------------------------
SEALED_P, SEALED_DIM = 37, 1000


@functools.lru_cache(maxsize=None)
def sealed_case():
    """37 seeds of 4 words, the oracle's boxes of their varint encodings (injected ephemeral keys), and every seed's mask"""
    from oracle import coracle, sealedbox_oracle as so
    pk, sk = _keys(41)
    S = np.random.default_rng(37).integers(0, 1 << 32, size=(SEALED_P, 4), dtype=np.int64)
    esks = [bytes(np.random.default_rng(1000 + r).integers(0, 256, 32, dtype=np.uint8)) for r in range(SEALED_P)]
    boxes = [so.seal(coracle.varint_encode(S[r]), pk, esks[r]) for r in range(SEALED_P)]
    masks = [coracle.chacha_expand([int(w) for w in S[r]], P62, SEALED_DIM) for r in range(SEALED_P)]
    return pk, sk, S, boxes, masks


def mask_sum(masks, skip=()):
    total = np.zeros(SEALED_DIM, dtype=object)
    for r, m in enumerate(masks):
        if r not in skip:
            total = (total + m.astype(object)) % P62
    return np.array(total, dtype=np.int64)


def test_sealed_chacha_seeds_sealed_on_the_device(gpu):
    from oracle import coracle
    from sda_amd import crypto
    pk, sk, S, _, _ = sealed_case()
    job = seal_rows(S, pk)
    got, status, ok = combine_sealed(crypto.ChaCha(P62, SEALED_DIM, 128), job, pk, sk, SEALED_DIM, calls=2)
    assert status == 0 and ok.all()
    assert np.array_equal(got, coracle.chacha_combine(S, P62, SEALED_DIM))


def test_sealed_chacha_seeds_sealed_by_the_oracle(gpu):
    from oracle import coracle
    from sda_amd import crypto
    pk, sk, S, boxes, masks = sealed_case()
    want = coracle.chacha_combine(S, P62, SEALED_DIM)
    assert np.array_equal(mask_sum(masks), want)
    got, status, ok = combine_sealed(crypto.ChaCha(P62, SEALED_DIM, 128), upload_boxes(boxes), pk, sk, SEALED_DIM)
    assert status == 0 and ok.all()
    assert np.array_equal(got, want)
    # the convenience form on the same boxes as an SDAJOBv1 blob
    blob = bytes(crypto.JobContainer.build(capi_const("JOB_SEALED"), boxes))
    assert np.array_equal(crypto.MaskCombiner(crypto.ChaCha(P62, SEALED_DIM, 128)).combine_sealed_job(blob, pk, sk), want)


def capi_const(name):
    from sda_amd import capi
    return getattr(capi, name)


def test_sealed_rows_that_fail_add_nothing(gpu):
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import crypto
    pk, sk, S, boxes, masks = sealed_case()
    boxes = list(boxes)
    lens = [len(b) for b in boxes]
    t = bytearray(boxes[3]); t[50] ^= 0x04; boxes[3] = bytes(t)               # one tampered ciphertext byte
    lens[10] = 47                                                              # one 47-byte row
    other_pk, _ = _keys(99)
    boxes[20] = so.seal(coracle.varint_encode(S[20]), other_pk, bytes(range(32)))   # one row sealed to another key
    bad = {3, 10, 20}
    got, status, ok = combine_sealed(crypto.ChaCha(P62, SEALED_DIM, 128), upload_boxes(boxes, lens), pk, sk, SEALED_DIM)
    print(f"status {status}, rows refused {sorted(np.nonzero(ok == 0)[0])}")
    assert status & 16
    assert set(np.nonzero(ok == 0)[0]) == bad
    assert np.array_equal(got, mask_sum(masks, skip=bad))


def test_sealed_payload_that_ends_inside_a_value(gpu):
    from oracle import sealedbox_oracle as so
    from sda_amd import crypto
    pk, sk, S, boxes, masks = sealed_case()
    boxes = list(boxes[:6])
    boxes[2] = so.seal(b"\x80", pk, bytes(range(1, 33)))
    got, status, ok = combine_sealed(crypto.ChaCha(P62, SEALED_DIM, 128), upload_boxes(boxes), pk, sk, SEALED_DIM)
    assert status == 4 and ok.all()                                            # the box authenticates; its payload is no varint vector
    assert np.array_equal(got, mask_sum(masks[:6], skip={2}))


def test_sealed_overlong_value_and_words_past_the_eighth(gpu):
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import crypto
    pk, sk, S, boxes, masks = sealed_case()
    boxes = list(boxes[:4])
    boxes[1] = so.seal(b"\x81" * 10 + b"\x01", pk, bytes(range(2, 34)))        # a value of 11 bytes
    ten = [5, -1, (1 << 40) + 5, 1 << 32, 7, 8, 9, 10, 11, 12]                   # ten words: `as u32`, the last two ignored
    boxes[3] = so.seal(coracle.varint_encode(ten), pk, bytes(range(3, 35)))
    got, status, ok = combine_sealed(crypto.ChaCha(P62, SEALED_DIM, 128), upload_boxes(boxes), pk, sk, SEALED_DIM)
    assert status == 1 and ok.all()
    m3 = coracle.chacha_expand([w & 0xFFFFFFFF for w in ten[:8]], P62, SEALED_DIM)
    assert np.array_equal(got, mask_sum([masks[0], masks[2], m3]))


def test_sealed_empty_seed(gpu):
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import crypto
    pk, sk, S, boxes, masks = sealed_case()
    empty = so.seal(b"", pk, bytes(range(4, 36)))
    assert len(empty) == 48
    got, status, ok = combine_sealed(crypto.ChaCha(P62, SEALED_DIM, 128), upload_boxes([boxes[0], empty]), pk, sk, SEALED_DIM)
    assert status == 0 and ok.all()
    assert np.array_equal(got, mask_sum([masks[0], coracle.chacha_expand([], P62, SEALED_DIM)]))


def test_sealed_seeds_through_the_rejection_repair(gpu):
    """the counted fast pass, the plan and both listed repairs from sealed rows: the shape meant for both lists, 300 boxes"""
    from oracle import coracle
    from sda_amd import crypto
    q, dim, seeds = mc.BOTH_LISTS
    pk, sk = _keys(43)
    S = mc.seed_matrix(q, dim, seeds)
    got, status, ok = combine_sealed(crypto.ChaCha(q, dim, 128), seal_rows(S, pk), pk, sk, dim)
    assert status == 0 and ok.all()
    assert np.array_equal(got, coracle.chacha_combine(S, q, dim))
    # ... and exact order for all, whose key count lives on the device too
    q, dim, seeds = mc.Q_HEAVY, 3000, 6
    S = mc.seed_matrix(q, dim, seeds)
    got, status, ok = combine_sealed(crypto.ChaCha(q, dim, 128), seal_rows(S, pk), pk, sk, dim)
    assert status == 0 and ok.all()
    assert np.array_equal(got, coracle.chacha_combine(S, q, dim))


# ---- 5. Full masks --------------------------------------------------------------------------------------------------------------------
FULL_P, FULL_L = 12, 1001


def test_full_update_dev_and_sealed_form(gpu):
    from oracle import coracle
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    M = np.random.default_rng(12).integers(0, P62, size=(FULL_P, FULL_L), dtype=np.int64)
    want = coracle.combine(P62, M)
    comb = crypto.MaskCombiner(crypto.Full(P62))
    assert np.array_equal(comb.combine(list(M)), want)
    stride = FULL_L + 3
    padded = np.full((FULL_P, stride), -7, dtype=np.int64)
    padded[:, :FULL_L] = M
    d_M, d_out = DeviceBuffer.from_numpy(padded), DeviceBuffer(FULL_L)
    comb.begin_dev(FULL_L)
    comb.update_dev(d_M.ptr, 5, FULL_L, stride)
    comb.update_dev(d_M.at(5 * stride), 0, FULL_L, stride)
    comb.update_dev(d_M.at(5 * stride), FULL_P - 5, FULL_L, stride)
    with pytest.raises(AssertionError, match="full.rs:43"):
        comb.update_dev(d_M.ptr, 1, FULL_L - 1, stride)
    comb.finish_dev(d_out.ptr, FULL_L)
    assert np.array_equal(d_out.to_numpy(), want)
    # the same rows sealed: the mask combiner's sums are the share combiner's sealed sums
    pk, sk = _keys(12)
    job = seal_rows(M, pk)
    got, status, ok = combine_sealed(crypto.Full(P62), job, pk, sk, FULL_L, calls=2)
    sc = crypto.ShareCombiner(crypto.Additive(3, P62))
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_status, d_sums = DeviceBytes(4).zero(), DeviceBuffer(FULL_L)
    sc.begin_dev(1, FULL_L)
    sc.update_sealed_rows_dev(codec, box, pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, FULL_P, job.slot, d_status.ptr)
    sc.finish_dev(d_sums.ptr)
    assert status == 0 == int(u32(d_status)[0]) and ok.all()
    assert np.array_equal(got, d_sums.to_numpy()) and np.array_equal(got, want)


def test_full_signed_mode(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    q = P62
    M = np.random.default_rng(13).integers(-(q - 1), q, size=(FULL_P, FULL_L), dtype=np.int64)
    comb = crypto.MaskCombiner(crypto.Full(q))
    comb.set_value_mode("rust_signed")
    want = comb.combine(list(M))
    assert (want < 0).any(), "the signed case needs a negative running value"
    d_M, d_out = DeviceBuffer.from_numpy(M), DeviceBuffer(FULL_L)
    comb.begin_dev(FULL_L)
    comb.update_dev(d_M.ptr, 7, FULL_L, FULL_L)
    comb.update_dev(d_M.at(7 * FULL_L), FULL_P - 7, FULL_L, FULL_L)
    pk, sk = _keys(14)
    job = seal_rows(np.abs(M[:2]), pk)
    with pytest.raises(crypto.SdaError) as e:
        comb.update_sealed_rows_dev(crypto.VarintCodec(), crypto.SealedBox(), pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, 2,
                                    job.slot, DeviceBuffer(1).zero().ptr)
    assert e.value.code == capi.ERR_UNSUPPORTED
    comb.finish_dev(d_out.ptr, FULL_L)
    assert np.array_equal(d_out.to_numpy(), want)


# ---- 6. the recipient's chain on the device -----------------------------------------------------------------------------------------
def test_recipient_chain_sealed_seeds_to_unmasked_total(gpu):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    P, dim, q = 24, 1000, P62
    scheme = crypto.ChaCha(q, dim, 128)
    secrets = np.random.default_rng(24).integers(0, q, size=(P, dim), dtype=np.int64)
    d_sec = DeviceBuffer.from_numpy(secrets)
    d_seeds, d_masked = DeviceBuffer(P * 4).zero(), DeviceBuffer(P * dim).zero()
    crypto.SecretMasker(scheme).mask_batch_dev(d_sec.ptr, P, dim, dim, d_seeds.ptr, 4, d_masked.ptr, dim)      # participate.rs:52-54
    masked = d_masked.to_numpy().reshape(P, dim)                              # the sharing step is not under test: summed on the host
    total = np.array([sum(int(x) for x in masked[:, i]) % q for i in range(dim)], dtype=np.int64)
    d_total = DeviceBuffer.from_numpy(total)
    # every participant seals its seed for the recipient (participate.rs:57-60); seeds and masks stay in HBM from here on
    pk, sk = _keys(24)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    slot = max(codec.slot_size(4), 16) + 48
    d_boxes, d_lens = DeviceBytes(P * slot).zero(), DeviceBytes(P * 8).zero()
    box.seal_share_rows_dev(codec, [pk], P, d_seeds.ptr, P, 4, 4, d_boxes.ptr, slot, d_lens.ptr)
    comb = crypto.MaskCombiner(scheme)
    d_status, d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * P).zero()
    d_mask, d_out = DeviceBuffer(dim), DeviceBuffer(dim)
    comb.begin_dev(dim)
    comb.update_sealed_rows_dev(codec, box, pk, sk, d_boxes.ptr, slot, d_lens.ptr, P, slot, d_status.ptr, d_ok.ptr)
    comb.finish_dev(d_mask.ptr, dim)
    crypto.SecretUnmasker(scheme).unmask_dev(d_mask.ptr, d_total.ptr, dim, d_out.ptr)                         # receive.rs:149-152
    assert int(u32(d_status)[0]) == 0 and u32(d_ok, P).all()
    truth = np.array([sum(int(x) for x in secrets[:, i]) % q for i in range(dim)], dtype=np.int64)
    assert np.array_equal(d_out.to_numpy(), truth)

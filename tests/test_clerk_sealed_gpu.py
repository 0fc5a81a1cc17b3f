"""sda_share_combiner_update_sealed_rows_dev: a clerking job summed straight from its sealed boxes (clerk.rs:78-86) - tags
verified by the sealed-box kernels, then ONE pass that decrypts, varint-decodes and sums, with no plaintext buffer.

Every case runs the new call and the two-call sequence it replaces (sda_sealedbox_open_rows_dev, then
sda_share_combiner_update_varint_rows_dev on its output) on the same boxes and asks for
  * identical sums after finish_dev,
  * identical bit 16 of the status word, and zero / non-zero status alike,
  * the whole status word identical when every box authenticates,
and, where the inputs are canonical residues, for the oracle's combine of the plaintext shares."""
import random

import numpy as np
import pytest

from conftest import set_knob, use_test_hooks

pytestmark = pytest.mark.gpu
P62 = 4611686006577364993
SMALL_ORDER = bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800")


def _keys(seed):
    from oracle import sealedbox_oracle as so
    sk = bytes(np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8))
    return so.x25519_base(sk), sk


class Job:
    """boxes resident in HBM in the slotted layout: box r at d_boxes + r * slot, lens[r] bytes"""

    def __init__(self, d_boxes, slot, d_lens, rows, keep=()):
        self.d_boxes, self.slot, self.d_lens, self.rows, self.keep = d_boxes, slot, d_lens, rows, keep

    @property
    def box_bytes(self):
        return self.rows * self.slot


def seal_matrix(shares, pk):
    """participate.rs:82-101 on the device: varint-encode every row of `shares`, seal each payload (OS-entropy ephemeral keys)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    P, L = shares.shape
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_sh = DeviceBuffer.from_numpy(shares)
    vslot = max(codec.slot_size(L), 16)
    d_wire, d_wlen = DeviceBytes(P * vslot), DeviceBytes(P * 8).zero()
    codec.encode_rows_dev(d_sh.ptr, P, L, L, d_wire.ptr, vslot, d_wlen.ptr)
    bslot = vslot + 48
    d_boxes, d_blen = DeviceBytes(P * bslot), DeviceBytes(P * 8).zero()
    box.seal_rows_dev([pk], P, d_wire.ptr, vslot, d_wlen.ptr, P, vslot, d_boxes.ptr, bslot, d_blen.ptr)
    from sda_amd.device import synchronize
    synchronize()
    return Job(d_boxes, bslot, d_blen, P)


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


def u32(buf, n=1):
    return np.frombuffer(buf.to_bytes(), dtype="<u4")[:n].copy()


def run_fused(job, L, pk, sk, max_box=None, calls=1, want_ok=True):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    max_box = job.slot if max_box is None else max_box
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    comb = crypto.ShareCombiner(crypto.Additive(3, P62))
    d_status, d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * job.rows).zero()
    comb.begin_dev(1, L)
    per = (job.rows + calls - 1) // calls
    for r0 in range(0, job.rows, per):
        n = min(per, job.rows - r0)
        comb.update_sealed_rows_dev(codec, box, pk, sk, job.d_boxes.ptr + r0 * job.slot, job.slot, job.d_lens.ptr + 8 * r0, n, max_box,
                                    d_status.ptr, d_ok.ptr + 4 * r0 if want_ok else 0)
    sums = DeviceBuffer(max(L, 1))
    comb.finish_dev(sums.ptr)
    return sums.to_numpy()[:L], int(u32(d_status)[0]), u32(d_ok, job.rows)


def run_two_call(job, L, pk, sk, max_box=None):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    max_box = job.slot if max_box is None else max_box
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    comb = crypto.ShareCombiner(crypto.Additive(3, P62))
    d_status, d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * job.rows).zero()
    pslot = job.slot
    d_plain, d_plen = DeviceBytes(job.rows * pslot).zero(), DeviceBytes(job.rows * 8).zero()
    box.open_rows_dev(pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, job.rows, max_box, d_plain.ptr, pslot, d_plen.ptr, d_status.ptr,
                      d_ok.ptr)
    comb.begin_dev(1, L)
    comb.update_encoded_rows_dev(codec, d_plain.ptr, pslot, d_plen.ptr, job.rows, d_status.ptr)
    sums = DeviceBuffer(max(L, 1))
    comb.finish_dev(sums.ptr)
    return sums.to_numpy()[:L], int(u32(d_status)[0]), u32(d_ok, job.rows)


def check_agreement(job, L, pk, sk, max_box=None, calls=1):
    """the rules of the module docstring; returns (sums, status, ok) of the new call"""
    got, st, ok = run_fused(job, L, pk, sk, max_box, calls)
    ref, st2, ok2 = run_two_call(job, L, pk, sk, max_box)
    print(f"rows {job.rows} L {L}: status fused {st} two-call {st2}, rows ok {int(ok.sum())}/{job.rows}")
    assert np.array_equal(ok, ok2), "d_ok differs from open_rows_dev's"
    assert (st & 16) == (st2 & 16)
    assert (st != 0) == (st2 != 0)
    if ok2.all():
        assert st == st2
    assert np.array_equal(got, ref), "sums differ from open_rows_dev + update_varint_rows_dev"
    return got, st, ok


# ---- 1. shapes over the 62-bit prime ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,L,calls", [(1, 1, 1), (17, 333, 1), (64, 5000, 1), (2048, 2000, 2)])
def test_shapes_over_the_62_bit_prime(gpu, P, L, calls):
    from oracle import coracle
    pk, sk = _keys(P * 131 + L)
    shares = np.random.default_rng(P + L).integers(0, P62, size=(P, L), dtype=np.int64)
    job = seal_matrix(shares, pk)
    got, st, ok = check_agreement(job, L, pk, sk, calls=calls)
    assert st == 0 and ok.all()
    assert np.array_equal(got, coracle.combine(P62, shares))


def test_negative_values_zigzag(gpu):
    pk, sk = _keys(5)
    rng = np.random.default_rng(55)
    shares = rng.integers(-(1 << 62), 1 << 62, size=(40, 1500), dtype=np.int64)
    shares[:, ::7] = rng.integers(-300, 300, size=shares[:, ::7].shape)
    shares[0, :4] = [-(1 << 63), (1 << 63) - 1, -1, 0]
    got, st, ok = check_agreement(seal_matrix(shares, pk), 1500, pk, sk)
    assert st == 0 and ok.all()


# ---- 2. block and chunk edges ----------------------------------------------------------------------------------------------
def test_payload_lengths_across_the_chunk_group_and_block_boundaries(gpu):
    """L = 4000, row p holds exactly p two-byte values: payloads of 4000 .. 4200 bytes, across the 4064 / 4096 boundary of a
    group of four 1 KiB chunks and across many 64-byte Salsa20 blocks"""
    from oracle import coracle
    pk, sk = _keys(6)
    rng = np.random.default_rng(66)
    P, L = 201, 4000
    shares = rng.integers(0, 64, size=(P, L), dtype=np.int64)                # one byte each
    for p in range(P):
        where = rng.choice(L, size=p, replace=False)
        shares[p, where] = rng.integers(64, 8192, size=p)                    # two bytes each
    job = seal_matrix(shares, pk)
    lens = np.frombuffer(job.d_lens.to_bytes(), dtype="<u8")
    assert list(lens) == [4000 + p + 48 for p in range(P)]
    got, st, ok = check_agreement(job, L, pk, sk)
    assert st == 0 and ok.all() and np.array_equal(got, coracle.combine(P62, shares))


@pytest.mark.parametrize("L", range(1, 71))
def test_payloads_shorter_than_a_block(gpu, L):
    from oracle import coracle
    pk, sk = _keys(7)
    shares = np.random.default_rng(L).integers(0, 64, size=(9, L), dtype=np.int64)
    got, st, ok = check_agreement(seal_matrix(shares, pk), L, pk, sk)
    assert st == 0 and ok.all() and np.array_equal(got, coracle.combine(P62, shares))


# ---- 3. rows drifting apart -------------------------------------------------------------------------------------------------
def test_rows_drifting_past_the_column_window(gpu):
    """half the rows all one-byte values, half all nine-byte values: per group of chunks the short rows advance nine times
    as many columns, past the 2048-column LDS window, so the direct-to-global branch of the sink runs"""
    from oracle import coracle
    pk, sk = _keys(8)
    rng = np.random.default_rng(88)
    P, L = 32, 6000
    shares = np.empty((P, L), dtype=np.int64)
    shares[0::2] = rng.integers(0, 64, size=(P // 2, L))
    shares[1::2] = rng.integers(1 << 60, P62, size=(P // 2, L))
    got, st, ok = check_agreement(seal_matrix(shares, pk), L, pk, sk)
    assert st == 0 and ok.all() and np.array_equal(got, coracle.combine(P62, shares))


@pytest.mark.parametrize("waves", [8, 16])
def test_both_instances_of_the_kernel(gpu, waves):
    """the library launches the 8-row instance; the 16-row one is reachable through the knob only.  Both pinned here so that both instances meet ragged
    rows, rows of very different value sizes, a group that is not full (37 rows) and a bad box"""
    from oracle import coracle
    set_knob("SDA_SEALED_WAVES", waves)
    pk, sk = _keys(20 + waves)
    rng = np.random.default_rng(waves)
    P, L = 37, 5000
    shares = rng.integers(0, P62, size=(P, L), dtype=np.int64)
    shares[0::3] = rng.integers(0, 64, size=shares[0::3].shape)
    shares[1::3, ::2] = rng.integers(64, 8192, size=shares[1::3, ::2].shape)
    job = seal_matrix(shares, pk)
    got, st, ok = check_agreement(job, L, pk, sk)
    assert st == 0 and ok.all() and np.array_equal(got, coracle.combine(P62, shares))
    assert gpu.sda_debug_last_kernel().decode() != ""
    run_fused(job, L, pk, sk)
    from sda_amd import capi
    assert capi.load().sda_debug_last_kernel().decode() == f"sbox_poly_kernel + sealed_stream_combine_kernel<{waves}>"
    # one flipped ciphertext bit in row 5
    raw = bytearray(job.d_boxes.to_bytes())
    raw[5 * job.slot + 48 + 4097] ^= 0x20
    from sda_amd.device import DeviceBytes
    bad = Job(DeviceBytes.from_bytes(raw), job.slot, job.d_lens, P)
    got, st, ok = check_agreement(bad, L, pk, sk)
    assert st & 16 and list(np.flatnonzero(ok == 0)) == [5]
    assert np.array_equal(got, coracle.combine(P62, np.delete(shares, 5, axis=0)))


# ---- 4. bad boxes -----------------------------------------------------------------------------------------------------------
def test_bad_boxes_add_nothing_and_flag_the_job(gpu):
    from oracle import coracle, sealedbox_oracle as so
    pk, sk = _keys(9)
    rng = random.Random(99)
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    P, L = 24, 300
    shares = np.random.default_rng(9).integers(0, P62, size=(P, L), dtype=np.int64)
    payloads = [coracle.varint_encode(shares[p]) for p in range(P)]
    boxes = [bytearray(so.seal(m, pk, rb(32))) for m in payloads]
    lens = [len(b) for b in boxes]
    bad = {3: "ciphertext bit", 5: "tag bit", 8: "epk bit", 11: "47 bytes", 14: "longer than max_box_bytes", 17: "small-order key"}
    boxes[3][48 + 1000] ^= 0x10
    boxes[5][32 + 7] ^= 0x01
    boxes[8][13] ^= 0x40
    lens[11] = 47
    lens[14] = max(lens) + 16                              # the header lies: longer than the bound the caller declares
    # a box anybody can make: ephemeral key of small order -> all-zero shared secret; its tag VERIFIES under that key
    forged = SMALL_ORDER + so.secretbox(payloads[17], so.seal_nonce(SMALL_ORDER, pk), so.hsalsa20(bytes(32), bytes(16)))
    assert so.x25519(sk, SMALL_ORDER) == bytes(32) and len(forged) == len(boxes[17])
    boxes[17] = bytearray(forged)
    max_box = max(len(b) for b in boxes)
    job = upload_boxes([bytes(b) for b in boxes], lens)
    got, st, ok = check_agreement(job, L, pk, sk, max_box=max_box)
    assert [bool(x) for x in ok] == [p not in bad for p in range(P)]
    assert st & 16
    survivors = np.stack([shares[p] for p in range(P) if p not in bad])
    assert np.array_equal(got, coracle.combine(P62, survivors))
    # without the optional d_ok array: same sums, same verdict for the job
    got2, st2, _ = run_fused(job, L, pk, sk, max_box, want_ok=False)
    assert np.array_equal(got2, got) and st2 == st


# ---- 5. wrong dimension -----------------------------------------------------------------------------------------------------
def test_wrong_dimension_sets_the_count_bit(gpu):
    from oracle import coracle, sealedbox_oracle as so
    pk, sk = _keys(10)
    rng = random.Random(10)
    L = 200
    shares = np.random.default_rng(10).integers(0, P62, size=(6, L + 1), dtype=np.int64)
    counts = [L, L - 1, L, L + 1, L, L]
    boxes = [so.seal(coracle.varint_encode(shares[p][:n]), pk, bytes(rng.getrandbits(8) for _ in range(32))) for p, n in enumerate(counts)]
    got, st, ok = check_agreement(upload_boxes(boxes), L, pk, sk)
    assert ok.all() and st & 2 and not st & 16
    # an authentic payload that ends inside a value: the "unterminated" bit, as in the two-call sequence
    cut = coracle.varint_encode(shares[0][:L])[:-1] + b"\x80"
    boxes = [so.seal(cut, pk, bytes(32 - 1) + b"\x07"), boxes[0]]
    got, st, ok = check_agreement(upload_boxes(boxes), L, pk, sk)
    assert ok.all() and st & 4 and not st & 16


def test_dimension_zero_behaves_as_the_two_call_sequence(gpu):
    from oracle import sealedbox_oracle as so
    pk, sk = _keys(11)
    for payloads in ([b"", b""], [b"", b"\x05"]):
        boxes = [so.seal(m, pk, bytes([i + 1]) * 32) for i, m in enumerate(payloads)]
        got, st, ok = check_agreement(upload_boxes(boxes), 0, pk, sk)
        assert ok.all() and (st != 0) == any(payloads)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBytes
    pk, sk = _keys(12)
    shares = np.random.default_rng(12).integers(0, P62, size=(4, 10), dtype=np.int64)
    job = seal_matrix(shares, pk)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_status = DeviceBytes(4).zero()

    def call(comb, d_boxes=job.d_boxes.ptr, slot=job.slot, max_box=job.slot, rows=4):
        comb.update_sealed_rows_dev(codec, box, pk, sk, d_boxes, slot, job.d_lens.ptr, rows, max_box, d_status.ptr)

    def refused(code, comb, **kw):
        with pytest.raises(capi.SdaError) as e:
            call(comb, **kw)
        assert e.value.code == code, e.value
        return str(e.value)

    comb = crypto.ShareCombiner(crypto.Additive(3, P62))
    refused(capi.ERR_STATE, comb)                                            # update before begin
    comb.begin_dev(2, 10)
    refused(capi.ERR_STATE, comb)                                            # one job per call
    comb.begin_dev(1, 10)
    refused(capi.ERR_INVALID_ARGUMENT, comb, slot=job.slot + 8)              # misaligned slot
    refused(capi.ERR_INVALID_ARGUMENT, comb, d_boxes=job.d_boxes.ptr + 8)    # misaligned buffer
    refused(capi.ERR_INVALID_ARGUMENT, comb, max_box=job.slot + 16)          # max_box_bytes > slot_bytes
    refused(capi.ERR_INVALID_ARGUMENT, comb, d_boxes=0)                      # NULL device pointer
    call(comb, rows=0)                                                       # nothing to do: fine, nothing launched
    signed = crypto.ShareCombiner(crypto.Additive(3, P62))
    signed.set_value_mode(crypto.RUST_SIGNED)
    signed.begin_dev(1, 10)
    assert "SDA_VALUES_RUST_SIGNED" in refused(capi.ERR_UNSUPPORTED, signed)
    assert u32(d_status)[0] == 0
    # ... and after all the refusals the handle still works
    call(comb)
    from sda_amd.device import DeviceBuffer
    from oracle import coracle
    sums = DeviceBuffer(10)
    comb.finish_dev(sums.ptr)
    assert np.array_equal(sums.to_numpy(), coracle.combine(P62, shares)) and u32(d_status)[0] == 0


# ---- 7. footprint -----------------------------------------------------------------------------------------------------------
def test_footprint_no_second_copy_of_the_job(gpu):
    """P = 256 boxes of L = 100,000 shares (about 230 MB): the new call holds at most 5 % of the box bytes in new device memory
    (per-row key state and Poly1305 partials: about 2.5 KB against 900 KB of box, plus allocator granules), a second call of
    the same size takes nothing more, and the two-call sequence needs at least the box bytes for its plaintext."""
    import ctypes as C
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    from oracle import coracle
    lib = use_test_hooks()                                       # sda_debug_mem_info lives in the library with the test hooks
    pk, sk = _keys(13)
    P, L = 256, 100_000
    shares = np.random.default_rng(13).integers(0, P62, size=(P, L), dtype=np.int64)
    job = seal_matrix(shares, pk)
    lens = np.frombuffer(job.d_lens.to_bytes(), dtype="<u8")
    box_bytes = int(lens.sum())
    assert box_bytes > 220e6

    def free_now():
        synchronize()
        f, t = C.c_size_t(), C.c_size_t()
        capi.check(lib.sda_debug_mem_info(C.byref(f), C.byref(t)))
        return f.value

    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    comb = crypto.ShareCombiner(crypto.Additive(3, P62))
    d_status, sums = DeviceBytes(4).zero(), DeviceBuffer(L)
    comb.begin_dev(1, L)                                         # the accumulators are the combiner's, not this call's
    before = free_now()
    comb.update_sealed_rows_dev(codec, box, pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, P, job.slot, d_status.ptr)
    first = before - free_now()
    comb.finish_dev(sums.ptr)
    assert u32(d_status)[0] == 0 and np.array_equal(sums.to_numpy(), coracle.combine(P62, shares))
    comb.begin_dev(1, L)
    mid = free_now()
    comb.update_sealed_rows_dev(codec, box, pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, P, job.slot, d_status.ptr)
    second = mid - free_now()
    print(f"box bytes {box_bytes}, newly held after the first call {first} ({100.0 * first / box_bytes:.3f} %), after the second {second}")
    assert first <= 0.05 * box_bytes
    assert second == 0
    # the two-call sequence: its plaintext buffer alone (payload of every box) is the job again
    before2 = free_now()
    d_plain, d_plen = DeviceBytes(P * job.slot), DeviceBytes(P * 8).zero()
    box.open_rows_dev(pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, P, job.slot, d_plain.ptr, job.slot, d_plen.ptr, d_status.ptr)
    two = before2 - free_now()
    print(f"two-call sequence: {two} bytes newly held, payload bytes {box_bytes - 48 * P}")
    assert two >= box_bytes


# ---- 8. the host helper -----------------------------------------------------------------------------------------------------
def test_combine_sealed_job_helper(gpu):
    from sda_amd import capi, crypto
    from oracle import coracle, sealedbox_oracle as so
    pk, sk = _keys(14)
    P, L = 12, 777
    shares = np.random.default_rng(14).integers(0, P62, size=(P, L), dtype=np.int64)
    boxes = [so.seal(coracle.varint_encode(shares[p]), pk, bytes([p + 1]) * 32) for p in range(P)]
    comb = crypto.ShareCombiner(crypto.Additive(3, P62))
    blob = bytes(crypto.JobContainer.build(capi.JOB_SEALED, boxes))
    assert np.array_equal(comb.combine_sealed_job(blob, pk, sk, L), coracle.combine(P62, shares))
    tampered = list(boxes)
    tampered[4] = tampered[4][:100] + bytes([tampered[4][100] ^ 2]) + tampered[4][101:]
    with pytest.raises(capi.SdaError) as e:
        comb.combine_sealed_job(bytes(crypto.JobContainer.build(capi.JOB_SEALED, tampered)), pk, sk, L)
    assert e.value.code == capi.ERR_SODIUM_DECRYPTION and "Sodium decryption failure" in str(e.value)
    with pytest.raises(capi.SdaError) as e:
        comb.combine_sealed_job(blob, pk, sk, L + 1)
    assert e.value.code == capi.ERR_WRONG_DIMENSION and "Wrong dimension" in str(e.value)
    # ... and the combiner is fit for the next job
    assert np.array_equal(comb.combine_sealed_job(blob, pk, sk, L), coracle.combine(P62, shares))


def test_the_call_reports_both_kernels(gpu):
    pk, sk = _keys(15)
    shares = np.random.default_rng(15).integers(0, P62, size=(8, 50), dtype=np.int64)
    run_fused(seal_matrix(shares, pk), 50, pk, sk)
    assert gpu.sda_debug_last_kernel().decode().startswith("sbox_poly_kernel + sealed_stream_combine_kernel<")

"""The reconstructor's streaming device job on the GPU: sda_secret_reconstructor_begin_dev / update_dev / update_sealed_rows_dev /
finish_dev (receive.rs:120-146 with the clerking results in HBM).  Every case of tests/reconstruct_stream_cases.py is bit-exact
against the C oracle, equal to sda_secret_reconstructor_reconstruct_dev on the decoded rows, and leaves the sentinel behind d_out
alone.  tests/test_reconstruct_stream_cpu.py proves on the CPU which cases reach the kernel's global fallback."""
import numpy as np
import pytest

import reconstruct_stream_cases as rc
from conftest import load_golden

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A
SMALL_ORDER = [bytes(32), (1).to_bytes(32, "little"),
               bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800")]    # tests/test_sealedbox_gpu.py


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
    """every row of `values` varint-encoded and sealed on the device in one call (OS-entropy ephemeral keys)"""
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


def scheme_of(case):
    from sda_amd import crypto
    p, k, t, n, w2, w3 = rc.SCHEMES[case.scheme]
    return crypto.Additive(n, p) if case.scheme == "additive" else crypto.PackedShamir(k, n, t, p, w2, w3)


def out_len(case, row_len):
    return row_len if case.scheme == "additive" else case.dim


def run_job(case, rows, job, pk, sk, feed=None, rec=None):
    """begin_dev, the updates of the case's feeding, finish_dev -> (result, status, d_ok); the sentinel behind d_out is checked"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    pos, row_len = rows.shape
    n_out = out_len(case, row_len)
    rec = rec or crypto.SecretReconstructor(scheme_of(case), case.dim)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_rows = DeviceBuffer.from_numpy(rows)
    d_out = DeviceBuffer.from_numpy(np.full(n_out + 8, SENTINEL, dtype=np.int64))
    d_status, d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * pos).zero()

    def sealed(first, n):
        rec.update_sealed_rows_dev(codec, box, pk, sk, first, job.d_boxes.ptr + first * job.slot, job.slot, job.d_lens.ptr + 8 * first, n,
                                   job.slot, d_status.ptr, d_ok.ptr + 4 * first)
    rec.begin_dev(None if case.scheme == "additive" else case.indices, pos, row_len)
    feed = feed or case.feed
    if feed == "one":
        sealed(0, pos)
    elif feed == "descending":
        for i in reversed(range(pos)):
            sealed(i, 1)
    else:                                         # mixed: the first half as decoded rows, the rest sealed, the sealed part first
        h = pos // 2
        sealed(h, pos - h)
        rec.update_dev(0, d_rows.ptr, h, row_len)
    rec.finish_dev(d_out.ptr, n_out)
    got = d_out.to_numpy()
    assert (got[n_out:] == SENTINEL).all(), "finish_dev wrote past its output"
    return got[:n_out], int(u32(d_status)[0]), u32(d_ok, pos)


def chain(job, pk, sk, row_len):
    """open_rows_dev + decode_rows_dev on the same boxes -> (decoded rows, status, d_ok)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_status, d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * job.rows).zero()
    d_plain, d_plen = DeviceBytes(job.rows * job.slot).zero(), DeviceBytes(job.rows * 8).zero()
    box.open_rows_dev(pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, job.rows, job.slot, d_plain.ptr, job.slot, d_plen.ptr, d_status.ptr,
                      d_ok.ptr)
    d_vals = DeviceBuffer(job.rows * max(row_len, 1)).zero()
    codec.decode_rows_dev(d_plain.ptr, job.slot, d_plen.ptr, job.rows, row_len, d_vals.ptr, row_len, d_status.ptr)
    return d_vals.to_numpy().reshape(job.rows, max(row_len, 1)), int(u32(d_status)[0]), u32(d_ok, job.rows)


def oracle_of(case, rows):
    from oracle import coracle
    p, k, t, n, w2, w3 = rc.SCHEMES[case.scheme]
    canon = (rows[:, :rc.batches(case)].astype(object) % p).astype(np.int64)
    if case.scheme == "additive":
        return coracle.combine(p, canon)
    return coracle.packed_reconstruct(p, k, t, w2, w3, case.dim, list(case.indices), canon)


def reconstruct_dev_of(case, rows):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    pos, row_len = rows.shape
    n_out = out_len(case, row_len)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    d_rows, d_out = DeviceBuffer.from_numpy(rows), DeviceBuffer(n_out + 1)
    n = rec.reconstruct_dev(list(case.indices), d_rows.ptr, row_len, row_len, d_out.ptr, n_out)
    assert n == n_out
    return d_out.to_numpy()[:n_out]


# ---- 1. every case: oracle, reconstruct_dev, sentinel ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_case_equals_the_oracle_and_reconstruct_dev(gpu, name):
    case, b = rc.BY_NAME[name], rc.build(name)
    pk, sk = _keys(7)
    job = seal_rows(b.rows, pk)
    got, status, ok = run_job(case, b.rows, job, pk, sk)
    want = oracle_of(case, b.rows)
    ref = reconstruct_dev_of(case, b.rows)
    print(f"{name}: rows {b.rows.shape}, status {status}, mismatches vs oracle {int((got != want).sum())}, vs reconstruct_dev {int((got != ref).sum())}")
    assert status == 0
    if case.feed == "mixed":
        h = len(case.indices) // 2
        assert not ok[:h].any() and ok[h:].all()                    # d_ok belongs to the sealed positions
    else:
        assert ok.all()
    assert np.array_equal(want, b.want)
    assert np.array_equal(got, want), "differs from the C oracle"
    assert np.array_equal(got, ref), "differs from reconstruct_dev on the decoded rows"


def test_convenience_wrapper_on_a_job_blob(gpu):
    from sda_amd import capi, crypto
    case, b = rc.BY_NAME["k3_62-scattered-d1000"], rc.build("k3_62-scattered-d1000")
    pk, sk = _keys(8)
    enc = crypto.ShareEncryptor(pk)
    job = crypto.JobContainer.build(0, [enc.encrypt(row) for row in b.rows])
    blob = bytes(job)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    assert np.array_equal(rec.reconstruct_sealed_job(blob, case.indices, pk, sk), b.want)
    bad = bytearray(blob)
    bad[job.layout.payload_offset + 2 * job.layout.slot_bytes + 40] ^= 1        # a tag byte of the third box
    with pytest.raises(crypto.SdaError) as e:
        rec.reconstruct_sealed_job(bytes(bad), case.indices, pk, sk)
    assert e.value.code == capi.ERR_SODIUM_DECRYPTION


# ---- 2. failures -------------------------------------------------------------------------------------------------------------
FAIL = "k3_62-all-d1000"


def _host_boxes(rows, pk, seed):
    from oracle import coracle, sealedbox_oracle as so
    esk = np.random.default_rng(seed).integers(0, 256, size=(len(rows), 32), dtype=np.uint8)
    payloads = [coracle.varint_encode(r) for r in rows]
    return payloads, [so.seal(m, pk, e.tobytes()) for m, e in zip(payloads, esk)]


def _check_failure(boxes, lens, pk, sk, bad_rows):
    """the job over tampered boxes: bit 16 and no other, d_ok per row as open_rows_dev sets it, the sentinel (run_job)"""
    case, b = rc.BY_NAME[FAIL], rc.build(FAIL)
    job = upload_boxes(boxes, lens)
    got, status, ok = run_job(case, b.rows, job, pk, sk, feed="one")
    _, st2, ok2 = chain(job, pk, sk, b.row_len)
    print(f"bad rows {bad_rows}: status {status}, chain {st2}, ok {ok.tolist()}")
    # a refused row is not decoded at all: bit 16 alone, where the chain also decodes the empty row open_rows_dev leaves (bit 4)
    assert status == 16 and st2 & 16
    assert np.array_equal(ok, ok2)
    assert [int(i) for i in np.flatnonzero(ok == 0)] == list(bad_rows)
    # a row that failed adds nothing: the others alone, through the weighted plaintext kernel
    p, k = rc.SCHEMES[case.scheme][:2]
    keep = [i for i in range(len(boxes)) if i not in bad_rows]
    R = rc.lagrange_matrix(p, k, *rc.SCHEMES[case.scheme][4:6], case.indices)
    want = [sum(R[e][i] * int(b.rows[i][bb]) for i in keep) % p for bb in range(b.batches) for e in range(k)][:case.dim]
    assert np.array_equal(got, np.array(want, dtype=np.int64))


def test_flipped_tag_byte(gpu):
    pk, sk = _keys(9)
    _, boxes = _host_boxes(rc.build(FAIL).rows, pk, 9)
    boxes[2] = boxes[2][:37] + bytes([boxes[2][37] ^ 0x40]) + boxes[2][38:]
    _check_failure(boxes, None, pk, sk, [2])


def test_box_of_47_bytes(gpu):
    pk, sk = _keys(10)
    _, boxes = _host_boxes(rc.build(FAIL).rows, pk, 10)
    lens = [len(x) for x in boxes]
    lens[5] = 47
    _check_failure(boxes, lens, pk, sk, [5])


@pytest.mark.parametrize("which", range(3))
def test_small_order_ephemeral_key(gpu, which):
    """a box anybody can make: ephemeral key of small order -> all-zero shared secret; its tag VERIFIES under that key"""
    from oracle import sealedbox_oracle as so
    pk, sk = _keys(11)
    payloads, boxes = _host_boxes(rc.build(FAIL).rows, pk, 11)
    epk = SMALL_ORDER[which]
    assert so.x25519(sk, epk) == bytes(32)
    boxes[1] = epk + so.secretbox(payloads[1], so.seal_nonce(epk, pk), so.hsalsa20(bytes(32), bytes(16)))
    _check_failure(boxes, None, pk, sk, [1])


@pytest.mark.parametrize("what,bit", [("eleven-byte value", 1), ("one value too few", 2), ("unterminated end", 4)])
def test_malformed_payload_gives_the_chain_status(gpu, what, bit):
    from oracle import coracle, sealedbox_oracle as so
    case, b = rc.BY_NAME[FAIL], rc.build(FAIL)
    pk, sk = _keys(12)
    payloads, boxes = _host_boxes(b.rows, pk, 12)
    row = b.rows[4]
    if what == "eleven-byte value":
        raw = coracle.varint_encode(row[:100]) + bytes([0x80] * 10 + [0x01]) + coracle.varint_encode(row[101:])
    elif what == "one value too few":
        raw = coracle.varint_encode(row[:-1])
    else:
        raw = coracle.varint_encode(row)[:-1] + b"\x80"
    boxes[4] = so.seal(raw, pk, bytes(range(32)))
    job = upload_boxes(boxes)
    _, status, ok = run_job(case, b.rows, job, pk, sk, feed="one")
    _, st2, ok2 = chain(job, pk, sk, b.row_len)
    print(f"{what}: status {status}, chain {st2}")
    assert status == st2 and status & bit and not status & 16
    assert ok.all() and ok2.all()


# ---- 3. state machine --------------------------------------------------------------------------------------------------------
def _raises(code, call):
    from sda_amd import crypto
    with pytest.raises(crypto.SdaError) as e:
        call()
    assert e.value.code == code, e.value


def test_state_machine(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    name = "k3_62-scattered-d1000"
    case, b = rc.BY_NAME[name], rc.build(name)
    pk, sk = _keys(13)
    job = seal_rows(b.rows, pk)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_rows, d_out, d_status = DeviceBuffer.from_numpy(b.rows), DeviceBuffer(case.dim + 1), DeviceBytes(4).zero()
    L = b.row_len

    def sealed(first, n, d_boxes=job.d_boxes.ptr, slot=job.slot, max_box=job.slot, d_lens=job.d_lens.ptr, status=d_status.ptr):
        rec.update_sealed_rows_dev(codec, box, pk, sk, first, d_boxes and d_boxes + first * job.slot, slot, d_lens and d_lens + 8 * first, n,
                                   max_box, status)
    # update and finish before begin
    _raises(capi.ERR_STATE, lambda: rec.update_dev(0, d_rows.ptr, 1, L))
    _raises(capi.ERR_STATE, lambda: sealed(0, 1))
    _raises(capi.ERR_STATE, lambda: rec.finish_dev(d_out.ptr, case.dim))
    # begin: too few rows, duplicate indices, a row too short
    _raises(capi.ERR_NOT_ENOUGH_SHARES, lambda: rec.begin_dev(case.indices[:3], 3, L))
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_dev((7, 0, 3, 7), 4, L))
    _raises(capi.ERR_ASSERTION, lambda: rec.begin_dev(case.indices, 4, L - 1))
    _raises(capi.ERR_STATE, lambda: rec.update_dev(0, d_rows.ptr, 1, L))                   # a refused begin starts no job
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_dev(case.indices[:3], 4, L))     # the mirror counts the indices
    rec.begin_dev(case.indices, 4, L)                                                     # ... and leaves a job in flight alone
    rec.update_dev(0, d_rows.ptr, 2, L)
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_dev((7, 0, 3, 7), 4, L))
    _raises(capi.ERR_ASSERTION, lambda: rec.begin_dev(case.indices, 4, L - 1))
    rec.update_dev(2, d_rows.at(2 * L), 2, L)
    rec.finish_dev(d_out.ptr, case.dim)
    assert np.array_equal(d_out.to_numpy()[:case.dim], b.want)
    for _ in range(2):                                                                    # a second job on the same handle
        rec.begin_dev(case.indices, 4, L)
        rec.update_dev(1, d_rows.at(L), 0, L)                                             # rows == 0 launches nothing
        sealed(2, 0)
        rec.update_dev(1, d_rows.at(L), 1, L)
        _raises(capi.ERR_STATE, lambda: rec.update_dev(1, d_rows.at(L), 1, L))            # a position fed twice, either form
        _raises(capi.ERR_STATE, lambda: sealed(0, 2))
        _raises(capi.ERR_STATE, lambda: rec.update_dev(4, d_rows.ptr, 1, L))              # a position >= n_rows
        _raises(capi.ERR_STATE, lambda: sealed(3, 2))
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.update_dev(0, 0, 1, L))
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.update_dev(0, d_rows.ptr, 1, L - 1))
        for kw in (dict(d_boxes=0), dict(d_lens=0), dict(status=0), dict(d_boxes=job.d_boxes.ptr + 8), dict(slot=job.slot + 8),
                   dict(max_box=job.slot + 16)):                                          # one bad argument each, position 0 stays free
            _raises(capi.ERR_INVALID_ARGUMENT, lambda: sealed(0, 1, **kw))
        sealed(2, 2)
        _raises(capi.ERR_STATE, lambda: rec.finish_dev(d_out.ptr, case.dim))              # position 0 is missing
        sealed(0, 1)
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_dev(d_out.ptr, case.dim - 1))
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_dev(0, case.dim))
        rec.finish_dev(d_out.ptr, case.dim)
        assert np.array_equal(d_out.to_numpy()[:case.dim], b.want)
        _raises(capi.ERR_STATE, lambda: rec.finish_dev(d_out.ptr, case.dim))              # finish ended the job
    assert int(u32(d_status)[0]) == 0
    # the host form on the same handle still works, and a job is not disturbed by it
    rec.begin_dev(case.indices, 4, L)
    sealed(0, 2)
    other = rc.build("k3_62-permuted-d1000")
    assert np.array_equal(rec.reconstruct([(i, r) for i, r in zip(rc.PERMUTED, other.rows)]), other.want)
    sealed(2, 2)
    rec.finish_dev(d_out.ptr, case.dim)
    assert np.array_equal(d_out.to_numpy()[:case.dim], b.want)


def test_rust_signed_takes_rows_only(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    case, b = rc.BY_NAME["additive-d1000"], rc.build("additive-d1000")
    pk, sk = _keys(14)
    job = seal_rows(b.rows, pk)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    rec.set_value_mode("rust_signed")
    rec.begin_dev(None, 3, b.row_len)
    _raises(capi.ERR_UNSUPPORTED, lambda: rec.update_sealed_rows_dev(crypto.VarintCodec(), crypto.SealedBox(), pk, sk, 0, job.d_boxes.ptr,
                                                                     job.slot, job.d_lens.ptr, 3, job.slot, DeviceBytes(4).zero().ptr))
    d_rows, d_out = DeviceBuffer.from_numpy(b.rows), DeviceBuffer(case.dim)
    rec.update_dev(0, d_rows.ptr, 3, b.row_len)
    rec.finish_dev(d_out.ptr, case.dim)
    assert np.array_equal(d_out.to_numpy(), rec.reconstruct([(i, r) for i, r in enumerate(b.rows)]))


# ---- 4. end to end through the device forms --------------------------------------------------------------------------------------
def test_full_loop_through_device_forms(gpu):
    """tests/golden/full_loop.json has no scenario with packed Shamir AND ChaCha masks: this takes F4_with_packedshamir (its
    aggregation, inputs and output) with the masking scheme of F3_with_chachamask.  Masks and share randomness are drawn on the
    device, so only the end of the loop - the sum of the inputs - is the fixture's."""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    scen = {s["name"]: s for s in load_golden("full_loop.json")["scenarios"]}
    sc, a = scen["F4_with_packedshamir"], scen["F4_with_packedshamir"]["aggregation"]
    s = a["committee_sharing_scheme"]
    m = scen["F3_with_chachamask"]["aggregation"]["masking_scheme"]
    dim, q = a["vector_dimension"], a["modulus"]
    assert m["modulus"] == q and m["dimension"] == dim
    sharing = crypto.PackedShamir(s["secret_count"], s["share_count"], s["privacy_threshold"], s["prime_modulus"], s["omega_secrets"],
                                  s["omega_shares"])
    masking = crypto.ChaCha(m["modulus"], m["dimension"], m["seed_bitsize"])
    inputs = np.array(sc["inputs"], dtype=np.int64)
    P, n, k = inputs.shape[0], s["share_count"], s["secret_count"]
    B, W = -(-dim // k), (m["seed_bitsize"] + 31) // 32
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    clerk_keys = [_keys(100 + c) for c in range(n)]
    rpk, rsk = _keys(99)
    # 1. participate.rs:52-54
    d_in, d_seeds, d_masked = DeviceBuffer.from_numpy(inputs), DeviceBuffer(P * W).zero(), DeviceBuffer(P * dim).zero()
    crypto.SecretMasker(masking).mask_batch_dev(d_in.ptr, P, dim, dim, d_seeds.ptr, W, d_masked.ptr, dim)
    # 2. participate.rs:75-76, clerk-major: the share of participant p for clerk c at (c * P + p) * B
    d_shares = DeviceBuffer(n * P * B).zero()
    crypto.ShareGenerator(sharing).generate_batch_dev(d_masked.ptr, P, dim, dim, d_shares.ptr, B, P * B)
    # 3. participate.rs:82-101: every share row sealed to its clerk
    slot = max(codec.slot_size(B), 16) + 48
    d_boxes, d_lens = DeviceBytes(n * P * slot).zero(), DeviceBytes(n * P * 8).zero()
    box.seal_share_rows_dev(codec, [pk for pk, _ in clerk_keys], P, d_shares.ptr, n * P, B, B, d_boxes.ptr, slot, d_lens.ptr)
    # 4. clerk.rs:78-86, one job per clerk
    d_sums, d_status = DeviceBuffer(n * B).zero(), DeviceBytes(4).zero()
    comb = crypto.ShareCombiner(sharing)
    for c, (cpk, csk) in enumerate(clerk_keys):
        comb.begin_dev(1, B)
        comb.update_sealed_rows_dev(codec, box, cpk, csk, d_boxes.ptr + c * P * slot, slot, d_lens.ptr + 8 * c * P, P, slot, d_status.ptr)
        comb.finish_dev(d_sums.at(c * B))
    # 5. clerk.rs:88-91: every clerk seals its result to the recipient
    d_rboxes, d_rlens = DeviceBytes(n * slot).zero(), DeviceBytes(n * 8).zero()
    box.seal_share_rows_dev(codec, [rpk], n, d_sums.ptr, n, B, B, d_rboxes.ptr, slot, d_rlens.ptr)
    # 6. receive.rs:120-146: the new sealed job, clerk results in arrival order 7 .. 0
    rec = crypto.SecretReconstructor(sharing, dim)
    d_total = DeviceBuffer(dim)
    rec.begin_dev(list(range(n)), n, B)
    for c in reversed(range(n)):
        rec.update_sealed_rows_dev(codec, box, rpk, rsk, c, d_rboxes.ptr + c * slot, slot, d_rlens.ptr + 8 * c, 1, slot, d_status.ptr)
    rec.finish_dev(d_total.ptr, dim)
    # 7. receive.rs:101-118: the mask combiner's sealed job
    mslot = max(codec.slot_size(W), 16) + 48
    d_mboxes, d_mlens = DeviceBytes(P * mslot).zero(), DeviceBytes(P * 8).zero()
    box.seal_share_rows_dev(codec, [rpk], P, d_seeds.ptr, P, W, W, d_mboxes.ptr, mslot, d_mlens.ptr)
    d_mask, d_out = DeviceBuffer(dim), DeviceBuffer(dim)
    mcomb = crypto.MaskCombiner(masking)
    mcomb.begin_dev(dim)
    mcomb.update_sealed_rows_dev(codec, box, rpk, rsk, d_mboxes.ptr, mslot, d_mlens.ptr, P, mslot, d_status.ptr)
    mcomb.finish_dev(d_mask.ptr, dim)
    # 8. receive.rs:149-152
    crypto.SecretUnmasker(masking).unmask_dev(d_mask.ptr, d_total.ptr, dim, d_out.ptr)
    assert int(u32(d_status)[0]) == 0
    assert list(map(int, d_out.to_numpy())) == sc["stages"]["canonical"]["output"]

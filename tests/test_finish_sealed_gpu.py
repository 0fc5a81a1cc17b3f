"""sda_share_combiner_finish_sealed_rows_dev: the clerk's last step (clerk.rs:84-100) in one call - the setup pass, a kernel that
folds the 128-bit clerk sums and counts each 2048-value block's bytes, the scan, ONE kernel that folds the sums again, encodes a
block and xors the XSalsa20 keystream of exactly its byte range into it in LDS, then the Poly1305 pass.  Every row is split over
the whole chip; no plaintext result and no wire buffer reach device memory.

The reference of every case (tests/finish_sealed_cases.py; what the table reaches is proved in
tests/test_finish_sealed_reach.py) is sum(rows) mod m in Python integers -> pyoracle.varint_encode -> sealedbox_oracle.seal with
injected ephemeral secrets; the "chain" is sda_share_combiner_finish_dev + sda_sealedbox_seal_share_rows_dev with the same
secrets.  The box buffer is prefilled with 0xA5, so a byte written past a row's length or into the slot padding shows
(check_against of tests/test_participant_seal_gpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import finish_sealed_cases as fc
from conftest import use_test_hooks
from test_participant_seal_gpu import PATTERN, _pattern_buffer, check_against

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in fc.CASES]
KERNELS = b"sum_len_kernel + sum_seal_wide_kernel + sbox_poly_kernel"


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def combiner_of(case):
    from sda_amd import crypto
    return crypto.ShareCombiner(crypto.Additive(3, case["m"]))        # a combiner uses the modulus of its scheme only


def feed(comb, rows, begin=True):
    """rows [jobs][n][dim] through update_dev; returns the device buffer (alive until the caller has synchronised)"""
    from sda_amd.device import DeviceBuffer
    jobs, n, dim = rows.shape
    d = DeviceBuffer.from_numpy(np.concatenate([rows.reshape(-1), np.zeros(2, dtype=np.int64)]))
    if begin:
        comb.begin_dev(jobs, dim)
    comb.update_dev(d.ptr, n * dim, n, dim)
    return d


def slot_of(dim, extra=0):
    from sda_amd import crypto
    return crypto.VarintCodec().slot_size(dim) + 48 + extra


def _lens(d_lens, rows):
    return np.frombuffer(d_lens.to_bytes(rows * 8), dtype="<u8").copy()


def seal_new(comb, jobs, dim, pk, esk, slot=None):
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    slot = slot_of(dim) if slot is None else slot
    d_boxes, d_lens = _pattern_buffer(jobs * slot), DeviceBytes(jobs * 8).zero()
    comb.finish_sealed_rows_dev(codec, box, pk, d_boxes.ptr, slot, d_lens.ptr, esk)
    return d_boxes.to_bytes(jobs * slot), _lens(d_lens, jobs), slot


def seal_chain(comb, jobs, dim, pk, esk, slot):
    """finish_dev into a result buffer, then seal_share_rows_dev over its `jobs` rows"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_out = DeviceBuffer(max(jobs * dim, 2)).zero()
    comb.finish_dev(d_out.ptr)
    d_boxes, d_lens = _pattern_buffer(jobs * slot), DeviceBytes(jobs * 8).zero()
    box.seal_share_rows_dev(codec, [pk], jobs, d_out.ptr, jobs, dim, dim, d_boxes.ptr, slot, d_lens.ptr, esk)
    return d_boxes.to_bytes(jobs * slot), _lens(d_lens, jobs), d_out.to_numpy()[:jobs * dim].reshape(jobs, dim)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """rows, residues and the reference's boxes of a case: computed once, shared by the tests, never modified"""
    case = fc.BY_NAME[name]
    rows = fc.rows_of(case)
    rows.setflags(write=False)
    return rows, fc.residues_of(case, rows), tuple(fc.oracle_boxes(case, rows=rows))


# ---- 1. byte-exact against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_boxes_equal_the_references(gpu, name):
    case = fc.BY_NAME[name]
    rows, _, want = case_data(name)
    pk, esk = fc.recipient_keys()[0], fc.esk_of(case)
    comb = combiner_of(case)
    d = feed(comb, rows)
    raw, lens, slot = seal_new(comb, case["jobs"], case["dim"], pk, esk, slot_of(case["dim"], extra=32))
    assert gpu.sda_debug_last_kernel() == KERNELS
    print(f"{name}: jobs {case['jobs']} dim {case['dim']} lengths {list(lens)} slot {slot}")
    assert all(int(l) == len(w) for l, w in zip(lens, want))
    check_against(raw, lens, slot, want, esk, name)
    del d


# ---- 2. byte-exact against finish_dev + seal_share_rows_dev -------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_boxes_equal_the_chain(gpu, name):
    case = fc.BY_NAME[name]
    rows, res, _ = case_data(name)
    pk, esk = fc.recipient_keys()[0], fc.esk_of(case)
    comb = combiner_of(case)
    d = feed(comb, rows)
    raw, lens, slot = seal_new(comb, case["jobs"], case["dim"], pk, esk)
    raw2, lens2, sums = seal_chain(comb, case["jobs"], case["dim"], pk, esk, slot)
    assert np.array_equal(lens, lens2), f"{name}: lengths differ from finish_dev + seal_share_rows_dev"
    assert raw == raw2, f"{name}: boxes (or the bytes around them) differ from finish_dev + seal_share_rows_dev"
    assert sums.tolist() == res
    del d


# ---- 3. the state stays valid ----------------------------------------------------------------------------------------------------
def test_the_job_stays_valid_for_finish_update_and_another_finish(gpu):
    case = fc.BY_NAME["jobs3"]
    rows, res, want = case_data("jobs3")
    pk, esk = fc.recipient_keys()[0], fc.esk_of(case)
    jobs, dim = case["jobs"], case["dim"]
    comb = combiner_of(case)
    d = feed(comb, rows)
    raw, lens, slot = seal_new(comb, jobs, dim, pk, esk)
    check_against(raw, lens, slot, want, esk, "first finish")
    _, _, sums = seal_chain(comb, jobs, dim, pk, esk, slot)                # finish_dev after the call: the chain's sums
    assert sums.tolist() == res
    more = np.random.default_rng(31).integers(fc.I64_MIN, fc.I64_MAX, size=(jobs, 2, dim), dtype=np.int64)
    d2 = feed(comb, more, begin=False)
    both = np.concatenate([rows, more], axis=1)
    esk2 = bytes(reversed(esk))
    raw, lens, slot = seal_new(comb, jobs, dim, pk, esk2)
    check_against(raw, lens, slot, fc.oracle_boxes(case, rows=both, esk=esk2), esk2, "after another update")
    _, _, sums = seal_chain(comb, jobs, dim, pk, esk2, slot)
    assert sums.tolist() == fc.residues_of(case, both)
    del d, d2


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBytes
    lib = gpu
    case = fc.BY_NAME["jobs2"]
    rows, _, want = case_data("jobs2")
    jobs, dim = case["jobs"], case["dim"]
    pk, esk = fc.recipient_keys()[0], fc.esk_of(case)
    slot = slot_of(dim)
    assert slot % 16 == 0
    comb, codec, box = combiner_of(case), crypto.VarintCodec(), crypto.SealedBox()
    d = feed(comb, rows)
    d_boxes, d_lens = _pattern_buffer(jobs * slot + 64), DeviceBytes(jobs * 8).zero()
    good = dict(c=comb._h, codec=codec._h, b=box._h, pk=pk, esk=esk, d_boxes=d_boxes.ptr, slot_bytes=slot, d_row_bytes=d_lens.ptr, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sda_share_combiner_finish_sealed_rows_dev(*[a[k] for k in good])

    untouched = bytes([PATTERN]) * (jobs * slot + 64)
    signed = combiner_of(case)
    signed.set_value_mode("rust_signed")
    signed.begin_dev(jobs, dim)
    fresh = combiner_of(case)
    bad, unsupported, state = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED, capi.ERR_STATE
    cases = {"NULL combiner": (dict(c=None), bad), "NULL codec": (dict(codec=None), bad), "NULL box handle": (dict(b=None), bad),
             "NULL pk": (dict(pk=None), bad), "NULL d_boxes": (dict(d_boxes=None), bad), "NULL d_row_bytes": (dict(d_row_bytes=None), bad),
             "slot_bytes not a multiple of 16": (dict(slot_bytes=slot + 8), bad), "slot_bytes too small": (dict(slot_bytes=slot - 16), bad),
             "d_boxes misaligned": (dict(d_boxes=d_boxes.ptr + 8), bad), "SDA_VALUES_RUST_SIGNED": (dict(c=signed._h), unsupported),
             "job not begun": (dict(c=fresh._h), state)}
    for what, (kw, status) in cases.items():
        assert call(**kw) == status, what
        assert d_boxes.to_bytes() == untouched, what + ": the box buffer was written"
    if lib.sda_device_count() > 1:                                       # handles on different devices
        capi.check(lib.sda_set_device(1))
        try:
            other_box, other_codec = crypto.SealedBox(), crypto.VarintCodec()
        finally:
            capi.check(lib.sda_set_device(0))
        for kw in (dict(b=other_box._h), dict(codec=other_codec._h), dict(b=other_box._h, codec=other_codec._h)):
            assert call(**kw) == bad
            assert d_boxes.to_bytes() == untouched
    # ... and after all the refusals the handles still work
    assert call() == capi.OK
    check_against(d_boxes.to_bytes(jobs * slot), _lens(d_lens, jobs), slot, want, esk, "after the refusals")
    del d


def test_a_small_order_recipient_key_refuses_every_row(gpu):
    case = fc.BY_NAME["jobs3"]
    rows, _, _ = case_data("jobs3")
    esk = fc.esk_of(case)
    comb = combiner_of(case)
    d = feed(comb, rows)
    raw, lens, slot = seal_new(comb, case["jobs"], case["dim"], fc.SMALL_ORDER, esk, slot_of(case["dim"], extra=16))
    assert list(lens) == [0] * case["jobs"]
    check_against(raw, lens, slot, [None] * case["jobs"], esk, "small-order key")      # the epk, then canaries only
    # the chain refuses the same way
    raw2, lens2, _ = seal_chain(comb, case["jobs"], case["dim"], fc.SMALL_ORDER, esk, slot)
    assert raw == raw2 and np.array_equal(lens, lens2)
    del d


def test_dimension_zero_gives_boxes_of_the_empty_message(gpu):
    from oracle import sealedbox_oracle as so
    from sda_amd import crypto
    pk = fc.recipient_keys()[0]
    esk = bytes(range(96))
    comb = crypto.ShareCombiner(crypto.Additive(3, fc.P62))
    comb.begin_dev(3, 0)
    raw, lens, slot = seal_new(comb, 3, 0, pk, esk)
    assert slot == 48 and list(lens) == [48] * 3
    assert all(raw[48 * j:48 * j + 48] == so.seal(b"", pk, esk[32 * j:32 * j + 32]) for j in range(3))
    raw, lens, slot = seal_new(comb, 3, 0, pk, esk, slot=64)
    check_against(raw, lens, 64, [so.seal(b"", pk, esk[32 * j:32 * j + 32]) for j in range(3)], esk, "dimension 0, padded slots")


# ---- 5. the host helper: process_clerking_job in one method ----------------------------------------------------------------------
def test_clerk_sealed_job_helper(gpu):
    from oracle import coracle, pyoracle as po, sealedbox_oracle as so
    from sda_amd import capi, crypto
    from test_participant_seal_gpu import _keys
    cpk, csk = _keys(41)
    rpk, rsk = fc.recipient_keys()
    P, L = 9, 2 * fc.V + 11
    shares = np.random.default_rng(41).integers(0, fc.P62, size=(P, L), dtype=np.int64)
    boxes = [so.seal(coracle.varint_encode(shares[p]), cpk, bytes([p + 1]) * 32) for p in range(P)]
    blob = bytes(crypto.JobContainer.build(capi.JOB_SEALED, boxes))
    comb = crypto.ShareCombiner(crypto.Additive(3, fc.P62))
    esk = bytes(range(7, 39))
    sums = [sum(int(x) for x in shares[:, i]) % fc.P62 for i in range(L)]
    got = comb.clerk_sealed_job(blob, cpk, csk, rpk, L, esk)
    assert got == so.seal(po.varint_encode(sums), rpk, esk)
    assert po.varint_decode(so.seal_open(comb.clerk_sealed_job(blob, cpk, csk, rpk, L), rpk, rsk)) == sums      # OS entropy
    with pytest.raises(capi.SdaError) as e:
        comb.clerk_sealed_job(blob, cpk, csk, rpk, L + 1, esk)
    assert e.value.code == capi.ERR_WRONG_DIMENSION
    with pytest.raises(capi.SdaError) as e:
        comb.clerk_sealed_job(blob, cpk, csk, fc.SMALL_ORDER, L, esk)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "small-order" in str(e.value)
    empty = bytes(crypto.JobContainer.build(capi.JOB_SEALED, []))
    assert comb.clerk_sealed_job(empty, cpk, csk, rpk, L, esk) == so.seal(b"", rpk, esk)


# ---- 6. the protocol loop in production mode -----------------------------------------------------------------------------------
def test_protocol_loop_in_production_mode(gpu):
    """OS entropy throughout: 5 participations of dimension 50 at k = 3, t = 1, n = 8 over the 62-bit prime, every clerk sums its
    slice of the rows straight from the boxes and seals its result into row c of one buffer, the recipient reconstructs from
    those rows as they are"""
    from oracle import pyoracle as po
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    from test_participant_seal_gpu import _keys
    P, n, k, dim, p = 5, 8, 3, 50, fc.P62
    sch = crypto.PackedShamir(k, n, 1, p, po.P62_OMEGA[8], po.P62_OMEGA[9])
    B = -(-dim // k)
    gen, codec, box = crypto.ShareGenerator(sch), crypto.VarintCodec(), crypto.SealedBox()
    clerk_keys = [_keys(200 + c) for c in range(n)]
    rpk, rsk = fc.recipient_keys()
    sec = np.random.default_rng(51).integers(0, p, size=(P, dim), dtype=np.int64)
    d_sec = DeviceBuffer.from_numpy(sec)
    slot = max(codec.slot_size(B), 16) + 48
    d_boxes, d_lens = _pattern_buffer(n * P * slot), DeviceBytes(n * P * 8).zero()
    gen.generate_sealed_rows_dev(codec, box, [pk for pk, _ in clerk_keys], d_sec.ptr, P, dim, dim, d_boxes.ptr, slot, d_lens.ptr)
    assert (_lens(d_lens, n * P) > 48).all()
    d_rboxes, d_rlens, d_status = _pattern_buffer(n * slot), DeviceBytes(n * 8).zero(), DeviceBytes(4).zero()
    for c, (cpk, csk) in enumerate(clerk_keys):
        comb = crypto.ShareCombiner(sch)
        comb.begin_dev(1, B)
        comb.update_sealed_rows_dev(codec, box, cpk, csk, d_boxes.ptr + c * P * slot, slot, d_lens.ptr + 8 * c * P, P, slot, d_status.ptr)
        comb.finish_sealed_rows_dev(codec, box, rpk, d_rboxes.ptr + c * slot, slot, d_rlens.ptr + 8 * c)
    assert d_status.to_bytes(4) == bytes(4)
    rlens = _lens(d_rlens, n)
    assert (rlens > 48).all() and (rlens <= 48 + 9 * B).all()
    rec = crypto.SecretReconstructor(sch, dim)
    d_total = DeviceBuffer(dim + 2)
    rec.begin_dev(list(range(n)), n, B)
    rec.update_sealed_rows_dev(codec, box, rpk, rsk, 0, d_rboxes.ptr, slot, d_rlens.ptr, n, slot, d_status.ptr)
    rec.finish_dev(d_total.ptr, dim)
    assert d_status.to_bytes(4) == bytes(4)
    truth = [sum(int(x) for x in sec[:, i]) % p for i in range(dim)]
    assert d_total.to_numpy()[:dim].tolist() == truth


# ---- 7. footprint --------------------------------------------------------------------------------------------------------------
def test_footprint_no_result_buffer(gpu):
    """One job of dimension 4 Mi: the chain's result buffer is 32 MiB.  Both forms hold the per-row key state, the Poly1305
    partials of a 40 MiB message bound, the staged keys and the lengths; the new call adds the block byte counts and their scan
    (12 bytes per 2048 values: about 25 KB) and the chain the result buffer.  What the new call newly holds beyond what
    seal_share_rows_dev newly holds for the same row on fresh handles must stay below a quarter of that buffer.  Measured on an
    MI355X: 4,194,304 B newly held by the new call, 0 B by the chain's seal afterwards - allocator granules, not sizes (every
    buffer either form reserves here is far below 1 MiB, and the second form finds room in what the first left reserved)."""
    from oracle import coracle, sealedbox_oracle as so
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    lib = use_test_hooks()                                       # sda_debug_mem_info lives in the library with the test hooks
    dim = 4 << 20
    result_bytes = dim * 8
    pk, sk = fc.recipient_keys()
    esk = bytes(range(50, 82))
    rows = np.random.default_rng(61).integers(fc.I64_MIN, fc.I64_MAX, size=(1, 2, dim), dtype=np.int64)
    comb = crypto.ShareCombiner(crypto.Additive(3, fc.P62))
    d = feed(comb, rows)
    slot = slot_of(dim)
    d_boxes, d_lens, d_out = DeviceBytes(slot), DeviceBytes(8).zero(), DeviceBuffer(dim)

    def free_now():
        synchronize()
        f, t = C.c_size_t(), C.c_size_t()
        capi.check(lib.sda_debug_mem_info(C.byref(f), C.byref(t)))
        return f.value

    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    before = free_now()
    comb.finish_sealed_rows_dev(codec, box, pk, d_boxes.ptr, slot, d_lens.ptr, esk)
    grown = before - free_now()
    n = int(_lens(d_lens, 1)[0])
    got = d_boxes.to_bytes(n)
    comb.finish_dev(d_out.ptr)
    sums = d_out.to_numpy()[:dim]
    assert np.array_equal(sums, coracle.combine(fc.P62, rows[0]))
    assert n == 48 + len(coracle.varint_encode(sums)) and got[:32] == so.x25519_base(esk)
    codec2, box2 = crypto.VarintCodec(), crypto.SealedBox()
    mid = free_now()
    box2.seal_share_rows_dev(codec2, [pk], 1, d_out.ptr, 1, dim, dim, d_boxes.ptr, slot, d_lens.ptr, esk)
    seal_only = mid - free_now()
    assert d_boxes.to_bytes(n) == got                            # the chain's box, which the case table ties to the reference
    print(f"result buffer {result_bytes} B; newly held by the new call {grown} B, by seal_share_rows_dev on fresh handles {seal_only} B, "
          f"excess {grown - seal_only} B")
    assert grown - seal_only < result_bytes / 4
    del d

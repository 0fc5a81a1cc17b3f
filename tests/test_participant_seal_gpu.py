"""sda_sealedbox_seal_share_rows_dev: a participation's share rows sealed in one call (participate.rs:82-101,
encryption/sodium.rs:33-46) - the setup pass, then ONE kernel that varint-encodes a row and xors the XSalsa20 keystream into its
bytes before they are stored, then the Poly1305 pass.  No wire buffer.

The oracle of every case is sealedbox_oracle.seal(coracle.varint_encode(row), pk, esk_r) with injected ephemeral secrets; the
"two-call sequence" is sda_varint_encode_rows_dev + sda_sealedbox_seal_rows_dev with the same secrets.  The box buffer is
prefilled with 0xA5, so a byte written past a row's length shows.

The keystream tile of the kernel holds 64 Salsa20 blocks: it is refilled when the write cursor reaches message byte 4064
(stream piece 256), and again every 4096 bytes (8160, ...)."""
import ctypes as C

import numpy as np
import pytest

from conftest import use_test_hooks

pytestmark = pytest.mark.gpu
P62 = 4611686006577364993
SMALL_ORDER = bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800")
PATTERN = 0xA5
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _keys(seed):
    from oracle import sealedbox_oracle as so
    sk = bytes(np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8))
    return so.x25519_base(sk), sk


def _esk(rows, seed=1):
    return bytes(np.random.default_rng(1000 + seed).integers(0, 256, 32 * rows, dtype=np.uint8))


def _key_of(r, n_pks, rows_per_key):
    return (r // rows_per_key) % n_pks


def oracle_boxes(shares, pks, rows_per_key, esk):
    """the reference's box of every row; None for a row whose recipient key gives the all-zero shared secret"""
    from oracle import coracle, sealedbox_oracle as so
    out = []
    for r in range(shares.shape[0]):
        pk, e = pks[_key_of(r, len(pks), rows_per_key)], esk[32 * r:32 * r + 32]
        try:
            out.append(so.seal(coracle.varint_encode(shares[r]) if shares.shape[1] else b"", pk, e))
        except ValueError:                                               # all-zero shared secret: crypto_box_seal returns -1
            assert so.x25519(e, pk) == bytes(32)
            out.append(None)
    return out


class Rows:
    """a share matrix resident in HBM with a chosen row stride and element offset; junk between the rows"""

    def __init__(self, shares, stride=None, offset=0):
        from sda_amd.device import DeviceBuffer
        self.rows, self.len = shares.shape
        self.stride = self.len if stride is None else stride
        host = np.random.default_rng(7).integers(I64_MIN, I64_MAX, size=offset + self.rows * self.stride + 1, dtype=np.int64)
        for r in range(self.rows):
            host[offset + r * self.stride:offset + r * self.stride + self.len] = shares[r]
        self.buf = DeviceBuffer.from_numpy(host)
        self.ptr = self.buf.at(offset)


def _pattern_buffer(nbytes):
    from sda_amd import capi
    from sda_amd.device import DeviceBytes
    d = DeviceBytes(nbytes)
    capi.check(capi.load().sda_dev_memset(d._p, PATTERN, max(nbytes, 16)))
    return d


def run_fused(R, pks, rows_per_key, esk, slot=None):
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    slot = codec.slot_size(R.len) + 48 if slot is None else slot
    d_boxes, d_lens = _pattern_buffer(R.rows * slot), DeviceBytes(R.rows * 8).zero()
    box.seal_share_rows_dev(codec, pks, rows_per_key, R.ptr, R.rows, R.len, R.stride, d_boxes.ptr, slot, d_lens.ptr, esk)
    return d_boxes.to_bytes(R.rows * slot), np.frombuffer(d_lens.to_bytes(R.rows * 8), dtype="<u8").copy(), slot


def run_two_call(R, pks, rows_per_key, esk, slot):
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    vslot = max(codec.slot_size(R.len), 16)
    d_wire, d_wlen = DeviceBytes(R.rows * vslot), DeviceBytes(R.rows * 8).zero()
    codec.encode_rows_dev(R.ptr, R.rows, R.len, R.stride, d_wire.ptr, vslot, d_wlen.ptr)
    d_boxes, d_lens = _pattern_buffer(R.rows * slot), DeviceBytes(R.rows * 8).zero()
    box.seal_rows_dev(pks, rows_per_key, d_wire.ptr, vslot, d_wlen.ptr, R.rows, codec.slot_size(R.len), d_boxes.ptr, slot, d_lens.ptr, esk)
    return d_boxes.to_bytes(R.rows * slot), np.frombuffer(d_lens.to_bytes(R.rows * 8), dtype="<u8").copy()


def check_against(raw, lens, slot, want, esk, what):
    from oracle import sealedbox_oracle as so
    tail = bytes([PATTERN])
    for r, w in enumerate(want):
        row = raw[r * slot:(r + 1) * slot]
        if w is None:                                                    # refused: length 0, the epk, nothing else
            assert lens[r] == 0, f"{what}: refused row {r} has length {lens[r]}"
            assert row[:32] == so.x25519_base(esk[32 * r:32 * r + 32]), f"{what}: refused row {r}: epk"
            assert row[32:] == tail * (slot - 32), f"{what}: refused row {r} was written past byte 32"
            continue
        assert lens[r] == len(w), f"{what}: row {r} has length {lens[r]}, the oracle's box {len(w)}"
        if row[:len(w)] != w:
            first = next(i for i in range(len(w)) if row[i] != w[i])
            raise AssertionError(f"{what}: row {r} differs from the oracle's box from byte {first} (message byte {first - 48}) of {len(w)}")
        assert row[len(w):] == tail * (slot - len(w)), f"{what}: row {r} was written past its length {len(w)}"


def check(shares, pks, rows_per_key=None, stride=None, offset=0, seed=1, two_call=True):
    """the new call against the oracle and against the two-call sequence; returns (raw boxes, lengths, slot, oracle boxes)"""
    shares = np.ascontiguousarray(shares, dtype=np.int64)
    rows = shares.shape[0]
    rows_per_key = rows if rows_per_key is None else rows_per_key
    esk = _esk(rows, seed)
    R = Rows(shares, stride, offset)
    raw, lens, slot = run_fused(R, pks, rows_per_key, esk)
    want = oracle_boxes(shares, pks, rows_per_key, esk)
    print(f"rows {rows} len {shares.shape[1]} stride {R.stride}: lengths {lens.min()}..{lens.max()}, slot {slot}")
    check_against(raw, lens, slot, want, esk, "one call")
    if two_call:
        raw2, lens2 = run_two_call(R, pks, rows_per_key, esk, slot)
        assert np.array_equal(lens, lens2), "lengths differ from encode_rows_dev + seal_rows_dev"
        assert raw == raw2, "boxes (or the bytes around them) differ from encode_rows_dev + seal_rows_dev"
    return raw, lens, slot, want


# ---- 1. shapes over the 62-bit prime ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,L", [(1, 1), (5, 7), (17, 333), (64, 5000)])
def test_shapes_over_the_62_bit_prime(gpu, rows, L):
    pk, _ = _keys(rows * 131 + L)
    shares = np.random.default_rng(rows + L).integers(0, P62, size=(rows, L), dtype=np.int64)
    check(shares, [pk])


# ---- 2. value widths -------------------------------------------------------------------------------------------------------
def test_every_varint_length_at_its_edges(gpu):
    pk, _ = _keys(2)
    vals = [0, -1, 1, 63, -63, 64, -64, 65, -65, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1]
    for k in range(1, 10):                                               # zig-zag(v) crosses 7k bits at +-2^(7k-1)
        e = 1 << (7 * k - 1)
        vals += [e - 1, e, e + 1, -e + 1, -e, -e - 1]
    vals = [v for v in vals if I64_MIN <= v <= I64_MAX]
    from oracle import coracle
    assert {len(coracle.varint_encode(np.array([v], dtype=np.int64))) for v in vals} == set(range(1, 11))
    rng = np.random.default_rng(22)
    rows = [np.array(vals, dtype=np.int64), rng.permutation(np.array(vals * 9, dtype=np.int64))[:len(vals)]]
    check(np.stack(rows), [pk])


def test_slowest_fastest_and_drifting_cursor(gpu):
    """all 1-byte values (128 B per step: two refills in 9000 bytes), all 10-byte values (1280 B per step: a refill every
    3.2 steps), and random widths, so that the cursor drifts against the step index"""
    pk, _ = _keys(3)
    rng = np.random.default_rng(33)
    L = 9000
    one = rng.integers(-64, 64, size=L)
    ten = np.where(rng.integers(0, 2, size=L) == 0, rng.integers(I64_MIN, -(1 << 62) - 1, size=L), rng.integers(1 << 62, I64_MAX, size=L))
    width = rng.integers(1, 11, size=L)                                   # zig-zag values of 7 w - 6 .. 7 w bits
    zz = np.array([int(rng.integers(1 << (7 * w - 7), 1 << min(7 * w, 64), dtype=np.uint64)) for w in map(int, width)], dtype=np.uint64)
    mixed = ((zz >> np.uint64(1)) ^ (np.uint64(0) - (zz & np.uint64(1)))).astype(np.int64)
    raw, lens, slot, want = check(np.stack([one, ten, mixed]).astype(np.int64), [pk])
    assert lens[0] == L + 48 and lens[1] == 10 * L + 48


# ---- 3. payload lengths across the boundaries the kernel has -------------------------------------------------------------
@pytest.mark.parametrize("L", range(1, 71))
def test_every_payload_length_up_to_70(gpu, L):
    """rows of 1-byte values: below and across the first Salsa20 block edge (message byte 32), the 16- and 64-byte grids"""
    pk, _ = _keys(4)
    shares = np.random.default_rng(L).integers(-64, 64, size=(2, L), dtype=np.int64)
    raw, lens, slot, want = check(shares, [pk], seed=L)
    assert list(lens) == [L + 48, L + 48]


@pytest.mark.parametrize("edge", [1024, 4064, 8160, 16384, 32768])
def test_payload_lengths_around_an_edge(gpu, edge):
    """payloads of edge - 2 .. edge + 2 bytes: 1024 (a step of 1-byte values ends), 4064 and 8160 (first and second refill of
    the 64-block keystream tile), 16384 and 32768 (Poly1305 regions).  L = edge - 2, row k holds k two-byte values."""
    pk, _ = _keys(5)
    rng = np.random.default_rng(edge)
    L = edge - 2
    shares = rng.integers(-64, 64, size=(5, L), dtype=np.int64)
    for k in range(5):
        shares[k, rng.choice(L, size=k, replace=False)] = rng.integers(64, 8192, size=k)
    raw, lens, slot, want = check(shares, [pk], seed=edge)
    assert list(lens) == [edge - 2 + k + 48 for k in range(5)]


def test_one_row_of_40_kilobytes(gpu):
    pk, _ = _keys(6)
    shares = np.random.default_rng(6).integers(0, P62, size=(1, 4500), dtype=np.int64)
    raw, lens, slot, want = check(shares, [pk])
    assert 40_000 < lens[0] < 41_000


# ---- 4. layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,offset", [(1400, 0), (1301, 0), (1300, 1), (1303, 1)])
def test_row_stride_and_unaligned_rows(gpu, stride, offset):
    """row_stride > len; an odd stride or an offset of one element puts rows off the 16-byte grid (the scalar load path)"""
    pk, _ = _keys(7)
    shares = np.random.default_rng(stride + offset).integers(0, P62, size=(6, 1300), dtype=np.int64)
    check(shares, [pk], stride=stride, offset=offset)


@pytest.mark.parametrize("rows", [1, 3, 4, 5])
def test_rows_either_side_of_a_workgroup(gpu, rows):
    pk, _ = _keys(8)
    shares = np.random.default_rng(rows).integers(0, P62, size=(rows, 700), dtype=np.int64)
    check(shares, [pk])


@pytest.mark.parametrize("major", ["job", "participant"])
def test_three_clerk_keys(gpu, major):
    """job-major [n][P] with rows_per_key = P, participant-major [P][n] with rows_per_key = 1; every box opens with the secret
    key of the clerk it was meant for and with no other"""
    from oracle import coracle, sealedbox_oracle as so
    keys = [_keys(90 + i) for i in range(3)]
    P, L = 4, 500
    shares = np.random.default_rng(9).integers(0, P62, size=(3 * P, L), dtype=np.int64)
    rpk = P if major == "job" else 1
    raw, lens, slot, want = check(shares, [k[0] for k in keys], rows_per_key=rpk)
    for r in range(3 * P):
        c = r // P if major == "job" else r % 3
        box = raw[r * slot:r * slot + int(lens[r])]
        assert so.seal_open(box, *keys[c]) == coracle.varint_encode(shares[r])
        with pytest.raises(ValueError):
            so.seal_open(box, *keys[(c + 1) % 3])


# ---- 5. len == 0 ---------------------------------------------------------------------------------------------------------------
def test_len_zero_gives_the_box_of_the_empty_message(gpu):
    from oracle import sealedbox_oracle as so
    pk, sk = _keys(10)
    raw, lens, slot, want = check(np.zeros((5, 0), dtype=np.int64), [pk])
    assert slot == 48 and list(lens) == [48] * 5
    assert all(so.seal_open(raw[r * 48:r * 48 + 48], pk, sk) == b"" for r in range(5))
    # d_values may be NULL when len == 0
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    d_boxes, d_lens = _pattern_buffer(5 * 48), DeviceBytes(5 * 8).zero()
    crypto.SealedBox().seal_share_rows_dev(crypto.VarintCodec(), [pk], 5, 0, 5, 0, 0, d_boxes.ptr, 48, d_lens.ptr, _esk(5))
    assert d_boxes.to_bytes(5 * 48) == raw


# ---- 6. small-order recipient key ------------------------------------------------------------------------------------------
def test_small_order_recipient_key_is_refused_per_row(gpu):
    pk0, _ = _keys(11)
    pk2, _ = _keys(12)
    shares = np.random.default_rng(11).integers(0, P62, size=(9, 600), dtype=np.int64)
    raw, lens, slot, want = check(shares, [pk0, SMALL_ORDER, pk2], rows_per_key=2)      # keys 0 0 1 1 2 2 0 0 1
    assert [w is None for w in want] == [False, False, True, True, False, False, False, False, True]
    assert [int(x) for x in lens[[2, 3, 8]]] == [0, 0, 0] and (lens[[0, 1, 4, 5, 6, 7]] > 48).all()


# ---- 7. OS entropy -----------------------------------------------------------------------------------------------------------
def test_os_entropy_boxes_open_and_differ_between_calls(gpu):
    from oracle import coracle
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    pk, sk = _keys(13)
    P, L = 64, 2000
    shares = np.random.default_rng(13).integers(0, P62, size=(P, L), dtype=np.int64)
    R = Rows(shares)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    slot = codec.slot_size(L) + 48
    runs = []
    for _ in range(2):
        d_boxes, d_lens = _pattern_buffer(P * slot), DeviceBytes(P * 8).zero()
        box.seal_share_rows_dev(codec, [pk], P, R.ptr, P, L, L, d_boxes.ptr, slot, d_lens.ptr)
        runs.append((d_boxes, d_lens, d_boxes.to_bytes(P * slot), np.frombuffer(d_lens.to_bytes(P * 8), dtype="<u8").copy()))
    d_boxes, d_lens, raw, lens = runs[0]
    assert (lens > 48).all()
    comb = crypto.ShareCombiner(crypto.Additive(3, P62))
    d_status, sums = DeviceBytes(4).zero(), DeviceBuffer(L)
    comb.begin_dev(1, L)
    comb.update_sealed_rows_dev(codec, box, pk, sk, d_boxes.ptr, slot, d_lens.ptr, P, slot, d_status.ptr)
    comb.finish_dev(sums.ptr)
    assert d_status.to_bytes(4) == bytes(4)
    assert np.array_equal(sums.to_numpy(), coracle.combine(P62, shares))
    assert np.array_equal(crypto.ShareDecryptor(pk, sk).decrypt(raw[:int(lens[0])]), shares[0])
    raw2 = runs[1][2]
    epk = lambda b, r: b[r * slot:r * slot + 32]
    assert all(epk(raw, r) != epk(raw2, r) for r in range(P))
    assert len({epk(raw, r) for r in range(P)}) == P


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBytes
    lib = capi.load()
    pk, _ = _keys(14)
    rows, L = 4, 10
    shares = np.random.default_rng(14).integers(0, P62, size=(rows, L), dtype=np.int64)
    R = Rows(shares)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    slot = codec.slot_size(L) + 48
    assert slot % 16 == 0
    d_boxes, d_lens = _pattern_buffer(rows * slot + 64), DeviceBytes(rows * 8).zero()
    esk = _esk(rows)
    good = dict(b=box._h, codec=codec._h, pks=pk, n_pks=1, rows_per_key=rows, esk=esk, d_values=R.ptr, rows=rows, len=L, row_stride=L,
                d_boxes=d_boxes.ptr, slot_bytes=slot, d_row_bytes=d_lens.ptr, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sda_sealedbox_seal_share_rows_dev(*[a[k] for k in good])

    untouched = bytes([PATTERN]) * (rows * slot + 64)
    cases = {"NULL box handle": dict(b=None), "NULL codec": dict(codec=None), "NULL pks": dict(pks=None), "NULL d_values": dict(d_values=None),
             "NULL d_boxes": dict(d_boxes=None), "NULL d_row_bytes": dict(d_row_bytes=None), "row_stride < len": dict(row_stride=L - 1),
             "slot_bytes not a multiple of 16": dict(slot_bytes=slot + 8), "slot_bytes too small": dict(slot_bytes=slot - 16),
             "d_boxes misaligned": dict(d_boxes=d_boxes.ptr + 8), "n_pks == 0": dict(n_pks=0), "rows_per_key == 0": dict(rows_per_key=0)}
    for what, kw in cases.items():
        assert call(**kw) == capi.ERR_INVALID_ARGUMENT, what
        assert d_boxes.to_bytes() == untouched, what + ": the box buffer was written"
    if lib.sda_device_count() > 1:                                       # handles on different devices
        capi.check(lib.sda_set_device(1))
        try:
            other = crypto.SealedBox()
        finally:
            capi.check(lib.sda_set_device(0))
        assert call(b=other._h) == capi.ERR_INVALID_ARGUMENT
        assert d_boxes.to_bytes() == untouched
    assert call(rows=0) == capi.OK
    assert d_boxes.to_bytes() == untouched
    # ... and after all the refusals the handles still work
    assert call() == capi.OK
    want = oracle_boxes(shares, [pk], rows, esk)
    check_against(d_boxes.to_bytes(rows * slot), np.frombuffer(d_lens.to_bytes(), dtype="<u8"), slot, want, esk, "after the refusals")


# ---- 9. footprint ------------------------------------------------------------------------------------------------------------
def test_footprint_no_wire_buffer(gpu):
    """256 rows of 100,000 shares (about 230 MB of boxes): the new call newly holds at most 5 % of the box bytes (per-row key
    state, Poly1305 partials, staged keys, message lengths: about 3.7 KB against 900 KB of box), a second call of the same size
    nothing more, and the two-call sequence needs at least the payload bytes for its wire buffer."""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    from oracle import coracle, sealedbox_oracle as so
    lib = use_test_hooks()                                       # sda_debug_mem_info lives in the library with the test hooks
    pk, sk = _keys(15)
    P, L = 256, 100_000
    shares = np.random.default_rng(15).integers(0, P62, size=(P, L), dtype=np.int64)
    d_sh = DeviceBuffer.from_numpy(shares)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    vslot = codec.slot_size(L)
    slot = vslot + 48
    d_boxes, d_lens = DeviceBytes(P * slot), DeviceBytes(P * 8).zero()
    esk = _esk(P)

    def free_now():
        synchronize()
        f, t = C.c_size_t(), C.c_size_t()
        capi.check(lib.sda_debug_mem_info(C.byref(f), C.byref(t)))
        return f.value

    before = free_now()
    box.seal_share_rows_dev(codec, [pk], P, d_sh.ptr, P, L, L, d_boxes.ptr, slot, d_lens.ptr, esk)
    first = before - free_now()
    lens = np.frombuffer(d_lens.to_bytes(), dtype="<u8").copy()
    box_bytes = int(lens.sum())
    assert box_bytes > 220e6
    for r in (0, 97, 255):
        got = d_boxes.to_bytes(int(lens[r]), r * slot)
        assert got == so.seal(coracle.varint_encode(shares[r]), pk, esk[32 * r:32 * r + 32]), f"row {r}"
    mid = free_now()
    box.seal_share_rows_dev(codec, [pk], P, d_sh.ptr, P, L, L, d_boxes.ptr, slot, d_lens.ptr, esk)
    second = mid - free_now()
    print(f"box bytes {box_bytes}, newly held after the first call {first} ({100.0 * first / box_bytes:.3f} %), after the second {second}")
    assert first <= 0.05 * box_bytes
    assert second == 0
    # the two-call sequence: its wire buffer alone is the payload of every box again
    codec2, box2 = crypto.VarintCodec(), crypto.SealedBox()
    before2 = free_now()
    d_wire, d_wlen = DeviceBytes(P * vslot), DeviceBytes(P * 8).zero()
    codec2.encode_rows_dev(d_sh.ptr, P, L, L, d_wire.ptr, vslot, d_wlen.ptr)
    box2.seal_rows_dev([pk], P, d_wire.ptr, vslot, d_wlen.ptr, P, vslot, d_boxes.ptr, slot, d_lens.ptr, esk)
    two = before2 - free_now()
    print(f"two-call sequence: {two} bytes newly held, payload bytes {box_bytes - 48 * P}")
    assert two >= box_bytes - 48 * P


# ---- 10. the host helper -----------------------------------------------------------------------------------------------------
def test_encrypt_rows_helper(gpu):
    from sda_amd import capi, crypto
    pk, sk = _keys(16)
    P, L = 12, 777
    shares = np.random.default_rng(16).integers(0, P62, size=(P, L), dtype=np.int64)
    esk = _esk(P)
    got = crypto.ShareEncryptor(pk).encrypt_rows(shares, esk)
    assert got == oracle_boxes(shares, [pk], P, esk)
    assert np.array_equal(crypto.ShareDecryptor(pk, sk).decrypt(got[5]), shares[5])
    with pytest.raises(capi.SdaError) as e:
        crypto.ShareEncryptor(SMALL_ORDER).encrypt_rows(shares, esk)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "small-order" in str(e.value)
    # OS entropy: the boxes open to the rows
    fresh = crypto.ShareEncryptor(pk).encrypt_rows(shares[:3])
    dec = crypto.ShareDecryptor(pk, sk)
    assert all(np.array_equal(dec.decrypt(fresh[r]), shares[r]) for r in range(3))


# ---- 11. kernel note ---------------------------------------------------------------------------------------------------------
def test_the_call_reports_its_kernels(gpu):
    pk, _ = _keys(17)
    shares = np.random.default_rng(17).integers(0, P62, size=(8, 50), dtype=np.int64)
    run_fused(Rows(shares), [pk], 8, _esk(8))
    assert gpu.sda_debug_last_kernel().decode().startswith("varint_seal_stream_kernel + sbox_poly_kernel")

"""The wire codec kernels at every tile, chunk and length boundary (pytest -m gpu), bit-exact.

The inputs are the crafted cases of tests/varint_limits.py: a value of every length across every lane, block, chunk and group
boundary at every split, rows at every start and end phase, encoder steps with every carried byte count and byte phase, the
u32 -> u64 scan with a second chunk, and damaged rows that name the status bit they must raise.  Expected bytes come from the
Python-integer codec of that module (held against both oracles by tests/test_varint_limits_reach.py, which also proves on the
CPU that the cases reach what their names say).  Every output buffer is prefilled with a sentinel that must survive wherever
the kernels have nothing to write; every legal input must leave the status at 0."""
import functools

import numpy as np
import pytest

import varint_limits as V
from conftest import set_knob

pytestmark = pytest.mark.gpu

SENT = -0x0123456789ABCDEF            # value sentinel
BYTE = 0xA5                           # byte sentinel
PATHS = ["scan", "stream"]


def _pattern(nbytes, byte=BYTE):
    from sda_amd import capi
    from sda_amd.device import DeviceBytes
    d = DeviceBytes(nbytes)
    capi.check(capi.load().sda_dev_memset(d._p, byte, max(nbytes, 16)))
    return d


def _wire(raw, base=0):
    """raw in HBM with `base` bytes of 0xff in front of it (the stream starts off the 16-byte grid) and 64 behind"""
    from sda_amd.device import DeviceBytes
    d = DeviceBytes.from_bytes(b"\xff" * base + bytes(raw) + b"\xff" * 64)
    return d, d.ptr + base


def _values(rows, stride, base8=False):
    """the value matrix in HBM: row r at element r * stride (+ 1 element: rows 8 bytes off the 16-byte grid), SENT in between"""
    from sda_amd.device import DeviceBuffer
    m = np.asarray(rows, dtype=np.int64)
    off = 1 if base8 else 0
    host = np.full(off + m.shape[0] * stride + 2, SENT, dtype=np.int64)
    for r in range(m.shape[0]):
        host[off + r * stride:off + r * stride + m.shape[1]] = m[r]
    d = DeviceBuffer.from_numpy(host)
    return d, d.at(off)


def _offsets(offs):
    from sda_amd.device import DeviceBuffer
    return DeviceBuffer.from_numpy(np.asarray(offs, dtype=np.int64))


# ---- encode_dev: the three-pass scan encode ----------------------------------------------------------------------------------------
def _check_encode_dev(rows, L, stride, base8, mat, want, want_offs, out_offsets=(0, 1, 2, 3)):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    codec = crypto.VarintCodec()
    d_vals, ptr = _values(mat, stride, base8)
    assert (ptr % 16 == 0 and stride % 2 == 0) == (not base8 and stride % 2 == 0)
    for o in out_offsets:
        d_out = _pattern(o + len(want) + 64)
        d_off = DeviceBuffer.from_numpy(np.full(rows + 2, SENT, dtype=np.int64))
        total = codec.encode_dev(ptr, rows, L, stride, d_out.ptr + o, len(want) + 8, d_off.ptr)
        got = d_out.to_bytes()
        assert total == len(want), (o, total, len(want))
        if got[o:o + total] != want:
            first = next(i for i in range(total) if got[o + i] != want[i])
            raise AssertionError(f"d_out + {o}: the bytes differ from byte {first} of {total}")
        assert got[:o] == bytes([BYTE]) * o and got[o + total:] == bytes([BYTE]) * (len(got) - o - total), f"d_out + {o}: written outside [0, total)"
        offs = d_off.to_numpy()
        assert offs[:rows + 1].tolist() == list(want_offs) and offs[rows + 1] == SENT, o


@pytest.mark.parametrize("shape", V.SCAN_ENCODE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-stride{s[2]}" + ("-base8" if s[3] else ""))
def test_scan_encode_shapes(gpu, shape):
    """varint_len_kernel's pair walk (several rows per step, the pair that takes the next row's first element, the scalar
    loads of odd strides and of a base 8 bytes off the grid) and varint_write_kernel's head / dword / tail copy-out at the four
    destination alignments; the first shape ends in a block of a single byte"""
    rows, L, stride, base8, _ = shape
    case = V.scan_encode_case(shape)
    _check_encode_dev(rows, L, stride, base8, case.rows, case.raw, case.offsets)


def test_scan_encode_length_edges(gpu):
    case = V.edges_case()
    for stride, base8 in V.EDGES_ENCODE_LAYOUTS:
        _check_encode_dev(1, case.L, stride, base8, case.rows, case.raw, case.offsets)


def test_scan_encode_1025_blocks(gpu):
    """2048 * 1024 + 1 one-byte values: block 1024 takes its offset from the second chunk of the u32 -> u64 scan"""
    vals, raw = V.scan_boundary_sizes()["encode"]()
    _check_encode_dev(1, vals.size, vals.size, False, vals[None, :], raw, [0, len(raw)])


# ---- decode_dev, both forms --------------------------------------------------------------------------------------------------------
def _check_decode_dev(path, raw, offsets, rows, L, want, base=0):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    set_knob("SDA_VARINT_PATH", path)
    d_bytes, ptr = _wire(raw, base)
    d_off = _offsets(offsets)
    stride = L + 3
    d_out = DeviceBuffer.from_numpy(np.full((rows + 2) * stride, SENT, dtype=np.int64))
    st = DeviceBuffer(1).zero()
    crypto.VarintCodec().decode_dev(ptr, len(raw), d_off.ptr if rows > 1 else 0, rows, L, d_out.ptr + 8 * stride, stride, st.ptr)
    got = d_out.to_numpy().reshape(rows + 2, stride)
    assert int(st.to_numpy()[0]) == 0, (path, base)
    bad = np.argwhere(got[1:-1, :L] != want)
    assert bad.size == 0, f"{path}, base {base}: row {bad[0][0]} value {bad[0][1]} of {L} is {got[1 + bad[0][0], bad[0][1]]}, expected {want[bad[0][0], bad[0][1]]}"
    assert (got[0] == SENT).all() and (got[-1] == SENT).all() and (got[1:-1, L:] == SENT).all(), f"{path}, base {base}: written outside the rows"


DECODE_CASES = ["straddle 16", "straddle 1024", "straddle 4096", "phases", "chunks", "single", "ends"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", range(len(DECODE_CASES)), ids=DECODE_CASES)
def test_decode_straddles_and_phased_rows(gpu, which, path):
    """a value of every length with every split across the lane, chunk, block and group boundaries; rows that start and end at
    every phase of the 16-byte grid (again with the stream itself 1..15 bytes off the grid), of 1, 4 and 5 chunks, ending on a
    chunk boundary and one byte past it, and a single byte"""
    case, bases = V.decode_stream_cases()[which]
    for base in bases:
        _check_decode_dev(path, case.raw, case.offsets, len(case.rows), case.L, case.matrix(), base)


@pytest.mark.parametrize("path", PATHS)
def test_decode_ragged_tails(gpu, path):
    """n_bytes % 16 = 0..15 behind a full block"""
    for case in V.scan_boundary_sizes()["tails"]:
        _check_decode_dev(path, case.raw, case.offsets, 1, case.L, case.matrix())


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_decode_across_1024_blocks(gpu, delta, path):
    """4096 * 1024 + delta bytes of ten-byte values that all differ: 1025 / 1025 / 1026 entries in the u32 -> u64 scan; with
    delta = 0 the row check reads the extra zero entry, the first of the scan's second chunk"""
    vals, raw = V.scan_boundary_sizes()["decode"][delta]()
    _check_decode_dev(path, raw, [0, len(raw)], 1, vals.size, vals[None, :])


def _status(path, d):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    set_knob("SDA_VARINT_PATH", path)
    d_bytes, ptr = _wire(d.raw)
    d_off = _offsets(d.offsets)
    stride = d.L + 3
    d_out = DeviceBuffer.from_numpy(np.full((d.rows + 2) * stride, SENT, dtype=np.int64))
    st = DeviceBuffer(1).zero()
    crypto.VarintCodec().decode_dev(ptr, len(d.raw), d_off.ptr if d.rows > 1 else 0, d.rows, d.L, d_out.ptr + 8 * stride, stride, st.ptr)
    got = d_out.to_numpy().reshape(d.rows + 2, stride)
    assert (got[0] == SENT).all() and (got[-1] == SENT).all() and (got[1:-1, d.L:] == SENT).all(), f"{path}, {d.name}: written outside the rows"
    return int(st.to_numpy()[0]), got[1:-1, :d.L]


@pytest.mark.parametrize("path", PATHS)
def test_damage_raises_the_bit_it_calls_for(gpu, path):
    """each decode form on its own: a row that ends inside a value -> 4, a wrong expected length -> 2, more than ten bytes
    without a terminator (across a lane, chunk and block boundary at every split, and with the whole look-back window empty)
    -> 1, and nothing else; ten bytes at the same splits, and ff x 9 7f, are legal and decode to the reference's values"""
    for d in V.damage_cases():
        st, got = _status(path, d)
        assert st == d.bit, f"{path}: {d.name}: status {st}, expected {d.bit}"
        if d.bit == 0:
            assert got[0].tolist() == d.values, f"{path}: {d.name}"


# ---- slotted rows: the streaming encoder and decoder -------------------------------------------------------------------------------
def _slotted(enc_rows, slot):
    """rows at r * slot, 0xff everywhere else"""
    from sda_amd.device import DeviceBuffer, DeviceBytes
    raw = bytearray(b"\xff" * (len(enc_rows) * slot + 64))
    for r, e in enumerate(enc_rows):
        raw[r * slot:r * slot + len(e)] = e
    return DeviceBytes.from_bytes(raw), DeviceBuffer.from_numpy(np.array([len(e) for e in enc_rows], dtype=np.int64))


ENCODE_CASES = ["4 steps + 1", "4 steps", "127 values", "128 values", "refills", "LENGTH_EDGES"]


def _encode_case(which):
    case = V.stream_encode_cases()[which]
    assert case.name == ENCODE_CASES[which]
    return case


@pytest.mark.parametrize("stride_pad", V.ENCODE_STRIDE_PADS, ids=lambda p: f"pad{p}")
@pytest.mark.parametrize("which", range(len(ENCODE_CASES)), ids=ENCODE_CASES)
def test_stream_encode_steps(gpu, which, stride_pad):
    """encode_rows_dev: every carried byte count, every length at every byte phase of tile_or, steps of 8 and of 80 units (the
    second store), 1, 4 and 5 steps, rows on and 8 bytes off the 16-byte grid; nothing written past a row's length"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    case = _encode_case(which)
    rows, L = len(case.rows), case.L
    stride = L + stride_pad
    d_vals, ptr = _values(case.rows, stride)
    codec = crypto.VarintCodec()
    slot = codec.slot_size(L) + 16
    d_out = _pattern(rows * slot + 32)
    d_len = DeviceBuffer.from_numpy(np.full(rows + 1, SENT, dtype=np.int64))
    codec.encode_rows_dev(ptr, rows, L, stride, d_out.ptr, slot, d_len.ptr)
    lens, raw = d_len.to_numpy(), d_out.to_bytes()
    assert lens[:rows].tolist() == [len(e) for e in case.enc] and lens[rows] == SENT
    for r, e in enumerate(case.enc):
        row = raw[r * slot:(r + 1) * slot]
        if row[:len(e)] != e:
            first = next(i for i in range(len(e)) if row[i] != e[i])
            raise AssertionError(f"row {r}: differs from byte {first} (unit {first // 16}) of {len(e)}")
        assert row[len(e):] == bytes([BYTE]) * (slot - len(e)), f"row {r}: written past its length {len(e)}"
    assert raw[rows * slot:] == bytes([BYTE]) * 32


SLOTTED_CASES = ["straddle 1024", "straddle 4096", "phases", "chunks", "single", "ends"]


@pytest.mark.parametrize("which", range(len(SLOTTED_CASES)), ids=SLOTTED_CASES)
def test_slotted_decode(gpu, which):
    """decode_rows_dev: rows at the start of their slots with 0xff in front of them"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    case = V.slotted_decode_cases()[which]
    rows, L = len(case.rows), case.L
    codec = crypto.VarintCodec()
    slot = codec.slot_size(L) + 16
    d_bytes, d_len = _slotted(case.enc, slot)
    stride = L + 3
    d_out = DeviceBuffer.from_numpy(np.full((rows + 2) * stride, SENT, dtype=np.int64))
    st = DeviceBuffer(1).zero()
    codec.decode_rows_dev(d_bytes.ptr, slot, d_len.ptr, rows, L, d_out.ptr + 8 * stride, stride, st.ptr)
    got = d_out.to_numpy().reshape(rows + 2, stride)
    assert int(st.to_numpy()[0]) == 0
    bad = np.argwhere(got[1:-1, :L] != case.matrix())
    assert bad.size == 0, f"row {bad[0][0]} value {bad[0][1]} of {L}"
    assert (got[0] == SENT).all() and (got[-1] == SENT).all() and (got[1:-1, L:] == SENT).all()


# ---- the wire-fed clerk sums -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _jobs(which, jobs):
    """(rows job-major, their bytes, expected sums [jobs][L]) of decode_stream_cases()[which]"""
    case = V.decode_stream_cases()[which][0]
    q = V.P62 if jobs == 1 else 433
    per_job = [case.rows] if jobs == 1 else V.three_jobs(case.rows)
    enc_of = {id(r): e for r, e in zip(case.rows, case.enc)}
    rows = [r for job in per_job for r in job]
    return rows, [enc_of[id(r)] for r in rows], np.stack([V.column_sums(job, q) for job in per_job]), q, case.L


def _finish(comb, jobs, L):
    from sda_amd.device import DeviceBuffer
    out = DeviceBuffer.from_numpy(np.full(jobs * L + 1, SENT, dtype=np.int64))
    comb.finish_dev(out.ptr)
    got = out.to_numpy()
    assert got[-1] == SENT, "finish_dev wrote past its jobs * L sums"
    return got[:-1].reshape(jobs, L)


@pytest.mark.parametrize("jobs", [1, 3])
@pytest.mark.parametrize("form", ["offsets-scan", "offsets-stream", "slots"])
@pytest.mark.parametrize("which", range(len(DECODE_CASES)), ids=DECODE_CASES)
def test_wire_fed_clerk_sums(gpu, which, form, jobs):
    """update_encoded_dev (under both decode forms) and update_encoded_rows_dev on the straddle and phased rows, one job and
    three jobs, against Python-integer column sums reduced mod q"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    rows, enc, want, q, L = _jobs(which, jobs)
    codec = crypto.VarintCodec()
    comb = crypto.ShareCombiner(crypto.Additive(3, q))
    st = DeviceBuffer(1).zero()
    comb.begin_dev(jobs, L)
    if form == "slots":
        slot = codec.slot_size(L)
        d_bytes, d_len = _slotted(enc, slot)
        comb.update_encoded_rows_dev(codec, d_bytes.ptr, slot, d_len.ptr, len(rows), st.ptr)
    else:
        set_knob("SDA_VARINT_PATH", form.split("-")[1])
        raw = b"".join(enc)
        d_bytes, ptr = _wire(raw)
        d_off = _offsets(np.cumsum([0] + [len(e) for e in enc]))
        comb.update_encoded_dev(codec, ptr, len(raw), d_off.ptr, len(rows), st.ptr)
    got = _finish(comb, jobs, L)
    assert int(st.to_numpy()[0]) == 0
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"job {bad[0][0]} column {bad[0][1]}: {got[bad[0][0], bad[0][1]]}, expected {want[bad[0][0], bad[0][1]]}"


# ---- the sealed forms --------------------------------------------------------------------------------------------------------------
SEALED_CASES = ["4 steps + 1", "4 steps", "127 values", "128 values", "refills", "LENGTH_EDGES", "straddle 1024/1024", "straddle 4096/4096",
                "phases", "chunks", "single", "ends"]


@pytest.mark.parametrize("stride_pad", V.SEALED_STRIDE_PADS, ids=lambda p: f"pad{p}")
@pytest.mark.parametrize("which", range(len(SEALED_CASES)), ids=SEALED_CASES)
def test_sealed_encode_and_sealed_sums(gpu, which, stride_pad):
    """seal_share_rows_dev: the boxes equal the oracle's boxes of the reference bytes (the refill rows: steps of 8, 40 and 80
    units with carried bytes straddle the keystream refills at message bytes 4064 and 8160), nothing written past a box; then
    update_sealed_rows_dev over those boxes equals the Python-integer column sums"""
    from oracle import sealedbox_oracle as so
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    from test_participant_seal_gpu import _esk, _keys, check_against
    case = V.sealed_cases()[which]
    assert case.name == SEALED_CASES[which]
    rows, L = len(case.rows), case.L
    pk, sk = _keys(40 + which)
    esk = _esk(rows, which)
    stride = L + stride_pad
    d_vals, ptr = _values(case.rows, stride)
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    slot = codec.slot_size(L) + 48
    d_boxes, d_lens = _pattern(rows * slot + 32), _pattern(rows * 8 + 8)
    box.seal_share_rows_dev(codec, [pk], rows, ptr, rows, L, stride, d_boxes.ptr, slot, d_lens.ptr, esk)
    raw, lens = d_boxes.to_bytes(rows * slot), np.frombuffer(d_lens.to_bytes(rows * 8), dtype="<u8").copy()
    assert d_boxes.to_bytes(32, rows * slot) == bytes([BYTE]) * 32 and d_lens.to_bytes(8, rows * 8) == bytes([BYTE]) * 8
    want = [so.seal(case.enc[r], pk, esk[32 * r:32 * r + 32]) for r in range(rows)]
    check_against(raw, lens, slot, want, esk, case.name)
    comb = crypto.ShareCombiner(crypto.Additive(3, V.P62))
    d_status, d_ok = DeviceBytes(4).zero(), _pattern(4 * rows + 4)
    comb.begin_dev(1, L)
    comb.update_sealed_rows_dev(codec, box, pk, sk, d_boxes.ptr, slot, d_lens.ptr, rows, slot, d_status.ptr, d_ok.ptr)
    got = _finish(comb, 1, L)[0]
    assert d_status.to_bytes(4) == bytes(4) and (np.frombuffer(d_ok.to_bytes(4 * rows), dtype="<u4") == 1).all()
    assert d_ok.to_bytes(4, 4 * rows) == bytes([BYTE]) * 4
    exp = V.column_sums(case.rows, V.P62)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"column {bad[0]}: {got[bad[0]]}, expected {exp[bad[0]]}"

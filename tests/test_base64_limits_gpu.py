"""The base64 kernels (sda_amd/csrc/wire_kernels.hip) on the crafted rows of tests/base64_limits.py, through the C ABI.

Every expectation is the module's RFC 4648 reference (held against oracle.wire_oracle in tests/test_base64_limits_reach.py): the verdict
d_row_status != 0, d_out_bytes and the bytes of every valid row; the text of every encoded row, byte for byte.  The decoder is fed the
reference's text, never the encoder's output.  Outputs are 0xA5 / 0x5A before a call, slots are as tight as the entry points allow and
64 more bytes lie behind the last row: what a call leaves outside a row's bytes shows, a zero byte included.  The checks are
base64_limits.check_decode / check_encode - the functions the reach test proves to notice every planted fault of the model."""
import numpy as np
import pytest

import base64_limits as B

pytestmark = pytest.mark.gpu


class Buffers:
    """the device buffers of one decode call, filled as base64_limits expects them before the call"""

    def __init__(self, call, status0=0):
        from sda_amd.device import DeviceBytes
        self.call = call
        self.text = DeviceBytes.from_bytes(call.doc + bytes(-len(call.doc) % 4))       # the last dword of the last row is ours
        self.lens = DeviceBytes.from_bytes(np.array(call.lens, dtype="<u8").tobytes())
        self.offsets = None if call.offsets is None else DeviceBytes.from_bytes(np.array(call.offsets, dtype="<u8").tobytes())
        self.out = DeviceBytes.from_bytes(bytes([B.OUT_FILL]) * (call.rows * call.out_slot + B.SLACK))
        self.nb = DeviceBytes.from_bytes(np.full(call.rows, B.NB_SENTINEL, dtype="<u8").tobytes())
        self.status = DeviceBytes.from_bytes(np.array([status0], dtype="<u4").tobytes())
        self.rs = DeviceBytes(call.rows * 4).zero()
        assert self.text.ptr % 16 == 0 and self.out.ptr % 16 == 0

    def decode(self, row_status=True, **change):
        from sda_amd import crypto
        c = self.call
        a = dict(d_text=self.text.ptr, text_slot=c.text_slot, d_text_bytes=self.lens.ptr, rows=c.rows, max_chars=c.max_chars, d_out=self.out.ptr,
                 out_slot=c.out_slot, d_out_bytes=self.nb.ptr, d_status=self.status.ptr, d_row_status=self.rs.ptr if row_status else 0,
                 d_text_offsets=self.offsets.ptr if self.offsets else 0)
        a.update(change)
        crypto.base64_decode_rows_dev(**a)

    def read(self):
        c = self.call
        return (int(np.frombuffer(self.status.to_bytes(), dtype="<u4")[0]), np.frombuffer(self.rs.to_bytes(), dtype="<u4"),
                np.frombuffer(self.nb.to_bytes(), dtype="<u8"), self.out.to_bytes())

    def untouched(self):
        status, rs, nb, out = self.read()
        return not rs.any() and (nb == B.NB_SENTINEL).all() and out == bytes([B.OUT_FILL]) * len(out)


class EncodeBuffers:
    def __init__(self, call):
        from sda_amd.device import DeviceBytes
        self.call = call
        self.inp = DeviceBytes.from_bytes(call.blob)
        self.lens = DeviceBytes.from_bytes(np.array(call.lens, dtype="<u8").tobytes())
        self.text = DeviceBytes.from_bytes(bytes([B.TEXT_FILL]) * (call.rows * call.text_slot + B.SLACK))
        self.tb = DeviceBytes.from_bytes(np.full(call.rows, B.NB_SENTINEL, dtype="<u8").tobytes())
        assert self.inp.ptr % 16 == 0 and self.text.ptr % 16 == 0

    def encode(self, **change):
        from sda_amd import crypto
        c = self.call
        a = dict(d_in=self.inp.ptr + c.in_shift, in_slot=c.in_slot, d_in_bytes=self.lens.ptr, rows=c.rows, max_bytes=c.max_bytes,
                 d_text=self.text.ptr, text_slot=c.text_slot, d_text_bytes=self.tb.ptr)
        a.update(change)
        crypto.base64_encode_rows_dev(**a)

    def read(self):
        return np.frombuffer(self.tb.to_bytes(), dtype="<u8"), self.text.to_bytes()

    def untouched(self):
        tb, text = self.read()
        return (tb == B.NB_SENTINEL).all() and text == bytes([B.TEXT_FILL]) * len(text)


def _run(call, status0=0):
    buf = Buffers(call, status0)
    buf.decode()
    errs = B.check_decode(call, *buf.read(), status0=status0)
    assert not errs, "\n".join(errs)


# ---- the families ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["slots", "offsets"])
def test_alphabet(gpu, form):
    """every byte value 0..255 at each position of a quad, as the only quad, inside a full lane and as the last quad of three lanes:
    in slots, and by offsets into one document at each of the four alignments"""
    _run(B.alphabet_calls()[form == "offsets"])


@pytest.mark.parametrize("place", ["short", "long"])
def test_padding(gpu, place):
    """all 64^2 "XY==" and all 64^2 "QYZ=": alone and behind one full lane (short, with "====", "Z===", "Zg==Zg==", "Zm9v====" and
    '=' at each position of a non-last quad), and as the only quad of block 1 behind one full workgroup (long)"""
    _run(B.padding_short_call() if place == "short" else B.padding_long_call())


@pytest.mark.parametrize("index", range(3), ids=["offsets", "odd slot", "slot = 2 mod 4"])
def test_edges_decode(gpu, index):
    """text of every multiple of 4 up to 36 characters and of 4096 j - 4, 4096 j, 4096 j + 4, each ending in each padding form, at each
    alignment - by offsets (and at offsets 0..3 of the document itself) and by slots of 12293 and 12294 characters; short and long rows
    share a call"""
    _run(B.edges_calls()[index])


def test_planted(gpu):
    """one foreign character at 0, 15, 16, 4079, 4080, 4095, 4096, 4111 or the end of a row of three blocks, at each alignment, between
    valid neighbours: only the planted row is flagged, and the neighbours decode"""
    _run(B.planted_call())


def test_stores_decode(gpu):
    """payloads of 0..52 bytes and their malformed twins in odd slots, the output slot as tight as the entry point allows: bytes
    [nb, out_slot) of a valid row and everything past the first decoded_max(len) bytes of a malformed one stay 0xA5"""
    _run(B.stores_decode_call())


@pytest.mark.parametrize("index", range(2), ids=["0..52 bytes", "edges"])
def test_encode(gpu, index):
    """payloads of 0..52 bytes, and of every length around 3072 j (the text of the decoder's edges): in_slot a multiple of 4 and not of
    16, d_in 4 bytes behind the buffer, text compared byte for byte with the reference and [text_len, text_slot) left 0x5A"""
    call = B.encode_calls()[index]
    buf = EncodeBuffers(call)
    buf.encode()
    errs = B.check_encode(call, *buf.read())
    assert not errs, "\n".join(errs)


# ---- the status words -------------------------------------------------------------------------------------------------------------------
def _valid_rows_only(call):
    keep = [r for r in range(call.rows) if call.want[r] is not None]
    return B.DecodeCall(call.name + ", valid rows", call.doc, [call.lens[r] for r in keep], [call.names[r] for r in keep],
                        [call.want[r] for r in keep], offsets=[call.start(r) for r in keep])


def test_status_word_keeps_what_it_held(gpu):
    call = B.stores_decode_call()
    buf = Buffers(call, 0x4 | 0x10)
    buf.decode()
    assert buf.read()[0] == 0x1C                                        # malformed rows in the call: bit 8 joins what was there
    assert not B.check_decode(call, *buf.read(), status0=0x4 | 0x10)
    for preset in (0x4 | 0x10, 0):                                      # a clean call leaves it as it was
        clean = Buffers(_valid_rows_only(call), preset)
        clean.decode()
        assert clean.read()[0] == preset
        assert not B.check_decode(clean.call, *clean.read(), status0=preset)


def test_row_status_is_optional(gpu):
    for call in (B.stores_decode_call(), B.planted_call()):
        a, b = Buffers(call, 0x14), Buffers(call, 0x14)
        a.decode()
        b.decode(row_status=False)
        sa, rsa, nba, outa = a.read()
        sb, rsb, nbb, outb = b.read()
        assert sa == sb == 0x1C and not rsb.any() and rsa.any()
        assert (nba == nbb).all() and outa == outb
        assert not B.check_decode(call, sa, rsa, nba, outa, status0=0x14)


# ---- the argument checks ----------------------------------------------------------------------------------------------------------------
def _refused(fn, message, **change):
    from sda_amd import capi
    with pytest.raises(capi.SdaError) as e:
        fn(**change)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and e.value.message == message, (change, e.value.message)


def test_decode_argument_checks(gpu):
    call = B.stores_decode_call()
    buf = Buffers(call, 0x14)
    slot_msg = "output rows must be 4-byte aligned (buffer and out_slot)"
    _refused(buf.decode, slot_msg, out_slot=call.out_slot + 1)
    _refused(buf.decode, slot_msg, out_slot=call.out_slot + 2)
    _refused(buf.decode, slot_msg, d_out=buf.out.ptr + 2)
    _refused(buf.decode, "out_slot < 3/4 of max_chars", out_slot=call.out_slot - 4)
    _refused(buf.decode, "out_slot < 3/4 of max_chars", max_chars=call.max_chars + 4)          # 57 > 56
    _refused(buf.decode, "text_slot < max_chars", text_slot=call.max_chars - 1)
    _refused(buf.decode, "text_slot < max_chars", text_slot=0)
    for name in ("d_text", "d_text_bytes", "d_out", "d_out_bytes", "d_status"):
        _refused(buf.decode, "NULL device pointer", **{name: 0})
    assert buf.untouched() and buf.read()[0] == 0x14
    buf.decode(rows=0)                                                   # OK, and nothing touched
    buf.decode(rows=0, d_text=0, d_out=0, out_slot=3)
    assert buf.untouched() and buf.read()[0] == 0x14
    # with offsets text_slot is not looked at: the same rows by offsets and a text_slot of 0 decode
    by_offsets = B.DecodeCall(call.name + " by offsets", call.doc, call.lens, call.names, call.want, offsets=[call.start(r) for r in range(call.rows)])
    _run(by_offsets, status0=0x14)
    buf.decode()                                                         # and the buffers the refusals left alone still serve
    assert not B.check_decode(call, *buf.read(), status0=0x14)


def test_encode_argument_checks(gpu):
    call = B.encode_calls()[0]
    buf = EncodeBuffers(call)
    in_msg = "input rows must be 4-byte aligned (buffer and in_slot)"
    text_msg = "text rows must be 16-byte aligned (buffer and text_slot)"
    _refused(buf.encode, in_msg, in_slot=call.in_slot + 2)
    _refused(buf.encode, in_msg, in_slot=call.in_slot + 1)
    _refused(buf.encode, in_msg, d_in=buf.inp.ptr + 2)
    _refused(buf.encode, text_msg, text_slot=call.text_slot + 8)
    _refused(buf.encode, text_msg, text_slot=call.text_slot + 4)
    _refused(buf.encode, text_msg, d_text=buf.text.ptr + 4)
    _refused(buf.encode, text_msg, d_text=buf.text.ptr + 8)
    _refused(buf.encode, "text_slot < sda_base64_encoded_size(max_bytes)", text_slot=call.text_slot - 16)
    for name in ("d_in", "d_in_bytes", "d_text", "d_text_bytes"):
        _refused(buf.encode, "NULL device pointer", **{name: 0})
    assert buf.untouched()
    buf.encode(rows=0)
    buf.encode(rows=0, d_in=0, d_text=0, text_slot=3)
    assert buf.untouched()
    buf.encode()
    assert not B.check_encode(call, *buf.read())

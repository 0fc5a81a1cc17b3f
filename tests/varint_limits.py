"""Crafted inputs and a geometry model for the wire codec kernels (sda_amd/csrc/varint_kernels.hip): no GPU, no library.

The codec is cursor arithmetic on data-dependent byte positions; random rows do not show which boundary a value crossed.  Here
every case is built by hand so that a value of a chosen length lies on a chosen boundary with a chosen split, the bytes are
written by a reference encoder on Python integers, and the model functions below say - from POSITIONS only - which named events
a case reaches in which kernel form.  tests/test_varint_limits_reach.py asserts per form that the cases
tests/test_varint_limits_gpu.py feeds it reach the form's whole list.

Not reachable at a size a test can afford, and therefore in no list: the second pass of scan_totals_kernel's loop (more than
1024 scan chunks = more than 2^20 blocks: 4 GiB of wire bytes) and the launch-size refusals of the launchers (2^32 work-items).

Event names
  len.x=K                     varint_len's division input (bit length of the zig-zag word + 6), K in 7..70
  lenk.* / write.* / encscan.* the scan encode's pair walk, copy-out and u32->u64 scan
  scan.lane|halo ...          the scan decode: a value across a 16-byte lane boundary / the 4096-byte block boundary (halo)
  stream.lane|chunk|group ... the stream decode: across a lane, a 1024-byte chunk (lane 63 -> halo carry), a 4-chunk group
  ... n=N s=S                 a value of N bytes with S bytes before the boundary
  stream.row ...              start / end phase of a row on the 16-byte grid, chunks per row, rows ending on / one past a chunk
  enc.*                       the streaming encoder: carried bytes, byte phase of tile_or, units per step, second store
  seal.refill=R units=U       a step of U units with cb != 0 straddling the keystream refill at message byte R"""
import functools

import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
P62 = 4611686006577364993

# ---- geometry, restated by hand ---------------------------------------------------------------------------------------------
ENC_BLOCK_VALUES = 2048     # kVT * kVals: values per workgroup of varint_len_kernel / varint_write_kernel
DEC_BLOCK_BYTES = 4096      # kVT * kBytes: bytes per workgroup of varint_count_kernel / varint_decode_kernel
LANE_BYTES = 16             # kBytes: bytes per lane (both decode forms)
HALO_BYTES = 16             # the 16 bytes in front of the tile (varint_decode_kernel's `tile`, kStreamTile)
CHUNK_BYTES = 1024          # 64 lanes x 16 B of RowStreamT, on the 16-byte grid at or below the row start (base0)
GROUP_CHUNKS = 4            # kStreamDepth
ENC_STEP_VALUES = 128       # kEncVals
UNIT_BYTES = 16             # the streaming encoder's store unit (uint4)
SCAN_CHUNK = 1024           # entries per workgroup of scan_chunks_kernel / scan_add_kernel
KS_FIRST_REFILL = 4064      # EncXSalsa: 64 blocks of 64 bytes less the 32 bytes of the Poly1305 key
KS_REFILL_PERIOD = 4096     # ... and every 64 blocks after
PAIR_STRIDE = 512           # varint_len_kernel: 2 * kVT values between a lane's pairs


# ---- reference codec on Python integers ------------------------------------------------------------------------------------
def zigzag(v):
    return ((v << 1) ^ (v >> 63)) & M64


def unzigzag(zz):
    return (zz >> 1) ^ -(zz & 1)


def encode_word(zz):
    out = bytearray()
    while zz >= 0x80:
        out.append(0x80 | (zz & 0x7F))
        zz >>= 7
    out.append(zz)
    return bytes(out)


def encode(values):
    return b"".join(encode_word(zigzag(int(v))) for v in values)


def decode(raw):
    """values of a well-formed row; bits above the 64th are dropped as integer-encoding does"""
    out, zz, shift = [], 0, 0
    for b in raw:
        zz |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            out.append(unzigzag(zz & M64))
            zz, shift = 0, 0
    assert shift == 0, "the row ends inside a value"
    return out


def length_of(v):
    return len(encode_word(zigzag(int(v))))


def _length_edges():
    words = []
    for b in range(65):
        lo, hi = (0, 0) if b == 0 else (1 << (b - 1), (1 << b) - 1)
        words += [lo, hi]
    return [unzigzag(w) for w in words] + [I64_MAX]


LENGTH_EDGES = _length_edges()          # smallest and largest zig-zag word of every bit length 0..64, as i64; and 2^63 - 1


def word_of_len(n, k=0):
    """a zig-zag word that takes n bytes, varied with k (k = 0: the smallest, k = 1: the largest)"""
    lo = 0 if n == 1 else 1 << (7 * (n - 1))
    hi = min(1 << (7 * n), 1 << 64) - 1
    if k == 0:
        return lo
    if k == 1:
        return hi
    return lo + (k * 0x9E3779B97F4A7C15) % (hi - lo + 1)


def value_of_len(n, k=0):
    return unzigzag(word_of_len(n, k))


def values_of_lens(lens, salt=0):
    return [value_of_len(n, salt + i) for i, n in enumerate(lens)]


def lens_for_bytes(L, nbytes):
    """L value lengths (1..10) that add up to nbytes, the long ones first"""
    assert L <= nbytes <= 10 * L, (L, nbytes)
    extra, lens = nbytes - L, []
    for _ in range(L):
        add = min(9, extra)
        lens.append(1 + add)
        extra -= add
    return lens


class Case:
    """rows of values (equal length) with their hand-built bytes; `claims`: the events the builder placed on purpose"""

    def __init__(self, name, rows, claims=(), enc=None):
        self.name, self.rows, self.claims = name, rows, set(claims)
        self.L = len(rows[0])
        assert all(len(r) == self.L for r in rows), name
        self.enc = [encode(r) for r in rows] if enc is None else enc

    @property
    def raw(self):
        return b"".join(self.enc)

    @property
    def offsets(self):
        return [0] + list(np.cumsum([len(e) for e in self.enc]))

    def matrix(self):
        return np.array(self.rows, dtype=np.int64).reshape(len(self.rows), self.L)


# ---- bit tricks restated with explicit masks -----------------------------------------------------------------------------------
def div7_trick(x):
    return ((x * 37) & M32) >> 8


def varint_len_trick(zz):
    x = (zz | 1).bit_length() + 6                               # 64 - clz(zz | 1) + 6
    return div7_trick(x)


def alignbyte(hi, lo, sh):
    return (((hi << 32) | lo) >> (8 * sh)) & M32


def _words(raw):
    raw = bytes(raw) + b"\0" * (-len(raw) % 4)
    return [int.from_bytes(raw[i:i + 4], "little") for i in range(0, len(raw), 4)]


def _unzz64(x):
    v = ((x >> 1) ^ (-(x & 1) & M64)) & M64
    return v - (1 << 64) if v >> 63 else v


def scan_squeeze(tile, start, nb):
    """varint_decode_kernel's assembly of one value: tile = bytes, start = coordinate of its first byte, nb = 1..10"""
    t = _words(tile)[start >> 2:]
    sh = start & 3
    d0, d1, d2 = alignbyte(t[1], t[0], sh), alignbyte(t[2], t[1], sh), alignbyte(t[3], t[2], sh)
    x = (d1 << 32) | d0
    if nb < 8:
        x &= (1 << (8 * nb)) - 1
    x &= 0x7F7F7F7F7F7F7F7F
    x = ((x & 0x7F007F007F007F00) >> 1) | (x & 0x007F007F007F007F)
    x = ((x & 0x3FFF00003FFF0000) >> 2) | (x & 0x00003FFF00003FFF)
    x = ((x & 0x0FFFFFFF00000000) >> 4) | (x & 0x000000000FFFFFFF)
    if nb > 8:
        x |= ((d2 & 0x7F) << 56) & M64
    if nb > 9:
        x |= (((d2 >> 8) & 0x7F) << 63) & M64
    return _unzz64(x)


def tile_value(tile, start, nb):
    """tile_value of the streaming decoder"""
    t = _words(tile)[start >> 2:]
    sh = start & 3
    d0, d1, d2 = alignbyte(t[1], t[0], sh), alignbyte(t[2], t[1], sh), alignbyte(t[3], t[2], sh)
    d0 = (d0 & 0x007F007F) | ((d0 >> 1) & 0x3F803F80)
    d1 = (d1 & 0x007F007F) | ((d1 >> 1) & 0x3F803F80)
    d0 = (d0 & 0x00003FFF) | ((d0 >> 2) & 0x0FFFC000)
    d1 = (d1 & 0x00003FFF) | ((d1 >> 2) & 0x0FFFC000)
    x = d0 | (d1 << 28)
    keep = 7 * min(nb, 8)
    x = ((x << (64 - keep)) & M64) >> (64 - keep)
    top = (d2 & 0x7F if nb > 8 else 0) | ((d2 & 0x100) >> 1 if nb > 9 else 0)
    x |= (top << 56) & M64
    return _unzz64(x)


def value_bytes(zz, n):
    d0, d1 = zz & 0x0FFFFFFF, (zz >> 28) & 0x0FFFFFFF
    d0 = (d0 & 0x00003FFF) | ((d0 & 0x0FFFC000) << 2)
    d1 = (d1 & 0x00003FFF) | ((d1 & 0x0FFFC000) << 2)
    d0 = (d0 & 0x007F007F) | ((d0 & 0x3F803F80) << 1)
    d1 = (d1 & 0x007F007F) | ((d1 & 0x3F803F80) << 1)
    d2 = ((zz >> 56) & 0x7F) | ((zz >> 63) << 8)
    cont = 0x8080808080808080 if n >= 9 else 0x0080808080808080 >> (8 * ((8 - n) & 7))
    b0, b1, b2 = d0 | (cont & M32), d1 | (cont >> 32), d2 | (0x80 if n > 9 else 0)
    return (0, 0, 0) if n == 0 else (b0, b1, b2)


def tile_or(tile32, pos, b0, b1, b2):
    sh = 8 * (pos & 3)
    lo = (((b1 << 32) | b0) << sh) & M64
    hi = (((b2 << 32) | b1) << sh) & M64
    t = pos >> 2
    tile32[t] |= lo & M32
    tile32[t + 1] |= lo >> 32
    tile32[t + 2] |= hi >> 32
    if sh:
        tile32[t + 3] |= (((b2 << sh) & M64) >> 32)


def cont_bits16(raw16):
    r = 0
    for k, w in enumerate(_words(raw16)):
        r |= (((((w & 0x80808080) >> 7) * 0x10204080) & M32) >> 28) << (4 * k)
    return r


# ---- layout of a byte row: (first byte, terminator) of every value -----------------------------------------------------------
def spans(raw):
    out, f = [], 0
    for i, b in enumerate(raw):
        if not b & 0x80:
            out.append((f, i))
            f = i + 1
    return out


def _boundary_events(prefix, kind, period, f, e, prev_n, origin=0):
    """events of one value [f, e] against the boundaries origin + k * period (k >= 1)"""
    ev = set()
    n = e - f + 1
    rf, re = f - origin, e - origin
    if rf // period != re // period and n <= 10:
        ev.add(f"{prefix}.{kind} n={n} s={(re // period) * period - rf}")
    if n == 10 and re % period == period - 1:
        ev.add(f"{prefix}.{kind} term=last n=10")
    if n == 10 and rf % period == 0 and rf > 0:
        ev.add(f"{prefix}.{kind} start=first n=10")
    if n == 1 and rf % period == 0 and rf > 0 and prev_n == 10:
        ev.add(f"{prefix}.{kind} term=first after n=10")
    return ev


def scan_decode_events(raw, base=0):
    """the three-pass decode of a stream whose first byte sits at address `base` (mod 16): its grid is the STREAM's"""
    ev, prev_n = set(), 0
    for f, e in spans(raw):
        ev |= _boundary_events("scan", "lane", LANE_BYTES, f, e, prev_n)
        ev |= _boundary_events("scan", "halo", DEC_BLOCK_BYTES, f, e, prev_n)
        prev_n = e - f + 1
    return ev | scan_size_events(len(raw), base)


def scan_size_events(n, base=0):
    """what the SIZE of a stream reaches in the scan decode: ragged tail, base alignment, the u32 -> u64 scan's chunks"""
    ev = set()
    ev.add(f"scan.tail={n % 16}")
    ev.add(f"scan.base={base % 16}")
    blocks = -(-n // DEC_BLOCK_BYTES)
    if n >= DEC_BLOCK_BYTES * SCAN_CHUNK - 1:
        ev.add(f"scan.dec bytes=4096*1024{n - DEC_BLOCK_BYTES * SCAN_CHUNK:+d}")
        ev.add(f"scan.chunks={-(-(blocks + 1) // SCAN_CHUNK)}")
        if n % DEC_BLOCK_BYTES == 0:
            ev.add(f"scan.zero_entry={blocks}")
    return ev


def stream_decode_events(enc_rows, starts, base=0, before=None):
    """one wave per row: enc_rows[r] lies at address base + starts[r]; chunks are laid from base0 = that address & ~15"""
    ev = set()
    for r, (row, a) in enumerate(zip(enc_rows, starts)):
        addr = base + a
        base0 = addr & ~15
        end = addr + len(row)
        ev.add(f"stream.row a={addr % 16}")
        ev.add(f"stream.row b={end % 16}")
        chunks = -(-(end - base0) // CHUNK_BYTES)
        if chunks in (1, 4, 5):
            ev.add(f"stream.row chunks={chunks}")
        if (end - base0) % CHUNK_BYTES == 0:
            ev.add("stream.row ends on a chunk")
        if (end - base0) % CHUNK_BYTES == 1 and end - base0 > 1:
            ev.add("stream.row ends one past a chunk")
        if len(row) == 1:
            ev.add("stream.row single byte")
        prev_n = 0
        for f, e in spans(row):
            n = e - f + 1
            if f == 0 and n == 10:
                ev.add("stream.row first n=10" + (" after 0xff" if before and before[r] else ""))
            ev |= _boundary_events("stream", "lane", LANE_BYTES, addr + f, addr + e, prev_n, base0)
            ev |= _boundary_events("stream", "chunk", CHUNK_BYTES, addr + f, addr + e, prev_n, base0)
            ev |= _boundary_events("stream", "group", CHUNK_BYTES * GROUP_CHUNKS, addr + f, addr + e, prev_n, base0)
            prev_n = n
    return ev


def length_events(rows):
    return {f"len.x={(zigzag(int(v)) | 1).bit_length() + 6}" for row in rows for v in row}


def stream_encode_events(rows, row_addr_mod16=(0,), refills=False):
    """encode_row: 128 values per step, the bytes that do not fill a unit carried; row_addr_mod16[r % len]: alignment of row r"""
    ev = set()
    for r, row in enumerate(rows):
        L = len(row)
        if L % ENC_STEP_VALUES in (0, 1, 127):
            ev.add(f"enc.len%128={L % ENC_STEP_VALUES}")
        if L & 1:
            ev.add("enc.len odd")
        steps = -(-L // ENC_STEP_VALUES)
        if steps in (1, 4, 5):
            ev.add(f"enc.steps={steps}")
        ev.add(f"enc.base={16 if row_addr_mod16[r % len(row_addr_mod16)] == 0 else 8}")
        cur, cb = 0, 0
        for j in range(steps):
            lens = [length_of(v) for v in row[j * ENC_STEP_VALUES:(j + 1) * ENC_STEP_VALUES]]
            pos = cb
            for n in lens:
                ev.add(f"enc.phase={pos & 3} n={n}")
                pos += n
            have = pos
            units = have >> 4
            full = len(lens) == ENC_STEP_VALUES
            if full and set(lens) == {1}:
                ev.add(f"enc.units={units} of 1-byte values")
            if full and set(lens) == {10} and cb == 15:
                ev.add(f"enc.units={units} of 10-byte values, cb=15")
            if units > 64:
                ev.add("enc.second store")
            if have and have % 16 == 0:
                ev.add("enc.have%16=0")
            if refills and cb:
                for R in (KS_FIRST_REFILL, KS_FIRST_REFILL + KS_REFILL_PERIOD):
                    if cur < R < cur + 16 * units and units in (8, 40, 80):
                        ev.add(f"seal.refill={R} units={units}")
            cur += 16 * units
            cb = have & 15
            ev.add(f"enc.cb={cb}")
    return ev


def scan_encode_events(rows, L, stride, base8=False, out_offsets=(0, 1, 2, 3), byte_lens=None):
    """varint_len_kernel's pair walk and varint_write_kernel's copy-out; byte_lens: per-value byte lengths, row-major"""
    ev = set()
    N = rows * L
    vec = stride % 2 == 0 and not base8
    ev.add("lenk.vector" if vec else ("lenk.scalar, base offset of 8 bytes" if base8 else "lenk.scalar, odd stride"))
    blocks = -(-N // ENC_BLOCK_VALUES)
    if blocks > 1:
        ev.add("lenk.blocks>1")
    if 2 * L <= PAIR_STRIDE:                                   # i += 512 passes more than one row end
        ev.add("lenk.several rows per step")
    if L & 1 and rows > 1:                                      # a pair (g, g + 1) with g even whose first element ends a row
        ev.add("lenk.pair takes the next row's first element" + (", vector" if vec else ", scalar"))
    if L in (1, 2, 3, 511, 512, 513, 2047, 2048, 2049):
        ev.add(f"lenk.len={L}")
    if blocks > SCAN_CHUNK:
        ev.add(f"encscan.chunks={-(-blocks // SCAN_CHUNK)}")
    if byte_lens is not None:
        boff = np.concatenate([[0], np.cumsum(np.add.reduceat(np.asarray(byte_lens), np.arange(0, N, ENC_BLOCK_VALUES)))])
        for b in range(1, blocks):
            ev.add(f"write.boff%4={int(boff[b]) % 4}")
        last = int(boff[blocks] - boff[blocks - 1])
        for o in out_offsets:
            for b in range(blocks):
                ev.add(f"write.head={(4 - (o + int(boff[b])) % 4) % 4}")
            if last < (4 - (o + int(boff[blocks - 1])) % 4) % 4:
                ev.add("write.last block shorter than its head")
    return ev


# ---- builders ---------------------------------------------------------------------------------------------------------------------
STRADDLES = [(n, s) for n in range(2, 11) for s in range(1, n)]          # 45


@functools.lru_cache(maxsize=None)
def straddle_stream(period, first):
    """one row: 1-byte fillers, and on consecutive boundaries first + k * period a value of n bytes with s bytes before the
    boundary, for every (n, s); then (two boundaries on) a 10-byte value whose terminator is the last byte before a boundary with
    a 10-byte value starting on the boundary, and a 10-byte value ending before a boundary with a 1-byte value on it"""
    lens, claims, pos, B = [], set(), 0, first

    def put(at, n):
        nonlocal pos
        assert at >= pos, (period, first, at, pos)
        lens.extend([1] * (at - pos))
        lens.append(n)
        pos = at + n
    for n, s in STRADDLES:
        put(B - s, n)
        claims.add(f"n={n} s={s}")
        B += period
    B += period
    put(B - 10, 10)
    put(B, 10)
    claims |= {"term=last n=10", "start=first n=10"}
    B += 2 * period
    put(B - 10, 10)
    put(B, 1)
    claims.add("term=first after n=10")
    lens.extend([1] * 5)
    return Case(f"straddle {period}/{first}", [values_of_lens(lens, salt=period)], claims)


@functools.lru_cache(maxsize=None)
def phased_rows():
    """four groups of rows (one expected length each)"""
    phases = []
    for r in range(18):                                         # 33 bytes each: back to back they start at every a % 16
        lens = [10] + lens_for_bytes(23, 23) if r == 0 else lens_for_bytes(24, 33)
        lens = lens if r == 0 else lens[::-1] if r & 1 else lens
        phases.append(values_of_lens(lens, salt=100 * r))
    assert all(len(encode(r)) == 33 for r in phases)
    chunks = [values_of_lens(lens_for_bytes(600, nb)[::(1 if i & 1 else -1)], salt=1000 * i)
              for i, nb in enumerate((600, 4088, 4097, 3500, 4096, 1024, 1025))]
    single = [[5], [I64_MAX], [-1], [I64_MIN]]
    ends = [values_of_lens(lens_for_bytes(24, 40 + k)[::(1 if k & 1 else -1)], salt=77 * k) for k in range(16)]     # every b % 16 from a slot start
    return (Case("phases", phases, {"stream.row first n=10"}), Case("chunks", chunks), Case("single", single, {"stream.row single byte"}),
            Case("ends", ends))


def _step(lens_):
    assert len(lens_) == ENC_STEP_VALUES
    return list(lens_)


def _phased_lens(n, count):
    """`count` value lengths in which a value of n bytes lands on every byte phase in turn (the phase of a value in the encoder's
    tile is its byte offset in the row & 3: every step starts on a multiple of 16 less the carried bytes)"""
    lens, pos, want = [], 0, 0
    while len(lens) < count:
        if pos & 3 == want or len(lens) + 1 == count:
            lens.append(n)
            pos += n
            want = (want + 1) & 3
        else:
            lens.append(1)
            pos += 1
    return lens


@functools.lru_cache(maxsize=None)
def encode_steps():
    """rows for the streaming encoder, as groups of equal length"""
    one, ten = [1] * 128, [10] * 128
    groups = []
    # 4 steps + 1 value (5 steps, len % 128 == 1, odd)
    a = []
    for k in range(4):
        a += _step([2] * (k + 1) + [1] * (127 - k))             # 129 + k bytes
    b = _step([9] + [10] * 127) + _step(ten) + _step(ten) + _step(one)      # cb = 15, then two steps of 80 units with cb = 15
    groups.append(("4 steps + 1", [a + [1], b + [10]]))
    # every length at every byte phase (the carried byte counts these rows leave take every value 0..15): 4 steps, len % 128 == 0
    rows = [_phased_lens(n, 512) for n in range(1, 11)]
    rows.append(_step(one) * 4)                                 # 8 units a step, have % 16 == 0
    groups.append(("4 steps", rows))
    # one step: len = 127 (odd, len % 128 == 127) and len = 128
    groups.append(("127 values", [[1 + (i * 7 + r) % 10 for i in range(127)] for r in range(5)]))
    groups.append(("128 values", [ten, one, [1 + i % 10 for i in range(128)], [10 - i % 10 for i in range(128)], [3] * 128]))
    return tuple(Case(name, [values_of_lens(l, salt=31 * i) for i, l in enumerate(rows)]) for name, rows in groups)


@functools.lru_cache(maxsize=None)
def seal_rows():
    """three rows of 8449 values: steps of 8, 40 and 80 units with carried bytes across the refills at 4064 and 8160"""
    L = 66 * 128 + 1
    rows = []
    for w, steps in ((1, 66), (5, 14), (10, 8)):
        first = [w + 1 if w == 1 else w - 1] + [w] * 127
        lens = first + [w] * 128 * (steps - 1)
        lens += [1] * (L - len(lens))
        rows.append(values_of_lens(lens, salt=w))
    return Case("refills", rows, {f"seal.refill={R} units={u}" for R in (4064, 8160) for u in (8, 40, 80)})


SCAN_ENCODE_SHAPES = [   # rows, len, stride, base offset of 8 bytes, value lengths cycle
    (2049, 1, 1, False, (1, 2)), (1025, 2, 2, False, (3,)), (700, 3, 3, False, (1, 1, 2)), (683, 3, 4, True, (10, 9, 1)),
    (5, 511, 511, False, (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)), (5, 512, 512, False, (2, 3, 1)), (4, 513, 514, False, (2, 1, 1)),
    (3, 2047, 2048, True, (1, 1, 1, 2)), (2, 2048, 2048, False, (5,)), (2, 2049, 2049, False, (7, 1)), (3, 2049, 2050, False, (10,))]
# (the first shape ends in a block of a single byte: shorter than its head at three of the four destination alignments)


def scan_encode_case(shape):
    rows, L, stride, base8, cyc = shape
    lens = [cyc[i % len(cyc)] for i in range(rows * L)]
    vals = values_of_lens(lens, salt=L)
    return Case(f"{rows}x{L} stride {stride}" + (" +8" if base8 else ""), [vals[r * L:(r + 1) * L] for r in range(rows)])


@functools.lru_cache(maxsize=None)
def scan_encode_shapes():
    return tuple((s, scan_encode_case(s)) for s in SCAN_ENCODE_SHAPES)


def fixed_length_bytes(words, n):
    """encoding of zig-zag words that all take n bytes, [len(words)][n] uint8"""
    w = np.asarray(words, dtype=np.uint64)
    out = np.empty((w.size, n), dtype=np.uint8)
    for k in range(n):
        out[:, k] = ((w >> np.uint64(7 * k)) & np.uint64(0x7F)).astype(np.uint8) | np.uint8(0x80 if k + 1 < n else 0)
    return out


def _unzigzag_np(w):
    return ((w >> np.uint64(1)) ^ (np.uint64(0) - (w & np.uint64(1)))).astype(np.int64)


@functools.lru_cache(maxsize=None)
def big_encode_case():
    """2048 * 1024 + 1 one-byte values: 1025 blocks, the smallest shape with a second scan chunk -> (values, bytes)"""
    n = ENC_BLOCK_VALUES * SCAN_CHUNK + 1
    words = (np.arange(n, dtype=np.uint64) * np.uint64(37)) % np.uint64(128)
    return _unzigzag_np(words), fixed_length_bytes(words, 1).tobytes()


@functools.lru_cache(maxsize=None)
def big_decode_case(delta):
    """a stream of 4096 * 1024 + delta bytes: one value of 4 + delta bytes, then ten-byte values that differ -> (values, bytes)"""
    n_bytes = DEC_BLOCK_BYTES * SCAN_CHUNK + delta
    head = 4 + delta
    k = (n_bytes - head) // 10
    assert head + 10 * k == n_bytes
    words = (np.uint64(1) << np.uint64(63)) | (np.arange(k, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(1))
    vals = np.concatenate([[value_of_len(head, 5)], _unzigzag_np(words)]).astype(np.int64)
    return vals, encode_word(word_of_len(head, 5)) + fixed_length_bytes(words, 10).tobytes()


def short_stream(n_bytes):
    """n_bytes of values of mixed lengths (the scan decode's ragged tail: n_bytes % 16)"""
    lens, left, k = [], n_bytes, 0
    while left:
        n = min(1 + (k * 7) % 10, left)
        lens.append(n)
        left -= n
        k += 1
    return Case(f"{n_bytes} bytes", [values_of_lens(lens, salt=n_bytes)])


TAIL_SIZES = tuple(range(4096 + 160, 4096 + 176))               # n_bytes % 16 = 0..15, two blocks
BASE_OFFSETS = tuple(range(1, 16))


class Damage:
    def __init__(self, name, raw, offsets, L, bit, events, values=None):
        self.name, self.raw, self.offsets, self.L, self.bit, self.events, self.values = name, raw, offsets, L, bit, set(events), values
        self.rows = len(offsets) - 1


UNTERMINATED, ROW_COUNT, MALFORMED = 4, 2, 1
DAMAGE_BOUNDARIES = {"lane": 16 * 5, "chunk": CHUNK_BYTES, "block": DEC_BLOCK_BYTES}     # block = the stream form's group too


def _run(kind, split, cont, last=0x01):
    """fillers, then `cont` continuation bytes and a terminator with `split` of them before the boundary, then fillers"""
    B = DAMAGE_BOUNDARIES[kind]
    raw = encode(values_of_lens([1] * (B - split), salt=split)) + bytes(0x80 | ((7 * i + split) & 0x7F) for i in range(cont)) + bytes([last])
    return raw + encode(values_of_lens([1] * 7, salt=3))


@functools.lru_cache(maxsize=None)
def damage_cases():
    out = []
    good = Case("three rows", [values_of_lens([1 + (i + r) % 10 for i in range(40)], salt=r) for r in range(3)])
    for r in (1, 2):
        enc = [bytearray(e) for e in good.enc]
        enc[r][-1] |= 0x80
        out.append(Damage(f"row {r} of 3 ends inside a value", b"".join(bytes(e) for e in enc), good.offsets, 40, UNTERMINATED,
                          {f"dmg.unterminated row={r}"}))
    for d in (1, -1):
        out.append(Damage(f"expected length {d:+d}", good.raw, good.offsets, 40 + d, ROW_COUNT, {f"dmg.count{d:+d}"}))
    for kind in DAMAGE_BOUNDARIES:
        for s in range(1, 11):
            raw = _run(kind, s, 11)
            out.append(Damage(f"11 continuation bytes, {s} before a {kind} boundary", raw, [0, len(raw)], len(spans(raw)), MALFORMED,
                              {f"dmg.run11 {kind} s={s}"}))
            raw = _run(kind, s, 9)
            out.append(Damage(f"10 bytes, {s} before a {kind} boundary", raw, [0, len(raw)], len(spans(raw)), 0,
                              {f"legal.run10 {kind} s={s}"}, decode(raw)))
    for k, cont in ((1, 17), (15, 31), (6, 40)):                # the terminator at lane byte k with an empty 32-byte window before it
        raw = encode(values_of_lens([1] * (64 + k - cont), salt=k)) + bytes([0x80 | i for i in range(cont)]) + b"\x01" + encode([3, -4])
        assert spans(raw)[-3][1] % 16 == k
        out.append(Damage(f"{cont} continuation bytes", raw, [0, len(raw)], len(spans(raw)), MALFORMED, {f"dmg.window empty k={k}"}))
    raw = encode([9, -9]) + b"\xff" * 9 + b"\x7f" + encode([1])
    out.append(Damage("ff x 9, 7f: the bits above the 64th are dropped", raw, [0, len(raw)], 4, 0, {"legal.ff9 7f"}, decode(raw)))
    return tuple(out)


def column_sums(rows, q):
    L = len(rows[0])
    return np.array([sum(int(row[c]) for row in rows) % q for c in range(L)], dtype=np.int64)


def three_jobs(rows):
    """job j = the rows and row j once more (job-major): the three sums differ"""
    return [rows + [rows[j % len(rows)]] for j in range(3)]


# ---- which cases the GPU file feeds to which form: ONE list per form, read by the GPU file and by the reach test -------------------
def edges_case():
    return Case("LENGTH_EDGES", [list(LENGTH_EDGES)])


OFF_GRID_BLOCK_BASES = (5, 11)                                  # the 4096-byte straddles again with the stream off the 16-byte grid


def scan_boundary_sizes():
    """the sizes at which the u32 -> u64 scan and the ragged loads change: the 1025-block encode shape, decode streams of
    4096 * 1024 - 1 / + 0 / + 1 bytes (as functions: they are 4 MiB each), short streams with n_bytes % 16 = 0..15, and the base
    offsets 1..15 of a stream (applied to the `phases` rows, and two of them to the 4096-byte straddles)"""
    return {"encode": big_encode_case, "decode": {d: functools.partial(big_decode_case, d) for d in (-1, 0, 1)},
            "tails": [short_stream(n) for n in TAIL_SIZES], "bases": BASE_OFFSETS, "block bases": OFF_GRID_BLOCK_BASES}


def decode_stream_cases():
    """single-row and back-to-back streams for decode_dev and update_encoded_dev: (case, base offsets)"""
    p = phased_rows()
    return [(straddle_stream(16, 16), (0,)), (straddle_stream(1024, 1024), (0,)), (straddle_stream(4096, 4096), (0,) + OFF_GRID_BLOCK_BASES),
            (p[0], (0,) + BASE_OFFSETS), (p[1], (0,)), (p[2], (0,)), (p[3], (0,))]


def slotted_decode_cases():
    p = phased_rows()
    return [straddle_stream(1024, 1024), straddle_stream(4096, 4096)] + list(p)


def stream_encode_cases():
    return list(encode_steps()) + [seal_rows(), edges_case()]


def sealed_cases():
    return stream_encode_cases() + [straddle_stream(1024, 1024), straddle_stream(4096, 4096)] + list(phased_rows())


EDGES_ENCODE_LAYOUTS = ((131, False), (132, True))    # (stride, base offset of 8 bytes) of LENGTH_EDGES in the scan-encode test
ENCODE_STRIDE_PADS = (0, 1, 2)          # row stride = len + pad in the streaming-encoder test
SEALED_STRIDE_PADS = (0, 1)             # ... and in the sealed test


def row_alignments(rows, L, pad):
    """address mod 16 of every row of a [rows][L + pad] i64 matrix that starts on the 16-byte grid"""
    return tuple((r * (L + pad) * 8) % 16 for r in range(rows))

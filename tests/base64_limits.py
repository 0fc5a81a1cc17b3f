"""Crafted rows, a reference and a switchable model for the base64 kernels (sda_amd/csrc/wire_kernels.hip): no GPU, no library.

Base64 text is network input: lengths, offsets into a JSON document and every character.  Random round trips show none of the
places where `base64_decode_rows_kernel` can be wrong, so every row here is built by hand:

  reference   `ref_decode` / `ref_encode`: RFC 4648 section 4 restated on Python integers with a plain 64-entry table.  A row is valid
              iff its length is a multiple of 4, every character is in the alphabet except '=' as the last one or two characters of
              the last quad, and the bits under the padding are zero.  It is the expected value of EVERY case; nothing is expected
              from the kernels' own round trip.  tests/test_base64_limits_reach.py holds it against oracle.wire_oracle on every row.
              (The 2 x 4096 PADDING rows behind one full workgroup share their first 4096 characters: their expectation is
              ref_decode(prefix) + ref_decode(last quad) - the RFC decodes quad by quad and only the last quad can be padded -
              and the reach test holds ALL of them against the oracle as whole rows and every 16th against ref_decode as a whole row.)
  geometry    `decode_labels` / `encode_labels`: from POSITIONS only, what a call reaches - decode: the lane of 16 characters, its
              misalignment `mis`, its quads `nq`, its padding form, its store path (3 dwords or 1..11 bytes) and the block index;
              encode: the lane of 12 bytes, its load and store form, `quads`, `have` of its last quad and the block index.
  model       `model_decode` / `model_encode`: the two kernels restated lane by lane (five aligned dwords and the byte funnel
              included), with the planted faults of DECODE_FAULTS / ENCODE_FAULTS switchable.  Without a fault it passes
              `check_decode` / `check_encode` - the very functions tests/test_base64_limits_gpu.py applies to the device's
              buffers - on every call; with any one fault some case fails (the reach test records which one first).

Every call's output is 0xA5 (decode) or 0x5A (encode) before it runs, `out_slot` is exactly sda_base64_decoded_max(max_chars) rounded
up to 4, and text between rows is foreign characters, input bytes between rows 0xFF: a stray byte, zero included, shows.

Out of reach and in no list: reads past the last dword of a row (the read stays inside the allocation's granule; the model's
`funnel.last_dword` fault covers the rule from the other side) and rows beyond the 2^31 - 1 chunk limit of the launchers."""
import functools
import random

M32 = (1 << 32) - 1
DEC_LANE_CHARS, ENC_LANE_BYTES, LANES = 16, 12, 256          # one lane = 16 characters <-> 12 bytes; kB64Threads lanes per workgroup
DEC_BLOCK_CHARS, ENC_BLOCK_BYTES = DEC_LANE_CHARS * LANES, ENC_LANE_BYTES * LANES          # 4096, 3072
OUT_FILL, TEXT_FILL, IN_FILL = 0xA5, 0x5A, 0xFF
SLACK = 64                                                     # bytes behind the last output row, filled and checked as well
STATUS_BIT = 8
NB_SENTINEL = 0x7777777777777777                               # d_out_bytes / d_text_bytes before a call

# ---- reference: RFC 4648 section 4 -------------------------------------------------------------------------------------------------
TABLE = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
VALUE = {c: v for v, c in enumerate(TABLE)}
PAD = ord("=")
assert len(TABLE) == len(VALUE) == 64


def ref_encode(raw):
    out = bytearray()
    for i in range(0, len(raw), 3):
        group = bytes(raw[i:i + 3])
        n = len(group)
        v = int.from_bytes(group + bytes(3 - n), "big")
        out += bytes([TABLE[v >> 18], TABLE[(v >> 12) & 63], TABLE[(v >> 6) & 63] if n > 1 else PAD, TABLE[v & 63] if n > 2 else PAD])
    return bytes(out)


def ref_decode(text):
    """the bytes of a valid row, None for a malformed one"""
    if len(text) % 4:
        return None
    out, quads = bytearray(), len(text) // 4
    for k in range(quads):
        q = text[4 * k:4 * k + 4]
        pad = 0
        if k == quads - 1 and q[3] == PAD:                      # only the last quad may be padded
            pad = 2 if q[2] == PAD else 1
        vals = []
        for c in q[:4 - pad]:
            if c not in VALUE:
                return None
            vals.append(VALUE[c])
        if (pad == 2 and vals[1] & 0xF) or (pad == 1 and vals[2] & 0x3):      # the bits under the padding are zero
            return None
        vals += [0] * pad
        v = (vals[0] << 18) | (vals[1] << 12) | (vals[2] << 6) | vals[3]
        out += v.to_bytes(3, "big")[:3 - pad]
    return bytes(out)


def decoded_max(n_chars):
    return n_chars // 4 * 3


def encoded_size(n_bytes):
    return (n_bytes + 2) // 3 * 4


def tight_out_slot(max_chars):
    return (decoded_max(max_chars) + 3) // 4 * 4


# ---- calls ---------------------------------------------------------------------------------------------------------------------------
class DecodeCall:
    """one call of base64_decode_rows_dev: the text buffer (4-byte aligned on the device), rows by offsets or by slots"""

    def __init__(self, name, doc, lens, names, want, offsets=None, text_slot=0):
        self.name, self.doc, self.lens, self.names, self.want = name, bytes(doc), list(lens), list(names), list(want)
        self.offsets, self.text_slot = (None if offsets is None else list(offsets)), text_slot
        self.rows = len(self.lens)
        self.max_chars = max(self.lens)
        self.out_slot = tight_out_slot(self.max_chars)
        assert len(self.names) == len(self.want) == self.rows and (offsets is None or len(offsets) == self.rows), name
        assert offsets is not None or text_slot >= self.max_chars, name
        assert all(self.start(r) + self.lens[r] <= len(self.doc) for r in range(self.rows)), name

    def start(self, r):
        return self.offsets[r] if self.offsets is not None else r * self.text_slot

    def text(self, r):
        return self.doc[self.start(r):self.start(r) + self.lens[r]]


class EncodeCall:
    """one call of base64_encode_rows_dev: raw row r at `in_shift` + r * in_slot of a 16-byte aligned buffer"""

    def __init__(self, name, raws, names, in_slot, in_shift=0):
        self.name, self.raws, self.names, self.in_slot, self.in_shift = name, [bytes(b) for b in raws], list(names), in_slot, in_shift
        self.rows = len(self.raws)
        self.lens = [len(b) for b in self.raws]
        self.max_bytes = max(self.lens)
        self.text_slot = (encoded_size(self.max_bytes) + 15) // 16 * 16
        self.want = [ref_encode(b) for b in self.raws]
        assert in_slot >= self.max_bytes and in_slot % 4 == 0 and in_shift % 4 == 0, name
        blob = bytearray([IN_FILL]) * (in_shift + self.rows * in_slot)
        for r, b in enumerate(self.raws):
            blob[in_shift + r * in_slot:in_shift + r * in_slot + len(b)] = b
        self.blob = bytes(blob)


class Layout:
    """a JSON-like document: every row placed at a chosen address mod 4, foreign characters between the rows"""

    def __init__(self, head=b'{"encryptions":["'):
        self.doc, self.offsets, self.lens = bytearray(head), [], []

    def put(self, text, align):
        self.doc += b'","'
        self.doc += b" " * ((align - len(self.doc)) % 4)
        self.offsets.append(len(self.doc))
        self.lens.append(len(text))
        self.doc += text

    def finish(self):
        return bytes(self.doc + b'"]}')


def _payload(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


# ---- ALPHABET: every byte value at each position of a quad, in three places ------------------------------------------------------------
ALPHABET_QUAD = b"TWE0"          # values 19, 22, 4, 52: 'E' leaves the two bits under a trailing '=' zero, so "TWE=" is valid
ALPHABET_PLACES = (("a: the row's only quad", 4, 0), ("b: quad 2 of a full lane", 16, 2), ("c: the last quad of three lanes", 48, 11))


@functools.lru_cache(maxsize=None)
def alphabet_rows():
    """3072 (name, text, expected)"""
    rng = random.Random(4648)
    out = []
    for place, length, quad in ALPHABET_PLACES:
        base = bytearray(ref_encode(_payload(rng, decoded_max(length))))
        base[4 * quad:4 * quad + 4] = ALPHABET_QUAD
        for pos in range(4):
            for byte in range(256):
                t = bytearray(base)
                t[4 * quad + pos] = byte
                out.append((f"ALPHABET {place[0]} pos={pos} byte=0x{byte:02x}", bytes(t), ref_decode(bytes(t))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def alphabet_calls():
    rows = alphabet_rows()
    slot = 48
    doc = bytearray(b"*") * (slot * len(rows))
    for r, (_, t, _) in enumerate(rows):
        doc[r * slot:r * slot + len(t)] = t
    slots = DecodeCall("ALPHABET slots", doc, [len(t) for _, t, _ in rows], [n for n, _, _ in rows], [w for _, _, w in rows], text_slot=slot)
    lay, names, want = Layout(), [], []
    for name, t, w in rows:
        for a in range(4):
            lay.put(t, a)
            names.append(f"{name} @{a}")
            want.append(w)
    offs = DecodeCall("ALPHABET offsets", lay.finish(), lay.lens, names, want, offsets=lay.offsets)
    return slots, offs


# ---- PADDING: all 64^2 "XY==" and "QYZ=", alone, behind one lane and behind one workgroup --------------------------------------------
PADDING_SPECIALS = (b"====", b"Z===", b"Zg==Zg==", b"Zm9v====", b"=m9vZm9v", b"Z=9vZm9v", b"Zm=vZm9v", b"Zm9=Zm9v")


@functools.lru_cache(maxsize=None)
def padding_tails():
    two = [bytes([x, y, PAD, PAD]) for x in TABLE for y in TABLE]
    one = [bytes([ord("Q"), y, z, PAD]) for y in TABLE for z in TABLE]
    return tuple(two), tuple(one)


@functools.lru_cache(maxsize=None)
def padding_prefix(chars):
    return ref_encode(_payload(random.Random(chars), decoded_max(chars)))


def _slotted(name, texts, names, want, slot):
    doc = bytearray(b"*") * (slot * len(texts))
    for r, t in enumerate(texts):
        doc[r * slot:r * slot + len(t)] = t
    return DecodeCall(name, doc, [len(t) for t in texts], names, want, text_slot=slot)


@functools.lru_cache(maxsize=None)
def padding_short_call():
    """the 2 x 4096 tails alone and behind one full lane, and the specials, by offsets into one document"""
    lay, names, want = Layout(), [], []
    for chars in (0, DEC_LANE_CHARS):
        _put_tails(lay, names, want, padding_prefix(chars), None)
    for k, t in enumerate(PADDING_SPECIALS):
        lay.put(t, k % 4)
        names.append(f"PADDING special {t.decode()}")
        want.append(ref_decode(t))
    return DecodeCall("PADDING short", lay.finish(), lay.lens, names, want, offsets=lay.offsets)


def _put_tails(lay, names, want, pre, head):
    """tail i = 64 hi + lo at alignment (hi + lo + lo // 16) mod 4: the valid tails (lo a multiple of 16, or of 4) take every alignment"""
    for group in padding_tails():
        for i, tail in enumerate(group):
            lay.put(pre + tail, (i // 64 + i % 64 + i % 64 // 16) % 4)
            names.append(f"PADDING {tail.decode()} behind {len(pre)} characters @{lay.offsets[-1] % 4}")
            if head is None:
                want.append(ref_decode(pre + tail))
            else:                                                # quad by quad: the shared head and the last quad
                last = ref_decode(tail)
                want.append(None if last is None else head + last)


@functools.lru_cache(maxsize=None)
def padding_long_call():
    """the 2 x 4096 tails as the only quad of block 1, by offsets into one document"""
    pre = padding_prefix(DEC_BLOCK_CHARS)
    head = ref_decode(pre)
    assert head is not None and len(head) == ENC_BLOCK_BYTES
    lay, names, want = Layout(), [], []
    _put_tails(lay, names, want, pre, head)
    return DecodeCall("PADDING long", lay.finish(), lay.lens, names, want, offsets=lay.offsets)


# ---- EDGES: every length around a lane and around a workgroup, with each padding form, at each alignment -----------------------------
EDGE_CHARS = tuple(range(0, 40, 4)) + tuple(DEC_BLOCK_CHARS * j + d for j in (1, 2, 3) for d in (-4, 0, 4))


@functools.lru_cache(maxsize=None)
def edge_rows():
    """(name, payload, text): 55 rows - text lengths EDGE_CHARS, each ending in each padding form its length allows"""
    rng = random.Random(3072)
    out = []
    for chars in EDGE_CHARS:
        for pad in (0, 1, 2) if chars else (0,):
            raw = _payload(rng, decoded_max(chars) - pad)
            text = ref_encode(raw)
            assert len(text) == chars and text.count(b"=") == pad
            out.append((f"EDGES {chars} characters pad={pad}", raw, text))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edges_offsets_call():
    """every edge row at every alignment in one document; and windows at offsets 0, 1, 2, 3 of the document itself"""
    lay, names, want = Layout(head=b"QUJDREVGR0hJSktMTU5PUFFS"), [], []
    for k in range(4):                                          # overlapping windows of the document's first 24 characters
        lay.offsets.append(k); lay.lens.append(12 + 4 * (k & 1)); names.append(f"EDGES window at document offset {k}")
        want.append(ref_decode(bytes(lay.doc[k:k + lay.lens[-1]])))
    for name, raw, text in edge_rows():
        for a in range(4):
            lay.put(text, a)
            names.append(f"{name} @{a}")
            want.append(raw)
    return DecodeCall("EDGES offsets", lay.finish(), lay.lens, names, want, offsets=lay.offsets)


@functools.lru_cache(maxsize=None)
def edges_slot_call(slot_extra, reps):
    """the edge rows `reps` times over in slots of max_chars + slot_extra characters: row r starts at r * text_slot"""
    rows = edge_rows()
    slot = max(EDGE_CHARS) + slot_extra
    texts, names, want = [], [], []
    for k in range(reps):
        for name, raw, text in rows:
            r = len(texts)
            texts.append(text); names.append(f"{name} @{r * slot % 4} (slot {slot})"); want.append(raw)
    return _slotted(f"EDGES text_slot={slot}", texts, names, want, slot)


def edges_calls():
    return edges_offsets_call(), edges_slot_call(1, 4), edges_slot_call(2, 2)      # 12293: odd, 12294: = 2 mod 4


# ---- PLANTED: one foreign character in a row of three blocks, valid neighbours either side ----------------------------------------------
PLANTED_CHARS = DEC_BLOCK_CHARS * 3 - 4                        # 12284, ends in one '='
PLANTED_POSITIONS = (0, 15, 16, 4079, 4080, 4095, 4096, 4111, PLANTED_CHARS - 1)
PLANTED_FOREIGN = (ord("*"), ord("\n"), PAD, 0x80, ord("-"), ord("_"), ord(" "), 0x00, ord("@"))
NEIGHBOUR_CHARS = DEC_BLOCK_CHARS + 16


@functools.lru_cache(maxsize=None)
def planted_call():
    rng = random.Random(12284)
    good = ref_encode(_payload(rng, decoded_max(PLANTED_CHARS) - 1))
    assert len(good) == PLANTED_CHARS and good.endswith(b"=") and not good.endswith(b"==")
    lay, names, want = Layout(), [], []

    def neighbour(i):
        raw = _payload(rng, decoded_max(NEIGHBOUR_CHARS))
        lay.put(ref_encode(raw), (i * 3) % 4)
        names.append(f"PLANTED neighbour {i}")
        want.append(raw)
    neighbour(0)
    i = 1
    for a in range(4):
        for pos, byte in zip(PLANTED_POSITIONS, PLANTED_FOREIGN):
            t = bytearray(good)
            t[pos] = byte
            lay.put(bytes(t), a)
            names.append(f"PLANTED 0x{byte:02x} at {pos} @{a}")
            want.append(ref_decode(bytes(t)))
            assert want[-1] is None
            neighbour(i)
            i += 1
    return DecodeCall("PLANTED", lay.finish(), lay.lens, names, want, offsets=lay.offsets)


# ---- STORES: every payload length 0..52 and its malformed twin in odd slots; the encoder's small rows off the 16-byte grid ------------
STORES_BYTES = tuple(range(53))


@functools.lru_cache(maxsize=None)
def stores_decode_call():
    rng = random.Random(52)
    texts, names, want = [], [], []
    for n in STORES_BYTES:
        raw = _payload(rng, n)
        texts.append(ref_encode(raw)); names.append(f"STORES {n} bytes"); want.append(raw)
    for n in STORES_BYTES[1:]:
        t = bytearray(texts[n])
        t[len(t) - 4] = ord("*")                                # the twin: a foreign character first in the last quad
        texts.append(bytes(t)); names.append(f"STORES {n} bytes, malformed twin"); want.append(ref_decode(bytes(t)))
        assert want[-1] is None
    return _slotted("STORES decode", texts, names, want, 73)     # row r starts at r mod 4


@functools.lru_cache(maxsize=None)
def encode_calls():
    rng = random.Random(16)
    small = EncodeCall("STORES encode", [_payload(rng, n) for n in STORES_BYTES], [f"STORES encode {n} bytes" for n in STORES_BYTES], 52, in_shift=4)
    rows = edge_rows()
    slot = (max(len(raw) for _, raw, _ in rows) + 3) // 4 * 4          # 9220: a multiple of 4, not of 16
    edges = EncodeCall("EDGES encode", [raw for _, raw, _ in rows], [f"{name} (encode {len(raw)} bytes)" for name, raw, _ in rows], slot, in_shift=4)
    assert slot % 16 and all(text == w for (_, _, text), w in zip(rows, edges.want))
    return small, edges


def decode_calls():
    """every decode call, the small ones first (the order the planted-fault table walks)"""
    return [stores_decode_call(), *alphabet_calls(), padding_short_call(), *edges_calls(), planted_call(), padding_long_call()]


LONG_SAMPLE = 16                                               # the CPU model and ref_decode walk every 16th row of "PADDING long" whole


# ---- geometry, restated by hand ---------------------------------------------------------------------------------------------------------
def decode_lane_label(mis, nq, pad):
    n_out = 3 * nq - pad
    return f"dec mis={mis} nq={nq} pad={'none' if pad == 0 else '=' * pad} store={'3 dwords' if n_out == 12 else f'{n_out} bytes'}"


def decode_labels(call):
    """what the VALID rows of a call reach (lane shapes, block index per misalignment), and where the malformed ones are flagged"""
    ev = set()
    for r in range(call.rows):
        n, start = call.lens[r], call.start(r)
        text = call.text(r)
        if call.want[r] is None:
            first = next((i for i in range(n - n % 4) if text[i] not in VALUE and not (text[i] == PAD and i >= n - 2)), None)
            if first is not None and n % 4 == 0:
                lane = first // DEC_LANE_CHARS
                ev.add(f"dec flag block={'0' if lane < LANES else '>0'} lane={lane % LANES if lane % LANES in (0, LANES - 1) else 'inner'}")
            continue
        pad = text[-2:].count(b"=") if n else 0
        for c0 in range(0, n, DEC_LANE_CHARS):
            mis = (start + c0) & 3
            avail = n - c0
            nq = 4 if avail >= DEC_LANE_CHARS else avail // 4
            ev.add(decode_lane_label(mis, nq, pad if avail <= DEC_LANE_CHARS else 0))
            ev.add(f"dec mis={mis} block={'0' if c0 < DEC_BLOCK_CHARS else '>0'}")
        if n == 0:
            ev.add("dec empty row")
    return ev


def encode_labels(call):
    ev = set()
    for n in call.lens:
        for b0 in range(0, n, ENC_LANE_BYTES):
            left = n - b0
            nb = min(left, ENC_LANE_BYTES)
            quads = (nb + 2) // 3
            have = nb - 3 * (quads - 1)
            block = "0" if b0 < ENC_BLOCK_BYTES else ">0"
            ev.add(f"enc quads={quads} have={have}")
            ev.add(f"enc load={'3 dwords' if left >= ENC_LANE_BYTES else 'bytes'} block={block}")
            ev.add(f"enc store={'uint4' if quads == 4 else 'dwords'} block={block}")
        if n == 0:
            ev.add("enc empty row")
    return ev


# ---- the kernels restated, with switchable faults -----------------------------------------------------------------------------------------
_RANGES = (("upper", ord("A"), 26, 0), ("lower", ord("a"), 26, 26), ("digit", ord("0"), 10, 52))
DECODE_FAULTS = tuple(f"{name}.{end}" for name, _, _, _ in _RANGES for end in ("lo-1", "lo+1", "hi-1", "hi+1")) + (
    "accepts - and _", "= accepted in a non-last quad", "mask == dropped", "mask = dropped", "masks swapped", "count ignores the padding",
    "funnel.mis1+1", "funnel.mis2+1", "funnel.mis3+1", "funnel.last_dword", "store.12 bytes for a tail", "flag on row r+1", "62 and 63 swapped")
ENCODE_FAULTS = ("62 and 63 swapped", "= count for have == 1", "store.uint4 for a tail", "load.12 bytes for a tail")


def model_value(c, fault=None):
    v = 0xFF
    for name, lo, count, base in _RANGES:
        if fault == name + ".lo-1":
            lo -= 1
        elif fault == name + ".lo+1":
            lo += 1
        elif fault == name + ".hi-1":
            count -= 1
        elif fault == name + ".hi+1":
            count += 1
        d = (c - lo) & M32
        if d < count:
            v = d + base
    swap = fault == "62 and 63 swapped"
    if c == ord("+"):
        v = 63 if swap else 62
    if c == ord("/"):
        v = 62 if swap else 63
    if fault == "accepts - and _":
        v = 62 if c == ord("-") else 63 if c == ord("_") else v
    return v


def model_char(v, fault=None):
    if fault == "62 and 63 swapped" and v >= 62:
        v ^= 1
    return v + 65 if v < 26 else v + 97 - 26 if v < 52 else v + 48 - 52 if v < 62 else ord("+") if v == 62 else ord("/")


def alignbyte(hi, lo, sh):
    return (((hi << 32) | lo) >> (8 * sh)) & M32


def model_decode(call, fault=None, status0=0, rows=None):
    """-> (status, row_status, out_bytes, out) as the device leaves them, for `rows` (default: all)"""
    n_rows, slot, doc = call.rows, call.out_slot, call.doc
    out = bytearray([OUT_FILL]) * (n_rows * slot + SLACK)
    nbs, rs, status = [NB_SENTINEL] * n_rows, [0] * n_rows, status0
    values = [model_value(c, fault) for c in range(256)]

    def word(at):
        return int.from_bytes(doc[at:at + 4].ljust(4, b"\0"), "little")

    def flag(r):
        rr = r + 1 if fault == "flag on row r+1" else r
        if rr < n_rows:
            rs[rr] = 1
        return status | STATUS_BIT
    for r in (range(n_rows) if rows is None else rows):
        n, start = call.lens[r], call.start(r)
        if n > call.max_chars:
            nbs[r], status = 0, flag(r)
            continue
        nb = n // 4 * 3
        if n & 3:
            nbs[r], status = 0, flag(r)
            continue
        if n >= 4 and doc[start + n - 1] == PAD and fault != "count ignores the padding":
            nb -= 2 if doc[start + n - 2] == PAD else 1
        nbs[r] = nb
        for c0 in range(0, n, DEC_LANE_CHARS):
            addr = start + c0
            mis = addr & 3
            avail = n - c0
            nq = 4 if avail >= 16 else avail // 4
            reach = 4 * nq if fault == "funnel.last_dword" else mis + 4 * nq
            d = [word(addr - mis + 4 * i) if 4 * i < reach else 0 for i in range(5)]      # never past the row's last dword
            sh = mis + 1 if fault == f"funnel.mis{mis}+1" else mis
            q = [alignbyte(d[i + 1], d[i], sh) if mis else d[i] for i in range(4)]
            bad, ob = False, []
            for i in range(nq):
                ch = [(q[i] >> (8 * j)) & 0xFF for j in range(4)]
                last = c0 + 4 * i + 4 == n or fault == "= accepted in a non-last quad"
                v = [values[c] for c in ch]
                nbytes = 3
                if last and ch[3] == PAD:
                    v[3], nbytes = 0, 2
                    m2, m1 = (0x3, 0xF) if fault == "masks swapped" else (0xF, 0x3)
                    if ch[2] == PAD:
                        v[2], nbytes = 0, 1
                        bad |= fault != "mask == dropped" and (v[1] & m2) != 0
                    else:
                        bad |= fault != "mask = dropped" and (v[2] & m1) != 0
                bad |= (v[0] | v[1] | v[2] | v[3]) > 63
                tri = ((v[0] << 18) | (v[1] << 12) | (v[2] << 6) | v[3]) & 0xFFFFFF
                ob += list(tri.to_bytes(3, "big")[:nbytes])
            if bad:
                status = flag(r)
            dst = r * slot + c0 // 4 * 3
            if fault == "store.12 bytes for a tail":
                ob += [0] * (12 - len(ob))
            out[dst:dst + len(ob)] = bytes(ob)
    return status, rs, nbs, bytes(out)


def model_encode(call, fault=None):
    """-> (text_bytes, text) as the device leaves them"""
    slot = call.text_slot
    text = bytearray([TEXT_FILL]) * (call.rows * slot + SLACK)
    tbs = [NB_SENTINEL] * call.rows
    blob = call.blob + bytes([IN_FILL]) * 16
    for r, n in enumerate(call.lens):
        if n > call.max_bytes:
            tbs[r] = 0
            continue
        tbs[r] = (n + 2) // 3 * 4
        for b0 in range(0, n, ENC_LANE_BYTES):
            src = call.in_shift + r * call.in_slot + b0
            left = n - b0
            w = blob[src:src + 12] if left >= 12 or fault == "load.12 bytes for a tail" else blob[src:src + left] + bytes(12 - left)
            nb = min(left, 12)
            outw = bytearray()
            for i in range(4):
                p = 3 * i
                tri = (w[p] << 16) | (w[p + 1] << 8) | w[p + 2]
                have = min(nb - p, 3) if nb > p else 0
                c = [model_char((tri >> s) & 63, fault) for s in (18, 12, 6, 0)]
                if have < 3:
                    c[3] = PAD
                if have < 2 and not (fault == "= count for have == 1" and have == 1):
                    c[2] = PAD
                outw += bytes(c)
            quads = 4 if fault == "store.uint4 for a tail" else (nb + 2) // 3
            dst = r * slot + b0 // 3 * 4
            text[dst:dst + 4 * quads] = outw[:4 * quads]
    return tbs, bytes(text)


# ---- the checks: applied to the model's buffers on the CPU and to the device's on the GPU -----------------------------------------------
def check_decode(call, status, row_status, out_bytes, out, status0=0, rows=None, limit=5):
    """every violation as one line that names the case; [] when the buffers are what the reference expects"""
    errs, slot = [], call.out_slot
    fill = bytes([OUT_FILL])

    def err(r, what):
        if len(errs) < limit:
            errs.append(f"{call.name}: {call.names[r]}: {what}")
    walk = range(call.rows) if rows is None else rows
    for r in walk:
        want, got = call.want[r], bytes(out[r * slot:(r + 1) * slot])
        nb = int(out_bytes[r])
        if (row_status[r] != 0) != (want is None):
            err(r, f"d_row_status = {row_status[r]}, the reference says {'malformed' if want is None else 'valid'}")
        if want is not None:
            if nb != len(want):
                err(r, f"d_out_bytes = {nb}, the reference decodes {len(want)} bytes")
            elif got[:nb] != want:
                at = next(i for i in range(nb) if got[i] != want[i])
                err(r, f"byte {at} is 0x{got[at]:02x}, the reference has 0x{want[at]:02x}")
            if got[len(want):] != fill * (slot - len(want)):
                err(r, f"written in [{len(want)}, {slot}) of its slot")
        else:
            bound = decoded_max(call.lens[r]) if call.lens[r] <= call.max_chars else 0
            if nb > bound:
                err(r, f"d_out_bytes = {nb} for a malformed row of {call.lens[r]} characters, beyond {bound}")
            if got[bound:] != fill * (slot - bound):
                err(r, f"a malformed row written beyond the first {bound} bytes of its slot")
    if rows is None:
        if bytes(out[call.rows * slot:]) != fill * (len(out) - call.rows * slot):
            errs.append(f"{call.name}: written behind the last row")
        want_status = status0 | (STATUS_BIT if any(w is None for w in call.want) else 0)
        if status != want_status:
            errs.append(f"{call.name}: *d_status = 0x{status:x}, expected 0x{want_status:x}")
    return errs


def check_encode(call, text_bytes, text, limit=5):
    errs, slot = [], call.text_slot
    fill = bytes([TEXT_FILL])
    for r in range(call.rows):
        want, got = call.want[r], bytes(text[r * slot:(r + 1) * slot])
        if int(text_bytes[r]) != len(want):
            errs.append(f"{call.name}: {call.names[r]}: d_text_bytes = {int(text_bytes[r])}, the reference encodes {len(want)} characters")
        elif got[:len(want)] != want:
            at = next(i for i in range(len(want)) if got[i] != want[i])
            errs.append(f"{call.name}: {call.names[r]}: character {at} is {bytes(got[at:at + 1])!r}, the reference has {want[at:at + 1]!r}")
        if got[len(want):] != fill * (slot - len(want)):
            errs.append(f"{call.name}: {call.names[r]}: written in [{len(want)}, {slot}) of its slot")
        if len(errs) >= limit:
            break
    if bytes(text[call.rows * slot:]) != fill * (len(text) - call.rows * slot):
        errs.append(f"{call.name}: written behind the last row")
    return errs

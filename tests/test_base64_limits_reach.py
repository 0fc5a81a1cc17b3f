"""Reach checks for the crafted base64 rows of tests/test_base64_limits_gpu.py (CPU).

1. The module's RFC 4648 reference equals oracle.wire_oracle - verdict and bytes - on every row of every call, and the published vectors.
2. The counts the alphabet and the strict padding imply hold: 64 valid bytes per non-padding position, 65 in the last position of a row,
   256 valid "XY==" and 1024 valid "QYZ=" wherever the quad stands.
3. The calls reach every label of the geometry model; the lists are written out here, so a case that moves off its edge fails by name.
4. The kernels' restatement passes the checks of the GPU file without a fault, and every planted fault is noticed; the table
   fault -> first case that notices it is written out below."""
import pytest

import base64_limits as B

DECODE_LANES = [B.decode_lane_label(mis, nq, pad) for mis in range(4) for nq in (1, 2, 3, 4) for pad in (0, 1, 2)]
DECODE_FULL = DECODE_LANES + [f"dec mis={mis} block={b}" for mis in range(4) for b in ("0", ">0")] + ["dec empty row"] + \
              [f"dec flag block={b} lane={lane}" for b in ("0", ">0") for lane in (0, 255)] + ["dec flag block=0 lane=inner"]
ENCODE_FULL = [f"enc quads={q} have={h}" for q in (1, 2, 3, 4) for h in (1, 2, 3)] + ["enc empty row"] + \
              [f"enc {what} block={b}" for what in ("load=3 dwords", "load=bytes", "store=uint4", "store=dwords") for b in ("0", ">0")]

# fault -> the first case (in the order of base64_limits.decode_calls() / encode_calls()) whose check fails under it
DECODE_NOTICED = {
    "upper.lo-1": "STORES decode: STORES 1 bytes: d_row_status = 1, the reference says valid",
    "upper.lo+1": "STORES decode: STORES 1 bytes: d_row_status = 1, the reference says valid",
    "upper.hi-1": "STORES decode: STORES 17 bytes: d_row_status = 1, the reference says valid",
    "upper.hi+1": "ALPHABET slots: ALPHABET a pos=0 byte=0x5b: d_row_status = 0, the reference says malformed",
    "lower.lo-1": "STORES decode: STORES 1 bytes: byte 0 is 0x8d, the reference has 0x89",
    "lower.lo+1": "STORES decode: STORES 1 bytes: byte 0 is 0x85, the reference has 0x89",
    "lower.hi-1": "STORES decode: STORES 16 bytes: d_row_status = 1, the reference says valid",
    "lower.hi+1": "ALPHABET slots: ALPHABET a pos=0 byte=0x7b: d_row_status = 0, the reference says malformed",
    "digit.lo-1": "STORES decode: STORES 4 bytes: byte 1 is 0x61, the reference has 0x51",
    "digit.lo+1": "STORES decode: STORES 4 bytes: byte 1 is 0x41, the reference has 0x51",
    "digit.hi-1": "STORES decode: STORES 7 bytes: d_row_status = 1, the reference says valid",
    "digit.hi+1": "ALPHABET slots: ALPHABET a pos=0 byte=0x3a: d_row_status = 0, the reference says malformed",
    "accepts - and _": "ALPHABET slots: ALPHABET a pos=0 byte=0x2d: d_row_status = 0, the reference says malformed",
    "= accepted in a non-last quad": "ALPHABET slots: ALPHABET b pos=3 byte=0x3d: d_row_status = 0, the reference says malformed",
    "mask == dropped": "PADDING short: PADDING AB== behind 0 characters @1: d_row_status = 0, the reference says malformed",
    "mask = dropped": "PADDING short: PADDING QAB= behind 0 characters @1: d_row_status = 0, the reference says malformed",
    "masks swapped": "STORES decode: STORES 2 bytes: d_row_status = 1, the reference says valid",
    "count ignores the padding": "STORES decode: STORES 1 bytes: d_out_bytes = 3, the reference decodes 1 bytes",
    "funnel.mis1+1": "STORES decode: STORES 1 bytes: d_row_status = 1, the reference says valid",
    "funnel.mis2+1": "STORES decode: STORES 2 bytes: d_row_status = 1, the reference says valid",
    "funnel.mis3+1": "STORES decode: STORES 3 bytes: d_row_status = 1, the reference says valid",
    "funnel.last_dword": "STORES decode: STORES 1 bytes: d_row_status = 1, the reference says valid",
    "store.12 bytes for a tail": "STORES decode: STORES 1 bytes: written in [1, 56) of its slot",
    "flag on row r+1": "STORES decode: STORES 1 bytes, malformed twin: d_row_status = 0, the reference says malformed",
    "62 and 63 swapped": "STORES decode: STORES 2 bytes: byte 1 is 0xe7, the reference has 0xf7",
}
ENCODE_NOTICED = {
    "62 and 63 swapped": "STORES encode: STORES encode 8 bytes: character 8 is b'+', the reference has b'/'",
    "= count for have == 1": "STORES encode: STORES encode 1 bytes: character 2 is b'A', the reference has b'='",
    "store.uint4 for a tail": "STORES encode: STORES encode 1 bytes: written in [4, 80) of its slot",
    "load.12 bytes for a tail": "STORES encode: STORES encode 1 bytes: character 1 is b'f', the reference has b'Q'",
}


def _oracle_decode(text):
    from oracle import wire_oracle as wo
    try:
        return wo.binary_from_base64(text)
    except ValueError:
        return None


def _sample(call):
    return range(0, call.rows, B.LONG_SAMPLE) if call.name == "PADDING long" else None


# ---- 1. the reference -------------------------------------------------------------------------------------------------------------
def test_reference_reproduces_the_rfc_vectors():
    from oracle import wire_oracle as wo
    for raw, text in wo.RFC4648_VECTORS:
        assert B.ref_encode(raw) == text and B.ref_decode(text) == raw
    assert bytes(sorted(B.TABLE)) == bytes(sorted(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/")) and B.TABLE[62:] == b"+/"


@pytest.mark.parametrize("index", range(9))
def test_reference_equals_the_oracle_on_every_decode_row(index):
    call = B.decode_calls()[index]
    walk = _sample(call)
    for r in range(call.rows):
        text = call.text(r)
        assert call.want[r] == _oracle_decode(text), call.names[r]                 # every row, whole, the long ones too
        if walk is None or r in walk:
            assert call.want[r] == B.ref_decode(text), call.names[r]
        if call.want[r] is not None and (walk is None or r in walk):
            assert B.ref_encode(call.want[r]) == text, call.names[r]


def test_reference_equals_the_oracle_on_every_encode_row():
    from oracle import wire_oracle as wo
    for call in B.encode_calls():
        for r in range(call.rows):
            assert call.want[r] == wo.binary_to_base64(call.raws[r]) == B.ref_encode(call.raws[r]), call.names[r]
            assert B.ref_decode(call.want[r]) == call.raws[r] == _oracle_decode(call.want[r]), call.names[r]


# ---- 2. the counts ------------------------------------------------------------------------------------------------------------------
def test_alphabet_counts():
    rows = B.alphabet_rows()
    assert len(rows) == 3 * 4 * 256 and max(len(t) for _, t, _ in rows) == 48
    for p, (place, length, quad) in enumerate(B.ALPHABET_PLACES):
        for pos in range(4):
            group = rows[(4 * p + pos) * 256:(4 * p + pos + 1) * 256]
            valid = {t[4 * quad + pos] for _, t, w in group if w is not None}
            ends_row = 4 * quad + pos == length - 1
            assert valid == set(B.TABLE) | ({B.PAD} if ends_row else set()), (place, pos)
            assert len(valid) == (65 if ends_row else 64)
    slots, offs = B.alphabet_calls()
    assert slots.rows == 3072 and offs.rows == 12288
    assert [offs.start(r) % 4 for r in range(offs.rows)] == [0, 1, 2, 3] * 3072
    assert all(offs.text(4 * r + a) == slots.text(r) for r in range(0, 3072, 7) for a in range(4))


def test_padding_counts():
    short, long_ = B.padding_short_call(), B.padding_long_call()
    assert short.rows == 2 * 8192 + len(B.PADDING_SPECIALS) and long_.rows == 8192 and long_.max_chars == 4096 + 4
    for call, groups in ((short, 4), (long_, 2)):
        for g in range(groups):
            valid = sum(w is not None for w in call.want[4096 * g:4096 * (g + 1)])
            assert valid == (256 if g % 2 == 0 else 1024), (call.name, g)
            tails = {call.text(r)[-4:] for r in range(4096 * g, 4096 * (g + 1))}
            assert len(tails) == 4096 and all(t.endswith(b"==" if g % 2 == 0 else b"=") for t in tails)
    assert all(w is None for w in short.want[-len(B.PADDING_SPECIALS):])
    for call in (short, long_):                                  # valid and malformed tails of either form at every alignment
        seen = {(call.text(r)[-2:].count(b"="), call.want[r] is None, call.start(r) % 4) for r in range(call.rows - call.rows % 4096)}
        assert len(seen) == 2 * 2 * 4, call.name


def test_edges_and_planted_are_laid_out_as_named():
    rows = B.edge_rows()
    assert len(rows) == 55 and sorted({len(t) for _, _, t in rows}) == sorted(B.EDGE_CHARS)
    assert set(B.EDGE_CHARS) == set(range(0, 40, 4)) | {4096 * j + d for j in (1, 2, 3) for d in (-4, 0, 4)}
    assert {len(raw) for _, raw, _ in rows} >= {3072 * j + d for j in (1, 2, 3) for d in range(-5, 4)}       # the encoder's edge, 3072 bytes
    offs, odd, two = B.edges_calls()
    assert [offs.start(r) for r in range(4)] == [0, 1, 2, 3] and all(offs.want[r] is not None for r in range(4))
    assert odd.text_slot % 2 == 1 and two.text_slot % 4 == 2
    for call in (offs, odd):                                                          # every row shape at every alignment
        seen = {(call.lens[r], call.text(r)[-2:].count(b"="), call.start(r) % 4) for r in range(call.rows)}
        assert seen >= {(len(t), t[-2:].count(b"="), a) for _, _, t in rows for a in range(4)}, call.name
    assert {two.start(r) % 4 for r in range(two.rows)} == {0, 2}
    planted = B.planted_call()
    bad = [r for r in range(planted.rows) if planted.want[r] is None]
    assert len(bad) == 4 * len(B.PLANTED_POSITIONS) == 36 and B.PLANTED_POSITIONS == (0, 15, 16, 4079, 4080, 4095, 4096, 4111, 12283)
    for k, r in enumerate(bad):
        assert planted.want[r - 1] is not None and planted.want[r + 1] is not None and planted.lens[r] == B.PLANTED_CHARS
        assert planted.start(r) % 4 == k // 9 and planted.text(r)[B.PLANTED_POSITIONS[k % 9]] == B.PLANTED_FOREIGN[k % 9]
    for call in B.decode_calls():
        assert call.out_slot == (B.decoded_max(call.max_chars) + 3) // 4 * 4 and call.max_chars == max(call.lens), call.name
    for call in B.encode_calls():
        assert call.in_slot % 4 == 0 and call.in_slot % 16 and call.in_shift == 4 and call.text_slot % 16 == 0, call.name
        assert call.text_slot - B.encoded_size(call.max_bytes) < 16


# ---- 3. reach ----------------------------------------------------------------------------------------------------------------------------
def _same(full, got, what):
    want = set(full)
    assert len(want) == len(full)
    missing, extra = sorted(want - got), sorted(got - want)
    assert not missing, f"{what}: no case reaches {missing[:6]}"
    assert not extra, f"{what}: the model names labels the list does not hold: {extra[:6]}"


def test_reach_decode():
    assert len(DECODE_LANES) == 48
    got = set()
    for call in B.decode_calls():
        got |= B.decode_labels(call)
    _same(DECODE_FULL, got, "decode")
    # the families on their own: every lane shape by offsets and by an odd slot; a misaligned last lane of block > 0 with each padding form
    offs, odd, _ = B.edges_calls()
    for call in (offs, odd):
        assert B.decode_labels(call) >= set(DECODE_LANES), call.name
    stores = {label.split("store=")[1] for label in B.decode_labels(B.stores_decode_call()) if "store=" in label}
    assert stores == {"3 dwords"} | {f"{n} bytes" for n in range(1, 12)}            # every tail length against the 0xA5 background
    long_ = B.decode_labels(B.padding_long_call())
    assert long_ >= {f"dec mis={m} block=>0" for m in range(4)} | {B.decode_lane_label(m, 1, p) for m in range(4) for p in (1, 2)}
    assert B.decode_labels(B.planted_call()) >= {f"dec flag block={b} lane={lane}" for b in ("0", ">0") for lane in (0, 255)}


def test_reach_encode():
    small, edges = B.encode_calls()
    _same(ENCODE_FULL, B.encode_labels(small) | B.encode_labels(edges), "encode")
    assert B.encode_labels(small) >= set(ENCODE_FULL[:13])                         # every (quads, have) off the 16-byte grid


# ---- 4. the model and its planted faults ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(9))
def test_model_without_a_fault_is_the_reference(index):
    call = B.decode_calls()[index]
    walk = _sample(call)
    for status0 in (0, 0x14) if call.rows < 200 else (0,):
        assert B.check_decode(call, *B.model_decode(call, status0=status0, rows=walk), status0=status0, rows=walk) == []


def test_encode_model_without_a_fault_is_the_reference():
    for call in B.encode_calls():
        assert B.check_encode(call, *B.model_encode(call)) == []


def test_alignbyte_funnel_restated():
    raw = bytes(range(1, 21))
    d = [int.from_bytes(raw[4 * i:4 * i + 4], "little") for i in range(5)]
    for mis in range(1, 4):
        for i in range(4):
            assert B.alignbyte(d[i + 1], d[i], mis).to_bytes(4, "little") == raw[4 * i + mis:4 * i + mis + 4]


@pytest.mark.parametrize("fault", B.DECODE_FAULTS)
def test_a_planted_decode_fault_is_noticed(fault):
    for call in B.decode_calls()[:-1]:
        errs = B.check_decode(call, *B.model_decode(call, fault=fault), limit=1)
        if errs:
            assert errs[0] == DECODE_NOTICED[fault]
            return
    pytest.fail(f"no case notices the planted fault '{fault}'")


@pytest.mark.parametrize("fault", B.ENCODE_FAULTS)
def test_a_planted_encode_fault_is_noticed(fault):
    for call in B.encode_calls():
        errs = B.check_encode(call, *B.model_encode(call, fault=fault), limit=1)
        if errs:
            assert errs[0] == ENCODE_NOTICED[fault]
            return
    pytest.fail(f"no case notices the planted fault '{fault}'")


def test_the_fault_tables_are_whole():
    assert set(DECODE_NOTICED) == set(B.DECODE_FAULTS) and set(ENCODE_NOTICED) == set(B.ENCODE_FAULTS)
    assert len(B.DECODE_FAULTS) == 25 and len(B.ENCODE_FAULTS) == 4


def test_faults_that_only_the_large_rows_can_show():
    """the funnel faults again on the rows of block > 0 alone, the row flag on the planted rows alone: each family notices by itself"""
    long_ = B.padding_long_call()
    walk = range(0, long_.rows, 97)
    for mis in (1, 2, 3):
        assert B.check_decode(long_, *B.model_decode(long_, fault=f"funnel.mis{mis}+1", rows=walk), rows=walk)
    planted = B.planted_call()
    errs = B.check_decode(planted, *B.model_decode(planted, fault="flag on row r+1"), limit=100)
    assert len(errs) == 72                                                          # 36 rows not flagged, 36 neighbours flagged

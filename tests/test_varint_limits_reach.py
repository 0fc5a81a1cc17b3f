"""Reach checks for the crafted wire-codec cases of tests/test_varint_limits_gpu.py (CPU).

1. The hand-built bytes of every case are what both oracles encode from the case's values, and decode back to them: the fixtures
   are right without a GPU.
2. Per kernel form, the events that the cases fed to that form reach (tests/varint_limits.py: computed from byte positions only)
   are exactly the form's list, which is written out here - so an edit that moves a value off its boundary, or drops a case,
   fails here by the name of the missing event and not silently on the GPU box.  Nothing is waived; what cannot be reached at
   a size a test can afford is named in the docstring of varint_limits.py and appears in no list.
3. The restatements of the kernels' bit tricks equal the Python-integer codec."""
import numpy as np
import pytest

import varint_limits as V

STRADDLE = [f"n={n} s={s}" for n in range(2, 11) for s in range(1, n)] + ["term=last n=10", "start=first n=10", "term=first after n=10"]
LEN_X = [f"len.x={x}" for x in range(7, 71)]
ROW_PHASES = [f"stream.row a={a}" for a in range(16)] + [f"stream.row b={b}" for b in range(16)]
ROW_SHAPES = ["stream.row chunks=1", "stream.row chunks=4", "stream.row chunks=5", "stream.row ends on a chunk",
              "stream.row ends one past a chunk", "stream.row single byte"]
ENC = [f"enc.cb={c}" for c in range(16)] + [f"enc.phase={p} n={n}" for p in range(4) for n in range(1, 11)] + \
      ["enc.have%16=0", "enc.units=8 of 1-byte values", "enc.units=80 of 10-byte values, cb=15", "enc.second store", "enc.len%128=0",
       "enc.len%128=1", "enc.len%128=127", "enc.len odd", "enc.steps=1", "enc.steps=4", "enc.steps=5", "enc.base=16", "enc.base=8"]
REFILLS = [f"seal.refill={R} units={u}" for R in (4064, 8160) for u in (8, 40, 80)]

FULL = {
    "scan encode": LEN_X + [f"lenk.len={L}" for L in (1, 2, 3, 511, 512, 513, 2047, 2048, 2049)] +
                   ["lenk.vector", "lenk.scalar, odd stride", "lenk.scalar, base offset of 8 bytes", "lenk.blocks>1", "lenk.several rows per step",
                    "lenk.pair takes the next row's first element, vector", "lenk.pair takes the next row's first element, scalar",
                    "write.last block shorter than its head", "encscan.chunks=2"] +
                   [f"write.head={h}" for h in range(4)] + [f"write.boff%4={k}" for k in range(4)],
    "scan decode": [f"scan.{k} {e}" for k in ("lane", "halo") for e in STRADDLE] + [f"scan.tail={k}" for k in range(16)] +
                   [f"scan.base={k}" for k in range(16)] + ["scan.dec bytes=4096*1024-1", "scan.dec bytes=4096*1024+0", "scan.dec bytes=4096*1024+1",
                                                            "scan.chunks=2", "scan.zero_entry=1024"],
    "stream decode": [f"stream.{k} {e}" for k in ("lane", "chunk", "group") for e in STRADDLE] + ROW_PHASES + ROW_SHAPES +
                     ["stream.row first n=10", "stream.row first n=10 after 0xff"],
    "slotted decode": [f"stream.{k} {e}" for k in ("lane", "chunk", "group") for e in STRADDLE] + ["stream.row a=0"] + ROW_PHASES[16:] + ROW_SHAPES +
                      ["stream.row first n=10 after 0xff"],
    "stream encode": LEN_X + ENC,
    "sealed encode": LEN_X + ENC + REFILLS,
}
FULL["wire-fed clerk sum"] = [f"stream.{k} {e}" for k in ("lane", "chunk", "group") for e in STRADDLE] + ROW_PHASES + ROW_SHAPES + ["stream.row first n=10"]
FULL["sealed clerk sum"] = [f"stream.{k} {e}" for k in ("lane", "chunk", "group") for e in STRADDLE] + ["stream.row a=0"] + ROW_PHASES[16:] + ROW_SHAPES + \
                           ["stream.row first n=10"]                              # (the bytes in front of a sealed row are its tag)
DAMAGE = ["dmg.unterminated row=1", "dmg.unterminated row=2", "dmg.count+1", "dmg.count-1", "dmg.window empty k=1", "dmg.window empty k=15",
          "dmg.window empty k=6", "legal.ff9 7f"] + [f"{w} {k} s={s}" for w in ("dmg.run11", "legal.run10") for k in ("lane", "chunk", "block") for s in range(1, 11)]


def _same(form, got):
    want = set(FULL[form])
    assert len(want) == len(FULL[form])
    missing, extra = sorted(want - got), sorted(got - want)
    assert not missing, f"{form}: no case reaches {missing[:6]}" + (f" (and {len(missing) - 6} more)" if len(missing) > 6 else "")
    assert not extra, f"{form}: the model names events the list does not hold: {extra[:6]}"


def _all_cases():
    cases = [V.edges_case(), V.seal_rows()] + list(V.encode_steps()) + list(V.phased_rows()) + [c for _, c in V.scan_encode_shapes()]
    cases += [V.straddle_stream(p, p) for p in (16, 1024, 4096)] + [V.short_stream(n) for n in V.TAIL_SIZES]
    return cases


# ---- 1. the fixtures ----------------------------------------------------------------------------------------------------------
def test_length_edges():
    zz = [V.zigzag(v) for v in V.LENGTH_EDGES]
    assert len(zz) == 131 and zz[130] == (1 << 64) - 2 and all(V.I64_MIN <= v <= V.I64_MAX for v in V.LENGTH_EDGES)
    for b in range(65):
        assert zz[2 * b].bit_length() == b and zz[2 * b + 1].bit_length() == b
        assert zz[2 * b] == (1 << b >> 1) and zz[2 * b + 1] == (1 << b) - 1
    assert {V.length_of(v) for v in V.LENGTH_EDGES} == set(range(1, 11))
    assert V.I64_MAX in V.LENGTH_EDGES and V.I64_MIN in V.LENGTH_EDGES
    for n in range(1, 11):                                       # the lower and the upper end of every length
        assert V.length_of(V.value_of_len(n, 0)) == n == V.length_of(V.value_of_len(n, 1))
        assert V.zigzag(V.value_of_len(n, 0)) - 1 in zz + [-1] and V.zigzag(V.value_of_len(n, 1)) in zz


def test_bytes_equal_both_oracles_and_decode_back():
    from oracle import coracle, pyoracle as po
    for case in _all_cases():
        for row, enc in zip(case.rows, case.enc):
            assert all(V.I64_MIN <= v <= V.I64_MAX for v in row), case.name
            arr = np.array(row, dtype=np.int64)
            assert enc == coracle.varint_encode(arr) == po.varint_encode(row), case.name
            assert V.decode(enc) == row == po.varint_decode(enc) == coracle.varint_decode(enc).tolist(), case.name
            assert V.spans(enc) and len(V.spans(enc)) == case.L and max(e - f for f, e in V.spans(enc)) < 10, case.name


def test_big_streams_equal_the_oracles():
    """the 1025-block encode case and the three 4 MiB decode streams: built with numpy, held against the C oracle whole and
    against the Python-integer codec and the Python oracle on their ends and across the 1024-block edge"""
    from oracle import coracle, pyoracle as po
    vals, raw = V.big_encode_case()
    assert vals.size == 2048 * 1024 + 1 == len(raw) and raw == coracle.varint_encode(vals)
    assert V.encode(vals[:300].tolist()) == raw[:300] == po.varint_encode(vals[:300].tolist()) and set(vals.tolist()) == set(range(-64, 64))
    for delta in (-1, 0, 1):
        vals, raw = V.big_decode_case(delta)
        assert len(raw) == 4096 * 1024 + delta and raw == coracle.varint_encode(vals)
        assert np.array_equal(coracle.varint_decode(raw), vals)
        head = 4 + delta
        assert V.decode(raw[:head + 500]) == vals[:51].tolist() == po.varint_decode(raw[:head + 500])
        assert V.decode(raw[-200:]) == vals[-20:].tolist()
        assert np.unique(vals).size == vals.size                 # a value written to another index shows


def test_damage_fixtures():
    from oracle import coracle, pyoracle as po
    cases = V.damage_cases()
    assert sorted(e for d in cases for e in d.events) == sorted(DAMAGE)
    for d in cases:
        rows = [d.raw[d.offsets[r]:d.offsets[r + 1]] for r in range(d.rows)]
        sizes = [e - f + 1 for row in rows for f, e in V.spans(row)]
        if d.bit == V.UNTERMINATED:
            assert any(row[-1] & 0x80 for row in rows) and max(sizes) <= 10, d.name
        elif d.bit == V.ROW_COUNT:
            assert all(len(V.spans(row)) == 40 for row in rows) and abs(d.L - 40) == 1 and not any(row[-1] & 0x80 for row in rows), d.name
        elif d.bit == V.MALFORMED:
            assert sorted(sizes)[-2:] in ([1, 12], [1, 18], [1, 32], [1, 41]) and len(sizes) == d.L and not d.raw[-1] & 0x80, d.name
        else:
            assert max(sizes) == 10 and len(sizes) == d.L and d.values == V.decode(d.raw), d.name
            assert d.values == po.varint_decode(d.raw) == coracle.varint_decode(d.raw).tolist(), d.name
        for ev in d.events:                                      # the run lies where its name says
            if " s=" in ev:
                kind, s = ev.split()[1], int(ev.split("s=")[1])
                f, e = next((f, e) for f, e in V.spans(d.raw) if e - f >= 9)
                assert f == V.DAMAGE_BOUNDARIES[kind] - s and e - f + 1 == (12 if ev.startswith("dmg") else 10), d.name
            if "window empty" in ev:
                k = int(ev.split("k=")[1])
                f, e = next((f, e) for f, e in V.spans(d.raw) if e - f >= 9)
                assert e % 16 == k and e - f >= 16 + k, d.name


def test_builders_place_what_they_claim():
    for period, kinds in ((16, ("scan.lane", "stream.lane")), (1024, ("stream.chunk",)), (4096, ("scan.halo", "stream.group"))):
        case = V.straddle_stream(period, period)
        assert sorted(case.claims) == sorted(STRADDLE)
        ev = V.scan_decode_events(case.raw) | V.stream_decode_events(case.enc, [0])
        for kind in kinds:
            assert {f"{kind} {c}" for c in case.claims} <= ev, (period, kind)
    for case in V.phased_rows():
        assert case.claims <= V.stream_decode_events(case.enc, case.offsets[:-1]), case.name
    assert V.seal_rows().claims <= V.stream_encode_events(V.seal_rows().rows, refills=True)


# ---- 2. reach, per form ---------------------------------------------------------------------------------------------------------
def test_reach_scan_encode():
    ev = V.length_events(V.edges_case().rows)
    for stride, base8 in V.EDGES_ENCODE_LAYOUTS:
        ev |= V.scan_encode_events(1, 131, stride, base8, byte_lens=[V.length_of(v) for v in V.LENGTH_EDGES])
    for shape, case in V.scan_encode_shapes():
        rows, L, stride, base8, _ = shape
        ev |= V.scan_encode_events(rows, L, stride, base8, byte_lens=[V.length_of(v) for r in case.rows for v in r]) | V.length_events(case.rows)
    ev |= V.scan_encode_events(1, 2048 * 1024 + 1, 2048 * 1024 + 1)
    _same("scan encode", ev)


def _decode_stream_events(scan):
    ev = set()
    for case, bases in V.decode_stream_cases():
        for base in bases:
            if scan:
                ev |= V.scan_decode_events(case.raw, base)
            else:
                ev |= V.stream_decode_events(case.enc, case.offsets[:-1], base, before=[base > 0] + [False] * len(case.enc))
    return ev


def test_reach_scan_decode():
    ev = _decode_stream_events(True)
    sizes = V.scan_boundary_sizes()
    for case in sizes["tails"]:
        ev |= V.scan_decode_events(case.raw)
    for delta in sizes["decode"]:
        ev |= V.scan_size_events(4096 * 1024 + delta)
    _same("scan decode", ev)


def test_reach_stream_decode():
    _same("stream decode", _decode_stream_events(False))


def test_reach_wire_fed_clerk_sum():
    ev = set()
    for case, _ in V.decode_stream_cases():
        ev |= V.stream_decode_events(case.enc, case.offsets[:-1])
    _same("wire-fed clerk sum", ev)


def test_reach_slotted_decode():
    ev = set()
    for case in V.slotted_decode_cases():                        # every row at the start of its slot, 0xff before it
        ev |= V.stream_decode_events(case.enc, [0] * len(case.enc), before=[True] * len(case.enc))
    _same("slotted decode", ev)


def test_reach_stream_encode():
    ev = set()
    for case in V.stream_encode_cases():
        ev |= V.length_events(case.rows)
        for pad in V.ENCODE_STRIDE_PADS:
            ev |= V.stream_encode_events(case.rows, V.row_alignments(len(case.rows), case.L, pad))
    _same("stream encode", ev)


def test_reach_sealed_forms():
    enc, dec = set(), set()
    for case in V.sealed_cases():
        enc |= V.length_events(case.rows)
        for pad in V.SEALED_STRIDE_PADS:
            enc |= V.stream_encode_events(case.rows, V.row_alignments(len(case.rows), case.L, pad), refills=True)
        dec |= V.stream_decode_events(case.enc, [0] * len(case.enc))
    _same("sealed encode", enc)
    _same("sealed clerk sum", dec)


# ---- 3. the bit tricks ----------------------------------------------------------------------------------------------------------
def test_division_by_seven():
    assert [V.div7_trick(x) for x in range(7, 71)] == [x // 7 for x in range(7, 71)]
    assert V.div7_trick(71) == 10 and (7 * 36 >> 8, 70 * 36 >> 8) == (0, 9)       # 36 instead of 37 is wrong from the first input on
    for v in V.LENGTH_EDGES:
        assert V.varint_len_trick(V.zigzag(v)) == V.length_of(v)


def test_value_bytes_and_tile_or_at_every_phase():
    for v in V.LENGTH_EDGES + [V.value_of_len(n, k) for n in range(1, 11) for k in range(2, 6)]:
        zz, n = V.zigzag(v), V.length_of(v)
        for phase in range(4):
            tile = [0] * 8
            V.tile_or(tile, phase, 0x7F, 0, 0) if phase else None              # a neighbour's byte in the shared dword
            V.tile_or(tile, phase + 4, *V.value_bytes(zz, n))
            V.tile_or(tile, phase + 4 + n, 0x55, 0, 0)                          # and the next value right behind
            raw = b"".join(w.to_bytes(4, "little") for w in tile)
            assert raw[phase + 4:phase + 4 + n] == V.encode([v]), (v, phase)
            assert raw[phase + 4 + n] == 0x55 and raw[phase + 5 + n:phase + 5 + n + 6] == bytes(6), (v, phase)
            assert all(w <= V.M32 for w in tile)
    assert V.value_bytes(123, 0) == (0, 0, 0)


def test_squeezes_at_every_phase():
    for v in V.LENGTH_EDGES + [V.value_of_len(n, k) for n in range(1, 11) for k in range(2, 6)]:
        enc = V.encode([v])
        for phase in range(4):
            tile = b"\xff" * (16 + phase) + enc + b"\xff" * 16                   # foreign bytes either side
            assert V.tile_value(tile, 16 + phase, len(enc)) == v, (v, phase)
            assert V.scan_squeeze(tile, 16 + phase, len(enc)) == v, (v, phase)
    over = b"\xff" * 9 + b"\x7f"                                                 # the bits above the 64th are dropped
    assert V.tile_value(over + bytes(8), 0, 10) == V.scan_squeeze(over + bytes(8), 0, 10) == V.decode(over)[0] == V.I64_MIN


def test_continuation_bitmap_multiplier():
    rng = np.random.default_rng(5)
    rows = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(200)] + [bytes(16), b"\xff" * 16, b"\x80" + bytes(15), bytes(15) + b"\x80"]
    for raw in rows:
        assert V.cont_bits16(raw) == sum((b >> 7) << k for k, b in enumerate(raw))

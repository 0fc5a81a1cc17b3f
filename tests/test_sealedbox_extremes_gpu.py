"""The sealed-box kernels at the limits of their limb arithmetic (the device side of tests/test_sbox_model.py): edge scalars
and edge u-coordinates through x25519_quad in both setup kernels, every low-order encoding refused by open and by seal, chosen
ciphertexts under real keys, and - through the test-only sda_debug_poly1305_rows_dev of libsda_hip_test.so - Poly1305 with a
CHOSEN r and s through the production sbox_poly_kernel / sbox_final_kernel: r = 0, 1, 2, all clamped bits; s = 0, 2^128 - 1;
h through p - 1, p, 2^130 - 1; and the messages of sbox_model.limb_extreme_message, which put 2^26 - 1 into every limb of every
lane so that the 64-lane uint32_t sums are 2^32 - 64 and the carry behind them 2^32 - 1.  Everything is byte-exact against
oracle/sealedbox_oracle.py (big-int X25519 and Poly1305) and Python integers."""
import ctypes as C
import random

import numpy as np
import pytest

import sbox_model as S

pytestmark = pytest.mark.gpu
P = S.P25519
SK = bytes(range(41, 73))
MSG = b"shares of a clerking job, forty-one bytes"


def _rb(seed):
    rng = random.Random(seed)
    return lambda n: bytes(rng.getrandbits(8) for _ in range(n))


def _slotted(rows_bytes, slot, fill=0):
    blob = bytearray([fill]) * (len(rows_bytes) * slot)
    for r, b in enumerate(rows_bytes):
        blob[r * slot:r * slot + len(b)] = b
    return blob


def _open_rows(pk, sk, boxes, fill=0xC3):
    """-> (ok flags, lengths, output slots, status) of one open_rows_dev call over `boxes`"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    rows = len(boxes)
    longest = max(len(b) for b in boxes)
    slot = (longest + 15) // 16 * 16 + 16
    out_slot = (max(longest - 48, 0) + 15) // 16 * 16 + 16
    d_boxes = DeviceBytes.from_bytes(_slotted(boxes, slot))
    d_lens = DeviceBytes.from_bytes(np.array([len(b) for b in boxes], dtype="<u8").tobytes())
    d_out, d_nb = DeviceBytes.from_bytes(bytes([fill]) * (rows * out_slot)), DeviceBytes(rows * 8).zero()
    d_ok, d_status = DeviceBytes(rows * 4).zero(), DeviceBytes(4).zero()
    crypto.SealedBox().open_rows_dev(pk, sk, d_boxes.ptr, slot, d_lens.ptr, rows, longest, d_out.ptr, out_slot, d_nb.ptr, d_status.ptr, d_ok.ptr)
    ob = d_out.to_bytes()
    return (list(np.frombuffer(d_ok.to_bytes(), dtype="<u4")), list(np.frombuffer(d_nb.to_bytes(), dtype="<u8")),
            [ob[r * out_slot:(r + 1) * out_slot] for r in range(rows)], int(np.frombuffer(d_status.to_bytes(), dtype="<u4")[0]))


def _seal_rows(pks, msgs, esks, fill=0x3C):
    """-> (box lengths, box slots) of one seal_rows_dev call: row r to pks[r] (one row per key)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    rows = len(msgs)
    longest = max(len(m) for m in msgs)
    mslot = (longest + 15) // 16 * 16 + 16
    bslot = (longest + 48 + 15) // 16 * 16
    d_msgs = DeviceBytes.from_bytes(_slotted(msgs, mslot))
    d_mlen = DeviceBytes.from_bytes(np.array([len(m) for m in msgs], dtype="<u8").tobytes())
    d_boxes, d_blen = DeviceBytes.from_bytes(bytes([fill]) * (rows * bslot)), DeviceBytes(rows * 8).zero()
    crypto.SealedBox().seal_rows_dev(pks, 1, d_msgs.ptr, mslot, d_mlen.ptr, rows, longest, d_boxes.ptr, bslot, d_blen.ptr, esk=b"".join(esks))
    bb = d_boxes.to_bytes()
    return list(np.frombuffer(d_blen.to_bytes(), dtype="<u8")), [bb[r * bslot:(r + 1) * bslot] for r in range(rows)]


def _forge(so, epk, pk, shared, m):
    """a box with the chosen first 32 bytes whose tag verifies under the given shared secret"""
    return epk + so.secretbox(m, so.seal_nonce(epk, pk), so.hsalsa20(shared, bytes(16)))


def test_public_keys_of_edge_scalars(gpu):
    """first quad of the seal setup: scalars whose ladders are runs of swaps / no swaps"""
    from sda_amd import crypto
    from oracle import sealedbox_oracle as so
    box = crypto.SealedBox()
    for name, sk in S.edge_scalars().items():
        assert box.public_key(sk) == so.x25519_base(sk), name


def test_boxes_forged_at_edge_points_open(gpu):
    """x25519_quad with a chosen point: epk = 2, 9, 9 + 2^255, p + k (k = 2 .. 18), p - 2, one saturated limb, the nine limb
    boundaries - one call, so neighbouring quads of a wave carry different points"""
    from oracle import sealedbox_oracle as so
    pk = so.x25519_base(SK)
    pts = S.edge_points()
    assert len(pts) == 4 + 17 + 10 + 27
    for k in range(2, 19):                                            # non-canonical: must behave as u = k; bit 255 is ignored
        assert so.x25519(SK, pts["p+%d" % k]) == so.x25519(SK, k.to_bytes(32, "little"))
    assert so.x25519(SK, pts["9+2^255"]) == so.x25519(SK, pts["9"])
    names = list(pts)
    msgs = [MSG + n.encode() for n in names]
    boxes = [_forge(so, pts[n], pk, so.x25519(SK, pts[n]), m) for n, m in zip(names, msgs)]
    for b, m in zip(boxes, msgs):
        assert so.seal_open(b, pk, SK) == m
    ok, nb, out, status = _open_rows(pk, SK, boxes)
    assert status == 0 and ok == [1] * len(boxes), [n for n, o in zip(names, ok) if not o]
    for n, m, o, l in zip(names, msgs, out, nb):
        assert l == len(m) and o[:len(m)] == m, n


def test_sealing_to_edge_points_equals_the_oracle(gpu):
    """the second quad of the seal setup (the recipient-key ladder) with the same values as recipient keys, injected ephemeral
    secrets, one key per row"""
    from oracle import sealedbox_oracle as so
    pts = S.edge_points()
    names = list(pts)
    rb = _rb(77)
    esks = [rb(32) for _ in names]
    edge = list(S.edge_scalars().values())
    esks[:len(edge)] = edge                                           # ... and edge scalars against edge points
    msgs = [MSG + n.encode() for n in names]
    lens, boxes = _seal_rows([pts[n] for n in names], msgs, esks)
    for n, m, e, l, b in zip(names, msgs, esks, lens, boxes):
        assert l == len(m) + 48 and b[:l] == so.seal(m, pts[n], e), n


def _low_order_encodings():
    """every 32-byte string below 2^255 that X25519 maps to zero, DERIVED: multiply random x-coordinates by the odd part of the
    order of the curve (8 L) or of its twist (4 L') with a plain Montgomery ladder; what is left has order dividing 8; the
    non-canonical encodings x + p are added where they fit in 255 bits"""
    L = 2**252 + 27742317777372353535851937790883648493
    Lt = (2 * P + 2 - 8 * L) // 4
    assert (2 * P + 2 - 8 * L) % 4 == 0

    def ladder(n, x1):
        x2, z2, x3, z3 = 1, 0, x1, 1
        for t in range(n.bit_length() - 1, -1, -1):
            bit = (n >> t) & 1
            if bit:
                x2, z2, x3, z3 = x3, z3, x2, z2
            A, B, Cc, D = x2 + z2, x2 - z2, x3 + z3, x3 - z3
            E = A * A - B * B
            x3, z3 = (D * A + Cc * B) ** 2 % P, x1 * (D * A - Cc * B) ** 2 % P
            x2, z2 = A * A * B * B % P, E * (A * A + 121665 * E) % P
            if bit:
                x2, z2, x3, z3 = x3, z3, x2, z2
        return None if z2 == 0 else x2 * pow(z2, P - 2, P) % P
    rng = random.Random(8)
    xs = set()
    for _ in range(200):
        x = rng.randrange(2, P)
        on_curve = pow((x * x * x + 486662 * x * x + x) % P, (P - 1) // 2, P) == 1
        r = ladder(L if on_curve else Lt, x)
        if r is not None:
            xs.add(r)
    return sorted({x + k * P for x in xs for k in (0, 1) if x + k * P < 2**255})


def test_every_low_order_encoding_is_refused_by_open_and_by_seal(gpu):
    from oracle import sealedbox_oracle as so
    rb = _rb(13)
    cands = _low_order_encodings()
    low = [u for u in cands if so.x25519(SK, u.to_bytes(32, "little")) == bytes(32) == so.x25519(rb(32), u.to_bytes(32, "little"))]
    assert low == cands and len(low) == 7 and {0, 1, P - 1, P, P + 1} <= set(low)
    encodings = [u.to_bytes(32, "little") for u in low] + [(u | 1 << 255).to_bytes(32, "little") for u in low]
    pk = so.x25519_base(SK)
    # open: a forged box whose tag verifies under the all-zero shared secret, good boxes around each of them
    boxes, want = [], []
    for i, e in enumerate(encodings):
        boxes.append(so.seal(MSG + bytes([i]), pk, rb(32))); want.append(MSG + bytes([i]))
        boxes.append(_forge(so, e, pk, bytes(32), MSG)); want.append(None)
        with pytest.raises(ValueError):
            so.seal_open(boxes[-1], pk, SK)
    boxes.append(so.seal(MSG, pk, rb(32))); want.append(MSG)
    ok, nb, out, status = _open_rows(pk, SK, boxes)
    assert status == 16 and ok == [0 if w is None else 1 for w in want]
    for r, w in enumerate(want):
        if w is None:
            assert nb[r] == 0 and out[r] == b"\xC3" * len(out[r]), r          # nothing written for a refused box
        else:
            assert nb[r] == len(w) and out[r][:len(w)] == w, r
    # seal: row length 0, nothing encrypted, the good keys around unaffected
    good = [so.x25519_base(rb(32)) for _ in range(3)]
    pks, esks = [], []
    for i, e in enumerate(encodings):
        pks += [good[i % 3], e]
    pks.append(good[0])
    esks = [rb(32) for _ in pks]
    msgs = [MSG + bytes([r]) for r in range(len(pks))]
    lens, sealed = _seal_rows(pks, msgs, esks)
    for r, k in enumerate(pks):
        if k in encodings:
            assert lens[r] == 0 and sealed[r][32:] == b"\x3C" * (len(sealed[r]) - 32), r
        else:
            assert lens[r] == len(msgs[r]) + 48 and sealed[r][:lens[r]] == so.seal(msgs[r], k, esks[r]), r


CT_LENGTHS = [0, 1, 15, 16, 17, 16 * 64 - 1, 16 * 64, 16 * 64 + 1, 16384 - 16, 16384 - 1, 16384, 16384 + 1, 16384 + 16,
              2 * 16384 - 1, 2 * 16384, 2 * 16384 + 1, 3 * 16384 - 1, 3 * 16384, 3 * 16384 + 1]


def test_chosen_ciphertexts_under_real_keys(gpu):
    """boxes whose CIPHERTEXT is all 0xFF / all 0x00 / the limb-extreme pattern, tag by the oracle, very different lengths in one
    call (used < regions for most rows): rows open to ct xor keystream; with one tag bit flipped they are refused and the
    output slot stays as it was"""
    from oracle import sealedbox_oracle as so
    rb = _rb(21)
    pk = so.x25519_base(SK)
    boxes, want = [], []
    for n in CT_LENGTHS:
        for ct in (b"\xff" * n, bytes(n), S.limb_extreme_message(n)):
            epk = so.x25519_base(rb(32))
            stream = so.xsalsa20_stream(so.hsalsa20(so.x25519(SK, epk), bytes(16)), so.seal_nonce(epk, pk), 32 + n)
            boxes.append(epk + so.poly1305(stream[:32], ct) + ct)
            want.append((np.frombuffer(ct, dtype=np.uint8) ^ np.frombuffer(stream[32:], dtype=np.uint8)).tobytes())
    for r in (0, 4, len(boxes) - 1):
        assert so.seal_open(boxes[r], pk, SK) == want[r]
    ok, nb, out, status = _open_rows(pk, SK, boxes)
    assert status == 0 and ok == [1] * len(boxes), [len(w) for w, o in zip(want, ok) if not o]
    for r, w in enumerate(want):
        assert nb[r] == len(w) and out[r][:len(w)] == w, (r, len(w))
    bad = []
    for r, b in enumerate(boxes):
        b = bytearray(b); b[32 + r % 16] ^= 1 << (r % 8); bad.append(bytes(b))
    ok, nb, out, status = _open_rows(pk, SK, bad)
    assert status == 16 and ok == [0] * len(bad) and nb == [0] * len(bad)
    assert all(o == b"\xC3" * len(o) for o in out)


# ---- Poly1305 with a chosen one-time key: the production poly / final kernels behind the test-only entry point ------------
def _device_tags(keys, msgs, max_msg=None):
    from sda_amd import capi
    from sda_amd.device import DeviceBytes
    rows = len(msgs)
    longest = max(len(m) for m in msgs) if max_msg is None else max_msg
    slot = (longest + 15) // 16 * 16 + 16
    d_msgs = DeviceBytes.from_bytes(_slotted(msgs, slot, fill=0xA5))           # bytes past a message's end are not zero
    d_lens = DeviceBytes.from_bytes(np.array([len(m) for m in msgs], dtype="<u8").tobytes())
    tags = C.create_string_buffer(16 * rows)
    capi.check(capi.hooks_library().sda_debug_poly1305_rows_dev(b"".join(keys), d_msgs.ptr, slot, d_lens.ptr, rows, longest, tags))
    return [tags.raw[16 * r:16 * r + 16] for r in range(rows)]


def _poly_cases():
    p = S.P1305
    rb = _rb(1305)
    s_values = (bytes(16), b"\xff" * 16)
    r_values = (bytes(16), (1).to_bytes(16, "little"), (2).to_bytes(16, "little"), b"\xff" * 16)
    cases = []
    for s16 in s_values:
        for r16 in r_values:
            for m in (b"", b"\x00", b"\xff" * 15, b"\xff" * 16, bytes(17), b"\xff" * 1024, rb(3072), b"\xff" * 16385, bytes(16384), rb(40000)):
                cases.append((r16 + s16, m))
        # the limb-extreme messages: one lane, 64 lanes, one full region, three regions and a ragged head, tails
        for n in (48, 3072, 16384, 3 * 16384 + 5007, 2 * 16384 + 3072):
            cases.append((S.KEY_R1(s16), S.limb_extreme_message(n)))
        for tail in range(1, 16):
            cases.append((S.KEY_R1(s16), S.limb_extreme_message(3072 + tail)))
    # h through p - 1, p, p + 1, 2^130 - 1 (and 2^130) before the final reduction: r = 1, three pieces summing to the target
    for target in (p - 1, p, p + 1, p + 4, p + 5):
        rest = target - 3 * 2**128
        m1 = min(rest, 2**128 - 1); m2 = min(rest - m1, 2**128 - 1); m3 = rest - m1 - m2
        msg = b"".join(m.to_bytes(16, "little") for m in (m1, m2, m3))
        for s in (0, 2**128 - 1, (2**128 - target % p) % 2**128, (2**128 - 1 - target % p) % 2**128):
            cases.append((S.KEY_R1(s.to_bytes(16, "little")), msg))
    return cases


def test_poly1305_kernels_with_chosen_r_and_s(gpu):
    cases = _poly_cases()
    keys, msgs = [k for k, _ in cases], [m for _, m in cases]
    want = [S.poly1305_bigint(k, m) for k, m in cases]
    # all rows in one call: the launch is sized for the longest, so most rows use fewer regions than it has
    got = _device_tags(keys, msgs)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, (r, keys[r].hex(), len(msgs[r]))
    # the longest and the limb-extreme rows alone, in launches sized for themselves
    for r in [i for i, m in enumerate(msgs) if len(m) in (48, 3072, 16384, 3 * 16384 + 5007)]:
        assert _device_tags([keys[r]], [msgs[r]]) == [want[r]], (r, len(msgs[r]))
    # a launch sized far beyond every row
    short = [i for i, m in enumerate(msgs) if len(m) <= 3072]
    assert _device_tags([keys[i] for i in short], [msgs[i] for i in short], max_msg=5 * 16384) == [want[i] for i in short]

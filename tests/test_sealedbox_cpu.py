"""Host unit test of sda_amd/csrc/sbox_primitives.hpp - the header the sealed-box kernels are built from - compiled
with g++ and compared with the published vectors (tests/golden/sealedbox.json) and the oracle on random operands.
(The kernels themselves are covered by tests/test_sealedbox_gpu.py; this catches arithmetic slips without a GPU.)
The raw primitives are driven on explicit limbs at the operand bounds tests/test_sbox_model.py proves, and Poly1305 is
evaluated in the device's order by the harness's own restatement (command polydev); expected values are Python integers.
Every command list runs twice: through the -O2 build and through one built with -fsanitize=undefined."""
import hashlib
import os
import random
import subprocess

import pytest

from conftest import load_golden
from oracle import sealedbox_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sbox") / "sbox_primitives_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "sbox_primitives_test.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def exe_ubsan(tmp_path_factory):
    """the same harness with the undefined-behaviour sanitizer (host code): a signed overflow in 19 * g or a shift of a
    negative carry ends the run instead of passing by luck"""
    out = str(tmp_path_factory.mktemp("sbox_ub") / "sbox_primitives_test_ubsan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror",
                           "-fsanitize=undefined", "-fno-sanitize-recover",
                           os.path.join(ROOT, "tests", "cpp", "sbox_primitives_test.cpp"), "-o", out])
    return out


@pytest.fixture(params=["O2", "ubsan"])
def harness(request, exe, exe_ubsan):
    return exe if request.param == "O2" else exe_ubsan


def _run(exe, cmds):
    out = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout.split()


def _published_and_oracle_commands():
    g = load_golden("sealedbox.json")["kats"]
    rng = random.Random(1)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    cmds, want = [], []
    for v in g["x25519"]:
        cmds.append(f"x25519 {v['scalar']} {v['u']}"); want.append(v["out"])
    for v in g["x25519_base"]:
        cmds.append(f"x25519 {v['scalar']} {(9).to_bytes(32, 'little').hex()}"); want.append(v["out"])
    for v in g["hsalsa20"]:
        cmds.append(f"hsalsa {v['key']} {v['in']}"); want.append(v["out"])
    for v in g["poly1305"]:
        cmds.append(f"poly {v['key']} {v['msg']}"); want.append(v["tag"])
    for _ in range(12):
        k, u = rb(32), rb(32)
        cmds.append(f"x25519 {k.hex()} {u.hex()}"); want.append(so.x25519(k, u).hex())
    for u in (bytes(32), (1).to_bytes(32, "little"), (2**255 - 19).to_bytes(32, "little"), b"\xff" * 32,
              (2**255 - 20).to_bytes(32, "little")):                       # edge u-coordinates, incl. non-canonical ones
        k = rb(32)
        cmds.append(f"x25519 {k.hex()} {u.hex()}"); want.append(so.x25519(k, u).hex())
    for ctr in (0, 1, 2**32 - 1, 2**32, 2**40 + 7):
        k, n = rb(32), rb(8)
        cmds.append(f"salsa {k.hex()} {n.hex()} {ctr}"); want.append(so.salsa20_stream(k, n, 64, ctr).hex())
    for _ in range(5):
        e, p = rb(32), rb(32)
        cmds.append(f"nonce {e.hex()} {p.hex()}"); want.append(hashlib.blake2b(e + p, digest_size=24).digest().hex())
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 100, 1000):
        k, m = rb(32), rb(n)
        cmds.append(f"poly {k.hex()} {m.hex() or '-'}"); want.append(so.poly1305(k, m).hex())
    cmds.append(f"poly {'ff' * 32} {'ff' * 64}"); want.append(so.poly1305(b"\xff" * 32, b"\xff" * 64).hex())
    return cmds, want


def test_header_primitives_match_published_vectors_and_the_oracle(exe):
    cmds, want = _published_and_oracle_commands()
    got = _run(exe, cmds)
    assert len(got) == len(want)
    for c, a, b in zip(cmds, got, want):
        assert a == b, c[:40]


def test_header_primitives_under_the_undefined_behaviour_sanitizer(exe_ubsan):
    cmds, want = _published_and_oracle_commands()
    assert _run(exe_ubsan, cmds) == want


# ---- the raw primitives on explicit limbs ------------------------------------------------------------------------
P25519, P1305, M26 = 2**255 - 19, 2**130 - 5, 2**26 - 1
_csv = lambda v: ",".join(str(x) for x in v)
_limbs = lambda tok: [int(x) for x in tok.split(",")]


def _fe_operands():
    """limbs at +- the proven operand bounds (tests/test_sbox_model.py): what two carried elements add up to, and the widest
    fe_mul takes (19 g_i in int32_t), in every position and sign pattern"""
    import sbox_model as S
    rng = random.Random(19)
    ladder = [2 * c for c in S.FE_CARRIED]
    ops = []
    for bound in (ladder, [S.FE_G_MAX] * 10):
        for sign in ((1,) * 10, (-1,) * 10, (1, -1) * 5, (-1, 1) * 5):
            ops.append([s * b for s, b in zip(sign, bound)])
        for i in range(10):
            for sg in (1, -1):
                ops.append([sg * bound[j] if j == i else rng.randrange(-3, 4) for j in range(10)])
    ops += [[rng.randrange(-b, b + 1) for b in ladder] for _ in range(10)]
    return ops


def _spell(v, signs):
    """ten limbs of value v: limb i < 9 takes the remainder in [0, 2^bits) (sign +) or in (-2^bits, 0] (sign -), limb 9 the rest"""
    import sbox_model as S
    h = []
    for i in range(9):
        b = 1 << S.fe_bits(i)
        r = v % b
        if signs[i] < 0 and r:
            r -= b
        h.append(r); v = (v - r) >> S.fe_bits(i)
    h.append(v)
    assert S.fe_value(h) == sum(x << S.FE_OFF[i] for i, x in enumerate(h)) and abs(h[9]) < 2**27
    return h


def test_field_primitives_on_raw_limbs_at_the_operand_bounds(harness):
    import sbox_model as S
    ops = _fe_operands()
    cmds, want = [], []
    partners = ops[:8] + ops[-3:]
    for f in ops:
        cmds.append(f"fesq {_csv(f)}"); want.append(("fe", S.fe_value(f) ** 2 % P25519, S.fe_sq(f)))
        for g in partners:
            cmds.append(f"femul {_csv(f)} {_csv(g)}"); want.append(("fe", S.fe_value(f) * S.fe_value(g) % P25519, S.fe_mul(f, g)))
    rng = random.Random(62)
    cols = [[s * (2**62 - 1) for s in sign] for sign in ((1,) * 10, (-1,) * 10, (1, -1) * 5, (-1, 1) * 5)]
    cols += [[(2**62 - 1) * sg if j == i else 0 for j in range(10)] for i in range(10) for sg in (1, -1)]
    cols += [[2**25, 2**24, 2**25, 2**24, 2**25, 2**24, 2**25, 2**24, 2**25, 2**24], [2**25 - 1, 2**24 - 1] * 5, [-2**25 - 1, -2**24 - 1] * 5]
    cols += [[rng.randrange(-2**61, 2**61) for _ in range(10)] for _ in range(20)]
    for h in cols:
        cmds.append(f"fecarry {_csv(h)}"); want.append(("fe", S.fe_value(h) % P25519, S.fe_carry(h)))
    # canonical bytes: representatives of the edge values, spelt with minimal and with maximally unbalanced limbs
    p = P25519
    for v in (p - 1, p, p + 1, 2 * p - 1, -1, -p, 0, 2**255 - 1, 19, 18, -19, 2**255 - 20 + p):
        for signs in ((1,) * 9, (-1,) * 9, (1, -1) * 4 + (1,), (-1, 1) * 4 + (-1,)):
            cmds.append(f"fewords {_csv(_spell(v, signs))}"); want.append(("bytes", (v % p).to_bytes(32, "little").hex()))
    for f in ops[:8]:                                                 # ... and of products at the operand bounds
        cmds.append(f"fewords {_csv(S.fe_sq(f))}"); want.append(("bytes", (S.fe_value(f) ** 2 % p).to_bytes(32, "little").hex()))
    got = _run(harness, cmds)
    assert len(got) == len(want)
    for c, a, w in zip(cmds, got, want):
        if w[0] == "bytes":
            assert a == w[1], c
            continue
        h = _limbs(a)
        assert S.fe_value(h) % P25519 == w[1], c                      # the value, from Python integers
        for i, x in enumerate(h):                                     # the ranges the header states for fe_carry
            half = 1 << (S.fe_bits(i) - 1)
            assert (-half - 1 <= x <= half) if i == 1 else (-half <= x < half), (c, i, x)
        assert h == w[2], c                                           # and limb for limb what the width-checked model gives


def test_poly1305_primitives_on_raw_limbs(harness):
    import sbox_model as S
    rng = random.Random(26)
    A, B = S.MUL_A_MAX, S.MUL_B_MAX
    cmds, want = [], []
    avals = [[A] * 5, [0] * 5, [M26] * 5, [A, 0, A, 0, A], [0, A, 0, A, 0]] + [[A if j == i else 0 for j in range(5)] for i in range(5)]
    bvals = [[B] * 5, [M26] * 5, [1, 0, 0, 0, 0], [0] * 5, [B, 0, B, 0, B]] + [[B if j == i else 1 for j in range(5)] for i in range(5)]
    avals += [[rng.randrange(A + 1) for _ in range(5)] for _ in range(10)]
    bvals += [[rng.randrange(B + 1) for _ in range(5)] for _ in range(10)]
    for a in avals:
        for b in bvals:
            cmds.append(f"p26mul {_csv(a)} {_csv(b)}"); want.append(("p26", S.p26_value(a) * S.p26_value(b) % P1305, S.p26_mul(a, b), S.MUL_OUT1_MAX))
    top = S.CARRY_IN_MAX
    carries = [[2**26 - 5, M26, M26, M26, 2**26], [top] * 5, [2**32 - 1, top, top, top, top], [M26] * 5, [0] * 5, [M26, M26 + 51, M26, M26, M26]]
    carries += [[top if j == i else 0 for j in range(5)] for i in range(5)] + [[rng.randrange(top + 1) for _ in range(5)] for _ in range(20)]
    for h in carries:
        cmds.append(f"p26carry {_csv(h)}"); want.append(("p26", S.p26_value(h) % P1305, S.p26_carry(h), M26 + 1))
    spell = lambda v: [(v >> (26 * i)) & M26 for i in range(5)]
    for v in (P1305 - 1, P1305, P1305 + 1, P1305 + 4, 0, 4, 5, 2**128 - 1, 2**128):
        hs = [spell(v)]
        if hs[0][2]:
            hs.append([hs[0][0], hs[0][1] + 2**26, hs[0][2] - 1, hs[0][3], hs[0][4]])       # partially reduced: excess in limb 1
        hs.append([x + y for x, y in zip(spell(v), [M26, 2**26, M26, M26, M26])])             # an accumulator before p26_finish: + carried sums
        for h in hs:
            hv = S.p26_value(h)
            for s in (0, 2**128 - 1, (2**128 - hv % P1305) % 2**128, (2**128 - 1 - hv % P1305) % 2**128, 2**96):
                cmds.append(f"p26finish {_csv(h)} {s.to_bytes(16, 'little').hex()}")
                want.append(("bytes", ((hv % P1305 + s) % 2**128).to_bytes(16, "little").hex()))
    got = _run(harness, cmds)
    assert len(got) == len(want)
    for c, a, w in zip(cmds, got, want):
        if w[0] == "bytes":
            assert a == w[1], c
            continue
        h = _limbs(a)
        assert S.p26_value(h) % P1305 == w[1], c
        assert all(h[i] <= M26 for i in (0, 2, 3, 4)) and h[1] <= w[3], c
        assert h == w[2], c


def test_poly1305_in_the_device_order_on_the_host(harness):
    """polydev: the lane / step / region decomposition of the kernels, composed from the compiled header"""
    import sbox_model as S
    rng = random.Random(64)
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    cases = []
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 16383, 16384, 16385, 16400, 32768, 32769, 3 * 16384 + 5007):
        cases.append((rb(32), rb(n), 0))
    cases += [(rb(32), rb(n), 5) for n in (0, 7, 16384, 20000)]                      # used < regions
    for s16 in (bytes(16), b"\xff" * 16):
        for n in (48, 3072, 16384, 3 * 16384 + 5007):
            cases.append((S.KEY_R1(s16), S.limb_extreme_message(n), 0))
        for tail in range(1, 16):
            cases.append((S.KEY_R1(s16), S.limb_extreme_message(3072 + tail), 0))
            cases.append((S.KEY_RMAX(s16), b"\xff" * (16384 + tail), 0))
        for key in (bytes(16) + s16, (2).to_bytes(16, "little") + s16, S.KEY_RMAX(s16)):
            for fill in (b"\xff", b"\x00"):
                cases.append((key, fill * 20000, 0))
    cmds = [f"polydev {k.hex()} {m.hex() or '-'} {g}" for k, m, g in cases]
    got = _run(harness, cmds)
    assert len(got) == len(cases)
    for (k, m, g), a in zip(cases, got):
        assert a == S.poly1305_bigint(k, m).hex() == so.poly1305(k, m).hex(), (k.hex(), len(m), g)

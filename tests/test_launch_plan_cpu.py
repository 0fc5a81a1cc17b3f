"""Host unit test of sda_amd/csrc/launch_plan.hpp - the participant-slice loop and the ChaCha round-count dispatch that every
share-generation launcher goes through - compiled with g++ and compared with Python integers (CPU; the slice arithmetic only
comes into play above 2^24 workgroups per launch, which no GPU test can afford).  tests/cpp/launch_plan_test.cpp binds the loop's
callable to a recorder; it is built twice, -O2 and -O1 with the undefined-behaviour sanitizer, and both run as child processes on
the same lines.

Cases: both block caps; blocks_per_participant in {0, 1, 2, cap/2, cap/2 + 1, cap - 1, cap, cap + 1}; participants in
{0, 1, 2, per - 1, per, per + 1, 2 per + 1} for per = cap // blocks_per_participant, plus one count above 2^32.  Slices number
participants / per, so that count stays at a few hundred slices only where per is large: it goes with the blocks_per_participant
whose per is at least 2^22 (1 and 2 under either cap), and with the two that make no slice at all (0 and cap + 1)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "launch_plan_test.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include")]
CAPS = {"sda_kernels": 0xFFFFFFFF // 256, "fft_ngemm": 0x7FFFFFFF}
BIG = (1 << 32) + 5
SECRETS_STRIDE, RAND_STRIDE, OUT_STRIDE = 3, 7, 5           # the layout of launch_plan_test.cpp's `loop`


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lplan") / "launch_plan_test")
    subprocess.check_call(["g++", "-O2"] + WARN + [SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def exe_ubsan(tmp_path_factory):
    """the same program with the undefined-behaviour sanitizer (host code): a product, a cast or a pointer step that overflows
    ends the run instead of passing by luck"""
    out = str(tmp_path_factory.mktemp("lplan_ub") / "launch_plan_test_ubsan")
    subprocess.check_call(["g++", "-O1", "-g"] + WARN + ["-fsanitize=undefined", "-fno-sanitize-recover", SRC, "-o", out])
    return out


@pytest.fixture(params=["O2", "ubsan"])
def harness(request, exe, exe_ubsan):
    return exe if request.param == "O2" else exe_ubsan


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    head = got[0].split()
    assert head[0] == "codes" and len(got) == len(lines) + 1
    codes = dict(zip(("ok", "invalid_value", "invalid_configuration", "recorder"), map(int, head[1:])))
    assert codes["ok"] == 0 and len(set(codes.values())) == 4
    return codes, got[1:]


def _shapes():
    """(cap, blocks_per_participant, participants) of the module docstring"""
    shapes = []
    for cap in CAPS.values():
        for bpp in (0, 1, 2, cap // 2, cap // 2 + 1, cap - 1, cap, cap + 1):
            per = cap // bpp if 0 < bpp <= cap else None
            counts = {0, 1, 2} | ({per - 1, per, per + 1, 2 * per + 1} if per else set())
            if per is None or per >= 1 << 22:
                counts.add(BIG)
            shapes += [(cap, bpp, p) for p in sorted(counts)]
    return shapes


def _slices(cap, bpp, participants):
    """what the loop must do: None = refused, else the list of (p0, count)"""
    if bpp == 0 or participants == 0:
        return []
    if bpp > cap:
        return None
    per = min(cap // bpp, participants)
    return [(p0, min(per, participants - p0)) for p0 in range(0, participants, per)]


def _parse(line, fields):
    t = line.split()
    calls = [tuple(int(x) for x in c.split(":")) for c in t[2:]]
    assert int(t[1]) == len(calls) and all(len(c) == fields for c in calls)
    return int(t[0]), calls


def _check_cover(cap, bpp, participants, calls):
    """contiguous, in order, [0, participants) exactly once; within the cap and unsigned; all but the last of the full size"""
    at = 0
    for i, (p0, count, blocks) in enumerate(calls):
        assert p0 == at and count >= 1 and blocks == bpp * count
        assert blocks <= cap and blocks < 1 << 32
        if i + 1 < len(calls):
            assert count == min(cap // bpp, participants)
        at += count
    assert at == participants


def test_shapes_hold_what_they_are_named_for():
    shapes = _shapes()
    assert all(len(_slices(*s) or []) < 3000 for s in shapes)
    assert max(len(_slices(*s) or []) for s in shapes) > 100                       # ... and many slices are among them
    for cap in CAPS.values():
        mine = [s for s in shapes if s[0] == cap]
        assert {b for _, b, _ in mine} == {0, 1, 2, cap // 2, cap // 2 + 1, cap - 1, cap, cap + 1}
        assert any(p > 1 << 32 and _slices(c, b, p) for c, b, p in mine)           # the count above 2^32 is really sliced
        assert any(_slices(*s) is None for s in mine) and any(_slices(*s) == [] for s in mine)
        for b in (1, 2, cap // 2, cap // 2 + 1, cap - 1, cap):
            per = cap // b
            assert {p for _, bb, p in mine if bb == b} >= {0, 1, 2, per - 1, per, per + 1, 2 * per + 1}


@pytest.mark.parametrize("with_rand", [0, 1])
def test_slices_cover_the_participants_within_the_cap(harness, with_rand):
    shapes = _shapes()
    codes, got = _run(harness, [f"loop {c} {b} {p} {with_rand} -1" for c, b, p in shapes])
    for (cap, bpp, participants), line in zip(shapes, got):
        ret, calls = _parse(line, 7)
        want = _slices(cap, bpp, participants)
        if want is None:                                                           # one participant alone exceeds the cap
            assert ret == codes["invalid_configuration"] and calls == [], (cap, bpp, participants, line[:200])
            continue
        assert ret == codes["ok"]
        if not want:
            assert calls == []                                                     # nothing to do: no call
            continue
        _check_cover(cap, bpp, participants, [c[:3] for c in calls])
        assert [c[:2] for c in calls] == want
        for p0, _, _, secrets, rand, out, same in calls:                           # slice(): every pointer by p0 times its stride
            assert secrets == p0 * SECRETS_STRIDE and out == p0 * OUT_STRIDE and same == 1
            assert rand == (p0 * RAND_STRIDE if with_rand else -1)                 # a null rand stays null


def test_ranges_are_the_same_cut(harness):
    """the pointer-and-stride callers' form (launch_drbg_fill, launch_fill_synthetic)"""
    shapes = _shapes()
    codes, got = _run(harness, [f"range {c} {b} {p} -1" for c, b, p in shapes])
    for (cap, bpp, participants), line in zip(shapes, got):
        ret, calls = _parse(line, 3)
        want = _slices(cap, bpp, participants)
        assert ret == (codes["invalid_configuration"] if want is None else codes["ok"])
        assert [c[:2] for c in calls] == (want or [])
        if want:
            _check_cover(cap, bpp, participants, calls)


@pytest.mark.parametrize("form", ["loop", "range"])
def test_a_failing_launch_ends_the_loop(harness, form):
    cases = []
    for cap, bpp, participants in _shapes():
        n = len(_slices(cap, bpp, participants) or [])
        cases += [(cap, bpp, participants, i, n) for i in sorted({0, n // 2, n - 1}) if 0 <= i < n]
    assert any(n > 100 and 0 < i < n - 1 for *_, i, n in cases)
    codes, got = _run(harness, [f"{form} {c} {b} {p} {'1 ' if form == 'loop' else ''}{i}" for c, b, p, i, _ in cases])
    for (cap, bpp, participants, i, _), line in zip(cases, got):
        ret, calls = _parse(line, 7 if form == "loop" else 3)
        assert ret == codes["recorder"] and len(calls) == i + 1, (cap, bpp, participants, i, line[:200])
        assert [c[:2] for c in calls] == _slices(cap, bpp, participants)[:i + 1]


def test_slice_moves_the_pointers_and_copies_the_rest(harness):
    base = dict(secrets=1 << 30, secrets_stride=1001, rand=1 << 31, rand_stride=77, out=1 << 32, out_stride_participant=4099,
                out_stride_clerk=123457, participants=50, len=999, first_participant=(1 << 40) + 9, direct_rows=4)
    cases = []
    for rand in (base["rand"], 0):
        for p0, count in ((0, 50), (1, 1), (7, 43), (49, 1), ((1 << 32) + 3, 2)):
            cases.append((dict(base, rand=rand), p0, count))
    _, got = _run(harness, ["slice " + " ".join(str(v) for v in L.values()) + f" {p0} {count}" for L, p0, count in cases])
    for (L, p0, count), line in zip(cases, got):
        S = dict(zip(L.keys(), map(int, line.split())))
        assert S["secrets"] == L["secrets"] + 8 * p0 * L["secrets_stride"]
        assert S["out"] == L["out"] + 8 * p0 * L["out_stride_participant"]
        assert S["rand"] == (L["rand"] + 8 * p0 * L["rand_stride"] if L["rand"] else 0)
        assert S["first_participant"] == L["first_participant"] + p0 and S["participants"] == count
        for f in ("len", "secrets_stride", "rand_stride", "out_stride_participant", "out_stride_clerk", "direct_rows"):
            assert S[f] == L[f], f


def test_round_counts(harness):
    rounds = [20, 12, 8, 0, 10, 19, 21, -8]
    codes, got = _run(harness, [f"rounds {r}" for r in rounds])
    for r, line in zip(rounds, got):
        ret, calls, value, supported = map(int, line.split())
        if r in (20, 12, 8):
            assert (ret, calls, value, supported) == (codes["ok"], 1, r, 1)
        else:
            assert (ret, calls, value, supported) == (codes["invalid_value"], 0, 0, 0)

"""Host unit test of sda_amd/csrc/signed_rem.hpp - trunc_rem128, the one function every reference-representative kernel reduces
with - compiled with g++ and compared with Python integers (CPU; the kernels are covered by tests/test_signed_limits_gpu.py).
tests/cpp/signed_rem_test.cpp is built twice, -O2 and -O1 with the undefined-behaviour sanitizer, and both run as child
processes on the same lines: every named boundary point of tests/signed_limits.py and its neighbours for the six moduli, and
100,000 seeded random x in [-2^64, 2^64 - 1], the range a sum or difference of two int64 can take."""
import os
import random
import subprocess

import pytest

import signed_limits as SL
from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "signed_rem_test.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"]
LO, HI = -(1 << 64), (1 << 64) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("srem") / "signed_rem_test")
    subprocess.check_call(["g++", "-O2"] + WARN + [SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def exe_ubsan(tmp_path_factory):
    """the same program with the undefined-behaviour sanitizer (host code): a negation, a doubling or a cast that overflows ends
    the run instead of passing by luck"""
    out = str(tmp_path_factory.mktemp("srem_ub") / "signed_rem_test_ubsan")
    subprocess.check_call(["g++", "-O1", "-g"] + WARN + ["-fsanitize=undefined", "-fno-sanitize-recover", SRC, "-o", out])
    return out


@pytest.fixture(params=["O2", "ubsan"])
def harness(request, exe, exe_ubsan):
    return exe if request.param == "O2" else exe_ubsan


def _line(x, q):
    assert LO <= x <= HI
    return f"{x >> 64} {x & ((1 << 64) - 1)} {q}"


def _run(exe, cases):
    out = subprocess.run([exe], input="\n".join(_line(x, q) for x, q in cases) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [int(t) for t in out.stdout.split()]
    assert len(got) == len(cases)
    return got


def _same(cases, got):
    for (x, q), g in zip(cases, got):
        want = po.trunc_rem(x, q)
        assert g == want == SL.trem(x, q), (x, q, g, want, SL.branch(x, q))


def _boundary_cases():
    """every fixed point with its two neighbours, multiples of q up to the ends of the range with theirs, and every sum and
    difference of two special operands"""
    cases = []
    for q in SL.MODULI:
        xs = set()
        for v in SL.point_values(q).values():
            xs |= {v - 1, v, v + 1}
        for k in (3, 4, 5, 7, HI // q, HI // q - 1, (1 << 63) // q, (1 << 63) // q + 1):
            for m in (k * q, -k * q):
                xs |= {m - 1, m, m + 1}
        sp = SL.specials(q)
        for a in sp:
            for b in sp:
                xs |= {a + b, a - b}
        cases += [(x, q) for x in sorted(xs) if LO <= x <= HI]
    return cases


def test_boundary_points_and_special_sums(harness):
    cases = _boundary_cases()
    for q in SL.MODULI:                                                # the set holds what it is named for
        reach = SL.Reach(q)
        for x, m in cases:
            if m == q:
                reach.add(x)
        assert reach.branches == set(SL.BRANCHES) and reach.points == set(SL.POINTS), (q, reach.branches, set(SL.POINTS) - reach.points)
    got = _run(harness, cases)
    _same(cases, got)
    # what separates Rust's `%` from a canonical reduction: -q and every negative exact multiple give 0, not q; the sign follows x
    by = {c: g for c, g in zip(cases, got)}
    for q in SL.MODULI:
        assert by[(-q, q)] == 0 and by[(-2 * q, q)] == 0 and by[(-3 * q, q)] == 0 and by[(-q - 1, q)] == -(1 % q) and by[(q, q)] == 0
        assert by[(-q + 1, q)] == -q + 1 and by[(-2 * q + 1, q)] == -q + 1 and by[(2 * q - 1, q)] == q - 1
        assert by[(LO, q)] == -((1 << 64) % q) and by[(HI, q)] == HI % q


def test_random_sums_of_two_int64(harness):
    rng = random.Random(0x51D)
    cases = []
    for i in range(100_000):
        q = SL.MODULI[i % len(SL.MODULI)]
        cases.append((rng.randint(LO, HI), q))
    _same(cases, _run(harness, cases))
    for q in SL.MODULI:                                                # random x are far-branch values but for the large moduli
        seen = {SL.branch(x, q) for x, m in cases if m == q}
        assert "far" in seen

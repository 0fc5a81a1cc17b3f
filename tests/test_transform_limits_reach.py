"""CPU side of tests/test_transform_limits_gpu.py (no GPU): the case table of tests/transform_limits.py does what it is there for.

  * exactness: the whole-kernel model in the instantiation each case plans - 32-bit lazy, 32-bit reduced, wide - equals the oracle on
    that case's inputs (pyoracle's share_fft for n <= 728, Lagrange evaluation at three share points beyond), and no width or range
    assertion of the model fires;
  * conditions: every lazy case holds an intermediate >= 2^31 (bit 31 set: f_csub's unsigned minimum, __umulhi and the wrapping
    x w - q p see such an operand), every reduced case at a prime just below 2^30 holds one >= 3p both in the radix-2 part and in
    a radix-3 butterfly (a missed conditional subtraction would wrap 32 bits);
  * recorded reach: the per-stage maxima are the ones written down in transform_limits.REACH.  The lazy chain's proven bound
    (4b + 2) p is NOT reached by valid inputs; the table says what is;
  * branch coverage by name, and the plan - 32-bit values, lazy levels, batches per workgroup, twiddles in LDS - against the
    library's own (sda_debug_select_path: fft_narrow, fft_shape and fft_lazy, the function build_fft plans with), for every case
    and for the primes on either side of both thresholds."""
import ctypes
import functools

import pytest

import transform_limits as T
from oracle import pyoracle as po

IDS = [c["name"] for c in T.CASES]


@functools.lru_cache(maxsize=None)
def _model(name):
    return T.run_model(next(c for c in T.CASES if c["name"] == name))


def test_case_names_are_unique_and_every_kind_of_input_is_there():
    assert len(set(IDS)) == len(IDS)
    for c in T.CASES:
        kinds = {T.batch_kind(c, b) for b in T.model_batches(c)}
        assert kinds >= {"all p-1", "halves"} and (kinds >= {"specials", "any i64", "canonical"} or "mixed" in kinds), (c["name"], kinds)
        sec, dr = T.inputs(c)
        assert len(sec) == c["dim"] and len(dr) == c["batches"] * c["t"] and -(-c["dim"] // c["k"]) == c["batches"]
        assert all(-(1 << 62) <= v < (1 << 62) for v in sec + dr)
        assert (sec, dr) == T.inputs(c)                                        # fixed seeds
    by_kind = {kind: sum(c["kind"] == kind for c in T.CASES) for kind in ("sweep", "deep", "edge", "group")}
    assert by_kind == {"sweep": 3 * len(T.SWEEP), "deep": 2, "edge": 4 * len(T.EDGES), "group": 6}


@pytest.mark.parametrize("ab", sorted(T.PRIMES), ids=lambda ab: f"a{ab[0]}b{ab[1]}")
def test_the_recorded_primes_sit_on_either_side_of_both_thresholds(ab):
    a, b = ab
    step = 2 ** a * 3 ** b
    lazy_below, lazy_above, narrow_below, narrow_above = T.PRIMES[ab]
    assert T.PRIMES[ab] == T.threshold_primes(a, b)
    for p in T.PRIMES[ab]:
        assert T.is_prime(p) and p % step == 1
    assert (4 * b + 4) * lazy_below < (1 << 32) <= (4 * b + 4) * lazy_above and narrow_below < (1 << 30) <= narrow_above
    for lo, hi in ((lazy_below, lazy_above), (narrow_below, narrow_above)):   # neighbours: no prime of the progression in between
        assert not any(T.is_prime(q) for q in range(lo + step, hi, step))
    assert {(c["a"], c["b"]) for c in T.CASES} == set(T.PRIMES)


def _lagrange_at(p, N, w2, values, x):
    """the polynomial of degree < N through (w2^i, values[i]), i = 0..N-1 - ALL N-th roots of unity - at x:
    (x^N - 1) / N * sum_i values[i] w2^i / (x - w2^i); no transform involved"""
    acc, node = 0, 1
    for v in values:
        acc = (acc + v * node * pow(x - node, -1, p)) % p
        node = node * w2 % p
    return (pow(x, N, p) - 1) * pow(N, -1, p) * acc % p


def test_the_three_point_evaluation_is_the_oracles_lagrange_form():
    c = next(c for c in T.CASES if c["name"].startswith("edge-a3b3") and c["which"] == T.LAZY_BELOW)
    w2, w3 = T.case_roots(c)
    pss = po.PackedSecretSharing(c["t"], c["n"], c["k"], c["p"], w2, w3)
    sec, dr = T.inputs(c)
    for b in (0, 3, 4):
        s, r = T.batch_values(c, sec, dr, b)
        want = pss.share_lagrange(s, r)
        x = [0] + [v % c["p"] for v in s + r]
        assert [_lagrange_at(c["p"], len(x), w2, x, pow(w3, j, c["p"])) for j in range(1, c["n"] + 1)] == want


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_the_model_equals_the_oracle_and_no_assert_fires(case):
    p, k, t, n = case["p"], case["k"], case["t"], case["n"]
    shares, _ = _model(case["name"])                      # every width / range assertion of the model ran
    w2, w3 = T.case_roots(case)
    assert pow(w2, k + t + 1, p) == 1 and pow(w2, (k + t + 1) // 2, p) != 1 and pow(w3, n + 1, p) == 1 and pow(w3, (n + 1) // 3, p) != 1
    pss = po.PackedSecretSharing(t, n, k, p, w2, w3)
    assert pss.is_fft_shape()
    sec, dr = T.inputs(case)
    assert sorted(shares) == T.model_batches(case)
    for b, got in shares.items():
        s, r = T.batch_values(case, sec, dr, b)
        if n <= 728:
            assert got == [v % p for v in pss.share_fft(s, r, "canonical")], b
        else:
            x = [0] + [v % p for v in s + r]
            for j in (1, n // 2, n):
                assert got[j - 1] == _lagrange_at(p, len(x), w2, x, pow(w3, j, p)), (b, j)


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_conditions_and_recorded_reach(case):
    _, mx = _model(case["name"])
    p = case["p"]
    if case["lazy"]:
        assert max(mx.values()) >= 1 << 31, mx                              # bit 31 set somewhere in the lazy chain
        assert max(mx.values()) <= (4 * case["b"] + 2) * p                  # ... and the proven bound holds
    if case["narrow"] and case["which"] == T.NARROW_BELOW:
        assert mx["radix2"] >= 3 * p and max(mx["folded"], mx["later"]) >= 3 * p, mx
    if case["narrow"]:
        assert T.fractions(mx) == T.REACH[case["name"]], (T.fractions(mx), T.REACH[case["name"]])
    else:
        assert case["name"] not in T.REACH and max(mx.values()) < 4 * p


def test_the_reach_table_has_exactly_the_32_bit_cases():
    assert set(T.REACH) == {c["name"] for c in T.CASES if c["narrow"]}
    for c in T.CASES:
        if c["lazy"]:                                                       # what valid inputs reach, against the proven bound
            assert 0.5 <= max(T.REACH[c["name"]]) < (4 * c["b"] + 2) * c["p"] / (1 << 32) < 0.96, c["name"]


WANTED = ["a odd", "a even", "radix-4 pass with qd > 1", "last radix-4 pass (qd == 1)", "zero extension: m2 <= m3/9",
          "zero extension: m3/9 < m2 <= m3/3", "zero extension: m3/3 < m2", "in[0] shortcut", "first-level butterfly", "b-2 odd", "b-2 even",
          "non-last radix-9 pass", "LDS output path", "radix-9 output path", "G=16", "G=8", "G=4", "G=2", "G=1", "tw_lds=0", "tw_lds=1",
          "more than one padding unit", "ragged group", "ragged batch", "lazy", "reduced", "wide"]


@pytest.mark.parametrize("branch", WANTED)
def test_branch_coverage_by_name(branch):
    hit = [c for c in T.CASES if branch in T.coverage(c)]
    assert hit, branch
    if branch in ("lazy", "reduced", "wide", "G=8", "G=4", "G=2", "G=1", "more than one padding unit"):
        return
    # every structural branch runs in BOTH 32-bit forms
    assert any(c["lazy"] for c in hit) and any(c["narrow"] and not c["lazy"] for c in hit), branch


def test_the_group_cases_cross_a_padding_unit_and_end_ragged():
    for c in T.CASES:
        if c["kind"] != "group":
            continue
        G = c["G"]
        want = dict(c["knobs"]).get("SDA_FFT_G")
        assert want is None or G == want, c["name"]
        cov = T.coverage(c)
        assert ("more than one padding unit" in cov) == (G < 8), c["name"]
        assert "ragged group" in cov or G == 1 or c["n"] == 6560, c["name"]
        assert c["xcd"] == (G < 8)
    deep = next(c for c in T.CASES if c["kind"] == "group" and c["n"] == 6560)
    assert (deep["G"], deep["tw_lds"], deep["batches"]) == (2, 0, 130)


def test_selection_edges_name_the_expected_instantiation():
    for a, b in T.EDGES:
        got = [c["kernel"] for c in T.CASES if c["kind"] == "edge" and (c["a"], c["b"]) == (a, b)]
        assert got == ["unsigned int, true>", "unsigned int, false>", "unsigned int, false>", "unsigned long, false>"], (a, b)
    for c in T.CASES:
        if c["kind"] == "sweep":
            assert c["kernel"] == ("unsigned int, true>" if c["which"] == T.LAZY_BELOW and ("SDA_NO_LAZY", 1) not in c["knobs"] else "unsigned int, false>")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from sda_amd import capi
    return capi.hooks_library()


def _library_plan(lib, case, p=None, extra=()):
    from test_path_select import select
    w2, w3 = T.case_roots(case) if p is None else (T.root(p, case["k"] + case["t"] + 1), T.root(p, case["n"] + 1))
    knobs = tuple(case["knobs"]) + tuple(extra)
    text = ",".join(f"{nm}={v}" if nm == "SDA_FFT_G" else nm for nm, v in knobs)
    got = select(lib, case["k"], case["t"], case["n"], p or case["p"], w2, w3, knobs=text)
    assert got["wide"] == "fft" and got["narrow"] == "none" and got["injected"] == "fft" and got["call20"] == "fft" and got["transform_shape"] == "1", got
    return (got["transform_narrow"] == "1", got["transform_lazy"] == "1", int(got["transform_g"]), int(got["transform_tw_lds"])), knobs


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_plan_against_the_library(lib, case):
    """the library's own plan - the functions sda_share_generator_new() builds the kernel's plan with - equals the restated one: for
    the case as it runs, with the 64-bit kernel forced, and at all four primes of its (a, b).  Just above the lazy threshold a wrong
    admission cannot show as a wrong share (values reach ~0.6 of 2^32 there): this field and the kernel's name are the observers."""
    got, knobs = _library_plan(lib, case)
    assert got == T.plan(case["p"], case["k"], case["t"], case["n"], knobs) == (case["narrow"], case["lazy"], case["G"], case["tw_lds"])
    got, knobs = _library_plan(lib, case, extra=(("SDA_NO_NARROW", 1),))
    assert got == T.plan(case["p"], case["k"], case["t"], case["n"], knobs) and got[:2] == (False, False)
    if case["kind"] == "edge" or ("SDA_NO_LAZY", 1) in case["knobs"]:
        return
    want = [(True, True), (True, False), (True, False), (False, False)]
    for which, p in enumerate(T.PRIMES[(case["a"], case["b"])]):
        got, knobs = _library_plan(lib, case, p=p)
        assert got == T.plan(p, case["k"], case["t"], case["n"], knobs) and got[:2] == want[which], (which, p, got)


def test_a_transform_plan_is_reported_for_the_transform_family_only(lib):
    from test_path_select import select, P62, OMEGA
    got = select(lib, 3, 1, 8, P62, OMEGA[8], OMEGA[9])
    assert got["wide"] == "l31" and (got["transform_narrow"], got["transform_lazy"], got["transform_g"], got["transform_tw_lds"]) == ("0",) * 4
    got = select(lib, 100, 155, 728, P62, OMEGA[256], OMEGA[729])
    assert got["wide"] == "fft" and (got["transform_narrow"], got["transform_lazy"], got["transform_g"], got["transform_tw_lds"]) == ("0", "0", "8", "1")


def test_the_release_library_does_not_carry_the_selection_table(lib):
    from sda_amd import capi
    rel = ctypes.CDLL(capi.RELEASE_LIB_PATH)
    assert not hasattr(rel, "sda_debug_select_path") and hasattr(ctypes.CDLL(capi.TEST_LIB_PATH), "sda_debug_select_path")
    assert b"transform_lazy=" not in open(capi.RELEASE_LIB_PATH, "rb").read()
    assert b"transform_lazy=" in open(capi.TEST_LIB_PATH, "rb").read()

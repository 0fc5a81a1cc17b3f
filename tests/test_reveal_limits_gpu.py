"""The one-shot reveal (sda_secret_reconstructor_reconstruct_dev) over its shape space and at its sum limits, bit-exact against the
reference of tests/reveal_limits.py (pytest -m gpu): there is no tolerance anywhere, this is integer arithmetic.

The cases are tests/reveal_limits.py's: every instance of packed_reconstruct_n31_kernel<NMAX, GROUP> and
packed_reconstruct_vec_kernel<NMAX> over the instance edges 4|5, 8|9 and 16|17 rows and k up to 16 (65,536 bytes of dynamic LDS) at
eight primes, among them 2^31 - 1, the first prime above 2^31 and the primes on either side of 2^29; batch counts of 1, 2, 3 and
511 / 512 / 513 with every store tail; the grouped kernel with several secrets per group, a short last group and a single group;
misaligned bases and an odd stride (grouped kernel), padded rows (register/LDS kernels); one handle across changing index sets.
The rows are crafted: sign-aligned with the n31 constants of a target output row and sign-opposed, (p - 1) / 2, (p + 1) / 2,
p - 1, the any-int64 specials, random any-int64 and random canonical values.  tests/test_reveal_limits_reach.py shows on the CPU
what these rows reach (REACH) and that route() names every instance and branch.

Per case: the rows go into device memory with the case's stride and base offset, every word around them poisoned; `out` carries
canary words after `dim` (and before it for the + 8 byte base); the result equals the reference, the canaries are untouched, the
return value is `dim` and sda_debug_last_reveal_kernel() names the kernel route() predicts.  Every narrow-prime case of the
instance grid runs a second time on a fresh handle under SDA_NO_NARROW (prepare_R caches `narrow` with the matrix): the 64-bit
kernel's output equals the narrow one's."""
import numpy as np
import pytest

import reveal_limits as L
from conftest import set_knob, use_test_hooks

pytestmark = pytest.mark.gpu

TAIL = 8                                                               # canary words after `dim`


def _handle(case, no_narrow=False):
    from sda_amd import crypto
    w2, w3 = L.roots(case["p"], case["k"], case["t"], case["n"])
    set_knob("SDA_NO_NARROW", 1 if no_narrow else 0)                   # read when the handle is created
    rec = crypto.SecretReconstructor(crypto.PackedShamir(case["k"], case["n"], case["t"], case["p"], w2, w3), case["dim"])
    set_knob("SDA_NO_NARROW", 0)
    return rec


def _reveal(case, rec, no_narrow=False):
    """one reconstruct_dev call of the case on `rec`: checks the canaries, the return value and the kernel's name; -> [dim]"""
    from sda_amd import capi
    from sda_amd.device import DeviceBuffer
    rows = L.make_rows(case["name"])
    R, B = rows.shape
    stride, so, oo, dim = case["stride"], case["shares_off"], case["out_off"], case["dim"]
    assert stride >= B and R == len(case["indices"])
    host = np.full(so + R * stride + 2, L.POISON, dtype=np.int64)
    host[so:so + R * stride].reshape(R, stride)[:, :B] = rows
    d_sh = DeviceBuffer.from_numpy(host)
    d_out = DeviceBuffer.from_numpy(np.full(oo + dim + TAIL, L.CANARY, dtype=np.int64))
    assert d_sh.ptr % 16 == 0 and d_out.ptr % 16 == 0
    n_out = rec.reconstruct_dev(list(case["indices"]), d_sh.at(so), B, stride, d_out.at(oo), dim)
    name = capi.load().sda_debug_last_reveal_kernel().decode()
    out = d_out.to_numpy()
    assert n_out == dim
    want_name, lds = L.route(case["p"], case["k"], R, so == 0, oo == 0, stride, B, no_narrow)
    assert name == want_name, (name, want_name)
    if not no_narrow:
        assert (name, lds) == (case["kernel"], case["lds"])
    assert np.all(out[:oo] == L.CANARY) and np.all(out[oo + dim:] == L.CANARY), "the reveal wrote outside out[0 .. dim)"
    d_sh.free()
    d_out.free()
    return out[oo:oo + dim]


def _assert_equal(got, want, case, what="reveal"):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} secrets differ, first (batch, e) {[(int(o) // case['k'], int(o) % case['k']) for o in bad[:4]]}: "
                           f"got {got[bad[:4]].tolist()}, want {want[bad[:4]].tolist()}")


@pytest.mark.parametrize("case", L.CASES, ids=[c["name"] for c in L.CASES])
def test_reveal_at_its_limits(gpu, case):
    use_test_hooks()
    want = L.reference(case["name"])
    got = _reveal(case, _handle(case))
    _assert_equal(got, want, case)
    if case["twin"]:
        wide = _reveal(case, _handle(case, no_narrow=True), no_narrow=True)
        _assert_equal(wide, got, case, "SDA_NO_NARROW")


@pytest.mark.parametrize("p", sorted(L.REUSE), ids=[f"p{p}" for p in sorted(L.REUSE)])
def test_one_handle_with_changing_index_sets(gpu, p):
    """prepare_R's cache: index set A, another set of the same length, A again, A with one more row, A permuted with its rows
    permuted alike - each call against its own reference.  The reveal's name lives in a buffer of its own: sda_debug_last_kernel()
    reports the same share-generation call before and after the reveals"""
    from sda_amd import capi, crypto
    use_test_hooks()
    steps = L.REUSE[p]
    first = steps[0]
    gen = crypto.ShareGenerator(crypto.PackedShamir(first["k"], first["n"], first["t"], p, *L.roots(p, first["k"], first["t"], first["n"])))
    gen.generate(np.arange(30, dtype=np.int64), np.arange(40, dtype=np.int64))
    before = capi.load().sda_debug_last_kernel().decode()
    assert before and "reconstruct" not in before
    rec = _handle(first)
    got = {}
    for case in steps:
        got[case["name"]] = _reveal(case, rec)
        _assert_equal(got[case["name"]], L.reference(case["name"]), case, case["name"])
    assert np.array_equal(got[steps[4]["name"]], got[steps[0]["name"]]) and steps[4]["rows_of"][0] == steps[0]["name"]
    assert capi.load().sda_debug_last_kernel().decode() == before

"""The 32-bit forms of the transform kernel (packed_gen_fft_kernel<.., unsigned int, false | true>, sda_amd/csrc/fft_kernels.hip) at
their range limits and over the kernel's shape space, bit-exact against the C oracle (pytest -m gpu).

The cases and their inputs are tests/transform_limits.py's: every structure (a, b) of the wide kernel's sweep at the largest prime
that admits the lazy radix-3 levels ((4b + 4) p < 2^32; lazy and, under SDA_NO_LAZY, reduced) and at the largest prime below 2^30
(reduced, intermediates next to 4p = 2^32); the deep lazy chains of 8 and 9 levels; the four primes around both thresholds, where
the kernel's name is the observer of the selection; every batches-per-workgroup form, with jobs that cross a padding unit of the
XCD group permutation.  tests/test_transform_limits_reach.py shows on the CPU that these inputs put bit 31 into the lazy chain
and values >= 3p into the reduced one, and pins the plan.

Per case: injected generation against coracle.packed_generate; the kernel instance by name and path_name(); the device CSPRNG
for two participants with a padded row stride (padding stays zero); the round trip through SecretReconstructor from t + k random
clerks; lazy / reduced / wide agreement (sweep and deep cases); the plain group order (SDA_NO_XCD_MAP) where the permutation runs."""
import functools

import numpy as np
import pytest

import transform_limits as T
from conftest import set_knob

pytestmark = pytest.mark.gpu

KEY = bytes((i * 11 + 3) & 0xFF for i in range(32))
FIRST = (1 << 36) + 70


def _operands(case):
    """the case's injected secrets and draws, and the secrets of the two CSPRNG participants (the same operands, rotated by k)"""
    sec, dr = T.inputs(case)
    secrets, rand = np.array(sec, dtype=np.int64), np.array(dr, dtype=np.int64)
    return secrets, rand, np.stack([np.roll(secrets, case["k"] * q) for q in range(2)])


@functools.lru_cache(maxsize=2)
def _reference(p, k, t, n, B):
    """coracle.packed_generate for the injected call and for both CSPRNG participants, in ONE call of 3 B batches: the oracle spends
    its time on the share matrix (n (k + t)^2; seconds for the 1023-term shapes), which the cases at one prime - lazy and
    SDA_NO_LAZY run the same operands - then share.  The injected vector goes last, so that its ragged batch stays the oracle's own."""
    from oracle import coracle
    case = next(c for c in T.CASES if (c["p"], c["k"], c["t"], c["n"], c["batches"]) == (p, k, t, n, B))
    w2, w3 = T.case_roots(case)
    secrets, rand, sec2 = _operands(case)
    full = np.zeros((2, B * k), dtype=np.int64)
    full[:, :case["dim"]] = sec2                                         # zero padding of a ragged batch (batched.rs:37-43)
    draws = [coracle.drbg_fill(KEY, FIRST + q, B, t, p).reshape(-1) for q in range(2)]
    want = coracle.packed_generate(p, k, t, n, w2, w3, np.concatenate([full[0], full[1], secrets]), np.concatenate(draws + [rand]))
    assert want.shape == (n, 3 * B)
    return want[:, 2 * B:], [want[:, :B], want[:, B:2 * B]]


def _run(case, secrets, rand, sec2, extra=()):
    """a generator under the case's knobs (+ extra): injected shares, device-CSPRNG shares [2][n][Bs], the kernel names, handles"""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    p, k, t, n = case["p"], case["k"], case["t"], case["n"]
    knobs = dict(SDA_NO_NGEMM=1, SDA_FORCE_FFT=0, SDA_NO_LAZY=0, SDA_NO_NARROW=0, SDA_FFT_G=0, SDA_NO_XCD_MAP=0)
    knobs.update(case["knobs"])
    knobs.update(extra)
    for nm, v in knobs.items():                                         # read when the handle is created
        set_knob(nm, v)
    w2, w3 = T.case_roots(case)
    sch = crypto.PackedShamir(k, n, t, p, w2, w3)
    gen = crypto.ShareGenerator(sch)
    assert gen.path_name() == "fft" and gen.csprng_share_map() == gen.SHARE_MAP_TSS_NODES
    B = gen.batch_count(case["dim"])
    assert B == case["batches"]
    got = gen.generate(secrets, rand)
    names = [capi.load().sda_debug_last_kernel().decode()]
    gen.set_drbg_key(KEY)
    P, Bs = sec2.shape[0], B + 5                                         # padded row stride
    d_sec = DeviceBuffer.from_numpy(sec2)
    d_out = DeviceBuffer(P * n * Bs).zero()
    gen.generate_batch_dev(d_sec.ptr, P, case["dim"], case["dim"], d_out.ptr, n * Bs, Bs, first_participant=FIRST)
    names.append(capi.load().sda_debug_last_kernel().decode())
    return got, d_out.to_numpy().reshape(P, n, Bs), names, sch


def _assert_kernel(names, case, narrow, lazy, tw_lds):
    want = f", {'true' if tw_lds else 'false'}, {T.kernel_suffix(narrow, lazy)}"
    for name in names:
        assert name.startswith("packed_gen_fft_kernel<") and name.endswith(want), (name, want)


@pytest.mark.parametrize("case", T.CASES, ids=[c["name"] for c in T.CASES])
def test_transform_kernel_at_its_range_limits(gpu, case):
    from sda_amd import crypto
    p, k, t, n, B, dim = case["p"], case["k"], case["t"], case["n"], case["batches"], case["dim"]
    secrets, rand, sec2 = _operands(case)
    want, want_csprng = _reference(p, k, t, n, B)

    # 1. injected randomness, 2. the instance that ran
    got, out, names, sch = _run(case, secrets, rand, sec2)
    _assert_kernel(names, case, case["narrow"], case["lazy"], case["tw_lds"])
    assert names[0].endswith(case["kernel"])
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} shares differ, first (row, batch) {bad[:4].tolist()}"

    # 3. the device CSPRNG (tss's share map: the draws are the values at the secret nodes), padded rows
    for q in range(2):
        bad = np.argwhere(out[q, :, :B] != want_csprng[q])
        assert bad.size == 0, f"participant {q}: {len(bad)} shares differ, first (row, batch) {bad[:4].tolist()}"
    assert not out[:, :, B:].any()

    # 4. round trip from t + k random clerks
    rng = np.random.default_rng(k * 1000 + t + n)
    idx = sorted(rng.choice(n, size=t + k, replace=False).tolist())
    rec = crypto.SecretReconstructor(sch, dim).reconstruct([(i, out[0, i, :B]) for i in idx])
    assert np.array_equal(rec, np.mod(sec2[0], p))

    # 5. lazy / reduced / wide agreement; the plain group order
    others = []
    if case["agree"]:
        others += [(("SDA_NO_LAZY", 1),), (("SDA_NO_NARROW", 1),)]
    if case["xcd"]:
        others += [(("SDA_NO_XCD_MAP", 1),)]
    for extra in others:
        got2, out2, names2, _ = _run(case, secrets, rand, sec2, extra)
        narrow, lazy, G, tw_lds = T.plan(p, k, t, n, tuple(case["knobs"]) + extra)
        _assert_kernel(names2, case, narrow, lazy, tw_lds)
        assert np.array_equal(got2, got) and np.array_equal(out2, out), extra

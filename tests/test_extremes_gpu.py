"""Every share-generation family at its operand and modulus limits, bit-exact against the C oracle (pytest -m gpu).

The parity tests elsewhere draw uniform operands, whose dot products and digit columns stay far below the bounds the kernels'
comments rely on.  Here the secrets and injected draws are crafted against the constants each kernel holds (tests/extremes.py:
sign-aligned with a target row, extreme balanced digits / limbs, the target row cycling across batches) at the largest primes
each family admits: 2^62 - 57 for the wide families, 2^31 - 1 and the primes on either side of 2^29 for the one-limb kernels,
8355691 for the narrow limb GEMM.  Per case: injected generation against coracle.packed_generate; the device CSPRNG through
generate_batch_dev in both share maps (odd row stride once per family) against coracle.packed_generate_csprng; for the families
with a dual-role form two tiles through generate_combine_dev with every clerk row of the sums against coracle.combine; the round
trip through reconstruct; and sda_debug_last_kernel() names the family that ran (every generation call; the reveal kernels have
a name hook of their own, see RECON below).  tests/test_extremes_reach.py checks on the CPU
that the crafted batches do reach the bounds; tests/test_path_select.py pins the selection at these primes."""
import numpy as np
import pytest

import extremes as X
import reveal_limits
from conftest import set_knob, use_test_hooks

pytestmark = pytest.mark.gpu

KEY = bytes(range(7, 39))
MFMA_COMPILED = {(8, 7), (8, 2), (3, 4), (3, 1), (12, 3), (10, 5), (4, 11)}
DUAL = {"l31", "mfma", "n31", "ngemm"}

CASES = X.GPU_CASES


def _ids(c):
    return f"{c[0]}-k{c[1]}t{c[2]}n{c[3]}-p{c[4]}" + ("-" + "+".join(c[5]) if c[5] else "")


def expected_kernel(family, k, t, p, fused=False):
    """the kernel instance (or its prefix) sda_debug_last_kernel() names for this family and shape"""
    kt = k + t
    if family == "mfma":
        kk, tt = (k, t) if (k, t) in MFMA_COMPILED else (0, 0)
        return f"{'fused_packed' if fused else 'packed_gen'}_mfma_kernel<{kk}, {tt}, 20>"
    if family == "n31":
        ktmax = 4 if kt <= 4 else 8 if kt <= 8 else 12 if kt <= 12 else 16
        group = 4 if kt <= 4 else X.n31_group(p)
        return f"{'fused_packed' if fused else 'packed_gen'}_n31_kernel<{ktmax}, {group}, 20>"
    if family == "ngemm":
        ks = (kt + 63) // 64
        ks = 1 if ks <= 1 else 2 if ks <= 2 else 4 if ks <= 4 else 8
        return f"packed_gen_ngemm_kernel<{ks}, "
    if family == "l31":
        return "fused_packed_l31" if fused else "packed_gen_l31_"
    return {"l31_global": "packed_gen_l31_rtg_kernel<", "generic": "packed_gen_generic_kernel", "mont64": "packed_gen_kernel<"}[family]


def _assert_family(family, k, t, p, fused=False):
    from sda_amd import capi
    name = capi.load().sda_debug_last_kernel().decode()
    want = expected_kernel(family, k, t, p, fused)
    assert want in name, (name, want)
    if family == "l31" and not fused:
        assert "rtg" not in name, name


@pytest.mark.parametrize("case", CASES, ids=[_ids(c) for c in CASES])
def test_share_generation_at_the_limits(gpu, case):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    from oracle import coracle
    family, k, t, n, p, knobs, B, odd = case
    for kn in knobs:
        set_knob(kn, 1)
    w2, w3 = X.omegas(p, k, t, n)
    sch = crypto.PackedShamir(k, n, t, p, w2, w3)
    gen = crypto.ShareGenerator(sch)
    dim = B * k - (1 if k > 1 else 0)                     # a ragged last batch (zero padding) wherever k > 1
    assert gen.batch_count(dim) == B

    # 1. injected crafted secrets and draws (tss's share map)
    sec, dr = X.crafted_operands(family, p, k, t, n, w2, w3, B, systematic=False)
    got = gen.generate(sec[:dim], dr if t else None)
    _assert_family(family, k, t, p)
    want = coracle.packed_generate(p, k, t, n, w2, w3, sec[:dim], dr)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} shares differ, first (row, batch) {bad[:4].tolist()}"

    # 2. the device CSPRNG, secrets crafted against the constants of the map the call uses, both maps where t > 0
    gen.set_drbg_key(KEY)
    P = 2
    maps = [1, 0] if t > 0 and gen.csprng_share_map() == 1 else [gen.csprng_share_map()]
    for share_map in maps:
        gen.set_csprng_share_map(share_map)
        s1, _ = X.crafted_operands(family, p, k, t, n, w2, w3, B, systematic=share_map == 1 and t > 0)
        sec2 = np.stack([s1[:dim], np.roll(s1, k)[:dim]])          # participant 1: the same batches, shifted by one
        Bs = B | 1 if odd else B + (B & 1)
        d_sec = DeviceBuffer.from_numpy(sec2)
        d_out = DeviceBuffer(P * n * Bs).zero()
        first = (1 << 33) + 11 * share_map
        gen.generate_batch_dev(d_sec.ptr, P, dim, dim, d_out.ptr, n * Bs, Bs, first_participant=first)
        _assert_family(family, k, t, p)
        out = d_out.to_numpy().reshape(P, n, Bs)
        for q in range(P):
            w = coracle.packed_generate_csprng(p, k, t, n, w2, w3, sec2[q], coracle.drbg_fill(KEY, first + q, B, t, p), share_map)
            assert np.array_equal(out[q, :, :B], w), f"participant {q}, share map {share_map}"
        # 4. reconstruct from a t + k subset
        rng = np.random.default_rng(k * 1000 + t + n)
        idx = sorted(rng.choice(n, size=t + k, replace=False).tolist())
        rec = crypto.SecretReconstructor(sch, dim).reconstruct([(i, out[0, i, :B]) for i in idx])
        assert np.array_equal(rec, sec2[0] % p), f"reconstruct, share map {share_map}"
    gen.set_csprng_share_map(maps[0])

    # 3. the dual-role launch: two tiles, every clerk row of the sums against the oracle
    if family not in DUAL:
        return
    tiles, P = 2, 3
    Bs = (B + 15) // 16 * 16
    s1, _ = X.crafted_operands(family, p, k, t, n, w2, w3, B, systematic=gen.csprng_share_map() == 1 and t > 0)
    sec3 = np.stack([np.roll(s1, k * q)[:dim] for q in range(P)])
    S = dim + (dim & 1)                                   # the dual-role launch wants 16-byte aligned secret rows (even stride)
    padded = np.zeros((P, S), dtype=np.int64)
    padded[:, :dim] = sec3
    d_sec = DeviceBuffer.from_numpy(padded)
    comb = crypto.ShareCombiner(sch)
    comb.begin_dev(n, B)
    bufs = [DeviceBuffer(n * P * Bs).zero() for _ in range(2)]
    for i in range(tiles + 1):
        gen.generate_combine_dev(comb, d_sec.ptr, P if i < tiles else 0, dim, S, bufs[i % 2].ptr, Bs, P * Bs,
                                 d_prev=bufs[(i - 1) % 2].ptr if i else 0, prev_participants=P if i else 0, first_participant=i * P)
        if i == 1:
            _assert_family(family, k, t, p, fused=True)
    d_sums = DeviceBuffer(n * B)
    comb.finish_dev(d_sums.ptr)
    sums = d_sums.to_numpy().reshape(n, B)
    want = [coracle.packed_generate_csprng(p, k, t, n, w2, w3, sec3[q], coracle.drbg_fill(KEY, i * P + q, B, t, p),
                                           gen.csprng_share_map()) for i in range(tiles) for q in range(P)]
    tile1 = bufs[1].to_numpy().reshape(n, P, Bs)
    for q in range(P):
        assert np.array_equal(tile1[:, q, :B], want[P + q]), f"dual-role shares of participant {q}"
    for c in range(n):
        assert np.array_equal(sums[c], coracle.combine(p, np.stack([w[c] for w in want]))), f"clerk sum {c}"


# (k, t, n, p, row stride kind): 3 / 7 / 15 rows take packed_reconstruct_vec_kernel<4 | 8 | 16> above 2^31 and the n31 reveal
# below (4 terms per reduction at 2^31 - 1, 16 at 8355691); 33 rows or an odd row stride take the grouped kernel
# (launch_packed_reconstruct's general form).  The routing is asserted: sda_debug_last_reveal_kernel() (test library) against
# reveal_limits.route().  Shares of p - 1 are the UNSIGNED worst case, that of the two 64-bit kernels, which sum canonical
# products; the narrow kernel centres its values first and p - 1 centres to -1, so its sums stay 2^-28 below their bound here -
# its worst case, rows sign-aligned with its constants, lives in tests/test_reveal_limits_gpu.py.
RECON = [(k, t, n, p, odd) for p in (X.PMAX, X.P31MAX, X.NGEMM_PMAX)
         for k, t, n, odd in ((1, 2, 4, False), (3, 4, 8, False), (8, 7, 26, False), (20, 13, 50, False), (8, 7, 26, True))]


@pytest.mark.parametrize("k,t,n,p,odd", RECON, ids=[f"k{c[0]}t{c[1]}n{c[2]}-p{c[3]}" + ("-odd" if c[4] else "") for c in RECON])
def test_reconstruct_maximal_shares(gpu, k, t, n, p, odd):
    """every share p - 1, mixed with 0 and 1, against the oracle: the sums of the two 64-bit reconstruct kernels at their largest
    (canonical products).  NOT the narrow kernel's: it centres p - 1 to -1 (tests/test_reveal_limits_reach.py shows how far below
    its bound that stays; tests/test_reveal_limits_gpu.py holds its sign-aligned worst case).  The kernel that ran is asserted."""
    from sda_amd import capi
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    from oracle import coracle
    use_test_hooks()                                      # the reveal's name hook exists in the test library only
    w2, w3 = X.omegas(p, k, t, n)
    B = 1500
    dim = B * k - (1 if k > 1 else 0)
    rng = np.random.default_rng(p % 1000 + k)
    rows = t + k
    sh = np.full((rows, B), p - 1, dtype=np.int64)
    sh[:, : B // 2] = rng.choice(np.array([p - 1, p - 1, p - 1, 0, 1], dtype=np.int64), size=(rows, B // 2))
    sh[:, -1] = 0
    idx = sorted(rng.choice(n, size=rows, replace=False).tolist())
    stride = B | 1 if odd else B + (B & 1)
    host = np.zeros((rows, stride), dtype=np.int64)
    host[:, :B] = sh
    d_sh = DeviceBuffer.from_numpy(host)
    d_out = DeviceBuffer(dim + 1)
    rec = crypto.SecretReconstructor(crypto.PackedShamir(k, n, t, p, w2, w3), dim)
    assert rec.reconstruct_dev(idx, d_sh.ptr, B, stride, d_out.ptr, dim + 1) == dim
    assert capi.load().sda_debug_last_reveal_kernel().decode() == reveal_limits.route(p, k, rows, d_sh.ptr % 16 == 0, d_out.ptr % 16 == 0, stride, B)[0]
    got = d_out.to_numpy()[:dim]
    want = coracle.packed_reconstruct(p, k, t, w2, w3, dim, idx, sh)
    assert np.array_equal(got, want)

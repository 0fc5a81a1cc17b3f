"""The retry stream of the device CSPRNG (sda-drbg-v1) in every kernel that draws randomness, bit-exact against the C oracle
(pytest -m gpu).

Over the primes of the other suites a candidate word is rejected with probability 2^-18 .. 2^-56, so the retry counter each
kernel family writes out on its own (b T + i, under the paired rule b ceil(T / 2) + j; the attempt number in the top byte of
state word 15, above the top 24 bits of the stream id) practically never runs there.  Here (tests/drbg_retry.py):
  * primes just above 2^64 / 5 reject one candidate in five: the matrix families (family selection and knobs of
    extremes.GPU_CASES), their dual-role forms and the side-stream transform form, every retry branch of the transform kernel
    (8 batches per workgroup and 4 / 2 / 1; ChaCha20 / 12 / 8), additive sharing in both value modes, the full mask, and the
    draws the any-shape kernel has materialised (drbg_fill_kernel);
  * under the paired rule (moduli <= 0x7F7F7F) rejections are located on the CPU and small jobs run at those stream ids: the
    transform kernel's paired branch (narrow values, lazy and reduced) and the one-limb kernels;
  * one located stream per kernel holds a draw that needs a second retry attempt (additive, transform).
Every job has three participants or more whose stream ids have bits above bit 32 (once the last admissible ids), an odd batch count (a
ragged last group; with k > 1 a ragged last batch) and once per family an odd output row stride; both CSPRNG share maps where
the family offers both; sda_debug_last_kernel() names the kernel that ran (the mask calls record no name: a Full scheme has one kernel).  tests/test_drbg_retry_reach.py proves on the CPU
that each job does enter the retry stream where a wrong counter would show."""
import numpy as np
import pytest

import drbg_retry as R
from conftest import set_knob

pytestmark = pytest.mark.gpu



def _ids(cases):
    return [c["name"] for c in cases]


def _knobs(case):
    for kn in case["knobs"]:
        set_knob(*(kn if isinstance(kn, tuple) else (kn, 1)))


def _last_kernel():
    from sda_amd import capi
    return capi.load().sda_debug_last_kernel().decode()


def _generator(case):
    from sda_amd import crypto
    k, t, n, p = case["k"], case["t"], case["n"], case["p"]
    if case.get("additive"):
        sch, w2, w3 = crypto.Additive(n, p), None, None
    else:
        w2, w3 = R.omegas(case)
        sch = crypto.PackedShamir(k, n, t, p, w2, w3)
    gen = crypto.ShareGenerator(sch)
    if case.get("signed"):
        gen.set_value_mode("rust_signed")
    gen.set_drbg_key(R.KEY)
    if case.get("rounds", 20) != 20:
        gen.set_drbg_rounds(case["rounds"])                # deterministic mode only
    return sch, gen, w2, w3


def _want(case, w2, w3, secrets, streams, B, share_map):
    """the oracle's shares [n][B] of each participant (rows of `secrets`) from the oracle's draws of its stream.  Packed Shamir:
    ONE oracle call for all of them - batches are independent, so the participants' zero-padded batches are laid end to end (the
    oracle builds its Lagrange matrix once per call, seconds for the largest transform shape)"""
    from oracle import coracle, pyoracle as po
    k, t, n, p = case["k"], case["t"], case["n"], case["p"]
    draws = [coracle.drbg_fill(R.KEY, s, B, t, p, case.get("rounds", 20)) for s in streams]
    if case.get("signed"):
        sch = po.AdditiveSecretSharing(n, p, "rust_signed")
        return [np.array(po.generate(sch, [int(v) for v in sec], [int(v) for v in dr]), dtype=np.int64) for sec, dr in zip(secrets, draws)]
    if case.get("additive"):
        return [coracle.additive_generate(p, n, sec, dr) for sec, dr in zip(secrets, draws)]
    padded = np.zeros((len(streams), B * k), dtype=np.int64)
    padded[:, :secrets.shape[1]] = secrets
    out = coracle.packed_generate_csprng(p, k, t, n, w2, w3, padded.reshape(-1), np.concatenate(draws), share_map)
    return [out[:, q * B:(q + 1) * B] for q in range(len(streams))]


def _generate_and_compare(case, first, B, odd):
    """generate_batch_dev for participants first .. first + P - 1, participant-major rows of stride Bs (odd on request), against the
    oracle; nothing is written past a row"""
    from sda_amd.device import DeviceBuffer
    _knobs(case)
    k, n, P = case["k"], case["n"], case.get("participants", R.PARTICIPANTS)      # located jobs: three
    sch, gen, w2, w3 = _generator(case)
    dim = B * k - (1 if k > 1 else 0)                      # a ragged last batch wherever k > 1
    assert gen.batch_count(dim) == B and B % 2 == 1
    rng = np.random.default_rng(B * 131 + k)
    if case.get("signed"):
        sec = rng.integers(-(1 << 62) + 1, (1 << 62) - 1, size=(P, dim), dtype=np.int64)
    else:
        sec = rng.integers(0, case["p"], size=(P, dim), dtype=np.int64)
    d_sec = DeviceBuffer.from_numpy(sec)
    Bs = B if odd else B + 1
    maps = [0] if case.get("additive") else [1, 0] if gen.csprng_share_map() == 1 else [0]
    for share_map in maps:
        if not case.get("additive"):
            gen.set_csprng_share_map(share_map)
        d_out = DeviceBuffer(P * n * Bs).zero()
        gen.generate_batch_dev(d_sec.ptr, P, dim, dim, d_out.ptr, n * Bs, Bs, first_participant=first)
        name = _last_kernel()
        assert case["kernel"] in name, (name, case["kernel"])
        out = d_out.to_numpy().reshape(P, n, Bs)
        want = _want(case, w2, w3, sec, [first + q for q in range(P)], B, share_map)
        for q in range(P):
            bad = np.argwhere(out[q, :, :B] != want[q])
            assert bad.size == 0, f"participant {q}, share map {share_map}: {len(bad)} shares differ, first (row, batch) {bad[:4].tolist()}"
        assert not out[:, :, B:].any()


SINGLE = R.MATRIX_CASES + R.FFT_CASES + R.ADDITIVE_CASES


@pytest.mark.parametrize("case", SINGLE, ids=_ids(SINGLE))
def test_one_draw_in_five_comes_from_the_retry_stream(gpu, case):
    _generate_and_compare(case, case["first"], case["B"], case["odd"])


@pytest.mark.parametrize("case", R.DUAL_CASES, ids=_ids(R.DUAL_CASES))
def test_dual_role_forms_draw_from_the_retry_stream(gpu, case):
    """generate_combine_dev, two tiles: the shares of the second tile and every clerk row of the sums against the oracle (the
    dual-role kernels of l31, mfma and additive sharing; the transform kernel with its clerk sum on the side stream)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    from oracle import coracle
    _knobs(case)
    k, n, p, B, first, tiles, P = case["k"], case["n"], case["p"], case["B"], case["first"], case["tiles"], case["participants"]
    sch, gen, w2, w3 = _generator(case)
    dim = B * k - (1 if k > 1 else 0)
    assert gen.batch_count(dim) == B
    rng = np.random.default_rng(B * 17 + n)
    S = dim + (dim & 1)                                    # the dual-role launch wants 16-byte aligned secret rows (even stride)
    sec = np.zeros((P, S), dtype=np.int64)
    sec[:, :dim] = rng.integers(0, p, size=(P, dim), dtype=np.int64)
    d_sec = DeviceBuffer.from_numpy(sec)
    Bs = (B + 15) // 16 * 16
    comb = crypto.ShareCombiner(sch)
    # both share maps where the family has both (the dual-role l31 and mfma kernels store the draws as rows 0 .. t - 1 under the
    # systematic map): the combiner begins again for each
    maps = [0] if case.get("additive") else [1, 0] if gen.csprng_share_map() == 1 else [0]
    for share_map in maps:
        if not case.get("additive"):
            gen.set_csprng_share_map(share_map)
        comb.begin_dev(n, B)
        bufs = [DeviceBuffer(n * P * Bs).zero() for _ in range(2)]
        for i in range(tiles + 1):
            gen.generate_combine_dev(comb, d_sec.ptr, P if i < tiles else 0, dim, S, bufs[i % 2].ptr, Bs, P * Bs,
                                     d_prev=bufs[(i - 1) % 2].ptr if i else 0, prev_participants=P if i else 0, first_participant=first + i * P)
            if i == 1:
                name = _last_kernel()
                assert case["kernel"] in name, (name, case["kernel"], share_map)
                if "side stream" in case["kernel"]:
                    assert name.startswith("packed_gen_fft_kernel<20, "), name
        d_sums = DeviceBuffer(n * B)
        comb.finish_dev(d_sums.ptr)
        sums = d_sums.to_numpy().reshape(n, B)
        want = _want(case, w2, w3, np.concatenate([sec[:, :dim]] * tiles), [first + x for x in range(tiles * P)], B, share_map)
        tile1 = bufs[1].to_numpy().reshape(n, P, Bs)
        for q in range(P):
            assert np.array_equal(tile1[:, q, :B], want[P + q]), f"dual-role shares of participant {q}, share map {share_map}"
        for c in range(n):
            assert np.array_equal(sums[c], coracle.combine(p, np.stack([w[c] for w in want]))), f"clerk sum {c}, share map {share_map}"


@pytest.mark.parametrize("case", R.MASK_CASES, ids=_ids(R.MASK_CASES))
def test_full_mask_draws_from_the_retry_stream(gpu, case):
    """full_mask_drbg_kernel through mask_batch_dev (one draw per element, T = 1): even strides take its 16-byte path, an odd
    stride with an odd dimension its scalar one.  (The mask calls record no kernel name; a Full scheme has this one kernel.)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    from oracle import coracle
    p, dim, first, P = case["p"], case["B"], case["first"], case["participants"]
    stride = dim if case["odd"] else dim + 1
    assert dim % 2 == 1 and (stride % 2 == 1) == case["odd"]
    rng = np.random.default_rng(dim + stride)
    sec = np.zeros((P, stride), dtype=np.int64)
    sec[:, :dim] = rng.integers(-(1 << 62), 1 << 62, size=(P, dim), dtype=np.int64)
    d_sec = DeviceBuffer.from_numpy(sec)
    masker = crypto.SecretMasker(crypto.Full(p))
    masker.set_drbg_key(R.KEY)
    d_mask, d_masked = DeviceBuffer(P * stride).zero(), DeviceBuffer(P * stride).zero()
    masker.mask_batch_dev(d_sec.ptr, P, dim, stride, d_mask.ptr, stride, d_masked.ptr, stride, first_participant=first)
    masks, masked = d_mask.to_numpy().reshape(P, stride), d_masked.to_numpy().reshape(P, stride)
    for q in range(P):
        want = coracle.drbg_fill(R.KEY, first + q, dim, 1, p)
        assert np.array_equal(masks[q, :dim], want), q
        assert np.array_equal(masked[q, :dim], coracle.addsub(sec[q, :dim], want, p)), q
    assert not masks[:, dim:].any() and not masked[:, dim:].any()


@pytest.mark.parametrize("case", R.PAIRED_CASES, ids=_ids(R.PAIRED_CASES))
def test_paired_rule_rejections_are_redone_from_the_retry_stream(gpu, case):
    """one small job per located stream (participant 1 of 3): an even and an odd batch, two positions b & 7, the last pair of an
    odd count; the first job of a case with an odd row stride"""
    for x, (first, B, _, _) in enumerate(R.paired_jobs(case)):
        _generate_and_compare(case, first, B, odd=x == 0)


@pytest.mark.parametrize("case", R.DEEP_CASES, ids=_ids(R.DEEP_CASES))
def test_second_candidate_and_second_attempt(gpu, case):
    """a job whose located draw finds all eight candidates of attempt 1 rejected (a = 2 in the top byte of word 15), and that
    holds dozens of draws served by candidate j >= 1 of a retry block"""
    stream, b, _ = case["hit"]
    first, B = R.located_job(stream, b)
    _generate_and_compare(case, first, B, odd=True)

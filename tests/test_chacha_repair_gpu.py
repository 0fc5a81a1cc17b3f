"""The rejection repair of the rand-0.3 ChaCha mask expansion on the GPU (pytest -m gpu), on the located seeds of
tests/chacha_repair.py: every case through every entry point that takes it - sda_mask_combiner_combine, sda_secret_masker_mask with
an injected seed in both value modes, sda_mask_combiner_update_dev, update_sealed_rows_dev (with refused rows), and the seeded form
of sda_secret_masker_mask_batch_dev (test library) - bit for bit against the sequential oracle; there is no tolerance, this is integer
arithmetic.  After every call sda_debug_last_mask_plan() must report what the model predicts: whether every key walked in exact
order, the lengths of the two repair lists and the number of keys expanded - a plan kernel that sent every flagged seed to the
exact-order list would give the right sums and the wrong plan.  tests/test_chacha_repair_reach.py proves on the CPU which branches
these cases take.

The per-participant (APPLY) calls get row strides larger than the dimension, any-int64 secrets (negative, >= q, INT64_MIN /
INT64_MAX at the repaired positions) and canaries in every padding word.  Masking in place is refused for the ChaCha kind."""
import ctypes as C

import numpy as np
import pytest

import chacha_repair as cr
from conftest import use_test_hooks
from test_mask_combiner_dev_gpu import _keys, seal_rows, u32

pytestmark = pytest.mark.gpu
CANARY = -0x0123456789ABCDEF
NAMES = [c["name"] for c in cr.CASES]


def last_plan():
    from sda_amd import capi
    out = (C.c_uint * 4)()
    capi.check(capi.load().sda_debug_last_mask_plan(C.byref(out)))
    return tuple(out)


def key_rows(case):
    """the case's seeds, one row of 4 words per key, in key order"""
    return np.concatenate([np.tile(np.array(seed, dtype=np.int64), (n, 1)) for seed, n in case["keys"]])


def want_sum(case, entry="sum"):
    return np.array(cr.oracle_sum(case, entry), dtype=np.int64)


@pytest.mark.parametrize("name", NAMES)
def test_combine_and_update_dev(gpu, name):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    use_test_hooks()
    case = cr.CASE[name]
    q, dim = case["q"], case["dim"]
    S, want, plan = key_rows(case), want_sum(case), cr.model(case, "sum")["plan"]
    comb = crypto.MaskCombiner(crypto.ChaCha(q, dim, 128))
    got = comb.combine(list(S))
    assert last_plan() == plan
    assert np.array_equal(got, want), f"combine: {int((got != want).sum())} of {dim} columns differ"
    stride = 7                                                                # junk after the 4 seed words
    rows = np.full((len(S), stride), CANARY, dtype=np.int64)
    rows[:, :4] = S
    d_S, d_out = DeviceBuffer.from_numpy(rows), DeviceBuffer.from_numpy(np.full(dim + 4, CANARY, dtype=np.int64))
    comb.begin_dev(dim)
    comb.update_dev(d_S.ptr, len(S), 4, stride)
    assert last_plan() == plan
    comb.finish_dev(d_out.ptr, dim)
    out = d_out.to_numpy()
    assert np.array_equal(out[:dim], want), f"update_dev: {int((out[:dim] != want).sum())} of {dim} columns differ"
    assert np.all(out[dim:] == CANARY)


@pytest.mark.parametrize("name", [c["name"] for c in cr.CASES if "counted" in c["entries"]])
def test_update_sealed_rows_dev(gpu, name):
    """the counted route: the first case['refused'] boxes are cut to 47 bytes and give no key, so fewer keys are expanded than the
    grids were sized for"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes
    use_test_hooks()
    case = cr.CASE[name]
    q, dim, refused = case["q"], case["dim"], case["refused"]
    S = key_rows(case)
    pk, sk = _keys(61)
    job = seal_rows(S, pk)
    lens = np.frombuffer(job.d_lens.to_bytes(), dtype="<u8")[:len(S)].copy()
    assert (lens >= 48).all()
    lens[:refused] = 47
    d_lens = DeviceBytes.from_bytes(lens.tobytes())
    comb = crypto.MaskCombiner(crypto.ChaCha(q, dim, 128))
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_status, d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * len(S)).zero()
    d_out = DeviceBuffer(dim)
    comb.begin_dev(dim)
    comb.update_sealed_rows_dev(codec, box, pk, sk, job.d_boxes.ptr, job.slot, d_lens.ptr, len(S), job.slot, d_status.ptr, d_ok.ptr)
    plan = last_plan()
    comb.finish_dev(d_out.ptr, dim)
    ok = u32(d_ok, len(S))
    assert not ok[:refused].any() and ok[refused:].all()
    assert (int(u32(d_status)[0]) & 16 != 0) == (refused > 0)
    assert plan == cr.model(case, "counted")["plan"] and plan[3] == len(S) - refused
    got, want = d_out.to_numpy()[:dim], want_sum(case, "counted")
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {dim} columns differ"


def _distinct(case):
    return list(dict.fromkeys(seed for seed, _ in case["keys"]))


@pytest.mark.parametrize("mode", ["canonical", "rust_signed"])
@pytest.mark.parametrize("name", NAMES)
def test_mask_with_an_injected_seed(gpu, name, mode):
    from oracle import pyoracle as po
    from sda_amd import crypto
    use_test_hooks()
    case = cr.CASE[name]
    q, dim = case["q"], case["dim"]
    masker = crypto.SecretMasker(crypto.ChaCha(q, dim, 128))
    masker.set_value_mode(mode)
    rem = po._rem(mode)
    for k, seed in enumerate(_distinct(case)):
        secrets = cr.secrets_row(dim, q, k)
        if mode == "rust_signed":           # s + m is an i64 sum in the reference (chacha.rs:43): inside +-2^62 it cannot overflow
            secrets = [max(-(1 << 62) + 1, min((1 << 62) - 1, s)) for s in secrets]
        mask, masked = masker.mask(np.array(secrets, dtype=np.int64), np.array(seed, dtype=np.int64))
        one = {"q": q, "dim": dim, "keys": [(seed, 1)]}
        assert last_plan() == cr.model(one, "sum")["plan"]
        want = [rem(s + m, q) for s, m in zip(secrets, cr.oracle_mask(seed, q, dim))]
        assert [int(w) for w in mask] == list(seed)
        assert [int(v) for v in masked] == want, (name, seed)


def _seeded(masker, words, d_secrets, P, dim, s_stride, d_masks, m_stride, d_masked, o_stride):
    from sda_amd import capi
    return capi.load().sda_debug_secret_masker_mask_batch_seeded_dev(masker._h, words.ctypes.data, d_secrets, P, dim, s_stride, 0, d_masks,
                                                                     m_stride, d_masked, o_stride, None)


def _tile(case):
    """secrets [P][dim + 3] of any int64 - the first row of every distinct seed is cr.secrets_row, the specials at the front - the
    seed words, and the oracle's masked rows"""
    q, dim = case["q"], case["dim"]
    S = key_rows(case)
    P = len(S)
    secrets = np.random.default_rng(P + dim).integers(-(1 << 63), (1 << 63) - 1, size=(P, dim + 3), dtype=np.int64)
    masks = np.empty((P, dim), dtype=np.int64)
    r0 = 0
    first = {}
    for seed, n in case["keys"]:
        k = first.setdefault(seed, len(first))
        secrets[r0, :dim] = np.array(cr.secrets_row(dim, q, k), dtype=np.int64)
        masks[r0:r0 + n] = np.array(cr.oracle_mask(seed, q, dim), dtype=np.int64)
        r0 += n
    want = (np.mod(secrets[:, :dim], np.int64(q)) + masks) % np.int64(q)      # both terms below q < 2^62: no overflow
    return S, secrets, want


@pytest.mark.parametrize("name", [c["name"] for c in cr.CASES if "apply" in c["entries"]])
def test_seeded_mask_batch_dev(gpu, name):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    use_test_hooks()
    case = cr.CASE[name]
    q, dim = case["q"], case["dim"]
    S, secrets, want = _tile(case)
    P, s_stride, o_stride, m_stride = len(S), dim + 3, dim + 5, 6
    row = cr.oracle_applied(tuple(int(w) for w in S[0]), q, dim, [int(x) for x in secrets[0, :dim]])           # the vectorised expectation, checked once in Python integers
    assert [int(x) for x in want[0]] == row
    words = np.ascontiguousarray(S, dtype=np.uint32)
    d_sec = DeviceBuffer.from_numpy(secrets)
    d_masks = DeviceBuffer.from_numpy(np.full((P, m_stride), CANARY, dtype=np.int64))
    d_out = DeviceBuffer.from_numpy(np.full((P, o_stride), CANARY, dtype=np.int64))
    masker = crypto.SecretMasker(crypto.ChaCha(q, dim, 128))
    capi.check(_seeded(masker, words, d_sec.ptr, P, dim, s_stride, d_masks.ptr, m_stride, d_out.ptr, o_stride))
    assert last_plan() == cr.model(case, "apply")["plan"]
    out = d_out.to_numpy().reshape(P, o_stride)
    sent = d_masks.to_numpy().reshape(P, m_stride)
    bad = np.argwhere(out[:, :dim] != want)
    assert bad.size == 0, f"{len(bad)} masked values differ, first (participant, position) {bad[:4].tolist()}"
    assert np.all(out[:, dim:] == CANARY) and np.all(sent[:, 4:] == CANARY), "a padding word was written"
    assert np.array_equal(sent[:, :4], S)
    assert np.array_equal(d_sec.to_numpy().reshape(P, s_stride), secrets)


@pytest.mark.parametrize("name", ["r2_at_0", "both_lists", "thr_q8_9"])
def test_masking_in_place_is_refused_for_the_chacha_kind(gpu, name):
    """a shift-route case, one with both lists and an all-exact one: d_masked == d_secrets, and ranges that overlap in one word,
    answer SDA_ERR_INVALID_ARGUMENT and write nothing; the first word after the secrets is a valid place for the result"""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    use_test_hooks()
    case = cr.CASE[name]
    q, dim = case["q"], case["dim"]
    S, secrets, want = _tile(case)
    P, stride = len(S), dim + 3
    words = np.ascontiguousarray(S, dtype=np.uint32)
    span = (P - 1) * stride + dim                                            # words from the first secret to the last
    host = np.full(2 * P * stride, CANARY, dtype=np.int64)
    host[:P * stride] = secrets.reshape(-1)
    d = DeviceBuffer.from_numpy(host)
    d_masks = DeviceBuffer.from_numpy(np.full((P, 4), CANARY, dtype=np.int64))
    masker = crypto.SecretMasker(crypto.ChaCha(q, dim, 128))
    for off in (0, 1, span - 1):
        assert _seeded(masker, words, d.ptr, P, dim, stride, d_masks.ptr, 4, d.at(off), stride) == capi.ERR_INVALID_ARGUMENT
        assert b"in place" in capi.load().sda_last_error()
        assert np.array_equal(d.to_numpy(), host) and np.all(d_masks.to_numpy() == CANARY)
    # the release entry point has the same rule (same code): refused before any seed is drawn
    assert capi.load().sda_secret_masker_mask_batch_dev(masker._h, d.ptr, P, dim, stride, 0, d_masks.ptr, 4, d.ptr, stride, None) == capi.ERR_INVALID_ARGUMENT
    assert np.array_equal(d.to_numpy(), host)
    capi.check(_seeded(masker, words, d.ptr, P, dim, stride, d_masks.ptr, 4, d.at(span), stride))
    out = d.to_numpy()
    assert np.array_equal(out[:span], host[:span])
    got = np.stack([out[span + p * stride:span + p * stride + dim] for p in range(P)])
    assert np.array_equal(got, want)


def test_the_full_kind_still_masks_in_place(gpu):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    q, P, dim = cr.P62, 3, 37
    secrets = np.random.default_rng(3).integers(0, q, size=(P, dim), dtype=np.int64)
    masker = crypto.SecretMasker(crypto.Full(q))
    masker.set_drbg_key(bytes(range(32)))
    d_sec, d_mask, d_out = DeviceBuffer.from_numpy(secrets), DeviceBuffer(P * dim), DeviceBuffer(P * dim)
    masker.mask_batch_dev(d_sec.ptr, P, dim, dim, d_mask.ptr, dim, d_out.ptr, dim, first_participant=5)
    apart = d_out.to_numpy()
    masker.mask_batch_dev(d_sec.ptr, P, dim, dim, d_mask.ptr, dim, d_sec.ptr, dim, first_participant=5)
    assert np.array_equal(d_sec.to_numpy(), apart)

"""Reach checks for tests/test_drbg_retry_gpu.py (CPU): every GPU case there must provably enter the retry stream of the device
CSPRNG, at the batches, positions and participants a wrong retry counter would show at - so a later edit that makes a case
benign (another key, another first participant, fewer batches) fails here and not silently on the GPU.

The first-attempt candidates of every case are recomputed with the numpy restatement of tests/drbg_retry.py (tied to the C
oracle's block function and to the big-int spec below).  For the 0.2-rate cases: at least 20 rejected draws, every position
b & 7 and every draw index rejected at least once, a rejection in the ragged last group and one for a participant other than
the first - and the batch count is the smallest odd one with those properties (the two largest transform shapes keep to three
batches and take the smallest participant count with them instead).  For the located cases (the paired rule; a
second retry attempt) the recorded stream ids are re-derived by the same search, and at every located draw the C oracle
(coracle.drbg_fill, the GPU test's reference) equals the big-int restatement of the spec (pyoracle.drbg_value)."""
import numpy as np
import pytest

import drbg_retry as R


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    from oracle import coracle
    coracle.build()


def test_the_primes_make_rejection_the_rule():
    for use, (p, div) in R.WIDE_PRIMES.items():
        assert R.is_prime(p) and (p - 1) % div == 0 and p < 1 << 62 and R.rejection_rate(p) > 0.19, use
        assert not R.paired(p)
    assert R.is_prime(2 ** 61 - 1) and not R.is_prime(2 ** 61 + 1) and not R.is_prime(3215031751)      # the test itself: a strong pseudoprime to 2, 3, 5, 7
    for use, (p, div) in R.PAIRED_PRIMES.items():
        assert R.is_prime(p) and (p - 1) % div == 0 and R.paired(p), use
        assert p == R.best_paired_prime(div), use                  # the highest rejection rate that admits the shape
        assert 2.0 ** -19 < R.rejection_rate(p) < 2.0 ** -18
    assert R.PAIRED_PRIMES["fft242"][0] == R.NGEMM_VOLUME["p"]


def test_the_numpy_restatement_is_the_oracles_stream():
    """chacha_words against the C oracle's block function (attempt byte and the top part of the stream id in word 15, every round
    count), and first_attempt's word mapping against the spec: where the first attempt is accepted the draw is hi64(x m)"""
    from oracle import coracle, pyoracle as po
    rng = np.random.default_rng(1)
    for rounds, attempt in ((20, 0), (20, 1), (12, 2), (8, 255)):
        ctr = rng.integers(0, 1 << 63, size=5, dtype=np.uint64)
        streams = np.array([0, 1, R.FIRST, R.FIRST_LAST + 2, (1 << 56) - 1], dtype=np.uint64)
        got = R.chacha_words(R.KEY, ctr, streams, attempt, rounds)
        for i in range(5):
            st = list(R.CHACHA_CONST) + R.key_words(R.KEY) + [int(ctr[i]) & 0xFFFFFFFF, int(ctr[i]) >> 32, int(streams[i]) & 0xFFFFFFFF,
                                                              ((int(streams[i]) >> 32) & 0xFFFFFF) | (attempt << 24)]
            assert got[:, i].tolist() == coracle.chacha_block(st, rounds).tolist(), (rounds, attempt, i)
    for m, T in ((R.PM, 3), (R.PAIRED_PRIMES["any"][0], 5)):
        B = 21
        x, rej = R.first_attempt(R.KEY, [R.FIRST + 1], B, T, m)
        want = coracle.drbg_fill(R.KEY, R.FIRST + 1, B, T, m).reshape(B, T)
        for b in range(B):
            for i in range(T):
                d = i >> 1 if R.paired(m) else i
                if not rej[0, b, d]:
                    xm = int(x[0, b, d]) * m
                    val = (((xm & R.M64) * m) >> 64 if i & 1 else xm >> 64) if R.paired(m) else xm >> 64
                    assert want[b, i] == val == po.drbg_value(R.KEY, R.FIRST + 1, b, T, i, m), (m, b, i)
                else:
                    assert R.retry_depth(R.KEY, R.FIRST + 1, b, d, T, m)[0] >= 1


@pytest.mark.parametrize("case", R.WIDE_CASES, ids=[c["name"] for c in R.WIDE_CASES])
def test_wide_cases_reject_one_draw_in_five_where_it_matters(case):
    from oracle import coracle, pyoracle as po
    B, T, p, rounds = case["B"], case["T"], case["p"], case.get("rounds", 20)
    streams = R.case_streams(case)
    assert len(streams) >= 3 and all(s >> 32 for s in streams) and streams[-1] < 1 << 56
    assert B % 2 == 1 and B % 8 != 0
    rej = R.case_rejections(case)
    count, pos, idx, last, others = R.coverage(rej)
    assert count >= 20 and last >= 1 and others >= 1, (count, last, others)
    assert pos == set(range(min(B, 8))), pos
    assert idx == set(range(T)), sorted(set(range(T)) - idx)
    if case["fixed"]:
        # three batches (positions 0 .. 2 are all there are): the participant count is the smallest that covers every draw index
        assert B == 3 and len(streams) == R.smallest_participants(R.KEY, case["first"], B, T, p, rounds, limit=len(streams))
    else:
        assert len(streams) == R.PARTICIPANTS * case.get("tiles", 1)
        assert B == R.smallest_batches(R.KEY, streams, T, p, rounds, limit=B + 2)          # no smaller job covers the same
    # the reference of the GPU test against the big-int spec at rejected draws of the last participant (a few per case)
    q = len(streams) - 1
    got = coracle.drbg_fill(R.KEY, streams[q], B, T, p, rounds).reshape(B, T)
    for b, i in np.argwhere(rej[q])[:3]:
        assert got[b, i] == po.drbg_value(R.KEY, streams[q], int(b), T, int(i), p, rounds), (b, i)


def test_every_family_has_a_case_with_an_odd_row_stride_and_the_last_ids_are_used():
    for table in (R.MATRIX_CASES, R.FFT_CASES, R.ADDITIVE_CASES, R.MASK_CASES):
        assert any(c["odd"] for c in table)
    for prefix in ("mfma", "l31", "mont64", "generic", "fft", "additive", "full-mask"):
        assert any(c["odd"] for c in R.WIDE_CASES if c["name"].startswith(prefix)), prefix
    assert sum(c["first"] == (1 << 56) - R.PARTICIPANTS for c in R.WIDE_CASES) >= 1


@pytest.mark.parametrize("key", sorted(R.PAIRED_HITS), ids=[f"p{m}-T{T}" for m, T in sorted(R.PAIRED_HITS)])
def test_paired_rule_rejections_are_where_the_table_says(key):
    from oracle import coracle, pyoracle as po
    m, T = key
    hits = R.PAIRED_HITS[key]
    assert hits == R.locate_paired(m, T)                           # the search, re-derived
    assert any(c["p"] == m and c["t"] == T for c in R.PAIRED_CASES)
    batches = [b for _, pairs in hits for b, _ in pairs]
    assert any(b & 1 for b in batches) and any(not b & 1 for b in batches)        # lanes r0 and r1 of drbg_pair
    assert len({b & 7 for b in batches}) >= 2
    for case in (c for c in R.PAIRED_CASES if (c["p"], c["t"]) == key):
        for first, B, stream, pairs in R.paired_jobs(case):
            assert B <= R.PAIRED_BATCHES + 1 and B % 2 == 1 and first >> 32 and first + 1 == stream
            _, rej = R.first_attempt(R.KEY, [first + q for q in range(R.PARTICIPANTS)], B, T, m)
            assert [(int(b), int(j)) for b, j in np.argwhere(rej[1])] == pairs         # a participant other than the first
            got = coracle.drbg_fill(R.KEY, stream, B, T, m).reshape(B, T)
            for b, j in pairs:
                assert R.retry_depth(R.KEY, stream, b, j, T, m)[0] >= 1
                for i in range(2 * j, min(2 * j + 2, T)):
                    assert got[b, i] == po.drbg_value(R.KEY, stream, b, T, i, m), (stream, b, i)


def test_paired_hits_include_the_discarded_half_of_an_odd_count():
    """the last pair of an odd T (its second element is discarded): in the transform kernel AND in the one-limb kernels"""
    for want in ("fft-paired-40-23-242-lazy", "n31-paired-8-7-26"):
        case = next(c for c in R.PAIRED_CASES if c["name"] == want)
        T = case["t"]
        assert T % 2 == 1 and any(j == T // 2 for _, pairs in R.PAIRED_HITS[(case["p"], T)] for _, j in pairs), want
    assert {c["t"] % 2 for c in R.PAIRED_CASES if c["name"].startswith("n31")} == {0, 1}


@pytest.mark.parametrize("case", R.DEEP_CASES, ids=[c["name"] for c in R.DEEP_CASES])
def test_a_draw_needs_the_second_candidate_and_one_a_second_attempt(case):
    from oracle import coracle, pyoracle as po
    m, T = case["p"], case["t"]
    stream, b, i = case["hit"]
    found = R.locate_second_attempt(m, T)
    assert found[:3] == case["hit"] and found[3] <= 4 << 20, found            # re-derived; the scan stays below 4 Mi draws
    a, j = R.retry_depth(R.KEY, stream, b, i, T, m)
    assert a >= 2, (a, j)
    first, B = R.located_job(stream, b)
    assert B <= R.DEEP_BATCHES + 1 and first >> 32
    streams = [first + q for q in range(R.PARTICIPANTS)]
    _, rej = R.first_attempt(R.KEY, streams, B, T, m)
    assert rej[1, b, i]
    s, bb, ii = np.nonzero(rej)
    second = R.retry_attempt(R.KEY, np.array(streams, dtype=np.uint64)[s], bb, ii, T, m, 1)[:, 0]      # candidate 0 of attempt 1 rejected too
    assert second.sum() >= 20, second.sum()                                   # candidate j >= 1 of a retry block serves the draw
    got = [coracle.drbg_fill(R.KEY, streams[q], B, T, m).reshape(B, T) for q in range(R.PARTICIPANTS)]
    located = [(1, b, i)] + [(int(s[x]), int(bb[x]), int(ii[x])) for x in np.flatnonzero(second)[:5]]
    for q, b1, i1 in located:
        assert got[q][b1, i1] == po.drbg_value(R.KEY, streams[q], b1, T, i1, m), (q, b1, i1)


def test_the_limb_gemm_volume_job_rejects_in_a_lanes_second_block():
    """tests/test_ngemm_gpu.py::test_narrow_limb_gemm_rejected_draw_pairs_are_redone_from_the_retry_stream marks a rejected pair in
    a 64-bit mask, eight bits per block of the lane; its job must hold a rejected pair at bit 8 or above (ng_draw_fixup's
    `bit >> 3` term), or a fixup that only handled a lane's first block would pass it"""
    V = R.NGEMM_VOLUME
    bits = []
    for q in range(V["participants"]):
        _, rej = R.first_attempt(V["key"], [V["first"] + q], V["batches"], V["t"], V["p"])
        bits += [R.ngemm_rej_bit(int(b), int(j), V["t"], V["wgb"], V["workers"]) for b, j in np.argwhere(rej[0])]
    assert len(bits) >= 20, len(bits)
    assert sum(bit >= 8 for bit in bits) >= 3 and sum(bit < 8 for bit in bits) >= 3, sorted(bits)
    assert max(bits) < 16                       # 768 blocks per workgroup on 512 lanes: two rounds


PACKED = [c for c in R.WIDE_CASES + R.PAIRED_CASES + R.DEEP_CASES if not c.get("additive") and not c.get("mask")]


@pytest.mark.parametrize("case", PACKED, ids=[c["name"] for c in PACKED])
def test_the_library_selects_the_family_each_case_names(case):
    """sda_debug_select_path on the host: with the case's prime, omegas and knobs the call runs the family whose kernel the GPU
    test expects by name (the knobs that do not take part in the selection - batches per workgroup, lazy levels - left out)"""
    import __graft_entry__ as ge
    ge.build()
    from test_path_select import select
    from sda_amd import capi
    w2, w3 = R.omegas(case)
    knobs = ",".join(kn for kn in case["knobs"] if isinstance(kn, str) and kn != "SDA_NO_LAZY")
    got = select(capi.hooks_library(), case["k"], case["t"], case["n"], case["p"], w2, w3, knobs=knobs)
    rounds = case.get("rounds", 20)
    if case.get("tiles"):
        want = "none" if R.family_of(case) == "fft" else R.family_of(case)          # the transform kernel has no dual-role form
        assert got["fused20"] == want, got
    else:
        assert got["call20" if rounds == 20 else "call12"] == R.family_of(case), got
    if R.family_of(case) == "fft":
        assert got["wide"] == "fft" and got["transform_shape"] == "1", got

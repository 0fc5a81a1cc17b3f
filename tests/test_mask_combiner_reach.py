"""CPU proof that the seeds test_mask_combiner_dev_gpu.py feeds the mask combiner's device form reach the three outcomes of
its repair-plan kernel (clean, shift list, exact-order list) and the tail walk of the shift pass: the rejected candidates of
every seed are counted with the oracle's rand-0.3 ChaCha stream."""
import numpy as np
import pytest

import mask_combiner_cases as mc
from oracle import pyoracle as po


def test_the_vectorised_stream_is_the_oracles():
    S = mc.seed_matrix(*mc.BOTH_LISTS)[:3]
    v = mc.candidates(S, 3)
    for r in range(3):
        rng = po.ChaChaRng([int(w) for w in S[r]])
        assert [rng.next_u64() for _ in range(24)] == [int(x) for x in v[r]]
    long_seed = np.array([[(1 << 40) + 5, -1, 1 << 32, 7, 8, 9, 10, 11, 12, 13]], dtype=np.int64)   # `as u32`, first 8 words
    rng = po.ChaChaRng([int(w) for w in long_seed[0]])
    assert [rng.next_u64() for _ in range(8)] == [int(x) for x in mc.candidates(long_seed, 1)[0]]
    assert mc.zone(433) == (1 << 64) - 1 - ((1 << 64) - 1) % 433


def test_which_shapes_take_exact_order_for_all():
    took = [s for s in mc.CHACHA_SHAPES if mc.all_exact_order(s[0], s[1])]
    assert took == [(mc.Q_HEAVY, 3000, 6)]
    assert not mc.all_exact_order(*mc.STREAM_ORDER[:2])


def test_the_case_meant_for_both_lists_fills_both():
    q, dim, seeds = mc.BOTH_LISTS
    count, _ = mc.rejections(mc.seed_matrix(q, dim, seeds), q, dim)
    assert (count == 0).any(), "no clean seed"
    assert ((count >= 1) & (count <= 3)).any(), "no seed for the shift list"
    assert (count > 3).any(), "no seed for the exact-order list"


@pytest.mark.parametrize("q,dim,seeds", mc.SHORT_STREAMS)
def test_short_streams_walk_past_the_dimension(q, dim, seeds):
    S = mc.seed_matrix(q, dim, seeds)
    v = mc.candidates(S, (dim + 16 + 7) // 8)
    bad = v >= np.uint64(mc.zone(q))
    count = bad[:, :dim].sum(axis=1)
    shift = (count >= 1) & (count <= 3)
    # a seed with R recorded rejections takes its last R masks from candidates `dim` onwards: the shifted tail runs past `dimension`
    assert shift.any(), "no seed whose shifted tail runs past dimension"
    last = np.array([bad[r, dim - 1] for r in range(seeds)])
    assert (shift & last).any(), "no rejection at the last position of a stream"
    if q == mc.Q_HEAVY:        # the tail itself meets a rejected candidate
        assert any(bad[r, dim:dim + int(count[r])].any() for r in np.nonzero(shift)[0])


def test_the_2_pow_minus_13_case_has_fix_ups_and_clean_seeds():
    q, dim, seeds = (1 << 62) - (1 << 49), 2000, 60
    count, _ = mc.rejections(mc.seed_matrix(q, dim, seeds), q, dim)
    assert (count == 0).any() and (count > 0).any()


def test_stream_order_case_needs_its_repair_lists():
    q, dim, n = mc.STREAM_ORDER
    A, B = mc.stream_order_seeds()
    ca, _ = mc.rejections(A, q, dim)
    cb, _ = mc.rejections(B, q, dim)
    assert ((ca >= 1) & (ca <= 3)).any() and ((cb >= 1) & (cb <= 3)).any()
    assert not np.array_equal(A, B)

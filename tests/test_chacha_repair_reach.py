"""CPU proof of what tests/test_chacha_repair_gpu.py relies on (tests/chacha_repair.py): the Python-integer model of the ChaCha mask
driver equals the oracle on every case, every located seed takes the branches it is pinned for, the cases together take every
branch that is not declared out of reach, the plan prediction agrees with the library's host-side threshold on both sides of each
edge, and every planted fault is noticed by a case that names the branch it breaks.  No search runs here: the seeds are constants."""
import pytest

import chacha_repair as cr
import mask_combiner_cases as mc
from oracle import pyoracle as po


def _oracle(case, entry):
    if entry != "apply":
        return cr.oracle_sum(case, entry)
    seeds = list(dict.fromkeys(seed for seed, _ in case["keys"]))
    return {seed: cr.oracle_applied(seed, case["q"], case["dim"], cr.secrets_row(case["dim"], case["q"], k)) for k, seed in enumerate(seeds)}


def _differs(case, faults, **kw):
    return [e for e in case["entries"] if cr.model(case, e, faults, **kw)["result"] != _oracle(case, e)]


def test_the_c_oracle_is_sequential_gen_range():
    """the reference of the reference: rand-0.3 gen_range(0, q) drawn one after the other from ChaChaRng, in Python integers"""
    for name, (seed, q, dim, _) in cr.SEEDS.items():
        if dim <= 64:
            rng = po.ChaChaRng(list(seed))
            assert [rng.gen_range_i64(0, q) for _ in range(dim)] == list(cr.oracle_mask(seed, q, dim)), name


@pytest.mark.parametrize("name", [c["name"] for c in cr.CASES])
def test_model_equals_oracle_and_takes_its_pinned_branches(name):
    case = cr.CASE[name]
    taken = set()
    for entry in case["entries"]:
        m = cr.model(case, entry)
        assert m["result"] == _oracle(case, entry), (name, entry)
        assert m["plan"][0] == int(mc.all_exact_order(case["q"], case["dim"]))
        assert m["plan"][3] == sum(n for _, n in case["keys"]) - (case["refused"] if entry == "counted" else 0)
        taken |= m["branches"]
    assert case["pins"] <= taken, (name, sorted(case["pins"] - taken))
    assert 3 <= case["dim"] <= 2049 or name == "three_chunks"


def test_every_branch_is_taken_or_declared_out_of_reach():
    taken = set()
    for case in cr.CASES:
        for entry in case["entries"]:
            taken |= cr.model(case, entry)["branches"]
    assert len(set(cr.BRANCHES)) == len(cr.BRANCHES) and set(cr.REACH) <= set(cr.BRANCHES)
    assert taken == set(cr.BRANCHES) - set(cr.REACH), (sorted(taken ^ (set(cr.BRANCHES) - set(cr.REACH))))
    pinned = set().union(*(c["pins"] for c in cr.CASES))
    assert pinned == taken, sorted(taken - pinned)                       # every branch has a case that names it
    for fault, hit in cr.FAULTS.items():
        assert hit <= set(cr.BRANCHES), fault


def test_thresholds_of_exact_order_for_all():
    for q, last_shift, first_exact in cr.THRESHOLDS:
        assert first_exact == last_shift + 1
        assert not mc.all_exact_order(q, last_shift) and mc.all_exact_order(q, first_exact)
        for dim in (last_shift, first_exact):
            cases = [c for c in cr.CASES if (c["q"], c["dim"]) == (q, dim)]
            assert cases, (q, dim)
            for c in cases:
                assert cr.model(c, "sum")["plan"][0] == int(dim == first_exact)
    assert not any(mc.all_exact_order(cr.P62, d) for d in (3, 2049, 1 << 20))


@pytest.mark.parametrize("fault", sorted(cr.FAULTS))
def test_each_planted_fault_is_noticed_by_a_case_that_names_its_branch(fault):
    for branch in sorted(cr.FAULTS[fault]):
        named = [c for c in cr.CASES if branch in c["pins"]]
        assert named, branch
        caught = [c["name"] for c in named if _differs(c, {fault})]
        print(f"{fault}: {branch} caught by {caught}")
        assert caught, (fault, branch)


def test_the_chunk_edge_cases_sit_on_their_seeds_own_first_chunk():
    """`dimension` = 2048 - R and one more, R the rejected among the seed's first 2048 candidates, on both routes"""
    for name, q, fit in (("chunk_fit", cr.Q2048, "chunk_fit"), ("clean8", cr.Q8, "all_exact_chunk_fit")):
        R = cr.first_chunk_rejections(cr.SEEDS[name][0], q)
        assert cr.CASE[fit]["dim"] == cr.CHUNK - R and cr.CASE[fit + "_plus_1"]["dim"] == cr.CHUNK - R + 1, (name, R)
    assert mc.all_exact_order(cr.Q8, cr.CASE["all_exact_chunk_fit"]["dim"]) and not mc.all_exact_order(cr.Q2048, cr.CASE["chunk_fit_plus_1"]["dim"])


def test_a_chunk_too_many_changes_nothing():
    for case in cr.CASES:
        if case["pins"] & {"slow_chunk_exact_fit", "slow_next_chunk_one_mask", "slow_three_chunks", "exact_R4", "all_exact"} and case["dim"] <= 4100 \
                and sum(n for _, n in case["keys"]) < 100:
            assert not _differs(case, cr.BENIGN_FAULTS), case["name"]


def test_in_place_masking_is_wrong_exactly_where_a_repair_overwrites():
    """why sda_secret_masker_mask_batch_dev refuses d_masked == d_secrets for the ChaCha kind: mask_apply_put reads `secrets` again"""
    apply_only = lambda c: dict(c, entries=("apply",))
    assert _differs(apply_only(cr.CASE["r2_at_0"]), (), aliased=True)
    assert _differs(apply_only(cr.CASE["r4"]), (), aliased=True)
    assert not _differs(apply_only(cr.CASE["thr_q8_9"]), (), aliased=True)      # every position written once
    assert not _differs(apply_only(cr.CASE["clean8"]), (), aliased=True)

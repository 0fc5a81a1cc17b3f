"""What the cases of tests/reveal_limits.py reach, shown on the CPU (no device): every case passes the integer model of the kernel
its route names, register by register, and the model equals the plain Python-integer Lagrange reconstruction; route() names every
instance, partition form and branch; the sign-aligned batches bring the n31 kernel's group sum S to the stated fraction of the
bound |S| < p 2^31 that n31_redc needs, where the p - 1 / 0 / 1 rows of tests/test_extremes_gpu.py stay 2^-28 below it.  The floors
are stated here and were not tuned against the device code: 0.6 of p 2^31 at 2^31 - 1 with 7 or more rows (4 terms per sum: the
mean |constant| of the best group is at least 0.6 of p / 2), 0.5 just below 2^29 with 15 or 16 rows (16 terms per sum).  Just above
2^29 the launcher sums 4 terms and the same rows reach 0.13 - 0.23: that edge is why GROUP changes there.
tests/test_reveal_limits_gpu.py runs the same cases on the device."""
import numpy as np
import pytest

import extremes as X
import reveal_limits as L

ALL = L.CASES + [c for steps in L.REUSE.values() for c in steps]


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_case_passes_the_model_and_the_model_is_the_reconstruction(case):
    k, dim = case["k"], case["dim"]
    want = L.reference(case["name"])
    assert want.shape == (dim,) and want.min() >= 0 and want.max() < case["p"]
    got, stats = L.run_model(case)
    for b, secrets in got.items():
        for e, s in enumerate(secrets):
            if b * k + e < dim:
                assert s == want[b * k + e], (b, e)
    assert L.fractions(case, stats) == L.REACH[case["name"]]
    if not case["sample"]:                                            # the C oracle agrees with the Python integers (canonical rows)
        from oracle import coracle
        w2, w3 = L.roots(case["p"], k, case["t"], case["n"])
        rows = np.mod(L.make_rows(case["name"]), case["p"])
        assert np.array_equal(coracle.packed_reconstruct(case["p"], k, case["t"], w2, w3, dim, list(case["indices"]), rows), want)


def test_route_restates_the_launchers():
    P = L.P62
    assert L.route(X.P31MAX, 16, 16, True, True, 1030, 1030) == ("packed_reconstruct_n31_kernel<16, 4>", 65536)
    assert L.route(X.P29_BELOW, 3, 7, True, True, 1030, 1030) == ("packed_reconstruct_n31_kernel<8, 16>", 12288)
    assert L.route(X.P31MAX, 3, 7, True, True, 1030, 1030, no_narrow=True) == ("packed_reconstruct_vec_kernel<8>", 12288)
    assert L.route(L.P31_ABOVE, 3, 4, True, True, 1030, 1030)[0] == "packed_reconstruct_vec_kernel<4>"
    assert L.route(P, 17, 17, True, True, 32764, 32763)[0] == "packed_reconstruct_kernel groups=9 e_per_group=2"
    assert L.route(P, 3, 4, True, True, 262101, 262100)[0] == "packed_reconstruct_kernel groups=2 e_per_group=2"
    assert L.route(P, 3, 4, True, True, 524289, 524289)[0] == "packed_reconstruct_kernel groups=1 e_per_group=3"
    assert L.route(P, 20, 33, True, True, 76600, 76600)[0] == "packed_reconstruct_kernel groups=7 e_per_group=3"
    for kw in (dict(shares_aligned=False, out_aligned=True, stride=1030), dict(shares_aligned=True, out_aligned=False, stride=1030),
               dict(shares_aligned=True, out_aligned=True, stride=1031)):
        assert L.route(X.P31MAX, 8, 15, batches=1030, **kw)[0] == "packed_reconstruct_kernel groups=8 e_per_group=1"
    assert L.partition(17, 32763) == (128, 9, 2) and L.partition(20, 76600) == (300, 7, 3) and L.partition(3, 524289) == (2049, 1, 3)


def test_every_instance_partition_form_and_branch_is_named():
    seen = set()
    for c in ALL:
        seen |= L.coverage(c)
    for nmax in (4, 8, 16):
        assert f"packed_reconstruct_vec_kernel<{nmax}>" in seen
        for group in (4, 16):
            assert f"packed_reconstruct_n31_kernel<{nmax}, {group}>" in seen
    # the grouped kernel: one secret per group, several with a short last group, a single group
    assert {"e_per_group=1", "e_per_group>1", "short last group", "groups=1", "truncated batch"} <= seen
    short = [c for c in L.CASES if "short last group" in L.coverage(c)]
    assert {(c["k"], L.partition(c["k"], c["B"])[1:]) for c in short} == {(17, (9, 2)), (3, (2, 2)), (20, (7, 3))}
    # both load branches of the last lane, every store branch, the largest dynamic LDS the kernels ever ask for
    assert {"load pair", "load single", "idle lane", "store pair", "store single", "store nothing", "more than one workgroup",
            "lds=65536"} <= seen
    for kernel in ("n31", "vec"):
        mine = [c for c in L.CASES if f"_{kernel}_kernel" in c["kernel"]]
        for nmax in (4, 8, 16):
            got = set().union(*(L.coverage(c) for c in mine if f"kernel<{nmax}" in c["kernel"]))
            assert {"load pair", "load single", "store pair", "store single", "store nothing"} <= got, (kernel, nmax)
        assert any(c["lds"] == 65536 for c in mine)
    # a single batch: one lane loads one value and stores one secret
    one = [c for c in L.CASES if c["B"] == 1 and c["dim"] == 1]
    assert one and all({"load single", "store single"} <= L.coverage(c) and "load pair" not in L.coverage(c) for c in one)
    # 2147483659 is the first prime above 2^31 and never takes the narrow kernel; every smaller grid prime does where the layout allows
    assert all(L.P31_ABOVE % d for d in range(2, 46342)) and not any(all(q % d for d in range(2, 46342)) for q in range(1 << 31, L.P31_ABOVE))
    for c in L.CASES:
        if c["name"].startswith("grid-"):
            rows = len(c["indices"])
            assert L.narrow_route(c) == (c["p"] < (1 << 31) and rows <= 16), c["name"]
            assert c["twin"] == (c["p"] < (1 << 31))
    # scattered, unsorted index subsets everywhere
    assert all(list(c["indices"]) != sorted(c["indices"]) for c in ALL if len(c["indices"]) > 2)


def test_sign_aligned_batches_reach_the_stated_fraction_of_the_bound():
    """the floors hold for every narrow case that runs a whole cycle of target rows (B >= 8 k): the recorded |S| / (p 2^31)"""
    floored = 0
    for c in ALL:
        rows = len(c["indices"])
        floor = L.floor_for(c["p"], rows)
        if not (L.narrow_route(c) and floor and c["B"] >= 8 * c["k"]):
            continue
        S, t = L.REACH[c["name"]]
        assert S >= floor, (c["name"], S)
        assert t < 1.0
        floored += 1
    assert floored >= 30
    # every narrow case stays inside the bound, and the 4-term edge above 2^29 reaches far less than the 16-term one below it
    for c in ALL:
        if L.narrow_route(c):
            assert L.REACH[c["name"]][0] < 1.0 and L.REACH[c["name"]][1] < 1.0
    above = [L.REACH[c["name"]][0] for c in L.CASES if c["p"] == X.P29_ABOVE and len(c["indices"]) in (15, 16) and L.narrow_route(c)]
    assert above and max(above) < 0.25


@pytest.mark.parametrize("p", [q for q in L.GRID_PRIMES if q < (1 << 31)])
def test_the_older_maximal_shares_stay_far_below_the_bound(p):
    """tests/test_extremes_gpu.py::test_reconstruct_maximal_shares feeds p - 1, 0 and 1: centred -1, 0 and 1, so |S| <= GROUP p / 2,
    below 2^-20 of p 2^31 - the unsigned worst case, not the narrow kernel's"""
    rng = np.random.default_rng(p % 1000)
    for rows, k, t, n in ((3, 1, 2, 7), (7, 3, 4, 11), (15, 8, 7, 19)):
        idx = L.choose_indices(p, k, t, n, rows)
        C31 = L.r31(L.matrix(p, k, t, n, idx), p)
        stats = dict(S=0, t=0, acc=0)
        for _ in range(24):
            col = [int(x) for x in rng.choice(np.array([p - 1, p - 1, p - 1, 0, 1], dtype=np.int64), size=rows)]
            M = L.matrix(p, k, t, n, idx)
            assert L.model_n31(p, C31, col, stats) == [sum(m * v for m, v in zip(row, col)) % p for row in M]
        assert 0 < stats["S"] << 20 < p << 31

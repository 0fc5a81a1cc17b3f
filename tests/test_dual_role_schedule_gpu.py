"""The dual-role launch over its schedule space (pytest -m gpu): every case of tests/dual_role_schedule.py through
generate_combine_dev, bit-exact against the C oracle and Python integer sums.

The other dual-role tests pin the numbers inside the launch; they run it with a period of 1 or with one large odd period.  The
cases here walk what fuse_plan and the role map of fuse_role / fuse_dispatch decide - the even-to-odd period correction, the grid
extension with idle positions, the clamp once the clerk items are used up, one, two, three and 64 row splits beside one and several
column blocks, tiles whose row count differs from the previous tile's, odd B and dimension 1, first and drain calls - in every
family that has a dual-role kernel.  Per case:
  * every element of every generated tile against coracle.packed_generate_csprng / additive_generate on coracle.drbg_fill (never
    the library's own generate_batch_dev);
  * all n x B clerk sums after finish_dev against clerk_limits.want (Python integers) over the oracle's shares (pipelines) or
    over crafted any-int64 rows (crafted previous tiles: a row summed twice or skipped changes the sum whatever its value);
  * the output buffers are pre-filled with a sentinel: columns B .. Bs - 1 and the rows beyond the call's participants are unchanged;
  * the kernel instance by name (sda_debug_last_kernel), and the plan the library made (sda_debug_last_fuse_plan) equal to the
    model's - for the layouts fuse_plan refuses: "(two launches)" and fused = 0;
  * three runs in a row with fresh handles, equal results: a role map that depended on the dispatch order would show.
tests/test_dual_role_schedule_reach.py proves on the CPU that the table reaches every class and notices every planted fault."""
import ctypes as C
import functools

import numpy as np
import pytest

import clerk_limits as CL
import dual_role_schedule as S
import extremes as X
from conftest import use_test_hooks

pytestmark = pytest.mark.gpu

KEY = bytes(range(7, 39))
SENTINEL = int(np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64).view(np.int64)[0])
RUNS = 3
BY_NAME = {c.name: c for c in S.CASES}


def _scheme(case):
    from sda_amd import crypto
    if case.family == "additive":
        return crypto.Additive(case.n, case.p), None, None
    w2, w3 = X.omegas(case.p, case.k, case.t, case.n)
    return crypto.PackedShamir(case.k, case.n, case.t, case.p, w2, w3), w2, w3


def _generator(case, sch):
    from sda_amd import crypto
    gen = crypto.ShareGenerator(sch)
    gen.set_drbg_key(KEY)
    if case.rounds != 20:
        gen.set_drbg_rounds(case.rounds)                       # (only a handle in deterministic mode takes another round count)
    return gen


def _first(i):
    return 1000 * i + 5                                        # stream ids of call i: first + q


def _rows(case):
    """rows in a clerk's stride: one more than any call generates or sums, so every buffer has rows no call may touch"""
    return max(max(P, prev) for P, prev in S.calls_of(case)) + 1


@functools.lru_cache(maxsize=None)
def _expect(name):
    """computed once per case, shared by its runs and left unchanged: the secrets, per call the oracle's shares [n][P][B] (None: a
    drain call) and the crafted previous tile [n][prev][B] (None: a pipeline), and the clerk sums [n][B]"""
    from oracle import coracle
    case = BY_NAME[name]
    sch, w2, w3 = _scheme(case)
    share_map = _generator(case, sch).csprng_share_map()
    calls, length = S.calls_of(case), S.length_of(case)
    stride = (length | 1) if case.layout == "fallback: odd secrets stride" else length + (length & 1)
    sec = np.zeros((max(P for P, _ in calls), stride), dtype=np.int64)
    sec[:, :length] = np.random.default_rng(case.B * 1000 + case.n).integers(0, case.p, size=(sec.shape[0], length), dtype=np.int64)
    shares, crafted = [], []
    for i, (P, prev) in enumerate(calls):
        tile = np.empty((case.n, P, case.B), dtype=np.int64) if P else None
        for q in range(P):
            draws = coracle.drbg_fill(KEY, _first(i) + q, case.B, case.t, case.p, case.rounds)
            tile[:, q, :] = (coracle.additive_generate(case.p, case.n, sec[q, :length], draws) if case.family == "additive" else
                             coracle.packed_generate_csprng(case.p, case.k, case.t, case.n, w2, w3, sec[q, :length], draws, share_map))
        shares.append(tile)
        crafted.append(CL.crafted_jobs(case.n, prev, case.B, case.p, i) if case.kind == "crafted prev" and prev else None)
    summed = [t for t in (crafted if case.kind == "crafted prev" else shares) if t is not None]
    for a in [sec] + summed:
        a.setflags(write=False)
    return sec, shares, crafted, CL.want(np.concatenate(summed, axis=1), case.p)


def _sentinel_tile(case, fill=None, offset=0):
    """a device buffer of [n][rows][Bs] sentinels (+ `offset` elements in front, as many behind), `fill` [n][r][B] written into its
    top left corner -> (buffer, pointer of the tile)"""
    from sda_amd.device import DeviceBuffer
    n, R, Bs = case.n, _rows(case), case.Bs
    host = np.full(n * R * Bs + 2 * offset, SENTINEL, dtype=np.int64)
    if fill is not None:
        host[offset:offset + n * R * Bs].reshape(n, R, Bs)[:, :fill.shape[1], :case.B] = fill
    d = DeviceBuffer.from_numpy(host)
    return d, d.at(offset)


def _run(case, exp):
    """the case's calls on fresh handles -> (generated tiles as read back [n][rows][Bs] or None, sums [n][B], kernel names, plans)"""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    sec, _, crafted, _ = exp
    lib = capi.load()
    sch, _, _ = _scheme(case)
    gen = _generator(case, sch)
    comb = crypto.ShareCombiner(sch)
    n, R, B, Bs = case.n, _rows(case), case.B, case.Bs
    d_sec = DeviceBuffer.from_numpy(sec)
    comb.begin_dev(n, B)
    outs, names, plans, keep = [], [], [], []
    prev_ptr = 0
    for i, (P, prev) in enumerate(S.calls_of(case)):
        d_out, out_ptr = _sentinel_tile(case) if P else (None, 0)
        if case.kind == "crafted prev" and prev:
            d_prev, prev_ptr = _sentinel_tile(case, crafted[i], 1 if case.layout == "fallback: d_prev off by 8 bytes" else 0)
            keep.append(d_prev)
        if prev:
            assert prev_ptr % 16 == (8 if case.layout == "fallback: d_prev off by 8 bytes" else 0)
        gen.generate_combine_dev(comb, d_sec.ptr if P else 0, P, S.length_of(case), sec.shape[1], out_ptr, Bs, R * Bs,
                                 d_prev=prev_ptr if prev else 0, prev_participants=prev, first_participant=_first(i))
        names.append(lib.sda_debug_last_kernel().decode())
        plan = (C.c_ulonglong * 8)()
        capi.check(lib.sda_debug_last_fuse_plan(C.byref(plan)))
        plans.append(tuple(int(x) for x in plan))
        outs.append(d_out)
        if case.kind == "pipeline":
            prev_ptr = out_ptr                                 # the next call sums what this one generated
    d_sums = DeviceBuffer(n * B)
    comb.finish_dev(d_sums.ptr)
    sums = d_sums.to_numpy().reshape(n, B)                     # (synchronises: every buffer above may go after this)
    return [d.to_numpy().reshape(n, R, Bs) if d else None for d in outs], sums, names, plans


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_dual_role_schedule(gpu, case):
    use_test_hooks()                                           # sda_debug_last_fuse_plan exists in the test library only
    exp = _expect(case.name)
    _, shares, _, want_sums = exp
    calls = S.calls_of(case)
    model = [S.hook_fields(pl, 0 if case.layout else 1) for pl in S.plans_of(case)]
    if case.family in ("mfma", "n31"):
        from test_extremes_gpu import expected_kernel
        assert case.kernel == expected_kernel(case.family, case.k, case.t, case.p, fused=True)
    first_run = None
    for run in range(RUNS):
        tiles, sums, names, plans = _run(case, exp)
        for i, (P, prev) in enumerate(calls):
            what = f"run {run}, call {i} ({P} participants, {prev} previous rows)"
            print(f"{case.name}: {what}: {names[i]}, plan {plans[i]}")
            assert plans[i] == model[i], f"{what}: the library planned {plans[i]}, the model {model[i]}"
            if case.layout is None:
                assert names[i] == case.kernel, f"{what}: {names[i]}"
            else:
                assert names[i].endswith("(two launches)") and "fused" not in names[i], f"{what}: {names[i]}"
            if not P:
                continue
            bad = np.argwhere(tiles[i][:, :P, :case.B] != shares[i])
            assert bad.size == 0, f"{what}: {len(bad)} generated shares differ from the oracle's, first (clerk, participant, batch) {bad[:4].tolist()}"
            rest = tiles[i].copy()
            rest[:, :P, :case.B] = SENTINEL
            bad = np.argwhere(rest != SENTINEL)
            assert bad.size == 0, f"{what}: {len(bad)} elements written outside the tile, first (clerk, row, column) {bad[:4].tolist()}"
        diff = CL.first_difference(sums, want_sums)
        assert diff is None, f"run {run}: clerk sums: {diff}"
        if first_run is None:
            first_run = (tiles, sums, names, plans)
        else:
            assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(first_run[0], tiles)), f"run {run} generated other tiles than run 0"
            assert np.array_equal(first_run[1], sums) and first_run[2:] == (names, plans), f"run {run} differs from run 0"

"""The schedule of the dual-role launch, restated (shared by tests/test_dual_role_schedule_reach.py and
tests/test_dual_role_schedule_gpu.py - a helper module, not a conftest; nothing in it needs a device).

sda_share_generator_generate_combine_dev puts the share generation of tile i + 1 and the clerk sum of tile i into ONE grid.  The
host (fuse_plan, sda_kernels.hip) counts the share-gen chunks and the clerk-sum items, picks the distance between two clerk-sum
positions and the size of the grid; every workgroup then finds its own role (fuse_role / fuse_dispatch), a clerk workgroup its
(column block, job, row split) (fuse_combine) and a share-gen workgroup its (participant, chunk) (split_item).  None of this is
arithmetic: a slip there gives no fault and no error, only a row summed twice or a chunk never generated for SOME (participants,
previous rows, batches, clerks).  This module holds
  * plan: the host side in Python integers; role / item_of / chunk_of: the device side; schedule: every block index of a grid
    walked, with what ran how often and which (job, column pair, row) cells of the previous tile were summed; check: that
    against what the call has to do;
  * classes / coverage: the named regimes of the schedule space (CLASSES) a call reaches;
  * CASES: the calls both test modules run, each with the kernel instance it must name; PERIOD_CLASSES need two families each;
  * FAULTS: slips planted in the model only (plan(..., fault=name) and so on), each of which some case of the table must notice -
    so that the table cannot shrink to the shapes at which a slip does not matter;
  * REACH: what the table does not reach.
The model produces NO expected shares or sums: those come from the C oracle and from clerk_limits.want."""
from collections import Counter, namedtuple

import numpy as np

import clerk_limits as CL
import extremes as X

KTHREADS = 256
MFMA_FUSED_ITERS = 2                     # kMfmaFusedIters: 512 batches per share-gen chunk of the 62-bit limb GEMM
MAX_BLOCKS = 0xFFFFFFFF // KTHREADS      # kMaxBlocks: 16 777 215
FAMILIES = ("l31", "mfma", "n31", "additive")

# ---- planted faults (the model only) ------------------------------------------------------------------------------------------
F_EVEN = "the period is left even"
F_TWO_TO_ONE = "period 2 becomes 1"
F_NO_EXTENSION = "the grid is not extended"
F_NO_CLAMP = "the clamp on `before` is dropped"
F_NO_Q_TEST = "`rem == 0 && q < n_comb` loses its second half"
F_SPLITS_STALE = "`splits` is not recomputed after `rows_per_split`"
F_CAP_LATE = "the cap of 64 is not applied to `rows_per_split`"
F_NO_CLIP = "the last split is not clipped at `n_rows`"
F_COL_BLOCKS = "`col_blocks` is computed from `dimension` instead of ceil(dimension / 2)"
F_SWAP = "the job and split indices are swapped in `fuse_combine`"
F_CHUNK_MOD = "the chunk index is taken modulo the wrong operand"
FAULTS = (F_EVEN, F_TWO_TO_ONE, F_NO_EXTENSION, F_NO_CLAMP, F_NO_Q_TEST, F_SPLITS_STALE, F_CAP_LATE, F_NO_CLIP, F_COL_BLOCKS, F_SWAP,
          F_CHUNK_MOD)
# A fault that changes NOTHING, for any number of previous rows: with items of 512 rows and a cap of 64 the second ceil(prev /
# rows_per_split) always gives back the number of splits it started from (it could only drop below s splits for prev < s (s - 1),
# and s splits are only ever asked for above 512 (s - 1) rows).  tests/test_dual_role_schedule_reach.py proves that over every row
# count up to 2^17 instead of asking a case to notice it; should the constants change so that the line matters, that proof fails
# and a case is due.
EQUIVALENT = {F_SPLITS_STALE: "ceil(prev / rows_per_split) == splits for every prev: 512-row items, at most 64 of them"}

REACH = ("a grid beyond kMaxBlocks (16 777 215 workgroups: fuse_plan's refusal on size, which needs tens of GB of shares)",
         "more than 65 535 jobs (clerks)")

_ceil = CL._ceil

Plan = namedtuple("Plan", "chunks col_blocks splits rows_per_split n_gen n_comb raw_period period grid idle "
                          "jobs dimension prev_rows participants")


def gen_chunks(family, k, length):
    """share-gen chunks of one participant, as the four launchers count them"""
    assert family in FAMILIES
    batches = _ceil(length, k)
    if family == "mfma":
        return _ceil(batches, KTHREADS * MFMA_FUSED_ITERS)
    return _ceil(_ceil(batches, 2), KTHREADS)            # one lane = two adjacent batches (additive: k = 1, two elements)


def plan(family, k, n, length, participants, prev_rows, fault=None):
    """fuse_plan.  The first ten fields are (chunks, col_blocks, splits, rows_per_split, n_gen, n_comb, raw_period, period, grid,
    idle); the other four are the geometry the device side needs beside them"""
    assert fault is None or fault in FAULTS
    chunks = gen_chunks(family, k, length)
    dimension = _ceil(length, k)
    n_gen = chunks * (participants if length else 0)
    col_blocks = _ceil(dimension if fault == F_COL_BLOCKS else _ceil(dimension, 2), KTHREADS)
    have_comb = prev_rows > 0 and n > 0 and dimension > 0
    if not have_comb:
        splits, rps = 1, 1
    elif fault == F_SPLITS_STALE:
        splits = min(_ceil(prev_rows, 512), 64)
        rps = _ceil(prev_rows, splits)
    elif fault == F_CAP_LATE:
        rps = _ceil(prev_rows, _ceil(prev_rows, 512))
        splits = _ceil(prev_rows, rps)
    else:
        splits, rps = CL.fuse_split(prev_rows)
    n_comb = col_blocks * n * splits if have_comb else 0
    raw = n_gen // n_comb + 1 if n_comb else 1
    period = raw
    if n_comb and period % 2 == 0 and fault != F_EVEN:
        period = period - 1 if period > 2 else (1 if fault == F_TWO_TO_ONE else 3)
    grid = n_gen + n_comb
    if n_comb and fault != F_NO_EXTENSION:
        grid = max(grid, (n_comb - 1) * period + 1)
    return Plan(chunks, col_blocks, splits, rps, n_gen, n_comb, raw, period, grid, grid - n_gen - n_comb, n, dimension, prev_rows,
                participants)


def hook_fields(pl, fused=1):
    """what sda_debug_last_fuse_plan() reports for this plan"""
    return (fused, pl.n_gen, pl.n_comb, pl.period, pl.grid, pl.splits, pl.rows_per_split, pl.col_blocks)


# ---- the device side ------------------------------------------------------------------------------------------------------------
def roles(b, pl, fault=None):
    """fuse_role + fuse_dispatch for an int64 array of workgroup indices at once (the one restatement of the role map; the grids of
    the sweep in tests/test_dual_role_schedule_reach.py hold ten million positions): -> (clerk?, index, idle?), index = the clerk
    item where clerk, else the share-gen chunk (idle: a chunk index at or beyond n_gen)"""
    q, rem = np.divmod(b, pl.period)
    clerk = (rem == 0) & ((q < pl.n_comb) | (fault == F_NO_Q_TEST))
    before = q + (rem != 0)                                          # clerk-sum positions below b
    idx = np.where(clerk, q, b - (before if fault == F_NO_CLAMP else np.minimum(before, pl.n_comb)))
    return clerk, idx, ~clerk & (idx >= pl.n_gen)


def role(b, pl, fault=None):
    """the role of workgroup b: ("clerk", item), ("gen", chunk) or ("idle",)"""
    clerk, idx, idle = (x[0] for x in roles(np.array([b], dtype=np.int64), pl, fault))
    return ("clerk", int(idx)) if clerk else ("idle",) if idle else ("gen", int(idx))


def item_of(q, pl, fault=None):
    """fuse_combine: clerk-sum item -> (column block, job, split)"""
    bx, t = q % pl.col_blocks, q // pl.col_blocks
    return (bx, t // pl.jobs, t % pl.jobs) if fault == F_SWAP else (bx, t % pl.jobs, t // pl.jobs)


def chunk_of(item, pl, fault=None):
    """split_item: share-gen chunk -> (participant, chunk)"""
    p = item // pl.chunks
    return (p, item % pl.participants) if fault == F_CHUNK_MOD else (p, item - p * pl.chunks)


Schedule = namedtuple("Schedule", "items chunks summed outside idle")


def schedule(pl, fault=None, cells=True):
    """every block index of the grid: how often each clerk item (column block, job, split) and each share-gen chunk (participant,
    chunk) ran; `summed` [jobs][column pairs][previous rows] = how often each (job, column pair, row) cell was summed, `outside`
    what was summed beside them; the number of idle positions.  cells = False skips `summed`"""
    pairs = _ceil(pl.dimension, 2)
    clerk, idx, idle = roles(np.arange(pl.grid, dtype=np.int64), pl, fault)
    items, outside = Counter(), []
    chunks = Counter(chunk_of(c, pl, fault) for c in idx[~clerk & ~idle].tolist())
    summed = np.zeros((pl.jobs, pairs, pl.prev_rows), dtype=np.int32) if cells else None
    for q in idx[clerk].tolist():
        bx, job, z = item = item_of(q, pl, fault)
        items[item] += 1
        if not cells:
            continue
        p0, p1 = bx * KTHREADS, min((bx + 1) * KTHREADS, pairs)             # combine_pair: lanes with 2 pair >= dimension return
        r0 = z * pl.rows_per_split
        r1 = r0 + pl.rows_per_split
        if fault != F_NO_CLIP:
            r1 = min(r1, pl.prev_rows)
        if p0 >= p1 or r0 >= r1:
            continue
        if job >= pl.jobs or r1 > pl.prev_rows:
            outside.append(f"item {q}: job {job}, rows {r0} .. {r1 - 1}")
        if job < pl.jobs:
            summed[job, p0:p1, r0:min(r1, pl.prev_rows)] += 1
    return Schedule(items, chunks, summed, outside, int(idle.sum()))


def check(family, k, n, length, participants, prev_rows, fault=None, cells=True):
    """the schedule of this call (planned and run under `fault`) against what the call has to do - every clerk item and every
    share-gen chunk of the SOUND plan once, every cell of the previous tile summed once, nothing else.  -> list of findings"""
    good = plan(family, k, n, length, participants, prev_rows)
    pl = plan(family, k, n, length, participants, prev_rows, fault)
    s = schedule(pl, fault, cells)
    want_items = {(bx, j, z) for bx in range(good.col_blocks) for j in range(n) for z in range(good.splits)} if good.n_comb else set()
    want_chunks = {(p, c) for p in range(participants) for c in range(good.chunks)} if good.n_gen else set()
    bad = []
    for what, got, want in (("clerk item", s.items, want_items), ("share-gen chunk", s.chunks, want_chunks)):
        wrong = sorted(x for x in set(got) | want if got.get(x, 0) != (1 if x in want else 0))
        if wrong:
            bad.append(f"{what} {wrong[0]} ran {got.get(wrong[0], 0)} times, not {1 if wrong[0] in want else 0} ({len(wrong)} such)")
    if s.outside:
        bad.append(f"summed outside the previous tile: {s.outside[0]} ({len(s.outside)} such)")
    if cells and good.n_comb and not (s.summed == 1).all():
        j, c, r = (int(x) for x in np.argwhere(s.summed != 1)[0])
        bad.append(f"job {j}, column pair {c}, row {r} summed {int(s.summed[j, c, r])} times ({int((s.summed != 1).sum())} such)")
    if s.idle != good.grid - good.n_gen - good.n_comb:
        bad.append(f"{s.idle} idle positions, not {good.grid - good.n_gen - good.n_comb}")
    return bad


# ---- the named classes ------------------------------------------------------------------------------------------------------------
P1, P23_IDLE, P23_FULL, P3, P43, P5, P65, P7 = ("period 1", "period 2 -> 3, idle surplus", "period 2 -> 3, no surplus", "period 3",
                                                 "period 4 -> 3", "period 5", "period 6 -> 5", "period >= 7")
CLAMP, FIRST, DRAIN = "clerk items used up before the grid ends", "first call (no clerk items)", "drain call (no share-gen chunks)"
PERIOD_CLASSES = (P1, P23_IDLE, P23_FULL, P3, P43, P5, P65, P7, CLAMP, FIRST, DRAIN)
SPLIT_CLASSES = ("one split (read-modify-write)", "two splits, uneven", "three splits", "64-split cap, rows_per_split > 512")
GEOMETRY_CLASSES = ("several column blocks, ragged last", "odd B", "dimension 1", "several share-gen chunks, ragged last",
                    "prev rows < participants", "prev rows > participants")
BOUNDARY_CLASSES = tuple(f"n_gen = {r} n_comb {what}" for r in (1, 2, 3) for what in ("exactly", "- 1"))
FALLBACK_CLASSES = ("fallback: odd row stride", "fallback: d_prev off by 8 bytes", "fallback: odd secrets stride")
CLASSES = PERIOD_CLASSES + SPLIT_CLASSES + GEOMETRY_CLASSES + BOUNDARY_CLASSES + FALLBACK_CLASSES


def classes(family, k, n, length, participants, prev_rows):
    """the classes one call reaches (the fallback classes belong to a case's layout: coverage)"""
    pl = plan(family, k, n, length, participants, prev_rows)
    out = set()
    if pl.n_gen and not pl.n_comb:
        out.add(FIRST)
    if pl.n_comb and not pl.n_gen:
        out.add(DRAIN)
    if pl.n_gen and pl.n_comb:
        out.add({1: P1, 2: P23_IDLE if pl.idle else P23_FULL, 3: P3, 4: P43, 5: P5, 6: P65}.get(pl.raw_period, P7))
        assert (pl.idle > 0) == (pl.raw_period == 2 and pl.n_gen < 2 * pl.n_comb - 2)     # surplus positions exist in no other regime
        if pl.grid >= pl.n_comb * pl.period + 2:             # some position has more clerk positions below it than there are items
            out.add(CLAMP)
        for r in (1, 2, 3):
            if pl.n_gen == r * pl.n_comb:
                out.add(f"n_gen = {r} n_comb exactly")
            if pl.n_gen == r * pl.n_comb - 1:
                out.add(f"n_gen = {r} n_comb - 1")
        out.add("prev rows < participants" if prev_rows < participants else "prev rows > participants" if prev_rows > participants else None)
        out.discard(None)
    if pl.n_comb:
        if pl.splits == 1:
            out.add(SPLIT_CLASSES[0])
        if pl.splits == 2 and prev_rows != 2 * pl.rows_per_split:
            out.add(SPLIT_CLASSES[1])
        if pl.splits == 3:
            out.add(SPLIT_CLASSES[2])
        if pl.splits == 64 and pl.rows_per_split > 512:
            out.add(SPLIT_CLASSES[3])
        if pl.col_blocks > 1 and _ceil(pl.dimension, 2) % KTHREADS:
            out.add(GEOMETRY_CLASSES[0])
        if pl.dimension == 1:
            out.add(GEOMETRY_CLASSES[2])
        elif pl.dimension % 2:
            out.add(GEOMETRY_CLASSES[1])
    if pl.n_gen and pl.chunks > 1:
        lanes = pl.dimension if family == "mfma" else _ceil(pl.dimension, 2)
        if lanes % (KTHREADS * MFMA_FUSED_ITERS if family == "mfma" else KTHREADS):
            out.add(GEOMETRY_CLASSES[3])
    return out


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# kind "pipeline": tiles of `tiles[i]` participants generated one after the other, each summed by the call that generates the next -
# the first call has nothing to sum, the drain call nothing to generate; kind "crafted prev": calls of (participants, previous rows)
# whose d_prev is clerk_limits.crafted_jobs (any int64: a row summed twice or skipped changes the sum whatever its value).
# layout: None, or the fallback class the case's buffers are laid out for (the launch is then refused: two launches).
Case = namedtuple("Case", "name family kernel k t n p rounds kind B Bs steps layout", defaults=(None,))
P62, PMAX, P31MAX, P29_BELOW = CL.P62, CL.PMAX, CL.P31MAX, X.P29_BELOW
L31_3_1, L31_8_2, L31_RT = "fused_packed_l31_kernel<3, 1, 20>", "fused_packed_l31_kernel<8, 2, 20>", "fused_packed_l31_rt_kernel<8, 20>"
MFMA_12_3, MFMA_RT = "fused_packed_mfma_kernel<12, 3, 20>", "fused_packed_mfma_kernel<0, 0, 20>"
N31_8_4, N31_16_16 = "fused_packed_n31_kernel<8, 4, 20>", "fused_packed_n31_kernel<16, 16, 20>"
ADDITIVE = "fused_additive_kernel<20>"

CASES = (
    # B = 520: two share-gen chunks (the second ragged) beside two column blocks (the second ragged), 16 clerk items: the
    # participant counts walk every period class; 7 after 8 is a short tile, 8 after 7 the tile after it
    Case("l31 (3, 1, 8): every period class", "l31", L31_3_1, 3, 1, 8, PMAX, 20, "pipeline", 520, 528, (8, 7, 8, 15, 16, 24, 48, 40, 32)),
    # the same walk in a second family: len = 520, 6 clerk items
    Case("additive n = 3: every period class", "additive", ADDITIVE, 1, 2, 3, P62, 20, "pipeline", 520, 528, (3, 2, 3, 5, 6, 9, 18, 15, 12)),
    Case("l31 (8, 2, 26): 130 participants beside 52 items", "l31", L31_8_2, 8, 2, 26, PMAX, 20, "pipeline", 520, 528, (26, 130)),
    # one chunk, one column block, 8 items: n_gen = r n_comb - 1 and r n_comb for r = 1, 2, 3
    Case("l31 run-time (4, 3, 8): the boundaries", "l31", L31_RT, 4, 3, 8, PMAX, 20, "pipeline", 300, 304, (8, 7, 15, 23, 16, 24, 8)),
    Case("mfma (12, 3, 26): two 512-batch chunks", "mfma", MFMA_12_3, 12, 3, 26, P62, 20, "pipeline", 520, 528, (3, 40, 3)),
    Case("mfma run-time (9, 6, 26)", "mfma", MFMA_RT, 9, 6, 26, PMAX, 20, "pipeline", 40, 48, (5, 60, 100)),
    Case("n31 (3, 4, 8) at 2^31 - 1: odd B", "n31", N31_8_4, 3, 4, 8, P31MAX, 20, "pipeline", 521, 528, (8, 24, 40, 9)),
    Case("n31 (8, 7, 26) below 2^29", "n31", N31_16_16, 8, 7, 26, P29_BELOW, 20, "pipeline", 40, 48, (4, 130, 30)),
    Case("additive n = 2: dimension 1", "additive", ADDITIVE, 1, 1, 2, P62, 20, "pipeline", 1, 2, (3, 1, 4, 9)),
    Case("l31 (3, 1, 8), ChaCha12", "l31", "fused_packed_l31_kernel<3, 1, 12>", 3, 1, 8, PMAX, 12, "pipeline", 300, 304, (3, 20, 5)),
    # the split classes, on crafted rows: 513 rows = 257 + 256, 1025 = 342 + 342 + 341 beside two column blocks, a drain call with
    # two splits, 32 769 rows = 63 x 513 + 450
    Case("l31 (3, 1, 8): 513 crafted rows", "l31", L31_3_1, 3, 1, 8, PMAX, 20, "crafted prev", 300, 304, ((2, 513), (20, 9))),
    Case("additive n = 3: 1025 crafted rows", "additive", ADDITIVE, 1, 2, 3, P62, 20, "crafted prev", 520, 528, ((2, 1025), (0, 513), (3, 40))),
    Case("additive n = 3: 32 769 crafted rows", "additive", ADDITIVE, 1, 2, 3, P62, 20, "crafted prev", 2, 4, ((2, 32769), (1, 5))),
    Case("n31 (3, 4, 8): 1025 crafted rows, odd B", "n31", N31_8_4, 3, 4, 8, P31MAX, 20, "crafted prev", 41, 48, ((30, 1025), (0, 40))),
    # layouts the 16-byte accesses do not admit: fuse_plan refuses, the call takes two launches
    Case("l31 (3, 1, 8): odd row stride", "l31", L31_3_1, 3, 1, 8, PMAX, 20, "crafted prev", 41, 43, ((2, 9), (0, 9)), "fallback: odd row stride"),
    Case("additive n = 3: d_prev off by 8 bytes", "additive", ADDITIVE, 1, 2, 3, P62, 20, "crafted prev", 41, 48, ((2, 9), (0, 9)), "fallback: d_prev off by 8 bytes"),
    Case("mfma (12, 3, 26): odd secrets stride", "mfma", MFMA_12_3, 12, 3, 26, P62, 20, "crafted prev", 41, 48, ((2, 9),), "fallback: odd secrets stride"),
)


def length_of(case):
    """secrets per participant: a ragged last batch (zero padding) wherever k > 1"""
    return case.B * case.k - (1 if case.k > 1 else 0)


def calls_of(case):
    """[(participants, previous rows)] of the case's generate_combine_dev calls, in order"""
    if case.kind == "crafted prev":
        return list(case.steps)
    t = list(case.steps)
    return list(zip(t + [0], [0] + t))


def plans_of(case, fault=None):
    return [plan(case.family, case.k, case.n, length_of(case), P, prev, fault) for P, prev in calls_of(case)]


def coverage(case):
    """the classes the case's calls reach, by name (a refused layout runs no dual-role grid: it reaches its fallback class alone)"""
    if case.layout is not None:
        return {case.layout}
    out = set()
    for P, prev in calls_of(case):
        out |= classes(case.family, case.k, case.n, length_of(case), P, prev)
    return out


def findings(case, fault=None):
    """check() over the case's calls: [] or what the first call that goes wrong shows"""
    for i, (P, prev) in enumerate(calls_of(case)):
        bad = check(case.family, case.k, case.n, length_of(case), P, prev, fault)
        if bad:
            return [f"call {i} ({P} participants, {prev} previous rows): {b}" for b in bad]
    return []

"""The rejection repair of the rand-0.3 ChaCha mask expansion (chacha_expand in sda_amd/csrc/sda_capi.cpp and the chacha_mask_*
kernels of sda_kernels.hip) on LOCATED seeds: the cases, a Python-integer model of the whole driver, and the seeds that were found
for every branch of it.  test_chacha_repair_reach.py proves on the CPU what the cases reach; test_chacha_repair_gpu.py runs them
through every entry point against the oracle.

  * model(): the driver step by step - the fast pass with its RejectRecords, the plan, chacha_shift_body lane by lane, the
    exact-order walk in chunks of 2048 candidates, and the launch geometry (splits, list strides, participant slices).  It names
    every branch it takes (BRANCHES) and predicts what sda_debug_last_mask_plan() reports.  It is NOT the reference: that is the
    sequential gen_range of oracle.pyoracle.ChaChaRng and coracle.chacha_expand / chacha_combine.  The model exists to say which
    code a seed runs, and - with a fault planted (FAULTS) - to show that a case would notice that code being wrong.
  * SEEDS: 4-word seeds found once by locate() (run by hand: `python tests/chacha_repair.py`, under a minute; no test runs it),
    each pinned beside its (q, dimension) and the branches it is there for.
  * CASES: what the GPU runs.  A long list repeats one located seed: the expected sum is n * mask mod q, one oracle run per seed.
  * REACH: the branches no case takes, and why.
"""
import functools

import numpy as np

import mask_combiner_cases as mc

P62 = mc.P62                               # 4611686006577364993: zone = 2^64 - 1 - 15, in effect never rejects
Q8 = (1 << 61) + 1                         # rejects just under 1/8: the shift route up to dimension 8
Q64 = (1 << 62) - (1 << 56)                # 2^-6: up to 64
Q2048 = (1 << 62) - (1 << 51)              # 2^-11: up to 2048
Q5 = (1 << 64) // 5 + 1                    # just under 1/5: up to 5 (not a prime; the expansion does not care)
THRESHOLDS = [(Q8, 8, 9), (Q64, 64, 65), (Q2048, 2048, 2049), (Q5, 5, 6)]      # (q, last shift-route dimension, first all-exact one)

K_THREADS = 256                            # sda_kernels.hip kThreads
CHUNK = 8 * K_THREADS                      # candidates per step of the exact-order walk
NONE = 0xFFFFFFFF

BRANCHES = [
    # plan
    "all_exact", "clean", "shift_R1", "shift_R2", "shift_R3", "exact_R4", "exact_many",
    # fast pass
    "fast_fourth_not_stored", "fast_reject_past_dimension_not_recorded",
    # shift body, lanes
    "shift_lane_before_first", "shift_skip_in_lane", "src_o0", "src_o1_d8", "src_o1_d9", "src_o1_d10", "fixpoint_2", "fixpoint_3",
    "adjacent_across_block_edge", "reject_at_0", "reject_at_last",
    # shift body, tail
    "tail_need_1", "tail_need_2", "tail_need_3", "tail_o0", "tail_o1", "tail_cached", "tail_cached_second_block", "tail_meets_reject",
    "tail_by_earlier_lane", "delta_neg", "delta_nonneg", "apply_shift_overwrite",
    # exact-order walk
    "slow_chunk_exact_fit", "slow_next_chunk_one_mask", "slow_three_chunks", "slow_cut_inside_lane", "slow_naive_subtract",
    "slow_no_subtract", "slow_apply_overwrite",
    # launch forms
    "shift_list_strides", "exact_list_strides_counted", "all_exact_strides_counted", "fast_split_last_short", "fast_split_past_count", "apply_second_slice",
    "dimension_ge_0xFFFFFFF0", "uncounted_list_past_grid_limit",
]
REACH = {
    "tail_cached_second_block": "the tail walk recomputing a second block needs 16 or more rejected candidates in a row after "
                                "`dimension` behind a seed with at most 3 before it: about 1e-10 per seed at Q8, less elsewhere",
    "dimension_ge_0xFFFFFFF0": "a RejectRecord position is 32 bits wide, so such a dimension walks in exact order: 32 GiB per row",
    "uncounted_list_past_grid_limit": "a list whose length the host knows gets one workgroup per entry up to 0xFFFFFFFF / 256 "
                                      "workgroups; only the all-exact route has such a list, and 2^24 keys in one chunk",
}
FAULTS = {                                 # planted fault -> the branches whose cases must notice it
    "two_fixpoint_iterations": {"fixpoint_3"},
    "unsorted_record": {"shift_R2", "shift_R3"},
    "past_dimension_rejection_counted": {"fast_reject_past_dimension_not_recorded"},
    "need_off_by_one": {"tail_need_1", "tail_need_2", "tail_need_3"},
    "tail_ignores_zone": {"tail_meets_reject"},
    "d8_from_o0": {"src_o1_d8", "src_o1_d9", "src_o1_d10"},
    "chunk_loop_one_early": {"slow_next_chunk_one_mask", "slow_three_chunks", "slow_chunk_exact_fit"},
    "fourth_to_shift": {"exact_R4"},
    "stride_stops_at_grid": {"shift_list_strides", "exact_list_strides_counted", "all_exact_strides_counted"},
    "apply_reads_out": {"apply_shift_overwrite", "slow_apply_overwrite"},
}
# One more chunk than needed (the loop ending late) cannot change a result: past `dimension` the walk neither adds nor takes back.
# The reach test asserts exactly that - the model with this fault equals the oracle on every case - instead of a difference.
BENIGN_FAULTS = {"chunk_loop_one_late"}


class Stream:
    """the next_u64 values of rand-0.3 ChaChaRng::from_seed(seed) as Python integers, computed as far as they are asked for"""

    def __init__(self, seed):
        self.seed, self.v = tuple(int(w) for w in seed), []

    def __getitem__(self, idx):
        if idx >= len(self.v):
            blocks = K_THREADS * (idx // CHUNK + 1)
            self.v = [int(x) for x in mc.candidates(np.array([self.seed], dtype=np.int64), blocks)[0]]
        return self.v[idx]


@functools.lru_cache(maxsize=None)
def stream(seed):
    return Stream(seed)


def canon(x, q):
    return x % q                           # canon_i64: the non-negative residue of any int64


def _fast_pass(st, q, dim, z, faults, br, sink):
    """chacha_fast_body / chacha_mask_apply_kernel for one key: candidate i goes to position i; -> the key's RejectRecord"""
    count, pos = 0, []
    for j in range((dim + 7) // 8):
        for m in range(8):
            i = 8 * j + m
            v = st[i]
            if v >= z and (i < dim or "past_dimension_rejection_counted" in faults):
                if count < 3:
                    pos.append(i)
                else:
                    br("fast_fourth_not_stored")
                count += 1
            elif v >= z:
                br("fast_reject_past_dimension_not_recorded")
            if i < dim:
                sink.fast(i, v)
    return count, pos[::-1]                # the atomics give the slots in any order: the model stores them backwards


def _shift_body(st, R, pos, dim, z, faults, br, sink):
    x = [pos[0], pos[1] if R > 1 else NONE, pos[2] if R > 2 else NONE]
    if "unsorted_record" not in faults:
        if x[0] > x[1]: x[0], x[1] = x[1], x[0]
        if x[1] > x[2]: x[1], x[2] = x[2], x[1]
        if x[0] > x[1]: x[0], x[1] = x[1], x[0]
    x0, x1, x2 = x
    real = [p for p in x if p != NONE]
    if x0 == 0: br("reject_at_0")
    if dim - 1 in real: br("reject_at_last")
    if any(a % 8 == 7 and a + 1 in real for a in real): br("adjacent_across_block_edge")
    for j in range((dim + 7) // 8):
        i0 = 8 * j
        if i0 + 7 < x0:
            br("shift_lane_before_first")
            continue
        cached = None
        for m in range(8):
            i = i0 + m
            if i >= dim:
                break
            if i < x0:
                br("shift_skip_in_lane")
                continue
            f = i
            for it in range(2 if "two_fixpoint_iterations" in faults else 3):
                g = i + (x0 <= f) + (x1 <= f) + (x2 <= f)
                if it and g != f: br("fixpoint_%d" % (it + 1))
                f = g
            if f < dim:
                d = f - i0
                if d < 8:
                    br("src_o0")
                    nv = st[i0 + d]
                else:
                    br("src_o1_d%d" % d)
                    nv = st[i0 + d - 8] if "d8_from_o0" in faults else st[i0 + 8 + (d - 8)]
            else:
                need = i - (dim - R) + (2 if "need_off_by_one" in faults else 1)
                br("tail_need_%d" % need)
                if j != (dim - 1) >> 3: br("tail_by_earlier_lane")
                idx = dim
                while True:
                    b = idx >> 3
                    if b == j: br("tail_o0")
                    elif b == j + 1: br("tail_o1")
                    else:
                        if b != cached:
                            br("tail_cached" if cached is None else "tail_cached_second_block")
                            cached = b
                    v = st[idx]
                    if v >= z: br("tail_meets_reject")
                    if v < z or "tail_ignores_zone" in faults:
                        need -= 1
                        if need == 0:
                            nv = v
                            break
                    idx += 1
            sink.shift(i, nv, st[i], br)


def _slow_walk(st, q, dim, z, subtract, faults, br, sink):
    accepted_base = block_base = chunks = 0
    late = 1 if "chunk_loop_one_late" in faults else 0
    while accepted_base < dim or late:
        if accepted_base >= dim: late = 0
        ok = [st[8 * block_base + c] < z for c in range(CHUNK)]
        chunk_total = sum(ok)
        if "chunk_loop_one_early" in faults and accepted_base + chunk_total >= dim:
            break
        chunks += 1
        pos = accepted_base
        for t in range(K_THREADS):
            inside = outside = False
            for m in range(8):
                ci = 8 * (block_base + t) + m
                r = st[ci] % q
                if subtract and ci < dim and r != 0:
                    sink.take_back(ci, r)
                if ok[8 * t + m]:
                    if pos < dim:
                        sink.slow(pos, r)
                        inside = True
                    else:
                        outside = True
                    pos += 1
            if inside and outside: br("slow_cut_inside_lane")
        accepted_base += chunk_total
        block_base += K_THREADS
        if accepted_base == dim: br("slow_chunk_exact_fit")
        if accepted_base == dim - 1: br("slow_next_chunk_one_mask")
        if chunks >= 3: br("slow_three_chunks")


class SumSink:
    """the 128-bit column accumulators: exact integers (lo + 2^64 hi of every atomic add is the signed value added)"""

    def __init__(self, dim, q):
        self.acc, self.q = [0] * dim, q

    def fast(self, i, v): self.acc[i] += v

    def shift(self, i, nv, ov, br):
        br("delta_neg" if nv < ov else "delta_nonneg")
        lo, hi = (nv - ov) % (1 << 64), -1 if nv < ov else 0
        self.acc[i] += lo + (hi << 64)

    def take_back(self, ci, r): self.acc[ci] += ((0 - r) % (1 << 64)) + (-1 << 64)

    def slow(self, pos, r): self.acc[pos] += r

    subtracts = True


class ApplySink:
    """MaskApply: out[i] = (canon(secrets[i]) + candidate mod q) mod q, every write reading `secrets` again (mask_apply_put);
    aliased = the caller gave d_masked == d_secrets"""

    def __init__(self, secrets, q, faults, br, aliased=False):
        self.q, self.out, self.br = q, [None] * len(secrets), br
        self.src = self.out if aliased or "apply_reads_out" in faults else list(secrets)
        if aliased or "apply_reads_out" in faults:
            self.out[:] = list(secrets)

    def put(self, i, cand): self.out[i] = (canon(self.src[i], self.q) + cand % self.q) % self.q

    def fast(self, i, v): self.put(i, v)

    def shift(self, i, nv, ov, br):
        br("apply_shift_overwrite")
        self.put(i, nv)

    def take_back(self, ci, r): pass

    def slow(self, pos, r): self.put(pos, r)

    subtracts = False


def model_key(seed, q, dim, sink, faults=frozenset(), br=lambda name: None):
    """one key through the driver -> 'all_exact' | 'clean' | 'shift' | 'exact': where the plan sent it"""
    st, z = stream(tuple(seed)), mc.zone(q)
    if mc.all_exact_order(q, dim):
        br("all_exact")
        br("slow_no_subtract")
        _slow_walk(st, q, dim, z, False, faults, br, sink)
        return "all_exact"
    count, pos = _fast_pass(st, q, dim, z, faults, br, sink)
    if count == 0:
        br("clean")
        return "clean"
    if count <= (4 if "fourth_to_shift" in faults else 3):
        br("shift_R%d" % min(count, 3))
        _shift_body(st, count, pos, dim, z, faults, br, sink)
        return "shift"
    br("exact_R4" if count == 4 else "exact_many")
    br("slow_naive_subtract" if sink.subtracts else "slow_apply_overwrite")
    _slow_walk(st, q, dim, z, True, faults, br, sink)
    return "exact"


def secrets_row(dim, q, salt=0):
    """a participant's secrets: any int64, with non-canonical values of every kind at the front, where the repairs of the short cases are"""
    special = [-1, q, -q, q + 5, -(1 << 63), (1 << 63) - 1, 0, q - 1, -(1 << 62), 3 * q // 2]
    row = [int(x) for x in np.random.default_rng(1000 + salt).integers(-(1 << 63), (1 << 63) - 1, size=dim, dtype=np.int64)]
    for i in range(dim):
        if (i + salt) % 3 != 2:
            row[i] = special[(i + salt) % len(special)]
    return row


def model(case, entry, faults=frozenset(), aliased=False):
    """the whole driver for one call of `entry` ('sum': combine / mask / update_dev; 'counted': update_sealed_rows_dev with
    case['refused'] rows failing; 'apply': mask_batch_dev) -> dict(result, plan, branches).  result: 'sum' / 'counted' the column
    sums mod q; 'apply' {seed: masked row of secrets_row(dim, q, index of the seed among the distinct ones)}"""
    q, dim, faults = case["q"], case["dim"], frozenset(faults)
    branches = set()
    br = branches.add
    rows = sum(n for _, n in case["keys"])
    refused = case.get("refused", 0) if entry == "counted" else 0      # the first `refused` sealed rows fail
    keys, left = [], refused                               # refused rows give no key: taken off the front group(s) here
    for seed, n in case["keys"]:
        take = min(left, n)
        left -= take
        if n - take: keys.append((seed, n - take))
    n_keys = rows - refused
    ns = rows                                              # the host's upper bound: sizes every grid
    pos_blocks = -(-((dim + 7) // 8) // K_THREADS)
    all_exact = mc.all_exact_order(q, dim)
    # ---- launch geometry of the fast pass
    if not all_exact and entry != "apply":
        split = min(max(1, -(-2048 // pos_blocks)) if pos_blocks < 2048 else 1, ns, 65535)
        per = -(-ns // split)
        split = -(-ns // per)
        covered = 0
        for y in range(split):
            begin, end = y * per, min((y + 1) * per, n_keys)
            if (y + 1) * per > ns: br("fast_split_last_short")
            if begin >= n_keys: br("fast_split_past_count")
            covered += max(0, end - begin)
        assert covered == n_keys
    if not all_exact and entry == "apply":
        per = min(0xFFFFFFFF // (pos_blocks * K_THREADS), 65535)
    # ---- every distinct key once
    total = [0] * dim
    applied = {}
    shift_len = exact_len = 0
    k0 = 0
    distinct = {}
    for seed, n in keys:
        distinct.setdefault(seed, len(distinct))
        if entry == "apply":
            sink = ApplySink(secrets_row(dim, q, distinct[seed]), q, faults, br, aliased)
        else:
            sink = SumSink(dim, q)
        if all_exact:
            grid = min(ns, 2048 if entry == "counted" else 0xFFFFFFFF // K_THREADS)
            if entry == "counted" and k0 + n > grid: br("all_exact_strides_counted")
            done = n if "stride_stops_at_grid" not in faults else max(0, min(k0 + n, grid) - k0)
            route = model_key(seed, q, dim, sink, faults, br)
            part = sink.acc if entry != "apply" else None
        else:
            fast = SumSink(dim, q) if entry != "apply" else sink
            route = model_key(seed, q, dim, fast, faults, br)
            # the repair of a listed key is launched apart from its fast pass: a list walked only as far as the grid loses repairs
            if route == "shift":
                gy = min(max(16, 4096 // pos_blocks), ns, 65535)
                if shift_len + n > gy: br("shift_list_strides")
                done = n if "stride_stops_at_grid" not in faults else max(0, min(shift_len + n, gy) - shift_len)
                shift_len += n
            elif route == "exact":
                grid = min(ns, 2048)
                if exact_len + n > grid: br("exact_list_strides_counted")
                done = n if "stride_stops_at_grid" not in faults else max(0, min(exact_len + n, grid) - exact_len)
                exact_len += n
            else:
                done = n
            if entry == "apply" and route != "clean" and k0 + n > per: br("apply_second_slice")
            part = fast.acc if entry != "apply" else None
        if entry == "apply":
            if done < n:                                   # some rows keep what the fast pass alone wrote
                sink = ApplySink(secrets_row(dim, q, distinct[seed]), q, faults, br, aliased)
                _fast_pass(stream(seed), q, dim, mc.zone(q), faults, lambda name: None, sink)
            applied[seed] = sink.out
        else:
            if done < n:
                only_fast = SumSink(dim, q)
                if not all_exact:
                    _fast_pass(stream(seed), q, dim, mc.zone(q), faults, lambda name: None, only_fast)
                for i in range(dim): total[i] += (n - done) * only_fast.acc[i]
            for i in range(dim): total[i] += done * part[i]
        k0 += n
    plan = (1, 0, 0, n_keys) if all_exact else (0, shift_len, exact_len, n_keys)
    result = applied if entry == "apply" else [t % q for t in total]
    return {"result": result, "plan": plan, "branches": branches}


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_mask(seed, q, dim):
    """the `dim` masks of a seed, rand-0.3 gen_range(0, q) in sequence (C oracle) -> tuple of Python integers"""
    from oracle import coracle
    return tuple(int(x) for x in coracle.chacha_expand([int(w) for w in seed], q, dim))


def oracle_sum(case, entry="sum"):
    q, dim = case["q"], case["dim"]
    left = case.get("refused", 0) if entry == "counted" else 0
    total = [0] * dim
    for seed, n in case["keys"]:
        take = min(left, n)
        left -= take
        m = oracle_mask(seed, q, dim)
        for i in range(dim): total[i] += (n - take) * m[i]
    return [t % q for t in total]


def oracle_applied(seed, q, dim, secrets):
    return [(canon(s, q) + m) % q for s, m in zip(secrets, oracle_mask(seed, q, dim))]


# ---- located seeds ------------------------------------------------------------------------------------------------------------------
# name: (seed words, q, dimension, the branches it is pinned for).  Found by locate(); test_chacha_repair_reach.py asserts every pin.
SEEDS = {
    "clean8": ((2139946102, 2083879367, 502244941, 4212234199), Q8, 8, ["clean"]),
    "r1_first_last_lane": ((4082534881, 3551187749, 1994664286, 3803280585), Q64, 20,
                           ["shift_R1", "shift_lane_before_first", "shift_skip_in_lane", "src_o0", "tail_need_1", "tail_o0"]),
    "r2_at_0": ((3717673525, 3236314158, 3598687396, 2311307930), Q8, 8,
                ["delta_neg", "delta_nonneg", "reject_at_0", "shift_R2", "tail_need_2", "tail_o1", "apply_shift_overwrite"]),
    "r3_adjacent": ((3117609497, 689995123, 1385451522, 4165797929), Q8, 8, ["fixpoint_2", "fixpoint_3", "shift_R3", "tail_need_3"]),
    "r2_adjacent_last": ((1233503577, 2276077602, 4192094545, 1910677217), Q8, 8, ["fixpoint_2", "reject_at_last", "shift_R2"]),
    "tail_meets": ((3217372416, 4130286196, 395584478, 3112949092), Q8, 8, ["tail_meets_reject", "tail_o1"]),
    "tail_oc": ((1207904409, 183858877, 1266126810, 4060043862), Q8, 8, ["tail_cached", "tail_meets_reject"]),
    "r4": ((2409223080, 331072436, 381405007, 2097873456), Q8, 8,
           ["exact_R4", "fast_fourth_not_stored", "slow_naive_subtract", "slow_apply_overwrite"]),
    "r6": ((3337470238, 266485196, 1692230341, 3083352953), Q8, 8, ["exact_many"]),
    "past_dim5": ((4015584280, 4155105776, 3727568734, 2933741072), Q8, 5,
                  ["fast_reject_past_dimension_not_recorded", "shift_R1", "tail_meets_reject", "tail_o0"]),
    "q5_r4": ((3522076660, 3222928831, 236187477, 2467314821), Q5, 5, ["exact_R4"]),
    "q5_r3": ((1632823342, 1682015850, 170858916, 804243663), Q5, 5, ["shift_R3", "tail_need_3"]),
    "q5_dim3": ((1632823342, 1682015850, 170858916, 804243663), Q5, 3,
                ["fast_reject_past_dimension_not_recorded", "reject_at_last", "shift_R2"]),
    "edge_7_8": ((3055336774, 4181728089, 2382850683, 163196789), Q64, 20,
                 ["adjacent_across_block_edge", "fixpoint_2", "src_o1_d8", "src_o1_d9"]),
    "d10": ((2335301127, 697661756, 763484018, 465273129), Q64, 20, ["shift_R3", "src_o1_d10", "src_o1_d8", "src_o1_d9"]),
    "earlier_lane": ((2335301127, 697661756, 763484018, 465273129), Q64, 10, ["shift_R3", "tail_by_earlier_lane", "tail_o0", "tail_o1"]),
    "q64_dim64": ((2903300497, 3743644996, 943408660, 2336210527), Q64, 64, ["shift_R2", "tail_o1"]),
    "q64_r5": ((3383353497, 209344708, 3542072091, 3891789711), Q64, 64, ["exact_many", "slow_cut_inside_lane"]),
    # 4 of this seed's first 2048 candidates are rejected at Q2048, all four below 2044: the first chunk emits exactly 2044 masks
    "chunk_fit": ((2881021352, 3457461230, 97294837, 3470079269), Q2048, CHUNK - 4, ["slow_chunk_exact_fit", "slow_naive_subtract", "exact_R4"]),
    "chunk_fit_plus_1": ((2881021352, 3457461230, 97294837, 3470079269), Q2048, CHUNK - 4 + 1, ["slow_next_chunk_one_mask", "slow_naive_subtract"]),
    "q2048_r2": ((763308099, 3855495969, 3426047449, 3625944696), Q2048, 2048, ["shift_R2"]),
}


def _case(name, q, dim, keys, pins, refused=0, entries=("sum", "counted", "apply")):
    return {"name": name, "q": q, "dim": dim, "keys": [(SEEDS[k][0] if isinstance(k, str) else k, n) for k, n in keys], "pins": set(pins),
            "refused": refused, "entries": entries}


# every located seed alone at its own (q, dimension) ...
CASES = [_case(name, q, dim, [(name, 1)], pins) for name, (seed, q, dim, pins) in SEEDS.items()]
# ... both sides of every threshold of chacha_exact_order_for_all, with rows refused under either plan ...
CASES += [
    _case("thr_q8_8", Q8, 8, [("clean8", 2), ("r2_at_0", 2)], ["shift_R2", "clean", "fast_split_past_count"], refused=2),
    _case("thr_q8_9", Q8, 9, [("clean8", 2), ("r2_at_0", 2)], ["all_exact", "slow_no_subtract", "slow_cut_inside_lane"], refused=1),
    _case("thr_q64_64", Q64, 64, [("q64_dim64", 1)], ["shift_R2"]),
    _case("thr_q64_65", Q64, 65, [("q64_dim64", 1)], ["all_exact"]),
    _case("thr_q2048_2048", Q2048, 2048, [("q2048_r2", 1)], ["shift_R2"]),
    _case("thr_q2048_2049", Q2048, 2049, [("q2048_r2", 1)], ["all_exact"]),
    _case("thr_q5_5", Q5, 5, [("q5_r3", 1)], ["shift_R3"]),
    _case("thr_q5_6", Q5, 6, [("q5_r3", 1)], ["all_exact"]),
    # ... the chunk edges of the walk on the all-exact route: 258 of clean8's first 2048 candidates are rejected at Q8
    _case("all_exact_chunk_fit", Q8, CHUNK - 258, [("clean8", 1)], ["all_exact", "slow_chunk_exact_fit", "slow_no_subtract"]),
    _case("all_exact_chunk_fit_plus_1", Q8, CHUNK - 258 + 1, [("clean8", 1)], ["all_exact", "slow_next_chunk_one_mask"]),
    _case("three_chunks", Q2048, 4100, [("chunk_fit", 1), ("q2048_r2", 1)], ["all_exact", "slow_three_chunks", "slow_no_subtract"]),
    _case("never_rejects", P62, 2049, [("clean8", 1), ("r4", 2)], ["clean"]),
    # ... both lists in one plan ...
    _case("both_lists", Q8, 8, [("clean8", 3), ("r2_at_0", 2), ("r4", 1), ("tail_oc", 1), ("r6", 2), ("r3_adjacent", 1)],
          ["clean", "shift_R2", "shift_R3", "exact_R4", "exact_many", "tail_cached"], refused=1),
    # ... and the launch forms: lists longer than their grids, a short last split, a participant slice of its own
    _case("shift_list_5000", Q8, 8, [("r2_at_0", 5000)], ["shift_list_strides", "shift_R2"]),
    _case("exact_list_5000", Q5, 5, [("q5_r4", 5000)], ["exact_list_strides_counted", "exact_R4"]),
    _case("all_exact_2500_counted", Q8, 9, [("clean8", 1200), ("r2_at_0", 1300)], ["all_exact", "all_exact_strides_counted"], refused=3),
    _case("split_2049", Q8, 8, [("clean8", 2048), ("r2_at_0", 1)], ["fast_split_last_short", "shift_R2"], entries=("sum", "apply")),
    _case("slice_65537", Q8, 8, [("clean8", 65535), ("r3_adjacent", 1), ("r4", 1)], ["apply_second_slice", "shift_R3", "exact_R4"],
          entries=("sum", "apply")),
]
CASE = {c["name"]: c for c in CASES}


def first_chunk_rejections(seed, q):
    z = mc.zone(q)
    st = stream(tuple(seed))
    return sum(st[c] >= z for c in range(CHUNK))


def locate():
    """Find SEEDS.  Every target draws 4-word seeds from np.random.default_rng(<generator seed>).integers(0, 1 << 32, (N, 4)),
    narrows them with a vectorised test on the rejected candidates, and takes the first seed whose model run names every wanted
    branch.  Prints the table to paste into SEEDS."""
    def bad_of(S, q, n):
        return mc.candidates(S, (n + 7) // 8) >= np.uint64(mc.zone(q))

    def find(name, q, dim, want, gen, N, narrow, entry="sum"):
        S = np.random.default_rng(gen).integers(0, 1 << 32, size=(N, 4), dtype=np.int64)
        bad = bad_of(S, q, dim + 24)
        for r in np.flatnonzero(narrow(bad)):
            seed = tuple(int(w) for w in S[r])
            got = model({"q": q, "dim": dim, "keys": [(seed, 1)]}, entry)["branches"]
            if set(want) <= got:
                print(f'    "{name}": ({seed}, {QNAME[q]}, {dim}, {sorted(want)!r}),')
                return seed
        raise LookupError(name)

    def R(lo, hi, dim):
        return lambda bad: (bad[:, :dim].sum(axis=1) >= lo) & (bad[:, :dim].sum(axis=1) <= hi)

    find("clean8", Q8, 8, {"clean"}, 1, 1000, R(0, 0, 8))
    find("r1_first_last_lane", Q64, 20, {"shift_R1", "shift_lane_before_first", "shift_skip_in_lane", "src_o0", "tail_need_1", "tail_o0"}, 1, 4000,
         lambda b: (b[:, :20].sum(axis=1) == 1) & b[:, 9:16].any(axis=1))
    find("r2_at_0", Q8, 8, {"shift_R2", "reject_at_0", "tail_need_2", "tail_o1", "delta_neg", "delta_nonneg"}, 1, 4000,
         lambda b: (b[:, :8].sum(axis=1) == 2) & b[:, 0])
    find("r3_adjacent", Q8, 8, {"shift_R3", "fixpoint_2", "fixpoint_3", "tail_need_3"}, 1, 400000,
         lambda b: (b[:, :8].sum(axis=1) == 3) & (b[:, 0:6] & b[:, 1:7] & b[:, 2:8]).any(axis=1))
    find("r2_adjacent_last", Q8, 8, {"shift_R2", "fixpoint_2", "reject_at_last"}, 1, 40000,
         lambda b: (b[:, :8].sum(axis=1) == 2) & b[:, 6] & b[:, 7])
    find("tail_meets", Q8, 8, {"tail_meets_reject", "tail_o1"}, 1, 4000,
         lambda b: (b[:, :8].sum(axis=1) >= 1) & (b[:, :8].sum(axis=1) <= 3) & b[:, 8])
    find("tail_oc", Q8, 8, {"tail_cached", "tail_meets_reject"}, 1, 400000,
         lambda b: (b[:, :8].sum(axis=1) >= 1) & (b[:, :8].sum(axis=1) <= 3) & (b[:, 8:16].sum(axis=1) >= 6))
    find("r4", Q8, 8, {"exact_R4", "fast_fourth_not_stored", "slow_naive_subtract"}, 1, 4000, R(4, 4, 8))
    find("r6", Q8, 8, {"exact_many"}, 1, 400000, R(6, 8, 8))
    find("past_dim5", Q8, 5, {"fast_reject_past_dimension_not_recorded", "shift_R1", "tail_o0", "tail_meets_reject"}, 2, 40000,
         lambda b: (b[:, :5].sum(axis=1) == 1) & b[:, 5])
    find("q5_r4", Q5, 5, {"exact_R4"}, 2, 4000, R(4, 4, 5))
    find("q5_r3", Q5, 5, {"shift_R3", "tail_need_3"}, 2, 4000, R(3, 3, 5))
    find("q5_dim3", Q5, 3, {"shift_R2", "reject_at_last", "fast_reject_past_dimension_not_recorded"}, 2, 4000,
         lambda b: (b[:, :3].sum(axis=1) == 2) & b[:, 2] & b[:, 3:8].any(axis=1))
    find("edge_7_8", Q64, 20, {"adjacent_across_block_edge", "src_o1_d8", "src_o1_d9", "fixpoint_2"}, 3, 400000,
         lambda b: b[:, 7] & b[:, 8] & (b[:, :20].sum(axis=1) <= 3))
    find("d10", Q64, 20, {"src_o1_d10", "src_o1_d9", "src_o1_d8", "shift_R3"}, 3, 400000,
         lambda b: (b[:, :11].sum(axis=1) == 3) & (b[:, :20].sum(axis=1) == 3))
    find("earlier_lane", Q64, 10, {"tail_by_earlier_lane", "shift_R3", "tail_o1", "tail_o0"}, 3, 400000, R(3, 3, 10))
    find("q64_dim64", Q64, 64, {"shift_R2", "tail_o1"}, 4, 4000, R(2, 2, 64))
    find("q64_r5", Q64, 64, {"exact_many", "slow_cut_inside_lane"}, 4, 40000, R(5, 9, 64))
    # the exact-order walk: dimension from the seed's own first chunk
    S = np.random.default_rng(5).integers(0, 1 << 32, size=(3000, 4), dtype=np.int64)
    bad = bad_of(S, Q2048, CHUNK)
    for r in range(len(S)):
        rej = int(bad[r].sum())
        dim = CHUNK - rej
        if int(bad[r, :dim].sum()) >= 4 and int(bad[r, :dim + 1].sum()) >= 4:
            seed = tuple(int(w) for w in S[r])
            print(f'    "chunk_fit": ({seed}, Q2048, {dim}, ["slow_chunk_exact_fit", "slow_naive_subtract"]),   # {rej} rejected in the first chunk')
            print(f'    "chunk_fit_plus_1": ({seed}, Q2048, {dim + 1}, ["slow_next_chunk_one_mask", "slow_naive_subtract"]),')
            break
    find("q2048_r2", Q2048, 2048, {"shift_R2"}, 5, 3000, R(2, 2, 2048))


QNAME = {Q8: "Q8", Q64: "Q64", Q2048: "Q2048", Q5: "Q5", P62: "P62"}

if __name__ == "__main__":
    locate()

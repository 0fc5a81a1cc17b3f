"""Cases of sda_secret_unmasker_unmask_jobs_dev - unmask() fed by the recipient's two device jobs, receive.rs:148-156 - shared by
tests/test_unmask_jobs_reach.py (which proves from the Python-integer model below what the table contains, and that a planted fault
is noticed by a named case) and tests/test_unmask_jobs_gpu.py (which runs every case against the model and against the three-call
chain on twin jobs).

A case names a sharing scheme of tests/reconstruct_stream_cases.py, a masking kind and modulus, a dimension and the clerk index of
every position, how the clerking results and the masks are made, the byte offset of d_out from a 16-byte boundary and the gates.
build(name) makes its inputs once (deterministic) and is cached; nothing here needs a device or the C oracle.

The kernel takes two adjacent elements per lane, 256 lanes per workgroup: the lengths are 1 .. 5 (the odd tail, a lone pair), 511,
512, 513 (either side of one workgroup), 1000 and 6301 (several workgroups, an odd tail behind them), each with d_out on a 16-byte
boundary (one 16-byte store per pair) and 8 bytes past one (8-byte stores)."""
import collections
import functools
import zlib

import numpy as np

import chacha_repair as cr
import mask_combiner_cases as mc
import reconstruct_stream_cases as rc

P62, P31 = rc.P62, rc.P31
Q61 = (1 << 61) + 1                       # a masking modulus BELOW the sharing modulus P62: masked values >= q_mask occur (chacha_repair.Q8)
SENTINEL = 0x5A5A5A5A5A5A5A5A
TAIL = 8                                  # sentinel words behind the output
I64_MIN, I64_MAX = rc.I64_MIN, rc.I64_MAX

LENGTHS = (1, 2, 3, 4, 5, 511, 512, 513, 1000, 6301)

# masking: "full" | "chacha" | "none-null" (c = NULL) | "none-combiner" (a None combiner, begun)
# values : "random" = clerking results uniform in [0, p); "crafted" = any-int64 rows
# masks  : Full: "random" = 3 mask vectors uniform in [0, q_mask); "crafted" = any-int64 vectors
#          ChaCha: "seeds" = 5 seeds of 4 words; "noseed" = the job begun and nothing fed; a name of chacha_repair.SEEDS = that seed
# gates  : "null" = no gate; "two" = two words, both zero; "equal" = one zero word given twice;
#          "closed-masks" / "closed-results" / "closed-equal" = the named word holds 16 when the call is made: nothing may be stored
Case = collections.namedtuple("Case", "name scheme indices dim masking q_mask values masks offset gates")


def _cases():
    out = []
    gates = ("two", "null", "equal")
    for i, L in enumerate(LENGTHS):
        for off in (0, 8):
            out.append(Case(f"k3_62-full-d{L}-off{off}", "k3_62", rc.ALL8, L, "full", P62, "random", "random", off, gates[(i + off // 8) % 3]))
    # packed padding beyond k = 3: the last batch of k8_62 at 805 holds 3 padding sums, of pss155 at 250 fifty
    out.append(Case("k8_62-full-d805", "k8_62", tuple(range(26)), 805, "full", P62, "random", "random", 0, "two"))
    out.append(Case("pss155-full-d250", "pss155", rc.PSS_255, 250, "full", rc.TSS_P, "random", "random", 8, "two"))
    # Additive: L = row_len; crafted rows and masks bring negative high words on either side
    out.append(Case("additive-full-d1000", "additive", (0, 1, 2), 1000, "full", P62, "random", "random", 0, "two"))
    out.append(Case("additive-crafted-d1000", "additive", (0, 1, 2), 1000, "full", P62, "crafted", "crafted", 8, "two"))
    out.append(Case("additive-crafted-d5", "additive", (0, 1, 2), 5, "full", P62, "crafted", "crafted", 0, "null"))
    # the moduli differ: q_mask < q_share (masked values at or above q_mask), q_share < q_mask
    out.append(Case("k3_62-full61-d1000", "k3_62", rc.SCATTERED, 1000, "full", Q61, "random", "random", 0, "two"))
    out.append(Case("k3_62-full61-crafted-d513", "k3_62", rc.PERMUTED, 513, "full", Q61, "crafted", "crafted", 8, "equal"))
    out.append(Case("additive-full61-crafted-d1000", "additive", (0, 1, 2), 1000, "full", Q61, "crafted", "crafted", 0, "two"))
    out.append(Case("k3_31-full62-d1000", "k3_31", rc.ALL8, 1000, "full", P62, "random", "random", 0, "two"))
    out.append(Case("k3_31-full62-d4", "k3_31", rc.SEVEN, 4, "full", P62, "random", "random", 8, "null"))
    # ChaCha: seeds, no seed at all (chacha.rs:58), a located seed whose repaired sum is read
    out.append(Case("k3_62-chacha-d1000", "k3_62", rc.ALL8, 1000, "chacha", P62, "random", "seeds", 0, "two"))
    out.append(Case("k3_62-chacha-noseed-d1000", "k3_62", rc.ALL8, 1000, "chacha", P62, "random", "noseed", 8, "two"))
    out.append(Case("k3_62-chacha61-noseed-d4", "k3_62", rc.SCATTERED, 4, "chacha", Q61, "random", "noseed", 0, "null"))
    out.append(Case("k3_62-chacha-rejecting-d8", "k3_62", rc.ALL8, 8, "chacha", cr.Q8, "random", "r2_at_0", 0, "two"))
    out.append(Case("additive-chacha-d513", "additive", (0, 1, 2), 513, "chacha", P62, "crafted", "seeds", 8, "equal"))
    # None masking: out = masked
    out.append(Case("k3_62-none-null-d1000", "k3_62", rc.ALL8, 1000, "none-null", 0, "random", "none", 0, "null"))
    out.append(Case("k3_62-none-null-d4-off8", "k3_62", rc.SCATTERED, 4, "none-null", 0, "random", "none", 8, "two"))
    out.append(Case("k3_62-none-combiner-d1000", "k3_62", rc.ALL8, 1000, "none-combiner", 0, "random", "none", 8, "two"))
    out.append(Case("additive-none-combiner-d5", "additive", (0, 1, 2), 5, "none-combiner", 0, "crafted", "none", 0, "equal"))
    # a gate that is shut when the kernel runs: no store at all
    out.append(Case("k3_62-full-d1000-closed-masks", "k3_62", rc.ALL8, 1000, "full", P62, "random", "random", 0, "closed-masks"))
    out.append(Case("k3_62-full-d513-closed-results", "k3_62", rc.ALL8, 513, "full", P62, "random", "random", 8, "closed-results"))
    out.append(Case("additive-chacha-d5-closed-equal", "additive", (0, 1, 2), 5, "chacha", P62, "random", "seeds", 0, "closed-equal"))
    out.append(Case("k3_62-none-null-d4-closed-results", "k3_62", rc.SCATTERED, 4, "none-null", 0, "random", "none", 0, "closed-results"))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

FAULTS = ("recon_under_mask_modulus", "no_canonicalisation", "padding_stored", "gate_ignored")


def additive(case):
    return case.scheme == "additive"


def has_mask(case):
    return case.masking in ("full", "chacha")


def batches(case):
    p, k = rc.SCHEMES[case.scheme][:2]
    return case.dim if additive(case) else -(-case.dim // k)


def accumulators(case):
    """how many 128-bit sums the reconstructor job keeps: the padding of the last packed batch is summed like every output"""
    return case.dim if additive(case) else batches(case) * rc.SCHEMES[case.scheme][1]


@functools.lru_cache(maxsize=None)
def _matrix(scheme, indices):
    p, k, t, n, w2, w3 = rc.SCHEMES[scheme]
    return rc.lagrange_matrix(p, k, w2, w3, indices)


def chacha_masks(seed, q, dim):
    """the first `dim` masks of a seed in Python integers: rand-0.3 gen_range(0, q) takes the candidates below the zone, mod q"""
    z = mc.zone(q)
    v = [int(x) for x in mc.candidates(np.array([seed], dtype=np.int64), (2 * dim + 64 + 7) // 8)[0]]
    taken = [x % q for x in v if x < z][:dim]
    assert len(taken) == dim
    return taken


def chacha_rejections(seed, q, dim):
    """how many of the seed's first `dim` candidates the zone rejects"""
    z = mc.zone(q)
    return sum(int(x) >= z for x in mc.candidates(np.array([seed], dtype=np.int64), (dim + 7) // 8)[0][:dim])


Built = collections.namedtuple("Built", "rows mask_rows")

_SPECIAL = (I64_MIN, I64_MIN + 1, -1, -(1 << 62), I64_MAX, 0, 1, -P62, P62, -Q61, Q61 - 1, I64_MIN + 7)


@functools.lru_cache(maxsize=None)
def build(name):
    """rows [positions][row_len] int64 for reconstructor update_dev; mask_rows: Full [3][dim] mask vectors, ChaCha [seeds][4] seed
    words, None an empty matrix"""
    case = BY_NAME[name]
    p = rc.SCHEMES[case.scheme][0]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pos, B = len(case.indices), batches(case)
    special = np.array(_SPECIAL, dtype=np.int64)
    if case.values == "random":
        rows = rng.integers(0, p, size=(pos, B), dtype=np.int64)
    else:                                  # three quarters of the values negative: columns whose 128-bit sum is negative
        rows = special[rng.integers(0, 4, size=(pos, B))]
        mixed = rng.integers(0, 4, size=(pos, B)) == 0
        rows[mixed] = special[rng.integers(0, special.size, size=int(mixed.sum()))]
    if case.masking == "full":
        if case.masks == "random":
            mask_rows = rng.integers(0, case.q_mask, size=(3, case.dim), dtype=np.int64)
        else:
            mask_rows = special[rng.integers(0, 4, size=(3, case.dim))]
            mixed = rng.integers(0, 4, size=(3, case.dim)) == 0
            mask_rows[mixed] = special[rng.integers(0, special.size, size=int(mixed.sum()))]
    elif case.masking == "chacha":
        if case.masks == "seeds":
            mask_rows = rng.integers(0, 1 << 32, size=(5, 4), dtype=np.int64)
        elif case.masks == "noseed":
            mask_rows = np.zeros((0, 4), dtype=np.int64)
        else:
            mask_rows = np.array([cr.SEEDS[case.masks][0]], dtype=np.int64)
    else:
        mask_rows = np.zeros((0, 0), dtype=np.int64)
    rows.setflags(write=False)
    mask_rows.setflags(write=False)
    return Built(rows, mask_rows)


Model = collections.namedtuple("Model", "buffer recon_sums mask_sums masked mask out")


def gate_shut(case):
    return case.gates.startswith("closed")


@functools.lru_cache(maxsize=None)
def model(name, faults=frozenset()):
    """What the call leaves in a sentinel-filled buffer of offset / 8 + dim + TAIL words whose output starts at word offset / 8, in
    Python integers - and the exact sums, folds and differences it came from.  `faults` plants one of FAULTS."""
    case, b = BY_NAME[name], build(name)
    p, k = rc.SCHEMES[case.scheme][:2]
    qm = case.q_mask
    n_acc = accumulators(case)
    if additive(case):
        recon = [sum(int(r[i]) for r in b.rows) for i in range(n_acc)]
    else:
        R = _matrix(case.scheme, case.indices)
        canon = [[int(v) % p for v in r] for r in b.rows]
        recon = [sum(R[e][i] * canon[i][bb] for i in range(len(canon))) for bb in range(batches(case)) for e in range(k)]
    if case.masking == "full":
        mask_sums = [sum(int(r[i]) for r in b.mask_rows) for i in range(case.dim)]
    elif case.masking == "chacha":
        per_seed = [chacha_masks([int(w) for w in s], qm, case.dim) for s in b.mask_rows]
        mask_sums = [sum(m[i] for m in per_seed) for i in range(case.dim)]
    else:
        mask_sums = []
    fold_mod = qm if "recon_under_mask_modulus" in faults and has_mask(case) else p
    masked = [s % fold_mod for s in recon]
    if has_mask(case):
        mask = [s % qm for s in mask_sums] + [0] * (n_acc - case.dim)        # no mask sum exists for the padding
        if "no_canonicalisation" in faults:                 # submod on the operand as it came: a >= b ? a - b : a + m - b
            out = [(x - y if x >= y else x + qm - y) for x, y in zip(masked, mask)]
        else:
            out = [(x % qm - y) % qm for x, y in zip(masked, mask)]
    else:
        mask, out = [], list(masked)
    stored = len(out) if "padding_stored" in faults else case.dim
    head = case.offset // 8
    buf = [SENTINEL] * (head + case.dim + TAIL)
    if not gate_shut(case) or "gate_ignored" in faults:
        for i in range(min(stored, case.dim + TAIL)):
            buf[head + i] = out[i]
    return Model(tuple(buf), tuple(recon), tuple(mask_sums), tuple(masked[:case.dim]), tuple(mask[:case.dim]), tuple(out[:case.dim]))


def want(name):
    """the expected buffer as int64 (SENTINEL fits)"""
    return np.array(model(name).buffer, dtype=np.int64)

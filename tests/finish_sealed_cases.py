"""The case table of sda_share_combiner_finish_sealed_rows_dev (the clerk's last step, clerk.rs:84-100: the sums of a device job
reduced, varint encoded and sealed to the recipient, every row split over the chip), its reference in Python integers and a
restatement of the kernels' geometry.  tests/test_finish_sealed_reach.py proves on the CPU what the table reaches,
tests/test_finish_sealed_gpu.py runs it bit for bit.

A case fixes the modulus, the number of jobs, the dimension and - per job and column - the 128-bit SUM the accumulators must
hold; every sum is split into three int64 rows (any sum in [-3 * 2^63, 3 * (2^63 - 1)] is one) that go in through update_dev.
The sums are crafted from the residue a column must have (which fixes its varint length) plus a multiple of the modulus (which
moves the sum below 0, past 2^64, or onto a multiple of m without touching the residue).

Reference: sum(rows) mod m per column in Python integers -> oracle/pyoracle.py varint_encode (the Python-integer zig-zag LEB128
codec; oracle/wire_oracle.py holds the containers, not this codec) -> oracle/sealedbox_oracle.py seal with the injected secret.

Geometry (sda_amd/csrc/varint_kernels.hip, sum_len_kernel / sum_seal_wide_kernel): a row is cut into blocks of V = 2048 values,
one workgroup each; a block whose bytes start at message byte `off` and number `total` covers the XSalsa20 stream bytes
[32 + off, 32 + off + total), i.e. the Salsa20 blocks (32 + off) >> 6 .. (32 + off + total - 1) >> 6: at most total // 64 + 2."""
import numpy as np

V = 2048                                          # values per workgroup (kSumVals)
P62 = 4611686006577364993                         # the 62-bit prime of the benchmark configurations
M433 = 433                                        # the reference's own test prime
M_ADD = 10 ** 18                                  # a non-prime additive modulus below 2^62
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SUM_MIN, SUM_MAX = 3 * I64_MIN, 3 * I64_MAX       # what three int64 rows can sum to
FEED_ROWS = 3
SMALL_ORDER = bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800")
RECIPIENT_SK = bytes(range(101, 133))


# ---- the wire format in Python integers -------------------------------------------------------------------------------------------
def varint_len(r: int) -> int:
    """bytes of zig-zag LEB128 of a non-negative value r (zig-zag of r >= 0 is 2 r)"""
    return max(1, -(-(2 * r).bit_length() // 7))


def len_range(L: int, m: int):
    """the residues below m whose encoding takes L bytes, as (lo, hi) inclusive; None when there is none"""
    lo = 0 if L == 1 else 1 << (7 * L - 8)
    hi = min((1 << (7 * L - 1)) - 1, m - 1)
    return (lo, hi) if lo <= hi else None


def max_len(m: int) -> int:
    return varint_len(m - 1)


# ---- building sums ----------------------------------------------------------------------------------------------------------------
def split3(T: int):
    """three int64 whose sum is T"""
    assert SUM_MIN <= T <= SUM_MAX, T
    a = min(max(T, I64_MIN), I64_MAX)
    b = min(max(T - a, I64_MIN), I64_MAX)
    c = T - a - b
    assert I64_MIN <= c <= I64_MAX
    return a, b, c


def _lift(rng, r, m):
    """a sum with residue r: r + q m with q drawn so that negative sums, sums past 2^64 and plain ones all occur"""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return r
    if kind == 1:
        q = -int(rng.integers(1, max(2, (1 << 63) // m)))
    elif kind == 2:
        q = ((1 << 64) - r) // m + 1 + int(rng.integers(0, max(1, (1 << 62) // m)))      # r + q m >= 2^64
    else:
        q = int(rng.integers(1, max(2, (1 << 62) // m)))
    T = r + q * m
    return T if SUM_MIN <= T <= SUM_MAX else r


def _residue_of_len(rng, L, m):
    lo, hi = len_range(L, m)
    return lo + int(rng.integers(0, min(hi - lo, (1 << 62) - 1) + 1))


def _mixed(seed, m, dim, jobs=1, lens=None):
    """seeded mix of lengths (all the modulus allows, or those given), sums lifted off their residues"""
    rng = np.random.default_rng(seed)
    allowed = [L for L in (lens or range(1, 10)) if len_range(L, m)]
    return [[_lift(rng, _residue_of_len(rng, allowed[int(rng.integers(0, len(allowed)))], m), m) for _ in range(dim)] for _ in range(jobs)]


def _block_with_total(rng, m, count, want_mod, mod):
    """`count` residues of seeded lengths whose encoded bytes total want_mod modulo mod: the last 16 values make up the difference"""
    assert count > 16 and max_len(m) == 9
    lens = [int(rng.integers(1, 10)) for _ in range(count - 16)]
    need = (want_mod - sum(lens) - 16) % mod                       # extra bytes over sixteen 1-byte values
    assert need <= 16 * 8
    tail = [1 + min(8, max(0, need - 8 * i)) for i in range(16)]
    lens += tail
    assert sum(lens) % mod == want_mod
    return [_residue_of_len(rng, L, m) for L in lens]


def _stepping_blocks(seed, m, blocks, last):
    """every full block's bytes total 1 modulo 64: block b then starts at message offset b modulo 64"""
    rng = np.random.default_rng(seed)
    res = []
    for _ in range(blocks - 1):
        res += _block_with_total(rng, m, V, 1, 64)
    res += [_residue_of_len(rng, int(rng.integers(1, 10)), m) for _ in range(last)]
    return [[_lift(rng, r, m) for r in res]]


def _of_lens(seed, m, per_job_lens):
    rng = np.random.default_rng(seed)
    return [[_lift(rng, _residue_of_len(rng, L, m), m) for L in lens] for lens in per_job_lens]


def _limits(m):
    """residues at both ends, every length boundary the modulus allows, sums at the ends of the 128-bit cases"""
    T = [0, m - 1, -1, -m, m, 3 * m, -3 * m, (1 << 64), (1 << 64) - 1, (1 << 64) + 5, SUM_MAX, SUM_MIN, -(1 << 64), I64_MAX, I64_MIN,
         ((1 << 64) // m + 1) * m, -(((1 << 64) // m + 1) * m)]
    for L in range(1, 10):
        if len_range(L, m):
            lo, hi = len_range(L, m)
            T += [lo, hi, lo - m, hi + (((1 << 64) // m) + 1) * m]
    return [[t for t in T if SUM_MIN <= t <= SUM_MAX]]


def _case(name, m, sums):
    jobs, dim = len(sums), len(sums[0])
    assert all(len(s) == dim for s in sums)
    return dict(name=name, m=m, jobs=jobs, dim=dim, sums=sums)


def _build():
    nine, one = [9] * V, [1] * V
    return [
        _case("limits-p62", P62, _limits(P62)),
        _case("limits-433", M433, _limits(M433)),
        _case("limits-additive", M_ADD, _limits(M_ADD)),
        _case("dim1", P62, _mixed(11, P62, 1)),
        _case("dim2", P62, _mixed(12, P62, 2)),
        _case("V-1", P62, _mixed(13, P62, V - 1)),
        _case("V", P62, _mixed(14, P62, V)),
        _case("V+1", P62, _mixed(15, P62, V + 1)),
        _case("2V", M_ADD, _mixed(16, M_ADD, 2 * V)),
        _case("2V+1", P62, _mixed(17, P62, 2 * V + 1)),
        _case("blocks70", P62, _stepping_blocks(18, P62, 70, V - 37)),
        _case("all1-all9", P62, _of_lens(19, P62, [one + nine + [1, 9, 1, 9, 5]])),
        # message lengths around the first Salsa20 block's edge (stream byte 64 = message byte 32): 31, 32 and 33 bytes
        _case("edge32", P62, _of_lens(20, P62, [[9, 9, 8, 1, 1, 1, 1, 1], [9, 9, 9, 1, 1, 1, 1, 1], [9, 9, 9, 2, 1, 1, 1, 1]])),
        # jobs whose rows differ in length and end inside a dword: the next job's first block starts its scan entry off a boundary
        _case("jobs2", P62, _of_lens(21, P62, [[9] * 100 + [1] * 201, [2] * 300 + [3]])),
        _case("jobs3", P62, _of_lens(22, P62, [[9] * V + [1] * 6 + [3], [1] * V + [9] * 6 + [4], [5] * V + [3] * 7])),
        _case("433-2V", M433, _mixed(23, M433, 2 * V - 3, jobs=2)),
    ]


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}


# ---- what a case feeds and what it must give ----------------------------------------------------------------------------------------
def rows_of(case):
    """[jobs][FEED_ROWS][dim] int64: job j's rows for update_dev (job_stride = FEED_ROWS * dim, row_stride = dim)"""
    out = np.empty((case["jobs"], FEED_ROWS, case["dim"]), dtype=np.int64)
    for j, sums in enumerate(case["sums"]):
        for i, T in enumerate(sums):
            out[j, :, i] = split3(T)
    return out


def residues_of(case, rows=None):
    """per job the canonical residues of the column sums, from the ROWS (Python integers)"""
    rows = rows_of(case) if rows is None else rows
    return [[sum(int(rows[j, r, i]) for r in range(rows.shape[1])) % case["m"] for i in range(rows.shape[2])] for j in range(rows.shape[0])]


def payloads_of(case, rows=None):
    from oracle import pyoracle as po
    return [po.varint_encode(res) for res in residues_of(case, rows)]


def recipient_keys():
    from oracle import sealedbox_oracle as so
    return so.x25519_base(RECIPIENT_SK), RECIPIENT_SK


def esk_of(case):
    return bytes(np.random.default_rng(5000 + CASES.index(BY_NAME[case["name"]])).integers(0, 256, 32 * case["jobs"], dtype=np.uint8))


def oracle_boxes(case, pk=None, rows=None, esk=None):
    from oracle import sealedbox_oracle as so
    pk = recipient_keys()[0] if pk is None else pk
    esk = esk_of(case) if esk is None else esk
    return [so.seal(m, pk, esk[32 * j:32 * j + 32]) for j, m in enumerate(payloads_of(case, rows))]


# ---- the kernels' geometry, restated -------------------------------------------------------------------------------------------------
def geometry(residues):
    """per block of one job: (message offset, byte total, first Salsa20 block, Salsa20 blocks needed)"""
    out, off = [], 0
    for b in range(0, len(residues), V):
        total = sum(varint_len(r) for r in residues[b:b + V])
        first = (32 + off) >> 6
        count = ((32 + off + total - 1) >> 6) - first + 1 if total else 0
        out.append((off, total, first, count))
        off += total
    return out


def scan_entries(case):
    """the exclusive scan the device runs over ALL jobs' block totals (job-major), per job"""
    out, run = [], 0
    for res in residues_of(case):
        entries = []
        for _, total, _, _ in geometry(res):
            entries.append(run)
            run += total
        out.append(entries)
    return out

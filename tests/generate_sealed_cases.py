"""The case table of sda_share_generator_generate_sealed_rows_dev (secrets in, sealed clerking-job rows out, no share in HBM),
shared by tests/test_generate_sealed_reach.py (what the cases reach, proved on the CPU with the oracle alone) and
tests/test_generate_sealed_gpu.py (the boxes, byte for byte) - a helper module, not a conftest.

The oracle is independent of the library: coracle.drbg_fill -> coracle.packed_generate_csprng / additive_generate ->
coracle.varint_encode -> sealedbox_oracle.seal.  Every case is the smallest shape at which the thing its name says can go
wrong: the kernel's step is 128 values (2 per lane), a DPP quad holds 8 batches, the keystream tile is refilled when the write
cursor reaches message byte 4064 and again at 8160."""
import numpy as np

import drbg_retry as dr

P62 = 4611686006577364993
P31 = 2147483647                                  # 2^31 - 1: above the paired rule's bound, below 2^31
P_PAIRED = 746497                                 # tss's shipped prime: <= 0x7F7F7F, the paired draw rule
PM = dr.PM                                        # just above 2^64 / 5: one candidate in five is rejected
KEY = dr.KEY
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SMALL_ORDER = bytes.fromhex("e0eb7a7c3b41b8ae1656e3faf19fc46ada098deb9c32b1fd866205165f49b800")

def _next_prime(x):
    while not dr.is_prime(x):
        x += 1
    return x


P41, P47 = _next_prime(1 << 41), _next_prime(1 << 47)   # shares of 6 and of 7 varint bytes (over P62 nearly all have 9)
STEP = 128                                        # values per encode step
REFILLS = (4064, 8160)                            # message bytes at which the keystream tile is refilled


def _case(name, k, t, n, p, length, participants=1, first=0, additive=False, stride=None, offset=0, secrets="canonical",
          small_order=None, seed=None):
    """k, t, n, p: the scheme (additive: k = 1, t = n - 1); length: secrets per participant; first: stream id of participant 0;
    stride / offset: layout of the secrets on the device (elements); secrets: "canonical" residues or "any" int64 with both
    extremes; small_order: index of the clerk whose key is a point of small order"""
    return dict(name=name, k=k, t=t, n=n, p=p, len=length, participants=participants, first=first, additive=additive,
                stride=length if stride is None else stride, offset=offset, secrets=secrets, small_order=small_order,
                seed=sum(name.encode()) if seed is None else seed)


def _paired_first(p, t):
    """a first participant whose job of 3 streams holds a located rejected pair (drbg_retry.PAIRED_HITS), and its batch count"""
    stream, pairs = dr.PAIRED_HITS[(p, t)][0]
    return dr.located_job(stream, max(b for b, _ in pairs))


_Q8, _QANY = dr.PAIRED_PRIMES["fft8"][0], dr.PAIRED_PRIMES["any"][0]
_F_EVEN, _B_EVEN = _paired_first(_Q8, 4)
_F_ODD, _B_ODD = _paired_first(_QANY, 7)
_DEEP = next(c for c in dr.DEEP_CASES if c["name"] == "deep-additive")["hit"]       # (stream, batch, draw) needing attempt 2

CASES = [
    # batch counts: an odd tail, a quad partly past the end, a group of 8 straddling the end, one and two step boundaries;
    # len = 3 B - 1, so the last batch of every one of them is zero padded
    *[_case(f"B{B}", 3, 1, 8, P62, 3 * B - 1) for B in (1, 2, 3, 7, 8, 9, 127, 128, 129, 257)],
    _case("len-below-k", 3, 1, 8, P62, 2),
    _case("len-multiple-of-k", 3, 1, 8, P62, 3 * 10),
    # the keystream tile: B values of 9 bytes cross message byte 4064 once, 8160 twice
    _case("refill-once", 3, 1, 8, P62, 3 * 460, participants=5, first=(1 << 32) + 5),
    _case("refill-twice", 3, 1, 8, P62, 3 * 920 - 2),
    # schemes
    _case("packed-8-2-26", 8, 2, 26, P62, 8 * 9 - 3, participants=2),
    _case("packed-3-4-8-p31", 3, 4, 8, P31, 3 * 9 - 1, participants=5, first=7),
    _case("packed-k-plus-t-32", 20, 12, 35, P62, 20 * 3 - 7),
    _case("additive-n3", 1, 2, 3, P62, 131, participants=5, additive=True, first=(1 << 40) + 1),
    _case("additive-n2", 1, 1, 2, P62, 9, additive=True),
    # value widths between the narrow primes and the 62-bit one
    _case("p41", 3, 1, 8, P41, 3 * 70 - 1),
    _case("p47", 1, 2, 3, P47, 200, additive=True),
    _case("p61", 1, 2, 3, 61, 40, additive=True),          # every share fits one byte
    # the paired draw rule (moduli <= 0x7F7F7F): odd and even t
    _case("paired-odd-t", 3, 1, 8, P_PAIRED, 3 * 9 - 1, participants=5),
    _case("paired-t3", 3, 3, 8, P_PAIRED, 3 * 9 - 1),
    _case("paired-even-t", 3, 4, 8, P_PAIRED, 3 * 9 - 1),
    # the retry stream: one candidate in five rejected; located rejected pairs; a located second attempt
    _case("retry-packed", 3, 1, 8, PM, 3 * 29 - 1, participants=3, first=dr.FIRST),
    _case("retry-additive", 1, 2, 3, PM, 15, participants=3, additive=True, first=dr.FIRST),
    _case("retry-paired-even-t", 3, 4, 8, _Q8, 3 * _B_EVEN - 1, participants=3, first=_F_EVEN),
    _case("retry-paired-odd-t", 8, 7, 26, _QANY, 8 * _B_ODD - 1, participants=3, first=_F_ODD),
    _case("retry-second-attempt", 1, 2, 3, PM, (_DEEP[1] + 1) | 1, additive=True, first=_DEEP[0]),
    # secrets: any int64, a stride with junk between the rows, an offset that leaves the rows off the 16-byte grid
    _case("any-i64-secrets", 3, 1, 8, P62, 3 * 50 - 1, participants=5, secrets="any", stride=3 * 50 + 6, offset=1),
    _case("any-i64-additive", 1, 2, 3, P62, 77, participants=5, additive=True, secrets="any", stride=81, offset=3),
    _case("odd-stride", 3, 1, 8, P62, 3 * 40, participants=5, stride=3 * 40 + 1, first=(1 << 55) + 3),
    # a clerk key of small order: that clerk's rows are refused, every other row is intact
    _case("small-order-clerk", 3, 1, 8, P62, 3 * 20 - 1, participants=5, small_order=5),
    _case("small-order-additive-last", 1, 2, 3, P62, 20, participants=5, additive=True, small_order=2),
]
BY_NAME = {c["name"]: c for c in CASES}


def batches(case):
    return (case["len"] + case["k"] - 1) // case["k"]


def rows(case):
    return case["n"] * case["participants"]


def omegas(case):
    import extremes
    return extremes.omegas(case["p"], case["k"], case["t"], case["n"])


def share_maps(case):
    """the share maps a generator of this scheme offers its CSPRNG calls: systematic (1) and tss's nodes (0) for packed Shamir
    with t > 0 on the matrix-form kernels; one map (None) for additive sharing"""
    return [None] if case["additive"] else [1, 0]


def secrets_of(case):
    """[participants][len] int64"""
    rng = np.random.default_rng(case["seed"])
    P, L = case["participants"], case["len"]
    if case["secrets"] == "any":
        s = rng.integers(I64_MIN, I64_MAX, size=(P, L), dtype=np.int64)
        s.flat[0], s.flat[-1] = I64_MIN, I64_MAX
        if s.size > 4:
            s.flat[1], s.flat[2] = I64_MAX, I64_MIN
        return s
    return rng.integers(0, case["p"], size=(P, L), dtype=np.int64)


def draws_of(case, q, key=KEY):
    """the sda-drbg-v1 draws of participant q: [B * T]"""
    from oracle import coracle
    return coracle.drbg_fill(key, case["first"] + q, batches(case), case["t"], case["p"])


def shares_of(case, share_map, key=KEY):
    """the oracle's shares: [n][participants][B] int64 (clerk-major, as the rows of the call)"""
    from oracle import coracle
    sec = secrets_of(case)
    p, k, t, n = case["p"], case["k"], case["t"], case["n"]
    out = np.empty((n, case["participants"], batches(case)), dtype=np.int64)
    w2, w3 = (0, 0) if case["additive"] else omegas(case)
    for q in range(case["participants"]):
        canon = sec[q] if case["secrets"] == "canonical" else np.array([int(x) % p for x in sec[q]], dtype=np.int64)
        if case["additive"]:
            out[:, q, :] = coracle.additive_generate(p, n, canon, draws_of(case, q, key))
        else:
            out[:, q, :] = coracle.packed_generate_csprng(p, k, t, n, w2, w3, canon, draws_of(case, q, key), share_map)
    return out


def clerk_keys(case):
    """[(pk, sk)] per clerk; the small-order clerk has no secret key"""
    from oracle import sealedbox_oracle as so
    rng = np.random.default_rng(case["seed"] + 17)
    keys = []
    for c in range(case["n"]):
        sk = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        keys.append((SMALL_ORDER, None) if c == case["small_order"] else (so.x25519_base(sk), sk))
    return keys


def esk_of(case):
    return bytes(np.random.default_rng(case["seed"] + 1000).integers(0, 256, 32 * rows(case), dtype=np.uint8))


def payloads_of(case, share_map, key=KEY):
    """the varint payload of every row, row r = c * participants + q"""
    from oracle import coracle
    sh = shares_of(case, share_map, key)
    return [coracle.varint_encode(sh[c, q]) if sh.shape[2] else b"" for c in range(case["n"]) for q in range(case["participants"])]


def oracle_boxes(case, share_map, key=KEY):
    """the reference's box of every row; None for the rows of the small-order clerk"""
    from oracle import sealedbox_oracle as so
    keys, esk, P = clerk_keys(case), esk_of(case), case["participants"]
    out = []
    for r, msg in enumerate(payloads_of(case, share_map, key)):
        out.append(None if r // P == case["small_order"] else so.seal(msg, keys[r // P][0], esk[32 * r:32 * r + 32]))
    return out

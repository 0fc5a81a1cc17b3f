"""The case table of sda_secret_masker_mask_sealed_rows_dev (secrets in; masked secrets and the sealed mask rows out, no mask in
HBM) and its reference, shared by tests/test_mask_sealed_reach.py (what the cases reach, proved on the CPU with the oracle alone)
and tests/test_mask_sealed_gpu.py (boxes, lengths and masked secrets, bit for bit) - a helper module, not a conftest.  It runs
no code under test.

Reference, Full:   masks  = coracle.drbg_fill(KEY, first + p, len, 1, q, rounds)
                   masked = (secret mod q + mask) mod q in Python integers
                   box    = sealedbox_oracle.seal(coracle.varint_encode(mask), pk, esk_p)
Reference, ChaCha: masked = (secret mod q + coracle.chacha_expand(seed, q, dimension)) mod q; the box of the seed words.

Every case is the smallest shape at which the thing its purpose names can go wrong: the kernel's step is 128 values (2 per
lane), the keystream tile is refilled when the write cursor reaches message byte 4064 and again at 8160, a workgroup holds 4
rows."""
import numpy as np

import drbg_retry as dr
import mask_combiner_cases as mc
from generate_sealed_cases import I64_MAX, I64_MIN, P31, P62, P_PAIRED, REFILLS, SMALL_ORDER, STEP

KEY, FIRST, PM = dr.KEY, dr.FIRST, dr.PM
WAVES = 4                                         # rows per workgroup


def _full(name, q, participants, length, purpose, first=0, s_stride=None, m_stride=None, offset=0, in_place=False, small_order=False):
    """s_stride / m_stride / offset: layout of the secrets and of the masked secrets on the device, in elements (in place: one
    buffer); small_order: the recipient key is a point of small order"""
    return dict(name=name, kind="full", q=q, participants=participants, len=length, first=first, purpose=purpose,
                s_stride=length if s_stride is None else s_stride, m_stride=length if m_stride is None else m_stride, offset=offset,
                in_place=in_place, small_order=small_order, seed=sum(name.encode()))


FULL_CASES = [
    _full("1x1", P62, 1, 1, "smallest row"),
    _full("3x129-misaligned", P62, 3, 129, "odd tail, second step of one value, 8-byte path", s_stride=131, m_stride=131, offset=1),
    _full("2x460", P62, 2, 460, "crosses keystream refill at message byte 4064"),
    _full("1x1000", P62, 1, 1000, "crosses keystream refill at message byte 8160"),
    _full("433-5x700", 433, 5, 700, "one- and two-byte values"),
    _full("paired-4x300", P_PAIRED, 4, 300, "paired draw rule"),
    _full("p31-2x257", P31, 2, 257, "31-bit prime"),
    _full("pm-3x2000", PM, 3, 2000, "rejected candidates in every row", first=FIRST),
    _full("last-streams-3x40", P62, 3, 40, "last admissible stream ids", first=(1 << 56) - 3),
    _full("70x40", P62, 70, 40, "a last workgroup with idle waves"),
    _full("3x129-in-place", P62, 3, 129, "in-place masking", in_place=True),
    _full("small-order-2x200", P62, 2, 200, "refused rows", small_order=True),
]


def _chacha(q, dim, seeds, bits, plan, small_order=False, tag=""):
    """plan: what the shape's source table (mask_combiner_cases) names - "clean" (no rejected candidate), "all-exact" ((modulus,
    dimension) send every seed through the exact-order walk) or "both-lists" (clean, shift-list and exact-order-list seeds)"""
    name = f"chacha-{q}-{dim}x{seeds}-{bits}{tag}"
    return dict(name=name, kind="chacha", q=q, len=dim, participants=seeds, bits=bits, words=(bits + 31) // 32, plan=plan,
                small_order=small_order, first=0, s_stride=dim + 3, m_stride=dim + 1, offset=0, in_place=False, seed=sum(name.encode()))


_PLANS = {(433, 1000, 5): "clean", (P62, 4099, 9): "clean", (mc.Q_HEAVY, 3000, 6): "all-exact", mc.BOTH_LISTS: "both-lists"}
assert all(s in mc.CHACHA_SHAPES for s in _PLANS)
CHACHA_CASES = [_chacha(*shape, bits, plan) for shape, plan in _PLANS.items() for bits in (128, 256)] + [
    _chacha(433, 1000, 5, 288, "clean"),                         # nine words: all sent, eight used
    _chacha(433, 1000, 5, 128, "clean", small_order=True, tag="-small-order"),
]
CASES = FULL_CASES + CHACHA_CASES
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def mask_len(case):
    """values in a participant's sealed mask: sda_secret_masker_mask_len"""
    return case["len"] if case["kind"] == "full" else case["words"]


def secrets_of(case):
    """[participants][len]: any int64, with INT64_MIN, INT64_MAX, -1 and 0 among them"""
    rng = np.random.default_rng(case["seed"])
    s = rng.integers(I64_MIN, I64_MAX, size=(case["participants"], case["len"]), dtype=np.int64)
    specials = [I64_MIN, I64_MAX, -1, 0]
    for r in range(s.shape[0]):                                  # at the front of every row as far as it reaches, rotated
        for i in range(min(4, s.shape[1])):
            s[r, i] = specials[(i + r) % 4]
    return s


def keys_of(case):
    """the recipient's (pk, sk); a small-order key has no secret key"""
    from oracle import sealedbox_oracle as so
    if case["small_order"]:
        return SMALL_ORDER, None
    sk = bytes(np.random.default_rng(case["seed"] + 17).integers(0, 256, 32, dtype=np.uint8))
    return so.x25519_base(sk), sk


def esk_of(case):
    return bytes(np.random.default_rng(case["seed"] + 1000).integers(0, 256, 32 * case["participants"], dtype=np.uint8))


def seeds_of(case):
    """ChaCha: [participants][words] seed words (u32 values held in int64).  128 bits: the source table's own seed matrix; wider
    seeds come from the next generator seed, because the table's seed gives the 8-word matrix of BOTH_LISTS no seed for the
    exact-order list (test_mask_sealed_reach.py asserts what every matrix reaches)"""
    q, dim, P, words = case["q"], case["len"], case["participants"], case["words"]
    if words == 4:
        return mc.seed_matrix(q, dim, P, 4)
    return np.random.default_rng(mc.generator_seed(q, dim, P) + 1).integers(0, 1 << 32, size=(P, words), dtype=np.int64)


def masks_of(case, rounds=20, key=KEY):
    """what each participant sends to the recipient: Full [participants][len] draws, ChaCha the seed words"""
    from oracle import coracle
    if case["kind"] == "chacha":
        return seeds_of(case)
    return np.stack([coracle.drbg_fill(key, case["first"] + p, case["len"], 1, case["q"], rounds) for p in range(case["participants"])])


def added_masks_of(case, rounds=20, key=KEY):
    """what is added onto the secrets: the draws themselves (Full), the expansion of the seed (ChaCha)"""
    from oracle import coracle
    if case["kind"] == "chacha":
        S = seeds_of(case)
        return np.stack([coracle.chacha_expand(S[p], case["q"], case["len"]) for p in range(case["participants"])])
    return masks_of(case, rounds, key)


def masked_of(case, rounds=20, key=KEY):
    q, sec, add = case["q"], secrets_of(case), added_masks_of(case, rounds, key)
    out = np.empty(sec.shape, dtype=np.int64)
    for p in range(sec.shape[0]):
        out[p] = [(int(s) % q + int(m)) % q for s, m in zip(sec[p], add[p])]
    return out


def payloads_of(case, rounds=20, key=KEY):
    from oracle import coracle
    M = masks_of(case, rounds, key)
    return [coracle.varint_encode(M[p]) if M.shape[1] else b"" for p in range(M.shape[0])]


def oracle_boxes(case, rounds=20, key=KEY):
    """the reference's recipient_encryption of every participant; None where the recipient key is of small order"""
    from oracle import sealedbox_oracle as so
    (pk, _), esk = keys_of(case), esk_of(case)
    return [None if case["small_order"] else so.seal(msg, pk, esk[32 * p:32 * p + 32]) for p, msg in enumerate(payloads_of(case, rounds, key))]

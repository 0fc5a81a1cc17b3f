"""Cases that make the retry stream of the device CSPRNG (sda-drbg-v1) run in every kernel that draws randomness
(shared by tests/test_drbg_retry_reach.py and tests/test_drbg_retry_gpu.py - a helper module, not a conftest).

A draw's first candidate comes from the main block of its batch group (block counter (b >> 3) T + i, word pair b & 7); a
candidate Lemire's test rejects is replaced from a retry block keyed by the batch's own counter (b T + i; under the paired rule
b ceil(T / 2) + j), attempt number a = 1, 2, .. in the top byte of state word 15 above the top 24 bits of the stream id, eight
candidates per attempt.  Each kernel family writes that retry counter out on its own (drbg_pair / drbg_retry /
drbg_retry_pair, drbg_pair_m32, three branches of the transform kernel, ng_draw_fixup), and over the primes of the other
suites (rejection rates 2^-18 .. 2^-56) no test of ordinary size ever enters it.  This module holds

  * moduli that make rejection the rule: primes just above 2^64 / 5, the peak of (2^64 mod m) / 2^64 for m < 2^62 (0.2), one
    per divisibility the transform shapes need (WIDE_PRIMES);
  * a vectorised numpy restatement of the first-attempt candidates (first_attempt) and of one retry attempt (retry_attempt):
    which draws of a job are rejected, at which batch, position b & 7, draw index and participant, and how deep a located
    draw goes into its retry stream (retry_depth).  The values themselves are never taken from here: the GPU test compares
    with the C oracle, the reach test ties the C oracle to the big-int one (pyoracle.drbg_value) at the located draws;
  * the case tables of the GPU test.  A batch count `B` of a 0.2-rate case is the SMALLEST odd one (never a multiple of 8: a
    ragged last group, and with dim = B k - 1 a ragged last batch) at which the coverage conditions of
    tests/test_drbg_retry_reach.py hold (smallest_batches re-derives it there);
  * the paired rule (moduli <= 0x7F7F7F, rejection below 2^-18 per pair): rejections are LOCATED, not forced - stream ids
    searched upward from a fixed start for streams whose first <= 1024 batches hold a rejected pair (locate_paired), recorded
    here as constants (PAIRED_HITS) and re-derived by the reach test;
  * streams whose first <= 4096 batches hold a draw that needs a SECOND retry attempt (a = 2; probability 0.2^9 per draw),
    located the same way (locate_second_attempt, DEEP_HITS).

Out of reach, and therefore not tested: the 32-bit Lemire forms (lemire_sample_m32 of narrow_gen.inc.hpp, f_lemire32 of
drbg_lane.hpp) serve 0x7F7F7F < p < 2^31, where a candidate word is rejected with probability p / 2^64 < 2^-33; no scan that
fits in a test finds such a candidate, so the retry calls behind those two forms stay unexercised."""
import numpy as np

M64 = (1 << 64) - 1
PAIRED_MAX = 0x7F7F7F
KEY = bytes((i * 11 + 3) & 0xFF for i in range(32))
PARTICIPANTS = 3
FIRST = (0xA5C3 << 32) | 0x89ABCDEF             # stream ids with bits above bit 32: word 15 of a retry block carries both parts
FIRST_LAST = (1 << 56) - PARTICIPANTS           # the last admissible ids

# ---- moduli ------------------------------------------------------------------------------------------------------------------
# use -> (prime, what must divide p - 1): the primes just above 2^64 / 5 with that divisibility
WIDE_PRIMES = {
    "matrix": (3689348814741910379, 1),                    # any omegas with distinct nodes (extremes.omegas)
    "fft8": (3689348814741910609, 8 * 9),                  # forced transform, k + t + 1 = 8, n + 1 = 9
    "fft242": (3689348814741974401, 64 * 243),             # (40, 23, 242)
    "fft728": (3689348814746422273, 256 * 729),            # (100, 155, 728)
    "fft2186": (3689348814754633729, 256 * 2187),          # (100, 155, 2186)
    "fft19682": (3689348814757433089, 256 * 19683),        # (100, 155, 19682)
}
PM = WIDE_PRIMES["matrix"][0]
# the primes <= 0x7F7F7F with the highest paired-rule rejection rate among those with that divisibility (best_paired_prime)
PAIRED_PRIMES = {
    "fft8": (8242849, 8 * 9),                              # 3.68e-6
    "fft242": (8211457, 64 * 243),                         # 2.95e-6 (the prime of the limb GEMM's volume test)
    "any": (8348261, 1),                                   # 3.77e-6: the highest of all
}


def is_prime(n):
    """Miller-Rabin with the first twelve primes as bases: deterministic below 3.3e24"""
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    if n < 2:
        return False
    for q in bases:
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in bases:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def paired(m):
    return m <= PAIRED_MAX


def threshold(m):
    """Lemire's rejection threshold of the rule m draws under: 2^64 mod m^2 (paired) or 2^64 mod m"""
    return (1 << 64) % (m * m if paired(m) else m)


def rejection_rate(m):
    return threshold(m) / 2.0 ** 64


def best_paired_prime(div):
    """the prime p <= 0x7F7F7F, p = 1 mod div, with the highest paired-rule rejection rate (sieve + big-int thresholds)"""
    sieve = np.ones(PAIRED_MAX + 1, dtype=bool)
    sieve[:2] = False
    for q in range(2, int(PAIRED_MAX ** 0.5) + 1):
        if sieve[q]:
            sieve[q * q::q] = False
    cand = np.flatnonzero(sieve[1::div]) * div + 1
    return max((int(p) for p in cand), key=threshold)


def root(p, order):
    """an element of exactly that order (order = 2^a 3^b)"""
    assert (p - 1) % order == 0
    for g in range(2, 2000):
        w = pow(g, (p - 1) // order, p)
        if all(pow(w, order // f, p) != 1 for f in (2, 3) if order % f == 0):
            return w
    raise AssertionError("no root")


def omegas(case):
    """roots of order k + t + 1 and n + 1 where the shape is a transform shape and the prime has them, else any distinct nodes"""
    import extremes
    k, t, n, p = case["k"], case["t"], case["n"], case["p"]
    m2, m3 = k + t + 1, n + 1
    if m2 & (m2 - 1) == 0 and m3 in [3 ** e for e in range(2, 10)] and (p - 1) % (m2 * m3) == 0:
        return root(p, m2), root(p, m3)
    return extremes.omegas(p, k, t, n)


def family_of(case):
    """the kernel family (sda_amd/csrc/path_select.hpp) the kernel name of a packed-Shamir case belongs to"""
    name = case["kernel"]
    for part, family in (("mfma", "mfma"), ("l31_rtg", "l31_global"), ("l31", "l31"), ("n31", "n31"), ("generic", "generic"),
                         ("fft", "fft"), ("side stream", "fft"), ("unsigned int", "fft"), ("packed_gen_kernel<", "mont64")):
        if part in name:
            return family
    raise AssertionError(name)


# ---- the stream layout, vectorised ---------------------------------------------------------------------------------------------
CHACHA_CONST = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


def key_words(key):
    return [int.from_bytes(key[4 * j:4 * j + 4], "little") for j in range(8)]


def chacha_words(key, counters, streams, attempt=0, rounds=20):
    """the ChaCha blocks of sda-drbg-v1 for arrays of block counters and stream ids: words 12, 13 = counter, 14 = lo32(stream),
    15 = (stream >> 32) & 0xFFFFFF | attempt << 24.  -> (16, len) uint32 (the block function itself is pinned by the RFC 7539
    vectors of tests/test_oracle.py; tests/test_drbg_retry_reach.py compares this restatement with the C oracle's block)"""
    counters = np.asarray(counters, dtype=np.uint64)
    streams = np.broadcast_to(np.asarray(streams, dtype=np.uint64), counters.shape)
    n = len(counters)
    st = [np.full(n, c, dtype=np.uint32) for c in CHACHA_CONST] + [np.full(n, w, dtype=np.uint32) for w in key_words(key)]
    st += [(counters & np.uint64(0xFFFFFFFF)).astype(np.uint32), (counters >> np.uint64(32)).astype(np.uint32),
           (streams & np.uint64(0xFFFFFFFF)).astype(np.uint32),
           ((streams >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.uint32) | np.uint32(attempt << 24)]
    x = [v.copy() for v in st]

    def rot(v, r):
        return (v << np.uint32(r)) | (v >> np.uint32(32 - r))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rot(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rot(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rot(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rot(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(rounds // 2):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        return np.stack([x[i] + st[i] for i in range(16)])


def _rejected(x, m):
    """Lemire's test on candidate words (uint64 array): lo64(x m) < 2^64 mod m, or under the paired rule lo64(x m m) < 2^64 mod m^2"""
    with np.errstate(over="ignore"):
        lo = x * np.uint64(m)
        if paired(m):
            lo = lo * np.uint64(m)
    return lo < np.uint64(threshold(m))


def draws_per_batch(T, m):
    """candidate words per batch: one per draw, or one per draw PAIR under the paired rule"""
    return (T + 1) // 2 if paired(m) else T


def first_attempt(key, streams, B, T, m, rounds=20):
    """the first-attempt candidates of batches 0 .. B - 1 of each stream: -> (x, rejected), both [streams][B][D] with
    D = draws_per_batch(T, m).  Main block of batch group g and draw (pair) d: counter g D + d; batch 8 g + w takes word pair
    (8 e + c, 8 e + 4 + c), c = w >> 1, e = w & 1."""
    streams = np.atleast_1d(np.asarray(streams, dtype=np.uint64))
    S, D, G8 = len(streams), draws_per_batch(T, m), (B + 7) // 8
    ctr = np.tile(np.arange(G8 * D, dtype=np.uint64), S)
    o = chacha_words(key, ctr, np.repeat(streams, G8 * D), 0, rounds).reshape(16, S, G8, D)
    x = np.empty((S, G8, 8, D), dtype=np.uint64)
    for w in range(8):
        hi = 8 * (w & 1) + (w >> 1)
        x[:, :, w, :] = (o[hi].astype(np.uint64) << np.uint64(32)) | o[hi + 4].astype(np.uint64)
    x = x.reshape(S, G8 * 8, D)[:, :B]
    return x, _rejected(x, m)


def retry_attempt(key, streams, b, d, T, m, attempt, rounds=20):
    """one retry attempt of the draws (stream, batch b, draw or pair d), arrays of equal length: counter b D + d, the attempt in
    the top byte of word 15, candidates (o[2 j] << 32) | o[2 j + 1].  -> rejected [len][8]"""
    D = draws_per_batch(T, m)
    ctr = np.asarray(b, dtype=np.uint64) * np.uint64(D) + np.asarray(d, dtype=np.uint64)
    o = chacha_words(key, ctr, streams, attempt, rounds)
    x = (o[0::2].astype(np.uint64) << np.uint64(32)) | o[1::2].astype(np.uint64)          # [8][len]
    return _rejected(x.T, m)


def retry_depth(key, stream, b, d, T, m, rounds=20):
    """(attempt, candidate index) that finally serves draw (pair) d of batch b; (0, 0) = the first attempt was accepted"""
    if not first_attempt(key, [stream], b + 1, T, m, rounds)[1][0, b, d]:
        return 0, 0
    for a in range(1, 256):
        rej = retry_attempt(key, [stream], [b], [d], T, m, a, rounds)[0]
        if not rej.all():
            return a, int(np.flatnonzero(~rej)[0])
    raise AssertionError("255 attempts rejected")


# ---- the 0.2-rate cases ---------------------------------------------------------------------------------------------------------
def coverage(rej):
    """what the reach test asserts of a 0.2-rate case, from rejected [participants][B][D]: (rejected draws, positions b & 7 hit,
    draw indices hit, rejections in the last group of 8, rejections of participants other than the first)"""
    P, B, D = rej.shape
    b = np.arange(B)
    pos = {int(w) for w in np.unique(b[rej.any(axis=(0, 2))] & 7)}
    idx = {int(i) for i in np.flatnonzero(rej.any(axis=(0, 1)))}
    return int(rej.sum()), pos, idx, int(rej[:, (B - 1) // 8 * 8:].sum()), int(rej[1:].sum())


def covered(rej):
    P, B, D = rej.shape
    count, pos, idx, last, others = coverage(rej)
    return count >= 20 and pos == set(range(min(B, 8))) and idx == set(range(D)) and last >= 1 and others >= 1


def smallest_batches(key, streams, T, m, rounds=20, limit=1025):
    """the smallest odd batch count (>= 9: more than one group) at which `covered` holds for these streams"""
    _, rej = first_attempt(key, streams, limit, T, m, rounds)
    for B in range(9, limit + 1, 2):
        if covered(rej[:, :B]):
            return B
    raise AssertionError("no batch count up to the limit covers the retry path")


def smallest_participants(key, first, B, T, m, rounds=20, limit=64):
    """for a job whose batch count is given: the smallest participant count (>= PARTICIPANTS) at which `covered` holds for the
    streams first, first + 1, .."""
    _, rej = first_attempt(key, [first + q for q in range(limit)], B, T, m, rounds)
    for P in range(PARTICIPANTS, limit + 1):
        if covered(rej[:P]):
            return P
    raise AssertionError("no participant count up to the limit covers the retry path")


def case_streams(case):
    """the stream ids a case draws from: participants first .. first + P - 1 of every tile"""
    return [case["first"] + i for i in range(case["participants"] * case.get("tiles", 1))]


def _case(name, kernel, k, t, n, prime, B, knobs=(), first=FIRST, odd=False, fixed=False, participants=PARTICIPANTS, **kw):
    """name; substring of sda_debug_last_kernel(); the shape; the modulus; batches; knobs; first participant; odd output row
    stride; fixed = the batch count is given and the PARTICIPANT count is the smallest covering one instead (the two largest
    transform shapes: a batch is 2187 or 19683 points in LDS and seconds of the oracle's time, so their jobs keep to three
    batches - positions b & 7 = 0 .. 2 are then all there are - and take as many participants as it needs for every one of the
    155 draw indices to be rejected at least once)"""
    return dict(name=name, kernel=kernel, k=k, t=t, n=n, p=prime, B=B, knobs=tuple(knobs), first=first, odd=odd, fixed=fixed, T=t,
                participants=participants, **kw)


# matrix families over PM, family selection and knobs as in extremes.GPU_CASES (sda_kernels.hip: drbg_pair + drbg_retry)
MATRIX_CASES = [
    _case("mfma-compiled", "packed_gen_mfma_kernel<12, 3, 20>", 12, 3, 26, PM, 11, odd=True),
    _case("mfma-forced", "packed_gen_mfma_kernel<8, 7, 20>", 8, 7, 26, PM, 9, knobs=["SDA_FORCE_MFMA"]),
    _case("mfma-runtime", "packed_gen_mfma_kernel<0, 0, 20>", 9, 6, 26, PM, 9, first=FIRST_LAST),
    _case("l31-two-digit", "packed_gen_l31_kernel<3, 1, 20", 3, 1, 8, PM, 29, odd=True),
    _case("l31-three-digit", "packed_gen_l31_kernel<8, 7, 20", 8, 7, 26, PM, 9),
    _case("l31-runtime", "packed_gen_l31_rt_kernel<8, 20>", 6, 2, 8, PM, 15),
    _case("l31-global", "packed_gen_l31_rtg_kernel<", 20, 13, 80, PM, 9, odd=True),
    _case("mont64", "packed_gen_kernel<3, 1, 20", 3, 1, 8, PM, 29, knobs=["SDA_FORCE_MONT64"], odd=True),
    # the any-shape kernel takes injected draws: the library materialises them first with drbg_fill_kernel
    _case("generic+drbg_fill", "packed_gen_generic_kernel", 3, 1, 8, PM, 29, knobs=["SDA_FORCE_GENERIC"], odd=True),
]

# dual-role forms (generate_combine_dev, two tiles of PARTICIPANTS): streams first .. first + 2 P - 1
DUAL_CASES = [
    _case("dual-l31", "fused_packed_l31_kernel<3, 1, 20>", 3, 1, 8, PM, 17, tiles=2),
    _case("dual-mfma", "fused_packed_mfma_kernel<12, 3, 20>", 12, 3, 26, PM, 9, tiles=2),
    _case("dual-additive", "fused_additive_kernel<20>", 1, 2, 3, PM, 9, tiles=2, additive=True),
    _case("side-stream-transform", "combine_update_walk_kernel (side stream)", 3, 4, 8, WIDE_PRIMES["fft8"][0], 9, knobs=["SDA_FORCE_FFT"], tiles=2),
]

# the transform kernel (fft_kernels.hip): its G >= 8 branch ((b_first + 8 nb + jj) t + i) and, with fewer batches per workgroup,
# its G = 1, 2, 4 branch ((b_first + jj) t + i, word pairs from off = b_first & 7 on).  The library picks G from the LDS a group
# needs (fft_shape, sda_capi.cpp): 8 for the wide (40, 23, 242) and (100, 155, 728), 4 for (100, 155, 2186) - three batches are one
# workgroup at off = 0 - and 1 for (100, 155, 19682), off = 0 .. 2.  The non-zero offsets of G = 4 and G = 2 and off = 3 .. 7 of
# G = 1 come from the knob SDA_FFT_G alone (snapshotted when the generator is created, so _knobs() runs first).  NOT OBSERVABLE
# on the device: sda_debug_last_kernel() does not report G, so a knob that was ignored would leave the G4 / G2 / G1 cases passing
# on the G = 8 branch.  On the host sda_debug_select_path reports the plan ("SDA_FFT_G=4" -> transform_g=4);
# tests/test_transform_limits_reach.py pins it for every group form.
_F8, _F242 = WIDE_PRIMES["fft8"][0], WIDE_PRIMES["fft242"][0]
FFT_CASES = [
    _case("fft-1-6-8", "packed_gen_fft_kernel<20, ", 1, 6, 8, _F8, 9, knobs=["SDA_FORCE_FFT"], odd=True),
    _case("fft-3-4-8", "packed_gen_fft_kernel<20, ", 3, 4, 8, _F8, 13, knobs=["SDA_FORCE_FFT"], first=FIRST_LAST),
    _case("fft-40-23-242", "packed_gen_fft_kernel<20, ", 40, 23, 242, _F242, 9),
    *[_case(f"fft-40-23-242-G{g}", "packed_gen_fft_kernel<20, ", 40, 23, 242, _F242, 9, knobs=[("SDA_FFT_G", g)]) for g in (4, 2, 1)],
    *[_case(f"fft-40-23-242-chacha{r}", f"packed_gen_fft_kernel<{r}, ", 40, 23, 242, _F242, b, rounds=r) for r, b in ((12, 13), (8, 17))],
    _case("fft-100-155-728", "packed_gen_fft_kernel<20, ", 100, 155, 728, WIDE_PRIMES["fft728"][0], 9),
    _case("fft-100-155-2186", "packed_gen_fft_kernel<20, ", 100, 155, 2186, WIDE_PRIMES["fft2186"][0], 3, fixed=True, participants=9),
    _case("fft-100-155-19682", "packed_gen_fft_kernel<20, ", 100, 155, 19682, WIDE_PRIMES["fft19682"][0], 3, fixed=True, participants=7),
]

# additive sharing (T = n - 1 draws per element), the signed value mode, the full mask (T = 1, one draw per element) - one
# "batch" is one element here
ADDITIVE_CASES = [
    _case("additive-n3", "additive_gen_kernel<20, ", 1, 2, 3, PM, 15, additive=True, odd=True),
    _case("additive-n2", "additive_gen_kernel<20, ", 1, 1, 2, PM, 25, additive=True, first=FIRST_LAST),
    _case("additive-signed", "signed_additive_gen_drbg_kernel<20>", 1, 3, 4, PM, 11, additive=True, signed=True),
]
MASK_CASES = [
    _case("full-mask-aligned", None, 1, 1, 1, PM, 29, mask=True),                  # even strides: the 16-byte path
    _case("full-mask-odd", None, 1, 1, 1, PM, 29, mask=True, odd=True),            # odd stride, odd dim: the scalar path
]
WIDE_CASES = MATRIX_CASES + DUAL_CASES + FFT_CASES + ADDITIVE_CASES + MASK_CASES


def case_rejections(case):
    """rejected [streams][B][D] of a case's first attempts"""
    return first_attempt(KEY, case_streams(case), case["B"], case["T"], case["p"], case.get("rounds", 20))[1]


# ---- the paired rule: located rejections ----------------------------------------------------------------------------------------
PAIRED_START = (0x5EED << 32) | 0x10000000      # the search starts here (stream ids with a non-zero top part) and goes upward
PAIRED_BATCHES = 1024
PAIRED_COUNT = 3                                # streams per (prime, T)


def locate_paired(m, T, count=PAIRED_COUNT, start=PAIRED_START, batches=PAIRED_BATCHES, chunk=256, limit=1 << 14):
    """the first `count` streams >= start whose first `batches` batches hold a rejected pair, and for an odd T one more - the
    next whose rejected pair is the LAST of its batch (the pair whose second element is discarded) - unless one of the first
    has it: [(stream, [(batch, pair), ..]), ..]"""
    out, last = [], (T + 1) // 2 - 1
    for s0 in range(start, start + limit, chunk):
        _, rej = first_attempt(KEY, np.arange(s0, s0 + chunk, dtype=np.uint64), batches, T, m)
        for s in np.flatnonzero(rej.any(axis=(1, 2))):
            pairs = [(int(b), int(j)) for b, j in np.argwhere(rej[s])]
            if len(out) < count or any(j == last for _, j in pairs):
                out.append((s0 + int(s), pairs))
            if len(out) >= count and (T % 2 == 0 or any(j == last for _, ps in out for _, j in ps)):
                return out
    raise AssertionError("the search range holds too few rejected pairs")


_Q8, _Q242, _QANY = PAIRED_PRIMES["fft8"][0], PAIRED_PRIMES["fft242"][0], PAIRED_PRIMES["any"][0]
# (prime, T) -> what locate_paired finds (tests/test_drbg_retry_reach.py re-derives it): stream, its rejected (batch, pair)s
PAIRED_HITS = {
    (_Q8, 4): [(104372268695574, [(355, 0)]), (104372268695640, [(332, 1)]), (104372268695737, [(340, 1)])],
    (_Q242, 23): [(104372268695567, [(894, 1)]), (104372268695579, [(200, 7)]), (104372268695587, [(13, 0)]), (104372268695868, [(470, 11)])],
    (_QANY, 7): [(104372268695710, [(560, 0)]), (104372268695817, [(601, 3)]), (104372268695824, [(979, 2)])],
}

# the transform kernel's paired branch ((b_first + bl) t2 + j; narrow values, lazy and reduced radix-3 levels, the limb GEMM
# switched off) and the one-limb kernels, which draw through drbg_pair / drbg_retry_pair
PAIRED_CASES = [
    dict(name="fft-paired-3-4-8-lazy", kernel="unsigned int, true>", k=3, t=4, n=8, p=_Q8, knobs=("SDA_FORCE_FFT", "SDA_NO_NGEMM")),
    dict(name="fft-paired-3-4-8-reduced", kernel="unsigned int, false>", k=3, t=4, n=8, p=_Q8, knobs=("SDA_FORCE_FFT", "SDA_NO_NGEMM", "SDA_NO_LAZY")),
    dict(name="fft-paired-40-23-242-lazy", kernel="unsigned int, true>", k=40, t=23, n=242, p=_Q242, knobs=("SDA_NO_NGEMM",)),
    dict(name="fft-paired-40-23-242-reduced", kernel="unsigned int, false>", k=40, t=23, n=242, p=_Q242, knobs=("SDA_NO_NGEMM", "SDA_NO_LAZY")),
    dict(name="n31-paired-3-4-8", kernel="packed_gen_n31_kernel<8, ", k=3, t=4, n=8, p=_Q8, knobs=()),
    dict(name="n31-paired-8-7-26", kernel="packed_gen_n31_kernel<16, ", k=8, t=7, n=26, p=_QANY, knobs=()),
]


def located_job(stream, batch):
    """(first participant, batches) of the small job around a located draw: the stream is participant 1 of PARTICIPANTS, the
    batch count the smallest odd one that holds the batch"""
    return stream - 1, (batch + 1) | 1


def paired_jobs(case):
    """[(first participant, batches, stream, [(batch, pair), ..]), ..]: one job per located stream of the case's prime and T"""
    return [located_job(s, max(b for b, _ in pairs)) + (s, pairs) for s, pairs in PAIRED_HITS[(case["p"], case["t"])]]


# ---- second candidate, second attempt --------------------------------------------------------------------------------------------
DEEP_START = (0xD1CE << 32) | 0x20000000
DEEP_BATCHES = 4096


def locate_second_attempt(m, T, start=DEEP_START, batches=DEEP_BATCHES, chunk=64, limit=1 << 13):
    """the first stream >= start whose first `batches` batches hold a draw whose eight candidates of attempt 1 are all rejected:
    -> (stream, batch, draw index, draws scanned)"""
    scanned = 0
    for s0 in range(start, start + limit, chunk):
        streams = np.arange(s0, s0 + chunk, dtype=np.uint64)
        _, rej = first_attempt(KEY, streams, batches, T, m)
        scanned += rej.size
        s, b, i = np.nonzero(rej)
        deep = retry_attempt(KEY, streams[s], b, i, T, m, 1).all(axis=1)
        if deep.any():
            j = int(np.flatnonzero(deep)[0])
            return int(streams[s[j]]), int(b[j]), int(i[j]), scanned
    raise AssertionError("the search range holds no draw that needs a second attempt")


# the draws (per batch) depend on T, so each of the two kernels has a stream of its own: what locate_second_attempt finds for
# its modulus and T, as (stream, batch, draw index)
DEEP_CASES = [
    dict(name="deep-additive", kernel="additive_gen_kernel<20, ", k=1, t=2, n=3, p=PM, knobs=(), additive=True, hit=(230683230339077, 1700, 0)),
    dict(name="deep-fft-1-6-8", kernel="packed_gen_fft_kernel<20, ", k=1, t=6, n=8, p=_F8, knobs=("SDA_FORCE_FFT",), hit=(230683230339095, 2019, 5)),
]


# ---- the limb GEMM's volume test (tests/test_ngemm_gpu.py): reach only ---------------------------------------------------------
# its parameters (that test takes them from here, so the reach check and the job cannot drift apart).
# packed_gen_ngemm_kernel<1, 4> = 512 batches per workgroup (the workgroup's first batch is a multiple of 512), 512 worker lanes;
# a lane's round-th block is unit u = lane + 512 round of the workgroup's (512 / 8) cp blocks (cp = ceil(t / 2) pairs), block
# group nb = u / cp, pair u % cp; bit 8 round + (b & 7) of the lane's 64-bit mask `rej` marks a rejected pair (ng_draw_pass /
# ng_draw_fixup, ngemm_kernels.hip)
NGEMM_VOLUME = dict(key=KEY, p=8211457, k=40, t=23, n=242, participants=2, batches=500_000, first=5, wgb=512, workers=512)


def ngemm_rej_bit(b, j, t, wgb=512, workers=512):
    """bit index of rejected pair j of batch b in its lane's mask"""
    cp = (t + 1) // 2
    u = ((b % wgb) >> 3) * cp + j
    return 8 * (u // workers) + (b & 7)

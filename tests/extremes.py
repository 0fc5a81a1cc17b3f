"""Crafted operands for the share-generation kernels at their operand and modulus limits (shared by tests/test_mfma_model.py,
tests/test_extremes_reach.py and tests/test_extremes_gpu.py - a helper module, not a conftest).

For a family and a scheme this module restates the constants the kernel holds (the host's preparation in sda_capi.cpp:
mfma_place_matrix, n31_place_matrix, build_ngemm_plan, l31_pack_matrix) and builds injected secrets and draws that push that
family's intermediates to their bounds:
  * sign-aligned with a target output row: every term's centred value is +-(p - 1)/2 with the sign of the constant the kernel
    multiplies it by (and the opposite batch, all signs flipped);
  * extreme digits / limbs: balanced bytes at -128 / 127 aligned with the constant's digits of one target column (mfma, ngemm),
    balanced 31-bit limbs at +-2^30 aligned with the constant's limbs (l31), the n31 limb at +-(p - 1)/2 (= sign-aligned);
  * unsigned extremes: every value the canonical p - 1 (the generic and 64-bit Montgomery kernels sum canonical products);
  * every row covered: the target row (and column) cycles across batches, so every output row gets its worst batch.
It also holds the big-int model of the 62-bit limb GEMM (packed_gen_mfma_kernel, sda_kernels.hip) that the model test and the
reach checks run, and small models of the n31 group sums and the narrow limb GEMM's columns for the reach checks."""
import numpy as np

P62 = 4611686006577364993
PMAX = (1 << 62) - 57            # the largest modulus the library admits (ModParams.m < 2^62)
P31MAX = (1 << 31) - 1           # the largest n31 prime
P29_BELOW, P29_ABOVE = 536870909, 536870923      # the primes on either side of 2^29 (n31: 16 / 4 terms per reduction)
NGEMM_PMAX = 8355691             # the largest prime the narrow limb GEMM takes (p <= 0x7F7F7F)
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
BIAS64 = 0x8080808080808080


def centred(v, p):
    """canonical residue -> (-p/2, p/2] (the kernels' `v > p >> 1 ? v - p : v`)"""
    return v - p if v > p >> 1 else v


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def balanced_digits(x, count=8):
    """balanced base-256 digits of a two's-complement value: the bytes of (x + 0x8080..80) ^ 0x8080..80, each in [-128, 127]"""
    y = ((x + BIAS64) & M64) ^ BIAS64
    d = [(y >> (8 * i)) & 0xFF for i in range(8)]
    d = [b - 256 if b >= 128 else b for b in d]
    return d[:count]


def digit_range(p):
    """max |balanced digit i| over the centred residues of p (both the constants and the values of the 62-bit limb GEMM)"""
    h = (p - 1) // 2
    out = []
    for i in range(8):
        if 128 * ((1 << (8 * (i + 1))) - 1) // 255 <= h:       # every digit 0..i can be -128
            out.append(128)
        else:                                                   # the top digit: monotone in x, extremes at +-h
            out.append(max(abs(balanced_digits(h)[i]), abs(balanced_digits(-h)[i])))
    return out


def omegas(p, k, t, n):
    """arbitrary omegas with distinct nodes (all the library requires): w2^0..w2^(k+t) and w3^1..w3^n pairwise distinct.  Drawn
    from a fixed pseudo-random sequence rather than 2 and 3: small omegas give small Lagrange coefficients (at 2^31 - 1 even the
    Montgomery factor 2^32 is 2), and constants far below p / 2 would keep every dot product far from its bound"""
    cand = [x % (p - 3) + 2 for x in ((i + 1) * 0x9E3779B97F4A7C15 for i in range(64))]
    for w2 in cand:
        nodes = [pow(w2, e, p) for e in range(k + t + 1)]
        if len(set(nodes)) < len(nodes):
            continue
        for w3 in cand:
            pts = [pow(w3, j + 1, p) for j in range(n)]
            if w3 != w2 and len(set(pts) | set(nodes)) == len(pts) + len(nodes):
                return w2, w3
    raise ValueError(f"no omegas with distinct nodes for p = {p}, k + t = {k + t}, n = {n}")


def share_matrix(p, k, t, n, w2, w3, systematic=False):
    """the plain share matrix (python ints): tss's map, n x (k + t); the systematic one (the device CSPRNG's default, draws =
    shares 0..t-1), (n - t) x (k + t) - read off the oracle with unit vectors"""
    from oracle import coracle
    if not systematic:
        return [[int(x) for x in row] for row in coracle.packed_share_matrix(p, k, t, n, w2, w3)]
    kt = k + t
    sec = np.zeros(kt * k, dtype=np.int64)
    dr = np.zeros(kt * t, dtype=np.int64)
    for b in range(kt):
        if b < k:
            sec[b * k + b] = 1
        else:
            dr[b * t + b - k] = 1
    out = coracle.packed_generate_systematic(p, k, t, n, w2, w3, sec, dr)
    return [[int(out[j][b]) for b in range(kt)] for j in range(t, n)]


# the Montgomery radix of each family's constants (the host multiplies the plain matrix by R mod p); limb-31: l31_radix
RADIX_BITS = {"mfma": 64, "generic": 64, "mont64": 64, "n31": 32, "ngemm": 0}
L31_THREE_DIGIT_COMPILED = {(3, 4), (8, 2), (8, 7)}          # L31UseR93 (sda_kernels.hip)


def l31_radix(family, k, t):
    """the radix 2^bits of the limb-31 constants, as l31_place_matrix picks it: packed_l31_r_bits for the kernarg kernels (the
    compiled three-digit shapes 93, every other compiled or run-time shape of <= 16 terms 62), packed_l31_rt_r_bits for the
    global-matrix form (93 from 17 terms on).  tests/test_extremes_reach.py checks it against the library's own choice."""
    kt = k + t
    if family == "l31" and (k, t) in L31_THREE_DIGIT_COMPILED:
        return 93
    return 93 if kt > 16 else 62


def family_constants(family, M, p, k=None, t=None):
    """centred constants the kernel multiplies each term by: M R mod p (limb-31 families: R from l31_radix(family, k, t))"""
    bits = l31_radix(family, k, t) if family.startswith("l31") else RADIX_BITS[family]
    r = pow(2, bits, p)
    return [[centred(m * r % p, p) for m in row] for row in M]


def l31_limbs(c):
    """l31_pack_matrix / the kernels' value split: c = m1 2^31 + m0, m0 in [-2^30, 2^30)"""
    m0 = c & ((1 << 31) - 1)
    if m0 >= 1 << 30:
        m0 -= 1 << 31
    return (c - m0) >> 31, m0


def _sgn(x):
    return -1 if x < 0 else 1


def _mfma_digit_value(consts, c, p):
    """a centred value per term whose balanced digits are -128 / 127 with the sign of constant digit c - l (column c as large
    as the digit ranges allow), digits that would leave (-p/2, p/2] dropped"""
    h = (p - 1) // 2
    out = []
    for m in consts:
        dm = balanced_digits(m)
        v = 0
        for l in range(8):
            if 0 <= c - l <= 7 and dm[c - l] != 0:
                d = 127 if dm[c - l] > 0 else -128
                if abs(v + d * 256 ** l) <= h:
                    v += d * 256 ** l
        out.append(v)
    return out


def _ngemm_digit_value(consts, c, p):
    """the narrow limb GEMM's values are canonical residues (not centred): digits aligned with constant digit c - l where the
    residue stays in [0, p)"""
    out = []
    for m in consts:
        dm = ngemm_digits(m)
        want = [0, 0, 0]
        for l in range(3):
            if 0 <= c - l <= 2 and dm[c - l] != 0:
                want[l] = 127 if dm[c - l] > 0 else -128
        low = want[0] + 256 * want[1]
        for d2 in ([want[2]] if want[2] else []) + [127, 126, 125, 64, 1, 0]:
            v = low + 65536 * d2
            if 0 <= v < p:
                break
        else:
            v = 0
        out.append(v)
    return out


def _l31_limb_value(consts, p):
    """balanced 31-bit limbs at +-2^30 with the signs of the constant's limbs (the top limb one short: |value| <= (p-1)/2)"""
    h = (p - 1) // 2
    out = []
    for m in consts:
        m1, m0 = l31_limbs(m)
        v = _sgn(m1) * ((1 << 30) - 1) * (1 << 31) + (-(1 << 30) if m0 < 0 else (1 << 30) - 1)
        while abs(v) > h:           # small primes: only the low limb
            v = -(1 << 30) if m0 < 0 else (1 << 30) - 1
            if abs(v) > h:
                v = _sgn(m0) * h
        out.append(v)
    return out


NPAT = 7


def target(family, b, rows):
    """(pattern, target row, target column) of batch b: rows and columns cycle together, so every row meets many columns"""
    return b % NPAT, (b // NPAT) % rows, (b // NPAT) % {"mfma": 15, "ngemm": 5}.get(family, 1)


def crafted_rows(family, C, p, batches, first_term=0, nterms=None):
    """[batches][terms] centred values: patterns in turn (sign-aligned, sign-opposed, digit / limb-extreme aligned and its
    negation, all (p-1)/2, all -(p-1)/2, all -1 = the canonical p - 1 that maximises the unsigned sums of the generic and
    64-bit Montgomery kernels), the target row and column (mfma: 15, ngemm: 5) cycling across batches.  C: centred constants
    [rows][k + t]; the values cover terms first_term .. + nterms."""
    rows = len(C)
    kt = len(C[0])
    nterms = kt - first_term if nterms is None else nterms
    h = (p - 1) // 2
    out = []
    cache = {}
    for b in range(batches):
        pat, r, col = target(family, b, rows)
        consts = C[r][first_term:first_term + nterms]
        if pat in (0, 1):
            s = 1 if pat == 0 else -1
            v = [s * _sgn(m) * h for m in consts]
        elif pat in (2, 3):
            key = (r, col)
            if key not in cache:
                if family == "mfma":
                    cache[key] = _mfma_digit_value(consts, col, p)
                elif family == "ngemm":
                    cache[key] = [centred(x, p) for x in _ngemm_digit_value(consts, col, p)]
                elif family.startswith("l31"):
                    cache[key] = _l31_limb_value(consts, p)
                else:
                    cache[key] = [_sgn(m) * h for m in consts]
            v = cache[key] if pat == 2 else [-x for x in cache[key]]
        else:
            v = [h if pat == 4 else -h if pat == 5 else -1] * nterms
        out.append(v)
    return out


def crafted_operands(family, p, k, t, n, w2, w3, batches, systematic=False):
    """(secrets [batches * k], draws [batches * t]) as canonical int64 residues, crafted against the constants of the share map
    the call uses: tss's (injected draws) or the systematic one (device CSPRNG: only the secrets are ours)"""
    M = share_matrix(p, k, t, n, w2, w3, systematic)
    C = ngemm_constants(M, p) if family == "ngemm" else family_constants(family, M, p, k, t)
    vals = crafted_rows(family, C, p, batches, 0, k if systematic else k + t)
    sec = np.array([x % p for v in vals for x in v[:k]], dtype=np.int64)
    dr = np.array([x % p for v in vals for x in v[k:]], dtype=np.int64) if not systematic else None
    return sec, dr


# the cases of tests/test_extremes_gpu.py (the reach checks run the same table on the CPU)
# (family, k, t, n, p, knobs, batches, odd row stride)
GPU_CASES = [
    # the 62-bit limb GEMM: compiled shapes by default and forced, the largest constant table, the small primes with the n31
    # overlay switched off; the run-time (k, t) form
    *[("mfma", k, t, 26, p, (), 2340, odd) for p in (P62, PMAX) for (k, t), odd in (((12, 3), p == PMAX), ((10, 5), False), ((4, 11), False))],
    *[("mfma", k, t, n, p, ("SDA_FORCE_MFMA",), 2340, False) for p in (P62, PMAX) for k, t, n in ((8, 7, 26), (3, 1, 8))],
    ("mfma", 8, 7, 242, PMAX, ("SDA_FORCE_MFMA",), 1500, False),
    *[("mfma", 12, 3, 26, p, ("SDA_NO_NARROW",), 2340, False) for p in (433, P31MAX)],
    *[("mfma", k, t, 26, PMAX, (), 2340, False) for k, t in ((9, 6), (13, 2), (1, 14), (16, 0))],
    # limb-31: two-digit compiled and run-time, three-digit / Karatsuba
    *[("l31", k, t, n, PMAX, (), 1000, (k, t) == (4, 3)) for k, t, n in ((3, 1, 8), (4, 3, 8), (6, 2, 8), (5, 4, 26), (8, 2, 26), (8, 7, 26))],
    # matrix in global memory, the any-shape kernel, the 64-bit Montgomery kernel (forced) and the any-shape kernel forced
    ("l31_global", 20, 13, 80, PMAX, (), 1000, True),
    ("generic", 40, 30, 100, PMAX, (), 1000, True),
    *[("mont64", k, t, n, PMAX, ("SDA_FORCE_MONT64",), 1000, k == 3) for k, t, n in ((3, 1, 8), (8, 2, 26))],
    *[("generic", k, t, n, PMAX, ("SDA_FORCE_GENERIC",), 1000, False) for k, t, n in ((3, 1, 8), (8, 2, 26))],
    # one 32-bit limb: KTMAX 4 / 8 / 12 / 16 at 2^31 - 1 and on either side of 2^29
    *[("n31", k, t, n, p, (), 1000, (k, t) == (3, 4)) for p in (P31MAX, P29_ABOVE, P29_BELOW)
      for k, t, n in ((1, 1, 2), (3, 4, 8), (5, 4, 26), (8, 7, 26))],
    # the narrow limb GEMM at the largest prime it takes: KS 1 / 2 / 8
    ("ngemm", 20, 13, 50, NGEMM_PMAX, (), 1000, True),
    ("ngemm", 70, 57, 242, NGEMM_PMAX, (), 600, False),
    ("ngemm", 300, 211, 728, NGEMM_PMAX, (), 200, False),
]

# ---- the 62-bit limb GEMM (packed_gen_mfma_kernel / fused_packed_mfma_kernel) ----------------------------------------------------
def mfma_place_row(row_mont, p):
    """mfma_place_matrix for one row: Montgomery form (R = 2^64), centred, balanced bytes, zero padded to 8 ceil((k+t)/8)"""
    kt = len(row_mont)
    width = 8 * ((kt + 7) // 8)
    tab = []
    for i in range(width):
        if i < kt:
            m = row_mont[i]
            if m > p >> 1:
                m -= p
            tab.append(((m + BIAS64) & M64) ^ BIAS64)
        else:
            tab.append(0)
    return tab


def mfma_share(row_plain, values, p, stats=None):
    """one share the way the limb-GEMM kernel forms it: values canonical [0, p) of k + t terms, row_plain the plain matrix row;
    every register is checked against its width and every range the kernel's comments state.  Returns the canonical share;
    `stats` (a dict) collects the largest |column| and |X| seen."""
    kt = len(row_plain)
    assert kt <= 16 and len(values) == kt
    KS = (kt + 7) // 8
    tab = mfma_place_row([m * (1 << 64) % p for m in row_plain], p)
    dM = [[b - 256 if b >= 128 else b for b in ((w >> (8 * i)) & 0xFF for i in range(8))] for w in tab]
    # values: canon_i64 -> centred -> balanced_bytes, zero padding beyond k + t (the LDS tile starts zeroed)
    dV = [balanced_digits(centred(v, p)) for v in values] + [[0] * 8] * (8 * KS - kt)
    # 15 Toeplitz columns, 16 rows of the A operand (row 15 is all zero): i8 x i8 products accumulated in i32 over KS steps
    col = [0] * 16
    for ks in range(KS):
        for c in range(16):
            for g in range(4):
                for b in range(16):                        # slot (g, b): term 8 ks + 2 g + b / 8, value byte l' = b % 8
                    term, l = 8 * ks + 2 * g + b // 8, b % 8
                    a = dM[term][c - l] if 0 <= c - l <= 7 else 0
                    assert -128 <= a <= 127 and -128 <= dV[term][l] <= 127
                    col[c] += a * dV[term][l]
            assert -(1 << 31) <= col[c] < (1 << 31)        # the i32 accumulator after every MFMA step
    assert col[15] == 0                                    # column 15 does not exist: mul3 = 0 drops nothing
    bound = column_bound(kt, p)
    for c in range(15):
        assert abs(col[c]) <= bound <= 1 << 21             # |column| < 2^21 (sda_kernels.hip): the digit ranges give <= `bound`
    # per tile: pa = col[4g] + col[4g+1] 2^8 + col[4g+2] 2^16 + col[4g+3] mul3, three v_mad_i64_i32 (i32 x i32 + i64)
    pa = []
    for g in range(4):
        mul3 = 0 if g == 3 else 1 << 24
        x = col[4 * g]
        for c, w in ((4 * g + 1, 1 << 8), (4 * g + 2, 1 << 16), (4 * g + 3, mul3)):
            assert -(1 << 31) <= col[c] < (1 << 31) and -(1 << 31) <= w < (1 << 31)
            x = col[c] * w + x
            assert -(1 << 63) <= x < (1 << 63)
        pa.append(x)
    lo = [x & M32 for x in pa]
    hi = [(x >> 32) & M32 for x in pa]
    # the 128-bit assembly exactly as written
    q0 = (hi[0] << 32) | lo[0]
    xlo = (q0 + (lo[1] << 32)) & M64
    carry = 1 if xlo < q0 else 0
    parts = [s32(hi[0]) >> 31, s32(hi[1]), carry, s64((hi[2] << 32) | lo[2]), s64((lo[3] << 32) & M64)]
    exact = sum(parts)
    xhi = s64(exact)
    X = sum(x << (32 * g) for g, x in enumerate(pa))
    dot = sum(centred(m * (1 << 64) % p, p) * centred(v, p) for m, v in zip(row_plain, values))
    assert X == dot                                        # the columns are exact
    assert X == (xhi << 64) + xlo                          # hi[3] dropped, q0 sign-extended, the xlo < q0 carry
    assert abs(X) <= kt * ((p - 1) // 2) ** 2 <= 4 * (p - 1) ** 2 < p << 64      # |X| <= 4 p^2 < p 2^64
    # signed REDC (R = 2^64): the quotient lies in [-p, 2p)
    pinv = (-pow(p, -1, 1 << 64)) & M64
    m = xlo * pinv & M64
    tq = xhi + ((m * p) >> 64) + (1 if xlo != 0 else 0)
    assert -(1 << 63) <= tq < (1 << 63)
    assert (tq << 64) == X + m * p and -p <= tq < 2 * p
    if tq < 0:
        tq += p
    share = tq - p if tq >= p else tq
    assert share == sum(a * v for a, v in zip(row_plain, values)) % p
    if stats is not None:
        stats["col"] = max(stats.get("col", 0), max(abs(c) for c in col))
        stats["X"] = max(stats.get("X", 0), abs(X))
    return share


def column_bound(kt, p):
    """the largest |column| the digit ranges of p allow at kt terms: kt max_c sum_{i + l = c} |d_i|max |d_l|max"""
    r = digit_range(p)
    return kt * max(sum(r[i] * r[c - i] for i in range(8) if 0 <= c - i <= 7) for c in range(15))


# ---- the one-limb kernels (n31, narrow_gen.inc.hpp): GROUP terms per signed 64-bit sum ----------------------------------------------
def n31_group(p):
    return 16 if p < (1 << 29) else 4


def n31_group_sums(C, vals, p):
    """the group sums S of one row (C: n31 constants, vals: centred values): every |S| < 2^62 (n31_redc's operand)"""
    G = n31_group(p)
    out = []
    for g0 in range(0, len(C), G):
        S = sum(m * v for m, v in zip(C[g0:g0 + G], vals[g0:g0 + G]))
        assert abs(S) < 1 << 62
        out.append((S, len(C[g0:g0 + G])))
    return out


# ---- the narrow limb GEMM (ngemm_kernels.hip): plain matrix, three balanced digits ----------------------------------------------------
def ngemm_constants(M, p):
    """build_ngemm_plan: the plain matrix, centred"""
    return [[centred(m, p) for m in row] for row in M]


def ngemm_digits(x):
    y = ((x + 0x00808080) & M32) ^ 0x00808080
    d = [(y >> (8 * i)) & 0xFF for i in range(3)]
    return [b - 256 if b >= 128 else b for b in d]


def ngemm_columns(C, vals, p):
    """the five column sums of one share and the merged top column C_3 + 256 C_4 (values: canonical residues' digits)"""
    col = [0] * 5
    for m, v in zip(C, vals):
        dm, dv = ngemm_digits(m), ngemm_digits(v % p)
        for a in range(3):
            for b in range(3):
                col[a + b] += dm[a] * dv[b]
    top = col[3] + 256 * col[4]
    assert all(-(1 << 31) <= c < (1 << 31) for c in col) and -(1 << 31) <= top < (1 << 31)
    return col, top

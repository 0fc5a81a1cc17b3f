// The per-batch Reed-Solomon decoder of the reconstructor's decoded finish (reveal_decode_finish_kernel, sda_kernels.hip): from
// the c = checks syndromes S_d = sum_{i in E} Y_i x_i^d of one batch to the error positions E and magnitudes Y, for |E| <= cap <=
// floor(c / 2).  Host + device: the kernel runs it one lane per batch, tests/cpp/reveal_decode_host.cpp runs it on the CPU.
//
// Number forms.  S is canonical, the points xs are in Montgomery form, and every product is ONE REDC: mm(a, b) = a b / 2^64.  A
// product with a point is therefore exact, a product of two canonical numbers carries a factor 2^-64.  Berlekamp-Massey without
// inversions only ever needs its polynomial up to a non-zero factor, and both terms of its update b C - d x^m B pick up the same
// 2^-64, as do the discrepancies d and b against each other - so the factors are left in.  They cancel in Y = num / den below.
//
// No array is indexed by a run-time value: the polynomials (9 coefficients: degree <= 8 = floor(16 / 2)) are walked by unrolled
// loops, x^m B is kept shifted (one compile-time shift per step) and the syndromes rotate through S[0] - sixteen rotations bring
// them back.  The located positions go through `pos` (LDS in the kernel).
#pragma once
#include <stddef.h>

#include "modarith.hpp"

namespace sda {

static constexpr int kDecodeChecks = 16;                   // SDA_RECONSTRUCT_MAX_CHECKS
static constexpr int kDecodeErrors = kDecodeChecks / 2;    // the most positions a batch can be decoded with

SDA_HD uint64_t dec_mm(uint64_t a, uint64_t b, uint64_t p, uint64_t pinv) { return mont_redc(mul64x64(a, b), p, pinv); }

// Inversion-free Berlekamp-Massey over S_0 .. S_{checks-1}: C = the connection polynomial times a non-zero factor (C[0] != 0,
// C[i] = 0 for i > L), returns L.  L never shrinks, and coefficients past x^8 are dropped: they can only be non-zero once L > 8,
// and such a batch is undecoded whatever its polynomial says.  (Stopping the coefficient loops at the wave-uniform cap was tried:
// 149 VGPRs against 117 and no faster on 4 or 16 checks.)  S is rotated in place and comes back as it was.
SDA_HD uint32_t decode_bm(uint64_t (&S)[kDecodeChecks], uint32_t checks, uint64_t p, uint64_t pinv, uint64_t (&C)[kDecodeErrors + 1]) {
    uint64_t Bs[kDecodeErrors + 1], W[kDecodeErrors + 1];  // Bs = x^m B;  W[i] = S_{n-i} (0 before S_0)
#pragma unroll
    for (int i = 0; i <= kDecodeErrors; ++i) C[i] = Bs[i] = W[i] = 0;
    C[0] = 1;
    Bs[1] = 1;
    uint64_t b = 1;
    uint32_t L = 0;
#pragma unroll 1
    for (uint32_t n = 0; n < (uint32_t)kDecodeChecks; ++n) {
        if (n < checks) {
#pragma unroll
            for (int i = kDecodeErrors; i > 0; --i) W[i] = W[i - 1];
            W[0] = S[0];
            U128 acc = mul64x64(C[0], W[0]);
#pragma unroll
            for (int i = 1; i <= kDecodeErrors; ++i) {
                mac128(acc, C[i], W[i]);
                mont_acc_condsub(acc, p);                  // 9 p^2 can pass p 2^64
            }
            const uint64_t d = mont_redc(acc, p, pinv);    // the discrepancy (times 2^-64)
            const bool upd = d != 0, grow = upd && 2 * L <= n;
            const uint64_t nd = p - d;
            uint64_t prev = 0;                             // coefficient i - 1 of what becomes the next x^m B
#pragma unroll
            for (int i = 0; i <= kDecodeErrors; ++i) {
                const uint64_t ci = C[i], bi = Bs[i];
                U128 t = mul64x64(b, ci);
                mac128(t, nd, bi);                         // b C - d x^m B: 2 p^2 < p 2^64
                const uint64_t tn = mont_redc(t, p, pinv);
                C[i] = upd ? tn : ci;
                Bs[i] = prev;
                prev = grow ? ci : bi;
            }
            if (grow) {
                L = n + 1 - L;
                b = d;
            }
        }
        const uint64_t s0 = S[0];
#pragma unroll
        for (int i = 0; i + 1 < kDecodeChecks; ++i) S[i] = S[i + 1];
        S[kDecodeChecks - 1] = s0;
    }
    return L;
}

// The positions i of the job with Lrev(x_i) = 0, Lrev(z) = sum_i C[i] z^(L-i).  Horner runs to the wave-uniform `cap`: that
// evaluates z^(cap-L) Lrev(z), which has the same roots among the (non-zero) points.  Returns how many there are (at most L for
// L <= cap); the first kDecodeErrors of them go to pos[0], pos[stride], ...
SDA_HD uint32_t decode_roots(const uint64_t (&C)[kDecodeErrors + 1], uint32_t cap, uint32_t n_rows, const uint64_t* __restrict__ xs,
                             uint64_t p, uint64_t pinv, uint16_t* pos, uint32_t stride) {
    uint32_t roots = 0;
    for (uint32_t i = 0; i < n_rows; ++i) {
        const uint64_t x = xs[i];
        uint64_t acc = C[0];
#pragma unroll
        for (int j = 1; j <= kDecodeErrors; ++j)
            if ((uint32_t)j <= cap) acc = addmod(dec_mm(acc, x, p, pinv), C[j], p);
        if (acc == 0) {
            if (roots < (uint32_t)kDecodeErrors) pos[roots * stride] = (uint16_t)i;
            ++roots;
        }
    }
    return roots;
}

// Om[m] = sum_{i <= m} C[i] S_{m-i} (times 2^-64), m < cap: the evaluator polynomial S(x) C(x) mod x^L of every L <= cap
SDA_HD void decode_omega(const uint64_t (&S)[kDecodeChecks], const uint64_t (&C)[kDecodeErrors + 1], uint32_t cap, uint64_t p,
                         uint64_t pinv, uint64_t (&Om)[kDecodeErrors]) {
#pragma unroll
    for (int m = 0; m < kDecodeErrors; ++m) {
        Om[m] = 0;
        if ((uint32_t)m < cap) {
            U128 acc = mul64x64(C[0], S[m]);
#pragma unroll
            for (int i = 1; i <= m; ++i) {
                mac128(acc, C[i], S[m - i]);
                mont_acc_condsub(acc, p);
            }
            Om[m] = mont_redc(acc, p, pinv);
        }
    }
}

// Y of the root X (Montgomery form): with sigma(z) = Lrev(z) / (z - X),
//     Y = (sum_{d < L} S_d sigma_d) / sigma(X) = (sum_{m < L} Om[m] X^(L-1-m)) / sigma(X)
// - the factor of C cancels.  num carries the 2^-64 of Om, den = sigma(X) is exact; a Fermat power of den by mm alone is
// den^(p-2) 2^(-64 (p-3)) = 2^128 / den, and one more mm with num gives Y, canonical.
SDA_HD uint64_t decode_magnitude(const uint64_t (&C)[kDecodeErrors + 1], const uint64_t (&Om)[kDecodeErrors], uint32_t L, uint64_t X,
                                 uint64_t p, uint64_t pinv) {
    uint64_t num = 0, q = 0, den = 0;
#pragma unroll
    for (int i = 0; i < kDecodeErrors; ++i) {
        if ((uint32_t)i < L) {
            num = addmod(dec_mm(num, X, p, pinv), Om[i], p);
            q = addmod(dec_mm(q, X, p, pinv), C[i], p);    // synthetic division: the coefficient of z^(L-1-i) of sigma
            den = addmod(dec_mm(den, X, p, pinv), q, p);
        }
    }
    const uint64_t e = p - 2;
    int top = 63;
    while (top > 0 && !((e >> top) & 1)) --top;
    uint64_t inv = den;
    for (int bit = top - 1; bit >= 0; --bit) {
        inv = dec_mm(inv, inv, p, pinv);
        if ((e >> bit) & 1) inv = dec_mm(inv, den, p, pinv);
    }
    return dec_mm(num, inv, p, pinv);
}

// ---- erasures: positions the caller knows to be unreliable (sda_secret_reconstructor_finish_erasures_dev) ---------------------------
// F = the f erased positions, Gamma(z) = prod_{j in F} (z - x_j).  The MODIFIED syndromes T_j = sum_m gamma_m S_{j+m}, j < c - f,
// are the power sums of Z_i = Y_i Gamma(x_i) over the non-erased positions alone: the decoder above runs on T with length c - f,
// Y_i = Z_i / Gamma(x_i), and once the located errors are taken out of S_0 .. S_{f-1} the erased magnitudes are f dot products with
// the rows g_{j,m} / Gamma_j(x_j), Gamma_j(z) = Gamma(z) / (z - x_j).  What depends on the job and F only - the erased positions,
// those rows and 1 / Gamma(x_i) - is built once per finish (reveal_erasure_setup_kernel) into a table of 64-bit words, all in
// Montgomery form like xs; S, T, Y and Z are canonical, so a product of a table entry and one of them is exact after its one REDC.
static constexpr int kEraseMax = kDecodeChecks;            // the most erased positions a job can repair
static constexpr int kEraseCount = 0;                      // [0] f, counted in full;  [1] 1 when f > checks: nothing is repaired
static constexpr int kEraseOver = 1;
static constexpr int kErasePos = 2;                        // [2 + j] the j-th erased position, ascending, j < min(f, 16)
static constexpr int kEraseRows = kErasePos + kEraseMax;   // [18 + 16 j + m] g_{j,m} / Gamma_j(x_j), j, m < f
static constexpr int kEraseInv = kEraseRows + kEraseMax * kEraseMax;   // [274 + i] 1 / Gamma(x_i); 0 = position i is erased
SDA_HD constexpr size_t erase_table_words(size_t n_rows) { return (size_t)kEraseInv + n_rows; }

// a R -> R / a (both Montgomery form) by Fermat; 0 -> 0
SDA_HD uint64_t dec_inv(uint64_t a, uint64_t p, uint64_t pinv) {
    const uint64_t e = p - 2;
    int top = 63;
    while (top > 0 && !((e >> top) & 1)) --top;
    uint64_t inv = a;
    for (int bit = top - 1; bit >= 0; --bit) {
        inv = dec_mm(inv, inv, p, pinv);
        if ((e >> bit) & 1) inv = dec_mm(inv, a, p, pinv);
    }
    return inv;
}

// gam[0 .. kEraseMax]: the coefficients of Gamma (Montgomery form, 0 past f) from the f <= 16 erased positions; one = 2^64 mod p
SDA_HD void erase_gamma(const uint64_t* xs, const uint32_t* epos, uint32_t f, uint64_t one, uint64_t p, uint64_t pinv, uint64_t* gam) {
    for (int m = 0; m <= kEraseMax; ++m) gam[m] = 0;
    gam[0] = one;
    for (uint32_t j = 0; j < f; ++j) {
        const uint64_t x = xs[epos[j]];
        for (uint32_t m = j + 1; m >= 1; --m) gam[m] = submod(gam[m - 1], dec_mm(gam[m], x, p, pinv), p);
        gam[0] = submod(0, dec_mm(gam[0], x, p, pinv), p);
    }
}

// row[m] = g_{j,m} / Gamma_j(x_j), m < f, for the erased point xj (f >= 1): synthetic division of Gamma by (z - xj) from the top,
// Horner for Gamma_j(xj) on the way down, one Fermat power
SDA_HD void erase_solve_row(const uint64_t* gam, uint32_t f, uint64_t xj, uint64_t p, uint64_t pinv, uint64_t* row) {
    uint64_t g = gam[f], den = g;
    row[f - 1] = g;
    for (uint32_t m = f - 1; m >= 1; --m) {
        g = addmod(gam[m], dec_mm(g, xj, p, pinv), p);
        row[m - 1] = g;
        den = addmod(dec_mm(den, xj, p, pinv), g, p);
    }
    const uint64_t inv = dec_inv(den, p, pinv);
    for (uint32_t m = 0; m < f; ++m) row[m] = dec_mm(row[m], inv, p, pinv);
}

// 1 / Gamma(x); 0 exactly when x is one of the erased points (the job's points are distinct).  Nothing erased: Gamma = 1, no power
SDA_HD uint64_t erase_inv_gamma(const uint64_t* gam, uint32_t f, uint64_t x, uint64_t p, uint64_t pinv) {
    if (f == 0) return gam[0];
    uint64_t acc = gam[f];
    for (uint32_t m = f; m >= 1; --m) acc = addmod(dec_mm(acc, x, p, pinv), gam[m - 1], p);
    return dec_inv(acc, p, pinv);
}

// T(z) <- (z - x) T(z) read as T_j <- T_{j+1} - x T_j: one erased point folded into the syndromes, in place.  Every such step
// costs the sequence its last valid entry - after f of them T_0 .. T_{c-f-1} are the modified syndromes, erase_keep drops the rest.
SDA_HD void erase_fold_point(uint64_t (&T)[kDecodeChecks], uint32_t checks, uint64_t x, uint64_t p, uint64_t pinv) {
#pragma unroll
    for (int j = 0; j + 1 < kDecodeChecks; ++j)
        if ((uint32_t)(j + 1) < checks) T[j] = submod(T[j + 1], dec_mm(T[j], x, p, pinv), p);
}
SDA_HD void erase_keep(uint64_t (&T)[kDecodeChecks], uint32_t len) {
#pragma unroll
    for (int j = 0; j < kDecodeChecks; ++j) T[j] = (uint32_t)j < len ? T[j] : 0;
}

// decode_roots among the non-erased positions: inv_gamma[i] == 0 marks an erased one
SDA_HD uint32_t decode_roots_live(const uint64_t (&C)[kDecodeErrors + 1], uint32_t cap, uint32_t n_rows, const uint64_t* __restrict__ xs,
                                  const uint64_t* __restrict__ inv_gamma, uint64_t p, uint64_t pinv, uint16_t* pos, uint32_t stride) {
    uint32_t roots = 0;
    for (uint32_t i = 0; i < n_rows; ++i) {
        const uint64_t x = xs[i];
        uint64_t acc = C[0];
#pragma unroll
        for (int j = 1; j <= kDecodeErrors; ++j)
            if ((uint32_t)j <= cap) acc = addmod(dec_mm(acc, x, p, pinv), C[j], p);
        if (acc == 0 && inv_gamma[i] != 0) {
            if (roots < (uint32_t)kDecodeErrors) pos[roots * stride] = (uint16_t)i;
            ++roots;
        }
    }
    return roots;
}

// S_d -= Y X^d, d < f: a located error taken out of the sums the erased magnitudes are solved from
SDA_HD void erase_remove(uint64_t (&S)[kDecodeChecks], uint32_t f, uint64_t Y, uint64_t X, uint64_t p, uint64_t pinv) {
    uint64_t pw = Y;
#pragma unroll
    for (int d = 0; d < kDecodeChecks; ++d) {
        if ((uint32_t)d < f) {
            S[d] = submod(S[d], pw, p);
            pw = dec_mm(pw, X, p, pinv);
        }
    }
}

// Ye[j] = sum_{m < f} rows[16 j + m] S_m, j < f (0 from f on): the erased magnitudes.  The rows are walked by a rolled loop and
// Ye rotates one place per row - sixteen rotations leave row j's result at Ye[j] - so that no array is indexed at run time.
SDA_HD void erase_magnitudes(const uint64_t (&S)[kDecodeChecks], uint32_t f, const uint64_t* __restrict__ rows, uint64_t p, uint64_t pinv,
                             uint64_t (&Ye)[kEraseMax]) {
#pragma unroll
    for (int j = 0; j < kEraseMax; ++j) Ye[j] = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < (uint32_t)kEraseMax; ++j) {
        uint64_t y = 0;
        if (j < f) {
            const uint64_t* row = rows + (size_t)kEraseMax * j;
            U128 acc = mul64x64(row[0], S[0]);
#pragma unroll
            for (int m = 1; m < kEraseMax; ++m) {
                if ((uint32_t)m < f) {
                    mac128(acc, row[m], S[m]);
                    mont_acc_condsub(acc, p);              // 16 p^2 can pass p 2^64
                }
            }
            y = mont_redc(acc, p, pinv);
        }
#pragma unroll
        for (int i = 0; i + 1 < kEraseMax; ++i) Ye[i] = Ye[i + 1];
        Ye[kEraseMax - 1] = y;
    }
}

// v - sum_{j < f} corr[epos_j] Ye[j]: the erased positions' share of one secret's correction (corr = that secret's row of the table)
SDA_HD uint64_t erase_apply(uint64_t v, const uint64_t* __restrict__ corr, const uint64_t* __restrict__ table, uint32_t f,
                            const uint64_t (&Ye)[kEraseMax], uint64_t p, uint64_t pinv) {
#pragma unroll
    for (int j = 0; j < kEraseMax; ++j)
        if ((uint32_t)j < f) v = submod(v, dec_mm(corr[table[kErasePos + j]], Ye[j], p, pinv), p);
    return v;
}

}  // namespace sda

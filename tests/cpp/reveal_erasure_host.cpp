// The erasure steps of the lane decoder (sda_amd/csrc/reveal_decode.hpp) on the CPU: the functions reveal_erasure_setup_kernel and
// reveal_erasure_finish_kernel inline, in the kernels' order, on planted patterns.  For every prime / committee size / number of
// checks below, every f from 0 to checks and every nu from 0 to e' + 1 (e' = floor((checks - f) / 2)): magnitudes are planted on f
// erased and nu other positions, the syndromes S formed, and then
//   nu <= e'               the located positions, their magnitudes Y = Z / Gamma(x) and the f erased magnitudes must come back as
//                          planted, and erase_apply must subtract exactly sum corr Y over the erased positions;
//   e' < nu <= c - f - e'  the batch must come back undecoded.
// The table is also checked for what it promises: 0 at 1 / Gamma exactly on the erased positions.  Then STEERED syndromes: next to
// f erased rows that added anything, magnitudes on NODES that are no point of the job - a value z, the node 1, 0 - alone, next to
// one point, next to e' - 1 points, and a double root at a point: the modified syndromes are the power sums of Y Gamma(node) over
// those nodes, the locator has a root the search must not find, and the batch must come back undecoded.  Exit status 0 and two
// lines per shape when everything holds.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <random>
#include <vector>

#include "reveal_decode.hpp"

using namespace sda;

struct Shape {
    uint64_t p;
    uint32_t n_rows, checks;
};

// the finish kernel's lane up to its verdict: -1 undecoded, 0 consistent, nu decoded
static int lane_verdict(const Shape& sh, const uint64_t (&S)[kDecodeChecks], const std::vector<uint64_t>& table, uint32_t f,
                        const std::vector<uint64_t>& xs, const MontCtx& mc) {
    const uint64_t p = sh.p;
    const uint32_t len = sh.checks - f, e = len / 2;
    uint64_t T[kDecodeChecks];
    std::copy(S, S + kDecodeChecks, T);
    for (uint32_t q = 0; q < f; ++q) erase_fold_point(T, sh.checks, xs[table[kErasePos + q]], p, mc.pinv);
    erase_keep(T, len);
    uint64_t any = 0;
    for (int d = 0; d < kDecodeChecks; ++d) any |= T[d];
    if (any == 0) return 0;
    if (e == 0) return -1;
    uint64_t C[kDecodeErrors + 1];
    uint16_t pos[kDecodeErrors] = {0};
    const uint32_t L = decode_bm(T, len, p, mc.pinv, C);
    if (L >= 1 && L <= e && decode_roots_live(C, e, sh.n_rows, xs.data(), &table[kEraseInv], p, mc.pinv, pos, 1) == L) return (int)L;
    return -1;
}

int main() {
    const Shape shapes[] = {{2305843009213693951ull, 8, 4},  {2305843009213693951ull, 8, 1}, {2305843009213693951ull, 26, 16},
                            {4611686018427387847ull, 26, 16}, {4611686018427387847ull, 8, 4}, {746497, 260, 5},
                            {433, 8, 4},                      {433, 26, 16},                  {433, 8, 1}};
    std::mt19937_64 rng(20);
    int failures = 0;
    for (const Shape& sh : shapes) {
        const uint64_t p = sh.p;
        const MontCtx mc = h_mont_ctx(p);
        const uint64_t one = h_to_mont(1, p);
        const uint64_t rinv = h_powmod(one, p - 2, p);             // 2^-64 mod p
        std::vector<uint64_t> x, xs;
        while (x.size() < sh.n_rows) {
            const uint64_t v = 1 + rng() % (p - 1);
            if (std::find(x.begin(), x.end(), v) == x.end()) x.push_back(v);
        }
        for (uint64_t v : x) xs.push_back(h_to_mont(v, p));
        long repaired = 0, refused = 0, beyond = 0;
        for (int round = 0; round < 40; ++round) {
            for (uint32_t f = 0; f <= sh.checks; ++f) {
                const uint32_t len = sh.checks - f, e = len / 2;
                for (uint32_t nu = 0; nu <= e + 1 && f + nu <= sh.n_rows; ++nu) {
                    std::vector<uint32_t> where(sh.n_rows);
                    for (uint32_t i = 0; i < sh.n_rows; ++i) where[i] = i;
                    std::shuffle(where.begin(), where.end(), rng);
                    std::vector<uint32_t> F(where.begin(), where.begin() + f), E(where.begin() + f, where.begin() + f + nu);
                    std::sort(F.begin(), F.end());
                    std::sort(E.begin(), E.end());
                    std::vector<uint64_t> YF(f), YE(nu);
                    for (auto& y : YF) y = round % 3 == 2 ? 0 : rng() % p;  // an erased row may have added the right thing
                    for (auto& y : YE) y = 1 + rng() % (p - 1);
                    uint64_t S[kDecodeChecks] = {0};
                    for (uint32_t d = 0; d < sh.checks; ++d) {
                        for (uint32_t j = 0; j < f; ++j) S[d] = addmod(S[d], h_mulmod(YF[j], h_powmod(x[F[j]], d, p), p), p);
                        for (uint32_t j = 0; j < nu; ++j) S[d] = addmod(S[d], h_mulmod(YE[j], h_powmod(x[E[j]], d, p), p), p);
                    }
                    // ---- the setup kernel's table ----
                    std::vector<uint64_t> table(erase_table_words(sh.n_rows), 0);
                    uint32_t epos[kEraseMax] = {0};
                    uint64_t gam[kEraseMax + 1];
                    for (uint32_t j = 0; j < f; ++j) table[kErasePos + j] = epos[j] = F[j];
                    table[kEraseCount] = f;
                    erase_gamma(xs.data(), epos, f, one, p, mc.pinv, gam);
                    for (uint32_t j = 0; j < f; ++j) erase_solve_row(gam, f, xs[epos[j]], p, mc.pinv, &table[kEraseRows + kEraseMax * j]);
                    for (uint32_t i = 0; i < sh.n_rows; ++i) {
                        table[kEraseInv + i] = erase_inv_gamma(gam, f, xs[i], p, mc.pinv);
                        const bool erased = std::find(F.begin(), F.end(), i) != F.end();
                        if ((table[kEraseInv + i] == 0) != erased) { std::printf("1 / Gamma marks the wrong positions\n"); ++failures; }
                    }
                    // ---- the finish kernel's lane ----
                    uint64_t T[kDecodeChecks];
                    std::copy(S, S + kDecodeChecks, T);
                    for (uint32_t q = 0; q < f; ++q) erase_fold_point(T, sh.checks, xs[table[kErasePos + q]], p, mc.pinv);
                    erase_keep(T, len);
                    uint64_t any = 0;
                    for (int d = 0; d < kDecodeChecks; ++d) any |= T[d];
                    uint16_t pos[kDecodeErrors] = {0};
                    uint64_t Y[kDecodeErrors] = {0};
                    uint32_t got = 0;
                    bool undecoded = false;
                    if (any != 0) {
                        undecoded = true;
                        uint64_t C[kDecodeErrors + 1], Om[kDecodeErrors];
                        if (e >= 1) {
                            const uint32_t L = decode_bm(T, len, p, mc.pinv, C);
                            if (L >= 1 && L <= e && decode_roots_live(C, e, sh.n_rows, xs.data(), &table[kEraseInv], p, mc.pinv, pos, 1) == L) {
                                decode_omega(T, C, e, p, mc.pinv, Om);
                                for (uint32_t j = 0; j < L; ++j)
                                    Y[j] = dec_mm(decode_magnitude(C, Om, L, xs[pos[j]], p, mc.pinv), table[kEraseInv + pos[j]], p, mc.pinv);
                                got = L;
                                undecoded = false;
                            }
                        }
                    }
                    if (nu <= e) {
                        bool same = !undecoded && got == nu;
                        for (uint32_t j = 0; same && j < nu; ++j) same = pos[j] == E[j] && Y[j] == YE[j];
                        uint64_t Ye[kEraseMax];
                        if (same) {
                            for (uint32_t q = 0; q < got; ++q) erase_remove(S, f, Y[q], xs[pos[q]], p, mc.pinv);
                            erase_magnitudes(S, f, &table[kEraseRows], p, mc.pinv, Ye);
                            for (uint32_t j = 0; j < (uint32_t)kEraseMax; ++j) same = same && Ye[j] == (j < f ? YF[j] : 0);
                        }
                        if (same) {
                            std::vector<uint64_t> corr(sh.n_rows);
                            uint64_t want = rng() % p;
                            const uint64_t v = want;
                            for (auto& cv : corr) cv = rng() % p;
                            for (uint32_t j = 0; j < f; ++j) want = submod(want, h_mulmod(h_mulmod(corr[F[j]], YF[j], p), rinv, p), p);   // corr is in Montgomery form
                            same = erase_apply(v, corr.data(), table.data(), f, Ye, p, mc.pinv) == want;
                        }
                        if (!same) {
                            std::printf("p %llu rows %u checks %u f %u nu %u: not repaired as planted (got %u)\n", (unsigned long long)p, sh.n_rows,
                                        sh.checks, f, nu, got);
                            ++failures;
                        }
                        ++repaired;
                    } else if (nu <= len - e) {
                        if (!undecoded) {
                            std::printf("p %llu rows %u checks %u f %u nu %u: decoded past the cap\n", (unsigned long long)p, sh.n_rows, sh.checks, f, nu);
                            ++failures;
                        }
                        ++refused;
                    } else {
                        ++beyond;                                          // may decode to other positions: no claim
                    }
                }
            }
        }
        std::printf("p %llu rows %u checks %u: %ld repaired as planted, %ld refused, %ld beyond the guarantee\n", (unsigned long long)p,
                    sh.n_rows, sh.checks, repaired, refused, beyond);
        // ---- steered syndromes ----
        long steered = 0;
        for (int round = 0; round < 12; ++round) {
            for (uint32_t f = 0; f < sh.checks; ++f) {
                const uint32_t len = sh.checks - f, e = len / 2;
                if (f + e + 1 > sh.n_rows) continue;
                std::vector<uint32_t> where(sh.n_rows);
                for (uint32_t i = 0; i < sh.n_rows; ++i) where[i] = i;
                std::shuffle(where.begin(), where.end(), rng);
                std::vector<uint32_t> F(where.begin(), where.begin() + f);
                std::sort(F.begin(), F.end());
                const uint32_t* pts = where.data() + f;                        // non-erased positions, e + 1 of them at least
                std::vector<uint64_t> table(erase_table_words(sh.n_rows), 0);
                uint32_t epos[kEraseMax] = {0};
                uint64_t gam[kEraseMax + 1];
                for (uint32_t j = 0; j < f; ++j) table[kErasePos + j] = epos[j] = F[j];
                table[kEraseCount] = f;
                erase_gamma(xs.data(), epos, f, one, p, mc.pinv, gam);
                for (uint32_t j = 0; j < f; ++j) erase_solve_row(gam, f, xs[epos[j]], p, mc.pinv, &table[kEraseRows + kEraseMax * j]);
                for (uint32_t i = 0; i < sh.n_rows; ++i) table[kEraseInv + i] = erase_inv_gamma(gam, f, xs[i], p, mc.pinv);
                uint64_t z;
                do z = 2 + rng() % (p - 2); while (std::find(x.begin(), x.end(), z) != x.end());
                uint64_t base[kDecodeChecks] = {0};                            // what the erased rows added: anything
                std::vector<uint64_t> added(f);
                for (auto& y : added) y = rng() % p;
                for (uint32_t d = 0; d < sh.checks; ++d)
                    for (uint32_t j = 0; j < f; ++j) base[d] = addmod(base[d], h_mulmod(added[j], h_powmod(x[F[j]], d, p), p), p);
                auto run = [&](const char* what, const std::vector<uint64_t>& nodes, uint64_t confluent) {
                    uint64_t S[kDecodeChecks];
                    std::copy(base, base + kDecodeChecks, S);
                    std::vector<uint64_t> ys;
                    for (size_t j = 0; j < nodes.size(); ++j) ys.push_back(1 + rng() % (p - 1));
                    for (uint32_t d = 0; d < sh.checks; ++d) {
                        for (size_t j = 0; j < nodes.size(); ++j) S[d] = addmod(S[d], h_mulmod(ys[j], h_powmod(nodes[j], d, p), p), p);
                        if (confluent && d >= 1) S[d] = addmod(S[d], h_mulmod(h_mulmod(7 % p, d, p), h_powmod(confluent, d - 1, p), p), p);
                    }
                    const int got = lane_verdict(sh, S, table, f, xs, mc);
                    if (got != -1) {
                        std::printf("p %llu rows %u checks %u f %u steered %s: verdict %d, not undecoded\n", (unsigned long long)p, sh.n_rows,
                                    sh.checks, f, what, got);
                        ++failures;
                    }
                    ++steered;
                };
                run("a non-point", {z}, 0);
                if (std::find(x.begin(), x.end(), 1) == x.end()) run("the node 1", {1}, 0);      // (a tiny prime can draw 1 as a point)
                run("the node 0", {0}, 0);
                if (len >= 3) {
                    run("a point and a non-point", {x[pts[0]], z}, 0);
                    run("a double root", {}, x[pts[0]]);
                }
                if (e >= 2) {
                    std::vector<uint64_t> nodes;
                    for (uint32_t j = 0; j + 1 < e; ++j) nodes.push_back(x[pts[j]]);
                    nodes.push_back(z);
                    run("cap - 1 points and a non-point", nodes, 0);
                }
            }
        }
        std::printf("p %llu rows %u checks %u: %ld steered batches undecoded as constructed\n", (unsigned long long)p, sh.n_rows, sh.checks, steered);
    }
    if (failures) std::printf("%d FAILURES\n", failures);
    return failures ? 1 : 0;
}

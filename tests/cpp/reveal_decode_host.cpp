// The lane decoder of reveal_decode_finish_kernel (sda_amd/csrc/reveal_decode.hpp) on the CPU: the same functions the kernel
// inlines, on planted error patterns.  For every prime / committee size / number of checks below and every nu from 0 to e + 2
// (e = floor(checks / 2)): nu <= e must come back as exactly the planted positions and magnitudes, e + 1 .. checks - e must come
// back undecoded (L > e, or fewer than L roots).  Exit status 0 and one line per shape when everything holds.
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

int main() {
    const Shape shapes[] = {{2305843009213693951ull, 8, 4},   {2305843009213693951ull, 8, 3},  {2305843009213693951ull, 26, 16},
                            {2305843009213693951ull, 26, 9},  {2305843009213693951ull, 12, 2}, {4611686018427387847ull, 26, 16},
                            {746497, 260, 5},                 {746497, 260, 4},                {433, 8, 4},
                            {4611686018427387847ull, 8, 4}};
    std::mt19937_64 rng(19);
    int failures = 0;
    for (const Shape& sh : shapes) {
        const uint64_t p = sh.p;
        const MontCtx mc = h_mont_ctx(p);
        const uint32_t e = sh.checks / 2;
        std::vector<uint64_t> x, xs;
        while (x.size() < sh.n_rows) {
            const uint64_t v = 1 + rng() % (p - 1);
            if (std::find(x.begin(), x.end(), v) == x.end()) x.push_back(v);
        }
        for (uint64_t v : x) xs.push_back(h_to_mont(v, p));
        long decoded = 0, refused = 0, beyond = 0;
        for (int round = 0; round < 200; ++round) {
            for (uint32_t nu = 0; nu <= e + 2 && nu <= sh.n_rows; ++nu) {
                std::vector<uint32_t> where(sh.n_rows);
                for (uint32_t i = 0; i < sh.n_rows; ++i) where[i] = i;
                std::shuffle(where.begin(), where.end(), rng);
                where.resize(nu);
                std::sort(where.begin(), where.end());
                std::vector<uint64_t> Y(nu);
                for (auto& y : Y) y = 1 + rng() % (p - 1);
                if (nu == 2 && round % 2) Y[1] = p - Y[0];                 // S_0 = 0
                uint64_t S[kDecodeChecks] = {0};
                for (uint32_t d = 0; d < sh.checks; ++d)
                    for (uint32_t j = 0; j < nu; ++j) S[d] = addmod(S[d], h_mulmod(Y[j], h_powmod(x[where[j]], d, p), p), p);
                uint64_t keep[kDecodeChecks];
                std::copy(S, S + kDecodeChecks, keep);
                uint64_t C[kDecodeErrors + 1], Om[kDecodeErrors];
                uint16_t pos[kDecodeErrors] = {0};
                const uint32_t L = decode_bm(S, sh.checks, p, mc.pinv, C);
                if (!std::equal(S, S + kDecodeChecks, keep)) { std::printf("S not restored\n"); ++failures; }
                bool ok = false;
                if (L >= 1 && L <= e) {
                    const uint32_t roots = decode_roots(C, e, sh.n_rows, xs.data(), p, mc.pinv, pos, 1);
                    ok = roots == L;
                }
                if (nu == 0) {
                    if (L != 0) { std::printf("clean syndromes gave L = %u\n", L); ++failures; }
                } else if (nu <= e) {
                    bool same = ok && L == nu;
                    if (same) {
                        decode_omega(S, C, e, p, mc.pinv, Om);
                        for (uint32_t j = 0; j < nu; ++j)
                            same = same && pos[j] == where[j] && decode_magnitude(C, Om, L, xs[pos[j]], p, mc.pinv) == Y[j];
                    }
                    if (!same) { std::printf("p %llu rows %u checks %u nu %u: not decoded as planted (L %u)\n", (unsigned long long)p, sh.n_rows, sh.checks, nu, L); ++failures; }
                    ++decoded;
                } else if (nu <= sh.checks - e) {
                    if (ok) { std::printf("p %llu rows %u checks %u nu %u: decoded past the cap (L %u)\n", (unsigned long long)p, sh.n_rows, sh.checks, nu, L); ++failures; }
                    ++refused;
                } else {
                    ++beyond;                                              // may decode to other positions: no claim
                }
            }
        }
        std::printf("p %llu rows %u checks %u: %ld decoded as planted, %ld refused, %ld beyond the guarantee\n", (unsigned long long)p,
                    sh.n_rows, sh.checks, decoded, refused, beyond);
    }
    if (failures) std::printf("%d FAILURES\n", failures);
    return failures ? 1 : 0;
}

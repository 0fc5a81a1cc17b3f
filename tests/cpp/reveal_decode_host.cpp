// The lane decoder of reveal_decode_finish_kernel (sda_amd/csrc/reveal_decode.hpp) on the CPU: the same functions the kernel
// inlines, on planted error patterns.  For every prime / committee size / number of checks below and every nu from 0 to e + 2
// (e = floor(checks / 2)): nu <= e must come back as exactly the planted positions and magnitudes, e + 1 .. checks - e must come
// back undecoded (L > e, or fewer than L roots).  Then STEERED syndromes, whose verdict their construction fixes: the degenerate
// walks no planted pattern reaches - a locator whose root is no point of the job, is the node 1 (no row), is 0; L jumping from 0
// to c at the last syndrome; zero discrepancies up to c / 2; a double root; a point next to a value that is no point; p - 1 in
// every place; one point with Y = p - 1; two points with Y_1 = -Y_2; exactly e points; e - 1 points and a value that is no point.
// Exit status 0 and two lines per shape when everything holds.
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

// One steered batch: S = sum of y * node^d over `nodes` (a node need not be a point of the job), or S given outright.  want: the
// positions it must be decoded with (ascending, with the nodes' magnitudes in that order), or undecoded when `decodes` is false.
static bool steered_as_constructed(const char* what, const Shape& sh, uint64_t (&S)[kDecodeChecks], const std::vector<uint64_t>& xs,
                                   const MontCtx& mc, bool decodes, const std::vector<uint32_t>& want, const std::vector<uint64_t>& wantY,
                                   int wantL = -1) {
    const uint64_t p = sh.p;
    const uint32_t e = sh.checks / 2;
    uint64_t C[kDecodeErrors + 1], Om[kDecodeErrors];
    uint16_t pos[kDecodeErrors] = {0};
    const uint32_t L = decode_bm(S, sh.checks, p, mc.pinv, C);
    bool ok = false;
    if (L >= 1 && L <= e) ok = decode_roots(C, e, sh.n_rows, xs.data(), p, mc.pinv, pos, 1) == L;
    bool good = ok == decodes && (wantL < 0 || L == (uint32_t)wantL);
    if (good && decodes) {
        good = L == want.size();
        decode_omega(S, C, e, p, mc.pinv, Om);
        for (uint32_t j = 0; good && j < L; ++j) good = pos[j] == want[j] && decode_magnitude(C, Om, L, xs[pos[j]], p, mc.pinv) == wantY[j];
    }
    if (!good)
        std::printf("p %llu rows %u checks %u steered %s: L %u, %s - not as constructed\n", (unsigned long long)p, sh.n_rows, sh.checks, what, L,
                    ok ? "decoded" : "undecoded");
    return good;
}

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
        // ---- steered syndromes ----
        long steered = 0;
        const uint32_t c = sh.checks;
        for (int round = 0; round < 50; ++round) {
            uint64_t z;
            do z = 2 + rng() % (p - 2); while (std::find(x.begin(), x.end(), z) != x.end());
            const uint64_t a = 1 + rng() % (p - 1), b = 1 + rng() % (p - 1);
            std::vector<uint32_t> at(sh.n_rows);
            for (uint32_t i = 0; i < sh.n_rows; ++i) at[i] = i;
            std::shuffle(at.begin(), at.end(), rng);
            std::sort(at.begin(), at.begin() + std::min<uint32_t>(e ? e : 1, sh.n_rows));    // the first e: the points of this round, ascending
            auto sums = [&](const std::vector<uint64_t>& nodes, const std::vector<uint64_t>& ys, uint64_t (&S)[kDecodeChecks]) {
                for (uint32_t d = 0; d < (uint32_t)kDecodeChecks; ++d) S[d] = 0;
                for (uint32_t d = 0; d < c; ++d)
                    for (size_t j = 0; j < nodes.size(); ++j) S[d] = addmod(S[d], h_mulmod(ys[j], h_powmod(nodes[j], d, p), p), p);
            };
            auto run = [&](const char* what, uint64_t (&S)[kDecodeChecks], bool decodes, const std::vector<uint32_t>& want,
                           const std::vector<uint64_t>& wantY, int wantL = -1) {
                if (!steered_as_constructed(what, sh, S, xs, mc, decodes, want, wantY, wantL)) ++failures;
                ++steered;
            };
            uint64_t S[kDecodeChecks];
            const uint64_t x0 = x[at[0]];
            sums({z}, {a}, S);                  run("ratio z", S, false, {}, {}, 1);
            if (std::find(x.begin(), x.end(), 1) == x.end()) {                            // (a tiny prime can draw 1 as a point)
                sums({1}, {a}, S);              run("ratio 1", S, false, {}, {}, 1);
                sums({1}, {p - 1}, S);          run("all p - 1", S, false, {}, {}, 1);
            }
            sums({0}, {a}, S);                  run("ratio 0", S, false, {}, {}, 1);      // h_powmod(0, 0) = 1: (a, 0, .., 0)
            if (S[0] != a || S[1] != 0) { std::printf("ratio 0 is not (a, 0, ..)\n"); ++failures; }
            sums({}, {}, S);  S[c - 1] = a;     run("late jump", S, false, {}, {}, (int)c);
            sums({}, {}, S);
            for (uint32_t d = c / 2; d < c; ++d) S[d] = 1 + rng() % (p - 1);
            run("zero first half", S, false, {}, {});
            sums({}, {}, S);
            for (uint32_t d = 1; d < c; ++d) S[d] = h_mulmod(h_mulmod(a, d, p), h_powmod(x0, d - 1, p), p);
            run("double root", S, false, {}, {}, 2);
            if (c >= 3) { sums({x0, z}, {a, b}, S); run("point and non-point", S, false, {}, {}, 2); }
            sums({x0}, {p - 1}, S);             run("one point, Y = p - 1", S, e >= 1, {at[0]}, {p - 1});
            if (e >= 2) { sums({x0, x[at[1]]}, {a, p - a}, S); run("Y_1 = -Y_2", S, true, {at[0], at[1]}, {a, p - a}); }
            if (e >= 2) {
                std::vector<uint64_t> nodes, ys;
                std::vector<uint32_t> where(at.begin(), at.begin() + e);
                for (uint32_t j = 0; j < e; ++j) { nodes.push_back(x[at[j]]); ys.push_back(1 + rng() % (p - 1)); }
                sums(nodes, ys, S);             run("cap points", S, true, where, ys, (int)e);
                nodes[e - 1] = z;
                sums(nodes, ys, S);             run("cap - 1 points and a non-point", S, false, {}, {}, (int)e);
            }
        }
        std::printf("p %llu rows %u checks %u: %ld steered batches as constructed\n", (unsigned long long)p, sh.n_rows, sh.checks, steered);
    }
    if (failures) std::printf("%d FAILURES\n", failures);
    return failures ? 1 : 0;
}

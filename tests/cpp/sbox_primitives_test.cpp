// Host unit test of sda_amd/csrc/sbox_primitives.hpp (the same header the device kernels compile): reads commands
// with hex operands on stdin, prints hex results; tests/test_sealedbox_cpu.py compares them with the published
// vectors and with oracle/sealedbox_oracle.py.
//   x25519 <k:32> <u:32>          hsalsa <key:32> <in:16>       salsa <key:32> <nonce:8> <counter decimal>
//   nonce <epk:32> <pk:32>        poly <key:32> <msg:any>
// and the raw primitives on limbs given explicitly (comma-separated decimals; results likewise, or hex bytes):
//   femul <f:10> <g:10>           fesq <f:10>                   fecarry <h:10, 64-bit>        fewords <f:10>
//   p26mul <a:5> <b:5>            p26carry <h:5>                p26finish <h:5> <s:16>
//   polydev <key:32> <msg:any> <regions, 0 = as many as the message needs>
//                                 Poly1305 in the DEVICE's order (sealedbox_kernels.hip: sbox_poly_kernel and
//                                 sbox_final_kernel), restated here from the header's own functions: the power table, 64
//                                 virtual lanes striding each 16 KiB region from the end of the message, uint32_t lane sums,
//                                 Horner over the regions with r^1024
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "../../sda_amd/csrc/sbox_primitives.hpp"

using namespace sda::sbx;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}
static void words(const std::vector<uint8_t>& b, uint32_t* w, size_t n) {
    for (size_t i = 0; i < n; ++i) w[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
}
static void put(const uint32_t* w, size_t n) {
    for (size_t i = 0; i < n; ++i) printf("%02x%02x%02x%02x", w[i] & 255, (w[i] >> 8) & 255, (w[i] >> 16) & 255, w[i] >> 24);
    printf("\n");
}

static std::vector<long long> csv(const std::string& s) {
    std::vector<long long> out;
    size_t pos = 0;
    while (pos <= s.size()) {
        size_t end = s.find(',', pos);
        if (end == std::string::npos) end = s.size();
        out.push_back(strtoll(s.substr(pos, end - pos).c_str(), nullptr, 10));
        pos = end + 1;
    }
    return out;
}
static bool read_fe(Fe& f) {
    std::string a; std::cin >> a;
    const std::vector<long long> v = csv(a);
    if (v.size() != 10) return false;
    for (int i = 0; i < 10; ++i) f.v[i] = (int32_t)v[i];
    return true;
}
static bool read_p26(P26& h) {
    std::string a; std::cin >> a;
    const std::vector<long long> v = csv(a);
    if (v.size() != 5) return false;
    for (int i = 0; i < 5; ++i) h.v[i] = (uint32_t)v[i];
    return true;
}
static void put_fe(const Fe& f) {
    for (int i = 0; i < 10; ++i) printf("%d%s", f.v[i], i < 9 ? "," : "\n");
}
static void put_p26(const P26& h) {
    for (int i = 0; i < 5; ++i) printf("%u%s", h.v[i], i < 4 ? "," : "\n");
}

// Poly1305 tag in the order of the kernels; `regions` >= the regions the message uses (the rest hold zero sums, as on the device)
static void poly_device_order(uint32_t tag[4], const uint32_t key[8], const std::vector<uint8_t>& msg, size_t regions) {
    const int steps = 16, lanes = 64;
    P26 r, rp, rpow[64], r64, rS;
    p26_clamped_r(r, key);
    rp = r;
    for (int i = 0; i < 64; ++i) {
        rpow[i] = rp;
        if (i < 63) { P26 t; p26_mul(t, rp, r); rp = t; }
    }
    r64 = rp;
    for (int s = steps; s > 1; s >>= 1) { P26 t; p26_mul(t, rp, rp); rp = t; }
    rS = rp;
    const uint64_t mlen = msg.size(), npieces = (mlen + 15) / 16;
    const uint32_t tail = (uint32_t)(mlen & 15);
    const size_t used = (size_t)((npieces + lanes * steps - 1) / (lanes * steps));
    if (regions < used || regions == 0) regions = used ? used : 1;
    std::vector<P26> partial(regions);
    for (size_t region = 0; region < regions; ++region) {
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (uint32_t lane = 0; lane < (uint32_t)lanes; ++lane) {
            P26 h;
            for (int j = 0; j < 5; ++j) h.v[j] = 0;
            const uint64_t d0 = (uint64_t)region * lanes * steps + lane + 1;
            if (d0 - lane <= npieces) {
                for (int m = steps - 1; m >= 0; --m) {
                    const uint64_t d = d0 + 64 * (uint64_t)m;
                    P26 t;
                    p26_mul(t, h, r64);
                    h = t;
                    if (d <= npieces) {
                        const uint64_t b = npieces - d;
                        const uint32_t nb = (d == 1 && tail) ? tail : 16u;
                        uint8_t buf[16] = {0};
                        memcpy(buf, msg.data() + 16 * b, nb);
                        uint32_t w[4];
                        words(std::vector<uint8_t>(buf, buf + 16), w, 4);
                        P26 c;
                        p26_from_piece(c, w, nb);
                        p26_add(h, h, c);
                    }
                }
                P26 t;
                p26_mul(t, h, rpow[lane]);
                h = t;
                p26_carry(h);
            }
            for (int j = 0; j < 5; ++j) sum[j] += h.v[j];                 // uint32_t, as the wave's shuffle sum
        }
        for (int j = 0; j < 5; ++j) partial[region].v[j] = sum[j];
    }
    P26 acc;
    for (int j = 0; j < 5; ++j) acc.v[j] = 0;
    for (size_t g = used; g-- > 0;) {
        P26 t, p = partial[g];
        p26_mul(t, acc, rS);
        p26_carry(p);
        p26_add(acc, t, p);
    }
    p26_finish(tag, acc, key + 4);
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "x25519") {
            std::string a, b; std::cin >> a >> b;
            uint32_t k[8], u[8], o[8];
            words(unhex(a), k, 8); words(unhex(b), u, 8);
            x25519(o, k, u); put(o, 8);
        } else if (cmd == "hsalsa") {
            std::string a, b; std::cin >> a >> b;
            uint32_t k[8], in[4], o[8];
            words(unhex(a), k, 8); words(unhex(b), in, 4);
            hsalsa20(o, k, in); put(o, 8);
        } else if (cmd == "salsa") {
            std::string a, b; unsigned long long ctr; std::cin >> a >> b >> ctr;
            uint32_t k[8], n[2], o[16];
            words(unhex(a), k, 8); words(unhex(b), n, 2);
            salsa20_block(o, k, n[0], n[1], ctr); put(o, 16);
        } else if (cmd == "nonce") {
            std::string a, b; std::cin >> a >> b;
            uint32_t e[8], p[8], o[6];
            words(unhex(a), e, 8); words(unhex(b), p, 8);
            seal_nonce(o, e, p); put(o, 6);
        } else if (cmd == "poly") {
            std::string a, b; std::cin >> a >> b;
            std::vector<uint8_t> key = unhex(a), msg = unhex(b);
            uint32_t kw[8];
            words(key, kw, 8);
            P26 r, h, c, t;
            p26_clamped_r(r, kw);
            for (int i = 0; i < 5; ++i) h.v[i] = 0;
            for (size_t off = 0; off < msg.size(); off += 16) {
                const size_t n = msg.size() - off < 16 ? msg.size() - off : 16;
                uint8_t buf[16] = {0};
                memcpy(buf, msg.data() + off, n);
                uint32_t w[4];
                words(std::vector<uint8_t>(buf, buf + 16), w, 4);
                p26_from_piece(c, w, (uint32_t)n);
                p26_add(t, h, c);
                p26_mul(h, t, r);
            }
            uint32_t tag[4];
            p26_finish(tag, h, kw + 4); put(tag, 4);
        } else if (cmd == "femul" || cmd == "fesq" || cmd == "fewords") {
            Fe f, g, o;
            if (!read_fe(f) || (cmd == "femul" && !read_fe(g))) return 3;
            if (cmd == "fewords") { uint32_t w[8]; fe_to_words(w, f); put(w, 8); continue; }
            if (cmd == "femul") fe_mul(o, f, g); else fe_sq(o, f);
            put_fe(o);
        } else if (cmd == "fecarry") {
            std::string a; std::cin >> a;
            const std::vector<long long> v = csv(a);
            if (v.size() != 10) return 3;
            int64_t h[10];
            for (int i = 0; i < 10; ++i) h[i] = v[i];
            Fe o;
            fe_carry(o, h); put_fe(o);
        } else if (cmd == "p26mul") {
            P26 a, b, o;
            if (!read_p26(a) || !read_p26(b)) return 3;
            p26_mul(o, a, b); put_p26(o);
        } else if (cmd == "p26carry") {
            P26 h;
            if (!read_p26(h)) return 3;
            p26_carry(h); put_p26(h);
        } else if (cmd == "p26finish") {
            P26 h;
            std::string b;
            if (!read_p26(h)) return 3;
            std::cin >> b;
            uint32_t s[4], tag[4];
            words(unhex(b), s, 4);
            p26_finish(tag, h, s); put(tag, 4);
        } else if (cmd == "polydev") {
            std::string a, b; unsigned long long regions; std::cin >> a >> b >> regions;
            uint32_t kw[8], tag[4];
            words(unhex(a), kw, 8);
            poly_device_order(tag, kw, unhex(b), (size_t)regions);
            put(tag, 4);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}

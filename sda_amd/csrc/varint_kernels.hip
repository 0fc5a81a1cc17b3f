// Zig-zag LEB128 codec of share vectors on gfx950: the wire format either side
// of the path - client/src/crypto/encryption/sodium.rs:36-41 (encode: `share.encode_var`) and :83-89
// (decode: `Share::decode_var` until the reader is empty); integer-encoding 1.0 `VarInt for i64`.
//
// Variable-length coding is a scan problem:
//   encode: byte length per value (clz) -> workgroup sums -> exclusive scan -> bytes staged in LDS and
//           copied out with dword stores;
//   decode: a byte with the MSB clear terminates a value, so value index = number of terminators
//           before it: terminator counts per 4 KiB -> exclusive scan -> every terminator's owner lane
//           looks back <= 9 bytes in an LDS tile (16-byte halo) and assembles the value.
// Both are HBM streams (about 9 B of wire + 8 B of value per 62-bit share).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "capi_internal.hpp"
#include "drbg_quad.hpp"
#include "kernels.hpp"
#include "launch_plan.hpp"
#include "modarith.hpp"
#include "sbox_primitives.hpp"

namespace sda {

static constexpr int kVT = 256;          // threads per workgroup
static constexpr int kVals = 8;          // encode: values per lane  (2048 per workgroup)
static constexpr int kBytes = 16;        // decode: bytes per lane   (4096 per workgroup)

__device__ __forceinline__ uint64_t zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
__device__ __forceinline__ uint32_t varint_len(uint64_t zz) {
    const uint32_t x = (64u - (uint32_t)__clzll(zz | 1ull)) + 6u;     // bits + 6, in 7..70
    return (x * 37u) >> 8;                                            // x / 7 for x <= 70
}

// workgroup exclusive scan of one u32 per lane; returns the lane's prefix, *total = workgroup sum
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t* lds_waves, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) lds_waves[wave] = incl;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kVT / 64; ++w) {
        const uint32_t t = lds_waves[w];
        if (w < wave) off += t;
        tot += t;
    }
    *total = tot;
    __syncthreads();
    return off + incl - v;
}

// ---- encode ---------------------------------------------------------------------------------------
// Only the workgroup total matters here, so the 2048 values of a block are dealt to the lanes in coalesced pairs
// (pair q of the block -> lane q % 256, one 16-byte load when the pair lies inside a row and is aligned) instead of
// the 8 consecutive values per lane the write kernel needs.
__global__ __launch_bounds__(kVT) void varint_len_kernel(VarintRows R, uint32_t* __restrict__ block_bytes) {
    __shared__ uint32_t waves[kVT / 64];
    const uint64_t N = (uint64_t)R.rows * R.len;
    const uint64_t base = (uint64_t)blockIdx.x * kVT * kVals;
    const bool vec_ok = (((uintptr_t)R.values) & 15u) == 0 && (R.row_stride & 1u) == 0;
    uint32_t sum = 0;
    uint64_t g = base + 2 * (uint64_t)threadIdx.x;
    if (g < N) {
        uint64_t r = g / R.len, i = g - r * R.len;
#pragma unroll
        for (int u = 0; u < kVals / 2; ++u) {
            if (g < N) {
                const int64_t* p = R.values + r * R.row_stride + i;
                if (vec_ok && i + 1 < R.len && (i & 1u) == 0) {
                    typedef long long ll2v __attribute__((ext_vector_type(2)));
                    const ll2v v = __builtin_nontemporal_load(reinterpret_cast<const ll2v*>(p));
                    sum += varint_len(zigzag(v.x)) + varint_len(zigzag(v.y));
                } else {
                    sum += varint_len(zigzag(p[0]));
                    if (g + 1 < N) sum += varint_len(zigzag(i + 1 < R.len ? p[1] : R.values[(r + 1) * R.row_stride]));
                }
            }
            g += 2 * kVT;
            i += 2 * kVT;
            if (i >= R.len) { const uint64_t q = i / R.len; r += q; i -= q * R.len; }
        }
    }
    uint32_t total;
    (void)block_exscan(sum, waves, &total);
    if (threadIdx.x == 0) block_bytes[blockIdx.x] = total;
}

// ---- exclusive scan of u32 -> u64, three small kernels: scan 1024-entry chunks in parallel, scan the
// chunk totals with one workgroup, add the chunk offsets back ------------------------------------------------
__device__ __forceinline__ uint64_t block1024_exscan(uint64_t v, uint64_t* wave_sum, uint64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint64_t off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const uint64_t t = wave_sum[w];
        if (w < wave) off += t;
        tot += t;
    }
    *total = tot;
    __syncthreads();
    return off + incl - v;
}

__global__ __launch_bounds__(1024) void scan_chunks_kernel(const uint32_t* __restrict__ in, uint64_t* __restrict__ out,
                                                           uint64_t* __restrict__ chunk_tot, size_t n) {
    __shared__ uint64_t wave_sum[16];
    const size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x;
    uint64_t total;
    const uint64_t ex = block1024_exscan(i < n ? in[i] : 0, wave_sum, &total);
    if (i < n) out[i] = ex;
    if (threadIdx.x == 0) chunk_tot[blockIdx.x] = total;
}

// one workgroup: in-place exclusive scan of the chunk totals, *total = grand total
__global__ __launch_bounds__(1024) void scan_totals_kernel(uint64_t* __restrict__ tot, size_t m, uint64_t* __restrict__ total) {
    __shared__ uint64_t wave_sum[16];
    uint64_t carry = 0;
    for (size_t base = 0; base < m; base += 1024) {
        const size_t i = base + threadIdx.x;
        uint64_t t;
        const uint64_t ex = block1024_exscan(i < m ? tot[i] : 0, wave_sum, &t);
        if (i < m) tot[i] = carry + ex;
        carry += t;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(1024) void scan_add_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ chunk_off,
                                                        size_t n) {
    const size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x;
    if (i < n) out[i] += chunk_off[blockIdx.x];
}

__global__ __launch_bounds__(kVT) void varint_write_kernel(VarintRows R, const uint64_t* __restrict__ block_off,
                                                           uint8_t* __restrict__ out, uint64_t* __restrict__ row_offsets) {
    __shared__ uint32_t waves[kVT / 64];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kVT * kVals * 10 + 16];
    const uint64_t N = (uint64_t)R.rows * R.len;
    const uint64_t g0 = ((uint64_t)blockIdx.x * kVT + threadIdx.x) * kVals;
    uint64_t zz[kVals];
    uint32_t ln[kVals];
    uint32_t sum = 0;
    uint64_t r0 = 0, i0 = 0;
    if (g0 < N) { r0 = g0 / R.len; i0 = g0 - r0 * R.len; }
    {
        uint64_t r = r0, i = i0;
#pragma unroll
        for (int k = 0; k < kVals; ++k) {
            zz[k] = 0; ln[k] = 0;
            if (g0 + k < N) {
                zz[k] = zigzag(R.values[r * R.row_stride + i]);
                ln[k] = varint_len(zz[k]);
                sum += ln[k];
            }
            if (++i == R.len) { i = 0; ++r; }
        }
    }
    uint32_t total;
    uint32_t pos = block_exscan(sum, waves, &total);
    const uint64_t boff = block_off[blockIdx.x];
    {
        uint64_t r = r0, i = i0;
#pragma unroll
        for (int k = 0; k < kVals; ++k) {
            if (g0 + k < N) {
                if (i == 0 && row_offsets) row_offsets[r] = boff + pos;     // this value opens row r
                uint64_t n = zz[k];
                for (uint32_t b = 0; b + 1 < ln[k]; ++b) { stage[pos++] = (uint8_t)(0x80u | (n & 0x7Fu)); n >>= 7; }
                stage[pos++] = (uint8_t)n;
            }
            if (++i == R.len) { i = 0; ++r; }
        }
    }
    __syncthreads();
    // copy out: bytes up to the first 4-byte boundary of the destination, then dwords, then the tail
    uint8_t* dst = out + boff;
    const uint32_t head = (uint32_t)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
    const uint32_t h = head < total ? head : total;
    if (threadIdx.x < h) dst[threadIdx.x] = stage[threadIdx.x];
    const uint32_t n_dw = (total - h) >> 2;
    const uint32_t* stage32 = reinterpret_cast<const uint32_t*>(stage);
    uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst + h);
    for (uint32_t d = threadIdx.x; d < n_dw; d += kVT) {
        const uint32_t byte = h + 4u * d;                  // source byte offset in stage
        const uint32_t lo = stage32[byte >> 2], hi = stage32[(byte >> 2) + 1];
        dst32[d] = __builtin_amdgcn_alignbyte(hi, lo, byte & 3u);
    }
    const uint32_t done = h + 4u * n_dw;
    if (threadIdx.x < total - done) dst[done + threadIdx.x] = stage[done + threadIdx.x];
}

// ---- decode -----------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t count_terminators16(const uint32_t (&w)[4]) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += __builtin_popcount(~w[k] & 0x80808080u);
    return c;
}

__device__ __forceinline__ void load16(const uint8_t* __restrict__ bytes, uint64_t n_bytes, uint64_t p, uint32_t (&w)[4]) {
    if (p + 16 <= n_bytes && ((uintptr_t)(bytes + p) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(bytes + p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {                                            // ragged tail / unaligned base: bytes beyond the end read as
#pragma unroll                                          // continuation bytes (0x80) so they are never terminators
        for (int k = 0; k < 4; ++k) {
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint64_t q = p + 4 * k + b;
                x |= (uint32_t)(q < n_bytes ? bytes[q] : 0x80u) << (8 * b);
            }
            w[k] = x;
        }
    }
}

__global__ __launch_bounds__(kVT) void varint_count_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                           uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t waves[kVT / 64];
    const uint64_t p = ((uint64_t)blockIdx.x * kVT + threadIdx.x) * kBytes;
    uint32_t w[4] = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    if (p < n_bytes) load16(bytes, n_bytes, p, w);
    uint32_t total;
    (void)block_exscan(count_terminators16(w), waves, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// status bits
#define SDA_VARINT_MALFORMED 1u      // more than 10 bytes without a terminator
#define SDA_VARINT_ROW_COUNT 2u      // a row does not hold exactly `len` values
#define SDA_VARINT_UNTERMINATED 4u   // a row (or the stream) ends inside a value

__global__ __launch_bounds__(kVT) void varint_decode_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                            const uint64_t* __restrict__ block_val_off, uint64_t rows,
                                                            uint64_t len, uint64_t row_stride,
                                                            int64_t* __restrict__ out, uint32_t* __restrict__ status) {
    __shared__ uint32_t waves[kVT / 64];
    __shared__ __attribute__((aligned(16))) uint8_t tile[16 + kVT * kBytes + 16];   // halo | span | read slack
    const uint64_t block_base = (uint64_t)blockIdx.x * kVT * kBytes;
    const uint64_t p = block_base + (uint64_t)threadIdx.x * kBytes;
    uint32_t w[4] = {0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    if (p < n_bytes) load16(bytes, n_bytes, p, w);
    uint32_t* tile32 = reinterpret_cast<uint32_t*>(tile);
#pragma unroll
    for (int k = 0; k < 4; ++k) tile32[4 + threadIdx.x * 4 + k] = w[k];
    if (threadIdx.x < 16) {                                 // halo: the 16 bytes before this workgroup's span
        const uint64_t q = block_base + threadIdx.x;
        tile[threadIdx.x] = q >= 16 ? bytes[q - 16] : 0u;   // before the stream: a terminator stops the look-back
    }
    uint32_t total;
    uint32_t idx = block_exscan(count_terminators16(w), waves, &total);   // also orders the tile writes
    uint64_t g = block_val_off[blockIdx.x] + idx;
    const uint64_t N = rows * len;
    uint64_t r = 0, i = 0;
    bool have_ri = false;
    // continuation-bit map of this lane's 16 bytes (bit k = MSB of byte k) and of the 16 bytes before it
    uint32_t own = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t m = w[k] & 0x80808080u;                      // bits 7,15,23,31 -> 0..3
        own |= (((m >> 7) | (m >> 14) | (m >> 21) | (m >> 28)) & 0xFu) << (4 * k);
    }
    uint32_t prev = 0;
    {
        const uint32_t* t32 = reinterpret_cast<const uint32_t*>(tile) + threadIdx.x * 4;   // the 16 bytes before
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t m = t32[k] & 0x80808080u;
            prev |= (((m >> 7) | (m >> 14) | (m >> 21) | (m >> 28)) & 0xFu) << (4 * k);
        }
        // (the halo before the start of the stream was filled with terminators, so prev == 0 there)
    }
    const uint32_t cont = (own << 16) | prev;                       // 32-byte window, bit q = byte q continues
    uint32_t terms = ~own & 0xFFFFu;
    if (p + 16 > n_bytes) terms &= p < n_bytes ? (1u << (uint32_t)(n_bytes - p)) - 1u : 0u;
    while (terms) {
        const int k = __builtin_ctz(terms);
        terms &= terms - 1;
        const int e = 16 + k;                                       // window position of the terminator
        // previous non-continuation byte below e: the value starts right after it
        const uint32_t below = ~cont & ((1u << e) - 1u);
        const int prev_term = below ? 31 - __builtin_clz(below) : -1;
        int nb = e - prev_term;                                     // bytes of this value
        if (nb > 10) { atomicOr(status, SDA_VARINT_MALFORMED); nb = 10; }
        const int start = 16 + (int)threadIdx.x * kBytes + k - (nb - 1);   // tile coordinate of the first byte
        // 12 bytes from the tile at an arbitrary byte offset
        const uint32_t* t32 = reinterpret_cast<const uint32_t*>(tile) + (start >> 2);
        const uint32_t sh = (uint32_t)start & 3u;
        const uint32_t d0 = __builtin_amdgcn_alignbyte(t32[1], t32[0], sh);
        const uint32_t d1 = __builtin_amdgcn_alignbyte(t32[2], t32[1], sh);
        const uint32_t d2 = __builtin_amdgcn_alignbyte(t32[3], t32[2], sh);
        uint64_t x = ((uint64_t)d1 << 32) | d0;                     // bytes 0..7 of the value
        if (nb < 8) x &= (1ull << (8 * nb)) - 1ull;
        x &= 0x7F7F7F7F7F7F7F7Full;                                 // drop the continuation bits, then squeeze
        x = ((x & 0x7F007F007F007F00ull) >> 1) | (x & 0x007F007F007F007Full);
        x = ((x & 0x3FFF00003FFF0000ull) >> 2) | (x & 0x00003FFF00003FFFull);
        x = ((x & 0x0FFFFFFF00000000ull) >> 4) | (x & 0x000000000FFFFFFFull);
        if (nb > 8) x |= (uint64_t)(d2 & 0x7Fu) << 56;
        if (nb > 9) x |= (uint64_t)((d2 >> 8) & 0x7Fu) << 63;
        const int64_t v = (int64_t)((x >> 1) ^ (uint64_t)(-(int64_t)(x & 1)));
        if (g < N) {
            if (!have_ri) { r = g / len; i = g - r * len; have_ri = true; }
            out[r * row_stride + i] = v;
            if (++i == len) { i = 0; ++r; }
        }
        ++g;
    }
}

// terminators in [block start, x) counted by a whole wave: 64 lanes x 16 B per step
__device__ __forceinline__ uint64_t wave_prefix(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                const uint64_t* __restrict__ block_val_off, uint64_t x) {
    const uint64_t blk = x / (kVT * kBytes);
    const uint64_t base = blk * (kVT * kBytes);
    const int lane = threadIdx.x & 63;
    uint32_t c = 0;
    for (uint64_t q = base + (uint64_t)lane * 16; q < x; q += 64 * 16) {
        uint32_t w[4];
        load16(bytes, n_bytes, q, w);
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t m = ~w[k] & 0x80808080u;
            t |= (((m >> 7) | (m >> 14) | (m >> 21) | (m >> 28)) & 0xFu) << (4 * k);
        }
        if (q + 16 > x) t &= (1u << (uint32_t)(x - q)) - 1u;
        c += __builtin_popcount(t);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    return block_val_off[blk] + c;
}

// one WAVE per row: the row must end on a terminator and hold exactly `len` values
__global__ __launch_bounds__(kVT) void varint_rowcheck_kernel(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                              const uint64_t* __restrict__ offsets, uint64_t rows,
                                                              uint64_t len, const uint64_t* __restrict__ block_val_off,
                                                              uint32_t* __restrict__ status) {
    const uint64_t r = (uint64_t)blockIdx.x * (kVT / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const bool lead = (threadIdx.x & 63) == 0;
    const uint64_t a = offsets ? offsets[r] : 0, b = offsets ? offsets[r + 1] : n_bytes;
    if (b < a || b > n_bytes) { if (lead) atomicOr(status, SDA_VARINT_ROW_COUNT); return; }
    if (len == 0) { if (a != b && lead) atomicOr(status, SDA_VARINT_ROW_COUNT); return; }
    if (a == b || (bytes[b - 1] & 0x80u)) { if (lead) atomicOr(status, SDA_VARINT_UNTERMINATED); return; }
    const uint64_t cnt = wave_prefix(bytes, n_bytes, block_val_off, b) - wave_prefix(bytes, n_bytes, block_val_off, a);
    if (cnt != len && lead) atomicOr(status, SDA_VARINT_ROW_COUNT);
}

// ---- single-pass row streaming ----------------------------------------------------------------------
// Every encoded vector (row) is its own message with a known byte range, so the only sequential dependence is
// inside a row.  One WAVE streams one row in fixed 1 KiB chunks (64 lanes x 16 B) laid on the 16-byte grid below
// the row start: chunk addresses do not depend on the content, so the next chunks are prefetched into registers
// while the current one is decoded; what is carried from chunk to chunk is the column index, the continuation
// bitmap of the last 16 bytes and those 16 bytes themselves (the halo a value crossing the chunk boundary needs).
// The bytes are read ONCE (the three-pass form reads them twice and needs the block scan in between).
static constexpr int kStreamWaves = 4;                 // rows per workgroup
static constexpr int kStreamDepth = 4;                 // chunks in flight per wave
static constexpr int kStreamTile = 16 + 64 * 16 + 16;  // halo | chunk | read slack, per wave


// bit k = MSB of byte k.  (m >> 7) has the four flags at bits 0, 8, 16, 24; the multiplier moves them to bits
// 28..31 (partial products below bit 28 never collide, so nothing carries in).
__device__ __forceinline__ uint32_t cont_bits16(const uint4& v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) r |= ((((w[k] & 0x80808080u) >> 7) * 0x10204080u) >> 28) << (4 * k);
    return r;
}

// wave64 inclusive scan with DPP row shifts / broadcasts (no LDS crossbar, no waits)
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t x, uint32_t src) {
    return x + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)src, CTRL, ROW_MASK, BANK_MASK, false);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    uint32_t x = dpp_add<0x111, 0xf, 0xf>(v, v);      // row_shr:1
    x = dpp_add<0x112, 0xf, 0xf>(x, v);               // row_shr:2
    x = dpp_add<0x113, 0xf, 0xf>(x, v);               // row_shr:3  -> lanes hold the sum of up to 4 neighbours
    x = dpp_add<0x114, 0xf, 0xe>(x, x);               // row_shr:4, banks 1-3
    x = dpp_add<0x118, 0xf, 0xc>(x, x);               // row_shr:8, banks 2-3 -> inclusive scan inside each row of 16
    x = dpp_add<0x142, 0xa, 0xf>(x, x);               // row_bcast:15 into rows 1 and 3
    x = dpp_add<0x143, 0xc, 0xf>(x, x);               // row_bcast:31 into rows 2 and 3
    return x;
}

// 16 bytes at bytes + rel (rel may reach 15 bytes below the buffer: same 16-byte granule as its first byte).
// Addressed from the kernel argument so that it stays a GLOBAL load: a flat load would also count as an LDS
// operation and every LDS wait would then drain the prefetch queue.
__device__ __forceinline__ uint4 stream_load(const uint8_t* __restrict__ bytes, int64_t rel, int64_t end_rel) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (rel < end_rel) {                                           // aligned, and the granule holds a byte of the row
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(bytes + rel));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
}

// One value out of the LDS tile: `start` = tile coordinate of its first byte, nb = 1..10 bytes.
__device__ __forceinline__ int64_t tile_value(const uint32_t* tile32, int start, int nb) {
    const uint32_t* t32 = tile32 + (start >> 2);
    const uint32_t sh = (uint32_t)start & 3u;
    uint32_t d0 = __builtin_amdgcn_alignbyte(t32[1], t32[0], sh);       // bytes 0..3
    uint32_t d1 = __builtin_amdgcn_alignbyte(t32[2], t32[1], sh);       // bytes 4..7
    const uint32_t d2 = __builtin_amdgcn_alignbyte(t32[3], t32[2], sh); // bytes 8..9 (+2 foreign)
    // squeeze 4 x 7 bits per dword (the MSBs are dropped by the masks)
    d0 = (d0 & 0x007F007Fu) | ((d0 >> 1) & 0x3F803F80u);
    d1 = (d1 & 0x007F007Fu) | ((d1 >> 1) & 0x3F803F80u);
    d0 = (d0 & 0x00003FFFu) | ((d0 >> 2) & 0x0FFFC000u);
    d1 = (d1 & 0x00003FFFu) | ((d1 >> 2) & 0x0FFFC000u);
    uint64_t x = (uint64_t)d0 | ((uint64_t)d1 << 28);                   // 56 bits of bytes 0..7
    const int keep = 7 * (nb < 8 ? nb : 8);                             // bits that belong to this value
    x = (x << (64 - keep)) >> (64 - keep);
    const uint32_t top = (nb > 8 ? (d2 & 0x7Fu) : 0u) | (nb > 9 ? (d2 & 0x100u) >> 1 : 0u);   // byte 8, bit 0 of byte 9
    x |= (uint64_t)top << 56;
    return (int64_t)((x >> 1) ^ (uint64_t)(-(int64_t)(x & 1)));         // zig-zag
}

// What a RowStream does to a chunk between the load and the decode.  The rows of the plaintext kernels are what they are:
struct PlainBytes {
    __device__ __forceinline__ void begin_group(uint64_t) {}
    __device__ __forceinline__ void apply(uint4&, int, bool) const {}
};

// A row being streamed by one wave.  next_group() decodes up to kStreamDepth chunks and hands every value to
// sink(column, value); the state between calls is the column index, the continuation bitmap of the last 16 bytes,
// the halo in the wave's LDS tile and the prefetched chunks.  Crypt: PlainBytes, or the XSalsa20 keystream of a sealed
// box (XSalsaBytes below), xor-ed into the chunk while it is in registers.
template <class Crypt>
struct RowStreamT {
    const uint8_t* bytes;
    int64_t rel0, end_rel;            // this lane's byte offset in chunk 0; end of the row
    int lo0;                          // bytes of this lane that precede the row in chunk 0 (0..16)
    uint64_t n_chunks, j0, len, col;
    uint32_t carry_prev, flags;
    uint32_t* tile32;
    uint4 w[kStreamDepth];
    Crypt crypt;

    __device__ __forceinline__ void open(const uint8_t* __restrict__ bytes_, uint64_t a, uint64_t b, uint64_t len_, uint8_t* tile) {
        const int lane = threadIdx.x & 63;
        bytes = bytes_;
        const uintptr_t start_addr = (uintptr_t)bytes + a;
        const uintptr_t base0 = start_addr & ~(uintptr_t)15;
        n_chunks = ((uintptr_t)bytes + b - base0 + 1023) / 1024;
        rel0 = (int64_t)(base0 - (uintptr_t)bytes) + lane * 16;
        end_rel = (int64_t)b;
        const int64_t before = (int64_t)a - rel0;
        lo0 = before <= 0 ? 0 : (before >= 16 ? 16 : (int)before);
        j0 = 0; len = len_; col = 0; carry_prev = 0; flags = 0;   // before the row every byte "terminates"
        tile32 = reinterpret_cast<uint32_t*>(tile);
#pragma unroll
        for (int d = 0; d < kStreamDepth; ++d) w[d] = stream_load(bytes, rel0 + (int64_t)d * 1024, end_rel);
    }
    __device__ __forceinline__ bool done() const { return j0 >= n_chunks; }

    template <class Sink>
    __device__ __forceinline__ void next_group(Sink&& sink) {
        const int lane = threadIdx.x & 63;
        crypt.begin_group(j0);
#pragma unroll
        for (int d = 0; d < kStreamDepth; ++d) {
            const uint64_t j = j0 + d;
            if (j >= n_chunks) continue;                          // wave-uniform
            uint4 cur = w[d];
            // Refill the slot only after `cur` has landed: the variable number of stores in the decode loop makes
            // the compiler wait for EVERY outstanding memory operation (vmcnt(0)) at the first use of `cur`; the
            // empty asm is that first use, so the wait sits before the new load, which then has a whole chunk's
            // work to arrive while the other kStreamDepth - 1 slots have long been in flight.
            asm volatile("" : "+v"(cur.x), "+v"(cur.y), "+v"(cur.z), "+v"(cur.w));
            __builtin_amdgcn_sched_barrier(0);
            w[d] = stream_load(bytes, rel0 + (int64_t)(j + kStreamDepth) * 1024, end_rel);
            __builtin_amdgcn_sched_barrier(0);
            crypt.apply(cur, d, rel0 + (int64_t)j * 1024 < end_rel);   // the 0x80 fill past the row is not ciphertext
            uint32_t own = cont_bits16(cur), terms = ~own & 0xFFFFu;
            if (j == 0 || j + 1 >= n_chunks) {                    // wave-uniform: only the edge chunks hold foreign bytes
                const int64_t q = rel0 + (int64_t)j * 1024;
                const int lo = j == 0 ? lo0 : 0;
                const int hi = q >= end_rel ? 0 : (end_rel - q >= 16 ? 16 : (int)(end_rel - q));
                const uint32_t below_lo = (1u << lo) - 1u;
                own &= ~below_lo;                                 // bytes before the row stop the look-back
                terms = ~own & ((1u << hi) - 1u) & ~below_lo & 0xFFFFu;
            }
            const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)carry_prev, (int)own, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
            carry_prev = __builtin_amdgcn_readlane(own, 63);
            const uint32_t cnt = __builtin_popcount(terms);
            const uint32_t incl = wave_incl_scan(cnt);
            const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
            uint64_t g = col + (incl - cnt);
            // stage the chunk behind the halo (LDS operations of one wave execute in order)
            tile32[4 + lane * 4 + 0] = cur.x; tile32[4 + lane * 4 + 1] = cur.y;
            tile32[4 + lane * 4 + 2] = cur.z; tile32[4 + lane * 4 + 3] = cur.w;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t cont = (own << 16) | prev;
            uint32_t t = terms;
            while (t) {
                const int k = __builtin_ctz(t);
                t &= t - 1;
                const int e = 16 + k;
                const uint32_t below = ~cont & ((1u << e) - 1u);
                const int prev_term = 31 - __builtin_clz(below | 1u);   // none in the window: nb >= 16, refused either way
                int nb = e - prev_term;
                if (nb > 10) { flags |= SDA_VARINT_MALFORMED; nb = 10; }
                const int64_t v = tile_value(tile32, 16 + lane * 16 + k - (nb - 1), nb);
                if (g < len) sink(g, v);
                ++g;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane == 63) { tile32[0] = cur.x; tile32[1] = cur.y; tile32[2] = cur.z; tile32[3] = cur.w; }   // next halo
            col += total;
        }
        j0 += kStreamDepth;
    }
    // row verdict once the stream is exhausted
    __device__ __forceinline__ void close(uint32_t* __restrict__ status) {
        if (col != len) flags |= SDA_VARINT_ROW_COUNT;
        if (flags) atomicOr(status, flags);
    }
};

using RowStream = RowStreamT<PlainBytes>;

struct StoreSink {
    int64_t* row;
    __device__ __forceinline__ void operator()(uint64_t c, int64_t v) const { row[c] = v; }
};

// row checks shared by the streaming kernels; true = stream the row
__device__ __forceinline__ bool stream_row_range(const uint8_t* __restrict__ bytes, uint64_t n_bytes,
                                                 const RowRanges& rr, uint64_t r, uint64_t len,
                                                 uint32_t* __restrict__ status, uint64_t& a, uint64_t& b) {
    const bool lead = (threadIdx.x & 63) == 0;
    if (rr.lengths) {
        a = r * rr.slot; b = a + rr.lengths[r];
        if (rr.lengths[r] > rr.slot) { if (lead) atomicOr(status, SDA_VARINT_ROW_COUNT); return false; }   // a row never leaves its slot
    } else { a = rr.offsets ? rr.offsets[r] : 0; b = rr.offsets ? rr.offsets[r + 1] : n_bytes; }
    if (b < a || b > n_bytes) { if (lead) atomicOr(status, SDA_VARINT_ROW_COUNT); return false; }
    if (len == 0) { if (a != b && lead) atomicOr(status, SDA_VARINT_ROW_COUNT); return false; }
    if (a == b || (bytes[b - 1] & 0x80u)) { if (lead) atomicOr(status, SDA_VARINT_UNTERMINATED); return false; }
    return true;
}

__global__ __launch_bounds__(kStreamWaves * 64) void varint_stream_decode_kernel(const uint8_t* __restrict__ bytes,
                                                                                 uint64_t n_bytes, RowRanges offsets,
                                                                                 uint64_t rows, uint64_t len,
                                                                                 uint64_t row_stride,
                                                                                 int64_t* __restrict__ out,
                                                                                 uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[kStreamWaves][kStreamTile];
    const int wave = threadIdx.x >> 6;
    const uint64_t r = (uint64_t)blockIdx.x * kStreamWaves + wave;
    if (r >= rows) return;
    uint64_t a, b;
    if (!stream_row_range(bytes, n_bytes, offsets, r, len, status, a, b)) return;
    RowStream rs;
    rs.open(bytes, a, b, len, tiles[wave]);
    const StoreSink sink{out + r * row_stride};
    while (!rs.done()) rs.next_group(sink);
    rs.close(status);
}

// ---- single-pass encode into slots ------------------------------------------------------------------------------
// The mirror image: one wave encodes one row, 128 values (2 per lane, one 16-byte load) per step, four steps
// prefetched.  Byte positions inside a step come from a wave scan of the lengths; each value's <= 10 bytes are
// shifted to their byte phase and OR-ed into the wave's zeroed LDS tile (neighbours share boundary dwords), and the
// tile leaves as aligned 16-byte stores.  The up to 15 bytes that do not fill a 16-byte unit are carried into
// the next step's tile, so every global store but the row's last few bytes is a full aligned unit.  The row's byte
// count is only known at the end, hence the slotted output (row r at r * slot): each vector is sealed on its own
// anyway (sodium.rs:36-43), so contiguity of the rows has no meaning on the wire.
static constexpr int kEncVals = 128;
static constexpr int kEncTile = 16 + kEncVals * 10 + 32;      // carry | bytes | slack for the last value's dwords

__device__ __forceinline__ void value_bytes(uint64_t zz, uint32_t len, uint32_t& b0, uint32_t& b1, uint32_t& b2) {
    uint32_t d0 = (uint32_t)zz & 0x0FFFFFFFu, d1 = (uint32_t)(zz >> 28) & 0x0FFFFFFFu;   // 2 x 28 bits -> 2 x 4 bytes
    d0 = (d0 & 0x00003FFFu) | ((d0 & 0x0FFFC000u) << 2);
    d1 = (d1 & 0x00003FFFu) | ((d1 & 0x0FFFC000u) << 2);
    d0 = (d0 & 0x007F007Fu) | ((d0 & 0x3F803F80u) << 1);
    d1 = (d1 & 0x007F007Fu) | ((d1 & 0x3F803F80u) << 1);
    const uint32_t d2 = ((uint32_t)(zz >> 56) & 0x7Fu) | ((uint32_t)(zz >> 63) << 8);     // bytes 8 and 9
    // continuation bit on every byte but the last one
    const uint64_t cont = len >= 9 ? 0x8080808080808080ull : (0x0080808080808080ull >> (8 * ((8 - len) & 7)));   // len 0: unused
    b0 = d0 | (uint32_t)cont;
    b1 = d1 | (uint32_t)(cont >> 32);
    b2 = d2 | (len > 9 ? 0x80u : 0u);
    if (len == 0) { b0 = 0; b1 = 0; b2 = 0; }
}

__device__ __forceinline__ void tile_or(uint32_t* tile32, uint32_t pos, uint32_t b0, uint32_t b1, uint32_t b2) {
    const uint32_t sh = 8u * (pos & 3u);
    const uint64_t lo = ((uint64_t)b1 << 32 | b0) << sh;                 // bytes 0..7 at their phase (low part)
    const uint64_t hi = (((uint64_t)b2 << 32) | b1) << sh;               // high dword: b2 and what left b1
    uint32_t* t = tile32 + (pos >> 2);
    atomicOr(t + 0, (uint32_t)lo);
    atomicOr(t + 1, (uint32_t)(lo >> 32));
    atomicOr(t + 2, (uint32_t)(hi >> 32));
    if (sh) atomicOr(t + 3, (uint32_t)(((uint64_t)b2 << sh) >> 32));
}

__device__ __forceinline__ void enc_load2(const int64_t* __restrict__ src, uint64_t len, bool vec, uint64_t i, int64_t& x,
                                          int64_t& y) {
    x = 0; y = 0;
    if (i + 1 < len && vec) {
        typedef long long ll2v __attribute__((ext_vector_type(2)));
        const ll2v v = __builtin_nontemporal_load(reinterpret_cast<const ll2v*>(src + i));
        x = v.x; y = v.y;
    } else {
        if (i < len) x = src[i];
        if (i + 1 < len) y = src[i + 1];
    }
}

// Where the encode loop's values come from.  Lane l of step j holds values 128 j + 2 l and 128 j + 2 l + 1; get(d, j, x, y) hands
// them over (d = j % kStreamDepth, a compile-time constant after unrolling).  LoadValues: a row in global memory, one 16-byte
// load per lane and step, kStreamDepth steps prefetched.
struct LoadValues {
    static constexpr int kDepth = kStreamDepth;
    const int64_t* __restrict__ src;
    uint64_t len;
    bool vec;
    int64_t wx[kStreamDepth], wy[kStreamDepth];
    __device__ __forceinline__ void open(const int64_t* __restrict__ src_, uint64_t len_) {
        const int lane = threadIdx.x & 63;
        src = src_; len = len_;
        vec = (((uintptr_t)src) & 15u) == 0;
#pragma unroll
        for (int d = 0; d < kStreamDepth; ++d) enc_load2(src, len, vec, (uint64_t)d * kEncVals + 2 * (uint64_t)lane, wx[d], wy[d]);
    }
    __device__ __forceinline__ void get(int d, uint64_t j, int64_t& x, int64_t& y) {
        const int lane = threadIdx.x & 63;
        x = wx[d]; y = wy[d];
        asm volatile("" : "+v"(x), "+v"(y));
        __builtin_amdgcn_sched_barrier(0);
        enc_load2(src, len, vec, (j + kStreamDepth) * kEncVals + 2 * (uint64_t)lane, wx[d], wy[d]);
        __builtin_amdgcn_sched_barrier(0);
    }
};

// What the encode loop does to a 16-byte unit between the LDS tile and the global store.  Unit u of a row is its bytes
// [16 u, 16 u + 16).  The rows of the plaintext kernel leave as they are:
struct EncPlain {
    __device__ __forceinline__ bool ends_before(uint64_t) const { return false; }
    __device__ __forceinline__ bool holds(uint64_t) const { return true; }
    __device__ __forceinline__ void refill() {}
    __device__ __forceinline__ void apply(uint4&, uint64_t) const {}
};

// One wave encodes the `len` values of `vals` as row r to dst (16-byte aligned) and stores its byte count in row_bytes[r].
// Values: LoadValues, or ShareValues below (the row's shares computed from the secrets and the draws).  Crypt: EncPlain, or the
// XSalsa20 keystream of the row's sealed box (EncXSalsa below), xor-ed into every unit on its way from the tile to global
// memory.  The write cursor depends on the data (a step emits 8..81 units), so the keystream follows the cursor: a step whose
// units reach past what the keystream tile holds stores the units it still covers, refills, and stores the rest.
template <class Values, class Crypt>
__device__ __forceinline__ void encode_row(Values& vals, uint64_t len, uint64_t r, uint8_t* __restrict__ dst, uint8_t* tile,
                                           uint64_t* __restrict__ row_bytes, Crypt& crypt) {
    const int lane = threadIdx.x & 63;
    uint32_t* tile32 = reinterpret_cast<uint32_t*>(tile);
    uint4* tile128 = reinterpret_cast<uint4*>(tile);
    const uint64_t n_steps = (len + kEncVals - 1) / kEncVals;
    uint64_t cur = 0;                 // bytes of this row already in global memory (multiple of 16)
    uint32_t cb = 0;                  // carried bytes (< 16), held by lane 0 in `carry`
    uint4 carry = make_uint4(0, 0, 0, 0);
    for (uint64_t j0 = 0; j0 < n_steps; j0 += Values::kDepth) {
#pragma unroll
        for (int d = 0; d < Values::kDepth; ++d) {
            const uint64_t j = j0 + d;
            if (j >= n_steps) continue;
            int64_t x, y;
            vals.get(d, j, x, y);
            const uint64_t i = j * kEncVals + 2 * (uint64_t)lane;
            const uint64_t zx = zigzag(x), zy = zigzag(y);
            const uint32_t lx = i < len ? varint_len(zx) : 0u, ly = i + 1 < len ? varint_len(zy) : 0u;
            const uint32_t cnt = lx + ly;
            const uint32_t incl = wave_incl_scan(cnt);
            const uint32_t T = __builtin_amdgcn_readlane(incl, 63);
            const uint32_t pos = cb + incl - cnt;
            // zero the tile, put the carried bytes in front
            const bool first = lane == 0;
            tile128[lane] = make_uint4(first ? carry.x : 0u, first ? carry.y : 0u, first ? carry.z : 0u, first ? carry.w : 0u);
            if (lane + 64 < kEncTile / 16) tile128[lane + 64] = make_uint4(0, 0, 0, 0);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint32_t b0, b1, b2;
            value_bytes(zx, lx, b0, b1, b2);
            tile_or(tile32, pos, b0, b1, b2);
            value_bytes(zy, ly, b0, b1, b2);
            tile_or(tile32, pos + lx, b0, b1, b2);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t have = cb + T, units = have >> 4;              // <= 81 units
            uint4* g = reinterpret_cast<uint4*>(dst + cur);
            bool s0 = (uint32_t)lane < units, s1 = (uint32_t)lane + 64 < units;
            const uint64_t u0 = (cur >> 4) + (uint32_t)lane;              // this lane's units: u0 and u0 + 64
            if (crypt.ends_before((cur >> 4) + units)) {                  // wave-uniform: the step straddles a refill
                if (s0 && crypt.holds(u0)) { uint4 v = tile128[lane]; crypt.apply(v, u0); g[lane] = v; s0 = false; }
                if (s1 && crypt.holds(u0 + 64)) { uint4 v = tile128[lane + 64]; crypt.apply(v, u0 + 64); g[lane + 64] = v; s1 = false; }
                crypt.refill();
            }
            if (s0) { uint4 v = tile128[lane]; crypt.apply(v, u0); g[lane] = v; }
            if (s1) { uint4 v = tile128[lane + 64]; crypt.apply(v, u0 + 64); g[lane + 64] = v; }
            const uint4 next = tile128[units];                            // bytes past `have` are zero
            carry = make_uint4(__builtin_amdgcn_readfirstlane(next.x), __builtin_amdgcn_readfirstlane(next.y),
                               __builtin_amdgcn_readfirstlane(next.z), __builtin_amdgcn_readfirstlane(next.w));
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            cur += (uint64_t)units * 16;
            cb = have & 15u;
        }
    }
    // the last bytes of the row: a partial unit of its own
    if (cb) {
        if (crypt.ends_before((cur >> 4) + 1)) crypt.refill();
        crypt.apply(carry, cur >> 4);
    }
    if ((uint32_t)lane < cb) {
        const uint32_t wsel = lane >> 2;
        const uint32_t word = wsel == 0 ? carry.x : wsel == 1 ? carry.y : wsel == 2 ? carry.z : carry.w;
        dst[cur + lane] = (uint8_t)(word >> (8 * (lane & 3)));
    }
    if (lane == 0) row_bytes[r] = cur + cb;
}

__global__ __launch_bounds__(kStreamWaves * 64) void varint_stream_encode_kernel(VarintRows R, uint8_t* __restrict__ out,
                                                                                 uint64_t slot,
                                                                                 uint64_t* __restrict__ row_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[kStreamWaves][kEncTile];
    const int wave = threadIdx.x >> 6;
    const uint64_t r = (uint64_t)blockIdx.x * kStreamWaves + wave;
    if (r >= R.rows) return;
    EncPlain crypt;
    LoadValues vals;
    vals.open(R.values + r * R.row_stride, R.len);
    encode_row(vals, R.len, r, out + r * slot, tiles[wave], row_bytes, crypt);
}

// ---- wire format -> clerk sums without the decoded tile ---------------------------------
// The 16 (or 8) waves of a workgroup stream as many rows of ONE job in lockstep (a group of kStreamDepth chunks each, then a
// barrier).  Values go into a sliding window of kCombWindow columns in LDS, two 64-bit planes per column (sum of
// the low 32 bits, sum of the arithmetic high 32 bits: no carries, plain ds_add_u64).  After every group the columns
// below min(current column of the 16 rows) can no longer be touched: they are folded into (lo, hi) and added to
// the global 128-bit accumulators, one pair of atomics per column and workgroup.  A value beyond the window (rows
// drifting apart by more than ~1500 columns: only with wildly different value sizes) goes to the global
// accumulator directly, so the result is exact for any input.
static constexpr int kCombWindow = 2048;

struct WindowSink {
    unsigned long long* lo32; unsigned long long* hi32;   // LDS planes
    uint64_t base;                                         // first column of the window
    uint64_t* acc_lo; int64_t* acc_hi;                     // this job's accumulators
    __device__ __forceinline__ void operator()(uint64_t c, int64_t v) const {
        if (c - base < (uint64_t)kCombWindow) {
            const uint32_t i = (uint32_t)c & (kCombWindow - 1);
            atomicAdd(&lo32[i], (unsigned long long)((uint64_t)v & 0xFFFFFFFFull));
            atomicAdd(&hi32[i], (unsigned long long)(v >> 32));
        } else {
            acc_atomic_add(acc_lo + c, acc_hi + c, (uint64_t)v, v >> 63);
        }
    }
};

// After a group: the columns below min(current column of the workgroup's rows) can no longer be touched - fold them and add
// them to the global accumulators, slide the window.  Called by every thread after cols[] is written and a barrier; true = every
// row is through.  Shared by the plaintext and the sealed kernel.
template <int kCombWaves>
__device__ __forceinline__ bool window_flush(unsigned long long* lo32, unsigned long long* hi32, WindowSink& sink, const uint64_t* cols,
                                             uint64_t len) {
    uint64_t nb = len;
#pragma unroll
    for (int w = 0; w < kCombWaves; ++w) nb = cols[w] < nb ? cols[w] : nb;
    // every later value has column >= nb: fold and flush [base, nb)
    uint64_t end = nb < sink.base + kCombWindow ? nb : sink.base + kCombWindow;
    for (uint64_t c = sink.base + threadIdx.x; c < end; c += kCombWaves * 64) {
        const uint32_t i = (uint32_t)c & (kCombWindow - 1);
        const uint64_t A = lo32[i];
        const int64_t Bq = (int64_t)hi32[i];
        if (A | (uint64_t)Bq) {
            lo32[i] = 0; hi32[i] = 0;
            const uint64_t lo = A + ((uint64_t)Bq << 32);
            acc_atomic_add(sink.acc_lo + c, sink.acc_hi + c, lo, (Bq >> 32) + (lo < A ? 1 : 0));
        }
    }
    sink.base = nb;
    __syncthreads();
    return nb >= len;
}

template <int kCombWaves>       // rows per workgroup: 16 (one pair of global atomics per column and 16 rows), 8 when rows are few
__global__ __launch_bounds__(kCombWaves * 64) void varint_stream_combine_kernel(
    const uint8_t* __restrict__ bytes, uint64_t n_bytes, RowRanges offsets, uint64_t rows_per_job,
    uint64_t groups_per_job, uint64_t len, uint64_t* __restrict__ acc_lo, int64_t* __restrict__ acc_hi,
    uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[kCombWaves][kStreamTile];
    __shared__ unsigned long long lo32[kCombWindow], hi32[kCombWindow];
    __shared__ uint64_t cols[kCombWaves];
    const int wave = threadIdx.x >> 6;
    const uint64_t job = blockIdx.x / groups_per_job, grp = blockIdx.x - job * groups_per_job;
    const uint64_t rj = grp * kCombWaves + wave;                  // row inside the job
    for (int i = threadIdx.x; i < kCombWindow; i += kCombWaves * 64) { lo32[i] = 0; hi32[i] = 0; }
    RowStream rs;
    bool live = false;
    if (rj < rows_per_job) {
        uint64_t a, b;
        live = stream_row_range(bytes, n_bytes, offsets, job * rows_per_job + rj, len, status, a, b);
        if (live) rs.open(bytes, a, b, len, tiles[wave]);
    }
    WindowSink sink{lo32, hi32, 0, acc_lo + job * len, acc_hi + job * len};
    __syncthreads();
    for (;;) {
        if (live) {
            rs.next_group(sink);
            if (rs.done()) { rs.close(status); live = false; }
        }
        if ((threadIdx.x & 63) == 0) cols[wave] = live ? rs.col : len;     // a finished row no longer holds the window
        __syncthreads();
        if (window_flush<kCombWaves>(lo32, hi32, sink, cols, len)) break;     // all 16 rows are through
    }
}

// ---- sealed boxes -> clerk sums without the plaintext (clerk.rs:78-86 in one pass over the ciphertext) -----------------
// The same kernel over rows that are still XSalsa20 ciphertext: row r is the payload of the sealed box at
// boxes + r * slot (epk 32 | tag 16 | ciphertext), whose tag the sealed-box verify pass has ALREADY checked - a row whose
// state says `bad` is not streamed, so no byte decrypted from an unauthenticated box reaches an accumulator.  The
// keystream is xor-ed into a chunk while it sits in registers; decrypted bytes exist in registers and LDS only.
//
// Geometry: the ciphertext starts at box offset 48 (16-byte aligned), message byte m is stream byte 32 + m (stream bytes
// 0..31 are the Poly1305 key), so lane l of chunk j holds the 16-byte stream piece 2 + 64 j + l and a group of
// kStreamDepth = 4 chunks spans the Salsa20 blocks 64 g (second half) .. 64 g + 64 (first half).  Per group lane l
// computes block 64 g + 1 + l into slot 1 + l of the wave's keystream tile; slot 0 is the previous group's slot 64
// (block 0 at open).  The tile is transposed ([word][slot]) so that the stores are lane-contiguous, with a slot stride
// of 66 words: the four pieces of a block are then 8 banks apart (4 * 66 = 8 mod 32) and the 32 lanes of a
// ds_read_b32 group - eight slots, four pieces each - fall on 32 different banks.
static constexpr int kKsStride = 66;
static constexpr int kKsTile = 16 * kKsStride;              // words per wave

struct XSalsaBytes {
    uint32_t key[8], n0, n1;                               // wave-uniform: the box's XSalsa20 subkey and nonce tail
    uint32_t* ks;
    __device__ __forceinline__ void open(const SboxState& st, uint32_t* tile) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int i = 0; i < 8; ++i) key[i] = st.subkey[i];
        n0 = st.n0; n1 = st.n1;
        ks = tile;
        // (wave-uniform inputs: all 64 lanes compute the same block and one stores it - once per row, against one block per
        // lane and group in the stream; likewise byte_at below)
        uint32_t b[16];
        sbx::salsa20_block(b, key, n0, n1, 0);             // block 0 into slot 64: the first group's carry moves it to slot 0
        if (lane == 0) {
#pragma unroll
            for (int w = 0; w < 16; ++w) ks[w * kKsStride + 64] = b[w];
        }
    }
    __device__ __forceinline__ void begin_group(uint64_t j0) {
        const int lane = threadIdx.x & 63;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the previous group's reads are done, open()'s store is in
        __builtin_amdgcn_wave_barrier();
        if (lane < 16) ks[lane * kKsStride] = ks[lane * kKsStride + 64];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t b[16];
        sbx::salsa20_block(b, key, n0, n1, 16 * j0 + 1 + (uint64_t)lane);   // j0 = 4 g
#pragma unroll
        for (int w = 0; w < 16; ++w) ks[w * kKsStride + 1 + lane] = b[w];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void apply(uint4& cur, int d, bool ciphertext) const {
        const uint32_t p = 2u + 64u * (uint32_t)d + (threadIdx.x & 63u);    // stream piece inside the group
        const uint32_t* k = ks + (p & 3u) * 4u * kKsStride + (p >> 2);
        if (ciphertext) {
            cur.x ^= k[0]; cur.y ^= k[kKsStride]; cur.z ^= k[2 * kKsStride]; cur.w ^= k[3 * kKsStride];
        }
    }
    // one decrypted message byte (wave-uniform m): the row's last byte decides "unterminated" before the row is streamed
    __device__ __forceinline__ uint32_t byte_at(uint8_t c, uint64_t m) const {
        const uint64_t sp = m + 32;
        uint32_t b[16];
        sbx::salsa20_block(b, key, n0, n1, sp >> 6);
        uint32_t word = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) word = ((uint32_t)(sp >> 2) & 15u) == (uint32_t)w ? b[w] : word;
        return (c ^ (word >> (8 * (uint32_t)(sp & 3)))) & 0xFFu;
    }
};

// Row r of a sealed job, for the wave that streams it: true = `rs` is open on the row's ciphertext.  A box the verify pass refused
// (tag, length, all-zero shared secret) carries `bad`; the length is tested again here so that the row can never leave its slot
// whatever the state says.  The other refusals are the verdicts of stream_row_range on the plaintext this row would have been
// opened to.
__device__ __forceinline__ bool sealed_row_open(RowStreamT<XSalsaBytes>& rs, const uint8_t* __restrict__ boxes, uint64_t slot,
                                                const uint64_t* __restrict__ row_bytes, uint64_t max_box,
                                                const SboxState* __restrict__ states, uint64_t r, uint64_t len,
                                                uint32_t* __restrict__ status, uint8_t* tile, uint32_t* kstream) {
    const bool lead = (threadIdx.x & 63) == 0;
    const uint64_t have = row_bytes[r];
    if (!(have >= 48 && have <= max_box && have <= slot && !states[r].bad)) return false;
    const uint64_t a = r * slot + 48, b = r * slot + have;
    if (len == 0) { if (a != b && lead) atomicOr(status, SDA_VARINT_ROW_COUNT); return false; }
    if (a == b) { if (lead) atomicOr(status, SDA_VARINT_UNTERMINATED); return false; }
    rs.crypt.open(states[r], kstream);
    if (rs.crypt.byte_at(boxes[b - 1], b - 1 - a) & 0x80u) { if (lead) atomicOr(status, SDA_VARINT_UNTERMINATED); return false; }
    rs.open(boxes, a, b, len, tile);
    return true;
}

template <int kCombWaves>
__global__ __launch_bounds__(kCombWaves * 64) void sealed_stream_combine_kernel(
    const uint8_t* __restrict__ boxes, uint64_t slot, const uint64_t* __restrict__ row_bytes, uint64_t max_box,
    const SboxState* __restrict__ states, uint64_t rows, uint64_t len, uint64_t* __restrict__ acc_lo,
    int64_t* __restrict__ acc_hi, uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[kCombWaves][kStreamTile];
    __shared__ uint32_t kstream[kCombWaves][kKsTile];
    __shared__ unsigned long long lo32[kCombWindow], hi32[kCombWindow];
    __shared__ uint64_t cols[kCombWaves];
    const int wave = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
    const uint64_t r = (uint64_t)blockIdx.x * kCombWaves + wave;
    for (int i = threadIdx.x; i < kCombWindow; i += kCombWaves * 64) { lo32[i] = 0; hi32[i] = 0; }
    RowStreamT<XSalsaBytes> rs;
    bool live = r < rows && sealed_row_open(rs, boxes, slot, row_bytes, max_box, states, r, len, status, tiles[wave], kstream[wave]);
    WindowSink sink{lo32, hi32, 0, acc_lo, acc_hi};
    __syncthreads();
    for (;;) {
        if (live) {
            rs.next_group(sink);
            if (rs.done()) { rs.close(status); live = false; }
        }
        if (lead) cols[wave] = live ? rs.col : len;               // a finished row no longer holds the window
        __syncthreads();
        if (window_flush<kCombWaves>(lo32, hi32, sink, cols, len)) break;
    }
}

// ---- sealed clerking results -> secrets (receive.rs:120-146: decrypt every clerking result, then reconstruct) ------------------
// Packed reconstruction is a fixed k x n' matrix R per clerk-index set, so secret[b k + s] = sum over rows i of
// R[s][i] * share_i[b] mod q: a WEIGHTED clerk sum, and a row can be folded in on its own, in any order, once its coefficient
// column is known.  The sealed kernel above with a Montgomery multiply between the decoder and the window: the sink reduces a
// value (any int64) to its canonical residue, multiplies it by the k coefficients of the row's position (Montgomery form, so
// the REDC of the product is the canonical R[s][i] * v mod q, below 2^62) and adds the k products to the outputs b k + s.  The
// window slides over OUTPUT columns; a product beyond it goes to the global 128-bit accumulator directly, so the sums are exact
// however far rows drift apart, and at most 65535 rows of products below 2^63 cannot overflow them.  The fold mod q happens
// once, at finish.  With k = 100 a 4 KiB group of a row spans far more outputs than the window holds: most products of such a
// shape take the direct path.
//
// The coefficients of position i are row i of the transposed matrix Rt [n'][k], contiguous.  k <= kCoefLds: the wave keeps its k
// coefficients in LDS.  Larger k (the shipped PSS_155 shapes have k = 100): read from Rt, the address is wave-uniform.
// LDS of the 8-wave instance: 8.3 KB of stream tiles + 33 KB of keystream tiles + 32 KB of window + 1 KB of coefficients =
// 75 KB, two workgroups in the 160 KB of a CU (the 16-wave form would leave room for one; it is not instantiated).
// One wave streams one row: a reveal of few, long rows has little parallelism.
static constexpr int kCoefLds = 16;

struct WeightedSink {
    WindowSink win;                   // over output columns b k + s
    const uint64_t* coef;             // the k coefficients of this wave's row
    uint32_t k;
    uint64_t batches, m, mu, pinv;
    __device__ __forceinline__ void operator()(uint64_t b, int64_t v) const {
        if (b >= batches) return;     // past ceil(dimension / k): decoded for validity, otherwise ignored
        const uint64_t x = canon_i64(v, m, mu);
        const uint64_t c = b * k;
        for (uint32_t s = 0; s < k; ++s) win(c + s, (int64_t)mont_redc(mul64x64(coef[s], x), m, pinv));
    }
};

template <int kCombWaves, bool kLds>
__global__ __launch_bounds__(kCombWaves * 64) void sealed_stream_weighted_kernel(
    const uint8_t* __restrict__ boxes, uint64_t slot, const uint64_t* __restrict__ row_bytes, uint64_t max_box,
    const SboxState* __restrict__ states, uint64_t rows, uint64_t len, uint64_t first_pos, WeightedJob J,
    uint64_t* __restrict__ acc_lo, int64_t* __restrict__ acc_hi, uint32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[kCombWaves][kStreamTile];
    __shared__ uint32_t kstream[kCombWaves][kKsTile];
    __shared__ unsigned long long lo32[kCombWindow], hi32[kCombWindow];
    __shared__ uint64_t cols[kCombWaves];
    __shared__ uint32_t alive[kCombWaves];
    __shared__ uint64_t coefs[kLds ? kCombWaves : 1][kCoefLds];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const bool lead = lane == 0;
    const uint64_t r = (uint64_t)blockIdx.x * kCombWaves + wave;
    const uint64_t total = J.batches * J.k;                      // outputs = accumulators (the last batch is padded)
    for (int i = threadIdx.x; i < kCombWindow; i += kCombWaves * 64) { lo32[i] = 0; hi32[i] = 0; }
    const uint64_t* coef = J.Rt + (first_pos + (r < rows ? r : 0)) * J.k;
    if (kLds) {
        if (r < rows && (uint32_t)lane < J.k) coefs[wave][lane] = coef[lane];
        coef = coefs[wave];
    }
    RowStreamT<XSalsaBytes> rs;
    bool live = r < rows && sealed_row_open(rs, boxes, slot, row_bytes, max_box, states, r, len, status, tiles[wave], kstream[wave]);
    WeightedSink sink{{lo32, hi32, 0, acc_lo, acc_hi}, coef, J.k, J.batches, J.m, J.mu, J.pinv};
    __syncthreads();
    for (;;) {
        if (live) {
            rs.next_group(sink);
            if (rs.done()) { rs.close(status); live = false; }
        }
        if (lead) {
            // a row past its last batch no longer holds the window, but is streamed to its end: the surplus is validated
            cols[wave] = live && rs.col < J.batches ? rs.col * J.k : total;
            alive[wave] = live;
        }
        __syncthreads();
        uint32_t any = 0;
#pragma unroll
        for (int w = 0; w < kCombWaves; ++w) any |= alive[w];
        const bool flushed = window_flush<kCombWaves>(lo32, hi32, sink.win, cols, total);   // ends on a barrier: alive[] is read
        if (flushed && !any) break;
    }
}

// The plaintext-row sibling: rows already decoded, [rows][row_stride] int64.  One lane per batch, the rows of the call in a loop:
// the un-reduced 128-bit dot product of packed_reconstruct_kernel over THIS call's rows, one REDC, one add to the accumulators.
__global__ __launch_bounds__(kVT) void weighted_rows_kernel(const int64_t* __restrict__ shares, uint64_t row_stride, uint32_t rows,
                                                            uint64_t first_pos, WeightedJob J, uint64_t* __restrict__ acc_lo,
                                                            int64_t* __restrict__ acc_hi, uint32_t e_per_group) {
    const uint64_t b = (uint64_t)blockIdx.x * kVT + threadIdx.x;
    if (b >= J.batches) return;
    const uint32_t e0 = blockIdx.y * e_per_group, e1 = e0 + e_per_group < J.k ? e0 + e_per_group : J.k;
    for (uint32_t e = e0; e < e1; ++e) {
        U128 acc{0, 0};
        uint32_t since = 0;
        for (uint32_t c = 0; c < rows; ++c) {
            const uint64_t v = canon_i64(shares[(uint64_t)c * row_stride + b], J.m, J.mu);
            mac128(acc, J.Rt[(first_pos + c) * J.k + e], v);
            if (++since == 4) { mont_acc_condsub(acc, J.m); since = 0; }
        }
        mont_acc_condsub(acc, J.m);
        const uint64_t o = b * J.k + e;
        acc_atomic_add(acc_lo + o, acc_hi + o, mont_redc(acc, J.m, J.pinv), 0);
    }
}

// R [k][n] -> Rt [n][k]
__global__ __launch_bounds__(kVT) void transpose_u64_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t k,
                                                            uint32_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kVT + threadIdx.x;
    if (i >= (uint64_t)k * n) return;
    const uint64_t pos = i / k, s = i - pos * k;
    out[i] = in[s * n + pos];
}

// ---- share rows -> sealed boxes without the wire buffer (participate.rs:82-101: encode_var every share, then seal) --------
// The encode kernel with the XSalsa20 keystream of the row's box xor-ed into every unit before it is stored: row r goes to
// boxes + r * slot + 48, where the ciphertext starts 16-byte aligned; plaintext varint bytes exist in registers and LDS only.
// The setup pass has written the box's epk and the per-row state; the Poly1305 pass over the ciphertext follows (its pieces
// are indexed from the END of the message, which is only known once the row is through).
//
// Geometry as above: unit u of the message is stream piece u + 2, Salsa20 block (u + 2) >> 2.  The wave keeps the 64 blocks
// base .. base + 63 in its keystream tile ([word][slot], slot stride 66 as XSalsaBytes); all 64 lanes refill it at once
// (block = base + lane) when the write cursor reaches its end - first at message byte 4064, then every 4096 bytes.
struct EncXSalsa {
    uint32_t key[8], n0, n1;                               // wave-uniform: the box's XSalsa20 subkey and nonce tail
    uint32_t* ks;
    uint64_t base;                                         // first block of the tile, a multiple of 64
    __device__ __forceinline__ void fill() {
        const int lane = threadIdx.x & 63;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the reads of the blocks being replaced are done
        __builtin_amdgcn_wave_barrier();
        uint32_t b[16];
        sbx::salsa20_block(b, key, n0, n1, base + (uint64_t)lane);
#pragma unroll
        for (int w = 0; w < 16; ++w) ks[w * kKsStride + lane] = b[w];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void open(const SboxState& st, uint32_t* tile) {
#pragma unroll
        for (int i = 0; i < 8; ++i) key[i] = st.subkey[i];
        n0 = st.n0; n1 = st.n1;
        ks = tile;
        base = 0;                                          // pieces 0 and 1 (the Poly1305 key) are computed and never read
        fill();
    }
    // units [.., unit_end) reach past the tile / unit u lies inside it (units only ever move forward)
    __device__ __forceinline__ bool ends_before(uint64_t unit_end) const { return unit_end + 2 > 4 * (base + 64); }
    __device__ __forceinline__ bool holds(uint64_t u) const { return u + 2 < 4 * (base + 64); }
    __device__ __forceinline__ void refill() { base += 64; fill(); }
    __device__ __forceinline__ void apply(uint4& v, uint64_t u) const {
        const uint32_t p = (uint32_t)(u + 2 - 4 * base);           // piece inside the tile, 0..255
        const uint32_t* k = ks + (p & 3u) * 4u * kKsStride + (p >> 2);
        v.x ^= k[0]; v.y ^= k[kKsStride]; v.z ^= k[2 * kKsStride]; v.w ^= k[3 * kKsStride];
    }
};

__global__ __launch_bounds__(kStreamWaves * 64) void varint_seal_stream_kernel(VarintRows R, uint8_t* __restrict__ boxes, uint64_t slot,
                                                                               const SboxState* __restrict__ states,
                                                                               uint64_t* __restrict__ msg_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[kStreamWaves][kEncTile];
    __shared__ uint32_t kstream[kStreamWaves][kKsTile];
    const int wave = threadIdx.x >> 6;
    const uint64_t r = (uint64_t)blockIdx.x * kStreamWaves + wave;
    if (r >= R.rows) return;
    // a row whose recipient key gave the all-zero shared secret is refused: nothing encoded, nothing encrypted under the
    // degenerate key; the final pass gives it length 0 and no tag
    if (states[r].bad) { if ((threadIdx.x & 63) == 0) msg_bytes[r] = 0; return; }
    EncXSalsa crypt;
    crypt.open(states[r], kstream[wave]);
    LoadValues vals;
    vals.open(R.values + r * R.row_stride, R.len);
    encode_row(vals, R.len, r, boxes + r * slot + 48, tiles[wave], msg_bytes, crypt);
}

// ---- secrets -> sealed clerking-job rows without the shares (participate.rs:75-101: share the secrets, seal every clerk's vector) ---
// The seal kernel above with the row's shares COMPUTED instead of loaded.  Row r = c * participants + p is clerk c's vector of
// participant p: one share per batch of k secrets.  The lane layout of the encode loop is the layout of the DPP-quad CSPRNG
// (drbg_quad.hpp): lane l of step j holds batches 2 * pair and 2 * pair + 1 with pair = 64 j + l, a quad holds one group of 8
// batches, so drbg_pair() gives the lane exactly the draws of its two batches.  All 64 lanes call it in every step - the lanes
// past the row's end too (a quad must be whole); encode_row gives their values the length 0.
//   additive      : clerk c < n - 1 gets draw c; the last clerk the secret minus all n - 1 draws (additive.rs:42-47)
//   packed Shamir : clerk c < direct_rows gets draw c (systematic share map); every other clerk the dot product of its matrix row
//                   with [k secrets ; t draws] - 128-bit sums folded every four terms, one REDC (as packed_gen_generic_kernel).
//                   The row's address is wave-uniform: its coefficients arrive through scalar loads.
// Every clerk wave derives the draws of its batches again: a participation costs up to n times the ChaCha blocks of
// generate_batch_dev (clerks that receive a draw itself compute one draw per batch, not t).
template <int ROUNDS>
struct ShareValues {
    static constexpr int kDepth = 1;          // nothing is prefetched: the step loop stays rolled
    const ShareJob& J;
    const int64_t* __restrict__ sp;          // the participant's secrets
    const uint64_t* __restrict__ row;        // packed, dot-product clerk: k + t coefficients (Montgomery form); else nullptr
    uint64_t stream;
    uint32_t T, draw;                         // draws per batch; draw >= T: not a clerk that receives a draw itself
    QuadCol qc;
    __device__ __forceinline__ ShareValues(const ShareJob& J_, uint32_t c, uint64_t p) : J(J_) {
        sp = J.secrets + p * J.secrets_stride;
        stream = J.first_participant + p;
        qc = quad_col(J.key);
        T = J.additive ? J.n - 1 : J.t;
        const uint32_t direct = J.additive ? J.n - 1 : J.direct_rows;
        draw = c < direct ? c : T;
        row = J.additive || c < direct ? nullptr : J.M + (uint64_t)(c - direct) * (J.k + J.t);
    }
    __device__ __forceinline__ void get(int, uint64_t j, int64_t& x, int64_t& y) {
        const uint64_t pair = j * (kEncVals / 2) + (threadIdx.x & 63u);
        const uint64_t b0 = 2 * pair;
        const uint64_t m = J.mod.m, mu = J.mod.mu;
        uint64_t r0, r1;
        if (draw < T) {                                               // wave-uniform, as every branch and loop bound below
            drbg_pair<ROUNDS>(J.key, qc, stream, pair, T, draw, J.mod, r0, r1);
            x = (int64_t)r0; y = (int64_t)r1;
            return;
        }
        if (J.additive) {
            uint64_t s0 = b0 < J.len ? canon_i64(sp[b0], m, mu) : 0;
            uint64_t s1 = b0 + 1 < J.len ? canon_i64(sp[b0 + 1], m, mu) : 0;
            for (uint32_t i = 0; i < T; ++i) {
                drbg_pair<ROUNDS>(J.key, qc, stream, pair, T, i, J.mod, r0, r1);
                s0 = submod(s0, r0, m);
                s1 = submod(s1, r1, m);
            }
            x = (int64_t)s0; y = (int64_t)s1;
            return;
        }
        U128 a0{0, 0}, a1{0, 0};
        uint32_t since = 0;
        const uint64_t e0 = b0 * J.k, e1 = e0 + J.k;                  // the last batch is zero padded (batched.rs:37-43)
        for (uint32_t i = 0; i < J.k; ++i) {
            const uint64_t v0 = e0 + i < J.len ? canon_i64(sp[e0 + i], m, mu) : 0;
            const uint64_t v1 = e1 + i < J.len ? canon_i64(sp[e1 + i], m, mu) : 0;
            const uint64_t cf = row[i];
            mac128(a0, cf, v0);
            mac128(a1, cf, v1);
            if (++since == 4) { mont_acc_condsub(a0, J.mont.p); mont_acc_condsub(a1, J.mont.p); since = 0; }
        }
        for (uint32_t i = 0; i < T; ++i) {
            drbg_pair<ROUNDS>(J.key, qc, stream, pair, T, i, J.mod, r0, r1);
            const uint64_t cf = row[J.k + i];
            mac128(a0, cf, r0);
            mac128(a1, cf, r1);
            if (++since == 4) { mont_acc_condsub(a0, J.mont.p); mont_acc_condsub(a1, J.mont.p); since = 0; }
        }
        mont_acc_condsub(a0, J.mont.p);
        mont_acc_condsub(a1, J.mont.p);
        x = (int64_t)mont_redc(a0, J.mont.p, J.mont.pinv);
        y = (int64_t)mont_redc(a1, J.mont.p, J.mont.pinv);
    }
};

// One wave per row.  by_rows == 0: the kStreamWaves waves of a workgroup take kStreamWaves clerks of ONE participant (workgroup
// p * ceil(n / kStreamWaves) + q holds clerks kStreamWaves q ..), so that participant's secrets come from HBM once per workgroup
// and from the cache for its other waves.  by_rows != 0 (A/B only): consecutive rows, i.e. kStreamWaves participants of one
// clerk, each wave fetching secrets of its own.
template <int ROUNDS>
__global__ __launch_bounds__(kStreamWaves * 64) void share_seal_stream_kernel(ShareJob J, uint32_t by_rows, uint8_t* __restrict__ boxes,
                                                                              uint64_t slot, const SboxState* __restrict__ states,
                                                                              uint64_t* __restrict__ msg_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[kStreamWaves][kEncTile];
    __shared__ uint32_t kstream[kStreamWaves][kKsTile];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t c, p;
    if (by_rows) {
        const uint64_t r = (uint64_t)blockIdx.x * kStreamWaves + wave;
        c = r / J.participants; p = r - c * J.participants;
    } else {
        const uint32_t groups = (J.n + kStreamWaves - 1) / kStreamWaves;
        p = blockIdx.x / groups;
        c = (uint64_t)(blockIdx.x - p * groups) * kStreamWaves + wave;
    }
    if (c >= J.n || p >= J.participants) return;
    const uint64_t r = c * J.participants + p;
    // a clerk key that gave the all-zero shared secret: that clerk's rows are refused (varint_seal_stream_kernel)
    if (states[r].bad) { if ((threadIdx.x & 63) == 0) msg_bytes[r] = 0; return; }
    EncXSalsa crypt;
    crypt.open(states[r], kstream[wave]);
    ShareValues<ROUNDS> vals(J, (uint32_t)c, p);
    encode_row(vals, J.batches, r, boxes + r * slot + 48, tiles[wave], msg_bytes, crypt);
}

// ---- secrets -> masked secrets and the sealed mask rows without the masks (participate.rs:52-72: mask the secrets, seal the mask to
// the recipient; full.rs:21-35) ---
// The seal kernel again, the row's values DRAWN: row p is participant p's mask, the sda-drbg-v1 draws of stream first_participant + p
// with T = 1 - what full_mask_drbg_kernel draws.  Lane l of step j owns elements 128 j + 2 l and + 1 = pair 64 j + l of the DPP-quad
// CSPRNG, so drbg_pair() hands the lane its two masks; all 64 lanes draw in every step (a quad must be whole), the lanes past the
// row's end store nothing and encode_row gives their values the length 0.  The same lane adds the masks onto its two secrets and
// stores the masked secrets; the masks go on to the encode loop and exist in registers only.  Each element is read once and
// written once by the lane that read it, so masked == secrets (equal strides) is fine.
template <int ROUNDS>
struct MaskValues {
    static constexpr int kDepth = 1;          // nothing is prefetched: the step loop stays rolled
    const MaskJob& J;
    const int64_t* sp;                        // the participant's secrets ...
    int64_t* mp;                              // ... and masked secrets (may be the same row)
    uint64_t stream;
    bool vec;                                 // wave-uniform: both rows 16-byte aligned
    QuadCol qc;
    __device__ __forceinline__ MaskValues(const MaskJob& J_, uint64_t p) : J(J_) {
        sp = J.secrets + p * J.secrets_stride;
        mp = J.masked + p * J.masked_stride;
        stream = J.first_participant + p;
        vec = ((((uintptr_t)sp) | ((uintptr_t)mp)) & 15u) == 0;
        qc = quad_col(J.key);
    }
    __device__ __forceinline__ void get(int, uint64_t j, int64_t& x, int64_t& y) {
        typedef long long ll2v __attribute__((ext_vector_type(2)));
        const uint64_t pair = j * (kEncVals / 2) + (threadIdx.x & 63u);
        const uint64_t b0 = 2 * pair;
        const bool two = vec && b0 + 1 < J.len;                       // the odd tail and a misaligned row take 8-byte accesses
        const bool one0 = !two && b0 < J.len, one1 = !two && b0 + 1 < J.len;
        // the secrets first: the ChaCha rounds of the draw cover the load's latency
        long long s0 = 0, s1 = 0;
        if (two) {
            const ll2v v = __builtin_nontemporal_load(reinterpret_cast<const ll2v*>(sp + b0));
            s0 = v.x; s1 = v.y;
        }
        if (one0) s0 = __builtin_nontemporal_load(reinterpret_cast<const long long*>(sp + b0));
        if (one1) s1 = __builtin_nontemporal_load(reinterpret_cast<const long long*>(sp + b0 + 1));
        __builtin_amdgcn_sched_barrier(0);
        uint64_t r0, r1;
        drbg_pair<ROUNDS>(J.key, qc, stream, pair, 1, 0, J.mod, r0, r1);
        const uint64_t m = J.mod.m, mu = J.mod.mu;
        const long long m0 = (long long)addmod(canon_i64(s0, m, mu), r0, m);
        const long long m1 = (long long)addmod(canon_i64(s1, m, mu), r1, m);
        if (two) {
            ll2v v;
            v.x = m0; v.y = m1;
            __builtin_nontemporal_store(v, reinterpret_cast<ll2v*>(mp + b0));
        }
        if (one0) __builtin_nontemporal_store(m0, reinterpret_cast<long long*>(mp + b0));
        if (one1) __builtin_nontemporal_store(m1, reinterpret_cast<long long*>(mp + b0 + 1));
        x = (int64_t)r0; y = (int64_t)r1;
    }
};

// One wave per participant row, kStreamWaves rows per workgroup
template <int ROUNDS>
__global__ __launch_bounds__(kStreamWaves * 64) void mask_seal_stream_kernel(MaskJob J, uint8_t* __restrict__ boxes, uint64_t slot,
                                                                             const SboxState* __restrict__ states,
                                                                             uint64_t* __restrict__ msg_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t tiles[kStreamWaves][kEncTile];
    __shared__ uint32_t kstream[kStreamWaves][kKsTile];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t p = (uint64_t)blockIdx.x * kStreamWaves + wave;
    if (p >= J.participants) return;
    // a recipient key that gave the all-zero shared secret: the row is refused (varint_seal_stream_kernel) and, nothing being
    // drawn, its secrets stay unmasked - masked row p is left as it was
    if (states[p].bad) { if ((threadIdx.x & 63) == 0) msg_bytes[p] = 0; return; }
    EncXSalsa crypt;
    crypt.open(states[p], kstream[wave]);
    MaskValues<ROUNDS> vals(J, p);
    encode_row(vals, J.len, p, boxes + p * slot + 48, tiles[wave], msg_bytes, crypt);
}

// ---- clerk sums -> the sealed clerking result, every row split over the chip (clerk.rs:84-100: reduce, encode_var, seal) ---------
// A clerk has ONE result row per job, so the one-wave-per-row seal above would put a whole job on one wave.  Here a row is cut
// into blocks of kSumVals values, one workgroup each, in the three passes of the scan-form encoder - lengths, scan, write - with
// the residues computed from the 128-bit accumulators in the first and the third pass (mod_i128, the fold of
// combine_finish_kernel) and the XSalsa20 keystream xor-ed into the block's bytes while they sit in LDS.  Neither the residues nor
// the plaintext varint bytes reach memory; the accumulators are read twice (32 B per value).
//
// Geometry: a block whose bytes start at message byte `off` covers stream bytes [32 + off, 32 + off + total) (stream bytes
// 0..31 are the Poly1305 key), i.e. the Salsa20 blocks from (32 + off) >> 6 on.  The stage is laid on that block grid - its byte
// 0 is the first byte of Salsa20 block (32 + off) >> 6, the block's own bytes start at pad = (32 + off) & 63 - so keystream
// word x of the workgroup belongs to stage word x.  The keystream tile is [block][17 words]: lane i stores its block with a stride
// of 17 words (no bank shared inside a wave), the xor pass reads it with consecutive lanes on consecutive words.
static constexpr int kSumVals = kVT * kVals;                  // values per workgroup
static constexpr int kSumStage = 64 + kSumVals * 10;          // pad (< 64) + at most 10 bytes per value
static constexpr int kSumKsBlocks = kSumStage / 64;           // Salsa20 blocks that can overlap the stage: 321, one or two per lane
static constexpr int kSumKsStride = 17;

size_t sum_seal_blocks(size_t len) { return (size_t)((len + kSumVals - 1) / kSumVals); }

// Only the block total matters: value i of the block goes to lane i % 256 (coalesced 8-byte loads).
__global__ __launch_bounds__(kVT) void sum_len_kernel(SumRows S, uint32_t* __restrict__ block_bytes) {
    __shared__ uint32_t waves[kVT / 64];
    const uint64_t job = blockIdx.y;
    const uint64_t* lo = S.acc_lo + job * S.len;
    const int64_t* hi = S.acc_hi + job * S.len;
    const uint64_t i0 = (uint64_t)blockIdx.x * kSumVals + threadIdx.x;
    uint32_t sum = 0;
    for (int u = 0; u < kVals; ++u) {
        const uint64_t i = i0 + (uint64_t)u * kVT;
        if (i < S.len) sum += varint_len(zigzag((int64_t)mod_i128(lo[i], hi[i], S.m, S.mu)));
    }
    uint32_t total;
    (void)block_exscan(sum, waves, &total);
    if (threadIdx.x == 0) block_bytes[job * gridDim.x + blockIdx.x] = total;
}

// Workgroup (blk, job): the block's residues again, their varint bytes into the stage (8 consecutive values per lane, as
// varint_write_kernel), the keystream of exactly the Salsa20 blocks the stage overlaps, the xor, and the copy into the box with
// varint_write_kernel's rule (bytes up to the destination's first dword boundary, dwords, tail bytes: two workgroups never store
// to the same dword).  block_off: the exclusive scan of sum_len_kernel's totals over all jobs; a block's offset inside its row is
// its entry minus that of its job's first block.  The job's last block stores the row's message length for the Poly1305 pass.
// A row whose state says `bad` (all-zero shared secret) is not encoded: length 0, nothing written.
__global__ __launch_bounds__(kVT) void sum_seal_wide_kernel(SumRows S, const uint64_t* __restrict__ block_off, uint8_t* __restrict__ boxes,
                                                            uint64_t slot, const SboxState* __restrict__ states,
                                                            uint64_t* __restrict__ msg_bytes) {
    __shared__ uint32_t waves[kVT / 64];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kSumStage + 16];
    __shared__ uint32_t ks[kSumKsBlocks * kSumKsStride];
    const uint64_t job = blockIdx.y, blk = blockIdx.x, n_blk = gridDim.x;
    const bool last = blk + 1 == n_blk;
    const SboxState& st = states[job];
    if (st.bad) { if (last && threadIdx.x == 0) msg_bytes[job] = 0; return; }       // workgroup-uniform
    const uint64_t off = block_off[job * n_blk + blk] - block_off[job * n_blk];
    const uint32_t pad = (uint32_t)((off + 32) & 63u);
    const uint64_t ks0 = (off + 32) >> 6;                     // the Salsa20 block under stage byte 0
    const uint64_t* lo = S.acc_lo + job * S.len;
    const int64_t* hi = S.acc_hi + job * S.len;
    const uint64_t i0 = blk * kSumVals + (uint64_t)threadIdx.x * kVals;
    uint64_t zz[kVals];
    uint32_t ln[kVals];
    uint32_t sum = 0;
    for (int k = 0; k < kVals; ++k) {
        zz[k] = 0; ln[k] = 0;
        if (i0 + k < S.len) {
            zz[k] = zigzag((int64_t)mod_i128(lo[i0 + k], hi[i0 + k], S.m, S.mu));
            ln[k] = varint_len(zz[k]);
            sum += ln[k];
        }
    }
    uint32_t total;
    uint32_t pos = pad + block_exscan(sum, waves, &total);
#pragma unroll
    for (int k = 0; k < kVals; ++k) {
        if (ln[k]) {
            uint64_t n = zz[k];
            for (uint32_t b = 0; b + 1 < ln[k]; ++b) { stage[pos++] = (uint8_t)(0x80u | (n & 0x7Fu)); n >>= 7; }
            stage[pos++] = (uint8_t)n;
        }
    }
    if (total) {
        uint32_t key[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) key[i] = st.subkey[i];
        const uint32_t n_ks = (pad + total + 63u) >> 6;       // <= kSumKsBlocks
        for (uint32_t i = threadIdx.x; i < n_ks; i += kVT) {
            uint32_t b[16];
            sbx::salsa20_block(b, key, st.n0, st.n1, ks0 + i);
#pragma unroll
            for (int w = 0; w < 16; ++w) ks[i * kSumKsStride + w] = b[w];
        }
    }
    __syncthreads();
    uint32_t* stage32 = reinterpret_cast<uint32_t*>(stage);
    const uint32_t n_words = total ? (pad + total + 3u) >> 2 : 0u;                   // whole words: the bytes around the block's never leave
    for (uint32_t x = threadIdx.x; x < n_words; x += kVT) stage32[x] ^= ks[(x >> 4) * kSumKsStride + (x & 15u)];
    __syncthreads();
    uint8_t* dst = boxes + job * slot + 48 + off;
    const uint32_t head = (uint32_t)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
    const uint32_t h = head < total ? head : total;
    if (threadIdx.x < h) dst[threadIdx.x] = stage[pad + threadIdx.x];
    const uint32_t n_dw = (total - h) >> 2;
    uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst + h);
    for (uint32_t d = threadIdx.x; d < n_dw; d += kVT) {
        const uint32_t byte = pad + h + 4u * d;                // source byte offset in stage
        const uint32_t w0 = stage32[byte >> 2], w1 = stage32[(byte >> 2) + 1];
        dst32[d] = __builtin_amdgcn_alignbyte(w1, w0, byte & 3u);
    }
    const uint32_t done = h + 4u * n_dw;
    if (threadIdx.x < total - done) dst[done + threadIdx.x] = stage[pad + done + threadIdx.x];
    if (last && threadIdx.x == 0) msg_bytes[job] = off + total;
}

// ---- launchers ------------------------------------------------------------------------------------
static inline uint64_t vceil(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

size_t varint_encode_blocks(size_t rows, size_t len) { return (size_t)vceil((uint64_t)rows * len, kVT * kVals); }
size_t varint_decode_blocks(size_t n_bytes) { return (size_t)vceil(n_bytes, kVT * kBytes); }

hipError_t launch_varint_lengths(const VarintRows& R, uint32_t* d_block_bytes, hipStream_t s) {
    const size_t nb = varint_encode_blocks(R.rows, R.len);
    if (nb == 0) return hipSuccess;
    if (nb > 0xFFFFFFFFull / kVT) return hipErrorInvalidConfiguration;   // < 2^32 work-items per launch
    varint_len_kernel<<<dim3((unsigned)nb), dim3(kVT), 0, s>>>(R, d_block_bytes);
    return hipGetLastError();
}

size_t scan_aux_entries(size_t n) { return (n + 1023) / 1024 + 1; }

hipError_t launch_scan_u32(const uint32_t* d_in, uint64_t* d_out, size_t n, uint64_t* d_total, uint64_t* d_aux,
                           hipStream_t s) {
    const size_t m = (n + 1023) / 1024;
    if (m == 0) return hipMemsetAsync(d_total, 0, 8, s);
    if (m > 0xFFFFFFFFull / 1024) return hipErrorInvalidConfiguration;
    scan_chunks_kernel<<<dim3((unsigned)m), dim3(1024), 0, s>>>(d_in, d_out, d_aux, n);
    scan_totals_kernel<<<dim3(1), dim3(1024), 0, s>>>(d_aux, m, d_total);
    scan_add_kernel<<<dim3((unsigned)m), dim3(1024), 0, s>>>(d_out, d_aux, n);
    return hipGetLastError();
}

hipError_t launch_varint_write(const VarintRows& R, const uint64_t* d_block_off, uint8_t* d_out, uint64_t* d_row_offsets,
                               hipStream_t s) {
    const size_t nb = varint_encode_blocks(R.rows, R.len);
    if (nb == 0) return hipSuccess;
    varint_write_kernel<<<dim3((unsigned)nb), dim3(kVT), 0, s>>>(R, d_block_off, d_out, d_row_offsets);
    return hipGetLastError();
}

hipError_t launch_varint_count(const uint8_t* d_bytes, size_t n_bytes, uint32_t* d_block_counts, hipStream_t s) {
    const size_t nb = varint_decode_blocks(n_bytes);
    if (nb == 0) return hipSuccess;
    if (nb > 0xFFFFFFFFull / kVT) return hipErrorInvalidConfiguration;
    varint_count_kernel<<<dim3((unsigned)nb), dim3(kVT), 0, s>>>(d_bytes, n_bytes, d_block_counts);
    return hipGetLastError();
}

hipError_t launch_varint_decode(const uint8_t* d_bytes, size_t n_bytes, const uint64_t* d_block_val_off, size_t rows,
                                size_t len, size_t row_stride, int64_t* d_out, uint32_t* d_status, hipStream_t s) {
    const size_t nb = varint_decode_blocks(n_bytes);
    if (nb == 0) return hipSuccess;
    varint_decode_kernel<<<dim3((unsigned)nb), dim3(kVT), 0, s>>>(d_bytes, n_bytes, d_block_val_off, rows, len, row_stride,
                                                                  d_out, d_status);
    return hipGetLastError();
}

hipError_t launch_varint_stream_decode(const uint8_t* d_bytes, size_t n_bytes, const RowRanges& d_offsets, size_t rows,
                                       size_t len, size_t row_stride, int64_t* d_out, uint32_t* d_status, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    varint_stream_decode_kernel<<<dim3((unsigned)vceil(rows, kStreamWaves)), dim3(kStreamWaves * 64), 0, s>>>(
        d_bytes, n_bytes, d_offsets, rows, len, row_stride, d_out, d_status);
    return hipGetLastError();
}

hipError_t launch_varint_stream_encode(const VarintRows& R, uint8_t* d_out, size_t slot_bytes, uint64_t* d_row_bytes,
                                       hipStream_t s) {
    if (R.rows == 0) return hipSuccess;
    varint_stream_encode_kernel<<<dim3((unsigned)vceil(R.rows, kStreamWaves)), dim3(kStreamWaves * 64), residency_pad_bytes(knob(KNOB_WIRE_WG_PER_CU), 8192), s>>>(
        R, d_out, slot_bytes, d_row_bytes);
    return hipGetLastError();
}

hipError_t launch_varint_seal_stream(const VarintRows& R, uint8_t* d_boxes, size_t slot_bytes, const SboxState* d_states,
                                     uint64_t* d_msg_bytes, hipStream_t s) {
    if (R.rows == 0) return hipSuccess;
    const uint64_t groups = vceil(R.rows, kStreamWaves);
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    varint_seal_stream_kernel<<<dim3((unsigned)groups), dim3(kStreamWaves * 64), 0, s>>>(R, d_boxes, slot_bytes, d_states, d_msg_bytes);
    return hipGetLastError();
}

static bool sum_grid(const SumRows& S, dim3* grid) {
    const uint64_t nb = sum_seal_blocks(S.len);
    if (S.jobs > 65535 || nb * S.jobs > 0xFFFFFFFFull / kVT) return false;          // grid.y; < 2^32 work-items per launch
    *grid = dim3((unsigned)nb, (unsigned)S.jobs);
    return true;
}

hipError_t launch_sum_lengths(const SumRows& S, uint32_t* d_block_bytes, hipStream_t s) {
    if (S.jobs == 0 || S.len == 0) return hipSuccess;
    dim3 grid;
    if (!sum_grid(S, &grid)) return hipErrorInvalidConfiguration;
    sum_len_kernel<<<grid, dim3(kVT), 0, s>>>(S, d_block_bytes);
    return hipGetLastError();
}

hipError_t launch_sum_seal_wide(const SumRows& S, const uint64_t* d_block_off, uint8_t* d_boxes, size_t slot_bytes,
                                const SboxState* d_states, uint64_t* d_msg_bytes, hipStream_t s) {
    if (S.jobs == 0) return hipSuccess;
    if (S.len == 0) return hipMemsetAsync(d_msg_bytes, 0, S.jobs * sizeof(uint64_t), s);   // no block: every row is the empty message
    dim3 grid;
    if (!sum_grid(S, &grid)) return hipErrorInvalidConfiguration;
    sum_seal_wide_kernel<<<grid, dim3(kVT), 0, s>>>(S, d_block_off, d_boxes, slot_bytes, d_states, d_msg_bytes);
    return hipGetLastError();
}

hipError_t launch_share_seal_stream(const ShareJob& J, int rounds, uint8_t* d_boxes, size_t slot_bytes, const SboxState* d_states,
                                    uint64_t* d_msg_bytes, hipStream_t s) {
    if (J.participants == 0 || J.n == 0) return hipSuccess;
    const bool by_rows = knob(KNOB_GENSEAL_BY_ROWS) != 0;
    const uint64_t groups = by_rows ? vceil((uint64_t)J.n * J.participants, kStreamWaves) : vceil(J.n, kStreamWaves) * (uint64_t)J.participants;
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)groups), block(kStreamWaves * 64);
    return with_rounds(rounds, [&](auto R) {
        share_seal_stream_kernel<decltype(R)::value><<<grid, block, 0, s>>>(J, by_rows, d_boxes, slot_bytes, d_states, d_msg_bytes);
        return hipGetLastError();
    });
}

hipError_t launch_mask_seal_stream(const MaskJob& J, int rounds, uint8_t* d_boxes, size_t slot_bytes, const SboxState* d_states,
                                   uint64_t* d_msg_bytes, hipStream_t s) {
    if (J.participants == 0) return hipSuccess;
    const uint64_t groups = vceil(J.participants, kStreamWaves);
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    const dim3 grid((unsigned)groups), block(kStreamWaves * 64);
    return with_rounds(rounds, [&](auto R) {
        mask_seal_stream_kernel<decltype(R)::value><<<grid, block, 0, s>>>(J, d_boxes, slot_bytes, d_states, d_msg_bytes);
        return hipGetLastError();
    });
}

hipError_t launch_varint_stream_combine(const uint8_t* d_bytes, size_t n_bytes, const RowRanges& d_offsets, size_t jobs,
                                        size_t rows_per_job, size_t len, uint64_t* d_acc_lo, int64_t* d_acc_hi,
                                        uint32_t* d_status, hipStream_t s) {
    if (jobs == 0 || rows_per_job == 0 || len == 0) return hipSuccess;
    // 16 rows per workgroup once that still gives every CU two workgroups, else 8 (more workgroups, twice the atomics)
    const bool wide = vceil(rows_per_job, 16) * jobs >= 512;
    const uint64_t groups = vceil(rows_per_job, wide ? 16 : 8);
    if (groups * jobs > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (wide)
        varint_stream_combine_kernel<16><<<dim3((unsigned)(groups * jobs)), dim3(16 * 64), residency_pad_bytes(knob(KNOB_WIRE_WG_PER_CU), 49152), s>>>(
            d_bytes, n_bytes, d_offsets, rows_per_job, groups, len, d_acc_lo, d_acc_hi, d_status);
    else
        varint_stream_combine_kernel<8><<<dim3((unsigned)(groups * jobs)), dim3(8 * 64), 0, s>>>(
            d_bytes, n_bytes, d_offsets, rows_per_job, groups, len, d_acc_lo, d_acc_hi, d_status);
    return hipGetLastError();
}

hipError_t launch_sealed_stream_combine(const uint8_t* d_boxes, size_t slot, const uint64_t* d_row_bytes, size_t rows,
                                        size_t max_box_bytes, const SboxState* d_states, size_t len, uint64_t* d_acc_lo,
                                        int64_t* d_acc_hi, uint32_t* d_status, hipStream_t s, int* waves) {
    if (waves) *waves = 0;
    if (rows == 0) return hipSuccess;
    // 8 rows per workgroup (75 KB of LDS: two workgroups per CU).  The 16-row instance needs 117 KB - ONE workgroup per CU, so
    // the plaintext kernel's reason for going wide does not carry over - and measured 12.99 ms against 8.47 ms on 2000 boxes
    // (profiles/r07/clerk_job_fused.txt); no larger job has been timed, so it is reachable through the A/B knob only
    const bool wide = knob(KNOB_SEALED_WAVES) == 16;
    const uint64_t groups = vceil(rows, wide ? 16 : 8);
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (waves) *waves = wide ? 16 : 8;
    if (wide)
        sealed_stream_combine_kernel<16><<<dim3((unsigned)groups), dim3(16 * 64), 0, s>>>(d_boxes, slot, d_row_bytes, max_box_bytes, d_states,
                                                                                       rows, len, d_acc_lo, d_acc_hi, d_status);
    else
        sealed_stream_combine_kernel<8><<<dim3((unsigned)groups), dim3(8 * 64), 0, s>>>(d_boxes, slot, d_row_bytes, max_box_bytes, d_states,
                                                                                     rows, len, d_acc_lo, d_acc_hi, d_status);
    return hipGetLastError();
}

hipError_t launch_sealed_stream_weighted(const uint8_t* d_boxes, size_t slot, const uint64_t* d_row_bytes, size_t rows,
                                         size_t max_box_bytes, const SboxState* d_states, size_t len, size_t first_pos,
                                         const WeightedJob& J, uint64_t* d_acc_lo, int64_t* d_acc_hi, uint32_t* d_status,
                                         hipStream_t s) {
    if (rows == 0) return hipSuccess;
    const uint64_t groups = vceil(rows, 8);
    if (groups > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (J.k <= (uint32_t)kCoefLds)
        sealed_stream_weighted_kernel<8, true><<<dim3((unsigned)groups), dim3(8 * 64), 0, s>>>(
            d_boxes, slot, d_row_bytes, max_box_bytes, d_states, rows, len, first_pos, J, d_acc_lo, d_acc_hi, d_status);
    else
        sealed_stream_weighted_kernel<8, false><<<dim3((unsigned)groups), dim3(8 * 64), 0, s>>>(
            d_boxes, slot, d_row_bytes, max_box_bytes, d_states, rows, len, first_pos, J, d_acc_lo, d_acc_hi, d_status);
    return hipGetLastError();
}

hipError_t launch_weighted_rows(const int64_t* d_shares, size_t row_stride, size_t rows, size_t first_pos, const WeightedJob& J,
                                uint64_t* d_acc_lo, int64_t* d_acc_hi, hipStream_t s) {
    if (rows == 0 || J.batches == 0) return hipSuccess;
    const uint64_t blocks = vceil(J.batches, kVT);
    if (blocks > 0x7FFFFFFFull || rows > 0xFFFFFFFFull) return hipErrorInvalidConfiguration;
    // as launch_packed_reconstruct: the k secrets of a batch are split into groups when the batches alone do not fill the chip
    uint64_t groups = blocks < 2048 ? vceil(2048, blocks) : 1;
    if (groups > J.k) groups = J.k;
    const uint32_t e_per_group = (uint32_t)vceil(J.k, groups);
    groups = vceil(J.k, e_per_group);
    weighted_rows_kernel<<<dim3((unsigned)blocks, (unsigned)groups), dim3(kVT), 0, s>>>(d_shares, row_stride, (uint32_t)rows, first_pos, J,
                                                                                      d_acc_lo, d_acc_hi, e_per_group);
    return hipGetLastError();
}

hipError_t launch_transpose_u64(const uint64_t* d_in, uint64_t* d_out, uint32_t k, uint32_t n, hipStream_t s) {
    const uint64_t blocks = vceil((uint64_t)k * n, kVT);
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    transpose_u64_kernel<<<dim3((unsigned)blocks), dim3(kVT), 0, s>>>(d_in, d_out, k, n);
    return hipGetLastError();
}

hipError_t launch_varint_rowcheck(const uint8_t* d_bytes, size_t n_bytes, const uint64_t* d_offsets, size_t rows, size_t len,
                                  const uint64_t* d_block_val_off, uint32_t* d_status, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    varint_rowcheck_kernel<<<dim3((unsigned)vceil(rows, kVT / 64)), dim3(kVT), 0, s>>>(d_bytes, n_bytes, d_offsets, rows, len,
                                                                                   d_block_val_off, d_status);
    return hipGetLastError();
}

}  // namespace sda

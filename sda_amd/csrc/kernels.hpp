// Launch interface between the C ABI (sda_capi.cpp) and the gfx950 kernels (sda_kernels.hip).
// Plain structs and device pointers only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

namespace sda {

struct ModParams {
    uint64_t m;           // modulus, 2 <= m < 2^62
    uint64_t mu;          // floor(2^64 / m)          (Barrett)
    uint64_t lemire_thr;  // 2^64 mod m               (Lemire rejection threshold of the one-word-per-draw rule), for EVERY modulus
    uint64_t lemire_thr2; // 2^64 mod m^2             (threshold of the PAIRED rule, modarith.hpp) when drbg_paired(m), else 0: a
                          //                          field of its own, so that no helper can be handed the other rule's threshold
};

struct MontParams {
    uint64_t p;     // odd prime modulus
    uint64_t pinv;  // -p^{-1} mod 2^64
};

struct DrbgKey {
    uint32_t w[8];
};

// Montgomery-form matrix passed BY VALUE in the kernarg segment, so that rows are fetched with
// scalar loads (s_load) and the multiplier operands live in SGPRs.
#define SDA_MAT_ARG_MAX 448   // u64 entries (3.5 KiB of the 4 KiB kernarg budget)
struct MatArg {
    uint64_t e[SDA_MAT_ARG_MAX];
};

// Constants of the balanced-31-bit-limb Montgomery path (R = 2^62, radix B = 2^31); see
// packed_gen_l31_kernel.  MatArg entries are then (uint32)m0 | (uint64)(uint32)m1 << 32 with
// m1 * B + m0 = centred representative of (M_ji * 2^62 mod p), m0 in [-2^30, 2^30).
struct L31Params {
    uint64_t p;       // modulus
    uint64_t p2;      // 2p
    uint64_t h;       // (p + 1) / 2 : v >= h is centred to v - p
    int32_t  p0;      // p mod 2^31
    int32_t  p1;      // p >> 31
    uint32_t pinvB;   // -p^{-1} mod 2^31
    uint32_t wide;    // 1: the three-digit shapes of 9 .. 12 terms run their dot product as ONE group (admitted by the host on the
                      // actual constants of both share maps, l31_wide_group_ok); 2: ... in Karatsuba form, three multiply-adds per
                      // term (round 6; l31_karatsuba_ok admits the halves' cross columns); 0 everywhere else
    uint64_t np, np2; // 2^64 - p and 2^64 - 2p: x + np wraps exactly when x >= p (the conditional subtractions)
};

// Constants of the narrow-modulus path (p < 2^31: one signed 32-bit limb per residue, R = 2^32); see narrow_gen.inc.hpp.
// MatArg then holds int32 constants (896 entries): centred representatives of M_ji * 2^32 mod p, rows back to back.
struct N31Params {
    uint32_t p;        // modulus < 2^31
    uint32_t pinv;     // -p^-1 mod 2^32
    uint32_t h;        // (p + 1) / 2: v >= h is centred to v - p
    uint32_t pad;
};

// The library reports what it ran (include/sda_hip_debug.h: sda_debug_last_kernel): every share-generation launcher names
// the kernel instance it is about to launch, as rocprofv3 will print it (sda_capi.cpp keeps the last name per thread).
void note_kernel(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// The same for the one-shot reveal (sda_debug_last_reveal_kernel, test library only), in a buffer of its own: sda_debug_last_kernel
// keeps reporting the last share-generation call whatever reveals follow it.  The grouped kernel is named with its partition:
// "packed_reconstruct_kernel groups=9 e_per_group=2".
void note_reveal_kernel(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
// What fuse_plan (sda_kernels.hip) decided for the dual-role launch it was last asked for on this thread, refused plans included:
// { fused, n_gen, n_comb, period, grid, splits, rows_per_split, col_blocks }.  Kept by the test library only
// (sda_debug_last_fuse_plan, for tests/test_dual_role_schedule_gpu.py); the release library's note_fuse_plan does nothing.
void note_fuse_plan(const unsigned long long plan[8]);

// strides in elements
struct GenLayout {
    const int64_t* secrets;   size_t secrets_stride;
    const int64_t* rand;      size_t rand_stride;     // rand == nullptr -> DRBG
    int64_t* out;             size_t out_stride_participant; size_t out_stride_clerk;
    size_t participants;      size_t len;             // secrets per participant
    uint64_t first_participant;                       // DRBG stream id of participant 0
    // packed Shamir with the device CSPRNG (rand == nullptr), "systematic" share map: output rows 0 .. direct_rows-1 ARE
    // the t draws of each batch (direct_rows = t) and the matrix the kernel is handed has the other n - direct_rows rows
    // (the polynomial through (1, 0), the secrets at omega_secrets^1..k and the draws at omega_shares^1..t).  0: every
    // row is a dot product with the n-row tss matrix (draws are the values at omega_secrets^(k+1..k+t)).
    uint32_t direct_rows;
};

// The clerk-sum side of a dual-role launch (below): the 128-bit column accumulators [jobs][dimension] and the previous tile's
// shares they take in, prev_rows participants in the SAME layout as the GenLayout's out
struct ClerkSumTarget {
    uint64_t* acc_lo;
    int64_t* acc_hi;
    const int64_t* prev;
    size_t prev_rows, jobs, dimension;
};

// ---- share generation ---------------------------------------------------------------------------
// additive: k = 1, n shares, n-1 randoms per element (additive.rs:32-51 through batched.rs:18-53)
hipError_t launch_additive_generate(const GenLayout& L, uint32_t n, const ModParams& mod,
                                    const DrbgKey& key, int rounds, hipStream_t s);

// packed Shamir, fast path: (k, t) must be one of the compiled pairs and n*(k+t) <= SDA_MAT_ARG_MAX
bool packed_fast_path_available(uint32_t k, uint32_t t, uint32_t n);
hipError_t launch_packed_generate(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t,
                                  const ModParams& mod, const MontParams& mont, const MatArg& Mmont,
                                  const DrbgKey& key, int rounds, hipStream_t s);

// packed Shamir, compiled (k, t) shapes: balanced 31-bit limbs, carry-free v_mad_i64_i32 dot products
bool packed_l31_path_available(uint32_t k, uint32_t t, uint32_t n);
unsigned packed_l31_r_bits(uint32_t k, uint32_t t);     // 62 or 93: the Montgomery radix 2^bits the kernels of this shape expect
unsigned packed_l31_rt_r_bits(uint32_t kt);             // ... and the run-time (k, t) kernels (the global-matrix form serves compiled shapes too when n is large)
bool packed_l31_three_digit_compiled(uint32_t k, uint32_t t);   // a COMPILED (k, t) instance in the three-digit form
hipError_t launch_packed_generate_l31(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t,
                                      const ModParams& mod, const L31Params& lp, const MatArg& Ml31,
                                      const DrbgKey& key, int rounds, hipStream_t s);

// packed Shamir over a NARROW prime (p < 2^31, the reference's own valid domain): run-time (k, t), k + t <= 16, ChaCha20 only
bool packed_n31_path_available(uint32_t k, uint32_t t, uint32_t rows, uint64_t p);
hipError_t launch_packed_generate_n31(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t, const ModParams& mod,
                                      const N31Params& np, const MatArg& M, const DrbgKey& key, hipStream_t s);
hipError_t launch_fused_packed_n31(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t, const ModParams& mod, const N31Params& np,
                                   const MatArg& M, const DrbgKey& key, const ClerkSumTarget& C, hipStream_t s, bool* fused);

// packed Shamir as a limb GEMM on the matrix cores (v_mfma_i32_16x16x64_i8 on balanced base-256 digits), compiled shapes
bool packed_mfma_path_available(uint32_t k, uint32_t t, uint32_t n);
hipError_t launch_packed_generate_mfma(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t, const ModParams& mod,
                                       const MontParams& mont, const uint64_t* d_Mbal /* [n][8 ceil((k+t)/8)] */,
                                       const DrbgKey& key, int rounds, hipStream_t s);

hipError_t launch_fused_packed_mfma(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t, const ModParams& mod,
                                    const MontParams& mont, const uint64_t* d_Mbal, const DrbgKey& key, int rounds,
                                    const ClerkSumTarget& C, hipStream_t s, bool* fused);

// the limb-31 kernel with run-time (k, t) and the matrix in global memory: any n, k + t <= 64
bool packed_l31_global_path_available(uint32_t k, uint32_t t);
hipError_t launch_packed_generate_l31_global(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t, const ModParams& mod,
                                             const L31Params& lp, const uint64_t* d_Ml31 /* n (k+t) entries + 7 zeros */,
                                             const DrbgKey& key, int rounds, hipStream_t s);

// packed Shamir, transform form (tss's own radix-2 inverse / radix-3 forward structure) for large tss-valid shapes:
// k + t + 1 = 2^a = ord(omega_secrets), n + 1 = 3^b = ord(omega_shares), b >= 2, p < 2^62.  Every constant w travels with
// its companion floor(w 2^64 / p) (Shoup): table entries are (w, companion) pairs of 16 bytes.
struct FftPlan {
    uint32_t k, t, n;
    uint32_t m2, a;            // k + t + 1 = 2^a
    uint32_t m3, b;            // n + 1 = 3^b
    uint32_t G, lgG;           // batches per workgroup (a power of two): 16 or 8 (one CSPRNG block per draw serves 8) or 1
    uint32_t tw_lds;           // 1: the workgroup copies both twiddle tables to LDS
    uint64_t groups_padded;    // set by the launcher for G < 8: groups per participant rounded up to 8 * (16 / G) (XCD-aware group map)
    uint32_t lazy;             // 1 (narrow only): (4 b + 4) p < 2^32 - the radix-3 levels run without conditional subtractions
    uint64_t one_s;            // floor(2^32 / p): the companion of the constant 1 (narrow: full reduction of a lazy value)
    uint32_t narrow;           // 1: p < 2^30 - uint32_t values, tables of (uint32 w, uint32 floor(w 2^32 / p)) pairs, 32-bit companions below
    uint32_t nz_mask;          // bit 3 e0 + e1: e1 (m3 / 9) + e0 (m3 / 3) < m2, i.e. some 9-block of the zero-extended
                               // vector holds a coefficient at that position (fft_kernels.hip, the folded first two levels)
    const uint64_t* tw2;       // m2 / 2 pairs: omega_secrets^-j              (device)
    const uint64_t* tw3;       // m3 pairs:     omega_shares^j                (device)
    uint64_t omega, omega_s;   // omega_shares^(m3 / 3) and its companion
    uint64_t scale, scale_s;   // 1 / m2 and its companion
    uint32_t magic_k1, magic_t; // floor(2^32 / d) + 1 for d = k + 1 and d = t (exact quotients of the loader's small indices)
    uint32_t want_threads;     // host only, A/B: threads per workgroup (0 = the launcher's choice), knob SDA_FFT_THREADS at handle creation
    uint32_t no_xcd_map;       // host only, A/B: plain group order for G < 8 (knob SDA_NO_XCD_MAP at handle creation)
};
size_t fft_lds_bytes(uint32_t m2, uint32_t m3, uint32_t G, bool tw_lds, bool narrow);
hipError_t launch_packed_generate_fft(const GenLayout& L, const ModParams& mod, const DrbgKey& key, const FftPlan& F, int rounds,
                                      hipStream_t s);

// packed Shamir over a narrow prime (p <= 0x7F7F7F, just below 2^23: three balanced base-256 digits per residue) as a limb GEMM on the
// matrix cores: any (k, t) with k + t <= 512, any n
// (ngemm_kernels.hip).  Draws are the transform kernel's (tss's nodes), ChaCha20 only.
struct NGemmPlan {
    uint32_t k, t, n;
    uint32_t ks;               // 64-term steps of the compiled instance: 1, 2, 4 or 8 (>= ceil((k + t) / 64), zero padded)
    uint32_t row_tiles;        // ceil(n / 16)
    int32_t c[5];              // centred representatives of 256^j 2^32 mod p: column j -> Montgomery operand
    N31Params np;
    const uint8_t* A;          // device: [row_tiles][ks][3 digits][64 lanes][16 bytes] - the A fragments of M's balanced digits,
                               // zero beyond n rows / k + t terms
};
size_t ngemm_tile_bytes(uint32_t ks);
bool packed_ngemm_path_available(uint32_t k, uint32_t t, uint64_t p);
uint32_t packed_ngemm_steps(uint32_t k, uint32_t t);
hipError_t launch_packed_generate_ngemm(const GenLayout& L, const ModParams& mod, const DrbgKey& key, const NGemmPlan& P, hipStream_t s);
// dual-role form.  d_progress != nullptr (room for ngemm_clerk_slots(L, P) x 2 u64): the clerk sum of the previous tile rides in three
// clerk WAVES of every share-generation workgroup, a follow-up kernel sums what they did not get to (round 6, the default);
// d_progress == nullptr: clerk WORKGROUPS at fixed positions of the same grid (rounds 4 - 5; A/B knob SDA_NGEMM_CLERK_WG)
uint64_t ngemm_clerk_slots(const GenLayout& L, const NGemmPlan& P);
hipError_t launch_fused_packed_ngemm(const GenLayout& L, const ModParams& mod, const DrbgKey& key, const NGemmPlan& P,
                                     const ClerkSumTarget& C, hipStream_t s, bool* fused, uint64_t* d_progress = nullptr,
                                     size_t progress_slots = 0);

// packed Shamir, any shape: matrix in global memory, randomness must be materialised (L.rand != 0)
hipError_t launch_packed_generate_generic(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t,
                                          const ModParams& mod, const MontParams& mont,
                                          const uint64_t* d_Mmont, hipStream_t s);

// materialise the DRBG draws exactly as the fused kernels would make them:
// out[p*stride + b*T + i], b < batches, i < T
hipError_t launch_drbg_fill(int64_t* d_out, size_t stride, size_t participants, size_t batches,
                            uint32_t T, uint64_t first_participant, const ModParams& mod,
                            const DrbgKey& key, int rounds, hipStream_t s);

// ---- clerk combine (combiner.rs:15-29) -------------------------------------------------------------
// acc (lo, hi) += sum over rows; element (job, row, i) at shares + job*job_stride + row*row_stride + i
hipError_t launch_combine_update(uint64_t* d_acc_lo, int64_t* d_acc_hi, const int64_t* d_shares,
                                 size_t jobs, size_t job_stride, size_t n_rows, size_t row_stride,
                                 size_t dimension, hipStream_t s, unsigned max_wg_per_cu = 0, unsigned walk_workgroups = 0);
hipError_t launch_combine_finish(const uint64_t* d_acc_lo, const int64_t* d_acc_hi, size_t count,
                                 const ModParams& mod, int64_t* d_out, hipStream_t s);

// ---- the reference's own signed representatives (value mode SDA_VALUES_RUST_SIGNED) - signed_kernels.hip --------------
// additive.rs:42-47: shares j < n-1 are the draws, untouched - injected (L.rand: (n-1) draws per element, ANY i64) or, with
// L.rand == nullptr, the sda-drbg-v1 draws of the canonical kernel made inside the kernel (no scratch)
hipError_t launch_additive_generate_signed(const GenLayout& L, uint32_t n, const ModParams& mod, const DrbgKey& key, int rounds,
                                           hipStream_t s);
hipError_t launch_additive_generate_signed_drbg(const GenLayout& L, uint32_t n, const ModParams& mod, const DrbgKey& key, int rounds,
                                                hipStream_t s);       // sda_kernels.hip (the DPP-quad CSPRNG lives there)
// combiner.rs:20-26: state[job][col] = (state + row) % q, rows in order; state is int64 [jobs][dimension]
hipError_t launch_combine_update_signed(int64_t* d_state, const int64_t* d_shares, size_t jobs, size_t job_stride, size_t n_rows,
                                        size_t row_stride, size_t dimension, int64_t q, hipStream_t s);
// (a + b) % q / (a - b) % q with Rust's truncated remainder, sums formed exactly
hipError_t launch_addsub_signed(const int64_t* d_a, const int64_t* d_b, size_t len, bool subtract, int64_t q, int64_t* d_out,
                                hipStream_t s);

// ---- dual-role launch: share generation of one tile + clerk-sum of the previous tile in ONE grid ----------
// C.prev holds the previous tile's shares in the SAME layout as L.out (job stride = L.out_stride_clerk, row
// stride = L.out_stride_participant), C.prev_rows participants; L.participants may be 0 (clerk-sum only) and
// C.prev may be null (generation only).  *fused = false (and nothing launched) when the layout or the shape
// rules the fused form out - the caller then issues the two ordinary launches.
hipError_t launch_fused_packed_l31(const GenLayout& L, uint32_t n, uint32_t k, uint32_t t, const ModParams& mod,
                                   const L31Params& lp, const MatArg& M, const DrbgKey& key, int rounds, const ClerkSumTarget& C,
                                   hipStream_t s, bool* fused);
hipError_t launch_fused_additive(const GenLayout& L, uint32_t n, const ModParams& mod, const DrbgKey& key, int rounds,
                                 const ClerkSumTarget& C, hipStream_t s, bool* fused);

// ---- packed reconstruct (batched.rs:68-97 + tss reconstruct as a k x n' Lagrange matrix) ------------
hipError_t launch_packed_reconstruct(const int64_t* d_shares, size_t row_stride, uint32_t n_rows,
                                     uint32_t k, size_t batches, size_t dimension,
                                     const ModParams& mod, const MontParams& mont,
                                     const uint64_t* d_Rmont /*[k][n_rows]*/, int64_t* d_out,
                                     hipStream_t s);

// the same over a narrow prime (p < 2^31): one-limb arithmetic, R31 = centred Montgomery-form (R = 2^32) int32 constants [k][n_rows]
bool packed_reconstruct_n31_available(uint32_t n_rows, uint32_t k, uint64_t p, const int64_t* d_shares, size_t row_stride,
                                      const int64_t* d_out);
hipError_t launch_packed_reconstruct_n31(const int64_t* d_shares, size_t row_stride, uint32_t n_rows, uint32_t k, size_t batches,
                                         size_t dimension, const ModParams& mod, const N31Params& np, const int32_t* d_R31,
                                         int64_t* d_out, hipStream_t s);

// ---- element-wise masking (full.rs / chacha.rs mask+unmask arithmetic) ----------------------------
// out = (a + b) mod m   or   (a - b) mod m, any i64 inputs
hipError_t launch_addsub_mod(const int64_t* d_a, const int64_t* d_b, size_t len, bool subtract,
                             const ModParams& mod, int64_t* d_out, hipStream_t s);
// unmask (full.rs:54-67, chacha.rs:79-93, none.rs:28-33) fed by the recipient's two device jobs: out[i] = (fold of the
// reconstructor job's sums mod recon_mod, canonicalised under mask_mod) - (fold of the mask job's sums mod mask_mod), mod mask_mod,
// i < len.  d_mask_lo == nullptr: no mask, out = the fold of the reconstructor's sums.  The accumulator arrays hold at least `len`
// entries and are 16-byte aligned; d_out any 8-byte aligned pointer.  d_gate_a / d_gate_b (nullptr: none): device words read when
// the kernel starts - one of them non-zero and nothing is stored
hipError_t launch_unmask_finish(const uint64_t* d_recon_lo, const int64_t* d_recon_hi, const ModParams& recon_mod,
                                const uint64_t* d_mask_lo, const int64_t* d_mask_hi, const ModParams& mask_mod, size_t len,
                                const uint32_t* d_gate_a, const uint32_t* d_gate_b, int64_t* d_out, hipStream_t s);
// the finish of a checked reconstruction job, one of three ends: accumulators [batches][k + checks] (k secrets, then `checks`
// syndromes, 1 .. 16), d_corr [k][n_rows] = R[s][i] / u_i and d_xs [n_rows] = the evaluation points, both in Montgomery form,
// n_rows 1 .. 65535.  Per batch: fold, test the syndromes, judge, correct under `correct`, store d_out[b k + s] for b k + s < dimension
//   Locate - exactly one position i with S_{d+1} = x_i S_d for every d < checks - 1 (checks == 1 locates nothing); under `correct`
// subtract corr[s][i] S_0.  d_report [4 + n_rows], initialised by the caller to {0, 0, 0, 2^64 - 1, 0 ...}: bad, located,
// corrected batches, first bad batch, batches that blame position i
//   Decode - per batch with a non-zero syndrome, Berlekamp-Massey + root search + magnitudes (reveal_decode.hpp); decoded with
// nu <= max_errors <= checks / 2 positions = all `checks` syndromes are reproduced by nu positions of the job.  Under `correct` the
// secrets lose sum_j corr[s][i_j] Y_j.  d_report [16 + n_rows], initialised by the caller to 0 with [3] = [4] = 2^64 - 1: bad,
// decoded, corrected batches, first bad, first undecoded batch, largest nu, 0, 0, batches decoded with nu = 1 .. 8, batches that
// blame position i.  checks 2 .. 16, max_errors 1 .. checks / 2
//   Erasures - d_ok [n_rows] device words, 0 = position i is erased whatever it added (nullptr: none); d_table:
// reveal_erasure_table_words(n_rows) device words of scratch.  reveal_erasure_setup_kernel (one workgroup) compacts the f erased
// positions and builds the per-job tables, the finish decodes the modified syndromes T_j = sum_m gamma_m S_{j+m}, j < checks - f,
// with at most min(max_errors or 8, (checks - f) / 2) non-erased positions and, under `correct`, solves the erased magnitudes and
// subtracts the correction over both sets.  d_report as for Decode, with [6] = f and [7] = 1 when f > checks (then d_out is the
// plain fold and nothing else is reported).  checks 1 .. 16, max_errors <= checks / 2
enum class RevealEnd { Locate, Decode, Erasures };
struct RevealFinishJob {
    const uint64_t* d_acc_lo;
    const int64_t* d_acc_hi;
    const uint64_t* d_corr;
    const uint64_t* d_xs;
    const uint32_t* d_ok;        // Erasures only
    uint64_t* d_table;           // Erasures only
    uint32_t k, checks, n_rows, max_errors;   // max_errors: not read for Locate
    bool correct;
    size_t batches, dimension;
    ModParams mod;
    MontParams mont;
};
// the unmasking form of a finish: where the finish stores a corrected secret v at d_out[e] it stores (canonical(v, mask_mod) -
// fold of the mask job's sum e under mask_mod) mod mask_mod.  d_mask_lo / d_mask_hi: the mask job's `dimension` 128-bit sums - no
// entry at or beyond `dimension` is read; nullptr: no mask, d_out[e] = v.  d_gate_masks / d_gate_results (nullptr: none): device
// words read when the kernel starts; *d_gate_masks != 0 or (*d_gate_results & ~results_pass_bits) != 0 and nothing is stored to
// d_out - the report is written all the same
struct RevealFinishUnmask {
    const uint64_t* d_mask_lo;
    const int64_t* d_mask_hi;
    ModParams mask_mod;
    const uint32_t* d_gate_masks;
    const uint32_t* d_gate_results;
    uint32_t results_pass_bits;
};
size_t reveal_erasure_table_words(size_t n_rows);
// one launch - reveal_{check,decode,erasure}_finish_kernel, with `unmask` reveal_check_unmask_kernel or
// reveal_decode_unmask_kernel<false | true> - for Erasures reveal_erasure_setup_kernel before it.  batches == 0 launches nothing
// but, for Erasures, the setup kernel (it writes the report's [6] and [7])
hipError_t launch_reveal_finish(RevealEnd end, const RevealFinishJob& job, const RevealFinishUnmask* unmask, int64_t* d_out,
                                uint64_t* d_report, hipStream_t s);
// full.rs:21-35 with the on-device CSPRNG, `participants` vectors at once: mask[p][i] uniform (DRBG stream
// first_stream + p), masked[p][i] = (s[p][i] + mask[p][i]) mod m
hipError_t launch_full_mask_drbg(const int64_t* d_secrets, size_t secrets_stride, size_t participants, size_t len,
                                 uint64_t first_stream, const ModParams& mod, const DrbgKey& key, int rounds,
                                 int64_t* d_mask, size_t mask_stride, int64_t* d_masked, size_t masked_stride, hipStream_t s);

// ---- rand-0.3 ChaChaRng mask expansion (chacha.rs:36-39, :60-73) ----------------------------------
// The i-th mask of a seed is its i-th ACCEPTED candidate.  One sequence serves every caller, and no launch in it waits for a
// result: fast pass (candidate i taken for mask i, rejections recorded per seed), launch_chacha_mask_plan (the records -> two
// lists and their lengths, on the device), launch_chacha_mask_shift_listed (1..3 rejections) and launch_chacha_mask_slow_listed
// (more) - or the exact-order launcher alone, over every key, where rejections are the rule.
// d_seeds: 8 u32 key words per seed (seed words beyond the given ones are 0).
// A count (of keys, of list entries) is `d_n, max`: the device word *d_n <= max, or max itself when d_n == nullptr.
struct RejectRecord {     // of seed s, zeroed by the caller: the rejected among its first `dimension` candidates, and where up to three are
    uint32_t count;
    uint32_t pos[3];
};
// where the masks go: into the 128-bit column accumulators d_acc_lo / d_acc_hi (mask combine, chacha.rs:56-77; `apply` null), or
// onto each participant's own secrets, out[s][i] = (secrets[s][i] + mask_i(seed s)) mod m (mask, chacha.rs:36-47)
struct MaskApply {
    const int64_t* secrets; size_t secrets_stride;
    int64_t* out; size_t out_stride;
    ModParams mod;
};
// fast pass into the accumulators: the candidates themselves are added (the sums are only read modulo m)
hipError_t launch_chacha_mask_accumulate(const uint32_t* d_seeds, const uint32_t* d_n_seeds, size_t max_seeds, size_t dimension,
                                         uint64_t zone, uint64_t* d_acc_lo, int64_t* d_acc_hi, RejectRecord* d_rejects,
                                         hipStream_t s);
// fast pass of the apply sink, one participant per seed
hipError_t launch_chacha_apply_fast(const uint32_t* d_seeds, size_t participants, size_t dimension, uint64_t zone,
                                    const MaskApply& apply, RejectRecord* d_rejects, hipStream_t s);
// the repair plan from the fast pass's records: d_plan[0] seeds with 1..3 rejections into d_shift_list, d_plan[1] with more into
// d_exact_list (both counters zeroed by the caller, both lists hold up to n entries, in no particular order)
hipError_t launch_chacha_mask_plan(const RejectRecord* d_rejects, size_t n, uint32_t* d_plan, uint32_t* d_shift_list,
                                   uint32_t* d_exact_list, hipStream_t s);
// Parallel correction of the seeds in d_list whose rejected candidates are all recorded (count 1..3): removing
// candidate x shifts every later mask by one, so position i >= x takes candidate i + (rejections so far) instead of
// candidate i - each lane recomputes two ChaCha blocks and adds the difference (apply: writes the mask's row anew).  The last
// few positions reach past candidate `dimension`, which the fast pass never tested: those lanes walk on until they have their mask.
hipError_t launch_chacha_mask_shift_listed(const uint32_t* d_seeds, const uint32_t* d_list, const uint32_t* d_n_list, size_t max_list,
                                           const RejectRecord* d_rejects, size_t dimension, uint64_t zone, uint64_t* d_acc_lo,
                                           int64_t* d_acc_hi, const MaskApply* apply, hipStream_t s);
// exact sequential-order expansion (handles rejections) of the seeds named by d_list (indices into d_seeds; d_list == nullptr:
// seeds 0, 1, ...).  With subtract_naive the fast pass's contribution to the accumulators is taken back first (apply: no need,
// the row is overwritten).
hipError_t launch_chacha_mask_slow_listed(const uint32_t* d_seeds, const uint32_t* d_list, const uint32_t* d_n_list, size_t max_list,
                                          size_t dimension, const ModParams& mod, uint64_t zone, uint64_t* d_acc_lo,
                                          int64_t* d_acc_hi, bool subtract_naive, const MaskApply* apply, hipStream_t s);

// ---- where the mask combiner's device form gets its keys ----
// seed rows ([rows][row_len] int64, stride row_stride; words `as u32`, the first 8 count) -> 8 key words per row
hipError_t launch_mask_rows_to_keys(const int64_t* d_rows, size_t rows, size_t row_len, size_t row_stride, uint32_t* d_keys,
                                    hipStream_t s);
// sealed seed rows (box r at d_boxes + r * slot, tags checked by launch_sealedbox_verify: rows marked bad in d_states are skipped)
// -> the keys of the rows that decrypt to a well-formed varint seed, packed from d_keys[0], their number added to *d_n_keys;
// *d_status |= 1 (a value of more than 10 bytes) / 4 (ends inside a value) for a row that does not
struct SboxState;
hipError_t launch_sealed_seed_keys(const uint8_t* d_boxes, size_t slot, const uint64_t* d_row_bytes, size_t rows, size_t max_box_bytes,
                                   const SboxState* d_states, uint32_t* d_keys, uint32_t* d_n_keys, uint32_t* d_status, hipStream_t s);

// ---- zig-zag LEB128 codec of share vectors (sodium.rs:36-41, :83-89) - varint_kernels.hip -------------
struct VarintRows {
    const int64_t* values;    // row r at values + r*row_stride
    size_t rows, len, row_stride;
};
size_t varint_encode_blocks(size_t rows, size_t len);     // workgroups (= entries of the block-sum arrays)
size_t varint_decode_blocks(size_t n_bytes);
hipError_t launch_varint_lengths(const VarintRows& R, uint32_t* d_block_bytes, hipStream_t s);
size_t scan_aux_entries(size_t n);                        // u64 scratch entries launch_scan_u32 needs
hipError_t launch_scan_u32(const uint32_t* d_in, uint64_t* d_out, size_t n, uint64_t* d_total, uint64_t* d_aux,
                           hipStream_t s);
hipError_t launch_varint_write(const VarintRows& R, const uint64_t* d_block_off, uint8_t* d_out,
                               uint64_t* d_row_offsets, hipStream_t s);
hipError_t launch_varint_count(const uint8_t* d_bytes, size_t n_bytes, uint32_t* d_block_counts, hipStream_t s);
hipError_t launch_varint_decode(const uint8_t* d_bytes, size_t n_bytes, const uint64_t* d_block_val_off,
                                size_t rows, size_t len, size_t row_stride, int64_t* d_out, uint32_t* d_status,
                                hipStream_t s);
// where the encoded rows lie in the byte buffer: contiguous (row r = [offsets[r], offsets[r+1]), offsets == nullptr:
// one row = the whole buffer) or slotted (lengths != nullptr: row r = [r*slot, r*slot + lengths[r]))
struct RowRanges {
    const uint64_t* offsets;
    const uint64_t* lengths;
    uint64_t slot;
};
// single pass, one wave per row (rows are independent messages with known byte ranges); pays off with >= ~1000 rows
hipError_t launch_varint_stream_decode(const uint8_t* d_bytes, size_t n_bytes, const RowRanges& rr, size_t rows,
                                       size_t len, size_t row_stride, int64_t* d_out, uint32_t* d_status, hipStream_t s);
// single-pass encode into slots: row r -> d_out + r*slot_bytes (16-byte aligned), its length -> d_row_bytes[r]
hipError_t launch_varint_stream_encode(const VarintRows& R, uint8_t* d_out, size_t slot_bytes, uint64_t* d_row_bytes,
                                       hipStream_t s);
// wire format -> 128-bit clerk accumulators directly: rows = jobs x rows_per_job encoded vectors (job-major), 16 rows
// of a job per workgroup through a sliding LDS column window; acc layout [jobs][len]
hipError_t launch_varint_stream_combine(const uint8_t* d_bytes, size_t n_bytes, const RowRanges& rr, size_t jobs,
                                        size_t rows_per_job, size_t len, uint64_t* d_acc_lo, int64_t* d_acc_hi,
                                        uint32_t* d_status, hipStream_t s);
// the same sums from rows that are still sealed boxes (box r at d_boxes + r * slot, d_row_bytes[r] bytes) whose tags
// launch_sealedbox_verify has checked: rows marked bad in d_states are skipped, the others are decrypted in registers.
// One job; *waves = rows per workgroup of the instance launched (8; 16 only through the A/B knob)
struct SboxState;
hipError_t launch_sealed_stream_combine(const uint8_t* d_boxes, size_t slot, const uint64_t* d_row_bytes, size_t rows,
                                        size_t max_box_bytes, const SboxState* d_states, size_t len, uint64_t* d_acc_lo,
                                        int64_t* d_acc_hi, uint32_t* d_status, hipStream_t s, int* waves);
// A streaming reconstruction job (sda_secret_reconstructor_begin_dev): secret[b k + s] = sum over positions i of
// Rt[i][s] * share_i[b] mod m, summed exactly into 128-bit accumulators [batches * k] and folded by launch_combine_finish.
struct WeightedJob {
    const uint64_t* Rt;      // [n'][k], Montgomery form: row i = the coefficients of position i
    uint32_t k;
    uint64_t batches;        // ceil(dimension / k): the values of a row that count
    uint64_t m, mu, pinv;    // the prime, floor(2^64 / m), -m^{-1} mod 2^64
};
// rows that are still sealed boxes (verified by launch_sealedbox_verify; row r is position first_pos + r, holds `len` values):
// keystream, varint decode, multiply and sums in one pass; 8 rows per workgroup
hipError_t launch_sealed_stream_weighted(const uint8_t* d_boxes, size_t slot, const uint64_t* d_row_bytes, size_t rows,
                                         size_t max_box_bytes, const SboxState* d_states, size_t len, size_t first_pos,
                                         const WeightedJob& J, uint64_t* d_acc_lo, int64_t* d_acc_hi, uint32_t* d_status,
                                         hipStream_t s);
// decoded rows [rows][row_stride], row r is position first_pos + r
hipError_t launch_weighted_rows(const int64_t* d_shares, size_t row_stride, size_t rows, size_t first_pos, const WeightedJob& J,
                                uint64_t* d_acc_lo, int64_t* d_acc_hi, hipStream_t s);
hipError_t launch_transpose_u64(const uint64_t* d_in, uint64_t* d_out, uint32_t k, uint32_t n, hipStream_t s);   // [k][n] -> [n][k]
// share rows -> the ciphertext of their sealed boxes in one pass (varint encode + XSalsa20 keystream, no wire buffer): row r to
// d_boxes + r * slot_bytes + 48 under d_states[r] (written by launch_sealedbox_seal_setup), its message length to d_msg_bytes[r];
// a row whose state says `bad` is left alone (length 0)
hipError_t launch_varint_seal_stream(const VarintRows& R, uint8_t* d_boxes, size_t slot_bytes, const SboxState* d_states,
                                     uint64_t* d_msg_bytes, hipStream_t s);
// secrets -> the ciphertext of a participation's sealed boxes in one pass: the shares of row r = c * participants + p (clerk c,
// participant p) are computed by the wave that encodes and encrypts them (sda-drbg-v1 draws, stream first_participant + p) and
// never reach memory.  States, box layout and d_msg_bytes as launch_varint_seal_stream
struct ShareJob {
    const int64_t* secrets;  size_t secrets_stride;   // participant p at secrets + p * secrets_stride
    size_t len, participants;                         // secrets per participant
    uint64_t batches;                                 // values per row: ceil(len / k)
    uint64_t first_participant;
    uint32_t n, k, t;                                 // additive: k = 1, t = n - 1
    uint32_t additive;
    uint32_t direct_rows;                             // packed: clerks 0 .. direct_rows - 1 receive the draws themselves (0 or t)
    const uint64_t* M;                                // packed, device: (n - direct_rows) x (k + t), Montgomery form
    ModParams mod;
    MontParams mont;
    DrbgKey key;
};
hipError_t launch_share_seal_stream(const ShareJob& J, int rounds, uint8_t* d_boxes, size_t slot_bytes, const SboxState* d_states,
                                    uint64_t* d_msg_bytes, hipStream_t s);
// secrets -> masked secrets in memory and the ciphertext of the participants' sealed mask rows in one pass (participate.rs:52-72,
// full.rs:21-35): row p's masks are the sda-drbg-v1 draws of stream first_participant + p (launch_full_mask_drbg's), drawn by the
// wave that adds them onto the secrets, encodes and encrypts them; no mask reaches memory.  masked == secrets with equal strides
// is allowed.  States (one key, rows_per_key = participants), box layout and d_msg_bytes as launch_varint_seal_stream; a row whose
// state says `bad` is left alone, its masked row too
struct MaskJob {
    const int64_t* secrets;  size_t secrets_stride;   // participant p at secrets + p * secrets_stride
    int64_t* masked;         size_t masked_stride;
    size_t len, participants;                         // values per row = secrets per participant
    uint64_t first_participant;
    ModParams mod;
    DrbgKey key;
};
hipError_t launch_mask_seal_stream(const MaskJob& J, int rounds, uint8_t* d_boxes, size_t slot_bytes, const SboxState* d_states,
                                   uint64_t* d_msg_bytes, hipStream_t s);
// clerk sums -> the ciphertext of the sealed clerking results, every row split over the chip (clerk.rs:84-100): job j's `len`
// 128-bit sums are folded mod m, encoded and encrypted into d_boxes + j * slot_bytes + 48 under d_states[j], in blocks of 2048
// values (sum_seal_blocks(len) per job, one workgroup each).  launch_sum_lengths writes the blocks' byte counts
// (jobs * sum_seal_blocks(len) entries, job-major), launch_scan_u32 scans them, launch_sum_seal_wide takes the scan and writes the
// bytes and d_msg_bytes[j]; a row whose state says `bad` is left alone (length 0).  Residues and plaintext bytes stay on the chip.
struct SumRows {
    const uint64_t* acc_lo;  const int64_t* acc_hi;   // [jobs][len]
    size_t jobs, len;
    uint64_t m, mu;
};
size_t sum_seal_blocks(size_t len);
hipError_t launch_sum_lengths(const SumRows& S, uint32_t* d_block_bytes, hipStream_t s);
hipError_t launch_sum_seal_wide(const SumRows& S, const uint64_t* d_block_off, uint8_t* d_boxes, size_t slot_bytes,
                                const SboxState* d_states, uint64_t* d_msg_bytes, hipStream_t s);
hipError_t launch_varint_rowcheck(const uint8_t* d_bytes, size_t n_bytes, const uint64_t* d_offsets, size_t rows,
                                  size_t len, const uint64_t* d_block_val_off, uint32_t* d_status, hipStream_t s);

// ---- RFC 4648 base64 of `Binary` payloads (protocol/src/helpers.rs:174-216) - wire_kernels.hip ----------------
// text row r at d_text + (d_offsets ? d_offsets[r] : r * text_slot), d_lengths[r] characters; raw row r at
// d_out + r * out_slot; max_chars / max_bytes bound the longest row (they size the grid)
hipError_t launch_base64_decode_rows(const uint8_t* d_text, const uint64_t* d_offsets, size_t text_slot,
                                     const uint64_t* d_lengths, size_t rows, size_t max_chars, uint8_t* d_out,
                                     size_t out_slot, uint64_t* d_out_bytes, uint32_t* d_status, uint32_t* d_row_status,
                                     hipStream_t s);
hipError_t launch_base64_encode_rows(const uint8_t* d_in, size_t in_slot, const uint64_t* d_in_bytes, size_t rows,
                                     size_t max_bytes, uint8_t* d_text, size_t text_slot, uint64_t* d_text_bytes,
                                     hipStream_t s);

// ---- libsodium sealed boxes, batched (sodium.rs:43, :78) - sealedbox_kernels.hip ----------------------------
// per-box state written by the setup kernel (first lane of the box's DPP quad) and read, wave-uniformly, by the bulk kernels
struct SboxState {
    uint32_t subkey[8];      // XSalsa20 subkey = HSalsa20(HSalsa20(X25519, 0), nonce[0:16])
    uint32_t n0, n1;         // nonce[16:24]
    uint32_t s[4];           // Poly1305 s
    uint32_t r64[5], rS[5];  // r^64 and r^1024, 26-bit limbs
    uint32_t bad, pad[7];    // 1: unusable box (shorter than 48 bytes, all-zero shared secret)
    uint32_t rpow[64][5];    // r^1 .. r^64
};
size_t sbox_regions(size_t max_msg_bytes);          // Poly1305 regions per box (sizes d_partial: rows * regions * 5 words)
// box r at d_boxes + r * slot (16-byte aligned), d_row_bytes[r] bytes; plaintext to d_out + r * out_slot (16-byte aligned)
hipError_t launch_sealedbox_open(const uint8_t pk[32], const uint8_t sk[32], const uint8_t* d_boxes, size_t slot,
                                 const uint64_t* d_row_bytes, size_t rows, size_t max_box_bytes, uint8_t* d_out, size_t out_slot,
                                 uint64_t* d_out_bytes, uint32_t* d_ok, uint32_t* d_status, SboxState* d_states,
                                 uint32_t* d_partial, hipStream_t s);
// the first half of launch_sealedbox_open: setup, Poly1305, tag compare (d_out_bytes[r] = message length, 0 for a box that fails;
// d_states[r].bad set on such rows) - and no keystream pass
hipError_t launch_sealedbox_verify(const uint8_t pk[32], const uint8_t sk[32], const uint8_t* d_boxes, size_t slot,
                                   const uint64_t* d_row_bytes, size_t rows, size_t max_box_bytes, uint64_t* d_out_bytes,
                                   uint32_t* d_ok, uint32_t* d_status, SboxState* d_states, uint32_t* d_partial, hipStream_t s);
// message r at d_msgs + r * msg_slot sealed to d_pks[(r / rows_per_key) % n_pks] with the ephemeral secret d_esk[r]
hipError_t launch_sealedbox_seal(const uint8_t* d_esk, const uint8_t* d_pks, size_t n_pks, size_t rows_per_key,
                                 const uint8_t* d_msgs, size_t msg_slot, const uint64_t* d_msg_bytes, size_t rows,
                                 size_t max_msg_bytes, uint8_t* d_boxes, size_t slot, uint64_t* d_row_bytes, SboxState* d_states,
                                 uint32_t* d_partial, hipStream_t s);
// the halves of launch_sealedbox_seal either side of its keystream pass, for a caller that writes the ciphertext itself
// (launch_varint_seal_stream): setup = ladders, epk and per-row state; auth = Poly1305 over the ciphertext in the boxes
// (d_msg_bytes[r] message bytes at box offset 48), tag, d_row_bytes[r] = message bytes + 48 (0 for a refused row)
hipError_t launch_sealedbox_seal_setup(const uint8_t* d_esk, const uint8_t* d_pks, size_t n_pks, size_t rows_per_key, uint8_t* d_boxes,
                                       size_t slot, size_t rows, SboxState* d_states, hipStream_t s);
hipError_t launch_sealedbox_seal_auth(const uint64_t* d_msg_bytes, size_t rows, size_t max_msg_bytes, uint8_t* d_boxes, size_t slot,
                                      uint64_t* d_row_bytes, SboxState* d_states, uint32_t* d_partial, hipStream_t s);
// test only (sda_debug_poly1305_rows_dev): Poly1305 of message r (d_msgs + r * msg_slot, 16-byte aligned) under the one-time key
// d_keys[32 r .. 32 r + 32) through the production poly / final kernels; tag at d_heads + 48 r + 32, d_head_bytes[r] = length + 48
hipError_t launch_sealedbox_poly_test(const uint8_t* d_keys, const uint8_t* d_msgs, size_t msg_slot, const uint64_t* d_msg_bytes,
                                      size_t rows, size_t max_msg_bytes, uint8_t* d_heads, uint64_t* d_head_bytes,
                                      SboxState* d_states, uint32_t* d_partial, hipStream_t s);

// ---- misc ---------------------------------------------------------------------------------------
// out[i] = sum over g < parts of parts[g*part_stride + i]  mod m   (cross-GPU partial sums)
hipError_t launch_modsum_parts(const int64_t* d_parts, size_t parts, size_t part_stride, size_t len,
                               const ModParams& mod, int64_t* d_out, hipStream_t s);
hipError_t launch_fill_synthetic(int64_t* d_out, size_t participants, size_t len, size_t stride,
                                 uint64_t first_participant, uint64_t seed, const ModParams& mod,
                                 hipStream_t s);

}  // namespace sda

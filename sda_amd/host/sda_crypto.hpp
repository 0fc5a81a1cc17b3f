// sda_crypto.hpp - C++ host-side mirror of the reference's `client::crypto` sharing / masking
// interface over the C ABI (include/sda_hip.h).  The reference is compiled code (Rust); its toolchain
// is absent from this image, so the host side above the C ABI is written in C++ with the same names,
// argument meaning and error behaviour:
//
//   reference (client/src/crypto)                         here
//   ------------------------------------------------      -------------------------------------------
//   trait ShareGenerator        sharing/mod.rs:14-17      struct ShareGenerator       ::generate
//   trait ShareCombiner         sharing/mod.rs:23-25      struct ShareCombiner        ::combine
//   trait SecretReconstructor   sharing/mod.rs:31-33      struct SecretReconstructor  ::reconstruct
//   trait SecretMasker          masking/mod.rs:13-15      struct SecretMasker         ::mask
//   trait MaskCombiner          masking/mod.rs:21-23      struct MaskCombiner         ::combine
//   trait SecretUnmasker        masking/mod.rs:29-31      struct SecretUnmasker       ::unmask
//   CryptoModule::new_* factories (sharing/mod.rs:35-96, masking/mod.rs:33-94)   CryptoModule::new_*
//   SdaClientResult<T> Err("...")                         throws SdaClientError("...") (same message)
//   assert!/assert_eq! panics of the masking traits       throws Panic
//
// Header-only; link against libsda_hip.so.  All arithmetic happens on the GPU behind the C ABI.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sda_hip.h"

namespace sda_client {

using Secret = int64_t;        // client/src/crypto/mod.rs:33-36
using Mask = int64_t;
using MaskedSecret = int64_t;
using Share = int64_t;

struct SdaClientError : std::runtime_error {        // error_chain string errors (client/src/errors.rs)
    int code;
    SdaClientError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
struct Panic : std::logic_error {                   // assert!/assert_eq! in the reference
    using std::logic_error::logic_error;
};

namespace detail {
inline void check(int status) {
    if (status == SDA_OK) return;
    std::string msg = sda_last_error();
    if (msg.empty()) msg = sda_strerror(status);
    if (status == SDA_ERR_ASSERTION) throw Panic(msg);
    throw SdaClientError(status, msg);
}
inline std::vector<const int64_t*> row_ptrs(const std::vector<std::vector<int64_t>>& rows, std::vector<size_t>& lens) {
    std::vector<const int64_t*> p(rows.size());
    lens.resize(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) { p[i] = rows[i].data(); lens[i] = rows[i].size(); }
    return p;
}
}  // namespace detail

// ---- protocol/src/crypto.rs:79-155 -------------------------------------------------------------
struct LinearSecretSharingScheme {
    sda_sharing_scheme_t c{};
    static LinearSecretSharingScheme Additive(size_t share_count, int64_t modulus) {
        LinearSecretSharingScheme s;
        s.c.kind = SDA_SHARING_ADDITIVE; s.c.share_count = share_count; s.c.modulus = modulus;
        return s;
    }
    static LinearSecretSharingScheme PackedShamir(size_t secret_count, size_t share_count, size_t privacy_threshold,
                                                  int64_t prime_modulus, int64_t omega_secrets, int64_t omega_shares) {
        LinearSecretSharingScheme s;
        s.c.kind = SDA_SHARING_PACKED_SHAMIR; s.c.share_count = share_count; s.c.modulus = prime_modulus;
        s.c.secret_count = secret_count; s.c.privacy_threshold = privacy_threshold;
        s.c.omega_secrets = omega_secrets; s.c.omega_shares = omega_shares;
        return s;
    }
    size_t input_size() const { return sda_scheme_input_size(&c); }
    size_t output_size() const { return sda_scheme_output_size(&c); }
    size_t privacy_threshold() const { return sda_scheme_privacy_threshold(&c); }
    size_t reconstruction_threshold() const { return sda_scheme_reconstruction_threshold(&c); }
};

// ---- protocol/src/crypto.rs:43-75 --------------------------------------------------------------
struct LinearMaskingScheme {
    sda_masking_scheme_t c{};
    static LinearMaskingScheme None() { LinearMaskingScheme s; s.c.kind = SDA_MASKING_NONE; return s; }
    static LinearMaskingScheme Full(int64_t modulus) {
        LinearMaskingScheme s; s.c.kind = SDA_MASKING_FULL; s.c.modulus = modulus; return s;
    }
    static LinearMaskingScheme ChaCha(int64_t modulus, size_t dimension, size_t seed_bitsize) {
        LinearMaskingScheme s;
        s.c.kind = SDA_MASKING_CHACHA; s.c.modulus = modulus; s.c.dimension = dimension; s.c.seed_bitsize = seed_bitsize;
        return s;
    }
    bool has_mask() const { return sda_masking_has_mask(&c) != 0; }
};

// ---- sharing traits -----------------------------------------------------------------------------
struct ShareGenerator {
    sda_share_generator_t* h = nullptr;
    explicit ShareGenerator(const LinearSecretSharingScheme& s) { detail::check(sda_share_generator_new(&s.c, &h)); }
    // SDA_VALUES_RUST_SIGNED: the reference's own signed representatives (sda_hip.h "value representation")
    void set_value_mode(int mode) { detail::check(sda_share_generator_set_value_mode(h, mode)); }
    // which parametrisation `generate` WITHOUT injected randomness uses (sda_hip.h "CSPRNG share map"): SDA_SHARE_MAP_SYSTEMATIC
    // (the t draws of a batch are its shares 0..t-1; default of the matrix-form kernels) or SDA_SHARE_MAP_TSS_NODES
    int csprng_share_map() const { return sda_share_generator_csprng_share_map(h); }
    void set_csprng_share_map(int map) { detail::check(sda_share_generator_set_csprng_share_map(h, map)); }
    ~ShareGenerator() { sda_share_generator_free(h); }
    ShareGenerator(const ShareGenerator&) = delete;
    /// generate(&mut self, secrets) -> Vec<Vec<Share>>: outer index = clerk (batched.rs:46-48)
    std::vector<std::vector<Share>> generate(const std::vector<Secret>& secrets, const std::vector<int64_t>* rand = nullptr) {
        const size_t n = sda_share_generator_share_count(h), B = sda_share_generator_batch_count(h, secrets.size());
        std::vector<Share> flat(n * B);
        detail::check(sda_share_generator_generate(h, secrets.data(), secrets.size(), rand ? rand->data() : nullptr,
                                                   rand ? rand->size() : 0, flat.data(), flat.size()));
        std::vector<std::vector<Share>> out(n);
        for (size_t j = 0; j < n; ++j) out[j].assign(flat.begin() + j * B, flat.begin() + (j + 1) * B);
        return out;
    }
};

struct ShareCombiner {
    sda_share_combiner_t* h = nullptr;
    explicit ShareCombiner(const LinearSecretSharingScheme& s) { detail::check(sda_share_combiner_new(&s.c, &h)); }
    // SDA_VALUES_RUST_SIGNED: the reference's own signed representatives (sda_hip.h "value representation")
    void set_value_mode(int mode) { detail::check(sda_share_combiner_set_value_mode(h, mode)); }
    ~ShareCombiner() { sda_share_combiner_free(h); }
    ShareCombiner(const ShareCombiner&) = delete;
    std::vector<Share> combine(const std::vector<std::vector<Share>>& shares) const {
        std::vector<size_t> lens;
        auto ptrs = detail::row_ptrs(shares, lens);
        std::vector<Share> out(shares.empty() ? 0 : shares[0].size());
        size_t n_out = 0;
        detail::check(sda_share_combiner_combine(h, ptrs.data(), lens.data(), shares.size(), out.data(), out.size(), &n_out));
        out.resize(n_out);
        return out;
    }
};

// ---- share-vector wire codec (sodium.rs:36-41 `share.encode_var`, :83-89 `Share::decode_var` until EOF) ----------
struct ShareCodec {
    sda_varint_codec_t* h = nullptr;
    ShareCodec() { detail::check(sda_varint_codec_new(&h)); }
    ~ShareCodec() { sda_varint_codec_free(h); }
    ShareCodec(const ShareCodec&) = delete;
    std::vector<uint8_t> encode(const std::vector<Share>& shares) const {
        std::vector<uint8_t> out(sda_varint_max_encoded_size(shares.size()) + 1);
        size_t n = 0;
        detail::check(sda_varint_encode(h, shares.data(), shares.size(), out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
    std::vector<Share> decode(const std::vector<uint8_t>& raw) const {
        std::vector<Share> out(raw.size() + 1);
        size_t n = 0;
        detail::check(sda_varint_decode(h, raw.data(), raw.size(), out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
};

/// clerk.rs:78-86 as a stream (the FIXME at :71-72): begin(dimension); add(payload) per opened sealed box; finish()
struct StreamingShareCombiner {
    sda_share_combiner_t* h = nullptr;
    size_t dimension = 0;
    explicit StreamingShareCombiner(const LinearSecretSharingScheme& s) { detail::check(sda_share_combiner_new(&s.c, &h)); }
    ~StreamingShareCombiner() { sda_share_combiner_free(h); }
    StreamingShareCombiner(const StreamingShareCombiner&) = delete;
    void begin(size_t dim) { dimension = dim; detail::check(sda_share_combiner_begin(h, dim)); }
    void add(const ShareCodec& codec, const std::vector<uint8_t>& payload) {
        detail::check(sda_share_combiner_update_varint(h, codec.h, payload.data(), payload.size()));
    }
    std::vector<Share> finish() {
        std::vector<Share> out(dimension);
        detail::check(sda_share_combiner_finish(h, out.data()));
        return out;
    }
};

// client/src/crypto/encryption/sodium.rs:33-46, :72-92: ShareEncryptor::encrypt = varint encode +
// sealedbox::seal (:43); ShareDecryptor::decrypt = sealedbox::open (:78; Err("Sodium decryption failure") :80) + decode
using EncryptionKey = std::vector<uint8_t>;         // 32 bytes, EncryptionKey::Sodium
using DecryptionKey = std::vector<uint8_t>;         // 32 bytes, DecryptionKey::Sodium
using Encryption = std::vector<uint8_t>;            // Encryption::Sodium(Binary)
struct SealedBox {
    sda_sealedbox_t* h = nullptr;
    SealedBox() { detail::check(sda_sealedbox_new(&h)); }
    ~SealedBox() { sda_sealedbox_free(h); }
    SealedBox(const SealedBox&) = delete;
    SealedBox& operator=(const SealedBox&) = delete;
    EncryptionKey public_key(const DecryptionKey& sk) {            // X25519(sk, 9), for tests and tools
        EncryptionKey pk(32);
        detail::check(sda_sealedbox_public_key(h, sk.data(), pk.data()));
        return pk;
    }
    Encryption seal(const std::vector<uint8_t>& m, const EncryptionKey& pk, const uint8_t* esk = nullptr) {
        Encryption out(m.size() + SDA_SEALBYTES);
        detail::check(sda_sealedbox_seal(h, pk.data(), esk, m.data(), m.size(), out.data(), out.size()));
        return out;
    }
    std::vector<uint8_t> open(const Encryption& c, const EncryptionKey& pk, const DecryptionKey& sk) {
        std::vector<uint8_t> out(c.size() + 1);
        size_t n = 0;
        detail::check(sda_sealedbox_open(h, pk.data(), sk.data(), c.data(), c.size(), out.data(), out.size(), &n));
        out.resize(n);
        return out;
    }
};
/// The clerk's last step (clerk.rs:84-100) for a StreamingShareCombiner's job through ONE call
/// (sda_share_combiner_finish_sealed_rows_dev): the sums are reduced, encoded and sealed to the recipient, the row split over the
/// whole chip; neither the result nor its wire bytes are written to device memory in plain.  The job stays valid.  esk: null, or
/// 32 injected bytes of ephemeral secret (tests only).
inline Encryption finish_sealed(StreamingShareCombiner& comb, ShareCodec& codec, SealedBox& box, const EncryptionKey& recipient_pk,
                                const uint8_t* esk = nullptr) {
    if (recipient_pk.size() != 32) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "finish_sealed: the recipient key is 32 bytes");
    const size_t slot = sda_varint_slot_size(comb.dimension) + SDA_SEALBYTES;
    struct Dev {                                                    // freed on every way out
        void* p = nullptr;
        ~Dev() { if (p) sda_dev_free(p); }
    } d_box, d_len;
    detail::check(sda_dev_malloc(&d_box.p, slot));
    detail::check(sda_dev_malloc(&d_len.p, sizeof(uint64_t)));
    detail::check(sda_share_combiner_finish_sealed_rows_dev(comb.h, codec.h, box.h, recipient_pk.data(), esk, static_cast<uint8_t*>(d_box.p), slot,
                                                            static_cast<uint64_t*>(d_len.p), nullptr));
    detail::check(sda_dev_synchronize());
    uint64_t len = 0;
    detail::check(sda_dev_download(&len, d_len.p, sizeof len));
    if (len == 0) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "sealing refused: the recipient public key is a small-order point");
    Encryption e(len);
    detail::check(sda_dev_download(e.data(), d_box.p, len));
    return e;
}
struct ShareEncryptor {
    EncryptionKey pk; SealedBox box; ShareCodec codec;
    explicit ShareEncryptor(EncryptionKey k) : pk(std::move(k)) {}
    Encryption encrypt(const std::vector<Share>& shares) { return box.seal(codec.encode(shares), pk); }
    /// `encrypt` for a batch of share vectors of one length through ONE call (sda_sealedbox_seal_share_rows_dev): no wire
    /// buffer on the device.  esk: null, or rows * 32 injected ephemeral secrets (tests only).
    std::vector<Encryption> encrypt_rows(const std::vector<std::vector<Share>>& rows, const uint8_t* esk = nullptr) {
        std::vector<Encryption> out;
        if (rows.empty()) return out;
        const size_t n = rows.size(), len = rows[0].size(), slot = sda_varint_slot_size(len) + SDA_SEALBYTES;
        std::vector<Share> flat;
        flat.reserve(n * len);
        for (const auto& r : rows) {
            if (r.size() != len) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "encrypt_rows: share vectors of one length");
            flat.insert(flat.end(), r.begin(), r.end());
        }
        struct Dev {                                                // freed on every way out
            void* p = nullptr;
            ~Dev() { if (p) sda_dev_free(p); }
        } d_values, d_boxes, d_lens;
        detail::check(sda_dev_malloc(&d_values.p, flat.size() * sizeof(Share) + 16));
        detail::check(sda_dev_malloc(&d_boxes.p, n * slot));
        detail::check(sda_dev_malloc(&d_lens.p, n * sizeof(uint64_t)));
        if (!flat.empty()) detail::check(sda_dev_upload(d_values.p, flat.data(), flat.size() * sizeof(Share)));
        detail::check(sda_sealedbox_seal_share_rows_dev(box.h, codec.h, pk.data(), 1, n, esk, static_cast<const int64_t*>(d_values.p), n, len,
                                                        len, static_cast<uint8_t*>(d_boxes.p), slot, static_cast<uint64_t*>(d_lens.p), nullptr));
        detail::check(sda_dev_synchronize());
        std::vector<uint64_t> lens(n);
        detail::check(sda_dev_download(lens.data(), d_lens.p, n * sizeof(uint64_t)));
        for (size_t r = 0; r < n; ++r) {
            if (lens[r] == 0) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "sealing refused: the recipient public key is a small-order point");
            Encryption e(lens[r]);
            detail::check(sda_dev_download(e.data(), static_cast<const uint8_t*>(d_boxes.p) + r * slot, lens[r]));
            out.push_back(std::move(e));
        }
        return out;
    }
};
/// new_participation's sharing and encryption (participate.rs:75-101) for ONE participant through ONE call
/// (sda_share_generator_generate_sealed_rows_dev): the secrets go in, clerk c's encryption comes out at index c, and no share is
/// written to device memory on the way.  Device CSPRNG, canonical values, additive or packed Shamir with
/// secret_count + privacy_threshold <= 32.  esk: null, or share_count * 32 injected ephemeral secrets (tests only).
inline std::vector<Encryption> generate_sealed(ShareGenerator& gen, ShareCodec& codec, SealedBox& box,
                                               const std::vector<EncryptionKey>& clerk_keys, const std::vector<Secret>& secrets,
                                               const uint8_t* esk = nullptr) {
    const size_t n = sda_share_generator_share_count(gen.h);
    if (clerk_keys.size() != n) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "generate_sealed: one key per clerk");
    std::vector<uint8_t> pks;
    for (const auto& k : clerk_keys) {
        if (k.size() != 32) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "generate_sealed: a clerk key is 32 bytes");
        pks.insert(pks.end(), k.begin(), k.end());
    }
    const size_t B = sda_share_generator_batch_count(gen.h, secrets.size()), slot = sda_varint_slot_size(B) + SDA_SEALBYTES;
    struct Dev {                                                    // freed on every way out
        void* p = nullptr;
        ~Dev() { if (p) sda_dev_free(p); }
    } d_secrets, d_boxes, d_lens;
    detail::check(sda_dev_malloc(&d_secrets.p, secrets.size() * sizeof(Secret) + 16));
    detail::check(sda_dev_malloc(&d_boxes.p, n * slot));
    detail::check(sda_dev_malloc(&d_lens.p, n * sizeof(uint64_t)));
    if (!secrets.empty()) detail::check(sda_dev_upload(d_secrets.p, secrets.data(), secrets.size() * sizeof(Secret)));
    detail::check(sda_share_generator_generate_sealed_rows_dev(gen.h, codec.h, box.h, pks.data(), esk, static_cast<const int64_t*>(d_secrets.p), 1,
                                                               secrets.size(), secrets.size(), 0, static_cast<uint8_t*>(d_boxes.p), slot,
                                                               static_cast<uint64_t*>(d_lens.p), nullptr));
    detail::check(sda_dev_synchronize());
    std::vector<uint64_t> lens(n);
    detail::check(sda_dev_download(lens.data(), d_lens.p, n * sizeof(uint64_t)));
    std::vector<Encryption> out;
    for (size_t c = 0; c < n; ++c) {
        if (lens[c] == 0) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "sealing refused: a clerk public key is a small-order point");
        Encryption e(lens[c]);
        detail::check(sda_dev_download(e.data(), static_cast<const uint8_t*>(d_boxes.p) + c * slot, lens[c]));
        out.push_back(std::move(e));
    }
    return out;
}
struct ShareDecryptor {
    EncryptionKey pk; DecryptionKey sk; SealedBox box; ShareCodec codec;
    ShareDecryptor(EncryptionKey p, DecryptionKey s) : pk(std::move(p)), sk(std::move(s)) {}
    std::vector<Share> decrypt(const Encryption& e) { return codec.decode(box.open(e, pk, sk)); }
};

// The clerking job as one binary blob: what server/src/stores.rs:86-101 would emit instead of
// Vec<Vec<Encryption>>; layout in sda_hip.h ("SDAJOBv1").
struct JobContainer {
    std::vector<uint8_t> blob;
    sda_job_layout_t layout{};
    static JobContainer build(uint32_t kind, const std::vector<std::vector<uint8_t>>& payloads) {
        size_t longest = 0;
        for (const auto& p : payloads) longest = p.size() > longest ? p.size() : longest;
        JobContainer j;
        const size_t slot = sda_job_slot_size(longest);
        const size_t size = sda_job_container_size(payloads.size(), slot);
        j.blob.resize(size < 64 ? 64 : size);
        detail::check(sda_job_container_init(j.blob.data(), j.blob.size(), kind, payloads.size(), slot, &j.layout));
        for (size_t r = 0; r < payloads.size(); ++r)
            detail::check(sda_job_container_set_row(j.blob.data(), j.blob.size(), r, payloads[r].data(), payloads[r].size()));
        return j;
    }
    static JobContainer parse(std::vector<uint8_t> bytes) {
        JobContainer j;
        j.blob = std::move(bytes);
        detail::check(sda_job_container_parse(j.blob.data(), j.blob.size(), &j.layout));
        return j;
    }
    std::vector<uint8_t> row(size_t r) const {
        const uint8_t* p = nullptr;
        size_t n = 0;
        detail::check(sda_job_container_get_row(blob.data(), blob.size(), r, &p, &n));
        return std::vector<uint8_t>(p, p + n);
    }
};

struct SecretReconstructor {
    sda_secret_reconstructor_t* h = nullptr;
    size_t dimension;
    SecretReconstructor(const LinearSecretSharingScheme& s, size_t dim) : dimension(dim) {
        detail::check(sda_secret_reconstructor_new(&s.c, dim, &h));
    }
    ~SecretReconstructor() { sda_secret_reconstructor_free(h); }
    void set_value_mode(int mode) { detail::check(sda_secret_reconstructor_set_value_mode(h, mode)); }
    SecretReconstructor(const SecretReconstructor&) = delete;
    std::vector<Secret> reconstruct(const std::vector<std::pair<size_t, std::vector<Share>>>& indexed_shares) const {
        HostCall c(indexed_shares, 0, 0);
        size_t cap = dimension;
        for (size_t len : c.lens) cap = len > cap ? len : cap;
        c.out.resize(cap);
        detail::check(sda_secret_reconstructor_reconstruct(h, c.idx.data(), c.ptrs.data(), c.lens.data(), c.idx.size(), c.out.data(), cap, &c.n_out));
        c.out.resize(c.n_out);
        return std::move(c.out);
    }
    // the same as a streaming job on device-resident rows (receive.rs:120-146); no update synchronises the stream.  indices[i] is
    // the clerk index of position i (Additive: may be empty); a position is fed once, in any order, by either update form
    void begin_dev(const std::vector<size_t>& indices, size_t n_rows, size_t row_len, void* stream = nullptr) {
        if (!indices.empty() && indices.size() != n_rows) detail::check(SDA_ERR_INVALID_ARGUMENT);
        detail::check(sda_secret_reconstructor_begin_dev(h, indices.empty() ? nullptr : indices.data(), n_rows, row_len, stream));
    }
    void update_dev(size_t first_pos, const int64_t* d_shares, size_t rows, size_t row_stride, void* stream = nullptr) {
        detail::check(sda_secret_reconstructor_update_dev(h, first_pos, d_shares, rows, row_stride, stream));
    }
    // clerking results that are still sealed boxes, laid out as for sda_sealedbox_open_rows_dev; *d_status != 0: do not use the result
    void update_sealed_rows_dev(ShareCodec& codec, SealedBox& box, const EncryptionKey& pk, const DecryptionKey& sk, size_t first_pos,
                                const uint8_t* d_boxes, size_t slot_bytes, const uint64_t* d_row_bytes, size_t rows,
                                size_t max_box_bytes, uint32_t* d_status, uint32_t* d_ok = nullptr, void* stream = nullptr) {
        detail::check(sda_secret_reconstructor_update_sealed_rows_dev(h, codec.h, box.h, pk.data(), sk.data(), first_pos, d_boxes, slot_bytes,
                                                                      d_row_bytes, rows, max_box_bytes, d_ok, d_status, stream));
    }
    void finish_dev(int64_t* d_out, size_t out_cap, void* stream = nullptr) {
        detail::check(sda_secret_reconstructor_finish_dev(h, d_out, out_cap, stream));
    }
    // the checked job (PackedShamir): `checks` parity columns ride behind the k secret columns, the updates above feed it, and the
    // finish reports which positions disagree with the others (sda_hip.h: the report words, the Reed-Solomon limits)
    struct RevealCheck {
        uint64_t bad = 0, located = 0, corrected = 0, first_bad = ~0ull;     // first_bad: 2^64 - 1 = none
        std::vector<uint64_t> blame;                                          // per position of the index set
        bool clean() const { return bad == 0; }
        static RevealCheck from_words(const std::vector<uint64_t>& w) {
            RevealCheck c;
            c.bad = w[0]; c.located = w[1]; c.corrected = w[2]; c.first_bad = w[3];
            c.blame.assign(w.begin() + 4, w.end());
            return c;
        }
    };
    void begin_checked_dev(const std::vector<size_t>& indices, size_t n_rows, size_t row_len, unsigned checks, void* stream = nullptr) {
        if (indices.size() != n_rows) detail::check(SDA_ERR_INVALID_ARGUMENT);
        detail::check(sda_secret_reconstructor_begin_checked_dev(h, indices.empty() ? nullptr : indices.data(), n_rows, row_len, checks, stream));
    }
    // d_report: sda_reconstruct_report_words(n_rows) device words; nothing synchronises or reaches the host
    void finish_checked_dev(int64_t* d_out, size_t out_cap, uint64_t* d_report, bool correct = false, void* stream = nullptr) {
        detail::check(sda_secret_reconstructor_finish_checked_dev(h, correct ? SDA_CHECK_CORRECT : SDA_CHECK_REPORT, d_out, out_cap, d_report,
                                                                  stream));
    }
    std::pair<std::vector<Secret>, RevealCheck> reconstruct_checked(const std::vector<std::pair<size_t, std::vector<Share>>>& indexed_shares,
                                                                    unsigned checks, bool correct = false) const {
        HostCall c(indexed_shares, dimension, sda_reconstruct_report_words(indexed_shares.size()));
        detail::check(sda_secret_reconstructor_reconstruct_checked(h, c.idx.data(), c.ptrs.data(), c.lens.data(), c.idx.size(), checks,
                                                                   correct ? SDA_CHECK_CORRECT : SDA_CHECK_REPORT, c.out.data(), dimension,
                                                                   &c.n_out, c.words.data()));
        c.out.resize(c.n_out);
        return {std::move(c.out), RevealCheck::from_words(c.words)};
    }
    // the decoding finish of a checked job: up to max_errors (0: checks / 2) disagreeing positions per batch are named and, on
    // request, repaired (sda_hip.h: the report words, what a cap guarantees)
    struct RevealDecode {
        uint64_t bad = 0, decoded = 0, corrected = 0, first_bad = ~0ull, first_undecoded = ~0ull, most = 0;   // 2^64 - 1 = none
        std::array<uint64_t, 8> by_count{};                                   // by_count[nu - 1]: batches decoded with nu positions
        std::vector<uint64_t> blame;                                          // per position of the index set
        bool clean() const { return bad == 0; }
        static RevealDecode from_words(const std::vector<uint64_t>& w) {
            RevealDecode d;
            d.bad = w[0]; d.decoded = w[1]; d.corrected = w[2]; d.first_bad = w[3]; d.first_undecoded = w[4]; d.most = w[5];
            for (size_t i = 0; i < 8; ++i) d.by_count[i] = w[8 + i];
            d.blame.assign(w.begin() + 16, w.end());
            return d;
        }
    };
    // d_report: sda_reconstruct_decode_report_words(n_rows) device words; nothing synchronises or reaches the host
    void finish_decoded_dev(int64_t* d_out, size_t out_cap, uint64_t* d_report, unsigned max_errors = 0, bool correct = false,
                            void* stream = nullptr) {
        detail::check(sda_secret_reconstructor_finish_decoded_dev(h, max_errors, correct ? SDA_CHECK_CORRECT : SDA_CHECK_REPORT, d_out, out_cap,
                                                                  d_report, stream));
    }
    std::pair<std::vector<Secret>, RevealDecode> reconstruct_decoded(const std::vector<std::pair<size_t, std::vector<Share>>>& indexed_shares,
                                                                     unsigned checks, unsigned max_errors = 0, bool correct = false) const {
        HostCall c(indexed_shares, dimension, sda_reconstruct_decode_report_words(indexed_shares.size()));
        detail::check(sda_secret_reconstructor_reconstruct_decoded(h, c.idx.data(), c.ptrs.data(), c.lens.data(), c.idx.size(), checks, max_errors,
                                                                   correct ? SDA_CHECK_CORRECT : SDA_CHECK_REPORT, c.out.data(), dimension,
                                                                   &c.n_out, c.words.data()));
        c.out.resize(c.n_out);
        return {std::move(c.out), RevealDecode::from_words(c.words)};
    }
    // the erasure finish of a checked job: positions known to be unreliable - the rows a sealed update refused - cost one check each,
    // not two.  d_ok: n_rows device words, 0 = erased (what update_sealed_rows_dev writes; nullptr: none), read by the kernels alone.
    // d_report as for finish_decoded_dev, [6] = the number of erased positions, [7] = 1 when they are more than checks
    void finish_erasures_dev(const uint32_t* d_ok, int64_t* d_out, size_t out_cap, uint64_t* d_report, unsigned max_errors = 0,
                             bool correct = false, void* stream = nullptr) {
        detail::check(sda_secret_reconstructor_finish_erasures_dev(h, d_ok, max_errors, correct ? SDA_CHECK_CORRECT : SDA_CHECK_REPORT, d_out,
                                                                   out_cap, d_report, stream));
    }
    struct Erasures {
        std::vector<Secret> values;
        RevealDecode decode;
        uint64_t erased = 0;                                                  // as the device counted them
        bool unrepaired = false;                                              // more erased rows than checks
    };
    // erased: one byte per row, non-zero = erased; empty = none
    Erasures reconstruct_erasures(const std::vector<std::pair<size_t, std::vector<Share>>>& indexed_shares, const std::vector<uint8_t>& erased,
                                  unsigned checks, unsigned max_errors = 0, bool correct = false) const {
        if (!erased.empty() && erased.size() != indexed_shares.size()) detail::check(SDA_ERR_INVALID_ARGUMENT);
        HostCall c(indexed_shares, dimension, sda_reconstruct_decode_report_words(indexed_shares.size()));
        detail::check(sda_secret_reconstructor_reconstruct_erasures(h, c.idx.data(), c.ptrs.data(), c.lens.data(), c.idx.size(), checks,
                                                                    erased.empty() ? nullptr : erased.data(), max_errors,
                                                                    correct ? SDA_CHECK_CORRECT : SDA_CHECK_REPORT, c.out.data(), dimension,
                                                                    &c.n_out, c.words.data()));
        c.out.resize(c.n_out);
        return {std::move(c.out), RevealDecode::from_words(c.words), c.words[6], c.words[7] != 0};
    }

private:
    // the arguments of a host reconstruct call: indexed_shares unpacked, the output and the report sized
    struct HostCall {
        std::vector<size_t> idx, lens;
        std::vector<const int64_t*> ptrs;
        std::vector<Secret> out;
        std::vector<uint64_t> words;
        size_t n_out = 0;
        HostCall(const std::vector<std::pair<size_t, std::vector<Share>>>& s, size_t out_cap, size_t n_words)
            : idx(s.size()), lens(s.size()), ptrs(s.size()), out(out_cap ? out_cap : 1), words(n_words) {
            for (size_t i = 0; i < s.size(); ++i) { idx[i] = s[i].first; ptrs[i] = s[i].second.data(); lens[i] = s[i].second.size(); }
        }
    };
};

// ---- masking traits -----------------------------------------------------------------------------
struct SecretMasker {
    sda_secret_masker_t* h = nullptr;
    explicit SecretMasker(const LinearMaskingScheme& s) { detail::check(sda_secret_masker_new(&s.c, &h)); }
    // SDA_VALUES_RUST_SIGNED: the reference's own signed representatives (sda_hip.h "value representation")
    void set_value_mode(int mode) { detail::check(sda_secret_masker_set_value_mode(h, mode)); }
    ~SecretMasker() { sda_secret_masker_free(h); }
    SecretMasker(const SecretMasker&) = delete;
    std::pair<std::vector<Mask>, std::vector<MaskedSecret>> mask(const std::vector<Secret>& secrets,
                                                                 const std::vector<int64_t>* rand = nullptr) {
        std::vector<Mask> m(sda_secret_masker_mask_len(h, secrets.size()));
        std::vector<MaskedSecret> ms(secrets.size());
        size_t n_mask = 0;
        detail::check(sda_secret_masker_mask(h, secrets.data(), secrets.size(), rand ? rand->data() : nullptr,
                                             rand ? rand->size() : 0, m.data(), m.size(), &n_mask, ms.data()));
        m.resize(n_mask);
        return {m, ms};
    }
};
/// new_participation's masking and recipient encryption (participate.rs:52-72) for ONE participant through ONE call
/// (sda_secret_masker_mask_sealed_rows_dev): the secrets go in, the masked secrets and the mask's encryption for the recipient
/// come out.  Full: the mask is never written to device memory; ChaCha: the sealed mask is the seed.  The None scheme has no
/// recipient encryption (SDA_ERR_UNSUPPORTED).  esk: null, or 32 bytes of an injected ephemeral secret (tests only).
inline std::pair<Encryption, std::vector<MaskedSecret>> mask_sealed(SecretMasker& masker, ShareCodec& codec, SealedBox& box,
                                                                    const EncryptionKey& recipient_key,
                                                                    const std::vector<Secret>& secrets, const uint8_t* esk = nullptr) {
    if (recipient_key.size() != 32) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "mask_sealed: the recipient key is 32 bytes");
    const size_t len = secrets.size(), slot = sda_varint_slot_size(sda_secret_masker_mask_len(masker.h, len)) + SDA_SEALBYTES;
    struct Dev {                                                    // freed on every way out
        void* p = nullptr;
        ~Dev() { if (p) sda_dev_free(p); }
    } d_secrets, d_masked, d_box, d_len;
    detail::check(sda_dev_malloc(&d_secrets.p, len * sizeof(Secret) + 16));
    detail::check(sda_dev_malloc(&d_masked.p, len * sizeof(MaskedSecret) + 16));
    detail::check(sda_dev_malloc(&d_box.p, slot));
    detail::check(sda_dev_malloc(&d_len.p, sizeof(uint64_t)));
    if (len) detail::check(sda_dev_upload(d_secrets.p, secrets.data(), len * sizeof(Secret)));
    detail::check(sda_secret_masker_mask_sealed_rows_dev(masker.h, codec.h, box.h, recipient_key.data(), esk,
                                                         static_cast<const int64_t*>(d_secrets.p), 1, len, len, 0,
                                                         static_cast<int64_t*>(d_masked.p), len, static_cast<uint8_t*>(d_box.p), slot,
                                                         static_cast<uint64_t*>(d_len.p), nullptr));
    detail::check(sda_dev_synchronize());
    uint64_t n = 0;
    detail::check(sda_dev_download(&n, d_len.p, sizeof n));
    if (n == 0) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "sealing refused: the recipient public key is a small-order point");
    Encryption e(n);
    detail::check(sda_dev_download(e.data(), d_box.p, n));
    std::vector<MaskedSecret> ms(len);
    if (len) detail::check(sda_dev_download(ms.data(), d_masked.p, len * sizeof(MaskedSecret)));
    return {e, ms};
}

struct MaskCombiner {
    sda_mask_combiner_t* h = nullptr;
    size_t chacha_dimension = 0;
    explicit MaskCombiner(const LinearMaskingScheme& s) {
        if (s.c.kind == SDA_MASKING_CHACHA) chacha_dimension = s.c.dimension;
        detail::check(sda_mask_combiner_new(&s.c, &h));
    }
    ~MaskCombiner() { sda_mask_combiner_free(h); }
    void set_value_mode(int mode) { detail::check(sda_mask_combiner_set_value_mode(h, mode)); }
    MaskCombiner(const MaskCombiner&) = delete;
    std::vector<Mask> combine(const std::vector<std::vector<Mask>>& masks) const {
        std::vector<size_t> lens;
        auto ptrs = detail::row_ptrs(masks, lens);
        std::vector<Mask> out(chacha_dimension ? chacha_dimension : (masks.empty() ? 0 : masks[0].size()));
        size_t n_out = 0;
        detail::check(sda_mask_combiner_combine(h, ptrs.data(), lens.data(), masks.size(), out.data(), out.size(), &n_out));
        out.resize(n_out);
        return out;
    }
    // the same sums as a streaming job on device-resident rows (receive.rs:101-118); nothing here synchronises the stream
    void begin_dev(size_t dimension, void* stream = nullptr) { detail::check(sda_mask_combiner_begin_dev(h, dimension, stream)); }
    void update_dev(const int64_t* d_rows, size_t rows, size_t row_len, size_t row_stride, void* stream = nullptr) {
        detail::check(sda_mask_combiner_update_dev(h, d_rows, rows, row_len, row_stride, stream));
    }
    // the participants' sealed mask encryptions, laid out as for sda_sealedbox_open_rows_dev; *d_status != 0: do not use the result
    void update_sealed_rows_dev(ShareCodec& codec, SealedBox& box, const EncryptionKey& pk, const DecryptionKey& sk,
                                const uint8_t* d_boxes, size_t slot_bytes, const uint64_t* d_row_bytes, size_t rows,
                                size_t max_box_bytes, uint32_t* d_status, uint32_t* d_ok = nullptr, void* stream = nullptr) {
        detail::check(sda_mask_combiner_update_sealed_rows_dev(h, codec.h, box.h, pk.data(), sk.data(), d_boxes, slot_bytes, d_row_bytes,
                                                               rows, max_box_bytes, d_ok, d_status, stream));
    }
    void finish_dev(int64_t* d_out, size_t out_cap, void* stream = nullptr) {
        detail::check(sda_mask_combiner_finish_dev(h, d_out, out_cap, stream));
    }
};

struct SecretUnmasker {
    sda_secret_unmasker_t* h = nullptr;
    explicit SecretUnmasker(const LinearMaskingScheme& s) { detail::check(sda_secret_unmasker_new(&s.c, &h)); }
    // SDA_VALUES_RUST_SIGNED: the reference's own signed representatives (sda_hip.h "value representation")
    void set_value_mode(int mode) { detail::check(sda_secret_unmasker_set_value_mode(h, mode)); }
    ~SecretUnmasker() { sda_secret_unmasker_free(h); }
    SecretUnmasker(const SecretUnmasker&) = delete;
    std::vector<Secret> unmask(const std::pair<std::vector<Mask>, std::vector<MaskedSecret>>& values) const {
        std::vector<Secret> out(values.second.size());
        detail::check(sda_secret_unmasker_unmask(h, values.first.data(), values.first.size(), values.second.data(),
                                                 values.second.size(), out.data()));
        return out;
    }
    // the recipient's last step for a CHECKED reconstructor job (begin_checked_dev, every position fed) and a mask combiner job,
    // through ONE call (sda_secret_unmasker_unmask_checked_jobs_dev): end = SDA_CHECKED_END_LOCATE / _DECODE / _ERASURES names the
    // finish whose verdicts and report (d_report, that finish's words) are wanted; d_out is that finish's output unmasked, with
    // neither the masked output nor the combined mask in device memory.  Ends both jobs.  d_status_*: the status words of the jobs'
    // sealed updates as gates - *d_status_masks != 0 or (*d_status_results & ~results_pass_bits) != 0 when the kernel runs and
    // nothing is stored to d_out (the report is written all the same); results_pass_bits: 0, or 16 for the caller who repairs
    // refused boxes.  combiner: null for a None unmasker only.  Nothing synchronises or reaches the host
    void unmask_checked_jobs_dev(MaskCombiner* combiner, SecretReconstructor& reconstructor, int end, int64_t* d_out, size_t out_cap,
                                 uint64_t* d_report, const uint32_t* d_ok = nullptr, unsigned max_errors = 0, bool correct = false,
                                 const uint32_t* d_status_masks = nullptr, const uint32_t* d_status_results = nullptr,
                                 uint32_t results_pass_bits = 0, void* stream = nullptr) {
        detail::check(sda_secret_unmasker_unmask_checked_jobs_dev(h, combiner ? combiner->h : nullptr, reconstructor.h, end, d_ok, max_errors,
                                                                  correct ? SDA_CHECK_CORRECT : SDA_CHECK_REPORT, d_status_masks,
                                                                  d_status_results, results_pass_bits, d_out, out_cap, d_report, stream));
    }
};

/// The recipient's last step (receive.rs:148-156) for a MaskCombiner job and a SecretReconstructor job, both begun and fed on the
/// device, through ONE call (sda_secret_unmasker_unmask_jobs_dev): their sums are folded and unmasked by one kernel, neither the
/// combined mask nor the masked output is written to device memory, and both jobs are ended.  out_len: the reconstructor job's
/// output length (PackedShamir: its dimension; Additive: row_len).  d_status_masks / d_status_results: the status words of the
/// jobs' sealed updates (device pointers, may be null or equal) - they gate the kernel's stores, and one that is non-zero
/// afterwards fails the reveal here with the reference's "Sodium decryption failure" (sodium.rs:80).  combiner: null for a None
/// unmasker only.
inline std::vector<Secret> unmask_jobs(SecretUnmasker& unmasker, MaskCombiner* combiner, SecretReconstructor& reconstructor, size_t out_len,
                                       const uint32_t* d_status_masks = nullptr, const uint32_t* d_status_results = nullptr,
                                       void* stream = nullptr) {
    struct Dev {                                                    // freed on every way out
        void* p = nullptr;
        ~Dev() { if (p) sda_dev_free(p); }
    } d_out;
    detail::check(sda_dev_malloc(&d_out.p, out_len * sizeof(Secret) + 16));
    detail::check(sda_secret_unmasker_unmask_jobs_dev(unmasker.h, combiner ? combiner->h : nullptr, reconstructor.h, d_status_masks,
                                                      d_status_results, static_cast<int64_t*>(d_out.p), out_len, stream));
    detail::check(sda_dev_synchronize());
    for (const uint32_t* d_status : {d_status_masks, d_status_results}) {
        uint32_t status = 0;
        if (d_status) detail::check(sda_dev_download(&status, d_status, sizeof status));
        if (status & 16) throw SdaClientError(SDA_ERR_SODIUM_DECRYPTION, "Sodium decryption failure");
        if (status & 2) throw SdaClientError(SDA_ERR_WRONG_DIMENSION, "Wrong dimension");
        if (status) throw SdaClientError(SDA_ERR_INVALID_ARGUMENT, "malformed varint stream");
    }
    std::vector<Secret> out(out_len);
    if (out_len) detail::check(sda_dev_download(out.data(), d_out.p, out_len * sizeof(Secret)));
    return out;
}

// ---- client/src/crypto/mod.rs:58-66 + the six *Construction traits ---------------------------------
struct CryptoModule {
    std::unique_ptr<ShareGenerator> new_share_generator(const LinearSecretSharingScheme& s) const { return std::make_unique<ShareGenerator>(s); }
    std::unique_ptr<ShareCombiner> new_share_combiner(const LinearSecretSharingScheme& s) const { return std::make_unique<ShareCombiner>(s); }
    std::unique_ptr<SecretReconstructor> new_secret_reconstructor(const LinearSecretSharingScheme& s, size_t dimension) const {
        return std::make_unique<SecretReconstructor>(s, dimension);
    }
    std::unique_ptr<SecretMasker> new_secret_masker(const LinearMaskingScheme& s) const { return std::make_unique<SecretMasker>(s); }
    std::unique_ptr<MaskCombiner> new_mask_combiner(const LinearMaskingScheme& s) const { return std::make_unique<MaskCombiner>(s); }
    std::unique_ptr<SecretUnmasker> new_secret_unmasker(const LinearMaskingScheme& s) const { return std::make_unique<SecretUnmasker>(s); }
};

// ---- client/src/receive.rs:7-21 ---------------------------------------------------------------------
struct RecipientOutput {
    int64_t modulus;
    std::vector<int64_t> values;
    RecipientOutput positive() const {
        RecipientOutput o{modulus, std::vector<int64_t>(values.size())};
        detail::check(sda_positive(values.data(), values.size(), modulus, o.values.data()));
        return o;
    }
};

}  // namespace sda_client

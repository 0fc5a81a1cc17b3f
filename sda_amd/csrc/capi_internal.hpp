// helpers shared by the translation units of the C ABI (sda_capi.cpp owns them)
#pragma once
#include <stdint.h>

#include "kernels.hpp"

int capi_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // sets sda_last_error(), returns code
int capi_make_mod(int64_t modulus, sda::ModParams& mod);                                  // validated Barrett / Lemire constants
int capi_device_ready();                                                                  // a device exists; make the selected one current
struct sda_sealedbox;
// rows that are still sealed boxes, as every update_sealed_rows_dev entry point takes them (the SDAJOBv1 SEALED layout)
struct SealedRows {
    const uint8_t* d_boxes; size_t slot_bytes; const uint64_t* d_row_bytes; size_t rows, max_box_bytes;
    uint32_t *d_ok, *d_status;
};
// first half of a sealed-box open on the handle's scratch (sda_sealedbox.cpp): every tag verified, d_ok / *d_status |= 16 /
// SboxState.bad written as sda_sealedbox_open_rows_dev writes them, NO keystream pass.  *d_states: the per-row states.
int capi_sealedbox_verify_rows(sda_sealedbox* b, const uint8_t pk[32], const uint8_t sk[32], const SealedRows& R, int device, hipStream_t s,
                               const sda::SboxState** d_states);
// the keys of a seal: row r goes to pks[r / rows_per_key]; esk: a secret per row, NULL draws them from the OS
struct SealKeys { const uint8_t* pks; size_t n_pks, rows_per_key; const uint8_t* esk; };
// the encode pass of a seal, by reference (two words, no allocation): a callable (const SboxState* d_states, uint64_t* d_msg_bytes,
// hipStream_t) -> hipError_t that must outlive the call it is passed to - a lambda written in the argument list does
class EncodePass {
    const void* f_;
    hipError_t (*call_)(const void*, const sda::SboxState*, uint64_t*, hipStream_t);
public:
    template <typename F>
    EncodePass(const F& f) : f_(&f), call_([](const void* p, const sda::SboxState* st, uint64_t* lens, hipStream_t s) { return (*static_cast<const F*>(p))(st, lens, s); }) {}
    hipError_t operator()(const sda::SboxState* st, uint64_t* lens, hipStream_t s) const { return call_(f_, st, lens, s); }
};
// every sealed-row producer after its argument checks (sda_sealedbox.cpp), all on the handle's scratch: stage the keys, setup, the
// caller's encode + encrypt pass, authenticate, wipe the ephemeral secrets.  max_msg: a row's longest plaintext; what: for the error text
int capi_sealedbox_seal(sda_sealedbox* b, const SealKeys& K, size_t rows, size_t max_msg, uint8_t* d_boxes, size_t slot_bytes,
                        uint64_t* d_row_bytes, hipStream_t s, const char* what, EncodePass encode);
int capi_sealedbox_device(const sda_sealedbox* b);

// ---- path-selection knobs (A/B measurements and parity tests of the non-default kernels) -----------------------------------
// A release build of the library reads NO environment variable: a knob changes only through the test-only entry point
// sda_debug_set_knob (include/sda_hip_debug.h).  Built with -DSDA_AB_KNOBS (tools/build_ab_variant.sh, never build()), a
// knob left unset falls back to the environment variable of the same name, for shell-driven A/B runs.
namespace sda {
enum Knob {
    KNOB_FORCE_GENERIC, KNOB_FORCE_MONT64, KNOB_FORCE_FFT, KNOB_FORCE_MFMA, KNOB_NO_MFMA, KNOB_NO_SIDE_STREAM,
    KNOB_SIDE_STREAM_WGS, KNOB_SIDE_STREAM_PRIORITY_HIGH, KNOB_FFT_G, KNOB_FFT_THREADS, KNOB_VARINT_PATH /* 1 stream, 2 scan */,
    KNOB_FORCE_COLLECTIVES, KNOB_NO_NARROW, KNOB_WIRE_WG_PER_CU, KNOB_SBOX_WG_PER_CU, KNOB_NO_LAZY, KNOB_NO_XCD_MAP, KNOB_NO_NGEMM, KNOB_NO_WIDE_GROUP, KNOB_NGEMM_CLERK_WG, KNOB_NO_KARATSUBA,
    KNOB_SEALED_WAVES /* 16: the wide instance */, KNOB_GENSEAL_BY_ROWS /* share_seal_stream_kernel: consecutive rows per workgroup */,
    KNOB_COUNT
};
long knob(Knob k);             // 0 = unset / default
// an UNUSED dynamic-LDS request that caps the resident workgroups of a launch at wg_per_cu per CU (0: no cap), so that a
// kernel bound by one resource leaves wave slots to a kernel bound by another on a second stream (DESIGN.md 5 "Schedules")
inline unsigned residency_pad_bytes(long wg_per_cu, unsigned static_lds) {
    if (wg_per_cu <= 0) return 0u;
    const unsigned share = (160u * 1024u) / (unsigned)wg_per_cu;
    const unsigned pad = share > static_lds + 256u ? share - static_lds - 256u : 0u;
    return pad > 64u * 1024u - static_lds ? 64u * 1024u - static_lds : pad;        // within the default per-workgroup limit
}
}  // namespace sda

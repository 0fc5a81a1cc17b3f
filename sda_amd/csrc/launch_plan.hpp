// Host arithmetic of the share-generation launchers: how a (participant, block)-indexed grid is cut into launches that respect
// the grid limit, and how a run-time ChaCha round count reaches a template argument.  Host only and no HIP runtime call, so that
// tests/cpp/launch_plan_test.cpp can drive it with g++ (tests/test_launch_plan_cpu.py); the callables do the launching.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "kernels.hpp"

namespace sda {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// workgroups per launch, sda_kernels.hip (256 threads each): HIP limits a launch to < 2^32 work-items per grid dimension
constexpr uint64_t kMaxBlocks = 0xFFFFFFFFull / 256;
// workgroups per launch, the transform and limb-GEMM launchers (fft_kernels.hip, ngemm_kernels.hip): kept as found - it does
// not follow from the work-item limit above, so a grid of 2^32 work-items or more under this cap is left to the runtime to refuse
constexpr uint64_t kMaxBlocksI31 = 0x7FFFFFFFull;

// (participant, block)-indexed kernels are launched in slices of participants that respect the limit; 0: not even one fits
inline uint64_t participants_per_launch(uint64_t blocks_per_participant, uint64_t participants, uint64_t max_blocks) {
    if (blocks_per_participant == 0 || blocks_per_participant > max_blocks) return 0;
    const uint64_t m = max_blocks / blocks_per_participant;
    return m < participants ? m : participants;
}

// participants p0 .. p0 + count - 1 of L as a layout of their own
inline GenLayout slice(const GenLayout& L, uint64_t p0, uint64_t count) {
    GenLayout S = L;
    S.secrets = L.secrets + p0 * L.secrets_stride;
    if (L.rand) S.rand = L.rand + p0 * L.rand_stride;
    S.out = L.out + p0 * L.out_stride_participant;
    S.participants = count;
    S.first_participant = L.first_participant + p0;
    return S;
}

// launch(p0, count, blocks) -> hipError_t for every slice in order, blocks = blocks_per_participant * count <= max_blocks; stops
// at the first error.  Nothing to do: hipSuccess; one participant alone above the limit: hipErrorInvalidConfiguration, no call
template <typename Launch>
hipError_t for_participant_ranges(uint64_t participants, uint64_t blocks_per_participant, uint64_t max_blocks, Launch&& launch) {
    if (blocks_per_participant == 0 || participants == 0) return hipSuccess;
    const uint64_t per = participants_per_launch(blocks_per_participant, participants, max_blocks);
    if (per == 0) return hipErrorInvalidConfiguration;
    for (uint64_t p0 = 0; p0 < participants; p0 += per) {
        const uint64_t count = per < participants - p0 ? per : participants - p0;
        if (hipError_t e = launch(p0, count, blocks_per_participant * count)) return e;
    }
    return hipSuccess;
}

// the same over a layout: launch(S, blocks) with S = slice(L, p0, count)
template <typename Launch>
hipError_t for_participant_slices(const GenLayout& L, uint64_t blocks_per_participant, uint64_t max_blocks, Launch&& launch) {
    return for_participant_ranges(L.participants, blocks_per_participant, max_blocks,
                                  [&](uint64_t p0, uint64_t count, uint64_t blocks) { return launch(slice(L, p0, count), blocks); });
}

// the ChaCha round counts the kernels are compiled for
inline bool rounds_supported(int rounds) { return rounds == 20 || rounds == 12 || rounds == 8; }

// f(std::integral_constant<int, ROUNDS>{}) -> hipError_t for a supported round count (decltype(R)::value is the template
// argument); hipErrorInvalidValue, and no call, for any other
template <typename F>
hipError_t with_rounds(int rounds, F&& f) {
    switch (rounds) {
        case 20: return f(std::integral_constant<int, 20>{});
        case 12: return f(std::integral_constant<int, 12>{});
        case 8: return f(std::integral_constant<int, 8>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace sda

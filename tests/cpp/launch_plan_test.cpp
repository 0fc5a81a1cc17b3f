// Host unit test of sda_amd/csrc/launch_plan.hpp (the slice loop and the round-count dispatch every share-generation launcher goes
// through): the loop's callable is bound to a recorder, and what it saw is printed for tests/test_launch_plan_cpu.py to compare
// with plain integers, through an -O2 build and through one built with -fsanitize=undefined.  No pointer here is dereferenced
// and nothing is launched.  The first line of output names the error codes:
//   codes <hipSuccess> <hipErrorInvalidValue> <hipErrorInvalidConfiguration> <the recorder's own error>
// then one line per line of stdin:
//   loop <cap> <blocks_per_participant> <participants> <with_rand> <fail_at>      for_participant_slices over the layout below; the
//        recorder fails at call fail_at (-1: never) ->  <ret> <calls> then per call  p0:count:blocks:secrets:rand:out:same
//        (offsets in elements from the layout's pointers, rand -1 when null; same = 1 when len, the strides and direct_rows are L's)
//   range <cap> <blocks_per_participant> <participants> <fail_at>                 for_participant_ranges -> <ret> <calls> then p0:count:blocks
//   slice <secrets> <secrets_stride> <rand> <rand_stride> <out> <out_stride_participant> <out_stride_clerk> <participants> <len>
//        <first_participant> <direct_rows> <p0> <count>  ->  the eleven fields of slice(L, p0, count), pointers as addresses
//   rounds <r>  ->  <ret> <calls> <the constant f was given, 0 when not called> <rounds_supported>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../sda_amd/csrc/launch_plan.hpp"

static const hipError_t kRecorderError = hipErrorUnknown;
static const size_t kSecretsStride = 3, kRandStride = 7, kOutStrideParticipant = 5, kOutStrideClerk = 11, kLen = 13;
static const uint64_t kFirst = 1000;

static int64_t* fake(uintptr_t address) { return reinterpret_cast<int64_t*>(address); }
static uintptr_t address(const void* p) { return reinterpret_cast<uintptr_t>(p); }

int main() {
    printf("codes %d %d %d %d\n", (int)hipSuccess, (int)hipErrorInvalidValue, (int)hipErrorInvalidConfiguration, (int)kRecorderError);
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "loop") || !strcmp(cmd, "range")) {
            const bool layout = cmd[0] == 'l';
            uint64_t cap, bpp, participants;
            int with_rand = 0;
            long long fail_at;
            if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &cap, &bpp, &participants) != 3) return 1;
            if (layout && scanf("%d", &with_rand) != 1) return 1;
            if (scanf("%lld", &fail_at) != 1) return 1;
            long long calls = 0;
            std::string seen;
            char buf[256];
            hipError_t ret;
            if (layout) {
                const sda::GenLayout L{fake(1 << 20), kSecretsStride, with_rand ? fake(2 << 20) : nullptr, kRandStride, fake(3 << 20),
                                       kOutStrideParticipant, kOutStrideClerk, (size_t)participants, kLen, kFirst, 4u};
                ret = sda::for_participant_slices(L, bpp, cap, [&](const sda::GenLayout& S, uint64_t blocks) {
                    const bool same = S.len == L.len && S.secrets_stride == L.secrets_stride && S.rand_stride == L.rand_stride &&
                                      S.out_stride_participant == L.out_stride_participant && S.out_stride_clerk == L.out_stride_clerk &&
                                      S.direct_rows == L.direct_rows;
                    snprintf(buf, sizeof buf, " %" PRIu64 ":%zu:%" PRIu64 ":%" PRIu64 ":%" PRId64 ":%" PRIu64 ":%d", S.first_participant - L.first_participant,
                             S.participants, blocks, (uint64_t)(address(S.secrets) - address(L.secrets)) / 8,
                             S.rand ? (int64_t)((address(S.rand) - address(L.rand)) / 8) : (int64_t)-1,
                             (uint64_t)(address(S.out) - address(L.out)) / 8, same ? 1 : 0);
                    seen += buf;
                    return calls++ == fail_at ? kRecorderError : hipSuccess;
                });
            } else {
                ret = sda::for_participant_ranges(participants, bpp, cap, [&](uint64_t p0, uint64_t count, uint64_t blocks) {
                    snprintf(buf, sizeof buf, " %" PRIu64 ":%" PRIu64 ":%" PRIu64, p0, count, blocks);
                    seen += buf;
                    return calls++ == fail_at ? kRecorderError : hipSuccess;
                });
            }
            printf("%d %lld%s\n", (int)ret, calls, seen.c_str());
        } else if (!strcmp(cmd, "slice")) {
            uint64_t v[13];
            for (int i = 0; i < 13; ++i)
                if (scanf("%" SCNu64, &v[i]) != 1) return 1;
            const sda::GenLayout L{fake((uintptr_t)v[0]), (size_t)v[1], v[2] ? fake((uintptr_t)v[2]) : nullptr, (size_t)v[3], fake((uintptr_t)v[4]),
                                   (size_t)v[5], (size_t)v[6], (size_t)v[7], (size_t)v[8], v[9], (uint32_t)v[10]};
            const sda::GenLayout S = sda::slice(L, v[11], v[12]);
            printf("%" PRIuPTR " %zu %" PRIuPTR " %zu %" PRIuPTR " %zu %zu %zu %zu %" PRIu64 " %u\n", address(S.secrets), S.secrets_stride,
                   address(S.rand), S.rand_stride, address(S.out), S.out_stride_participant, S.out_stride_clerk, S.participants, S.len,
                   S.first_participant, S.direct_rows);
        } else if (!strcmp(cmd, "rounds")) {
            int r, calls = 0, value = 0;
            if (scanf("%d", &r) != 1) return 1;
            const hipError_t ret = sda::with_rounds(r, [&](auto R) {
                ++calls;
                value = decltype(R)::value;
                return hipSuccess;
            });
            printf("%d %d %d %d\n", (int)ret, calls, value, sda::rounds_supported(r) ? 1 : 0);
        } else {
            return 1;                                           // a line that does not parse is an error, not the end
        }
    }
    return feof(stdin) ? 0 : 1;
}

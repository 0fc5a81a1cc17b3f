// Host unit test of sda_amd/csrc/signed_rem.hpp (the header the reference-representative kernels compile): reads lines of
//   <hi> <lo> <q>
// on stdin - x = hi * 2^64 + lo, hi a signed and lo an unsigned 64-bit decimal, q the modulus - and prints trunc_rem128(x, q),
// one decimal per line.  tests/test_signed_rem_cpu.py compares the lines with Python integers, through an -O2 build and
// through one built with -fsanitize=undefined.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include "../../sda_amd/csrc/signed_rem.hpp"

int main() {
    int64_t hi, q;
    uint64_t lo;
    while (scanf("%" SCNd64 " %" SCNu64 " %" SCNd64, &hi, &lo, &q) == 3) {
        const __int128 x = (__int128)hi * ((__int128)1 << 64) + (__int128)lo;
        printf("%" PRId64 "\n", sda::trunc_rem128(x, q));
    }
    return feof(stdin) ? 0 : 1;                              // a line that does not parse is an error, not the end
}

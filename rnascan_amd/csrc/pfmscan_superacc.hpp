// pfmscan_superacc.hpp -- the long accumulator of the library site profiles (include/pfmscan.h, "site profiles of a
// library"): a finite double v > 0 is the integer v / 2^-1074, at most 2098 bits long, and a sum of such integers does
// not depend on the order of its additions.  The accumulator holds that integer in PFMSCAN_SITE_LIMBS 64-bit words of
// weight 2^(32 i); this header cuts one double into the three 32-bit pieces that are added to three consecutive limbs.
// Shared by the device (k_site_sums_lib adds the pieces with 64-bit integer atomics) and the host
// (pfmscan_site_acc_from_doubles), so both decompose with the same code.  Plain 64-bit shifts and masks only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PFMSCAN_HD __host__ __device__
#else
#define PFMSCAN_HD
#endif

namespace pfmscan {

// v finite and > 0 -> the first limb; piece[i] (below 2^32, possibly 0) is added to limb first + i.
//   exponent field E, fraction f:  M = f, b = 0 (E == 0, subnormal), else M = f | 2^52, b = E - 1;  v = M 2^(b - 1074)
//   x = M << (b mod 32) < 2^85, cut at bits 32 and 64.  DBL_MAX: b = 2045, limbs 63, 64, 65.
PFMSCAN_HD inline int site_acc_pieces(double v, uint32_t piece[3])
{
    uint64_t bits;
    __builtin_memcpy(&bits, &v, sizeof(bits));
    const uint64_t f = bits & ((uint64_t(1) << 52) - 1);
    const int E = (int)((bits >> 52) & 0x7ff);
    const uint64_t M = E ? (f | (uint64_t(1) << 52)) : f;
    const int b = E ? E - 1 : 0;
    const int s = b & 31;
    const uint64_t lo = (M & 0xffffffffu) << s;              // below 2^63
    const uint64_t hi = ((M >> 32) << s) + (lo >> 32);       // weight 2^32; below 2^53
    piece[0] = (uint32_t)lo;
    piece[1] = (uint32_t)hi;
    piece[2] = (uint32_t)(hi >> 32);
    return b >> 5;
}

}  // namespace pfmscan

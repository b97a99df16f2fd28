// trr_round.h — the f64 -> f32 conversion of k_trr_unpack (kernels_trr.h), in integers.  Plain C++: the device code
// includes it, and so does tools/trr_round_check.cpp, which holds it against the host's `(float)` cast on the CPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TRR_ROUND_FN __host__ __device__
#else
#define TRR_ROUND_FN
#endif

// The bits of a double -> the bits of the nearest float, ties to even: what `(float)d` gives on the host.  In integers, so
// that the result does not depend on the kernel's floating-point mode (an f32 denormal stays a denormal whatever the
// denormal mode of the conversion instruction).  Beyond FLT_MAX: +-inf; below half the smallest denormal: +-0; a NaN
// stays a (quiet) NaN with the leading bits of its payload.
TRR_ROUND_FN inline uint32_t trr_f64_bits_to_f32_bits(unsigned long long b) {
    const uint32_t sign = (uint32_t)(b >> 63) << 31;
    const uint32_t e = (uint32_t)(b >> 52) & 0x7ffu;
    const unsigned long long m = b & 0xfffffffffffffull;
    if (e == 0x7ffu) return sign | 0x7f800000u | (m ? 0x400000u | (uint32_t)(m >> 29) : 0u);
    const int E = (int)e - 1023 + 127;                       // the float's biased exponent
    if (E >= 255) return sign | 0x7f800000u;
    if (E >= 1) {                                            // a normal float (a carry out of the mantissa steps the exponent,
        uint32_t r = ((uint32_t)E << 23) | (uint32_t)(m >> 29);   //  up to infinity from the largest one)
        const uint32_t rem = (uint32_t)m & 0x1fffffffu;
        if (rem > 0x10000000u || (rem == 0x10000000u && (r & 1u))) r++;
        return sign | r;
    }
    // a denormal float or zero: the 53-bit significand moved right by 29 + (1 - E) bits (a denormal DOUBLE is far below)
    const uint32_t shift = 30u - (uint32_t)E;
    if (e == 0u || shift > 63u) return sign;
    const unsigned long long sig = m | (1ull << 52);
    uint32_t r = (uint32_t)(sig >> shift);
    const unsigned long long rem = sig & ((1ull << shift) - 1ull), half = 1ull << (shift - 1u);
    if (rem > half || (rem == half && (r & 1u))) r++;
    return sign | r;
}

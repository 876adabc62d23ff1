// rt_jitter.hpp — the hash and the level function of the jittered render (rt_render_jitter_dev, include/rt_api.h),
// spelled once for rt_jitter_kernel (rt_sampled.hpp) and for the host's rt_jitter_sample (rt_host.cpp): what the CPU
// suite pins through rt_jitter_sample is the code the kernel runs.  Plain C++ but for the HIP function attributes.
#pragma once

#include <cstdint>

#if defined(__HIP__)
#define RT_JITTER_HD __host__ __device__
#else
#define RT_JITTER_HD
#endif

namespace rtj {

// The 32-bit finaliser of MurmurHash3; uint32 arithmetic, wrapping.  fmix32(0) = 0, fmix32(1) = 0x514e28b7.
RT_JITTER_HD inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// The word of sample q = Jr (S width) + I of the sample frame (its true width: never a tile's or a padded one).
RT_JITTER_HD inline uint32_t jitter_word(uint32_t q, uint32_t seed) { return fmix32(fmix32(q) ^ seed); }

// Level of dimension d in 0 .. 6 (0, 1 sub-pixel x, y; 2, 3 lens x, y; 4, 5 light x, z; 6 time): the top log2 J bits
// of nibble d of the word, in 0 .. J - 1.  jl = log2 J in 0 .. 4; J = 1 gives 0.
RT_JITTER_HD inline int jitter_level(uint32_t w, int d, int jl) { return (int)(((w >> (4 * d)) & 15u) >> (4 - jl)); }

// log2 of a jitter count in {1, 2, 4, 8, 16}, or -1.
inline int jitter_log2_of(int jitter) {
    return jitter == 1 ? 0 : jitter == 2 ? 1 : jitter == 4 ? 2 : jitter == 8 ? 3 : jitter == 16 ? 4 : -1;
}

}  // namespace rtj

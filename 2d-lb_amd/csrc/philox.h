// philox.h -- the random stream of the stochastic collisions: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
// easy as 1, 2, 3", SC'11), a counter-based generator -- four 32-bit words that are a pure function of a 128-bit counter and a 64-bit
// key.  Plain C++ without a HIP type: device code inlines it, a host program compiles it as it is (tests/test_noise_cpu.py does).
//
// The stream.  A handle has a 64-bit seed -- the key is its low and its high word -- and a 64-bit noise counter
// t, the number of noisy collisions since the seed was set.  The four cells x = 4j .. 4j+3 of row y, an aligned lane-of-four
// (kernels_lane4.h), take the words r0 .. r3 of the counter (j, y, t_lo, t_hi), x and y in BOX coordinates (a periodic image: the
// wrapped ones).  A word becomes a uniform by u(r) = float(r >> 9) 2^-23 + 2^-24: exact in float32, inside (0, 1), never 0.  Cells 0, 1
// get R cos(theta), R sin(theta) with R = sqrt(-2 ln u(r0)), theta = 2 pi u(r1); cells 2, 3 the same from r2, r3 (scalar_cell.h:
// ad_normal_pair, the one place where that arithmetic is written).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PHILOX_FN __host__ __device__ inline
#else
#define PHILOX_FN inline
#endif

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;       // the round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;       // the key increments

// r[0..3] = Philox4x32-10 of the counter (c0, c1, c2, c3) under the key (k0, k1)
PHILOX_FN void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&r)[4])
{
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// the words of the lane-of-four that holds box cell (x, y) at noise counter t under `seed`
PHILOX_FN void philox_lane_words(uint64_t seed, int x, int y, uint64_t t, uint32_t (&r)[4])
{
    philox4x32_10((uint32_t)(x >> 2), (uint32_t)y, (uint32_t)t, (uint32_t)(t >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
}

// a word as a uniform in (0, 1): 23 bits, the half-open cells' midpoints
PHILOX_FN float philox_uniform(uint32_t r) { return (float)(r >> 9) * (1.f / 8388608.f) + (1.f / 16777216.f); }

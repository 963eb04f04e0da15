// pve_noise.h -- exploration noise of the device actor (reference main.py:44, :239: every controlled vehicle's commanded
// action is the actor's output + np.random.randn(1) * noise_range, every tick of the training loop).
//
//   a_cmd(env, vehicle, tick) = (double) actor_f32(row) + sigma * z(seed, env_global, vehicle_id, tick)
//
// z is a PURE FUNCTION of its four arguments -- not of the slot, the wave, the launch form, the capacity, the chunking, the
// queue item or the rank a shard runs on -- so the stand-alone actor kernels, the resident closed loops, a batch cut into
// sub-batches and a NumPy restatement (pve_mcc_amd/noise.py) all draw the same number.  Host + device, header only.
//
// Bits: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123).
// Word layout (part of the ABI, include/pve_env.h):
//   counter = (vehicle_id, tick mod 2^32, env_global low word, env_global high word)      key = (seed low word, seed high word)
// One call gives four words; z uses words 0 and 1 (words 2 and 3 are unused).
//
// Gaussian: Box-Muller, z = sqrt(-2 ln u1) cos(2 pi u2) with u = (word + 0.5) 2^-32, SPECIFIED AS EXACT ARITHMETIC: IEEE
// binary64 + - * / and sqrt (each rounded once, no contraction into fused multiply-adds), integer operations and exact
// scalings by powers of two, in the evaluation order written below; no libm / ocml transcendental.  A noisy action moves a
// vehicle, positions decide ranks and collisions: this is the project's rule for everything that feeds discrete decisions
// (SURVEY.md App. G).  Every implementation that follows the order below is BIT-EQUAL to this one.
//
//   radius  m = 2 w0 + 1 (odd, < 2^33), u1 = m 2^-33.  (double)m = f 2^e with f in [1/2, 1) (exponent / mantissa bits of the
//           exactly converted integer); f < fl(sqrt(1/2)): f = 2 f, e = e - 1.  s = (f - 1) / (f + 1), |s| <= 0.1716,
//           ln f = 2 s L(s^2), L = sum_{j=0..8} s^2j / (2j + 1) by Horner (truncation 2 s^19 / 19 <= 3e-16);
//           -2 ln u1 = (double)(2 (33 - e)) fl(ln 2) - 4 (s L);   radius = sqrt of that  (0 < radius <= 6.764)
//   angle   n = 2 w1 + 1, 4 u2 = n 2^-31: quadrant q = n >> 31, k = n mod 2^31 (odd); k > 2^30: k = 2^31 - k and sine and cosine
//           change places.  x = (double)k (fl(pi / 2) 2^-31) in (0, pi / 4); Taylor polynomial in x^2 by Horner, 8 terms:
//           cos x = sum (-1)^j x^2j / (2j)!,  sin x = x sum (-1)^j x^2j / (2j + 1)!  (truncation <= 1e-15), the coefficients
//           being the correctly rounded quotients 1 / n!;  cos(2 pi u2) = +cos, -sin, -cos, +sin of the quadrant's angle.
//   z = radius * (that value).
// Against the same transform with libm's log / cos in float64: |z - z_libm| < 1e-14 over 2^20 draws (tests/test_action_noise.py; the
// requirement is 1e-6).  Cost per draw: ten Philox rounds (40 32-bit multiplies), ~50 float64 operations, one division, one
// square root.
#pragma once
#include <stdint.h>
#include <string.h>

#include "pve_types.h"

namespace pve {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox4x32-10: c[4] <- ten rounds of (counter c, key k0 k1)
PVE_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c[0], p1 = (uint64_t)PHILOX_M1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
}

PVE_HD uint64_t noise_bits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
PVE_HD double noise_from_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }

// the standard normal deviate of two 32-bit words (the arithmetic specified at the top of this file)
PVE_HD double noise_gauss(uint32_t w0, uint32_t w1)
{
#if defined(__clang__)
#pragma clang fp contract(off)                   // (whatever the translation unit's default: every operation rounds on its own)
#endif
    // ---- radius
    const uint64_t m = 2ull * w0 + 1ull;
    const uint64_t mb = noise_bits((double)(int64_t)m);                     // (exact: m < 2^53)
    int e = (int)(mb >> 52) - 1022;
    double f = noise_from_bits((mb & 0x000FFFFFFFFFFFFFull) | 0x3FE0000000000000ull);
    if (f < 0.70710678118654757) { f = f * 2.0; e -= 1; }
    const double s = (f - 1.0) / (f + 1.0), s2 = s * s;
    double L = 1.0 / 17.0;
    L = L * s2 + 1.0 / 15.0; L = L * s2 + 1.0 / 13.0; L = L * s2 + 1.0 / 11.0; L = L * s2 + 1.0 / 9.0;
    L = L * s2 + 1.0 / 7.0; L = L * s2 + 1.0 / 5.0; L = L * s2 + 1.0 / 3.0; L = L * s2 + 1.0;
    const double radius = __builtin_sqrt((double)(2 * (33 - e)) * 0.69314718055994529 - 4.0 * (s * L));
    // ---- angle
    const uint64_t n = 2ull * w1 + 1ull;
    const int q = (int)(n >> 31);
    int k = (int)(n & 0x7FFFFFFFull);
    const bool swap = k > (1 << 30);
    if (swap) k = (int)(0x80000000u - (uint32_t)k);
    const double x = (double)k * (1.5707963267948966 / 2147483648.0), x2 = x * x;
    const bool use_sin = ((q & 1) != 0) != swap;
    // (1 / (2j)! and 1 / (2j + 1)!, j = 7 .. 0)
    double P = use_sin ? -1.0 / 1307674368000.0 : -1.0 / 87178291200.0;
    P = P * x2 + (use_sin ? 1.0 / 6227020800.0 : 1.0 / 479001600.0);
    P = P * x2 + (use_sin ? -1.0 / 39916800.0 : -1.0 / 3628800.0);
    P = P * x2 + (use_sin ? 1.0 / 362880.0 : 1.0 / 40320.0);
    P = P * x2 + (use_sin ? -1.0 / 5040.0 : -1.0 / 720.0);
    P = P * x2 + (use_sin ? 1.0 / 120.0 : 1.0 / 24.0);
    P = P * x2 + (use_sin ? -1.0 / 6.0 : -1.0 / 2.0);
    P = P * x2 + 1.0;
    double cs = use_sin ? x * P : P;
    if (q == 1 || q == 2) cs = -cs;
    return radius * cs;
}

// z(seed, env_global, vehicle_id, tick): the word layout documented in include/pve_env.h
PVE_HD double action_noise_z(uint64_t seed, int64_t env_global, int32_t vehicle_id, uint32_t tick)
{
    uint32_t c[4] = {(uint32_t)vehicle_id, tick, (uint32_t)(uint64_t)env_global, (uint32_t)((uint64_t)env_global >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return noise_gauss(c[0], c[1]);
}

// the commanded action of a controlled vehicle: float64 sum of the actor's float32 output and sigma z
PVE_HD double action_with_noise(double a, const ActionNoise &nz, int64_t env_global, int32_t vehicle_id, uint32_t tick)
{
    return a + nz.sigma * action_noise_z(nz.seed, env_global, vehicle_id, tick);
}

}  // namespace pve

// pve_arrivals.h -- arrival streams generated where they are consumed (reference main.py:228-229 / :388-389: every episode
// loads its `arvTimeNewVeh` matrix with scipy.io.loadmat; ref :381, :390: the 8-lane layout draws random.randint(0, 1) per
// arriving vehicle).  pve_generate_arrivals writes the float64 block arrivals[n_envs][rows][lane_num] that pve_set_arrivals
// takes with env_stride_rows = rows, and for lane_num = 8 the int32 block intentions[n_envs][rows][8] of pve_set_intentions.
// Host + device, header only.  THIS FILE IS THE DEFINITION: the kernels below, the g++ build of arrivals_generate_host
// (tests/arrivals_host) and the NumPy restatement (pve_mcc_amd/arrivals.py: device_arrivals / device_intentions) are held to
// it bit for bit.  Arrival times decide spawns, so they fall under the project's rule for everything that feeds discrete
// decisions: exact arithmetic in a stated order.
//
// Draw.  Row r < rows - 1, lane l, env_global = env index in the handle + env_offset:
//   w = output word (r & 3) of Philox4x32-10 (pve_noise.h) with
//   counter = ((r >> 2) | (l << 28), epoch, env_global low word, env_global high word)
//   key     = (seed low word ^ 0x41525256, seed high word ^ 0x54494D45)                                  ("ARRV", "TIME")
// One Philox call serves four consecutive rows (rows < 2^28 + 1 and l < 16, so the two fields of counter word 0 never meet).
// The key tweak keeps these draws apart from the exploration noise (raw seed) and from the prioritised replay's draw
// (^ 0x5052494F / 0x52414E4B) under one user seed.
//
// Exponential deviate.  x = -ln u, u = (2 w + 1) 2^-33, evaluated as the radius of noise_gauss evaluates its logarithm:
//   m = 2 w + 1 (odd, < 2^33).  (double)m = f 2^e with f in [1/2, 1) from the exponent / mantissa bits of the exactly converted
//   integer; f < fl(sqrt(1/2)): f = 2 f, e = e - 1.  s = (f - 1) / (f + 1), L = sum_{j=0..8} s^2j / (2j + 1) by Horner,
//   x = (double)(33 - e) * fl(ln 2) - 2.0 * (s * L)
// in binary64 + - * / only, each rounded once, no contraction, no libm / ocml call.  x lies in [1.16e-10, 22.874] and is never 0
// (w = 0xFFFFFFFF: u = 1 - 2^-33; w = 0: u = 2^-33).  Against -log(u) of libm in float64: 1.13e-15 relative over 2^20 words
// (tests/test_arrivals_device.py; the bar is 1e-12).
//
// Gap.  d = mean * x;  if (d < min_gap) d = min_gap;   mean = 3600 / rate seconds, one value or one per environment
// (the clipped-exponential shape of BASELINE.md §3 that arrivals.synthetic_arrivals has; min_gap = 1.0 there).
//
// Cumulative time.  t[0] = d[0], t[r] = t[r-1] + d[r]: float64 additions in ascending r, one chain per (env, lane).  THIS ORDER IS
// THE DEFINITION; a parallel prefix scan adds in another order, gives other bits and is therefore not an implementation of it.
//
// Padding.  Row rows - 1 is +inf in every lane (an exhausted lane stops spawning).
//
// Consequences:
//   * a chain is a pure function of (seed, epoch, env_global, lane, r) and of (mean, min_gap) -- not of n_envs, rows, the
//     launch shape or block_threads;
//   * a stream of R1 rows is the prefix (rows 0 .. R1 - 2) of a stream of R2 > R1 rows;
//   * a batch cut into pieces with the matching env_offset generates what the uncut batch generates;
//   * with min_gap = 1.0, t[r] >= r + 1 EXACTLY (every gap >= 1, rounding is monotone and the integers up to 2^53 are exact):
//     rows - 1 seconds of run are covered whatever the draws.
//
// Intentions (lane_num = 8, every row r < rows): entry (e, r, l) = bit (r & 31) of output word ((r >> 5) & 3) of Philox4x32-10 with
//   counter = ((r >> 7) | (l << 28), epoch, env_global low word, env_global high word)
//   key     = (seed low word ^ 0x494E5445, seed high word ^ 0x4E54494F)                                  ("INTE", "NTIO")
// One Philox call gives 128 rows of one (env, lane).
//
// Coverage (optional): covered[e] = min over lanes of t[e][rows - 2][l], how far the stream of environment e is guaranteed to
// reach (a minimum is exact: no order to state).
#pragma once
#include <stdint.h>

#include "pve_noise.h"
#include "pve_types.h"

namespace pve {

constexpr uint32_t ARR_KEY0 = 0x41525256u, ARR_KEY1 = 0x54494D45u, ARR_INT_KEY0 = 0x494E5445u, ARR_INT_KEY1 = 0x4E54494Fu;
constexpr int ARR_MAX_ROWS = 1 << 28;
// (launch shape only, never results; -DPVE_ARR_GROUP / -DPVE_ARR_TILE build the variants tools/bench_arrivals.py compares)
#ifndef PVE_ARR_GROUP
#define PVE_ARR_GROUP 4
#endif
#ifndef PVE_ARR_TILE
#define PVE_ARR_TILE 64
#endif
constexpr int ARR_GROUP = PVE_ARR_GROUP;         // environments per workgroup of k_gen_arrivals
constexpr int ARR_TILE = PVE_ARR_TILE;           // rows per LDS tile (a multiple of 4: a Philox quad never straddles two tiles)
constexpr int ARR_MAX_LANES = 12;
static_assert(ARR_TILE % 4 == 0 && ARR_TILE >= 4 && ARR_GROUP >= 1 && ARR_GROUP * ARR_MAX_LANES <= 64 &&
              ARR_GROUP * ARR_TILE * ARR_MAX_LANES * 8 <= 60 * 1024,
              "a Philox quad per tile item; the chains of a group fit the smallest workgroup (64 threads); the tile fits static LDS");
constexpr int ARR_INT_ROWS = 128;                // rows of one (env, lane) per Philox call of the intentions

struct ArrivalArgs {
    uint64_t seed;
    long long env_offset;
    uint32_t epoch;
    int rows, n_envs, lane_num;
    double mean;                                 // used when mean_env is null
    const double *mean_env;                      // [n_envs] or null
    double min_gap;
    double *arrivals;                            // [n_envs][rows][lane_num]
    int32_t *intentions;                         // [n_envs][rows][8] or null
    double *covered;                             // [n_envs] or null
};

// x = -ln((2 w + 1) 2^-33): the arithmetic specified at the top of this file (the radius of noise_gauss, restated)
PVE_HD double arrival_exp(uint32_t w)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint64_t m = 2ull * w + 1ull;
    const uint64_t mb = noise_bits((double)(int64_t)m);                     // (exact: m < 2^53)
    int e = (int)(mb >> 52) - 1022;
    double f = noise_from_bits((mb & 0x000FFFFFFFFFFFFFull) | 0x3FE0000000000000ull);
    if (f < 0.70710678118654757) { f = f * 2.0; e -= 1; }
    const double s = (f - 1.0) / (f + 1.0), s2 = s * s;
    double L = 1.0 / 17.0;
    L = L * s2 + 1.0 / 15.0; L = L * s2 + 1.0 / 13.0; L = L * s2 + 1.0 / 11.0; L = L * s2 + 1.0 / 9.0;
    L = L * s2 + 1.0 / 7.0; L = L * s2 + 1.0 / 5.0; L = L * s2 + 1.0 / 3.0; L = L * s2 + 1.0;
    return (double)(33 - e) * 0.69314718055994529 - 2.0 * (s * L);
}

// the four words of rows 4 quad .. 4 quad + 3 of chain (env_global, lane)
PVE_HD void arrival_words(uint64_t seed, uint32_t epoch, long long env_global, int lane, uint32_t quad, uint32_t (&c)[4])
{
    c[0] = quad | ((uint32_t)lane << 28); c[1] = epoch;
    c[2] = (uint32_t)(uint64_t)env_global; c[3] = (uint32_t)((uint64_t)env_global >> 32);
    philox4x32_10(c, (uint32_t)seed ^ ARR_KEY0, (uint32_t)(seed >> 32) ^ ARR_KEY1);
}

PVE_HD double arrival_gap(uint32_t w, double mean, double min_gap)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double d = mean * arrival_exp(w);
    if (d < min_gap) d = min_gap;
    return d;
}

// the four words that hold rows 128 chunk .. 128 chunk + 127 of the intentions of (env_global, lane)
PVE_HD void intention_words(uint64_t seed, uint32_t epoch, long long env_global, int lane, uint32_t chunk, uint32_t (&c)[4])
{
    c[0] = chunk | ((uint32_t)lane << 28); c[1] = epoch;
    c[2] = (uint32_t)(uint64_t)env_global; c[3] = (uint32_t)((uint64_t)env_global >> 32);
    philox4x32_10(c, (uint32_t)seed ^ ARR_INT_KEY0, (uint32_t)(seed >> 32) ^ ARR_INT_KEY1);
}

PVE_HD int32_t intention_bit(const uint32_t (&c)[4], int r) { return (int32_t)((c[(r >> 5) & 3] >> (r & 31)) & 1u); }

PVE_HD double arrival_inf() { return noise_from_bits(0x7FF0000000000000ull); }

// The definition as a plain loop over HOST memory (every pointer of A is a host pointer here): what tests/arrivals_host builds.
inline void arrivals_generate_host(const ArrivalArgs &A)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t ln = (size_t)A.lane_num, rows = (size_t)A.rows;
    for (int e = 0; e < A.n_envs; e++) {
        const long long eg = (long long)e + A.env_offset;
        const double mean = A.mean_env ? A.mean_env[e] : A.mean;
        double *out = A.arrivals + (size_t)e * rows * ln;
        double cov = arrival_inf();
        for (int l = 0; l < A.lane_num; l++) {
            double t = 0.0;
            for (int r = 0; r < A.rows - 1; r++) {
                uint32_t c[4];
                arrival_words(A.seed, A.epoch, eg, l, (uint32_t)r >> 2, c);
                const double d = arrival_gap(c[r & 3], mean, A.min_gap);
                t = r == 0 ? d : t + d;
                out[(size_t)r * ln + l] = t;
            }
            out[(rows - 1) * ln + l] = arrival_inf();
            if (t < cov) cov = t;
        }
        if (A.covered) A.covered[e] = cov;
        if (A.intentions)
            for (int l = 0; l < A.lane_num; l++)
                for (int r = 0; r < A.rows; r++) {
                    uint32_t c[4];
                    intention_words(A.seed, A.epoch, eg, l, (uint32_t)r >> 7, c);
                    A.intentions[((size_t)e * rows + (size_t)r) * ln + l] = intention_bit(c, r);
                }
    }
}

#if defined(__HIPCC__)

// One workgroup per group of ARR_GROUP environments, tile after tile of ARR_TILE rows down the stream:
//   A. the tile's gaps, all threads: one item = one Philox quad of one chain (call, four logarithms, four multiplies, the clip)
//      into LDS, lanes fastest, so that consecutive threads write consecutive doubles;
//   B. the chains, ARR_GROUP x lane_num threads: the dependent additions over the tile in place, ascending r, the running time
//      in a register from tile to tile (the loads of a tile do not depend on the chain, only the additions do);
//   C. the store, all threads: each environment's tile is ONE contiguous run of tile rows x lane_num x 8 bytes of the output
//      (lane_num is even and the buffer 16-byte aligned: every run starts and ends on 16 bytes), written as 16-byte pieces.
// The padding row is written as a gap of +inf by phase A and skipped by phase B.  covered[] leaves from the chains' registers
// through LDS after the last tile.  Plain stores, no atomics, no flag between workgroups; every loop is bounded by the arguments.
__global__ __launch_bounds__(1024) void k_gen_arrivals(const ArrivalArgs A)
{
    __shared__ __attribute__((aligned(16))) double tile_s[ARR_GROUP * ARR_TILE * ARR_MAX_LANES];
    __shared__ double mean_s[ARR_GROUP];
    __shared__ double last_s[ARR_GROUP * ARR_MAX_LANES];
    const int ln = A.lane_num, tid = threadIdx.x, nthr = blockDim.x;
    const long long e0 = (long long)blockIdx.x * ARR_GROUP;
    const int ne = A.n_envs - e0 < ARR_GROUP ? (int)(A.n_envs - e0) : ARR_GROUP;        // environments of this group (>= 1)
    const int env_doubles = ARR_TILE * ln;                                              // one environment's tile in LDS
    if (tid < ne) mean_s[tid] = A.mean_env ? A.mean_env[e0 + tid] : A.mean;
    __syncthreads();
    const int chain_e = tid / ln, chain_l = tid - chain_e * ln;
    const bool is_chain = tid < ne * ln;
    double t = 0.0;
    const int last = A.rows - 1;                                                        // the padding row
    const int quads = ARR_TILE / 4, items = ne * quads * ln;
    for (int r0 = 0; r0 < A.rows; r0 += ARR_TILE) {
        const int tr = A.rows - r0 < ARR_TILE ? A.rows - r0 : ARR_TILE;                 // rows of this tile
        // ---- A
        for (int i = tid; i < items; i += nthr) {
            const int l = i % ln, eq = i / ln, q = eq % quads, e = eq / quads;
            const int r = r0 + 4 * q;
            if (r > last) continue;
            double *dst = tile_s + e * env_doubles + 4 * q * ln + l;
            if (r == last) { dst[0] = arrival_inf(); continue; }
            uint32_t c[4];
            arrival_words(A.seed, A.epoch, e0 + e + A.env_offset, l, (uint32_t)r >> 2, c);
            const double mean = mean_s[e];
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (r + k <= last) dst[k * ln] = r + k == last ? arrival_inf() : arrival_gap(c[k], mean, A.min_gap);
        }
        __syncthreads();
        // ---- B
        if (is_chain) {
            double *p = tile_s + chain_e * env_doubles + chain_l;
            const int n = last - r0 < tr ? last - r0 : tr;                               // rows of this tile before the padding row
            for (int k = 0; k < n; k++) {
                const double d = p[k * ln];
                t = (r0 + k == 0) ? d : t + d;
                p[k * ln] = t;
            }
        }
        __syncthreads();
        // ---- C
        const int run16 = tr * ln / 2;                                                  // 16-byte pieces of one environment's run
        for (int i = tid; i < ne * run16; i += nthr) {
            const int e = i / run16, k = i - e * run16;
            double2 *dst = (double2 *)(A.arrivals + ((size_t)(e0 + e) * (size_t)A.rows + (size_t)r0) * (size_t)ln);
            dst[k] = ((const double2 *)(tile_s + e * env_doubles))[k];
        }
        __syncthreads();
    }
    if (A.covered) {
        if (is_chain) last_s[tid] = t;
        __syncthreads();
        if (tid < ne) {
            double m = last_s[tid * ln];
            for (int l = 1; l < ln; l++) m = last_s[tid * ln + l] < m ? last_s[tid * ln + l] : m;
            A.covered[e0 + tid] = m;
        }
    }
}

// The intentions, elementwise.  One item = 128 rows of one environment = 4096 contiguous bytes of the output: eight threads
// draw the eight lanes' four words into LDS, then every thread writes 16-byte pieces (four lanes of one row).
__global__ __launch_bounds__(1024) void k_gen_intentions(const ArrivalArgs A)
{
    __shared__ uint32_t word_s[8][4];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long long chunks = ((long long)A.rows + ARR_INT_ROWS - 1) / ARR_INT_ROWS, n_items = chunks * A.n_envs;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const long long e = item / chunks;
        const int chunk = (int)(item - e * chunks), r0 = chunk * ARR_INT_ROWS;
        if (tid < 8) {
            uint32_t c[4];
            intention_words(A.seed, A.epoch, e + A.env_offset, tid, (uint32_t)chunk, c);
#pragma unroll
            for (int k = 0; k < 4; k++) word_s[tid][k] = c[k];
        }
        __syncthreads();
        const int tr = A.rows - r0 < ARR_INT_ROWS ? A.rows - r0 : ARR_INT_ROWS;
        int4 *dst = (int4 *)(A.intentions + ((size_t)e * (size_t)A.rows + (size_t)r0) * 8);
        for (int i = tid; i < 2 * tr; i += nthr) {
            const int r = i >> 1, l0 = (i & 1) * 4, w = (r >> 5) & 3, b = r & 31;
            dst[i] = make_int4((int)((word_s[l0][w] >> b) & 1u), (int)((word_s[l0 + 1][w] >> b) & 1u),
                               (int)((word_s[l0 + 2][w] >> b) & 1u), (int)((word_s[l0 + 3][w] >> b) & 1u));
        }
        __syncthreads();
    }
}

#endif  // __HIPCC__

}  // namespace pve

// pve_replay.h -- the uniform replay memory on the device (reference replay_buffer.py:45-53 `add`, :20-23 `getBatch` with
// rand_s = True; main.py:263 `agent1_memory_seq.add(...)`, main.py:50-77 `agent_memory.getBatch(batch_size)` and the split into
// obs_batch / the 7 actions / target): a ring of the 36-float records pve_nstep_gather writes, and minibatch draws from it
// without replacement.  No floating-point arithmetic anywhere: records move as 16-byte pieces, every check is bit for bit.
//
// RING.  `capacity` records of 36 float32 (144 B = 9 pieces of 16 B) in caller-owned device memory, and a device-resident
// state block of REPLAY_STATE_WORDS int64:
//   state[REPLAY_WRITTEN]  adds ever made (the reference's count())
//   state[REPLAY_DRAWS]    minibatches ever drawn
//   state[REPLAY_STATUS]   live records seen by the latest sample call (below the batch size: that call drew nothing)
// Record number w (0-based over all adds) lives in slot w mod capacity.  Live records are the last L = min(written, capacity);
// age index a in [0, L) names record written - L + a (0 = the oldest, the left end of the reference's deque).
// An append of n records writes records skip .. n - 1 of its input, skip = max(n - capacity, 0): of a chunk longer than the ring
// only the last `capacity` records survive, so no two records of one launch target the same slot.
//
// DRAW.  Minibatch number d (draws, draws + 1, ..) takes the records with age indices perm(seed, d, L)(j), j = 0 .. batch - 1.
// perm(seed, d, N) is a bijection of [0, N) and a pure function of its arguments -- not of the launch geometry, the batch size or
// the number of minibatches one call draws:
//   b = bit length of N - 1, at least 2, rounded up to even; h = b / 2
//   Feistel network of REPLAY_ROUNDS = 8 rounds over (L, R) = the high / low h bits of x:  (L, R) <- (R, L ^ F_r(R)),
//   F_r(R) = word 0 of Philox4x32-10(counter = (R, r, d low word, d high word),
//                                    key = (seed low word ^ REPLAY_TAG0, seed high word ^ REPLAY_TAG1)), masked to h bits
//   cycle walk: x = j, then x <- Feistel(x) until x < N.  The domain 2^b is below 4 N, so the expected walk is under 4 steps; it
//   ends because the cycle through a value below N returns to one.
// The tag keeps the draw's Philox inputs apart from the action noise's (pve_noise.h: same generator, key = the bare seed) when both
// are given the same seed.  Quality at N < 16 is not claimed (2-bit halves); bijectivity is.  Host + device, header only;
// pve_mcc_amd/replay.py restates it in NumPy.
#pragma once
#include <stdint.h>

#include "pve_noise.h"
#include "pve_types.h"

namespace pve {

constexpr int REPLAY_REC = 36;                               // float32 per record (NSTEP_REC): s0 row [28], actions [7], target [1]
constexpr int REPLAY_PIECES = REPLAY_REC / 4;                // 16-byte pieces per record
constexpr int REPLAY_ROUNDS = 8;
constexpr uint32_t REPLAY_TAG0 = 0x5245504Cu, REPLAY_TAG1 = 0x41594D45u;      // "REPL", "AYME"
constexpr int REPLAY_WRITTEN = 0, REPLAY_DRAWS = 1, REPLAY_STATUS = 2, REPLAY_STATE_WORDS = 4;

// h: bits of one Feistel half for a domain of N values
PVE_HD int replay_half_bits(uint32_t N)
{
    int b = 0;
    for (uint32_t v = N - 1u; v; v >>= 1) b++;
    if (b < 2) b = 2;
    return (b + 1) >> 1;
}

PVE_HD uint32_t replay_feistel(uint64_t seed, uint64_t d, int h, uint32_t x)
{
    const uint32_t mask = (1u << h) - 1u;
    uint32_t L = x >> h, R = x & mask;
    for (int r = 0; r < REPLAY_ROUNDS; r++) {
        uint32_t c[4] = {R, (uint32_t)r, (uint32_t)d, (uint32_t)(d >> 32)};
        philox4x32_10(c, (uint32_t)seed ^ REPLAY_TAG0, (uint32_t)(seed >> 32) ^ REPLAY_TAG1);
        const uint32_t nr = L ^ (c[0] & mask);
        L = R; R = nr;
    }
    return (L << h) | R;
}

// perm(seed, d, N)(j), 0 <= j < N <= 2^31 - 1
PVE_HD uint32_t replay_perm(uint64_t seed, uint64_t d, uint32_t N, uint32_t j)
{
    const int h = replay_half_bits(N);
    uint32_t x = j;
    do x = replay_feistel(seed, d, h, x); while (x >= N);
    return x;
}

PVE_HD long long replay_live(long long written, long long capacity) { return written < capacity ? written : capacity; }

// What one append does: n records accepted (n = n_max, or min(total, n_max) with a device-side total), the first `skip` of them
// dropped, input record skip + q (q = 0 .. n - skip - 1) stored in slot replay_append_slot(plan, capacity, q).
struct ReplayPlan {
    long long n, skip, start;                  // start = (written + skip) mod capacity
};
PVE_HD ReplayPlan replay_append_plan(long long written, bool has_total, long long total, long long n_max, long long capacity)
{
    ReplayPlan P;
    P.n = n_max;
    if (has_total) { const long long t = total < 0 ? 0 : total; P.n = t < n_max ? t : n_max; }
    P.skip = P.n > capacity ? P.n - capacity : 0;
    P.start = (written + P.skip) % capacity;
    return P;
}
PVE_HD long long replay_append_slot(const ReplayPlan &P, long long capacity, long long q)
{
    const long long s = P.start + q;           // (q < capacity: one conditional subtraction is the whole modulo)
    return s >= capacity ? s - capacity : s;
}

struct ReplayArgs {
    long long capacity;
    float *store;                              // [capacity][36]
    long long *state;                          // [REPLAY_STATE_WORDS]
    uint64_t seed;
};

// LDS of k_replay_sample per workgroup of `block` threads
PVE_HD size_t replay_sample_lds(int block) { return (size_t)block * (8 * sizeof(float) + sizeof(int)); }

static_assert(REPLAY_REC % 4 == 0 && OBSW % 4 == 0 && REPLAY_REC == OBSW + (NNB + 1) + 1 && REPLAY_REC - OBSW == 8,
              "a record is the s0 row, NNB + 1 actions and the target: 7 + 2 pieces of 16 bytes, which k_replay_sample splits");
#if defined(__HIPCC__)

// One thread per 16-byte piece, grid-stride: piece p of the accepted input = (record skip + p / 9, piece p mod 9); consecutive
// lanes read consecutive 16 bytes of the input and write consecutive 16 bytes of the ring (but for the one wrap).  Reads the
// state, never writes it: k_replay_append_commit does, behind this launch on the same stream.
__global__ __launch_bounds__(1024) void k_replay_append(const ReplayArgs A, const float *__restrict__ records,
                                                        const long long *__restrict__ total_dev, const long long n_max)
{
    const ReplayPlan P = replay_append_plan(A.state[REPLAY_WRITTEN], total_dev != nullptr, total_dev ? *total_dev : 0, n_max, A.capacity);
    const long long n_pieces = (P.n - P.skip) * REPLAY_PIECES, stride = (long long)gridDim.x * blockDim.x;
    const float4 *src = (const float4 *)records + P.skip * REPLAY_PIECES;
    float4 *dst = (float4 *)A.store;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n_pieces; p += stride) {
        const long long q = p / REPLAY_PIECES;
        const int k = (int)(p - q * REPLAY_PIECES);
        dst[replay_append_slot(P, A.capacity, q) * REPLAY_PIECES + k] = src[p];
    }
}

__global__ void k_replay_append_commit(const ReplayArgs A, const long long *__restrict__ total_dev, const long long n_max)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long written = A.state[REPLAY_WRITTEN];
    const ReplayPlan P = replay_append_plan(written, total_dev != nullptr, total_dev ? *total_dev : 0, n_max, A.capacity);
    A.state[REPLAY_WRITTEN] = written + P.n;
}

// One thread per drawn record g = minibatch * batch + j (the outputs are contiguous over g).  A wave of 64 draws:
//   1. every lane evaluates its own perm and stores its record number (seq, 8 B per lane, coalesced) and its slot (LDS);
//   2. the wave's 64 x 9 pieces are loaded piece after piece, lane after lane: 9 consecutive lanes read the 144 contiguous
//      bytes of one record.  Pieces 0-6 are the s0 row and go straight out as 16-byte stores (the rows of consecutive g are
//      contiguous); pieces 7-8 (7 actions + target) are staged in LDS;
//   3. act7 (28 B per record) and target (4 B) leave the LDS stage lane after lane: consecutive lanes, consecutive floats.
// With fewer live records than `batch` nothing is drawn: seq = -1, zeros.  Reads the state, never writes it (k_replay_sample_commit).
__global__ __launch_bounds__(1024) void k_replay_sample(const ReplayArgs A, const long long batch, const long long n_total,
                                                        float *__restrict__ rows, float *__restrict__ act7, float *__restrict__ target,
                                                        long long *__restrict__ seq)
{
    // dynamic LDS, 36 B per thread (replay_sample_lds): the staged 7 actions + target of every draw, then its slot
    extern __shared__ __attribute__((aligned(16))) float tail_s[];
    int *slot_s = (int *)(tail_s + (size_t)blockDim.x * 8);
    const long long written = A.state[REPLAY_WRITTEN], draws = A.state[REPLAY_DRAWS];
    const long long L = replay_live(written, A.capacity);
    const bool empty = L < batch;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x, g0 = g - lane;      // (g0: a multiple of 64)
    long long w = -1;
    if (g < n_total && !empty) {
        const long long m = g / batch, j = g - m * batch;
        w = written - L + (long long)replay_perm(A.seed, (uint64_t)(draws + m), (uint32_t)L, (uint32_t)j);
    }
    if (g < n_total) seq[g] = w;
    slot_s[threadIdx.x] = w < 0 ? -1 : (int)(w % A.capacity);         // (capacity < 2^31)
    __syncthreads();
    const long long left = n_total - g0;
    const int count = left >= 64 ? 64 : (left > 0 ? (int)left : 0);           // draws of this wave
    const float4 *store = (const float4 *)A.store;
    float4 *rows4 = (float4 *)rows + g0 * (OBSW / 4);
    float *tail = tail_s + wave * (64 * 8);
#pragma unroll
    for (int it = 0; it < REPLAY_PIECES; it++) {
        const int p = it * 64 + lane, rec = p / REPLAY_PIECES, k = p - rec * REPLAY_PIECES;
        if (rec < count) {
            const long long s = slot_s[wave * 64 + rec];                  // (widened: s * 9 pieces may pass 2^31)
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s >= 0) v = store[s * REPLAY_PIECES + k];
            if (k < OBSW / 4) rows4[rec * (OBSW / 4) + k] = v;
            else ((float4 *)tail)[rec * 2 + (k - OBSW / 4)] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 7; it++) {
        const int f = it * 64 + lane, rec = f / 7, c = f - rec * 7;
        if (rec < count) act7[g0 * 7 + f] = tail[rec * 8 + c];
    }
    if (lane < count) target[g0 + lane] = tail[lane * 8 + 7];
}

__global__ void k_replay_sample_commit(const ReplayArgs A, const long long batch, const long long n_batches)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long L = replay_live(A.state[REPLAY_WRITTEN], A.capacity);
    A.state[REPLAY_STATUS] = L;
    if (L >= batch) A.state[REPLAY_DRAWS] += n_batches;
}

#endif  // __HIPCC__

}  // namespace pve

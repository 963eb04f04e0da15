// pve_prio.h -- the rank-based prioritised replay memory on the device (reference rank_based.py `Experience`, which
// replay_buffer.py:13-18 builds in every run and `getBatch` draws from with rand_s = False; main.py:76-79 td_error /
// update_priority): a priority store beside the ring of pve_replay.h, the ranking of the live records, the stratified draw
// and the update.  Every integer part is bit-exact; the only floating-point arithmetic is one subtraction (exact IEEE) in the
// update and the importance weight.
//
// CAPACITY.  rank_based.py:82-99 cycles its index over 1 .. size: reference e_id = slot + 1, slot = w mod capacity with
// capacity = size (the uniform memory's deque holds size - 1).  Ring, state block and append are pve_replay.h's, unchanged.
//
// PRIORITY STORE.  prio uint32 [capacity] = the bit pattern of a non-negative float32, pseq int64 [capacity].  The priority of
// slot s is VALID only if pseq[s] equals the record number that lives in s now; otherwise the record is NEW and its key is the
// bits of +inf (rank_based.py:114-117 stores a new record with the heap's maximum) -- which is why the append needs no change.
// pstate int64 [PRIO_STATE_WORDS]: pdraws (minibatches ever drawn), the live count and the partition index of the latest
// ranking, the ids ignored by the latest update.
//
// RANKING.  order[r], r = 0 .. L - 1, is the age index of the record of rank r + 1 among the L = min(written, capacity) live
// records, sorted descending by (priority bits, record number): a total order.  NEW records come first, newest first.  For
// pairwise distinct priorities this is the reference's priority_to_experience(1 .. L) after rebalance() (binary_heap.py:194-221);
// the reference's order among ties follows its heap layout and is not reproduced.  The kernels sort the keys ~bits ascending with
// a stable least-significant-digit radix sort whose input is laid out newest first, which yields exactly that order.
//
// STRATA.  The tables are the caller's (rank_based.py:40-80 restated on the host): part_from[k], k = 0 .. 31, the smallest L
// with floor(1.0 * L / size * 32) >= k + 1; the partition index of L is the number of thresholds <= L (rank_based.py:159), and
// partition p = 1 .. 32 uses row p - 1 of ends int32 [32][batch + 1] (strata_ends, ends[0] = 0, ends[batch] = n_p).
//
// DRAW.  Minibatch d (pdraws, pdraws + 1, ..), stratum j = 0 .. batch - 1 (rank_based.py:166-173, with the swapped randint of its
// degenerate strata):  lo = min(ends[j] + 1, ends[j + 1]), hi = max(ends[j] + 1, ends[j + 1]),
//   rank = lo + mulhi32(u, hi - lo + 1),  u = word 0 of Philox4x32-10(counter = (j, 0, d low word, d high word),
//                                                                   key = (seed low word ^ PRIO_TAG0, seed high word ^ PRIO_TAG1))
// clamped to 1 .. L (never active with tables built as above: it keeps a foreign table inside `order`).  The age index is
// order[rank - 1], the record number written - L + age.  The reference's Mersenne-Twister draw is not reproduced.
//
// WEIGHT.  weight = (rank / rank_max)^(alpha beta) in float32, rank_max the minibatch's largest rank: rank_based.py:176-182 with
// the normaliser and partition_max cancelled.
//
// UPDATE (main.py:76-79).  p = |q - target| in float32 (|q| without a target), NaN stored as +inf.  An id outside
// [written - L, written) is ignored and counted (the reference would write onto the slot's new occupant).  Of an id named
// several times the largest p wins; the old value is replaced, not maxed: one launch stamps pseq and zeroes prio, the next
// takes the maximum of the bit patterns (non-negative floats order like their bits).
// Host + device, header only; pve_mcc_amd/replay.py (PrioritizedReplayModel) restates it in NumPy.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "pve_noise.h"
#include "pve_replay.h"
#include "pve_types.h"

namespace pve {

constexpr int PRIO_PARTS = 32;                               // partitions of the strata tables (replay_buffer.py:15)
constexpr int PRIO_TILE = 2048;                              // keys per workgroup and pass of the sort
constexpr int PRIO_RADIX = 256, PRIO_PASSES = 4;             // 8-bit digits of a 32-bit key
constexpr uint32_t PRIO_NEW_BITS = 0x7F800000u;              // +inf: the priority of a record that was never updated
constexpr uint32_t PRIO_TAG0 = 0x5052494Fu, PRIO_TAG1 = 0x52414E4Bu;          // "PRIO", "RANK"
constexpr int PRIO_DRAWS = 0, PRIO_LIVE = 1, PRIO_PART = 2, PRIO_IGNORED = 3, PRIO_STATE_WORDS = 4;

// the sort key of a slot: ascending keys = descending priorities
PVE_HD uint32_t prio_key(bool valid, uint32_t bits) { return ~(valid ? bits : PRIO_NEW_BITS); }

// partition index of L live records: 0 (below the first threshold: nothing can be drawn) .. PRIO_PARTS
template <class T> PVE_HD int prio_partition(const T &part_from, long long L)
{
    int k = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < PRIO_PARTS; i++) k += part_from[i] <= L ? 1 : 0;
    return k;
}

// the rank stratum j of minibatch d draws from a table row of batch + 1 entries
PVE_HD int32_t prio_draw_rank(const int32_t *ends_row, uint64_t seed, uint64_t d, uint32_t j, long long L)
{
    const int32_t e0 = ends_row[j] + 1, e1 = ends_row[j + 1];
    const int32_t lo = e0 < e1 ? e0 : e1, hi = e0 < e1 ? e1 : e0;
    uint32_t c[4] = {j, 0u, (uint32_t)d, (uint32_t)(d >> 32)};
    philox4x32_10(c, (uint32_t)seed ^ PRIO_TAG0, (uint32_t)(seed >> 32) ^ PRIO_TAG1);
    const long long r = (long long)lo + (long long)(uint32_t)(((uint64_t)c[0] * (uint32_t)(hi - lo + 1)) >> 32);
    return (int32_t)(r < 1 ? 1 : (r > L ? L : r));
}

PVE_HD float prio_weight(int32_t rank, int32_t rank_max, float alpha_beta)
{
    return powf((float)rank / (float)rank_max, alpha_beta);
}

// the priority bits of one update: |q - target| (|q| without a target), NaN -> +inf
PVE_HD uint32_t prio_update_bits(float q, bool has_target, float target)
{
    const float p = fabsf(has_target ? q - target : q);
    uint32_t b;
    memcpy(&b, &p, 4);
    return b > PRIO_NEW_BITS ? PRIO_NEW_BITS : b;              // (above +inf's pattern: a NaN)
}

// the slot an update of record number w goes to, or -1 when w is not live (stale, never written, -1)
PVE_HD long long prio_update_slot(long long w, long long written, long long capacity)
{
    const long long L = replay_live(written, capacity);
    return (w >= written - L && w < written) ? w % capacity : -1;
}

// scratch of the sort: ping-pong keys and payloads (each padded to 16 bytes), one histogram per tile, the digit totals per pass
PVE_HD long long prio_tiles(long long n) { return (n + PRIO_TILE - 1) / PRIO_TILE; }
PVE_HD long long prio_padded(long long capacity) { return (capacity + 3) & ~3LL; }
PVE_HD size_t prio_scratch_bytes(long long capacity)
{
    return (size_t)prio_padded(capacity) * 16 + ((size_t)prio_tiles(capacity) + PRIO_PASSES) * PRIO_RADIX * 4;
}

struct PrioArgs {
    ReplayArgs R;
    uint32_t *prio;                            // [capacity]
    long long *pseq;                           // [capacity]
    int32_t *order;                            // [capacity]
    long long *pstate;                         // [PRIO_STATE_WORDS]
    uint32_t *keys[2];                         // scratch
    int32_t *vals[2];
    uint32_t *hist;                            // [PRIO_RADIX][tiles], digit-major
    uint32_t *totals;                          // [PRIO_PASSES][PRIO_RADIX]: keys per digit value, per pass
    const int32_t *ends;                       // [PRIO_PARTS][batch + 1]
    long long batch;
    long long part_from[PRIO_PARTS];
};

PVE_HD void prio_carve_scratch(PrioArgs &A, void *scratch)
{
    const long long c = prio_padded(A.R.capacity);
    uint32_t *p = (uint32_t *)scratch;
    A.keys[0] = p; A.keys[1] = p + c;
    A.vals[0] = (int32_t *)(p + 2 * c); A.vals[1] = (int32_t *)(p + 3 * c);
    A.hist = p + 4 * c;
    A.totals = A.hist + prio_tiles(A.R.capacity) * PRIO_RADIX;
}

// LDS of k_prio_sample per workgroup of `block` threads: k_replay_sample's stage + one word per wave for the maximum
PVE_HD size_t prio_sample_lds(int block) { return replay_sample_lds(block) + 16 * sizeof(int); }

#if defined(__HIPCC__)

__global__ __launch_bounds__(1024) void k_prio_reset(const PrioArgs A)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < A.R.capacity; s += stride) A.pseq[s] = -1;
    if (blockIdx.x == 0 && threadIdx.x < PRIO_STATE_WORDS) A.pstate[threadIdx.x] = 0;
}

// Key build: position i of the sort's input is age index L - 1 - i (newest first), so that the stable sort leaves equal
// priorities in descending record number.  Also notes what this ranking saw (live count, partition index) and zeroes the digit
// totals the histogram launches behind it add to.
__global__ __launch_bounds__(1024) void k_prio_keys(const PrioArgs A)
{
    const long long written = A.R.state[REPLAY_WRITTEN], L = replay_live(written, A.R.capacity);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.pstate[PRIO_LIVE] = L;
        A.pstate[PRIO_PART] = prio_partition(A.part_from, L);
    }
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < PRIO_PASSES * PRIO_RADIX; t += blockDim.x) A.totals[t] = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += stride) {
        const long long a = L - 1 - i, w = written - L + a, s = w % A.R.capacity;
        A.keys[0][i] = prio_key(A.pseq[s] == w, A.prio[s]);
        A.vals[0][i] = (int32_t)a;
    }
}

// One pass of the sort, step 1: the digit histogram of every tile of PRIO_TILE keys (LDS integer atomics: the counts do not
// depend on their order), stored digit-major for the scan, and added to the pass's digit totals (integer atomics again).
__global__ __launch_bounds__(1024) void k_prio_hist(const PrioArgs A, const uint32_t *__restrict__ keys, const int shift)
{
    __shared__ uint32_t h[PRIO_RADIX];
    const long long L = replay_live(A.R.state[REPLAY_WRITTEN], A.R.capacity), T = prio_tiles(L), tile = blockIdx.x;
    if (tile >= T) return;                                           // (uniform over the workgroup)
    for (int t = threadIdx.x; t < PRIO_RADIX; t += blockDim.x) h[t] = 0;
    __syncthreads();
    const long long base = tile * PRIO_TILE, end = base + PRIO_TILE < L ? base + PRIO_TILE : L;
    for (long long i = base + threadIdx.x; i < end; i += blockDim.x) atomicAdd(&h[(keys[i] >> shift) & (PRIO_RADIX - 1)], 1u);
    __syncthreads();
    for (int t = threadIdx.x; t < PRIO_RADIX; t += blockDim.x) {
        A.hist[t * T + tile] = h[t];
        if (h[t]) atomicAdd(&A.totals[(shift >> 3) * PRIO_RADIX + t], h[t]);
    }
}

// Step 2: the exclusive scan of the PRIO_RADIX x tiles counts in digit-major order, one workgroup per digit value: its base is
// the sum of the totals of the smaller digit values, its row of per-tile counts is scanned in chunks of blockDim (shuffles inside
// a wave, LDS across the waves, a running carry across the chunks).
__global__ __launch_bounds__(1024) void k_prio_scan(const PrioArgs A, const int pass)
{
    __shared__ uint32_t wsum[16];
    const long long L = replay_live(A.R.state[REPLAY_WRITTEN], A.R.capacity), T = prio_tiles(L);
    const int d = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    uint32_t part = 0;
    for (int t = threadIdx.x; t < d; t += blockDim.x) part += A.totals[pass * PRIO_RADIX + t];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) part += __shfl_xor(part, s, 64);
    if (lane == 0) wsum[wave] = part;
    __syncthreads();
    uint32_t carry = 0;
    for (int w = 0; w < n_waves; w++) carry += wsum[w];
    __syncthreads();
    uint32_t *row = A.hist + d * T;
    for (long long c0 = 0; c0 < T; c0 += blockDim.x) {               // (uniform trip count)
        const long long i = c0 + threadIdx.x;
        const uint32_t v = i < T ? row[i] : 0u;
        uint32_t x = v;                                              // inclusive scan inside the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t y = __shfl_up(x, s, 64);
            if (lane >= s) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < n_waves; w++) {
            const uint32_t c = wsum[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        if (i < T) row[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
}

// Step 3: the scatter.  A tile is worked in rounds of blockDim keys in input order.  In a round every lane finds the lanes of
// its wave that hold the same digit (eight ballots), its rank among them (the lanes below it) and their number; the per-wave
// counts are turned into offsets in wave order behind the digit's running base, so that equal digits keep their input order:
// across tiles by the scan, across rounds by the base, across waves by the prefix, inside a wave by the lane rank.
__global__ __launch_bounds__(1024) void k_prio_scatter(const PrioArgs A, const uint32_t *__restrict__ kin, const int32_t *__restrict__ vin,
                                                       uint32_t *__restrict__ kout, int32_t *__restrict__ vout, const int shift)
{
    __shared__ uint32_t cnt[16 * PRIO_RADIX], off[16 * PRIO_RADIX], base_s[PRIO_RADIX];
    const long long L = replay_live(A.R.state[REPLAY_WRITTEN], A.R.capacity), T = prio_tiles(L), tile = blockIdx.x;
    if (tile >= T) return;                                           // (uniform over the workgroup)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (int t = threadIdx.x; t < PRIO_RADIX; t += blockDim.x) base_s[t] = A.hist[t * T + tile];
    for (int t = threadIdx.x; t < n_waves * PRIO_RADIX; t += blockDim.x) cnt[t] = 0;
    __syncthreads();
    const long long first = tile * PRIO_TILE, end = first + PRIO_TILE < L ? first + PRIO_TILE : L;
    for (long long r0 = first; r0 < end; r0 += blockDim.x) {         // (uniform trip count: every barrier is reached by all)
        const long long i = r0 + threadIdx.x;
        const bool valid = i < end;
        const uint32_t key = valid ? kin[i] : 0u;
        const int32_t val = valid ? vin[i] : 0;
        const uint32_t d = (key >> shift) & (PRIO_RADIX - 1);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long b = __ballot(one);
            same &= one ? b : ~b;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) cnt[wave * PRIO_RADIX + d] = (uint32_t)__popcll(same);
        __syncthreads();
        for (int t = threadIdx.x; t < PRIO_RADIX; t += blockDim.x) {
            uint32_t run = base_s[t];
            for (int w = 0; w < n_waves; w++) {
                const uint32_t c = cnt[w * PRIO_RADIX + t];
                off[w * PRIO_RADIX + t] = run;
                cnt[w * PRIO_RADIX + t] = 0;
                run += c;
            }
            base_s[t] = run;
        }
        __syncthreads();
        if (valid) {
            const uint32_t pos = off[wave * PRIO_RADIX + d] + rank;
            kout[pos] = key;
            vout[pos] = val;
        }
    }
}

// One workgroup per minibatch.  First the minibatch's largest rank (every thread draws the strata j = thread, thread + block,
// ..; wave reduction, then LDS across the waves), then the draws again in chunks of blockDim, each chunk through the 16-byte
// row path of k_replay_sample: seq / rank / weight per lane, the 9 pieces of a wave's 64 records lane after lane, the 7 actions
// and the target through the LDS stage.  Short (fewer live records than min_live, or below the first partition threshold):
// seq = -1 and zeros.  Reads the states, never writes them (k_prio_sample_commit).
__global__ __launch_bounds__(1024) void k_prio_sample(const PrioArgs A, const long long min_live, const float alpha_beta,
                                                      float *__restrict__ rows, float *__restrict__ act7, float *__restrict__ target,
                                                      long long *__restrict__ seq, int32_t *__restrict__ rank_out, float *__restrict__ weight)
{
    extern __shared__ __attribute__((aligned(16))) float tail_s[];
    int *slot_s = (int *)(tail_s + (size_t)blockDim.x * 8);
    int *max_s = slot_s + blockDim.x;
    const long long written = A.R.state[REPLAY_WRITTEN], draws = A.pstate[PRIO_DRAWS], L = replay_live(written, A.R.capacity);
    const int part = prio_partition(A.part_from, L);
    const bool empty = L < min_live || part == 0;
    const long long batch = A.batch, m = blockIdx.x;
    const int32_t *ends_row = A.ends + (long long)(part > 0 ? part - 1 : 0) * (batch + 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    int rank_max = 1;
    if (!empty)
        for (long long j = threadIdx.x; j < batch; j += blockDim.x) {
            const int r = prio_draw_rank(ends_row, A.R.seed, (uint64_t)(draws + m), (uint32_t)j, L);
            rank_max = r > rank_max ? r : rank_max;
        }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int other = __shfl_xor(rank_max, s, 64);
        rank_max = other > rank_max ? other : rank_max;
    }
    if (lane == 0) max_s[wave] = rank_max;
    __syncthreads();
    for (int w = 0; w < n_waves; w++) rank_max = max_s[w] > rank_max ? max_s[w] : rank_max;
    const float4 *store = (const float4 *)A.R.store;
    float *tail = tail_s + wave * (64 * 8);
    for (long long c0 = 0; c0 < batch; c0 += blockDim.x) {           // (uniform trip count)
        const long long j = c0 + threadIdx.x, g = m * batch + j;
        long long w = -1;
        int r = 0;
        if (j < batch && !empty) {
            r = prio_draw_rank(ends_row, A.R.seed, (uint64_t)(draws + m), (uint32_t)j, L);
            w = written - L + A.order[r - 1];
        }
        if (j < batch) {
            seq[g] = w;
            rank_out[g] = r;
            weight[g] = empty ? 0.0f : prio_weight(r, rank_max, alpha_beta);
        }
        slot_s[threadIdx.x] = w < 0 ? -1 : (int)(w % A.R.capacity);
        __syncthreads();
        const long long j0 = c0 + wave * 64, g0 = m * batch + j0, left = batch - j0;
        const int count = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        float4 *rows4 = (float4 *)rows + g0 * (OBSW / 4);
#pragma unroll
        for (int it = 0; it < REPLAY_PIECES; it++) {
            const int p = it * 64 + lane, rec = p / REPLAY_PIECES, k = p - rec * REPLAY_PIECES;
            if (rec < count) {
                const long long s = slot_s[wave * 64 + rec];
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
        __syncthreads();
    }
}

__global__ void k_prio_sample_commit(const PrioArgs A, const long long min_live, const long long n_batches)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long L = replay_live(A.R.state[REPLAY_WRITTEN], A.R.capacity);
    if (L >= min_live && prio_partition(A.part_from, L) > 0) A.pstate[PRIO_DRAWS] += n_batches;
}

// Update, launch 1: every live id named stamps its slot and zeroes its priority (racing writers write the same values)
__global__ __launch_bounds__(1024) void k_prio_update_stamp(const PrioArgs A, const long long *__restrict__ seq, const long long n)
{
    const long long written = A.R.state[REPLAY_WRITTEN], stride = (long long)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) A.pstate[PRIO_IGNORED] = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long w = seq[i], s = prio_update_slot(w, written, A.R.capacity);
        if (s >= 0) { A.pseq[s] = w; A.prio[s] = 0u; }
    }
}

// Update, launch 2: the maximum of the bit patterns; the ignored ids are counted, one atomic per wave
__global__ __launch_bounds__(1024) void k_prio_update_max(const PrioArgs A, const long long *__restrict__ seq, const float *__restrict__ q,
                                                          const float *__restrict__ target, const long long n)
{
    const long long written = A.R.state[REPLAY_WRITTEN], stride = (long long)gridDim.x * blockDim.x;
    const long long rounds = (n + stride - 1) / stride;              // (every lane makes every round: the ballot sees whole waves)
    for (long long r = 0; r < rounds; r++) {
        const long long i = r * stride + (long long)blockIdx.x * blockDim.x + threadIdx.x;
        bool ignored = false;
        if (i < n) {
            const long long s = prio_update_slot(seq[i], written, A.R.capacity);
            ignored = s < 0;
            if (s >= 0) atomicMax(&A.prio[s], prio_update_bits(q[i], target != nullptr, target ? target[i] : 0.0f));
        }
        const unsigned long long bal = __ballot(ignored);
        if ((threadIdx.x & 63) == 0 && bal) atomicAdd((unsigned long long *)&A.pstate[PRIO_IGNORED], (unsigned long long)__popcll(bal));
    }
}

#endif  // __HIPCC__

}  // namespace pve

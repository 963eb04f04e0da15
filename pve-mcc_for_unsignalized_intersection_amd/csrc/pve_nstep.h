// pve_nstep.h -- n-step training transitions from retained trajectory blocks (reference main.py:243-266: every controlled
// vehicle keeps its last seq_max_step + 1 = 13 ticks; when the buffer is full or the vehicle is Done the rewards are folded
// with gamma into one target, gamma * Q' is added behind the last entry unless the vehicle is Done, and ONE transition -- the
// oldest entry's (s0, a, target) -- goes into the replay buffer).
//
// A STATELESS pass over the [n_ticks][n_envs][cap] blocks pve_step_many(trajectory = 1) leaves behind; nothing is kept in the
// handle and no tick kernel is involved.  The pass is indexed by a window's START (u, env, slot), PVE_F_CTL set at u: one thread
// walks forward through new_slot, at most window - 1 links, and the start emits
//   - FULL WINDOW: the walk collected `window` entries; bootstrapped unless the last entry is Done;
//   - DONE BEFORE THE WINDOW IS FULL: only when u is the vehicle's first controlled tick (the reference emits the OLDEST buffered
//     entry at Done and drops the younger ones), recognised by its all-zero s0 row (only a vehicle spawned at the end of the
//     previous tick has one, ref :380; a live vehicle's row holds its speed >= vm > 0, ref :1336) -- or always with NSTEP_TAIL.
// A start emits in this call iff its window CLOSES at a tick of `cur`; a walk that runs off the end of `cur` is pending (it emits
// in the next call, which gets `cur` as `prev`), a window that closed inside `prev` was emitted by the previous call.
//
// Target: float64, the reference's backward Horner order  r = r_last (+ gamma * (double)Q');  r = r_k + gamma * r  for the older
// entries, every operation rounded on its own (no fused multiply-add): the kernel, a g++ build of this header and the NumPy
// restatement (pve_mcc_amd/nstep.py) are bit-equal.  Host + device, header only.
//
// Code word of a start: bits 0-7 entries used, bit 8 bootstrapped, bit 9 closed by Done; 0 = no transition.
#pragma once
#include <stdint.h>

#include "pve_types.h"

namespace pve {

constexpr int NSTEP_F_CTL = 0x02, NSTEP_F_DONE = 0x04;      // PVE_F_CTL / PVE_F_DONE of include/pve_env.h
constexpr int NSTEP_TAIL = 0x1;                              // PVE_NSTEP_TAIL
constexpr int NSTEP_MAX_WINDOW = 16;
constexpr int NSTEP_BOOT = 0x100, NSTEP_DONE = 0x200;
constexpr int NSTEP_REC = 36;                                // float32 per record: s0 row [28], actions [7], target [1]
constexpr int NSTEP_GROUP = 64;                              // slots per count group (one wave)

struct NstepSeg {
    int n_ticks;
    const void *obs_post, *state_pre;          // [n_ticks][n_envs][cap][28] / [..][7][28], float64 or float32 (obs_f32)
    const double *reward;                      // [n_ticks][n_envs][cap]
    const int32_t *flags, *new_slot;
};

struct NstepArgs {
    double gamma;
    int window, mode, n_envs, cap, obs_f32;
    int n_back;                                // candidate start ticks in front of cur: min(prev.n_ticks, window - 1)
    NstepSeg prev, cur;
    const void *obs_first;                     // [n_envs][cap][28]: the rows stored before cur's first tick (prev.n_ticks == 0)
    const float *q_boot;                       // [cur.n_ticks][n_envs][cap]
    double *target;                            // [n_back + cur.n_ticks][n_envs][cap], start-indexed
    int32_t *code;                             // same shape
    int32_t *offsets;                          // [groups + 1]: counts per 64-slot group, then their exclusive prefix sums
    long long *total;
    long long max_records;
    float *records;                            // [max_records][36]
    int32_t *index;                            // [max_records][4]: tick relative to cur, env, slot, code
};

// the s0 row of a start at tick t (relative to cur): what the tick before it stored for the slot
PVE_HD const void *nstep_row(const NstepArgs &A, int t, long long env_slot)
{
    const long long EK = (long long)A.n_envs * A.cap;
    const void *base;
    long long i;
    if (t > 0) { base = A.cur.obs_post; i = (long long)(t - 1) * EK + env_slot; }
    else if (A.prev.n_ticks > 0) { base = A.prev.obs_post; i = (long long)(A.prev.n_ticks + t - 1) * EK + env_slot; }
    else { base = A.obs_first; i = env_slot; }
    return A.obs_f32 ? (const void *)((const float *)base + i * OBSW) : (const void *)((const double *)base + i * OBSW);
}

PVE_HD bool nstep_row_is_zero(const NstepArgs &A, int t, long long env_slot)
{
    const void *row = nstep_row(A, t, env_slot);
    bool zero = true;
    for (int c = 0; c < OBSW; c++) zero = zero && (A.obs_f32 ? ((const float *)row)[c] == 0.0f : ((const double *)row)[c] == 0.0);
    return zero;
}

// The walk, the emit rule and the fold of the start (t, env, slot), t relative to cur (t < 0: tick prev.n_ticks + t of prev).
// Returns the code word (0: no transition in this call) and the target.
PVE_HD int nstep_window(const NstepArgs &A, int t, int env, int slot, double &target)
{
#if defined(__clang__)
#pragma clang fp contract(off)                   // (whatever the translation unit's default: every operation rounds on its own)
#endif
    const long long EK = (long long)A.n_envs * A.cap, base = (long long)env * A.cap;
    double r[NSTEP_MAX_WINDOW];
    int s = slot, n = 0, s_last = slot;
    bool walking = true, bad = false, done = false;
    target = 0.0;
    // Fully unrolled with constant indices (the rewards stay in registers) and without divergent branches: a lane that has
    // stopped walking keeps loading entry 0 of cur (a valid address, one broadcast line) and discards it.
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < NSTEP_MAX_WINDOW; k++) {
        r[k] = 0.0;
        if (k < A.window) {                                               // (uniform)
            const int tk = t + k;
            const bool pending = walking && tk >= A.cur.n_ticks;          // closes in a later call
            bad = bad || pending; walking = walking && !pending;
            const bool in_prev = tk < 0;
            const long long i = walking ? (long long)(in_prev ? tk + A.prev.n_ticks : tk) * EK + base + s : 0;
            const int32_t *fl = in_prev && walking ? A.prev.flags : A.cur.flags, *ns = in_prev && walking ? A.prev.new_slot : A.cur.new_slot;
            const double *rw = in_prev && walking ? A.prev.reward : A.cur.reward;
            const int f = fl[i];
            const double rk = rw[i];
            const int nx = ns[i];
            const bool lost = walking && !(f & NSTEP_F_CTL);              // not (or no longer) a controlled vehicle
            bad = bad || lost; walking = walking && !lost;
            r[k] = walking ? rk : 0.0;
            n = walking ? k + 1 : n; s_last = walking ? s : s_last;
            const bool d = walking && (f & NSTEP_F_DONE);
            done = done || d; walking = walking && !d;
            if (k + 1 < A.window) {                                       // (uniform)
                const bool broken = walking && (nx < 0 || nx >= A.cap);   // a broken link: no transition
                bad = bad || broken; walking = walking && !broken;
                s = walking ? nx : s;
            }
        }
    }
    if (bad) return 0;
    const int t_close = t + n - 1;
    if (n == 0 || t_close < 0) return 0;                                  // closed inside prev: the previous call's
    const bool full = n == A.window;
    if (!full && !(A.mode & NSTEP_TAIL) && !nstep_row_is_zero(A, t, base + slot)) return 0;   // a younger start of a vehicle that died
    const bool boot = !done;
    double q = 0.0;
    if (boot) q = (double)A.q_boot[(long long)t_close * EK + base + s_last];
    double acc = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = NSTEP_MAX_WINDOW - 1; k >= 0; k--) {
        if (k == n - 1) {
            acc = r[k];
            if (boot) { const double gq = A.gamma * q; acc = r[k] + gq; }
        } else if (k < n - 1) {
            const double ga = A.gamma * acc;
            acc = r[k] + ga;
        }
    }
    target = acc;
    return n | (boot ? NSTEP_BOOT : 0) | (done ? NSTEP_DONE : 0);
}

// number of 64-slot groups of the candidate starts
PVE_HD long long nstep_groups(const NstepArgs &A)
{
    return (long long)(A.n_back + A.cur.n_ticks) * A.n_envs * A.cap / NSTEP_GROUP;
}

#if defined(__HIPCC__)

// One thread per candidate start (tick, env, slot); a wave is one 64-slot group of one (tick, env) row (cap is a multiple of
// 64), so the group's record count is a ballot + popcount: no atomics, and the record order (tick, env, slot ascending) does not
// depend on the launch geometry.  Latency-bound on the dependent loads of the walk: the reads at the start tick are coalesced
// (lane = slot), later entries follow new_slot (near-monotone), q_boot is read at the closing entry only.
__global__ __launch_bounds__(1024) void k_nstep_scan(const NstepArgs A, const long long n_slots)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_slots) return;                          // (whole waves: n_slots and blockDim are multiples of 64)
    const long long EK = (long long)A.n_envs * A.cap;
    const int tc = (int)(g / EK);
    const long long es = g - (long long)tc * EK;
    const int env = (int)(es / A.cap), slot = (int)(es - (long long)env * A.cap);
    double target;
    const int code = nstep_window(A, tc - A.n_back, env, slot, target);
    A.target[g] = target;
    A.code[g] = code;
    const unsigned long long b = __ballot(code != 0);
    if ((threadIdx.x & 63) == 0) A.offsets[g >> 6] = (int32_t)__popcll(b);
}

// counts -> exclusive offsets (in place) and the total, one workgroup: every thread owns a contiguous run of groups, sums it,
// the 1024 sums are scanned in LDS, and the run is rewritten with its running offsets.
__global__ __launch_bounds__(1024) void k_nstep_offsets(int32_t *__restrict__ offsets, const long long n_groups, long long *__restrict__ total)
{
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const long long per = (n_groups + 1023) / 1024, lo = per * tid, hi = lo + per < n_groups ? lo + per : n_groups;
    long long sum = 0;
    for (long long i = lo; i < hi; i++) sum += offsets[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long run = part[tid] - sum;
    for (long long i = lo; i < hi; i++) { const int32_t c = offsets[i]; offsets[i] = (int32_t)run; run += c; }
    if (tid == 1023) { offsets[n_groups] = (int32_t)part[1023]; *total = part[1023]; }
}

// a 28-value row (16-byte aligned: 112 / 224 B per row) -> float32 in LDS, with 16-byte loads
__device__ __forceinline__ void nstep_load_row(const float *row, float *dst)
{
#pragma unroll
    for (int j = 0; j < OBSW / 4; j++) ((float4 *)dst)[j] = ((const float4 *)row)[j];
}
__device__ __forceinline__ void nstep_load_row(const double *row, float *dst)
{
#pragma unroll
    for (int j = 0; j < OBSW / 4; j++) {
        const double2 a = ((const double2 *)row)[2 * j], b = ((const double2 *)row)[2 * j + 1];
        float4 v; v.x = (float)a.x; v.y = (float)a.y; v.z = (float)b.x; v.w = (float)b.y;
        ((float4 *)dst)[j] = v;
    }
}

// Record i = 36 float32 (144 B = 9 x 16 B): every wave stages the records of its group in LDS in rank order and writes the
// group's contiguous run of the output with 16-byte stores, lane after lane; the index rows (16 B) go out one per lane.
template <typename OBS>
__global__ __launch_bounds__(256) void k_nstep_gather(const NstepArgs A, const long long n_slots)
{
    __shared__ __attribute__((aligned(16))) float stage[4][NSTEP_GROUP * NSTEP_REC];
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_slots) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long EK = (long long)A.n_envs * A.cap;
    const int tc = (int)(g / EK);
    const long long es = g - (long long)tc * EK;
    const int env = (int)(es / A.cap), slot = (int)(es - (long long)env * A.cap), t = tc - A.n_back;
    const int code = A.code[g];
    const unsigned long long b = __ballot(code != 0);
    if (b == 0) return;                                 // (wave-uniform)
    const int rank = (int)__popcll(b & ((1ull << lane) - 1ull)), count = (int)__popcll(b);
    const long long first = A.offsets[g >> 6];
    float *mine = stage[wave] + rank * NSTEP_REC;
    if (code != 0) {
        const OBS *row = (const OBS *)nstep_row(A, t, es);
        nstep_load_row(row, mine);
        const NstepSeg &S = t < 0 ? A.prev : A.cur;
        const OBS *st = (const OBS *)S.state_pre + ((long long)(t < 0 ? t + A.prev.n_ticks : t) * EK + es) * (OBSW * (NNB + 1));
#pragma unroll
        for (int k = 0; k < NNB + 1; k++) mine[OBSW + k] = (float)st[k * OBSW + 2];      // column 2 of the 7 rows (ref :290)
        mine[NSTEP_REC - 1] = (float)A.target[g];
        if (first + rank < A.max_records) {
            int4 ix; ix.x = t; ix.y = env; ix.z = slot; ix.w = code;
            ((int4 *)A.index)[first + rank] = ix;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    long long keep = A.max_records - first;              // records of this group inside the cut-off
    if (keep > count) keep = count;
    const int n16 = keep > 0 ? (int)keep * (NSTEP_REC / 4) : 0;
    float4 *dst = (float4 *)(A.records + first * NSTEP_REC);
    const float4 *src = (const float4 *)stage[wave];
    for (int i = lane; i < n16; i += 64) dst[i] = src[i];
}

#endif  // __HIPCC__

}  // namespace pve

// pve_stats.h -- roll-out and evaluation statistics reduced where the roll-out leaves them (reference main.py:286-304: the
// per-tick summaries `collisions`, v_mean = mean(state_next[:,0,1]), acc_mean = mean(state_next[:,0,2]), the reward mean and the
// collided-vehicle count; main.py:315-328: best.cptk is kept by the epoch's collisions_count / id_seq; main.py:413-415: test()
// prints np.std(reward) and np.mean(reward); main.py:543-583: batch_test() prints one line per density).
// pve_rollout_stats reduces retained output blocks of pve_step_many by tick and by group of environments; pve_metrics_groups
// reads the twelve sums of pve_get_metrics from the per-environment headers by group.  Both are stateless passes on the
// handle's stream: no tick kernel is involved, nothing is copied to the host and nothing waits.
// Host + device, header only.  THIS FILE IS THE DEFINITION: the kernels below, the g++ build of rollout_stats_host /
// metrics_groups_host (tests/stats_host) and the NumPy restatement (pve_mcc_amd/stats.py) are held to it bit for bit.
//
// Inputs of the roll-out pass (T ticks, E environments, cap slots, cap a multiple of 64):
//   flags[T][E][cap] int32, reward[T][E][cap] float64, env_out[T][E][8] int32, obs_pre[T][E][cap][28] float64 or float32
//   (PVE_CFG_OBS_F32) or null, group[E] int32 or null (null: every environment is in group 0 and G = 1).
// Output: series[T][G][STAT_N] float64.  Every column is additive over environments and over ticks.
//
// Columns of one (tick, env), the "env row" x[t][e][.] (also the layout of the scratch block [T][E][STAT_N]):
//   ENV_TICKS   1
//   ALIVE, SPAWNED, FINISHED, DELETED, COLLISIONS, LOCK
//               env_out[N_PRE], [N_SPAWNED], [N_FINISHED], [N_DELETED], [COLLISIONS] (the 9-tuple's `collisions`, ref :337,
//               main.py:287), [LOCK]
//   CTL         slots with F_CTL                              (= len(ids))
//   COLLIDED    slots with F_CTL and (flags >> 8) > 0         (main.py:276-278 / :410-412; what metrics()["collided"] accumulates)
//   DONE        slots with F_CTL and F_DONE
//   SUM_REWARD, SUM_REWARD_SQ, SUM_V, SUM_A
//               over the F_CTL slots: reward, reward * reward (one rounding), obs_pre[..][1], obs_pre[..][2] (float32 widened
//               exactly; main.py:290, :294).  SUM_V and SUM_A are +0.0 when obs_pre is null.
//
// Selection.  A slot enters a sum through a SELECT on its flags word, never through a multiplication by a mask: the value of a
// slot without F_CTL is +0.0 whatever bits its reward / obs_pre hold (pve_outputs leaves them unspecified; a NaN pattern there
// does not reach a sum); the observation row of such a slot is not even loaded.
//
// THE ORDER of the float64 sums (the integer columns are exact in any order: every count is far below 2^53).  One shape is used
// twice, tree64(v[0..63]):
//       for w = 1, 2, 4, 8, 16, 32:  v[l] = v[l] + v[l + w]  for every l that is a multiple of 2 w;       the result is v[0].
//   (neighbours first: the pairs a wave forms with its cheapest lane exchanges)
//   1. slots of one (tick, env):  p[l] = +0.0;  for k = 0 .. cap/64 - 1 ascending:  p[l] = p[l] + value(slot 64 k + l);
//      x = tree64(p).
//   2. environments of one (tick, group g):  chunk j holds the environments 64 j .. 64 j + 63;  m[l] = x[t][64 j + l][c] if that
//      environment exists and group[64 j + l] == g, else +0.0;  q[j] = tree64(m);  s = +0.0;  for j = 0 .. ceil(E / 64) - 1
//      ascending:  s = s + q[j];  series[t][g][c] = s.
//   3. totals (optional, [G][STAT_N]):  for t = 0 .. T - 1 ascending:  totals[g][c] = totals[g][c] + series[t][g][c].
// The order depends on (cap, E, the group map) alone: not on the grid, the workgroup size, the wave count or the device.  All
// fourteen columns go through 2. and 3. as float64 (exact for the integer ones).  No floating-point atomics anywhere.
// An environment whose group id lies outside [0, G) is a member of no group: it is counted nowhere (the host cannot check the
// map without a wait).
//
// Grouped metrics.  out[g][PVE_N_METRICS] float64 from the EnvHeaders: the ten counters are integer sums over the group's
// environments (slot_steps = (sum of ticks) * cap), converted once -- equal to pve_get_metrics' float64 accumulation while the sums
// stay below 2^53; sum_reward and sum_jerk:  s = +0.0;  for e ascending, group[e] == g:  s = s + header[e].sum_*  -- the order
// pve_get_metrics uses on the host, so one group reproduces its bits.
#pragma once
#include <stdint.h>

#include "pve_types.h"

namespace pve {

constexpr int STAT_N = 14;
enum { STAT_ENV_TICKS = 0, STAT_ALIVE, STAT_SPAWNED, STAT_FINISHED, STAT_DELETED, STAT_COLLISIONS, STAT_LOCK, STAT_CTL,
       STAT_COLLIDED, STAT_DONE, STAT_SUM_REWARD, STAT_SUM_REWARD_SQ, STAT_SUM_V, STAT_SUM_A };
constexpr int STAT_MAX_GROUPS = 1024;
constexpr int STAT_N_METRICS = 12;                          // PVE_N_METRICS, in the order of the PVE_M_* enum
constexpr int STAT_F_CTL = 0x02, STAT_F_DONE = 0x04;        // PVE_F_CTL / PVE_F_DONE of include/pve_env.h
// env_out index (PVE_EO_*) of the columns ALIVE .. LOCK, four bits each from bit 0: N_PRE 0, N_SPAWNED 6, N_FINISHED 5,
// N_DELETED 4, COLLISIONS 2, LOCK 3
constexpr unsigned STAT_EO_OF_COLUMN = 0x324560u;
constexpr int STAT_LANES = 64;                              // width of tree64: slots per step of 1., environments per chunk of 2.
constexpr int STAT_BATCH = 64;                              // chunks whose q[j] wait in LDS at a time (launch detail, never results)

struct StatsArgs {
    int n_envs, cap, n_ticks, n_groups, obs_f32;
    const int32_t *group;                                   // [n_envs] or null
    const int32_t *flags;
    const double *reward;
    const void *obs_pre;                                    // or null
    const int32_t *env_out;
    double *series;                                         // [n_ticks][n_groups][STAT_N]
    double *totals;                                         // [n_groups][STAT_N] or null
    double *scratch;                                        // [n_ticks][n_envs][STAT_N]: the env rows
};

inline size_t stats_scratch_bytes(long long n_envs, long long n_ticks)
{
    return (size_t)n_envs * (size_t)n_ticks * STAT_N * sizeof(double);
}

PVE_HD double stats_tree64_host(double *v)                 // (the plain statement of tree64; destroys v)
{
    for (int w = 1; w <= 32; w <<= 1)
        for (int l = 0; l < STAT_LANES; l += 2 * w) v[l] = v[l] + v[l + w];
    return v[0];
}

// ---------------------------------------------------------------------------------------------------------------- host loops
// The roll-out pass as plain loops: env rows into A.scratch, then series, then totals.
inline void rollout_stats_host(const StatsArgs &A)
{
    const long long E = A.n_envs, cap = A.cap;
    for (long long t = 0; t < A.n_ticks; t++)
        for (long long e = 0; e < E; e++) {
            const long long it = t * E + e;
            const int32_t *fl = A.flags + it * cap, *eo = A.env_out + it * 8;
            const double *rw = A.reward + it * cap;
            double p[4][STAT_LANES];
            for (int c = 0; c < 4; c++)
                for (int l = 0; l < STAT_LANES; l++) p[c][l] = 0.0;
            long long n_ctl = 0, n_col = 0, n_done = 0;
            for (long long s = 0; s < cap; s++) {
                const int f = fl[s];
                if (!(f & STAT_F_CTL)) continue;                                  // (adding +0.0 to p[l] changes nothing: p[l] is never -0.0)
                n_ctl++;
                n_col += (f >> 8) > 0;
                n_done += (f & STAT_F_DONE) != 0;
                const double r = rw[s];
                double v = 0.0, a = 0.0;
                if (A.obs_pre) {
                    const long long row = (it * cap + s) * OBSW;
                    if (A.obs_f32) { v = (double)((const float *)A.obs_pre)[row + 1]; a = (double)((const float *)A.obs_pre)[row + 2]; }
                    else { v = ((const double *)A.obs_pre)[row + 1]; a = ((const double *)A.obs_pre)[row + 2]; }
                }
                const int l = (int)(s % STAT_LANES);
                p[0][l] = p[0][l] + r;
                const double rr = r * r;
                p[1][l] = p[1][l] + rr;
                p[2][l] = p[2][l] + v;
                p[3][l] = p[3][l] + a;
            }
            double *x = A.scratch + it * STAT_N;
            x[STAT_ENV_TICKS] = 1.0;
            for (int c = STAT_ALIVE; c <= STAT_LOCK; c++) x[c] = (double)eo[(STAT_EO_OF_COLUMN >> (4 * (c - 1))) & 7];
            x[STAT_CTL] = (double)n_ctl; x[STAT_COLLIDED] = (double)n_col; x[STAT_DONE] = (double)n_done;
            for (int c = 0; c < 4; c++) x[STAT_SUM_REWARD + c] = stats_tree64_host(p[c]);
        }
    const long long chunks = (E + STAT_LANES - 1) / STAT_LANES;
    for (long long t = 0; t < A.n_ticks; t++)
        for (int g = 0; g < A.n_groups; g++)
            for (int c = 0; c < STAT_N; c++) {
                double s = 0.0;
                for (long long j = 0; j < chunks; j++) {
                    double m[STAT_LANES];
                    for (int l = 0; l < STAT_LANES; l++) {
                        const long long e = j * STAT_LANES + l;
                        const bool member = e < E && (A.group ? A.group[e] == g : g == 0);
                        m[l] = member ? A.scratch[(t * E + e) * STAT_N + c] : 0.0;
                    }
                    s = s + stats_tree64_host(m);
                }
                A.series[(t * A.n_groups + g) * STAT_N + c] = s;
            }
    if (A.totals)
        for (long long i = 0; i < (long long)A.n_groups * STAT_N; i++)
            for (long long t = 0; t < A.n_ticks; t++) A.totals[i] = A.totals[i] + A.series[t * A.n_groups * STAT_N + i];
}

// The grouped metrics as a plain loop over the headers.
inline void metrics_groups_host(const EnvHeader *hd, int n_envs, int cap, const int32_t *group, int n_groups, double *out)
{
    for (int g = 0; g < n_groups; g++) {
        long long ticks = 0, alive = 0, ctl = 0, spawned = 0, passed = 0, collided = 0, locks = 0, psteps = 0, overflow = 0;
        double sr = 0.0, sj = 0.0;
        for (int e = 0; e < n_envs; e++) {
            if (!(group ? group[e] == g : g == 0)) continue;
            ticks += hd[e].ticks; alive += hd[e].alive_steps; ctl += hd[e].ctl_steps; spawned += hd[e].id_seq; passed += hd[e].passed;
            collided += hd[e].collided; locks += hd[e].locks; psteps += hd[e].passed_step_total; overflow += hd[e].overflow;
            sr = sr + hd[e].sum_reward; sj = sj + hd[e].sum_jerk;
        }
        double *o = out + (long long)g * STAT_N_METRICS;
        o[0] = (double)(ticks * cap); o[1] = (double)alive; o[2] = (double)ctl; o[3] = (double)spawned; o[4] = (double)passed;
        o[5] = (double)collided; o[6] = (double)locks; o[7] = sr; o[8] = sj; o[9] = (double)psteps; o[10] = (double)overflow;
        o[11] = (double)ticks;
    }
}

#if defined(__HIPCC__)

// tree64 across the 64 lanes of a wave.  Every lane takes v[l] + v[l ^ w]; for the lanes the definition names that is its sum
// (IEEE addition is commutative), and after the step for w every aligned run of 2 w lanes holds one value.  So the steps 1 and
// 2 are quad permutations, 4 and 8 the mirrors of a half row and of a row (the mirrored lane lies in the other run, and all
// lanes of a run are equal), all on the DPP path; 16 and 32 add the four rows' values, read from lanes 0, 16, 32 and 48.
// Needs all 64 lanes active.  Returns tree64's result in every lane.
template <int CTRL> __device__ __forceinline__ double stats_dpp(double v)
{
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double stats_readlane(double x, int src)       // src is wave-uniform
{
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src), lo = __builtin_amdgcn_readlane(__double2loint(x), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double stats_tree64(double v)
{
    v = v + stats_dpp<0xB1>(v);                   // quad_perm [1, 0, 3, 2]: l ^ 1
    v = v + stats_dpp<0x4E>(v);                   // quad_perm [2, 3, 0, 1]: l ^ 2
    v = v + stats_dpp<0x141>(v);                  // row_half_mirror: 7 - l within 8 lanes
    v = v + stats_dpp<0x140>(v);                  // row_mirror: 15 - l within 16 lanes
    const double r01 = stats_readlane(v, 0) + stats_readlane(v, 16), r23 = stats_readlane(v, 32) + stats_readlane(v, 48);
    return r01 + r23;
}

// 1. The env rows.  One wave per (tick, env), waves striding over the items: a lane owns the slots 64 k + l, so the result does
// not depend on how many waves a workgroup has or how many workgroups run.  Reads: 4 + 8 bytes of every slot (the reward of a
// slot without F_CTL is loaded too: the line is there anyway, and the select drops it), 8 or 16 bytes of every controlled row,
// 24 of the 32 bytes of env_out; writes 112 bytes.  Counts are popcounts of ballots.
__global__ __launch_bounds__(1024) void k_stats_rows(const StatsArgs A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long long items = (long long)A.n_ticks * A.n_envs, cap = A.cap;
    const float *obs32 = (const float *)A.obs_pre;
    const double *obs64 = (const double *)A.obs_pre;
    for (long long it = (long long)blockIdx.x * nw + wave; it < items; it += (long long)gridDim.x * nw) {
        const int32_t *fl = A.flags + it * cap;
        const double *rw = A.reward + it * cap;
        double eo = 0.0;
        if (lane >= STAT_ALIVE && lane <= STAT_LOCK) eo = (double)A.env_out[it * 8 + ((STAT_EO_OF_COLUMN >> (4 * (lane - 1))) & 7)];
        double pr = 0.0, pq = 0.0, pv = 0.0, pa = 0.0;
        int n_ctl = 0, n_col = 0, n_done = 0;
        for (int s0 = 0; s0 < A.cap; s0 += STAT_LANES) {
            const int s = s0 + lane;
            const int f = fl[s];
            const double r_raw = rw[s];
            const bool ctl = (f & STAT_F_CTL) != 0;
            double v = 0.0, a = 0.0;
            if (ctl && A.obs_pre) {
                const long long row = (it * cap + s) * OBSW;
                if (A.obs_f32) { v = (double)obs32[row + 1]; a = (double)obs32[row + 2]; }
                else { v = obs64[row + 1]; a = obs64[row + 2]; }
            }
            const double r = ctl ? r_raw : 0.0;
            pr = pr + r;
            const double rr = r * r;
            pq = pq + rr;
            pv = pv + v;
            pa = pa + a;
            n_ctl += __popcll(__ballot(ctl));
            n_col += __popcll(__ballot(ctl && (f >> 8) > 0));
            n_done += __popcll(__ballot(ctl && (f & STAT_F_DONE) != 0));
        }
        pr = stats_tree64(pr); pq = stats_tree64(pq); pv = stats_tree64(pv); pa = stats_tree64(pa);
        double x = lane == STAT_ENV_TICKS ? 1.0 : eo;
        x = lane == STAT_CTL ? (double)n_ctl : x;
        x = lane == STAT_COLLIDED ? (double)n_col : x;
        x = lane == STAT_DONE ? (double)n_done : x;
        x = lane == STAT_SUM_REWARD ? pr : x;
        x = lane == STAT_SUM_REWARD_SQ ? pq : x;
        x = lane == STAT_SUM_V ? pv : x;
        x = lane == STAT_SUM_A ? pa : x;
        if (lane < STAT_N) A.scratch[it * STAT_N + lane] = x;
    }
}

// 2. The groups.  Workgroup (t, g): its waves take the chunks of 64 environments in turn (chunk j to wave j mod waves), a lane
// per environment, tree64 per column, q[j] into LDS; after every STAT_BATCH chunks the first STAT_N threads add their column's
// q[j] in ascending j.  Which wave computed q[j] does not matter: the additions are the ones the definition names.
__global__ __launch_bounds__(1024) void k_stats_groups(const StatsArgs A)
{
    __shared__ double q_s[STAT_BATCH][STAT_N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long long t = blockIdx.x, E = A.n_envs;
    const int g = blockIdx.y;
    const long long chunks = (E + STAT_LANES - 1) / STAT_LANES;
    double s = 0.0;
    for (long long j0 = 0; j0 < chunks; j0 += STAT_BATCH) {
        const int nb = chunks - j0 < STAT_BATCH ? (int)(chunks - j0) : STAT_BATCH;
        for (int j = wave; j < nb; j += nw) {
            const long long e = (j0 + j) * STAT_LANES + lane;
            bool member = e < E;
            if (member) member = A.group ? A.group[e] == g : g == 0;
            const double *row = A.scratch + (t * E + (member ? e : 0)) * STAT_N;
#pragma unroll
            for (int c = 0; c < STAT_N; c++) {
                double m = 0.0;
                if (member) m = row[c];
                m = stats_tree64(m);
                if (lane == 0) q_s[j][c] = m;
            }
        }
        __syncthreads();
        if (threadIdx.x < STAT_N)
            for (int j = 0; j < nb; j++) s = s + q_s[j][threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < STAT_N) A.series[(t * A.n_groups + g) * STAT_N + threadIdx.x] = s;
}

// 3. The totals: one thread per (group, column), ticks ascending.
__global__ __launch_bounds__(1024) void k_stats_totals(const StatsArgs A)
{
    const long long n = (long long)A.n_groups * STAT_N, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = A.totals[i];
    for (long long t = 0; t < A.n_ticks; t++) s = s + A.series[t * n + i];
    A.totals[i] = s;
}

__device__ __forceinline__ long long stats_wave_sum(long long v)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}

// The grouped metrics: one workgroup of STAT_METRIC_THREADS per group.  Per pass of as many environments, a thread per
// environment loads the header's counters (the integer sums stay in the threads until the end) and puts sum_reward / sum_jerk --
// +0.0 for a non-member, which leaves a sum that started at +0.0 as it is -- into LDS; then ONE thread per float sum adds the
// pass's entries in ascending environment order: the serial chain of the definition, which is what bounds the kernel.
constexpr int STAT_METRIC_THREADS = 1024;
__global__ __launch_bounds__(STAT_METRIC_THREADS) void k_stats_metrics(const EnvHeader *hd, int n_envs, int cap, const int32_t *group,
                                                                      int n_groups, double *out)
{
    __shared__ double r_s[STAT_METRIC_THREADS], j_s[STAT_METRIC_THREADS];
    __shared__ long long part_s[STAT_METRIC_THREADS / 64][9];
    const int tid = threadIdx.x, g = blockIdx.x;
    long long c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};        // ticks, alive, ctl, spawned, passed, collided, locks, passed steps, overflow
    double s = 0.0;                                      // thread 0: sum_reward; thread 64 (another wave): sum_jerk
    for (long long e0 = 0; e0 < n_envs; e0 += STAT_METRIC_THREADS) {
        const long long e = e0 + tid;
        bool member = e < n_envs;
        if (member) member = group ? group[e] == g : g == 0;
        double r = 0.0, j = 0.0;
        if (member) {
            const EnvHeader *h = hd + e;
            c[0] += h->ticks; c[1] += h->alive_steps; c[2] += h->ctl_steps; c[3] += h->id_seq; c[4] += h->passed;
            c[5] += h->collided; c[6] += h->locks; c[7] += h->passed_step_total; c[8] += h->overflow;
            r = h->sum_reward; j = h->sum_jerk;
        }
        r_s[tid] = r; j_s[tid] = j;
        __syncthreads();
        const int n = n_envs - e0 < STAT_METRIC_THREADS ? (int)(n_envs - e0) : STAT_METRIC_THREADS;
        if (tid == 0)
            for (int i = 0; i < n; i++) s = s + r_s[i];
        if (tid == 64)
            for (int i = 0; i < n; i++) s = s + j_s[i];
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const long long w = stats_wave_sum(c[k]);
        if ((tid & 63) == 0) part_s[tid >> 6][k] = w;
    }
    if (tid == 64) r_s[0] = s;                           // (r_s is free: the last pass ended with a barrier)
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < 9; k++) {
            c[k] = 0;
            for (int w = 0; w < STAT_METRIC_THREADS / 64; w++) c[k] += part_s[w][k];
        }
        double *o = out + (long long)g * STAT_N_METRICS;
        o[0] = (double)(c[0] * cap); o[1] = (double)c[1]; o[2] = (double)c[2]; o[3] = (double)c[3]; o[4] = (double)c[4];
        o[5] = (double)c[5]; o[6] = (double)c[6]; o[7] = s; o[8] = r_s[0]; o[9] = (double)c[7]; o[10] = (double)c[8];
        o[11] = (double)c[0];
    }
}

#endif  // __HIPCC__

}  // namespace pve

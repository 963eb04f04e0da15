/* pve_env_stats.h -- extension of the C ABI of pve_env.h (libpveenv.so, ABI 9): roll-out and evaluation statistics reduced on
 * the device, by group of environments and by tick.  The specification -- the columns, the selection by flags and THE ORDER of
 * every float64 sum -- is csrc/pve_stats.h; pve_mcc_amd/stats.py restates it in NumPy.  A library older than this header lacks
 * the symbols.
 *
 * What it replaces: the summaries main.py:286-304 writes per tick (`collisions`, v_mean = mean(state_next[:,0,1]), acc_mean =
 * mean(state_next[:,0,2]), the reward mean, the collided-vehicle count), the epoch's collisions_count / id_seq by which
 * main.py:315-328 keeps best.cptk, the np.std(reward) / np.mean(reward) of test() (main.py:413-415) and the one line per density
 * of batch_test() (main.py:543-583). */
#ifndef PVE_ENV_STATS_H
#define PVE_ENV_STATS_H

#include "pve_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Columns of series / totals / the scratch rows.  All are additive over environments and ticks. */
#define PVE_STAT_N 14
enum { PVE_STAT_ENV_TICKS = 0,   /* environments of the group (per tick: the group's size) */
       PVE_STAT_ALIVE,           /* sum of env_out[PVE_EO_N_PRE] */
       PVE_STAT_SPAWNED,         /* ... [PVE_EO_N_SPAWNED] */
       PVE_STAT_FINISHED,        /* ... [PVE_EO_N_FINISHED] */
       PVE_STAT_DELETED,         /* ... [PVE_EO_N_DELETED] */
       PVE_STAT_COLLISIONS,      /* ... [PVE_EO_COLLISIONS]: `collisions` of the 9-tuple (ref :337, main.py:287) */
       PVE_STAT_LOCK,            /* ... [PVE_EO_LOCK] */
       PVE_STAT_CTL,             /* slots with PVE_F_CTL (= len(ids)) */
       PVE_STAT_COLLIDED,        /* slots with PVE_F_CTL and (flags >> 8) > 0 (main.py:276-278 / :410-412; PVE_M_COLLIDED) */
       PVE_STAT_DONE,            /* slots with PVE_F_CTL and PVE_F_DONE */
       PVE_STAT_SUM_REWARD,      /* over PVE_F_CTL slots: reward */
       PVE_STAT_SUM_REWARD_SQ,   /* ... reward * reward, rounded once */
       PVE_STAT_SUM_V,           /* ... obs_pre[..][1] (main.py:290); 0 without obs_pre */
       PVE_STAT_SUM_A };         /* ... obs_pre[..][2] (main.py:294); 0 without obs_pre */
#define PVE_STAT_MAX_GROUPS 1024

/* One call of pve_rollout_stats.  Every pointer is DEVICE memory, aligned to its element type.  The blocks are those of
 * pve_outputs retained over n_ticks ticks ([n_ticks][n_envs]...; n_ticks = 1: the single-tick buffers themselves). */
typedef struct pve_stats {
    int32_t n_ticks;          /* >= 1 */
    int32_t n_groups;         /* 1 .. PVE_STAT_MAX_GROUPS; 1 when group is NULL */
    int32_t block_threads;    /* 0 (default) or a multiple of 64 up to 1024: launch shape only, never results */
    int32_t reserved;         /* 0 */
    const int32_t *group;     /* [n_envs], values in [0, n_groups), or NULL = one group.  An id outside the range cannot be
                                 checked without a wait: such an environment is counted in no group. */
    const int32_t *flags;     /* [n_ticks][n_envs][cap] */
    const double *reward;     /* [n_ticks][n_envs][cap] */
    const void *obs_pre;      /* [n_ticks][n_envs][cap][28], float64 or float32 by PVE_CFG_OBS_F32, or NULL */
    const int32_t *env_out;   /* [n_ticks][n_envs][PVE_ENV_OUT_N] */
    double *series;           /* out: [n_ticks][n_groups][PVE_STAT_N] */
    double *totals;           /* in/out or NULL: [n_groups][PVE_STAT_N]; series[t] is added to it for t ascending */
    void *scratch;            /* pve_stats_scratch_bytes(n_envs, n_ticks) bytes, 8-byte aligned: the per-(tick, env) rows
                                 [n_ticks][n_envs][PVE_STAT_N] float64, defined and readable after the call */
} pve_stats;

/* Bytes of pve_stats.scratch (0 for non-positive arguments). */
size_t pve_stats_scratch_bytes(int n_envs, int n_ticks);

/* series (and totals) of the retained blocks.  Asynchronous on the handle's stream; reads nothing back; writes only series,
 * totals and scratch.  Slots are selected by their flags word, never multiplied by a mask: unspecified values of dead or
 * uncontrolled slots (NaN patterns included) do not reach a sum.
 * Errors (PVE_ERR_INVALID): null handle / descriptor / flags / reward / env_out / series / scratch; n_ticks < 1; n_groups outside
 * 1 .. PVE_STAT_MAX_GROUPS or not 1 with group NULL; block_threads not 0 or a multiple of 64 up to 1024; reserved not 0; a
 * misaligned block; a backend without the statistics kernels. */
int pve_rollout_stats(pve_handle h, const pve_stats *st);

/* The twelve sums of pve_get_metrics per group, read from the per-environment headers on the device into out[n_groups]
 * [PVE_N_METRICS] (DEVICE memory, float64) on the handle's stream: no host copy, no wait.  With one group the result equals
 * pve_get_metrics bit for bit (sum_reward / sum_jerk are added in ascending environment index, as there).
 * Errors (PVE_ERR_INVALID): null handle / out; n_groups as above; misaligned group / out; a backend without the kernels. */
int pve_metrics_groups(pve_handle h, const int32_t *group /* [n_envs] or NULL */, int n_groups, double *out);

#ifdef __cplusplus
}
#endif
#endif /* PVE_ENV_STATS_H */

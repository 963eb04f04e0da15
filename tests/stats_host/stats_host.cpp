// Host shim of csrc/pve_stats.h for the CPU tests (tests/test_rollout_stats.py): the header's own loops compiled by g++, behind
// a C interface.  Test infrastructure only.
#include <stddef.h>
#include <stdint.h>

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_stats.h"

extern "C" {

// blocks as pve_rollout_stats takes them; scratch [n_ticks][n_envs][14]; series [n_ticks][n_groups][14]; totals [n_groups][14] or null
void stats_rollout_host(int n_envs, int cap, int n_ticks, int n_groups, int obs_f32, const int32_t *group, const int32_t *flags,
                        const double *reward, const void *obs_pre, const int32_t *env_out, double *series, double *totals, double *scratch)
{
    pve::StatsArgs A;
    A.n_envs = n_envs; A.cap = cap; A.n_ticks = n_ticks; A.n_groups = n_groups; A.obs_f32 = obs_f32; A.group = group; A.flags = flags;
    A.reward = reward; A.obs_pre = obs_pre; A.env_out = env_out; A.series = series; A.totals = totals; A.scratch = scratch;
    pve::rollout_stats_host(A);
}

// headers: n_envs EnvHeaders as they lie in a handle's workspace; out [n_groups][12]
void stats_metrics_groups_host(const void *headers, int n_envs, int cap, const int32_t *group, int n_groups, double *out)
{
    pve::metrics_groups_host((const pve::EnvHeader *)headers, n_envs, cap, group, n_groups, out);
}

int stats_header_bytes(void) { return (int)sizeof(pve::EnvHeader); }

size_t stats_scratch_bytes_host(long long n_envs, long long n_ticks) { return pve::stats_scratch_bytes(n_envs, n_ticks); }

}  // extern "C"

// Host shim of csrc/pve_nstep.h for the CPU tests (tests/test_nstep.py): the header's own nstep_window, compiled by g++, run
// over every candidate start, behind a C interface.  Test infrastructure only.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_nstep.h"

extern "C" {

// target / code: [min(n_prev, window - 1) + n_cur][n_envs][cap]; returns the number of transitions
long long nstep_scan_host(double gamma, int window, int mode, int n_envs, int cap, int obs_f32,
                          int n_prev, const void *p_obs, const double *p_reward, const int32_t *p_flags, const int32_t *p_new_slot,
                          int n_cur, const void *c_obs, const double *c_reward, const int32_t *c_flags, const int32_t *c_new_slot,
                          const void *obs_first, const float *q, double *target, int32_t *code)
{
    pve::NstepArgs A;
    memset(&A, 0, sizeof(A));
    A.gamma = gamma; A.window = window; A.mode = mode; A.n_envs = n_envs; A.cap = cap; A.obs_f32 = obs_f32;
    A.n_back = n_prev < window - 1 ? n_prev : window - 1;
    A.prev.n_ticks = n_prev; A.prev.obs_post = p_obs; A.prev.reward = p_reward; A.prev.flags = p_flags; A.prev.new_slot = p_new_slot;
    A.cur.n_ticks = n_cur; A.cur.obs_post = c_obs; A.cur.reward = c_reward; A.cur.flags = c_flags; A.cur.new_slot = c_new_slot;
    A.obs_first = obs_first; A.q_boot = q;
    long long total = 0, g = 0;
    for (int tc = 0; tc < A.n_back + n_cur; tc++)
        for (int env = 0; env < n_envs; env++)
            for (int slot = 0; slot < cap; slot++, g++) {
                code[g] = pve::nstep_window(A, tc - A.n_back, env, slot, target[g]);
                total += code[g] != 0;
            }
    return total;
}

}  // extern "C"

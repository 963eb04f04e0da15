// Host shim of csrc/pve_arrivals.h for the CPU tests (tests/test_arrivals_device.py): the header's own generator loop and its
// exponential deviate compiled by g++, behind a C interface.  Test infrastructure only.
#include <stddef.h>
#include <stdint.h>

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_arrivals.h"

extern "C" {

// arrivals [n_envs][rows][lane_num]; intentions [n_envs][rows][lane_num] or null; covered [n_envs] or null; mean_env or null
void arrivals_generate_host(uint64_t seed, long long env_offset, uint32_t epoch, int rows, int n_envs, int lane_num, double mean,
                            const double *mean_env, double min_gap, double *arrivals, int32_t *intentions, double *covered)
{
    pve::ArrivalArgs A;
    A.seed = seed; A.env_offset = env_offset; A.epoch = epoch; A.rows = rows; A.n_envs = n_envs; A.lane_num = lane_num;
    A.mean = mean; A.mean_env = mean_env; A.min_gap = min_gap; A.arrivals = arrivals; A.intentions = intentions; A.covered = covered;
    pve::arrivals_generate_host(A);
}

void arrival_exp_host(const uint32_t *w, long long n, double *x)
{
    for (long long i = 0; i < n; i++) x[i] = pve::arrival_exp(w[i]);
}

}  // extern "C"

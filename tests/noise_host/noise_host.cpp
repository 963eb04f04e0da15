// Host shim of csrc/pve_noise.h for the CPU tests (tests/test_action_noise.py): the header's own functions, compiled by g++,
// behind a C interface.  Test infrastructure only.
#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_noise.h"

extern "C" {

void noise_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
    pve::philox4x32_10(c, key[0], key[1]);
    for (int k = 0; k < 4; k++) out[k] = c[k];
}

void noise_gauss_many(const uint32_t *w0, const uint32_t *w1, double *out, long long n)
{
    for (long long i = 0; i < n; i++) out[i] = pve::noise_gauss(w0[i], w1[i]);
}

void noise_z_many(uint64_t seed, const int64_t *env_global, const int32_t *vehicle_id, const uint32_t *tick, double *out, long long n)
{
    for (long long i = 0; i < n; i++) out[i] = pve::action_noise_z(seed, env_global[i], vehicle_id[i], tick[i]);
}

double noise_apply(double a, double sigma, uint64_t seed, int64_t env_global, int32_t vehicle_id, uint32_t tick)
{
    pve::ActionNoise nz = {sigma, seed, 0, 0, 0};
    return pve::action_with_noise(a, nz, env_global, vehicle_id, tick);
}

}  // extern "C"

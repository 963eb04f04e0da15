// Host shim of csrc/pve_replay.h for the CPU tests (tests/test_replay.py): the header's own replay_perm and append plan, compiled
// by g++, behind a C interface.  Test infrastructure only.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_replay.h"

extern "C" {

int replay_half_bits_host(uint32_t N) { return pve::replay_half_bits(N); }

// out[i] = perm(seed, d[i], N)(j[i])
void replay_perm_host(uint64_t seed, const uint64_t *d, uint32_t N, const uint32_t *j, long long n, uint32_t *out)
{
    for (long long i = 0; i < n; i++) out[i] = pve::replay_perm(seed, d[i], N, j[i]);
}

// One append of n_max input records (total < 0 with has_total = 0: no device-side count): slot[i] = the ring slot input record i
// is stored in, -1 for a record that is not stored.  Returns the number of records accepted (what `written` grows by).
long long replay_append_host(long long written, int has_total, long long total, long long n_max, long long capacity, long long *slot)
{
    const pve::ReplayPlan P = pve::replay_append_plan(written, has_total != 0, total, n_max, capacity);
    for (long long i = 0; i < n_max; i++) slot[i] = -1;
    for (long long q = 0; q < P.n - P.skip; q++) slot[P.skip + q] = pve::replay_append_slot(P, capacity, q);
    return P.n;
}

}  // extern "C"

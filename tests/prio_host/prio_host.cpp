// Host shim of csrc/pve_prio.h for the CPU tests (tests/test_prio_replay.py): the header's own key, partition lookup, draw,
// weight and update rule compiled by g++, behind a C interface; the ranking is the header's key under a plain stable sort.
// Test infrastructure only.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_prio.h"

extern "C" {

unsigned long long prio_scratch_bytes_host(long long capacity) { return (unsigned long long)pve::prio_scratch_bytes(capacity); }

int prio_partition_host(const long long *part_from, long long L)
{
    long long pf[pve::PRIO_PARTS];
    for (int i = 0; i < pve::PRIO_PARTS; i++) pf[i] = part_from[i];
    return pve::prio_partition(pf, L);
}

// order[r] = age index of the record of rank r + 1; returns L
long long prio_rank_host(long long written, long long capacity, const uint32_t *prio, const long long *pseq, int32_t *order)
{
    const long long L = pve::replay_live(written, capacity);
    std::vector<uint32_t> key((size_t)L);
    std::vector<int32_t> at((size_t)L);
    for (long long i = 0; i < L; i++) {                     // position i = age L - 1 - i: newest first, as k_prio_keys lays them out
        const long long a = L - 1 - i, w = written - L + a, s = w % capacity;
        key[(size_t)i] = pve::prio_key(pseq[s] == w, prio[s]);
        at[(size_t)i] = (int32_t)i;
    }
    std::stable_sort(at.begin(), at.end(), [&](int32_t x, int32_t y) { return key[(size_t)x] < key[(size_t)y]; });
    for (long long r = 0; r < L; r++) order[r] = (int32_t)(L - 1 - at[(size_t)r]);
    return L;
}

// rank[m][j] of minibatches d0 .. d0 + n_batches - 1 from one table row, weight[m][j] with the minibatch's largest rank
void prio_draw_host(const int32_t *ends_row, long long batch, uint64_t seed, uint64_t d0, long long n_batches, long long L, float alpha_beta,
                    int32_t *rank, float *weight)
{
    for (long long m = 0; m < n_batches; m++) {
        int32_t top = 1;
        for (long long j = 0; j < batch; j++) {
            rank[m * batch + j] = pve::prio_draw_rank(ends_row, seed, d0 + (uint64_t)m, (uint32_t)j, L);
            top = std::max(top, rank[m * batch + j]);
        }
        for (long long j = 0; j < batch; j++) weight[m * batch + j] = pve::prio_weight(rank[m * batch + j], top, alpha_beta);
    }
}

// the two passes of the update; returns the ids ignored
long long prio_update_host(long long written, long long capacity, uint32_t *prio, long long *pseq, const long long *seq, const float *q,
                           const float *target, long long n)
{
    long long ignored = 0;
    for (long long i = 0; i < n; i++) {
        const long long s = pve::prio_update_slot(seq[i], written, capacity);
        if (s >= 0) { pseq[s] = seq[i]; prio[s] = 0u; }
    }
    for (long long i = 0; i < n; i++) {
        const long long s = pve::prio_update_slot(seq[i], written, capacity);
        if (s < 0) { ignored++; continue; }
        prio[s] = std::max(prio[s], pve::prio_update_bits(q[i], target != nullptr, target ? target[i] : 0.0f));
    }
    return ignored;
}

}  // extern "C"

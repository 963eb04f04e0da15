// Host build of the wide learner step of csrc/pve_learn.h for the tests (tests/test_learner_wide.py,
// tests/test_gpu_learner_wide.py): the header's own learn_steps_wide, compiled by g++ and run by the sequential executor, behind
// a C interface.  The workspace of the latest call is kept so that the tests can read the per-slice partial rows.  Test
// infrastructure only.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_learn.h"

static std::vector<float> g_work;       // the partial rows of the latest step of the latest call
static int g_slices = 0;

extern "C" {

// the constants the tests compare with include/pve_env.h and the Python binding
void learner_wide_host_layout(int32_t *out /* [8] */)
{
    const int v[8] = {pve::LEARN_SLICE, pve::LW_ROW, pve::LW_CRITIC, pve::LW_ACTOR, pve::LW_LOSS, pve::LEARN_SUB_1, pve::LEARN_SUB_2, 0};
    for (int k = 0; k < 8; k++) out[k] = v[k];
}

// pve_learner_step_wide on a host block; hyper = {actor_lr, critic_lr, beta1, beta2, epsilon, tau}.  The workspace starts as NaN:
// a float read before it is written would show in the result.
void learner_wide_host_step(float *P, const float *hyper, int flags, const float *rows, const float *act7, const float *target, int batch,
                            int n_batches, float *losses, float *grads)
{
    std::vector<float> tape(pve::LEARN_TAPE), S(pve::LEARN_SCALARS);
    g_slices = pve::learn_n_slices(batch);
    uint32_t nan_bits = 0x7fc00000u;
    float nan;
    memcpy(&nan, &nan_bits, 4);
    g_work.assign((size_t)g_slices * pve::LW_ROW, nan);
    pve::LearnCtx C;
    memset(&C, 0, sizeof(C));
    C.P = P; C.tape = tape.data(); C.S = S.data();
    C.rows = rows; C.act7 = act7; C.target = target; C.losses = losses; C.grads = grads; C.batch = batch; C.n_batches = n_batches;
    C.H.actor_lr = hyper[0]; C.H.critic_lr = hyper[1]; C.H.beta1 = hyper[2]; C.H.beta2 = hyper[3]; C.H.epsilon = hyper[4]; C.H.tau = hyper[5];
    C.H.flags = flags;
    pve::learn_steps_wide(pve::LearnSeq(), C, g_work.data());
}

// the per-slice partial rows of the latest step: -> the number of slices; out [n_slices][LW_ROW] (or null to ask for the count)
int learner_wide_host_partials(float *out)
{
    if (out) memcpy(out, g_work.data(), sizeof(float) * g_work.size());
    return g_slices;
}

}  // extern "C"

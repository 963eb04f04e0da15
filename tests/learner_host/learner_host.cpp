// Host build of csrc/pve_learn.h for the tests (tests/test_learner.py, tests/test_gpu_learner.py): the header's own learn_steps,
// compiled by g++ and run by the sequential executor, behind a C interface.  Test infrastructure only.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_learn.h"

extern "C" {

// the layout constants the tests compare with include/pve_env.h and the Python binding
void learner_host_layout(int32_t *out /* [16] */)
{
    const int v[16] = {pve::LB_ACTOR, pve::LB_CRITIC, pve::LB_TACTOR, pve::LB_TCRITIC, pve::LB_M_ACTOR, pve::LB_V_ACTOR, pve::LB_M_CRITIC,
                       pve::LB_V_CRITIC, pve::LB_POWERS, pve::LB_STEPS, pve::LB_GRAD, pve::LB_TOTAL, pve::LRN_ACTOR_W, pve::LRN_CRITIC_W,
                       pve::LEARN_SUB_1, pve::LEARN_SUB_2};
    for (int k = 0; k < 16; k++) out[k] = v[k];
}

// pve_learner_init on a host block
void learner_host_init(float *P, const float *actor, const float *critic, const float *tactor, const float *tcritic, float beta1, float beta2)
{
    memset(P, 0, sizeof(float) * pve::LB_TOTAL);
    memcpy(P + pve::LB_ACTOR, actor, sizeof(float) * pve::LRN_ACTOR_W);
    memcpy(P + pve::LB_CRITIC, critic, sizeof(float) * pve::LRN_CRITIC_W);
    memcpy(P + pve::LB_TACTOR, tactor ? tactor : actor, sizeof(float) * pve::LRN_ACTOR_W);
    memcpy(P + pve::LB_TCRITIC, tcritic ? tcritic : critic, sizeof(float) * pve::LRN_CRITIC_W);
    P[pve::LB_POWERS] = beta1; P[pve::LB_POWERS + 1] = beta2; P[pve::LB_POWERS + 2] = beta1; P[pve::LB_POWERS + 3] = beta2;
}

// pve_learner_step on a host block; hyper = {actor_lr, critic_lr, beta1, beta2, epsilon, tau}
void learner_host_step(float *P, const float *hyper, int flags, const float *rows, const float *act7, const float *target, int batch,
                       int n_batches, float *losses, float *grads)
{
    std::vector<float> tape(pve::LEARN_TAPE), S(pve::LEARN_SCALARS);
    pve::LearnCtx C;
    memset(&C, 0, sizeof(C));
    C.P = P; C.tape = tape.data(); C.S = S.data();
    C.rows = rows; C.act7 = act7; C.target = target; C.losses = losses; C.grads = grads; C.batch = batch; C.n_batches = n_batches;
    C.H.actor_lr = hyper[0]; C.H.critic_lr = hyper[1]; C.H.beta1 = hyper[2]; C.H.beta2 = hyper[3]; C.H.epsilon = hyper[4]; C.H.tau = hyper[5];
    C.H.flags = flags;
    pve::learn_steps(pve::LearnSeq(), C);
}

void learner_host_tanh3(const float *z, long long n, float *out, float *dout)
{
    for (long long i = 0; i < n; i++) { out[i] = pve::learn_tanh3(z[i]); dout[i] = pve::learn_dtanh3(out[i]); }
}

}  // extern "C"

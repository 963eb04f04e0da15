// pve_learn.h -- the MADDPG learner step (reference main.py:48-84 `train_agent_seq`: model_agent_maddpg.py:85-118 `train_critic`,
// `train_actor`, then main.py:19-33 the two soft target updates) as ONE statement in plain float32 C++ that g++ and hipcc both
// compile.  learn_steps<Exec> below IS the step: the host build (tests/learner_host) runs it with LearnSeq, a sequential loop;
// k_learner_step (pve_hip.hip) runs the same function with the work items of every phase dealt to the threads of one workgroup.
// The kernel is held to the host build bit for bit.
//
// ARITHMETIC.  Only + - * /, fmaf, sqrtf and comparisons; the library builds with -ffp-contract=off, every fused multiply-add is
// written out.  Every operation is correctly rounded on both sides, so equal order means equal bits.
// 3 tanh(z) is learn_tanh3 below: a rational function of these operations alone.  (actor_tanh3 of pve_actor.h is built on the
// device's exp2 and reciprocal approximations; it exists on the device only and cannot be held to a host build.)
//
// ORDERS (none depends on the launch geometry, the sub-block size or the number of threads):
//   dense, forward      acc = bias[u]; k = 0 .. K-1 ascending: acc = fmaf(W[k][u], x[k], acc)       (critic dense_1: K = 71,
//                       hidden units 0 .. 63, then own action, then the six other actions)
//   dense 64 -> 1       acc = b3; k = 0 .. 63: acc = fmaf(y2[k], W3[k], acc)
//   LayerNorm           mean = (sum x[k], k ascending from 0.f) / n;  var = (acc = fmaf(d, d, acc), d = x[k] - mean) / n;
//                       rstd = 1 / sqrtf(var + 1e-12f);  xh[k] = (x[k] - mean) * rstd;  y[k] = fmaf(xh[k], gamma[k], beta[k])
//   ReLU                y > 0 ? y : 0;  backward passes dy only where the output is > 0 (an output of exactly 0 passes nothing)
//   dense, backward dX  acc = 0; u = 0 .. 63 ascending: acc = fmaf(W[k][u], dh[u], acc)
//   LayerNorm, backward dxh[k] = dy[k] * gamma[k];  m1 = (sum dxh[k] from 0.f) / n;  m2 = (acc = fmaf(dxh[k], xh[k], acc)) / n;
//                       dx[k] = rstd * ((dxh[k] - m1) - xh[k] * m2)
//   every gradient of a parameter is acc = 0; b = 0 .. batch-1 ascending: acc = fmaf(A[b], B[b], acc) with the pair (A, B) of
//   learn_grad_src (A = 1 for biases and betas); the losses sum over b in the same way.
//   THE WIDE STEP (learn_steps_wide; pve_learner_step_wide) cuts a batch of B rows into ceil(B / 128) slices, slice s = rows
//   128 s .. min(B, 128 s + 128) - 1 (LEARN_SLICE).  Within a slice every chain above starts from 0 at the slice's first row and
//   runs as in learn_steps; dQ stays 2 (Q - target) / (float)B and -1 / (float)B with the whole batch B.  Then, per parameter and
//   for each of the two loss sums: acc = partial[0]; s = 1 .. n_slices - 1 ascending: acc = acc + partial[s], plain float32 adds;
//   the loss sums are divided by (float)B behind that.  For B <= 128 this IS learn_steps, bit for bit; for B > 128 it is another
//   order, as fixed as the first: it depends on B alone, not on the grid, the threads or the sub-block sizes.
//
// ADAM as tf.train.AdamOptimizer applies it (TF 1.x ApplyAdam, written from memory of TensorFlow -- this header is the project's
// definition): alpha = lr * sqrtf(1 - b2p) / (1 - b1p);  m += (g - m) * (1 - beta1);  v += (g * g - v) * (1 - beta2);
// w -= (m * alpha) / (sqrtf(v) + epsilon);  afterwards b1p *= beta1, b2p *= beta2 (the powers start at beta1, beta2).
// SOFT UPDATE (main.py:30): target = c1 * online + c2 * target, c1 = float32(1.0 - (double)tau), c2 = float32(tau), the two
// products rounded separately.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "pve_types.h"

namespace pve {

constexpr int LRN_IN = 28, LRN_H = 64, LRN_ACT = 7;
constexpr int LRN_ACTOR_W = 6393, LRN_CRITIC_W = 6841;            // PVE_ACTOR_N_WEIGHTS, PVE_CRITIC_N_WEIGHTS
constexpr int LRN_GRADS = LRN_CRITIC_W + LRN_ACTOR_W;             // one row of `grads`: critic, then actor
// the caller's parameter block (float32 offsets; include/pve_env.h PVE_LEARNER_*): every segment starts 16-byte aligned
constexpr int lrn_pad4(int n) { return (n + 3) / 4 * 4; }
constexpr int LB_ACTOR = 0, LB_CRITIC = LB_ACTOR + lrn_pad4(LRN_ACTOR_W), LB_TACTOR = LB_CRITIC + lrn_pad4(LRN_CRITIC_W),
              LB_TCRITIC = LB_TACTOR + lrn_pad4(LRN_ACTOR_W), LB_M_ACTOR = LB_TCRITIC + lrn_pad4(LRN_CRITIC_W),
              LB_V_ACTOR = LB_M_ACTOR + lrn_pad4(LRN_ACTOR_W), LB_M_CRITIC = LB_V_ACTOR + lrn_pad4(LRN_ACTOR_W),
              LB_V_CRITIC = LB_M_CRITIC + lrn_pad4(LRN_CRITIC_W),
              LB_POWERS = LB_V_CRITIC + lrn_pad4(LRN_CRITIC_W),   // beta1^t, beta2^t of the actor's optimizer, then of the critic's
              LB_STEPS = LB_POWERS + 4,                           // int32: steps taken (then 3 reserved words)
              LB_GRAD = LB_STEPS + 4,                             // the gradients of the latest step: critic, then (padded) actor
              LB_TOTAL = LB_GRAD + lrn_pad4(LRN_CRITIC_W) + lrn_pad4(LRN_ACTOR_W);
constexpr int LEARN_CRITIC_ONLY = 1;                              // PVE_LEARN_CRITIC_ONLY

// A network's flat float32 layout (pve_set_actor / pve_set_target_networks): K2 = 64 (actor) or 71 (critic) rows in dense_1
struct LearnNet {
    int k2, ln0g, ln0b, w1, b1, ln1g, ln1b, w2, b2, ln2g, ln2b, w3, b3, total;
};
PVE_HD LearnNet learn_net(bool critic)
{
    LearnNet N;
    N.k2 = critic ? LRN_H + LRN_ACT : LRN_H;
    N.ln0g = 0; N.ln0b = N.ln0g + LRN_IN; N.w1 = N.ln0b + LRN_IN; N.b1 = N.w1 + LRN_IN * LRN_H; N.ln1g = N.b1 + LRN_H;
    N.ln1b = N.ln1g + LRN_H; N.w2 = N.ln1b + LRN_H; N.b2 = N.w2 + N.k2 * LRN_H; N.ln2g = N.b2 + LRN_H; N.ln2b = N.ln2g + LRN_H;
    N.w3 = N.ln2b + LRN_H; N.b3 = N.w3 + LRN_H; N.total = N.b3 + 1;
    return N;
}

// The tape of one row and one network (float32 offsets).  T_Y1 and T_ACT are adjacent: together the 71 inputs of the critic's dense_1.
constexpr int T_XH0 = 0, T_A0 = T_XH0 + LRN_IN, T_DA0 = T_A0 + LRN_IN, T_X1 = T_DA0 + LRN_IN /* h1, then its normalised form */,
              T_Y1 = T_X1 + LRN_H, T_ACT = T_Y1 + LRN_H, T_X2 = T_ACT + LRN_ACT + 1, T_Y2 = T_X2 + LRN_H, T_DLN2 = T_Y2 + LRN_H,
              T_DH2 = T_DLN2 + LRN_H, T_DLN1 = T_DH2 + LRN_H, T_DH1 = T_DLN1 + LRN_H, T_RSTD1 = T_DH1 + LRN_H, T_RSTD2 = T_RSTD1 + 1,
              T_OUT = T_RSTD2 + 1 /* Q, or the action 3 tanh(z) */, T_DOUT = T_OUT + 1 /* d loss / d (dense_2 output) */,
              T_ONE = T_DOUT + 1 /* 1.0f: the A of biases and betas */, T_M1 = T_ONE + 1, T_M2 = T_M1 + 1, T_TGT = T_M2 + 1,
              T_NET = T_TGT + 1;
constexpr int LEARN_STRIDE_1 = T_NET | 1, LEARN_STRIDE_2 = (2 * T_NET) | 1;       // odd row strides: rows fall into different LDS banks
// rows per sub-block: critic step, actor step.  No result depends on them (every sum over the batch continues across sub-blocks
// in its one order); the defaults fill one workgroup's LDS, and tests/learner_host builds the header a second time with other values.
#ifndef PVE_LEARN_SUB_1
#define PVE_LEARN_SUB_1 64
#endif
#ifndef PVE_LEARN_SUB_2
#define PVE_LEARN_SUB_2 32
#endif
constexpr int LEARN_SUB_1 = PVE_LEARN_SUB_1, LEARN_SUB_2 = PVE_LEARN_SUB_2;
constexpr int LEARN_TAPE = LEARN_SUB_1 * LEARN_STRIDE_1 > LEARN_SUB_2 * LEARN_STRIDE_2 ? LEARN_SUB_1 * LEARN_STRIDE_1
                                                                                      : LEARN_SUB_2 * LEARN_STRIDE_2;
constexpr int LEARN_SCALARS = 8;                                  // S_*: the running sums of a step
constexpr int S_LOSS_C = 0, S_LOSS_A = 1;

// 3 tanh(z) from + - * / and fmaf: z clamped to [-9, 9], then the odd rational z P(z^2) / Q(z^2) of degree 13 / 6 that Eigen and
// XLA use for float32 tanh (public coefficients), Horner from the highest power, the quotient clamped to [-1, 1].  Within 4e-7 of tanh,
// relative; odd; not monotone to the last bit where it saturates (tests/test_learner.py).
PVE_HD float learn_tanh3(float z)
{
    const float x = z > 9.0f ? 9.0f : (z < -9.0f ? -9.0f : z);
    const float x2 = x * x;
    float p = -2.76076847742355e-16f;
    p = fmaf(p, x2, 2.00018790482477e-13f);
    p = fmaf(p, x2, -8.60467152213735e-11f);
    p = fmaf(p, x2, 5.12229709037114e-08f);
    p = fmaf(p, x2, 1.48572235717979e-05f);
    p = fmaf(p, x2, 6.37261928875436e-04f);
    p = fmaf(p, x2, 4.89352455891786e-03f);
    p = p * x;
    float q = 1.19825839466702e-06f;
    q = fmaf(q, x2, 1.18534705686654e-04f);
    q = fmaf(q, x2, 2.26843463243900e-03f);
    q = fmaf(q, x2, 4.89352518554385e-03f);
    const float t = p / q;                                         // (rounding can leave it an ulp or two outside [-1, 1])
    return 3.0f * (t > 1.0f ? 1.0f : (t < -1.0f ? -1.0f : t));
}
// d (3 tanh z) / dz from the forward value a = 3 tanh z
PVE_HD float learn_dtanh3(float a)
{
    const float t = a / 3.0f;
    return 3.0f * (1.0f - t * t);
}

// Gradient of parameter w of a network: sum over the batch of tape[A] * tape[B]
PVE_HD void learn_grad_src(const LearnNet &N, int w, int &A, int &B)
{
    if (w < N.ln0b) { A = T_XH0 + w; B = T_DA0 + w; }
    else if (w < N.w1) { A = T_ONE; B = T_DA0 + (w - N.ln0b); }
    else if (w < N.b1) { const int i = w - N.w1; A = T_A0 + i / LRN_H; B = T_DH1 + i % LRN_H; }
    else if (w < N.ln1g) { A = T_ONE; B = T_DH1 + (w - N.b1); }
    else if (w < N.ln1b) { A = T_X1 + (w - N.ln1g); B = T_DLN1 + (w - N.ln1g); }
    else if (w < N.w2) { A = T_ONE; B = T_DLN1 + (w - N.ln1b); }
    else if (w < N.b2) { const int i = w - N.w2; A = T_Y1 + i / LRN_H; B = T_DH2 + i % LRN_H; }
    else if (w < N.ln2g) { A = T_ONE; B = T_DH2 + (w - N.b2); }
    else if (w < N.ln2b) { A = T_X2 + (w - N.ln2g); B = T_DLN2 + (w - N.ln2g); }
    else if (w < N.w3) { A = T_ONE; B = T_DLN2 + (w - N.ln2b); }
    else if (w < N.b3) { A = T_Y2 + (w - N.w3); B = T_DOUT; }
    else { A = T_ONE; B = T_DOUT; }
}

struct LearnHyper {
    float actor_lr, critic_lr, beta1, beta2, epsilon, tau;
    int flags;
};

// What one call works on.  tape: LEARN_TAPE floats, S: LEARN_SCALARS floats (LDS on the device).
struct LearnCtx {
    float *P;                                  // the parameter block
    float *tape, *S;
    const float *rows, *act7, *target;         // [n_batches][batch][28], [..][7], [..]
    float *losses, *grads;                     // [n_batches][2], [n_batches][LRN_GRADS], or null
    int batch, n_batches;
    LearnHyper H;
};

// The sequential executor of the host build: phase after phase, item after item
struct LearnSeq {
    template <class F> void forall(int n, F f) const { for (int i = 0; i < n; i++) f(i); }
};

// The base of a weight vector inside a work item.  On the device the empty statement keeps the compiler from forming the address of
// every weight tensor once per launch and parking each in a scalar register pair across the whole step (they do not all fit).
PVE_HD const float *learn_base(const float *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(p));
#endif
    return p;
}

// ---- forward of `n` rows (tape rows at T, stride ts) through network N with weights W.  The rows' 28 features are read from
// x (row-major), the 7 actions of the critic must be in T_ACT already.  Leaves T_OUT (before the tanh for the actor: see caller).
template <class Exec> PVE_HD void learn_forward(const Exec &E, const LearnNet N, const float *W, float *T, int ts, const float *x, int n)
{
    E.forall(n, [=](int b) {                                       // LayerNorm over the 28 inputs
            const float *Wq = learn_base(W);
        float *t = T + b * ts;
        const float *xr = x + (size_t)b * LRN_IN;
        float s = 0.f;
        for (int k = 0; k < LRN_IN; k++) s += xr[k];
        const float mean = s / (float)LRN_IN;
        float e = 0.f;
        for (int k = 0; k < LRN_IN; k++) { const float d = xr[k] - mean; e = fmaf(d, d, e); }
        const float rstd = 1.0f / sqrtf(e / (float)LRN_IN + 1e-12f);
        for (int k = 0; k < LRN_IN; k++) {
            const float xh = (xr[k] - mean) * rstd;
            t[T_XH0 + k] = xh;
            t[T_A0 + k] = fmaf(xh, Wq[N.ln0g + k], Wq[N.ln0b + k]);
        }
        t[T_ONE] = 1.0f;
    });
    for (int layer = 1; layer <= 2; layer++) {
        const int K = layer == 1 ? LRN_IN : N.k2, wo = layer == 1 ? N.w1 : N.w2, bo = layer == 1 ? N.b1 : N.b2;
        const int in = layer == 1 ? T_A0 : T_Y1, h = layer == 1 ? T_X1 : T_X2, y = layer == 1 ? T_Y1 : T_Y2;
        const int go = layer == 1 ? N.ln1g : N.ln2g, beo = layer == 1 ? N.ln1b : N.ln2b, rs = layer == 1 ? T_RSTD1 : T_RSTD2;
        E.forall(n * LRN_H, [=](int i) {                           // dense
            const float *Wq = learn_base(W);
            const int b = i / LRN_H, u = i % LRN_H;
            float *t = T + b * ts;
            float acc = Wq[bo + u];
            for (int k = 0; k < K; k++) acc = fmaf(Wq[wo + k * LRN_H + u], t[in + k], acc);
            t[h + u] = acc;
        });
        E.forall(n, [=](int b) {                                   // LayerNorm statistics
            float *t = T + b * ts;
            float s = 0.f;
            for (int k = 0; k < LRN_H; k++) s += t[h + k];
            const float mean = s / (float)LRN_H;
            float e = 0.f;
            for (int k = 0; k < LRN_H; k++) { const float d = t[h + k] - mean; e = fmaf(d, d, e); }
            t[T_M1] = mean;
            t[rs] = 1.0f / sqrtf(e / (float)LRN_H + 1e-12f);
        });
        E.forall(n * LRN_H, [=](int i) {                           // normalise, scale, ReLU
            const float *Wq = learn_base(W);
            const int b = i / LRN_H, u = i % LRN_H;
            float *t = T + b * ts;
            const float xh = (t[h + u] - t[T_M1]) * t[rs];
            const float v = fmaf(xh, Wq[go + u], Wq[beo + u]);
            t[h + u] = xh;
            t[y + u] = v > 0.f ? v : 0.f;
        });
    }
    E.forall(n, [=](int b) {                                       // dense 64 -> 1
            const float *Wq = learn_base(W);
        float *t = T + b * ts;
        float acc = Wq[N.b3];
        for (int k = 0; k < LRN_H; k++) acc = fmaf(t[T_Y2 + k], Wq[N.w3 + k], acc);
        t[T_OUT] = acc;
    });
}

// ---- backward of `n` rows from T_DOUT.  to_input = false stops behind dense_1's dX (the critic under the actor loss: only
// d Q / d (own action) is needed, left in T_M1); true runs down to T_DA0.
template <class Exec> PVE_HD void learn_backward(const Exec &E, const LearnNet N, const float *W, float *T, int ts, int n, bool to_input)
{
    E.forall(n * LRN_H, [=](int i) {                               // dense_2 dX, ReLU
            const float *Wq = learn_base(W);
        const int b = i % n, k = i / n;
        float *t = T + b * ts;
        t[T_DLN2 + k] = t[T_Y2 + k] > 0.f ? t[T_DOUT] * Wq[N.w3 + k] : 0.f;
    });
    for (int layer = 2; layer >= 1; layer--) {
        const int go = layer == 2 ? N.ln2g : N.ln1g, xh = layer == 2 ? T_X2 : T_X1, dln = layer == 2 ? T_DLN2 : T_DLN1;
        const int dh = layer == 2 ? T_DH2 : T_DH1, rs = layer == 2 ? T_RSTD2 : T_RSTD1;
        E.forall(n, [=](int b) {                                   // LayerNorm backward: the two means
            const float *Wq = learn_base(W);
            float *t = T + b * ts;
            float s = 0.f, e = 0.f;
            for (int k = 0; k < LRN_H; k++) {
                const float d = t[dln + k] * Wq[go + k];
                s += d;
                e = fmaf(d, t[xh + k], e);
            }
            t[T_M1] = s / (float)LRN_H;
            t[T_M2] = e / (float)LRN_H;
        });
        E.forall(n * LRN_H, [=](int i) {
            const float *Wq = learn_base(W);
            const int b = i % n, k = i / n;
            float *t = T + b * ts;
            const float d = t[dln + k] * Wq[go + k];
            t[dh + k] = t[rs] * ((d - t[T_M1]) - t[xh + k] * t[T_M2]);
        });
        if (layer == 2 && !to_input) {
            E.forall(n, [=](int b) {                               // dX of dense_1, input column 64: the own action
            const float *Wq = learn_base(W);
                float *t = T + b * ts;
                float acc = 0.f;
                for (int u = 0; u < LRN_H; u++) acc = fmaf(Wq[N.w2 + LRN_H * LRN_H + u], t[T_DH2 + u], acc);
                t[T_M1] = acc;
            });
            return;
        }
        const int K = layer == 2 ? LRN_H : LRN_IN, wo = layer == 2 ? N.w2 : N.w1;
        E.forall(n * K, [=](int i) {                               // dense dX (+ ReLU below dense_1)
            const float *Wq = learn_base(W);
            const int b = i % n, k = i / n;
            float *t = T + b * ts;
            float acc = 0.f;
            for (int u = 0; u < LRN_H; u++) acc = fmaf(Wq[wo + k * LRN_H + u], t[dh + u], acc);
            if (layer == 2) t[T_DLN1 + k] = t[T_Y1 + k] > 0.f ? acc : 0.f;
            else t[T_DA0 + k] = acc;
        });
    }
}

// ---- the parameters' gradients: rows b0 .. b0 + n - 1 of the batch continue the sums in G (set to zero in front of row 0)
template <class Exec> PVE_HD void learn_accumulate(const Exec &E, const LearnNet N, float *G, const float *T, int ts, int n, bool first)
{
    E.forall(N.total, [=](int w) {
        int A, B;
        learn_grad_src(N, w, A, B);
        float acc = first ? 0.f : G[w];
        for (int b = 0; b < n; b++) acc = fmaf(T[b * ts + A], T[b * ts + B], acc);
        G[w] = acc;
    });
}

// ---- Adam on one network + the soft update of its target
template <class Exec> PVE_HD void learn_adam(const Exec &E, const LearnNet N, const LearnHyper H, float lr, float *P, int o_w, int o_t,
                                             int o_m, int o_v, int o_pow, const float *G, float *gout)
{
    E.forall(N.total, [=](int i) {
        const float b1p = P[o_pow], b2p = P[o_pow + 1];
        const float alpha = lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
        const float g = G[i];
        float m = P[o_m + i], v = P[o_v + i], w = P[o_w + i];
        m += (g - m) * (1.0f - H.beta1);
        v += (g * g - v) * (1.0f - H.beta2);
        w -= (m * alpha) / (sqrtf(v) + H.epsilon);
        P[o_m + i] = m; P[o_v + i] = v; P[o_w + i] = w;
        const float c1 = (float)(1.0 - (double)H.tau), c2 = H.tau;
        const float p1 = c1 * w, p2 = c2 * P[o_t + i];
        P[o_t + i] = p1 + p2;
        if (gout) gout[i] = g;
    });
    E.forall(1, [=](int) { P[o_pow] *= H.beta1; P[o_pow + 1] *= H.beta2; });
}

// ---- n_batches learner steps in sequence
template <class Exec> PVE_HD void learn_steps(const Exec &E, const LearnCtx C)
{
    const LearnNet NA = learn_net(false), NC = learn_net(true);
    const int B = C.batch;
    float *const P = C.P, *const S = C.S, *const T = C.tape;
    float *const Gc = P + LB_GRAD, *const Ga = P + LB_GRAD + lrn_pad4(LRN_CRITIC_W);
    const float *const Wa = P + LB_ACTOR, *const Wc = P + LB_CRITIC;         // the online networks, read where they live
    for (int step = 0; step < C.n_batches; step++) {
        const float *rows = C.rows + (size_t)step * B * LRN_IN, *act7 = C.act7 + (size_t)step * B * LRN_ACT;
        const float *target = C.target + (size_t)step * B;
        float *gout = C.grads ? C.grads + (size_t)step * LRN_GRADS : nullptr;
        // 1. critic_loss = mean((target - Q)^2), dQ = 2 (Q - target) / B; Adam on the critic
        for (int b0 = 0; b0 < B; b0 += LEARN_SUB_1) {
            const int n = B - b0 < LEARN_SUB_1 ? B - b0 : LEARN_SUB_1, ts = LEARN_STRIDE_1;
            E.forall(n * 8, [=](int i) {
                const int b = i / 8, e = i % 8;
                if (e < LRN_ACT) T[b * ts + T_ACT + e] = act7[(size_t)(b0 + b) * LRN_ACT + e];
                else T[b * ts + T_TGT] = target[b0 + b];
            });
            learn_forward(E, NC, Wc, T, ts, rows + (size_t)b0 * LRN_IN, n);
            E.forall(n, [=](int b) {
                float *t = T + b * ts;
                t[T_DOUT] = 2.0f * (t[T_OUT] - t[T_TGT]) / (float)B;
            });
            E.forall(1, [=](int) {
                float acc = b0 ? S[S_LOSS_C] : 0.f;
                for (int b = 0; b < n; b++) { const float d = T[b * ts + T_TGT] - T[b * ts + T_OUT]; acc = fmaf(d, d, acc); }
                S[S_LOSS_C] = acc;
            });
            learn_backward(E, NC, Wc, T, ts, n, true);
            learn_accumulate(E, NC, Gc, T, ts, n, b0 == 0);
        }
        learn_adam(E, NC, C.H, C.H.critic_lr, P, LB_CRITIC, LB_TCRITIC, LB_M_CRITIC, LB_V_CRITIC, LB_POWERS + 2, Gc, gout);
        // 2. actor_loss = -mean(Q(s, [actor(s), act7[1..6]])) with the updated critic, dQ = -1 / B; Adam on the actor
        const bool with_actor = !(C.H.flags & LEARN_CRITIC_ONLY);
        if (with_actor) {
            for (int b0 = 0; b0 < B; b0 += LEARN_SUB_2) {
                const int n = B - b0 < LEARN_SUB_2 ? B - b0 : LEARN_SUB_2, ts = LEARN_STRIDE_2;
                float *Tc = T + T_NET;                                          // the critic's tape behind the actor's, row by row
                learn_forward(E, NA, Wa, T, ts, rows + (size_t)b0 * LRN_IN, n);
                E.forall(n * 8, [=](int i) {
                    const int b = i / 8, e = i % 8;
                    if (e == 0) { const float a = learn_tanh3(T[b * ts + T_OUT]); T[b * ts + T_OUT] = a; Tc[b * ts + T_ACT] = a; }
                    else if (e < LRN_ACT) Tc[b * ts + T_ACT + e] = act7[(size_t)(b0 + b) * LRN_ACT + e];
                    else Tc[b * ts + T_DOUT] = -1.0f / (float)B;
                });
                learn_forward(E, NC, Wc, Tc, ts, rows + (size_t)b0 * LRN_IN, n);
                E.forall(1, [=](int) {
                    float acc = b0 ? S[S_LOSS_A] : 0.f;
                    for (int b = 0; b < n; b++) acc += Tc[b * ts + T_OUT];
                    S[S_LOSS_A] = acc;
                });
                learn_backward(E, NC, Wc, Tc, ts, n, false);
                E.forall(n, [=](int b) { T[b * ts + T_DOUT] = Tc[b * ts + T_M1] * learn_dtanh3(T[b * ts + T_OUT]); });
                learn_backward(E, NA, Wa, T, ts, n, true);
                learn_accumulate(E, NA, Ga, T, ts, n, b0 == 0);
            }
            learn_adam(E, NA, C.H, C.H.actor_lr, P, LB_ACTOR, LB_TACTOR, LB_M_ACTOR, LB_V_ACTOR, LB_POWERS, Ga,
                       gout ? gout + LRN_CRITIC_W : nullptr);
        }
        float *losses = C.losses;
        E.forall(with_actor || !gout ? 1 : 1 + LRN_ACTOR_W, [=](int i) {
            if (i == 0) {
                int32_t cnt;
                memcpy(&cnt, P + LB_STEPS, 4);
                cnt++;
                memcpy(P + LB_STEPS, &cnt, 4);
                if (losses) {
                    losses[2 * step] = S[S_LOSS_C] / (float)B;
                    losses[2 * step + 1] = with_actor ? -(S[S_LOSS_A] / (float)B) : 0.f;
                }
            } else gout[LRN_CRITIC_W + i - 1] = 0.f;                            // critic only: no actor gradient was applied
        });
    }
}

// =================================================================== the WIDE step: a batch in slices of PVE_LEARN_SLICE rows
// (see ORDERS).  A slice pass leaves its slice's partial gradients and partial loss sum in that slice's row of a caller-owned
// workspace; a combine phase adds the rows in ascending order into LB_GRAD and applies learn_adam.  Slice passes of different slices
// share nothing but the weights they read, so the device gives each to a workgroup of its own (pve_hip.hip k_learner_slice /
// k_learner_apply); learn_steps_wide under LearnSeq is the host definition.
constexpr int LEARN_SLICE = 128;                                  // PVE_LEARN_SLICE
// one slice's row of the workspace: critic gradients (padded), actor gradients (padded), then critic / actor loss sum + 2 reserved
constexpr int LW_CRITIC = 0, LW_ACTOR = LW_CRITIC + lrn_pad4(LRN_CRITIC_W), LW_LOSS = LW_ACTOR + lrn_pad4(LRN_ACTOR_W),
              LW_ROW = LW_LOSS + 4;                               // PVE_LEARNER_WIDE_ROW
PVE_HD int learn_n_slices(int batch) { return (batch + LEARN_SLICE - 1) / LEARN_SLICE; }

// ---- one pass (critic: learn_steps' step 1; else its step 2) over slice s of minibatch `step`, into the slice's row R.  Every
// chain starts from 0 at the slice's first row and continues across the slice's sub-blocks; dQ is scaled by the WHOLE batch.
template <class Exec> PVE_HD void learn_slice(const Exec &E, const LearnCtx C, int step, int s, bool critic, float *R)
{
    const LearnNet NA = learn_net(false), NC = learn_net(true);
    const int B = C.batch, r0 = s * LEARN_SLICE, ns = B - r0 < LEARN_SLICE ? B - r0 : LEARN_SLICE;
    float *const P = C.P, *const T = C.tape;
    const float *const Wa = P + LB_ACTOR, *const Wc = P + LB_CRITIC;
    const size_t first_row = (size_t)step * B + r0;
    const float *rows = C.rows + first_row * LRN_IN, *act7 = C.act7 + first_row * LRN_ACT, *target = C.target + first_row;
    if (critic) {
        float *const G = R + LW_CRITIC, *const L = R + LW_LOSS;
        for (int b0 = 0; b0 < ns; b0 += LEARN_SUB_1) {
            const int n = ns - b0 < LEARN_SUB_1 ? ns - b0 : LEARN_SUB_1, ts = LEARN_STRIDE_1;
            E.forall(n * 8, [=](int i) {
                const int b = i / 8, e = i % 8;
                if (e < LRN_ACT) T[b * ts + T_ACT + e] = act7[(size_t)(b0 + b) * LRN_ACT + e];
                else T[b * ts + T_TGT] = target[b0 + b];
            });
            learn_forward(E, NC, Wc, T, ts, rows + (size_t)b0 * LRN_IN, n);
            E.forall(n, [=](int b) {
                float *t = T + b * ts;
                t[T_DOUT] = 2.0f * (t[T_OUT] - t[T_TGT]) / (float)B;
            });
            E.forall(1, [=](int) {
                float acc = b0 ? L[S_LOSS_C] : 0.f;
                for (int b = 0; b < n; b++) { const float d = T[b * ts + T_TGT] - T[b * ts + T_OUT]; acc = fmaf(d, d, acc); }
                L[S_LOSS_C] = acc;
            });
            learn_backward(E, NC, Wc, T, ts, n, true);
            learn_accumulate(E, NC, G, T, ts, n, b0 == 0);
        }
    } else {
        float *const G = R + LW_ACTOR, *const L = R + LW_LOSS;
        for (int b0 = 0; b0 < ns; b0 += LEARN_SUB_2) {
            const int n = ns - b0 < LEARN_SUB_2 ? ns - b0 : LEARN_SUB_2, ts = LEARN_STRIDE_2;
            float *Tc = T + T_NET;
            learn_forward(E, NA, Wa, T, ts, rows + (size_t)b0 * LRN_IN, n);
            E.forall(n * 8, [=](int i) {
                const int b = i / 8, e = i % 8;
                if (e == 0) { const float a = learn_tanh3(T[b * ts + T_OUT]); T[b * ts + T_OUT] = a; Tc[b * ts + T_ACT] = a; }
                else if (e < LRN_ACT) Tc[b * ts + T_ACT + e] = act7[(size_t)(b0 + b) * LRN_ACT + e];
                else Tc[b * ts + T_DOUT] = -1.0f / (float)B;
            });
            learn_forward(E, NC, Wc, Tc, ts, rows + (size_t)b0 * LRN_IN, n);
            E.forall(1, [=](int) {
                float acc = b0 ? L[S_LOSS_A] : 0.f;
                for (int b = 0; b < n; b++) acc += Tc[b * ts + T_OUT];
                L[S_LOSS_A] = acc;
            });
            learn_backward(E, NC, Wc, Tc, ts, n, false);
            E.forall(n, [=](int b) { T[b * ts + T_DOUT] = Tc[b * ts + T_M1] * learn_dtanh3(T[b * ts + T_OUT]); });
            learn_backward(E, NA, Wa, T, ts, n, true);
            learn_accumulate(E, NA, G, T, ts, n, b0 == 0);
        }
    }
}

// ---- the combine phase of one network: the slices' rows added in ascending order into LB_GRAD, learn_adam on the sum; behind the
// last pass of a step (`last`: the actor's, or the critic's with LEARN_CRITIC_ONLY) the step count and what learn_steps reports
template <class Exec> PVE_HD void learn_combine(const Exec &E, const LearnCtx C, int step, bool critic, const float *work, int n_slices)
{
    const LearnNet N = learn_net(critic);
    const int B = C.batch, off = critic ? LW_CRITIC : LW_ACTOR;
    float *const P = C.P, *const G = P + LB_GRAD + (critic ? 0 : lrn_pad4(LRN_CRITIC_W));
    float *gout = C.grads ? C.grads + (size_t)step * LRN_GRADS : nullptr;
    E.forall(N.total, [=](int i) {
        const float *p = work + off + i;
        float acc = p[0];
        int s = 1;
        for (; s + 8 <= n_slices; s += 8) {                                     // eight loads in flight; the adds in their one order
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = p[(size_t)(s + j) * LW_ROW];
#pragma unroll
            for (int j = 0; j < 8; j++) acc = acc + v[j];
        }
        for (; s < n_slices; s++) acc = acc + p[(size_t)s * LW_ROW];
        G[i] = acc;
    });
    if (critic) learn_adam(E, N, C.H, C.H.critic_lr, P, LB_CRITIC, LB_TCRITIC, LB_M_CRITIC, LB_V_CRITIC, LB_POWERS + 2, G, gout);
    else learn_adam(E, N, C.H, C.H.actor_lr, P, LB_ACTOR, LB_TACTOR, LB_M_ACTOR, LB_V_ACTOR, LB_POWERS, G, gout ? gout + LRN_CRITIC_W : nullptr);
    const bool with_actor = !(C.H.flags & LEARN_CRITIC_ONLY), last = !critic || !with_actor;
    float *losses = C.losses;
    E.forall(last && !with_actor && gout ? 1 + LRN_ACTOR_W : 1, [=](int i) {
        if (i == 0) {
            if (last) {
                int32_t cnt;
                memcpy(&cnt, P + LB_STEPS, 4);
                cnt++;
                memcpy(P + LB_STEPS, &cnt, 4);
            }
            if (losses) {
                const int k = critic ? S_LOSS_C : S_LOSS_A;
                float acc = work[LW_LOSS + k];
                for (int s = 1; s < n_slices; s++) acc = acc + work[(size_t)s * LW_ROW + LW_LOSS + k];
                if (critic) {
                    losses[2 * step] = acc / (float)B;
                    if (!with_actor) losses[2 * step + 1] = 0.f;
                } else losses[2 * step + 1] = -(acc / (float)B);
            }
        } else gout[LRN_CRITIC_W + i - 1] = 0.f;                                // critic only: no actor gradient was applied
    });
}

// ---- n_batches wide steps in sequence (work: learn_n_slices(batch) * LW_ROW floats; no float of it is read before it is written)
template <class Exec> PVE_HD void learn_steps_wide(const Exec &E, const LearnCtx C, float *work)
{
    const int n_slices = learn_n_slices(C.batch);
    const bool with_actor = !(C.H.flags & LEARN_CRITIC_ONLY);
    for (int step = 0; step < C.n_batches; step++) {
        for (int s = 0; s < n_slices; s++) learn_slice(E, C, step, s, true, work + (size_t)s * LW_ROW);
        learn_combine(E, C, step, true, work, n_slices);
        if (!with_actor) continue;
        for (int s = 0; s < n_slices; s++) learn_slice(E, C, step, s, false, work + (size_t)s * LW_ROW);
        learn_combine(E, C, step, false, work, n_slices);
    }
}

}  // namespace pve

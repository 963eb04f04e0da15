// pve_critic.h -- the MADDPG critic and the bootstrap term of the n-step target on the device
// (reference model_agent_maddpg.py:52-74 `critic_network`; main.py:76-77 `agent_ddpg_target.Q(...)` on a replay batch,
// main.py:253-260: every one of the 7 rows of a vehicle's `state_next` through the TARGET actor, then the TARGET critic on
// row 0 with those 7 actions -- eight sess.run calls of batch 1 per vehicle and tick in the reference).
//
//   x(28) -> LayerNorm -> Dense 28x64 -> LayerNorm -> ReLU -> concat [h(64), own action, 6 other actions] (71)
//         -> Dense 71x64 -> LayerNorm -> ReLU -> Dense 64x1                      (no tanh, no gain)
//
// The critic is the actor's shape with a 71-wide second layer, and runs like the split-half actor (pve_actor.h): the same
// lane layout, the same helper functions, one more K-block in the second layer.
#pragma once
#include "pve_actor.h"

namespace pve {

constexpr int CRT_ACT = 7, CRT_K2 = ACT_H + CRT_ACT;      // the 7 actions; rows of dense_1/kernel (model_agent_maddpg.py:66, :82)
// flat float32 weight vector (6841 values), in this order (TF variable layouts, kernels [in][out]):
constexpr int CW_LN0_G = 0, CW_LN0_B = CW_LN0_G + ACT_IN, CW_W1 = CW_LN0_B + ACT_IN,
              CW_B1 = CW_W1 + ACT_IN * ACT_H, CW_LN1_G = CW_B1 + ACT_H, CW_LN1_B = CW_LN1_G + ACT_H,
              CW_W2 = CW_LN1_B + ACT_H /* rows 0..63 hidden, 64 own action, 65..70 the six other actions */,
              CW_B2 = CW_W2 + CRT_K2 * ACT_H, CW_LN2_G = CW_B2 + ACT_H, CW_LN2_B = CW_LN2_G + ACT_H,
              CW_W3 = CW_LN2_B + ACT_H, CW_B3 = CW_W3 + ACT_H, CW_TOTAL = CW_B3 + 1;
static_assert(CW_TOTAL == 6841 && CW_TOTAL * 4 <= (int)CRITIC_FLAT_BYTES, "critic weight count (PVE_CRITIC_N_WEIGHTS)");

// ------------------------------------------------------------------------------------------------------
// Canonical float32 evaluation order of the critic (plain code, host or device): the CPU-testable statement of the network,
// in the manner of actor_canonical -- LayerNorm sums by lane groups q = 0..3, the 64 hidden units contracted in the order
// (m, r, q), k = 16 m + 4 q + r, then the seven actions in their order, one rounding per fused multiply-add.
// x: the 28 features of row 0; a7: own action, then the six other actions.
inline float critic_canonical(const float *W, const float *x, const float *a7)
{
    float p[4], a0[ACT_IN];
    for (int q = 0; q < 4; q++) { p[q] = 0.f; for (int s = 0; s < ACT_IN / 4; s++) p[q] += x[4 * s + q]; }
    float mean = actor_ln_combine(p) / (float)ACT_IN;
    for (int q = 0; q < 4; q++) {
        p[q] = 0.f;
        for (int s = 0; s < ACT_IN / 4; s++) { const float d = x[4 * s + q] - mean; p[q] = fmaf(d, d, p[q]); }
    }
    float rstd = 1.0f / sqrtf(actor_ln_combine(p) / (float)ACT_IN + 1e-12f);
    for (int k = 0; k < ACT_IN; k++) {
        const float inv = rstd * W[CW_LN0_G + k];
        a0[k] = fmaf(x[k], inv, W[CW_LN0_B + k] - mean * inv);
    }
    float h[ACT_H], g[ACT_H];
    for (int u = 0; u < ACT_H; u++) {
        float acc = W[CW_B1 + u];
        for (int k = 0; k < ACT_IN; k++) acc = fmaf(W[CW_W1 + k * ACT_H + u], a0[k], acc);
        h[u] = acc;
    }
    for (int layer = 1; layer <= 2; layer++) {
        const int G = layer == 1 ? CW_LN1_G : CW_LN2_G, B = layer == 1 ? CW_LN1_B : CW_LN2_B;
        float *src = layer == 1 ? h : g;
        for (int q = 0; q < 4; q++) {
            float a4[4];
            for (int r = 0; r < 4; r++)
                a4[r] = (src[4 * q + r] + src[16 + 4 * q + r]) + (src[32 + 4 * q + r] + src[48 + 4 * q + r]);
            p[q] = (a4[0] + a4[1]) + (a4[2] + a4[3]);
        }
        mean = actor_ln_combine(p) / (float)ACT_H;
        for (int q = 0; q < 4; q++) {
            float e4[4];
            for (int r = 0; r < 4; r++) {
                float e = 0.f;
                for (int m = 0; m < 4; m++) { const float d = src[16 * m + 4 * q + r] - mean; e = fmaf(d, d, e); }
                e4[r] = e;
            }
            p[q] = (e4[0] + e4[1]) + (e4[2] + e4[3]);
        }
        rstd = 1.0f / sqrtf(actor_ln_combine(p) / (float)ACT_H + 1e-12f);
        for (int u = 0; u < ACT_H; u++) {
            const float inv = rstd * W[G + u];
            src[u] = fmaxf(fmaf(src[u], inv, W[B + u] - mean * inv), 0.f);
        }
        if (layer == 1) {
            // dense 71 -> 64: the hidden units in the order (m, r, q), then the actions 64 .. 70 (model_agent_maddpg.py:66)
            for (int u = 0; u < ACT_H; u++) {
                float acc = W[CW_B2 + u];
                for (int m = 0; m < 4; m++) for (int r = 0; r < 4; r++) for (int q = 0; q < 4; q++) {
                    const int k = 16 * m + 4 * q + r;
                    acc = fmaf(W[CW_W2 + k * ACT_H + u], h[k], acc);
                }
                for (int e = 0; e < CRT_ACT; e++) acc = fmaf(W[CW_W2 + (ACT_H + e) * ACT_H + u], a7[e], acc);
                g[u] = acc;
            }
        }
    }
    // dense 64 -> 1: per lane group in (m, r) order, groups combined like the LayerNorm sums; no tanh, no gain
    for (int q = 0; q < 4; q++) {
        p[q] = 0.f;
        for (int m = 0; m < 4; m++) for (int r = 0; r < 4; r++) { const int k = 16 * m + 4 * q + r; p[q] = fmaf(g[k], W[CW_W3 + k], p[q]); }
    }
    return actor_ln_combine(p) + W[CW_B3];
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------------
// The packed critic (device buffer written by k_critic_pack): the actor's packing scheme (dense kernels centered over their
// output units, split into half pairs, in A-operand order; parameter vectors in lane order) with a second layer of K = 71
// padded to 80 = FIVE K-blocks of 16: blocks 0..3 are the hidden units exactly as in the actor, block 4 carries the 7
// action rows of dense_1/kernel (k = 8 hf + e: rows 64 + e for hf = 0, e < 7) and zeros.  The float parameters use the
// actor's PV_* offsets (PV_B3 = dense_2/bias; PV_A0 is unused; PV_EPS1 / PV_EPS2 = the variance epsilons that go with the
// pack-time factors 2^e of the two dense kernels, the seven action rows included -- pack_exponent of pve_actor.h).  Byte offsets:
constexpr int CRT_KB2 = 5;
constexpr int CP_A1 = 0;                                          // _Float16 [hl 2][m 2][kb 2][lane 64][8]
constexpr int CP_A2 = CP_A1 + 2 * 2 * 2 * 64 * 8 * 2;             // _Float16 [hl 2][m2 2][kb 5][lane 64][8]
constexpr int CP_PRM = CP_A2 + 2 * 2 * CRT_KB2 * 64 * 8 * 2;      // float [PV_TOTAL]
constexpr int CP_BYTES = CP_PRM + PV_TOTAL * 4;
constexpr int CP_BYTES_PADDED = (CP_BYTES + 255) / 256 * 256;
static_assert(CP_PRM == 28672 && CP_BYTES_PADDED == (int)CRITIC_PACKED_BYTES, "packed critic layout");
constexpr int CRT_BLOCKS = 4 + 2 * CRT_KB2;                       // product blocks of one tile

__device__ __forceinline__ pve_v8h critic_a_operand(const pve_v8h *A1, const pve_v8h *A2, int s, int hl, unsigned ob)
{   // block s: 0..3 = layer 1 (m = s >> 1, kb = s & 1), 4..13 = layer 2 (m2 = (s - 4) / 5, kb = (s - 4) % 5)
    const pve_v8h *blk = s < 4 ? A1 + ((hl * 2 + (s >> 1)) * 2 + (s & 1)) * 64
                               : A2 + ((hl * 2 + (s - 4) / CRT_KB2) * CRT_KB2 + (s - 4) % CRT_KB2) * 64;
    return *(const pve_v8h *)((const char *)blk + ob);
}

// One tile of 32 vehicles on one wave, lane layout of actor_tile32 (lane (j, hf) holds half of vehicle j): x[16] = this lane's
// raw features of row 0, a7 = the seven actions of vehicle j (read in the hf = 0 lane only) -> Q of vehicle j (in both of its
// lanes).  Three v_mfma_f32_32x32x16_f16 per product block, float32 accumulation, the operand pair of block s + 1 requested
// while block s multiplies (see actor_tile32).  The B operand of K-block 4 is built from the actions: the hf = 0 lane holds
// a_0 .. a_6 and 0, the hf = 1 lane zeros.  actor_split8 closes with the `s_nop 1` its hazard note asks for, so every B
// operand built here is safe to feed to a matrix instruction.
__device__ __forceinline__ float critic_tile32(const pve_v8h *A1, const pve_v8h *A2, const float *prm, const float (&x)[16],
                                               const float (&a7)[CRT_ACT], int lane)
{
    const int hf = lane >> 5;
    unsigned o = (unsigned)lane * 16u;
    asm volatile("" : "+v"(o));
    pve_v8h ah[2], al[2];                                     // operand ring
    ah[0] = critic_a_operand(A1, A2, 0, 0, o); al[0] = critic_a_operand(A1, A2, 0, 1, o);
    // ---- LayerNorm over the 28 inputs
    pve_v16f d;
#pragma unroll
    for (int c = 0; c < 16; c++) d[c] = x[c];
    const float mean = actor_xsum2(actor_hsum16(d)) * (1.0f / (float)ACT_IN);
    d = d - mean;
    if (hf) { d[12] = 0.f; d[13] = 0.f; d[14] = 0.f; d[15] = 0.f; }   // features 28..31 do not exist
    const float var = actor_hsum16(d * d);
    const float rstd0 = __builtin_amdgcn_rsqf(actor_xsum2(var) * (1.0f / (float)ACT_IN) + 1e-12f);
    pve_v8h bh[CRT_KB2], bl[CRT_KB2];                         // B operands of the current layer: K-blocks as half pairs
    {
        const pve_v16f ga = *(const pve_v16f *)(prm + PV_LN0G + 16 * hf), be = *(const pve_v16f *)(prm + PV_LN0B + 16 * hf);
        const pve_v16f yv = __builtin_elementwise_fma(d, ga * rstd0, be);
        float y[16];
#pragma unroll
        for (int c = 0; c < 16; c++) y[c] = yv[c];
        actor_split8(y, bh[0], bl[0]);
        actor_split8(y + 8, bh[1], bl[1]);
    }
    pve_v16f h[2], g[2];
#pragma unroll
    for (int s = 0; s < CRT_BLOCKS; s++) {
        if (s + 1 < CRT_BLOCKS) {                             // request block s + 1
            asm volatile("" : "+v"(o));
            ah[(s + 1) % 2] = critic_a_operand(A1, A2, s + 1, 0, o); al[(s + 1) % 2] = critic_a_operand(A1, A2, s + 1, 1, o);
        }
        if (s == 4) {
            // ---- LayerNorm_1 + ReLU; K-blocks 0..3 of the next layer are the registers of h (as in the actor), K-block 4 the actions
            actor_ln_relu32(h, prm + PV_G1 + hf * 32, prm + PV_BE1 + hf * 32, prm[PV_EPS1]);
#pragma unroll
            for (int kb = 0; kb < 4; kb++) {
                float hv[8];
#pragma unroll
                for (int e = 0; e < 8; e++) hv[e] = h[kb >> 1][8 * (kb & 1) + e];
                actor_split8(hv, bh[kb], bl[kb]);
            }
            float av[8];
#pragma unroll
            for (int e = 0; e < 8; e++) av[e] = (e < CRT_ACT && !hf) ? a7[e < CRT_ACT ? e : 0] : 0.f;
            actor_split8(av, bh[4], bl[4]);
        }
        const int layer2 = s >= 4, m = layer2 ? (s - 4) / CRT_KB2 : s >> 1, kb = layer2 ? (s - 4) % CRT_KB2 : s & 1;
        pve_v16f &acc = layer2 ? g[m] : h[m];
        if (kb == 0) acc = *(const pve_v16f *)(prm + (layer2 ? PV_B2 : PV_B1) + (hf * 2 + m) * 16);   // centered bias
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s % 2], bh[kb], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s % 2], bl[kb], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[s % 2], bh[kb], acc, 0, 0, 0);
    }
    actor_ln_relu32(g, prm + PV_G2 + hf * 32, prm + PV_BE2 + hf * 32, prm[PV_EPS2]);
    // ---- dense 64 -> 1
    pve_v16f pv = g[0] * *(const pve_v16f *)(prm + PV_W3 + (hf * 2 + 0) * 16);
    pv = __builtin_elementwise_fma(g[1], *(const pve_v16f *)(prm + PV_W3 + (hf * 2 + 1) * 16), pv);
    return actor_xsum2(actor_hsum16(pv)) + prm[PV_B3];
}

// pve_set_target_networks: flat float32 critic weights -> the packed buffer (one workgroup of 256 threads)
__global__ __launch_bounds__(256) void k_critic_pack(const float *__restrict__ W, unsigned char *__restrict__ packed)
{
    __shared__ float cm1[ACT_IN], cm2[CRT_K2], bm[2];
    __shared__ unsigned mx[2];
    const int tid = threadIdx.x;
    // means over the OUTPUT units (what LayerNorm subtracts): per input row of each dense kernel, and of the biases
    if (tid < ACT_IN) { double s = 0; for (int u = 0; u < ACT_H; u++) s += (double)W[CW_W1 + tid * ACT_H + u]; cm1[tid] = (float)(s / ACT_H); }
    if (tid >= 64 && tid < 64 + CRT_K2) { const int k = tid - 64; double s = 0; for (int u = 0; u < ACT_H; u++) s += (double)W[CW_W2 + k * ACT_H + u]; cm2[k] = (float)(s / ACT_H); }
    if (tid == 192 || tid == 193) { const int o = tid == 192 ? CW_B1 : CW_B2; double s = 0; for (int u = 0; u < ACT_H; u++) s += (double)W[o + u]; bm[tid - 192] = (float)(s / ACT_H); }
    if (tid >= 194 && tid < 196) mx[tid - 194] = 0u;
    __syncthreads();
    // the largest centred entry of each dense kernel, the seven action rows included -> the layer's factor 2^e (pack_exponent)
    for (int n = tid; n < ACT_IN * ACT_H; n += 256) atomicMax(&mx[0], __float_as_uint(fabsf(W[CW_W1 + n] - cm1[n >> 6])));
    for (int n = tid; n < CRT_K2 * ACT_H; n += 256) atomicMax(&mx[1], __float_as_uint(fabsf(W[CW_W2 + n] - cm2[n >> 6])));
    __syncthreads();
    const int e1 = pack_exponent(mx[0]), e2 = pack_exponent(mx[1]);
    const float s1 = ldexpf(1.0f, e1), s2 = ldexpf(1.0f, e2);
    pve_v8h *A1 = (pve_v8h *)(packed + CP_A1), *A2 = (pve_v8h *)(packed + CP_A2);
    float *prm = (float *)(packed + CP_PRM);
    for (int n = tid; n < CRT_BLOCKS * 64; n += 256) {        // one thread per operand vector (8 halves of one lane)
        const int l = n & 63, t = n >> 6, hf = l >> 5, i = l & 31;
        float w[8];
        pve_v8h hi, lo;
        if (t < 4) {                                          // layer 1: A[i][8 hf + e] = W1c[16 kb + 8 hf + e][32 m + i]
            const int m = t >> 1, kb = t & 1;
#pragma unroll
            for (int e = 0; e < 8; e++) { const int k = 16 * kb + 8 * hf + e; w[e] = k < ACT_IN ? (W[CW_W1 + k * ACT_H + 32 * m + i] - cm1[k]) * s1 : 0.f; }
            actor_split8(w, hi, lo);
            A1[((0 * 2 + m) * 2 + kb) * 64 + l] = hi; A1[((1 * 2 + m) * 2 + kb) * 64 + l] = lo;
        } else {                                              // layer 2: kb < 4 the hidden units (as the actor), kb = 4 the action rows
            const int m2 = (t - 4) / CRT_KB2, kb = (t - 4) % CRT_KB2;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int k = kb < 4 ? actor_unit(kb >> 1, 8 * (kb & 1) + e, hf) : ((hf == 0 && e < CRT_ACT) ? ACT_H + e : -1);
                w[e] = k >= 0 ? (W[CW_W2 + k * ACT_H + 32 * m2 + i] - cm2[k]) * s2 : 0.f;
            }
            actor_split8(w, hi, lo);
            A2[((0 * 2 + m2) * CRT_KB2 + kb) * 64 + l] = hi; A2[((1 * 2 + m2) * CRT_KB2 + kb) * 64 + l] = lo;
        }
    }
    if (tid < 64) {                                           // parameter vectors in lane order
        const int hf = tid >> 5, m = (tid >> 4) & 1, r = tid & 15, u = actor_unit(m, r, hf);
        prm[PV_B1 + tid] = (W[CW_B1 + u] - bm[0]) * s1; prm[PV_G1 + tid] = W[CW_LN1_G + u]; prm[PV_BE1 + tid] = W[CW_LN1_B + u];
        prm[PV_B2 + tid] = (W[CW_B2 + u] - bm[1]) * s2; prm[PV_G2 + tid] = W[CW_LN2_G + u]; prm[PV_BE2 + tid] = W[CW_LN2_B + u];
        prm[PV_W3 + tid] = W[CW_W3 + u];
    }
    if (tid < 32) {
        const int hf = tid >> 4, c = tid & 15, f = actor_feature(c, hf);
        prm[PV_LN0G + tid] = f < ACT_IN ? W[CW_LN0_G + f] : 0.f; prm[PV_LN0B + tid] = f < ACT_IN ? W[CW_LN0_B + f] : 0.f;
    }
    if (tid == 0) { prm[PV_B3] = W[CW_B3]; prm[PV_A0] = 0.f; prm[PV_EPS1] = 1e-12f * ldexpf(1.0f, 2 * e1); prm[PV_EPS2] = 1e-12f * ldexpf(1.0f, 2 * e2); }
}

// ------------------------------------------------------------------------------------------------------
// k_target_q<OBS_T, BOOT>: BOOT = true is k_bootstrap_q (pve_bootstrap_q), BOOT = false is k_critic (pve_critic_forward): ONE
// kernel body, so the critic half of the two is the same device function on the same operands (bit-equal results).
//
// Persistent workgroups of 4 waves sharing one copy of the packed parameters in LDS (BOOT: target actor 26 880 B + critic
// 30 976 B: two workgroups per CU; critic alone: four).  Every wave is on its own: it walks the rows in chunks of 64, keeps
// the rows to evaluate (flags: PVE_F_CTL set and PVE_F_DONE clear -- main.py:250-251 does no bootstrap behind Done, uncontrolled
// slots have no transition; no flags = every row) in a wave-private ring in LDS and runs a tile as soon as 32 are pending, so
// tiles are full whatever the density of evaluated rows; every other row gets q = 0 and zero actions.
// Per tile (BOOT): the seven rows of `state` go through actor_tile32 -- the UNCHANGED device function of pve_actor.h with the
// packed target actor, all seven, the all-zero rows of absent neighbours included (main.py:254-255) -- then critic_tile32 on
// row 0 and the seven actions, which never leave the registers.  Row k + 1 is requested before row k is evaluated; every
// 112-byte row is read by exactly two lanes in 16-byte pieces (actor_fetch).
constexpr int TQ_F_CTL = 0x02, TQ_F_DONE = 0x04;                  // PVE_F_CTL, PVE_F_DONE (include/pve_env.h)
constexpr int TQ_STATE_ROWS = NNB + 1;                        // rows of a vehicle's state (PVE_STATE_ROWS)
constexpr int TQ_RING = 128;                                  // pending rows per wave: < 32 left over + 64 new
template <typename OBS_T, bool BOOT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BOOT ? 2 : 4, BOOT ? 2 : 4)))
void k_target_q(const unsigned char *__restrict__ actor_packed, const unsigned char *__restrict__ critic_packed,
                const OBS_T *__restrict__ rows, const float *__restrict__ act7_in, const int32_t *__restrict__ flags,
                float *__restrict__ q, float *__restrict__ act7_out, long long n)
{
    __shared__ __attribute__((aligned(64))) unsigned char sa[BOOT ? AP_BYTES_PADDED : 64];
    __shared__ __attribute__((aligned(64))) unsigned char sc[CP_BYTES_PADDED];
    __shared__ long long ring_s[4][TQ_RING];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long *ring = ring_s[wave];
    if constexpr (BOOT)
        for (int k = tid; k < AP_BYTES_PADDED / 16; k += 256) ((uint4 *)sa)[k] = ((const uint4 *)actor_packed)[k];
    for (int k = tid; k < CP_BYTES_PADDED / 16; k += 256) ((uint4 *)sc)[k] = ((const uint4 *)critic_packed)[k];
    __syncthreads();                                          // parameters staged
    const pve_v8h *A1 = (const pve_v8h *)(sa + AP_A1), *A2 = (const pve_v8h *)(sa + AP_A2);
    const float *aprm = (const float *)(sa + AP_PRM);
    const pve_v8h *C1 = (const pve_v8h *)(sc + CP_A1), *C2 = (const pve_v8h *)(sc + CP_A2);
    const float *cprm = (const float *)(sc + CP_PRM);
    constexpr int ROWS = BOOT ? TQ_STATE_ROWS : 1;               // observation rows per evaluated row
    const long long n_chunks = (n + 63) / 64, stride = (long long)gridDim.x * 4;
    int head = 0, npend = 0;                                  // wave-uniform: the ring holds entries head .. head + npend - 1
    for (long long c = (long long)blockIdx.x * 4 + wave; c < n_chunks + stride; c += stride) {
        const bool last = c >= n_chunks;                      // one pass behind the wave's last chunk: the partial tile
        if (!last) {
            const long long i = c * 64 + lane;
            const bool inside = i < n;
            const int f = (flags && inside) ? flags[i] : 0;
            const bool ev = inside && (!flags || (f & (TQ_F_CTL | TQ_F_DONE)) == TQ_F_CTL);
            const unsigned long long b = __ballot(ev);
            if (ev) ring[(head + npend + __builtin_popcountll(b & ((1ull << lane) - 1ull))) & (TQ_RING - 1)] = i;
            else if (inside) {
                q[i] = 0.f;
                if (BOOT && act7_out) {
#pragma unroll
                    for (int e = 0; e < CRT_ACT; e++) act7_out[i * CRT_ACT + e] = 0.f;
                }
            }
            npend += __builtin_popcountll(b);
        }
        __builtin_amdgcn_wave_barrier();                      // (wave-local: DS operations of one wave execute in order)
        while (npend >= 32 || (last && npend > 0)) {
            int wo = 0;
            asm volatile("" : "+v"(wo));                      // (keeps the parameter reads inside the loop)
            const int j = lane & 31, hf = lane >> 5, cnt = npend < 32 ? npend : 32;
            const bool valid = j < cnt;
            const long long i = ring[(head + (valid ? j : 0)) & (TQ_RING - 1)];
            float x0[16], a7[CRT_ACT];
            actor_fetch(rows, (size_t)i * ROWS, hf, x0);
            if constexpr (BOOT) {
                float x[16], xn[16];
#pragma unroll
                for (int e = 0; e < 16; e++) x[e] = x0[e];
#pragma unroll
                for (int e = 0; e < CRT_ACT; e++) a7[e] = 0.f;
#pragma unroll 1
                for (int k = 0; k < TQ_STATE_ROWS; k++) {
                    if (k + 1 < TQ_STATE_ROWS) actor_fetch(rows, (size_t)i * ROWS + k + 1, hf, xn);
                    const float a = actor_tile32(A1, A2, aprm + wo, x, lane);
#pragma unroll
                    for (int e = 0; e < CRT_ACT; e++) a7[e] = k == e ? a : a7[e];
#pragma unroll
                    for (int e = 0; e < 16; e++) x[e] = xn[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < CRT_ACT; e++) a7[e] = hf ? 0.f : act7_in[i * CRT_ACT + e];
            }
            const float qv = critic_tile32(C1, C2, cprm + wo, x0, a7, lane);
            if (valid && hf == 0) {
                q[i] = qv;
                if (BOOT && act7_out) {
#pragma unroll
                    for (int e = 0; e < CRT_ACT; e++) act7_out[i * CRT_ACT + e] = a7[e];
                }
            }
            head = (head + cnt) & (TQ_RING - 1);
            npend -= cnt;
        }
    }
}

#endif  // __HIPCC__
}  // namespace pve

// pve_hip.hip -- gfx950 (MI355X / CDNA4) kernels + HIP backend of the C ABI -> libpveenv.so
//
//   k_tick<CAP>     one workgroup (CAP = 64 or 128 threads = 1 or 2 wave64) per intersection:
//                   fused step* + scene_update + delete_vehicle, state staged in LDS, phases of
//                   pve_tick_core.h separated by workgroup barriers.
//   k_rollout<CAP>  pve_step_many: the same phases in a loop, the state resident on the chip between ticks
//   k_tick_geo<CAP> the 4- / 8-lane layouts (pve_tick_geo.h)
//   k_compact<CAP>  delete_vehicle() alone (split protocol of the single-env compat class)
//   k_reset<CAP>    constructor warm-up, one thread per intersection
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no FMA contraction: the discrete
// decisions of the reference sit on margins down to 4e-16).
#include <hip/hip_runtime.h>
#include <mutex>
#include <new>

#include "pve_host.h"
#include "pve_tick_core.h"
#include "pve_tick_geo.h"
#include "pve_actor.h"
#include "pve_critic.h"
#include "pve_nstep.h"
#include "pve_replay.h"
#include "pve_prio.h"
#include "pve_arrivals.h"
#include "pve_stats.h"
#include "pve_learn.h"

using namespace pve;

// A/B knobs of the measurement tooling (tools/ab_launch_shapes.py, tools/gpu.sh): environment variables that switch launch
// shapes.  Compiled in only with -DPVE_AB_KNOBS (`make knobs` -> build/libpveenv_knobs.so); the product library reads no
// environment variable on its launch path.
#ifdef PVE_AB_KNOBS
#define PVE_KNOB(name_) getenv(name_)
static constexpr bool knobs_built = true;
#else
#define PVE_KNOB(name_) ((const char *)nullptr)
static constexpr bool knobs_built = false;
#endif
// the HOME build of the persistent table-source kernel (k_rollout<128, 5, ..>, 10 workgroups per CU) is what pick_rollout
// takes when it is eligible; -DPVE_HOME_DEFAULT=0 builds a library that keeps the 8-workgroup kernel (A/B)
#ifndef PVE_HOME_DEFAULT
#define PVE_HOME_DEFAULT 1
#endif

typedef __attribute__((address_space(4))) const char *KernargPtr;
// diagnostics (pve_debug_phase_cycles): every wave keeps the clock ticks it spent in each phase (incl. the
// wait at the closing barrier) in registers and adds them to its private row of a [n_waves][16] device
// buffer at the end of the kernel (no shared atomics, no extra memory traffic inside the phases)
#define PVE_PHASE_MARK(idx)                                                              \
    if (P.phase_cycles) {                                                                \
        unsigned long long now_ = wall_clock64();                                        \
        pc_[idx] = now_ - tprev_;                                                        \
        tprev_ = now_;                                                                   \
    }

// The workgroup barrier between two phases.  __syncthreads() = workgroup-scope release + s_barrier + acquire; on gfx950
// outside threadgroup-split mode this compiles to `s_waitcnt lgkmcnt(0)` + `s_barrier` (checked in the ISA): LDS accesses
// are ordered, and so are the global accesses of the workgroup's waves (one CU, one in-order vector-memory path) WITHOUT
// a vmcnt(0) -- prefetches and the output stores of one tick stay in flight across the phases of the next.
__device__ __forceinline__ void lds_barrier() { __syncthreads(); }
// CAP = 128: 5 waves per SIMD (<= 96 VGPR) + the 15.1 KB LDS block = 10 workgroups of 128 threads per CU instead of 8: with
// the sub-batches pipelined on several streams the tick scales almost linearly with the resident workgroups.
// CAP = 64: one wave per workgroup, LDS (10 KB) admits 16 workgroups per CU = 4 waves per SIMD (<= 128 VGPR).
// CAP = 256: four waves per workgroup and a ~32 KB block: LDS admits 5 workgroups per CU = 5 waves per SIMD; held to 4 waves per
// SIMD (<= 128 VGPR, the budget of the 128-slot register build) so that the wider masks do not spill.
template <int CAP>
__global__ __launch_bounds__(CAP) __attribute__((amdgpu_waves_per_eu(CAP == 128 ? 5 : 4, CAP == 128 ? 5 : 4))) void k_tick(const Const c_arg, const Params P_arg)
{
    KernargPtr ka0_ = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const PVE_AS4 Const &c = *(const PVE_AS4 Const *)ka0_;
    const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka0_ + ((sizeof(Const) + 7) / 8 * 8));
    typedef Shared<CAP, false> ShT;                  // (without the lane << 16 | j words: 16 368 B, the 10th workgroup per CU)
    __shared__ ShT sh;
    const int t = threadIdx.x;
    const int env = blockIdx.x;
    Regs r;
    typedef Tick<CAP, ShT> T;
    unsigned long long pc_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev_ = P.phase_cycles ? wall_clock64() : 0ull;
    T::ph_load(c, P, env, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(0)
    if (P.stop_phase == 0) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_step1(c, P, env, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(1)
    if (P.stop_phase == 1) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_step2(c, t, sh, r);
    T::ph_lists_a(c, t, sh);
    lds_barrier();
    PVE_PHASE_MARK(2)
    if (P.stop_phase == 2) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_step3(c, t, sh, r);
    T::ph_step3_publish(t, sh, r);
    T::ph_lists_b(t, sh);
    lds_barrier();
    PVE_PHASE_MARK(3)
    if (P.stop_phase == 3) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_build(c, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(4)
    if (P.stop_phase == 4) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_rank(t, sh, env);
    lds_barrier();
    PVE_PHASE_MARK(5)
    if (P.stop_phase == 5) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_scan(c, t, sh, r);
    PVE_PHASE_MARK(11)
    T::ph_reward(c, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(6)
    if (P.stop_phase == 6) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_effects(c, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(7)
    if (P.stop_phase == 7) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_prefetch_arrival(P, env, t, sh, r, NL);
    T::ph_lock(c, t, sh, r);
    lds_barrier();
    T::ph_lock2(t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(8)
    if (P.stop_phase == 8) return;          // (diagnostics, uniform: pve_debug_stop_phase)
    T::ph_final(c, P, env, t, sh, r);
    PVE_PHASE_MARK(9)
    if (P.out.state_pre) {            // uniform branch: optional training output
        __threadfence_block();
        __syncthreads();
        if constexpr (CAP <= 128) {
            T::ph_state_publish(P.out, t, sh, r);
            __syncthreads();
            T::ph_state_coop(P, P.out, env, t, sh);
        } else T::ph_state(P, env, t, sh, r);        // (256 slots: the byte descriptors cannot name slots >= 128)
        PVE_PHASE_MARK(10)
    }
    if (P.phase_cycles && (t & 63) == 0) {
        unsigned long long *row = P.phase_cycles + ((size_t)env * (CAP / 64) + (t >> 6)) * 16;
#pragma unroll
        for (int k = 0; k < 12; k++) row[k] += pc_[k];
    }
}

// k_rollout<.., ACT>: the actor pass of one resident tick (behind STAGE: the carried state lives in the staging arrays, the
// registers are free).  The controlled vehicles are the dense threads 0 .. n_ctl-1 -- normally all of them in wave 0, whose
// chain is the workgroup's critical path -- so the work is split by TILE, not by owner: tile i = dense threads 32 i .. 32 i
// + 31 goes to wave i % (CAP / 64).  A tile's rows are the float32 images of what FIN stored to obs_post a moment ago (same
// CU: L1 / L2 hot, ordered by barrier A), addressed through the post-compaction slots the dense threads left in `adsts`
// (SLOT_NONE<CAP> = the vehicle is gone); lane (j, hf) fetches the half row it contracts.  act[slot] receives the action of every
// controlled vehicle that keeps a slot.  The launch's first tick uses the same routine on the rows in HBM.
template <int CAP>
__device__ __forceinline__ void rollout_actor(const unsigned char *packed, const float *aprm, double *act, const slot_t<CAP> *adsts,
                                              int n_ctl, const void *rows, bool obs_f32, size_t base, int t)
{
    const pve_v8h *A1 = (const pve_v8h *)(packed + AP_A1), *A2 = (const pve_v8h *)(packed + AP_A2);
    const int lane = t & 63, hf = lane >> 5, j = lane & 31;
    for (int tile = t >> 6; 32 * tile < n_ctl; tile += CAP / 64) {          // (uniform per wave)
        const int slot = adsts[32 * tile + j];
        const int srow = slot == SLOT_NONE<CAP> ? 0 : slot;
        float x[16];
        if (obs_f32) actor_fetch_env((const float *)rows + base * OBSW, srow, hf, x);
        else actor_fetch_env((const double *)rows + base * OBSW, srow, hf, x);
        const float a = actor_tile32(A1, A2, aprm, x, lane);
        if (lane < 32 && slot != SLOT_NONE<CAP>) act[slot] = (double)a;
    }
}

// k_rollout<.., ACT> / k_rollout_geo<.., ACT>: the exploration noise of pve_set_action_noise (pve_noise.h; main.py:44), added at the
// intake of a tick -- the slot's own thread holds this tick's action (from LOAD, RELOAD or the queue's hand-off buffer, which
// therefore keeps clean actor outputs), the vehicle's id and its controlled bit, and nothing else of the tick is live yet.
// `tick` = the tick's index within the call; the same float64 expression as the stand-alone kernels (actor_commanded), so every
// launch form commands the same bits.  The test on sigma is uniform: with the noise off a tick pays one scalar compare.
__device__ __forceinline__ void rollout_noise(const PVE_AS4 RolloutArgsNoisy &R, int env, int tick, Regs &r)
{
    const double sigma = R.noise.sigma;
    if (__builtin_expect(sigma != 0, 0)) {          // (laid out behind the loop: with the noise off the tick's code stays contiguous)
        if (r.alive && (r.meta & M_CONTROL))
            r.act = r.act + sigma * action_noise_z(R.noise.seed, (int64_t)env + R.noise.env_offset, r.id, R.noise.tick0 + (uint32_t)tick);
    }
}

// PVE_SRC_TABLE: table[row][min(id, table_ids - 1)] -- a UNIFORM 64-bit row base plus a 32-bit lane offset (the `saddr + voffset`
// form of a global load; the plain index is a sign extension + 64-bit multiply-add per lane); the unsigned minimum also clamps a
// negative id (an empty slot, whose value is never used)
__device__ __forceinline__ double table_action(const double *table, int row, int table_ids, int id)
{
    const unsigned col = (unsigned)id < (unsigned)table_ids ? (unsigned)id : (unsigned)(table_ids - 1);
    return *(const double *)((const char *)(table + (size_t)row * (size_t)table_ids) + col * 8u);
}

// ------------------------------------------------------------------ persistent roll-out: the work queue
// One launch for a whole pve_step_many call: as many workgroups as the chip holds at once, each pulling (intersection,
// chunk) items -- chunk c of intersection e = ticks [c T, (c + 1) T) of the call -- until the call is done.  Nothing waits in
// launch order for the slowest intersection of a chunk; an item only waits for the previous chunk of ITS intersection.
//
// Hand-off of an intersection between two workgroups (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement &
// inter-workgroup visibility"): the eight XCDs' L2s are not coherent with each other and a CU's vector L1 is never
// refreshed by another CU's stores.  So (1) every intersection is worked by ONE XCD for the whole launch: env e belongs to
// shard e % n_shards, and a shard belongs to the first XCD -- HW_REG_XCC_ID as read by the executing wave, not an
// assumption about dispatch -- whose workgroup claims it (compare-and-swap on owner[]; an XCD starts with the shard of
// its own number and adopts what nobody has claimed once that is exhausted, so every shard is worked whatever the
// placement).  All stores to an intersection's state AND to its output rows (which successive ticks overwrite) then
// meet in one L2, in program order of the workgroups that are ordered by the done[] hand-off; (2) the finishing workgroup
// drains its stores (`s_waitcnt vmcnt(0)` in every wave: the write-through L1 has handed them to the L2), joins at a
// barrier and publishes done[e] with an agent-scope atomic store; (3) the next workgroup polls done[e] with agent-scope
// atomic loads (one lane, `s_sleep` between polls), joins at a barrier and reads the state with agent-scope atomic
// loads (`sc1`: served by the L2, never by its own L1).  Queue heads and done[] are agent-scope atomics throughout.
// Items of a shard are handed out chunk-major (all intersections' chunk c before any chunk c + 1) by a returning
// atomic add, so whoever holds an item is a RUNNING workgroup and the item it may wait for was handed out earlier:
// the oldest unfinished item never waits, whatever the grid size or whoever shares the chip.
// diagnostics build only (make EXTRA=-DPVE_QUEUE_TRACE, tools/persistent_trace.py): per-item timestamps; compiled out of the
// product library (the extra live values cost the one-wave variant 32 spilled registers)
#ifdef PVE_QUEUE_TRACE
#define Q_TRACE(R_) ((R_).q_trace)
#else
#define Q_TRACE(R_) ((unsigned long long *)nullptr)
#endif
__device__ __forceinline__ unsigned q_xcc_id()
{
    return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 0xFu;      // HW_REG_XCC_ID[3:0] (gfx942 / gfx950)
}
__device__ __forceinline__ unsigned q_load(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void q_store(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// one lane: the next item of this workgroup's XCD -> (env, chunk), env < 0 when the call has no work left for it.
// `shard` / `probe` persist across calls (the shard being worked, the number of shards this workgroup has looked at).
__device__ __forceinline__ void q_dequeue(RolloutQueue *Q, int n_shards, int n_envs, int n_chunks, unsigned xcc, int &shard, int &probe,
                                          int &env, int &chunk)
{
    for (;;) {
        if (shard >= 0) {
            const unsigned es = (unsigned)(n_envs - shard + n_shards - 1) / (unsigned)n_shards;   // intersections of the shard
            const unsigned i = __hip_atomic_fetch_add(&Q->s[shard].head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (i < es * (unsigned)n_chunks) {
                const unsigned c = i / es;
                env = shard + (int)(i - c * es) * n_shards; chunk = (int)c;
                return;
            }
        }
        // the shard is exhausted (or this is the first call): the next shard this XCD may work -- its own number first.
        // Loads before atomics: at the end of a call every workgroup comes through here, and a compare-and-swap per
        // workgroup and shard on lines the running workgroups' XCDs share is a flood (measured: the last items of a call ran
        // 1.4x slower under it)
        shard = -1;
        while (probe < n_shards) {
            const int cand = (int)((xcc + (unsigned)probe) % (unsigned)n_shards);
            probe++;
            if (cand >= n_envs) continue;
            unsigned seen = q_load(&Q->s[cand].owner);
            if (seen == 0u)
                __hip_atomic_compare_exchange_strong(&Q->s[cand].owner, &seen, xcc + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen != 0u && seen != xcc + 1u) continue;          // another XCD's
            const unsigned es = (unsigned)(n_envs - cand + n_shards - 1) / (unsigned)n_shards;
            if (q_load(&Q->s[cand].head) >= es * (unsigned)n_chunks) continue;      // ours, but handed out already
            shard = cand;
            break;
        }
        if (shard < 0) { env = -1; chunk = 0; return; }
    }
}

// The workgroup's next item: lane 0 pulls it and waits for the previous chunk of its intersection (another workgroup's item);
// everybody learns it through q_word (LDS).  -> false when the call has no work left for this workgroup's XCD.
// q_word[0..1] = (env, chunk), [2..3] = lane 0's dequeue state (shard, shards looked at).
__device__ __forceinline__ bool q_take(const PVE_AS4 RolloutArgs &R, int n_envs, int t0, int *q_word, int &env, int &chunk, int &k_base,
                                       int &n_ticks)
{
    RolloutQueue *Q = (RolloutQueue *)R.queue;
    unsigned *done = R.queue + sizeof(RolloutQueue) / 4;
    if (t0 == 0) {
        int shard = q_word[2], probe = q_word[3], e, ch;
        const unsigned long long tq0 = Q_TRACE(R) ? wall_clock64() : 0ull;
        q_dequeue(Q, R.n_shards, n_envs, R.n_full + R.n_taper, q_xcc_id(), shard, probe, e, ch);
        q_word[0] = e; q_word[1] = ch; q_word[2] = shard; q_word[3] = probe;
        const unsigned long long tq1 = Q_TRACE(R) ? wall_clock64() : 0ull;
        if (e >= 0)                                   // the previous chunk of this intersection (another workgroup's item)
            while ((int)(q_load(&done[e]) - (R.done_base + (unsigned)ch)) < 0) __builtin_amdgcn_s_sleep(8);
        if (Q_TRACE(R) && e >= 0) {                    // diagnostics: dequeue start, item known, predecessor done, who
            unsigned long long *row = Q_TRACE(R) + ((size_t)ch * n_envs + e) * 8;
            row[0] = tq0; row[1] = tq1; row[2] = wall_clock64();
            row[6] = (unsigned long long)blockIdx.x | ((unsigned long long)q_xcc_id() << 32);
        }
    }
    __syncthreads();
    env = __builtin_amdgcn_readfirstlane(q_word[0]);
    chunk = __builtin_amdgcn_readfirstlane(q_word[1]);
    if (env < 0) return false;
    rollout_item(R, chunk, k_base, n_ticks);
    return true;
}
// hand the intersection on: every wave's stores (state, header, the ticks' output rows) have reached the L2, then the count of
// completed items of this intersection goes up by one
__device__ __forceinline__ void q_publish(const PVE_AS4 RolloutArgs &R, int n_envs, int t0, int env, int chunk)
{
    const unsigned long long tf0 = (Q_TRACE(R) && t0 == 0) ? wall_clock64() : 0ull;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t0 == 0) q_store(R.queue + sizeof(RolloutQueue) / 4 + env, R.done_base + (unsigned)chunk + 1u);
    if (Q_TRACE(R) && t0 == 0) {                      // diagnostics: state flushed (stores issued), handed on
        unsigned long long *row = Q_TRACE(R) + ((size_t)chunk * n_envs + env) * 8;
        row[4] = tf0; row[5] = wall_clock64();
    }
}
// the last workgroup to leave clears the queue words for the next launch (done[] stays: it is cumulative)
__device__ __forceinline__ void q_leave(const PVE_AS4 RolloutArgs &R, int t0)
{
    RolloutQueue *Q = (RolloutQueue *)R.queue;
    if (t0 == 0) {
        const unsigned left = __hip_atomic_fetch_add(&Q->exits, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (left + 1u == gridDim.x) {
            for (int k = 0; k < QUEUE_MAX_SHARDS; k++) { q_store(&Q->s[k].head, 0u); q_store(&Q->s[k].owner, 0u); }
            q_store(&Q->exits, 0u);
        }
    }
}

// pve_step_many: R.n_ticks ticks of one intersection per workgroup, the state resident in registers / LDS between the
// ticks (pve_tick_core.h, "k_rollout").  Per tick only the outputs go to HBM; the action of the next tick (pool) and
// the next arrival times are prefetched under the tail of the current one.
// WPE = waves per SIMD the register allocation is held to: 4 (<= 128 VGPR, no spills: 8 workgroups of 128 threads per CU,
// i.e. 4096 intersections in exactly two rounds) or 5 (<= 96 VGPR, 10 per CU for stream-pipelined sub-batches).
// PROF: the diagnostics build (pve_debug_phase_cycles) accumulates per-phase clock ticks over the ticks of the launch.
// ACT: pve_step_many(PVE_SRC_ACTOR) -- the closed loop of main.py:398-441 resident on the chip.  The dense thread of every
// controlled vehicle keeps the float32 observation row it has just built in FIN; behind STAGE (the carried state lives in
// the staging arrays by then, the registers are free) the wave runs the actor on its <= 2 tiles of 32 vehicles
// (pve_actor.h: actor_tile32, the same function the stand-alone k_actor_h calls), A operands streamed from L1 / L2, the
// float parameters in 2 KB of LDS, and deposits next tick's actions where RELOAD looks for them (act_next).  No new
// barrier; still ticks are staged like the others.  The first tick of a launch takes its rows from HBM.
// TRAIN: the training outputs (obs_pre, state_pre: SURVEY 8 f3) are written per tick; a variant of its own so that the
// default kernel keeps its register allocation (123 VGPR, no scratch).
// IDT: PVE_SRC_TABLE -- the action is a function of (tick, vehicle id) given as a table: every vehicle's own thread gathers
// its next action under FX (the id travels with the vehicle), the lanes that spawn gather theirs right behind FIN (in flight
// under barrier A and STAGE), and the values are parked at the vehicles' NEW slots (act_next) where RELOAD looks for them.
// PERS: the persistent form -- the workgroup pulls (intersection, chunk) items from the queue above; n_ticks = ticks per item.
template <int CAP, int WPE, bool PROF = false, bool ACT = false, bool TRAIN = false, bool IDT = false, bool PERS = false>
__global__ __launch_bounds__(CAP) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_rollout(const Const c_arg, const Params P_arg,
                                                                                               const typename rollout_args<ACT>::type R_arg)
{
    typedef typename rollout_args<ACT>::type RArgs;      // (ACT: RolloutArgs + the exploration noise)
    static_assert(!PERS || !PROF, "the persistent form has no phase-cycle diagnostics variant");
    static_assert(!(ACT && IDT), "one action source per variant");
    // NODRAIN: no global load is pending when a tick issues its first output store, so the wave executes no vmcnt wait from
    // there until the next tick consumes its own prefetches.  Not the ACT / TRAIN variants, which read rows back
    // from global memory within the tick.
    constexpr bool NODRAIN = !ACT && !TRAIN;
    KernargPtr ka0_ = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr size_t OFF_P = (sizeof(Const) + 7) / 8 * 8, OFF_R = OFF_P + (sizeof(Params) + 7) / 8 * 8;
    // (WPE = 5, the 96-VGPR experiment: the block without the lane << 16 | j words is 16 368 B -> 10 workgroups per CU)
    // (WPE = 5 also: HOME -- the carried per-slot fields live in LDS instead of registers, pve_tick_core.h)
    // (the HOME block without the lane << 16 | j words: with them it is 16 896 B = 9 workgroups per CU, measured 24.75 against
    //  24.78 us -- 9 and 10 resident workgroups per CU run at the same rate, the words buy nothing there)
    typedef Shared<CAP, (CAP == 128 && WPE == 4), (WPE == 5)> ShT;
    __shared__ ShT sh;
    constexpr bool PARK = NODRAIN && ShT::HOME;
    static_assert(!PARK || 2 * CAP + 2 * NL <= ShT::POOL, "PARK: 2 NL doubles behind the staged jerks in u_vd");
    __shared__ __attribute__((aligned(64))) float aprm[ACT ? PV_TOTAL : 1];
    __shared__ slot_t<CAP> adsts[ACT ? CAP : 1];     // post-compaction slot of every dense thread's vehicle (SLOT_NONE: gone)
    __shared__ int q_word[4];                       // PERS: item (env, chunk) of the workgroup + the dequeue state of lane 0
    int adst = -1;
    int t0_ = threadIdx.x;
    int env0_ = PERS ? 0 : blockIdx.x;
    int k_base_ = 0, chunk_ = 0;                     // PERS: first tick of the item within the call, its chunk number
    bool aprm_staged = false;                        // PERS + ACT: the float parameters are in LDS (once per workgroup)
    // the first wave carries the dense-mapped phases (the critical chain of the workgroup), the second one mostly waits at
    // the barriers: the first wave gets the issue slots first (30.0 -> 29.6 us per tick; not in k_tick, where the closed
    // loop's actor kernel shares the chip and loses more than the tick gains)
    // (round 6, the HOME build with its 5 waves per SIMD: the second wave at 2 instead of 0 -- whatever it runs is what the first wave
    //  waits for at the next barrier: 22.83 vs 22.95 us steady; 3 / 3 and 2 / 3 are worse: 23.1 / 23.45)
    if (CAP > 64) { if (__builtin_amdgcn_readfirstlane(t0_) < 64) __builtin_amdgcn_s_setprio(3); else if (WPE == 5) __builtin_amdgcn_s_setprio(2); }
    KernargPtr kav_ = ka0_;
    Regs r;
    FinCarry fc;
    typedef Tick<CAP, ShT> T;
    unsigned long long pc_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev_ = PROF ? wall_clock64() : 0ull;
    const unsigned long long sclk0_ = PROF ? clock64() : 0ull, wclk0_ = tprev_;   // shader clock vs the 100 MHz constant clock
#undef PVE_PHASE_MARK
#define PVE_PHASE_MARK(idx)                                                              \
    if (PROF) {                                                                          \
        unsigned long long now_ = wall_clock64();                                        \
        pc_[idx] += now_ - tprev_;                                                       \
        tprev_ = now_;                                                                   \
    }
    int pool_idx, n_ticks;
    if constexpr (PERS) { if (t0_ == 0) { q_word[2] = -1; q_word[3] = 0; } }
  for (;;) {                                        // PERS: one pass per item; else exactly one pass
    {
        const PVE_AS4 Const &c = *(const PVE_AS4 Const *)ka0_;
        const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka0_ + OFF_P);
        const PVE_AS4 RArgs &R = *(const PVE_AS4 RArgs *)(ka0_ + OFF_R);
        pool_idx = R.pool_tick0;
        n_ticks = R.n_ticks;
        const double *act0 = nullptr;
        if constexpr (PERS) {
            int e, ch, kb, nt;
            if (!q_take(R, P.n_envs, t0_, q_word, e, ch, kb, nt)) break;
            env0_ = e; chunk_ = ch; k_base_ = kb; n_ticks = nt;
            if (R.source == 1 || R.source == 3) pool_idx = (R.pool_tick0 + k_base_) % R.n_pool;
            if (R.source == 1) act0 = R.pool + (size_t)pool_idx * (size_t)P.n_envs * CAP;
        }
        // PERS + ACT: only the FIRST item of an intersection in a call computes its first actions from the caller's rows; every
        // later item takes them from `actor_actions`, where the previous item left them (its last tick ran the actor too)
        bool act_handed = false;
        if constexpr (PERS && ACT) {
            act_handed = chunk_ > 0;
            if (act_handed) act0 = R.actor_actions;      // ([n_envs][CAP], like a pool entry: LOAD adds the intersection's offset)
        }
        if constexpr (ACT) if (!act_handed) {
            // the first tick's actions = actor(rows in HBM), before the state is loaded (nothing else is live): the controlled
            // slots are compacted into `adsts` as if they were dense threads (wave 1's ranks follow wave 0's count)
            if (!PERS || !aprm_staged) {
                const float *gp = (const float *)(R.actor_packed + AP_PRM);
                for (int n = t0_; n < PV_TOTAL; n += CAP) aprm[n] = gp[n];
            }
            const int mt = P.i32[I_META][(size_t)env0_ * CAP + t0_];
            const bool cc = (mt & (M_ALIVE | M_CONTROL)) == (M_ALIVE | M_CONTROL);
            vote<CAP / 64>(sh.m_ctl, t0_, cc);
            adsts[t0_] = (slot_t<CAP>)SLOT_NONE<CAP>;  // (entries beyond the controlled count: no vehicle)
            lds_barrier();
            if (cc) adsts[mask_rank<CAP / 64>(sh.m_ctl, t0_)] = (slot_t<CAP>)t0_;
            const int nc = mask_count<CAP / 64>(sh.m_ctl);
            lds_barrier();                               // parameters staged, list complete
            rollout_actor<CAP>(R.actor_packed, aprm, sh.act_next, adsts, nc, R.actor_obs, P.obs_f32 != 0, (size_t)env0_ * CAP, t0_);
            lds_barrier();
        }
        if constexpr (PERS && ACT) {
            if (!aprm_staged && act_handed) {            // (a workgroup whose first item is a later chunk: parameters for its ticks)
                const float *gp = (const float *)(R.actor_packed + AP_PRM);
                for (int n = t0_; n < PV_TOTAL; n += CAP) aprm[n] = gp[n];
            }
            aprm_staged = true;
        }
        if constexpr (PERS) {
            T::template ph_load<true, ACT>(c, P, env0_, t0_, sh, r, act0, true);
            if (Q_TRACE(R) && t0_ == 0) Q_TRACE(R)[((size_t)chunk_ * P.n_envs + env0_) * 8 + 3] = wall_clock64();
        } else T::ph_load(c, P, env0_, t0_, sh, r);     // P.actions = the first tick's actions
        if constexpr (ACT) { if (!act_handed) r.act = sh.act_next[t0_]; }   // (uncontrolled slots: whatever is there, masked in S1)
        if constexpr (IDT) {                            // the first tick's action of the vehicle in this slot: table[row][id]
            r.act = r.alive ? table_action(R.pool, pool_idx, R.table_ids, r.id) : 0.0;
        }
        T::ph_home_store(t0_, sh, r);                   // (HOME: the carried fields to their LDS homes; ordered by the loop's first barrier)
        // NODRAIN: everything LOAD has requested is consumed in front of the loop.  A register of a load that may still be pending
        // at the loop's head gets its `s_waitcnt vmcnt` INSIDE the loop, where from the second tick on it waits for nothing but
        // the previous tick's output stores (one counter for loads and stores, in issue order)
        if constexpr (NODRAIN) {
            PVE_PIN(r.alive); PVE_PIN(r.meta); PVE_PIN(r.step); PVE_PIN(r.act);
            if constexpr (!ShT::HOME) {
                PVE_PIN(r.p); PVE_PIN(r.v); PVE_PIN(r.a); PVE_PIN(r.jerk_sum); PVE_PIN(r.vir_dis); PVE_PIN(r.closer_p);
                PVE_PIN(r.id); PVE_PIN(r.seq); PVE_PIN(r.vnum); PVE_PIN(r.count);
            }
        }
    }
    double sp_act = 0;                                  // IDT: the action of the vehicle this lane spawns
    for (int k = 0; k < n_ticks; k++) {
        // The loop body is one tick of the single-tick kernel.  Without the two opaque copies below the compiler's
        // loop-invariant code motion hoists every kernel-argument load and every per-thread address out of the loop
        // (~150 scalar + ~140 vector registers live across the whole tick -> spills / 2 waves per SIMD).
        // (the SAME variables are re-defined every iteration: a loop-carried value in one register, not an invariant plus a copy)
        // (PERS: the item's intersection travels through the outer loop's phi, which the compiler keeps in a vector register)
        if constexpr (PERS) env0_ = __builtin_amdgcn_readfirstlane(env0_);
        asm volatile("" : "+s"(kav_), "+v"(t0_), "+s"(env0_));
        const KernargPtr ka = kav_;
        const int t = t0_, env = env0_;
#ifndef PVE_NO_RANGE_ASSUME                        // (A/B build knob)
        // the opaque copy hides the range of t: with it the index arithmetic stays in 24 / 32 bits
#ifdef PVE_ASSUME_ONE_WAVE_ONLY                    // (A/B build knob)
        if constexpr (CAP == 64)
#endif
        __builtin_assume(t >= 0 && t < CAP);
#endif
        const PVE_AS4 Const &c = *(const PVE_AS4 Const *)ka;
        const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka + OFF_P);
        const PVE_AS4 RArgs &R = *(const PVE_AS4 RArgs *)(ka + OFF_R);
        lds_barrier();
        PVE_PHASE_MARK(0)
        if constexpr (CAP == 64 && !PERS) {
            // One wave per intersection, every intersection of the launch resident at once: the launch lasts as long as its
            // SLOWEST intersection (the one with the most vehicles: +-15 % over the 20 ticks of a short call), and nothing can be
            // re-balanced between workgroups.  So the waves of the crowded intersections get the issue slots first (uniform, one
            // scalar instruction per tick): they run at nearly their solo speed, the light ones -- which finish early anyway --
            // yield.  Thresholds: quartiles of the population at BASELINE config 2's load (31 vehicles on average).
            const int na = __builtin_amdgcn_readfirstlane(sh.hd.n_alive);
#ifndef PVE_NO_LOAD_PRIO                          // (A/B build knob)
            if (na > 38) __builtin_amdgcn_s_setprio(3);
            else if (na > 32) __builtin_amdgcn_s_setprio(2);
            else if (na > 26) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
#endif
        }
        if (k > 0) T::ph_tick_init(c, t, sh, r);
        if constexpr (ACT) rollout_noise(R, env, k_base_ + k, r);
        T::ph_step1(c, P, env, t, sh, r);
        lds_barrier();
        PVE_PHASE_MARK(1)
        T::ph_step2(c, t, sh, r);
        T::ph_lists_a(c, t, sh);
        lds_barrier();
        PVE_PHASE_MARK(2)
        const bool last_tick = k + 1 == n_ticks;      // (uniform)
        T::ph_step3(c, t, sh, r, last_tick);
        T::ph_step3_publish(t, sh, r);
        T::ph_lists_b(t, sh);
        lds_barrier();
        PVE_PHASE_MARK(3)
        if constexpr (ShT::HOME) {
            // the 304-entry pool: BUILD .. WALK in passes over groups of lists that fit it (one pass unless the intersection
            // holds ~100 controlled vehicles; pve_tick_core.h, group_end)
            T::ph_build_prep(c, t, sh, r);
            T::ph_scan_init(r);
            if (__builtin_amdgcn_readfirstlane((int)sh.loff[NL]) <= ShT::POOL) {      // (uniform; the rule: every list in ONE pass,
                T::template ph_build_fill<false>(c, t, sh, r, 0, NL);                 //  the very code of the 5 CAP blocks)
                lds_barrier();
                T::template ph_rank<false>(t, sh);
                lds_barrier();
                T::template ph_scan_lists<false>(c, t, sh, r, 0, NL);
            } else
            for (int d0 = 0, pass = 0; d0 < NL; pass++) {
                const int d1 = __builtin_amdgcn_readfirstlane(T::group_end(sh, d0));
                T::template ph_build_fill<true>(c, t, sh, r, d0, d1);
                lds_barrier();
                T::template ph_rank<true>(t, sh, pass, d0, d1);
                lds_barrier();
                T::template ph_scan_lists<true>(c, t, sh, r, d0, d1);
                d0 = d1;
                if (d0 < NL) lds_barrier();           // (the next pass files its entries over the lists this one has just read)
            }
        } else {
        T::ph_build(c, t, sh, r);
        lds_barrier();
        PVE_PHASE_MARK(4)
        T::ph_rank(t, sh);
        lds_barrier();
        PVE_PHASE_MARK(5)
        T::ph_scan(c, t, sh, r);
        }
        PVE_PHASE_MARK(11)
        T::ph_reward(c, t, sh, r);
        lds_barrier();
        PVE_PHASE_MARK(6)
        int nx = -1;
        if (k + 1 < n_ticks) { pool_idx = (pool_idx + 1 == R.n_pool) ? 0 : pool_idx + 1; nx = pool_idx; }
        if constexpr (IDT) {
            int my_id = r.id;
            if constexpr (ShT::HOME) my_id = sh.h_id[t];
            r.act_nx = (nx >= 0 && r.alive) ? table_action(R.pool, nx, R.table_ids, my_id) : 0.0;
        } else T::ph_prefetch_action(P, R, env, t, nx, r);
        T::ph_effects(c, t, sh, r);
        lds_barrier();
        PVE_PHASE_MARK(7)
        T::ph_prefetch_arrival(P, env, t, sh, r, NL);
        bool sp_late = false;                         // IDT: the intersection is full, FIN decides who spawns (uniform, rare)
        if constexpr (IDT) {
            // the first action of the vehicle lane t spawns at the end of this tick: the spawn votes are complete since the
            // barrier behind FX and, unless the intersection is full, every lane that wants to spawn does (ph_final), so its id
            // is known HERE -- the gather flies under LOCK .. FIN instead of sitting between FIN and STAGE
            const unsigned want = (unsigned)(sh.m_spawn[0] & 0xFFFull);
            sp_late = __builtin_popcount(want) > CAP - sh.hd.n_alive;
            sp_act = 0;
            if (t < NL && nx >= 0 && !sp_late && ((want >> t) & 1u))
                sp_act = table_action(R.pool, nx, R.table_ids, sh.hd.id_seq + __builtin_popcount(want & ((1u << t) - 1u)));
        }
        T::ph_lock(c, t, sh, r, last_tick);
        lds_barrier();
        T::ph_lock2(t, sh, r, last_tick);
        T::ph_keep_prefix(t, sh);
        lds_barrier();                                // (also what orders the previous tick's output stores before this tick's)
        PVE_PHASE_MARK(8)
        // NODRAIN: the tick's prefetches are consumed HERE, in every lane (0 / +inf where nothing was loaded), in front of FIN's
        // first output store: they were requested two barriers and the dead-lock scan ago, behind stores a whole tick old.  A
        // load still pending behind a store makes its consumer wait for the store's acknowledgement too.
        // PARK (HOME: no register to spare across the observation rows): the values wait in LDS instead -- the action in the
        // slot's own act_next[] cell (ph_lock2 has read the jerk it may have held), the spawn's action and the arrival time in
        // u_vd[2 CAP ..), which nothing uses between WALK and the next tick's BUILD
        if constexpr (NODRAIN) {
            PVE_PIN(r.next_arr); PVE_PIN(r.act_nx);
            if constexpr (IDT) PVE_PIN(sp_act);
            if constexpr (PARK) {
                if constexpr (IDT) sh.act_next[t] = r.act_nx;
                if (t < NL) { sh.u_vd[2 * CAP + t] = r.next_arr; if constexpr (IDT) sh.u_vd[2 * CAP + NL + t] = sp_act; }
            }
        }
        if constexpr (!ACT && !IDT) { if (!(ShT::HOME && last_tick)) T::ph_park_action(t, sh, r); }   // (HOME, last tick: the cells hold the jerks)
        const Outputs O = T::template tick_outputs<TRAIN>(P, R, k_base_ + k);
        if constexpr (ACT) {
            adst = -1;
            T::template ph_final<true>(c, P, O, env, t, sh, r, fc, true, &adst);
            adsts[t] = (slot_t<CAP>)(adst < 0 ? SLOT_NONE<CAP> : adst);  // (dense thread t; threads >= n_ctl: SLOT_NONE)
        } else T::template ph_final<true, !TRAIN>(c, P, O, env, t, sh, r, fc, k + 1 == n_ticks || (TRAIN && O.state_pre != nullptr));
        PVE_PHASE_MARK(9)
        double act_mv = 0;                            // PARK + IDT: the parked action on its way to the vehicle's new slot
        if constexpr (IDT) {
            // (PARK: a still tick leaves the action where S1 looks for it; else it follows the vehicle like the homes do)
            if constexpr (PARK) { if (!fc.still) act_mv = sh.act_next[t]; }
            else if (fc.new_slot >= 0) sh.act_next[fc.new_slot] = r.act_nx;   // (act_next = xy32: dead since REWARD)
            // (a full intersection: who spawns is known since FIN only)
            if (sp_late) {
                sp_act = (fc.sp_slot >= 0 && nx >= 0) ? table_action(R.pool, nx, R.table_ids, fc.sp_id) : 0.0;
                // (NODRAIN: waited for inside the rare branch -- merged with the common path, STAGE's use of sp_act would carry the
                //  wait, and with it a drain of FIN's stores, into every staged tick)
                if constexpr (NODRAIN) PVE_PIN(sp_act);
                if constexpr (PARK) { if (t < NL) sh.u_vd[2 * CAP + NL + t] = sp_act; }
            }
        }
        HomeRegs hr;
        T::ph_home_take(t, sh, r, fc, hr);                 // (HOME; the last reads of the old arrangement)
        if (fc.still) {                               // (uniform) nobody moves: the registers carry over
            T::ph_stage_header(t, sh, fc);
            T::ph_carry_over(t, sh, r, fc);
        } else {
            lds_barrier();                            // A: nobody reads the tick's work arrays any more
            // (uniform; barrier A also orders the obs_pre rows of this tick.  PERS: the stale rows of an item's first tick are what
            //  ANOTHER workgroup's item stored -- block k - 1 of the trajectory --: coherent loads)
            if constexpr (TRAIN) {
                if (O.state_pre) {                       // (uniform) the 7 x 28 states: descriptors, barrier, cooperative write
                    if constexpr (CAP <= 128) {
                        T::ph_state_publish(O, t, sh, r);
                        lds_barrier();
                        T::template ph_state_coop<PERS>(P, O, env, t, sh);
                    } else T::template ph_state<PERS>(P, O, env, t, sh, r);   // (256 slots: per thread, cf. k_tick)
                }
            }
            if constexpr (PARK) { if (fc.sp_slot >= 0) { r.next_arr = sh.u_vd[2 * CAP + t]; if constexpr (IDT) sp_act = sh.u_vd[2 * CAP + NL + t]; } }
            T::ph_stage(c, t, sh, r, fc);
            T::ph_home_put(t, sh, fc, hr);
            if constexpr (PARK && IDT) { if (fc.new_slot >= 0) sh.act_next[fc.new_slot] = act_mv; }
            if constexpr (IDT) { if (fc.sp_slot >= 0) sh.act_next[fc.sp_slot] = sp_act; }
            if constexpr (ACT) {
                // next tick's actions: the vehicle lane t spawns gets the action of an all-zero row (ref :380, :420), the
                // controlled vehicles that stay get actor(row)
                if (fc.sp_slot >= 0) sh.act_next[fc.sp_slot] = (double)aprm[PV_A0];
                // (PERS: also on an item's last tick, unless it is the call's last: the next item starts from these actions)
                const bool hand_on = PERS && k + 1 == n_ticks && chunk_ + 1 < R.n_full + R.n_taper;
                if (k + 1 < n_ticks || hand_on)
                    rollout_actor<CAP>(R.actor_packed, aprm, sh.act_next, adsts, fc.n_ctl, O.obs_post, P.obs_f32 != 0,
                                       (size_t)env * CAP, t);
                if (hand_on) {
                    lds_barrier();                    // (every tile's actions are in act_next)
                    R.actor_actions[(size_t)env * CAP + t] = sh.act_next[t];
                }
            }
            lds_barrier();                            // B: the staging area is complete
            if (k + 1 < n_ticks) T::ph_reload(t, sh, r);
        }
        PVE_PHASE_MARK(10)
    }
    {
        const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka0_ + OFF_P);
        T::ph_flush(P, env0_, t0_, sh);
        if (PROF && P.phase_cycles && (t0_ & 63) == 0) {
            unsigned long long *row = P.phase_cycles + ((size_t)env0_ * (CAP / 64) + (t0_ >> 6)) * 16;
#pragma unroll
            for (int k = 0; k < 12; k++) row[k] += pc_[k];
            row[12] += clock64() - sclk0_; row[13] += wall_clock64() - wclk0_;
        }
    }
    if constexpr (PERS) {
        const PVE_AS4 RArgs &R = *(const PVE_AS4 RArgs *)(ka0_ + OFF_R);
        const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka0_ + OFF_P);
        q_publish(R, P.n_envs, t0_, env0_, chunk_);
    } else break;
  }
    if constexpr (PERS) q_leave(*(const PVE_AS4 RArgs *)(ka0_ + OFF_R), t0_);
}

// General-geometry tick (lane_num 4 / 8): same workgroup-per-intersection structure, phases of
// pve_tick_geo.h (per-route sorted lists: PAIRS -> RANK -> WALK; the membership scan only as the overflow fallback).
// Registers: 5 waves per SIMD (<= 96 VGPR) for CAP = 128 = 10 workgroups per CU.  CAP = 64 is one wave per workgroup and its
// 9.4 KB of LDS admit 16 workgroups per CU = 4 waves per SIMD whatever the registers: 128 VGPR there (the 4-lane variant,
// which carries both the far-conflict table and its replay fallback, spilled 35 registers at 96).  The 4-lane variant takes
// 128 at CAP = 128 too (8 workgroups per CU instead of 10, no scratch; its fast path is k_rollout_geo anyway).
template <int CAP, bool PROF = false, bool FIX4 = false>
__global__ __launch_bounds__(CAP) __attribute__((amdgpu_waves_per_eu((CAP == 64 || FIX4) ? 4 : 5, (CAP == 64 || FIX4) ? 4 : 5))) void k_tick_geo(const GeoConst g_arg, const Params P_arg)
{
    KernargPtr ka0_ = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const PVE_AS4 GeoConst &g = *(const PVE_AS4 GeoConst *)ka0_;
    const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka0_ + ((sizeof(GeoConst) + 7) / 8 * 8));
    __shared__ SharedGeo<CAP> sh;
    const int t = threadIdx.x;
    const int env = blockIdx.x;
    Regs r;
    typedef TickGeo<CAP> T;
    typedef Tick<CAP, SharedGeo<CAP>> B;
    unsigned long long pc_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev_ = PROF ? wall_clock64() : 0ull;
#undef PVE_PHASE_MARK
#define PVE_PHASE_MARK(idx)                                                              \
    if (PROF) {                                                                          \
        unsigned long long now_ = wall_clock64();                                        \
        pc_[idx] = now_ - tprev_;                                                        \
        tprev_ = now_;                                                                   \
    }
    T::ph_load(g, P, env, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(0)
    T::ph_step1(g, P, env, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(1)
    B::ph_step2(g.base, t, sh, r);
    T::ph_order(t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(2)
    B::ph_step3(g.base, t, sh, r);
    B::ph_step3_publish(t, sh, r);
    T::ph_order2(t, sh, r);
    T::ph_pairs_mode(t, sh, P.geo_scan != 0);
    lds_barrier();
    PVE_PHASE_MARK(3)
    if (T::pairs_over(sh, P.geo_scan != 0)) {         // (uniform, rare: the capacity upper bounds overflow the entry pool)
        T::ph_pairs_count(g, t, sh, P.geo_scan != 0);
        lds_barrier();
        T::ph_pairs_exact(t, sh, P.geo_scan != 0);
        lds_barrier();
        T::ph_pairs_apply(t, sh);
        lds_barrier();
    }
    T::ph_pairs_fill(g, t, sh);
    lds_barrier();
    PVE_PHASE_MARK(4)
    T::ph_load_late(P, env, t, sh, r);
    if (FIX4) T::ph_fix_table(g, t, sh, r);      // (behind FILL: its rows are the back entries' indices)
    T::ph_rank(t, sh, env);
    lds_barrier();
    PVE_PHASE_MARK(5)
    T::template ph_scan<FIX4>(g, t, sh, r);
    PVE_PHASE_MARK(11)
    T::ph_reward(g, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(6)
    T::ph_effects(g, t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(7)
    B::ph_prefetch_arrival(P, env, t, sh, r, g.lane_num);
    B::ph_lock_slot(g.base, t, sh, r);
    if (P.out.state_pre) T::ph_state_order(t, sh, r);   // (uniform)
    lds_barrier();
    B::ph_lock2_slot(t, sh, r);
    lds_barrier();
    PVE_PHASE_MARK(8)
    T::ph_final(g, P, env, t, sh, r);
    PVE_PHASE_MARK(9)
    if (P.out.state_pre) {
        __threadfence_block();
        __syncthreads();
        T::ph_state(P, env, t, sh, r);
    }
    if (PROF && P.phase_cycles && (t & 63) == 0) {
        unsigned long long *row = P.phase_cycles + ((size_t)env * (CAP / 64) + (t >> 6)) * 16;
#pragma unroll
        for (int k = 0; k < 12; k++) row[k] += pc_[k];
    }
}

// pve_step_many for the 4- / 8-lane layouts: the phases of k_tick_geo in a loop, the state resident on the chip between the
// ticks (TickGeo::ph_final<true> / ph_stage / ph_reload: the staging arrays overlay the list storage, which is dead by
// FIN); the lookup tables are copied to LDS once per launch instead of once per tick, only the per-tick outputs and the
// prefetched actions / arrival times touch HBM.  What it buys beyond the bytes: a launch of k_tick_geo lasts as long as its
// slowest intersection (43 us against a mean of 30 for 4 lanes x 64 slots); here a slow tick of one intersection is
// averaged over the ticks of the launch.
// TRAIN: the training outputs (obs_pre, state_pre) per tick of a trajectory roll-out; IDT: PVE_SRC_TABLE (actions by (tick,
// vehicle id), gathered by the vehicle's own thread and parked at its NEW slot in `p[]`, which is free between FIN and the next
// S1) -- as in k_rollout, variants of their own so that the default kernel keeps its register allocation.
// PERS: the persistent work-queue form (k_rollout<.., PERS>: same queue, same hand-off), every source; with the training outputs
// for 8 lanes only (the 4-lane variant <.., true, 4, TRAIN, .., PERS> would spill 32-46 registers: never instantiated, refused by
// launch_rollout_geo).
// ACT: pve_step_many(PVE_SRC_ACTOR) -- the closed loop of main.py:398-441 for lane_num 4 / 8 resident on the chip, as in
// k_rollout<.., ACT>: behind STAGE every wave runs the actor (pve_actor.h: actor_tile32) on its tiles of 32 controlled
// vehicles, whose float32 / float64 rows FIN has just stored to obs_post; the phases here work per slot, so the list of the
// controlled vehicles' NEW slots (`adsts`, by rank among the controlled vehicles) is filed behind FIN; the actions wait in
// `p[]` (free between FIN and the next S1) where RELOAD looks for them, the spawned vehicles get the action of the all-zero
// row.  Every tick is staged (no `still` shortcut): the actor runs every tick.
template <int CAP, bool FIX4 = false, int WPE = 4, bool TRAIN = false, bool IDT = false, bool PERS = false, bool ACT = false>
__global__ __launch_bounds__(CAP) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_rollout_geo(const GeoConst g_arg, const Params P_arg,
                                                                                                const typename rollout_args<ACT>::type R_arg)
{
    typedef typename rollout_args<ACT>::type RArgs;      // (ACT: RolloutArgs + the exploration noise)
    static_assert(!(TRAIN && IDT), "lane_num 4 / 8: the table source without the training outputs");
    static_assert(!ACT || !IDT, "the closed loop of the geometry kernel: one action source");
    KernargPtr ka0_ = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr size_t OFF_P = (sizeof(GeoConst) + 7) / 8 * 8, OFF_R = OFF_P + (sizeof(Params) + 7) / 8 * 8;
    __shared__ SharedGeo<CAP> sh;
    __shared__ __attribute__((aligned(64))) float aprm[ACT ? PV_TOTAL : 1];
    __shared__ uint8_t adsts[ACT ? CAP : 1];         // NEW slot of the k-th controlled vehicle (255: gone / no such vehicle)
    __shared__ int q_word[4];
    int t0_ = threadIdx.x;
    int env0_ = PERS ? 0 : blockIdx.x;
    int k_base_ = 0, chunk_ = 0;
    bool aprm_staged = false;                        // PERS + ACT: the float parameters are in LDS (once per workgroup)
    KernargPtr kav_ = ka0_;
    Regs r;
    FinCarry fc;
    typedef TickGeo<CAP> T;
    typedef Tick<CAP, SharedGeo<CAP>> B;
    int pool_idx, n_ticks;
    if constexpr (PERS) { if (t0_ == 0) { q_word[2] = -1; q_word[3] = 0; } }
  for (;;) {                                        // PERS: one pass per item; else exactly one pass
    {
        const PVE_AS4 GeoConst &g = *(const PVE_AS4 GeoConst *)ka0_;
        const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka0_ + OFF_P);
        const PVE_AS4 RArgs &R = *(const PVE_AS4 RArgs *)(ka0_ + OFF_R);
        pool_idx = R.pool_tick0;
        n_ticks = R.n_ticks;
        const double *act0 = nullptr;
        if constexpr (PERS) {
            int e, ch, kb, nt;
            if (!q_take(R, P.n_envs, t0_, q_word, e, ch, kb, nt)) break;
            env0_ = e; chunk_ = ch; k_base_ = kb; n_ticks = nt;
            if (R.source == 1 || R.source == 3) pool_idx = (R.pool_tick0 + k_base_) % R.n_pool;
            if (R.source == 1) act0 = R.pool + (size_t)pool_idx * (size_t)P.n_envs * CAP;
        }
        // ACT (cf. k_rollout): the first item of an intersection in a call computes its first actions from the caller's rows,
        // every later item takes them from `actor_actions`, where the previous item's last tick left them
        bool act_handed = false;
        if constexpr (PERS && ACT) {
            act_handed = chunk_ > 0;
            if (act_handed) act0 = R.actor_actions;
        }
        if constexpr (ACT) if (!act_handed) {
            if (!PERS || !aprm_staged) {
                const float *gp = (const float *)(R.actor_packed + AP_PRM);
                for (int n = t0_; n < PV_TOTAL; n += CAP) aprm[n] = gp[n];
            }
            const int mt = P.i32[I_META][(size_t)env0_ * CAP + t0_];
            const bool cc = (mt & (M_ALIVE | M_CONTROL)) == (M_ALIVE | M_CONTROL);
            vote<CAP / 64>(sh.m_ctl, t0_, cc);
            adsts[t0_] = 255;
            lds_barrier();
            if (cc) adsts[mask_rank<CAP / 64>(sh.m_ctl, t0_)] = (uint8_t)t0_;
            const int nc = mask_count<CAP / 64>(sh.m_ctl);
            lds_barrier();                               // parameters staged, list complete
            rollout_actor<CAP>(R.actor_packed, aprm, sh.p, adsts, nc, R.actor_obs, P.obs_f32 != 0, (size_t)env0_ * CAP, t0_);
            lds_barrier();                               // (the actions wait in p[], which LOAD does not touch)
        }
        if constexpr (PERS && ACT) {
            if (!aprm_staged && act_handed) {            // (a workgroup whose first item is a later chunk: parameters for its ticks)
                const float *gp = (const float *)(R.actor_packed + AP_PRM);
                for (int n = t0_; n < PV_TOTAL; n += CAP) aprm[n] = gp[n];
            }
            aprm_staged = true;
        }
        if constexpr (PERS) {
            T::template ph_load<true, ACT>(g, P, env0_, t0_, sh, r, act0, true);
            lds_barrier();
            T::template ph_load_late<true>(P, env0_, t0_, sh, r);
        } else {
        T::ph_load(g, P, env0_, t0_, sh, r);            // P.actions = the first tick's actions
        lds_barrier();
        T::ph_load_late(P, env0_, t0_, sh, r);
        }
        if constexpr (ACT) { if (!act_handed) r.act = sh.p[t0_]; }   // (uncontrolled slots: whatever is there, masked in S1)
        if constexpr (IDT) {                            // the first tick's action of the vehicle in this slot: table[row][id]
            const int idc = r.id < 0 ? 0 : (r.id < R.table_ids ? r.id : R.table_ids - 1);
            r.act = r.alive ? R.pool[(size_t)pool_idx * (size_t)R.table_ids + idc] : 0.0;
        }
    }
    double sp_act = 0;                                  // IDT: the action of the vehicle this lane spawns
    for (int k = 0; k < n_ticks; k++) {
        // (the same opaque re-definitions as in k_rollout: nothing derived from the arguments is hoisted out of the loop)
        if constexpr (PERS) env0_ = __builtin_amdgcn_readfirstlane(env0_);
        asm volatile("" : "+s"(kav_), "+v"(t0_), "+s"(env0_));
        const KernargPtr ka = kav_;
        const int t = t0_, env = env0_;
#ifndef PVE_NO_RANGE_ASSUME                        // (A/B build knob)
        __builtin_assume(t >= 0 && t < CAP);          // (the opaque copy hides the range: index arithmetic stays in 24 / 32 bits)
#endif
        const PVE_AS4 GeoConst &g = *(const PVE_AS4 GeoConst *)ka;
        const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka + OFF_P);
        const PVE_AS4 RArgs &R = *(const PVE_AS4 RArgs *)(ka + OFF_R);
        lds_barrier();
        if (k > 0) T::ph_tick_init(g, t, sh, r);      // (the list counters S1 adds to were cleared in the previous tick's FX phase)
        if constexpr (ACT) rollout_noise(R, env, k_base_ + k, r);
        T::ph_step1(g, P, env, t, sh, r);
        lds_barrier();
        B::ph_step2(g.base, t, sh, r);
        T::ph_order(t, sh, r);
        lds_barrier();
        B::ph_step3(g.base, t, sh, r);
        B::ph_step3_publish(t, sh, r);
        T::ph_order2(t, sh, r);
        T::ph_pairs_mode(t, sh, P.geo_scan != 0);
        lds_barrier();
        if (T::pairs_over(sh, P.geo_scan != 0)) {     // (uniform, rare)
            T::ph_pairs_count(g, t, sh, P.geo_scan != 0);
            lds_barrier();
            T::ph_pairs_exact(t, sh, P.geo_scan != 0);
            lds_barrier();
            T::ph_pairs_apply(t, sh);
            lds_barrier();
        }
        T::ph_pairs_fill(g, t, sh);
        lds_barrier();
        if (FIX4) T::ph_fix_table(g, t, sh, r);      // (behind FILL: its rows are the back entries' indices)
        T::ph_rank(t, sh);
        lds_barrier();
        T::template ph_scan<FIX4>(g, t, sh, r);
        T::ph_reward(g, t, sh, r);
        lds_barrier();
        int nx = -1;
        if (k + 1 < n_ticks) { pool_idx = (pool_idx + 1 == R.n_pool) ? 0 : pool_idx + 1; nx = pool_idx; }
        if constexpr (IDT) {
            const int idc = r.id < 0 ? 0 : (r.id < R.table_ids ? r.id : R.table_ids - 1);
            r.act_nx = (nx >= 0 && r.alive) ? R.pool[(size_t)nx * (size_t)R.table_ids + idc] : 0.0;
        } else B::ph_prefetch_action(P, R, env, t, nx, r);
        T::ph_effects(g, t, sh, r);
        T::ph_lists_clear(t, sh);
        lds_barrier();
        B::ph_prefetch_arrival(P, env, t, sh, r, g.lane_num);
        B::ph_lock_slot(g.base, t, sh, r);
        const Outputs O = B::template tick_outputs<TRAIN>(P, R, k_base_ + k);
        if (TRAIN && O.state_pre) T::ph_state_order(t, sh, r);    // (uniform; `ord` is staging storage from FIN on)
        lds_barrier();
        B::ph_lock2_slot(t, sh, r);
        lds_barrier();
        T::template ph_final<true>(g, P, O, env, t, sh, r, fc, ACT || k + 1 == n_ticks || (TRAIN && O.state_pre != nullptr));
        if constexpr (ACT) {
            // the k-th controlled vehicle's NEW slot (m_ctl: the votes of S1); entries beyond the controlled count: no vehicle
            if (t >= fc.n_ctl) adsts[t] = 255;
            if (r.alive && r.ctl) adsts[mask_rank<CAP / 64>(sh.m_ctl, t)] = (uint8_t)(fc.new_slot < 0 ? 255 : fc.new_slot);
        }
        if constexpr (IDT) {
            if (!fc.still && fc.new_slot >= 0) sh.p[fc.new_slot] = r.act_nx;      // (p[] is free between FIN and the next S1)
            sp_act = 0;                               // the vehicle this lane spawns (id known since FIN): its first action
            if (fc.sp_slot >= 0 && nx >= 0) {
                const int idc = fc.sp_id < R.table_ids ? fc.sp_id : R.table_ids - 1;
                sp_act = R.pool[(size_t)nx * (size_t)R.table_ids + idc];
            }
        }
        if (fc.still) {                               // (uniform) nobody moves: the registers carry over
            T::ph_carry_over(t, sh, r, fc);
        } else {
            lds_barrier();                            // A: nobody reads the tick's work arrays any more
            // (uniform; barrier A also orders the obs_pre rows of this tick.  PERS: the stale rows of an item's first tick are what
            //  ANOTHER workgroup's item stored: coherent loads)
            if (TRAIN && O.state_pre) T::template ph_state<PERS>(P, O, env, t, sh, r);
            T::ph_stage(g, t, sh, r, fc);
            if constexpr (IDT) { if (fc.sp_slot >= 0) sh.p[fc.sp_slot] = sp_act; }
            if constexpr (ACT) {
                // next tick's actions: the vehicle lane t spawns gets the action of an all-zero row (ref :380, :420), the
                // controlled vehicles that stay get actor(row)
                if (fc.sp_slot >= 0) sh.p[fc.sp_slot] = (double)aprm[PV_A0];
                // (PERS: also on an item's last tick, unless it is the call's last: the next item starts from these actions)
                const bool hand_on = PERS && k + 1 == n_ticks && chunk_ + 1 < R.n_full + R.n_taper;
                if (k + 1 < n_ticks || hand_on)
                    rollout_actor<CAP>(R.actor_packed, aprm, sh.p, adsts, fc.n_ctl, O.obs_post, P.obs_f32 != 0, (size_t)env * CAP, t);
                if (hand_on) {
                    lds_barrier();                    // (every tile's actions are in p[])
                    R.actor_actions[(size_t)env * CAP + t] = sh.p[t];
                }
            }
            lds_barrier();                            // B: the staging area is complete
            if (k + 1 < n_ticks) {
                T::ph_reload(t, sh, r);
                if constexpr (IDT || ACT) r.act = sh.p[t];
            }
        }
    }
    {
        const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka0_ + OFF_P);
        B::ph_flush(P, env0_, t0_, sh);
    }
    if constexpr (PERS) {
        const PVE_AS4 RArgs &R = *(const PVE_AS4 RArgs *)(ka0_ + OFF_R);
        const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(ka0_ + OFF_P);
        q_publish(R, P.n_envs, t0_, env0_, chunk_);
    } else break;
  }
    if constexpr (PERS) q_leave(*(const PVE_AS4 RArgs *)(ka0_ + OFF_R), t0_);
}

// tools/probe_kernel.sh: compile ONE variant of k_rollout / k_rollout_geo (seconds instead of minutes for the whole library) to
// read its register allocation / ISA while working on it: -DPVE_PROBE_ONE="128, 5, false, false, false, true, true" or
// -DPVE_PROBE_GEO="128, true, 4, false, false, true, true"
#if defined(PVE_PROBE_ONE) || defined(PVE_PROBE_GEO)
#ifdef PVE_PROBE_ONE
template <int CAP, int WPE, bool PROF = false, bool ACT = false, bool... REST> struct probe_one_act { static constexpr bool value = ACT; };
template __global__ void k_rollout<PVE_PROBE_ONE>(const Const, const Params, const rollout_args<probe_one_act<PVE_PROBE_ONE>::value>::type);
#endif
#ifdef PVE_PROBE_GEO
template <int CAP, bool FIX4 = false, int WPE = 4, bool TRAIN = false, bool IDT = false, bool PERS = false, bool ACT = false> struct probe_geo_act { static constexpr bool value = ACT; };
template __global__ void k_rollout_geo<PVE_PROBE_GEO>(const GeoConst, const Params, const rollout_args<probe_geo_act<PVE_PROBE_GEO>::value>::type);
#endif
#else
template <int CAP>
__global__ __launch_bounds__(64) void k_reset_geo(const GeoConst g_arg, const Params P_arg, int cap_ticks)
{
    KernargPtr kar_ = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const PVE_AS4 GeoConst &g = *(const PVE_AS4 GeoConst *)kar_;
    const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(kar_ + ((sizeof(GeoConst) + 7) / 8 * 8));
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env < P.n_envs) reset_env_geo<CAP>(g, P, env, cap_ticks);
}

template <int CAP>
__global__ __launch_bounds__(CAP) void k_compact(const Params P_arg)
{
    const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ Shared<CAP> sh;
    const int t = threadIdx.x;
    const int env = blockIdx.x;
    CRegs r;
    Tick<CAP>::ph_c_load(P, env, t, sh, r);
    __syncthreads();
    Tick<CAP>::ph_c_store(P, env, t, sh, r);
}

// diagnostics (pve_debug_traffic_probe): exactly the load pattern of the tick's load phase (6 f64 + 6 i32
// SoA rows per env, 8 B / 4 B per lane, every slot) and one dword store per workgroup -- a kernel with a KNOWN
// byte count to calibrate rocprofv3's FETCH_SIZE for this access width (MI355X_MICROARCH.md, HBM section)
template <int CAP>
__global__ __launch_bounds__(CAP) void k_probe(const Params P, int *sink)
{
    const size_t g = (size_t)blockIdx.x * CAP + threadIdx.x;
    double a = P.f64[F_P][g] + P.f64[F_V][g] + P.f64[F_A][g] + P.f64[F_JERK_SUM][g] + P.f64[F_VIR_DIS][g] +
               P.f64[F_CLOSER_P][g];
    int b = P.i32[I_ID][g] + P.i32[I_SEQ][g] + P.i32[I_VNUM][g] + P.i32[I_STEP][g] + P.i32[I_COUNT][g] +
            P.i32[I_META][g];
    unsigned long long m = __ballot(a + (double)b == 12345.678);
    if (threadIdx.x == 0) sink[blockIdx.x] = (int)m;
}

template <int CAP>
__global__ __launch_bounds__(64) void k_reset(const Const c_arg, const Params P_arg, int cap_ticks)
{
    KernargPtr kar_ = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const PVE_AS4 Const &c = *(const PVE_AS4 Const *)kar_;
    const PVE_AS4 Params &P = *(const PVE_AS4 Params *)(kar_ + ((sizeof(Const) + 7) / 8 * 8));
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env < P.n_envs) reset_env<CAP>(c, P, env, cap_ticks);
}

// ------------------------------------------------------------------ the learner step (csrc/pve_learn.h)
// k_learner_step: ONE workgroup runs n_batches steps in sequence.  The work items of every phase of learn_steps are dealt to the
// threads (item i to thread i mod blockDim.x), one workgroup barrier closes each phase: no grid-wide barrier, no flag, no wait on
// another workgroup, every loop bounded by the arguments.  Which thread computes an item changes no bit of it: the orders of
// pve_learn.h are orders WITHIN an item.  LDS holds the tape of one sub-block of rows (odd row stride: the rows of neighbouring
// lanes fall into different banks) and the step's running sums.  Weights, moments, targets and gradients stay in the block in
// global memory (52 KB of online weights: resident in the CU's L1 / L2; measured faster than a copy in LDS with half the rows
// per sub-block); what one thread writes there another reads only behind a workgroup barrier, and one workgroup
// shares one L1.  A gradient is accumulated and applied by the same thread.
struct LearnWg {
    int tid, nt;
    template <class F> PVE_HD void forall(int n, F f) const
    {
        for (int i = tid; i < n; i += nt) f(i);
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
#endif
    }
};
constexpr int LEARN_LDS_FLOATS = LEARN_TAPE + LEARN_SCALARS;
static_assert(LEARN_LDS_FLOATS * 4 <= 160 * 1024, "one workgroup's LDS on gfx950");
static_assert((LEARN_SUB_1 - 1) * LEARN_STRIDE_1 + T_NET <= LEARN_TAPE && (LEARN_SUB_2 - 1) * LEARN_STRIDE_2 + 2 * T_NET <= LEARN_TAPE,
              "the tape of a sub-block stays inside its LDS region");
__global__ __launch_bounds__(1024) void k_learner_step(LearnCtx C)
{
    extern __shared__ __attribute__((aligned(16))) float learn_s[];
    if (blockIdx.x != 0) return;
    C.tape = learn_s; C.S = learn_s + LEARN_TAPE;
    learn_steps(LearnWg{(int)threadIdx.x, (int)blockDim.x}, C);
}

// The wide step (learn_steps_wide): per minibatch k_learner_slice<critic>, k_learner_apply<critic>, k_learner_slice<actor>,
// k_learner_apply<actor> on one stream; what one launch writes the next reads behind the kernel boundary, nothing else orders them.
// k_learner_slice: workgroup g of G runs learn_slice on slices g, g + G, ... as LearnWg does above (same LDS, same barriers) and
// leaves each slice's row of the workspace complete.  No workgroup reads what another writes.
template <bool CRITIC> __global__ __launch_bounds__(1024) void k_learner_slice(LearnCtx C, float *work, int step, int n_slices)
{
    extern __shared__ __attribute__((aligned(16))) float learn_s[];
    C.tape = learn_s; C.S = learn_s + LEARN_TAPE;
    const LearnWg E{(int)threadIdx.x, (int)blockDim.x};
    for (int s = blockIdx.x; s < n_slices; s += gridDim.x) learn_slice(E, C, step, s, CRITIC, work + (size_t)s * LW_ROW);
}
// k_learner_apply: ONE workgroup adds the rows in ascending slice order (item i to thread i mod blockDim.x, which also applies it),
// then Adam, the soft update, the powers and, behind the step's last pass, the count, the losses and the `grads` row.
template <bool CRITIC> __global__ __launch_bounds__(1024) void k_learner_apply(LearnCtx C, const float *__restrict__ work, int step, int n_slices)
{
    if (blockIdx.x != 0) return;
    learn_combine(LearnWg{(int)threadIdx.x, (int)blockDim.x}, C, step, CRITIC, work, n_slices);
}

// pve_learner_init: the four networks into the block, moments / count / gradients zeroed, the powers set to beta1, beta2
__global__ __launch_bounds__(256) void k_learner_init(float *__restrict__ P, const float *__restrict__ actor, const float *__restrict__ critic,
                                                      const float *__restrict__ tactor, const float *__restrict__ tcritic, float beta1, float beta2)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < LB_TOTAL; i += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < LB_CRITIC) { if (i - LB_ACTOR < LRN_ACTOR_W) v = actor[i - LB_ACTOR]; }
        else if (i < LB_TACTOR) { if (i - LB_CRITIC < LRN_CRITIC_W) v = critic[i - LB_CRITIC]; }
        else if (i < LB_TCRITIC) { if (i - LB_TACTOR < LRN_ACTOR_W) v = tactor[i - LB_TACTOR]; }
        else if (i < LB_M_ACTOR) { if (i - LB_TCRITIC < LRN_CRITIC_W) v = tcritic[i - LB_TCRITIC]; }
        else if (i >= LB_POWERS && i < LB_STEPS) v = ((i - LB_POWERS) & 1) ? beta2 : beta1;
        P[i] = v;
    }
}

static std::string hip_err(const char *what, hipError_t e)
{
    return std::string(what) + ": " + hipGetErrorString(e);
}

// hipOccupancyMaxActiveBlocksPerMultiprocessor + the LDS allocation granule.  The runtime's answer divides the CU's 160 KB by
// the block size, but the hardware hands LDS out in 128 granules of 1 280 B per CU (measured, tools/occupancy_probe.hip: ten
// 128-thread workgroups of 15 360 B start at once, of 15 488 .. 16 384 B only nine although the query says ten; sixteen
// one-wave workgroups of 10 240 B = 8 granules do).  A persistent grid sized by the query alone would park its surplus
// workgroups in the dispatcher until the resident ones leave.
template <typename K> static hipError_t resident_blocks(int *nb, K kernel, int threads)
{
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, kernel, threads, 0);
    if (e != hipSuccess) return e;
    hipFuncAttributes fa;
    e = hipFuncGetAttributes(&fa, (const void *)kernel);
    if (e != hipSuccess) return e;
    if (fa.sharedSizeBytes > 0) {
        const int granules = (int)((fa.sharedSizeBytes + 1279) / 1280), by_lds = 128 / granules;
        if (by_lds > 0 && by_lds < *nb) *nb = by_lds;
    }
    return hipSuccess;
}

// ------------------------------------------------------------------ run-time configuration -> kernel variant
// with_flags(f, a, b, ..) hands run-time booleans to f as compile-time constants: f(std::bool_constant<a>{}, std::bool_constant<b>{}, ..).
// (The capacity goes through Backend::with_cap.)  Every combination of the flags is compiled: a launcher instantiates only the
// variants its family declares (`exists` below).
template <typename F> static int with_flags(F f) { return f(); }
template <typename F, typename... Bs> static int with_flags(F f, bool b, Bs... rest)
{
    return b ? with_flags([&](auto... r) { return f(std::true_type{}, r...); }, rest...)
             : with_flags([&](auto... r) { return f(std::false_type{}, r...); }, rest...);
}

// The variants of k_rollout the library holds: `exists` names them (a launcher instantiates nothing else), `sized_by` is the kernel
// whose occupancy sizes the persistent grid, and kernel() is the only place in the host code that writes k_rollout<..> with
// arguments (tools/probe_kernel.sh's instantiation aside).
template <int CAP_, int WPE_, bool PROF_, bool ACT_, bool TRAIN_, bool IDT_, bool PERS_> struct Rollout12 {
    static constexpr int CAP = CAP_, WPE = WPE_;
    static constexpr bool GEO = false, PROF = PROF_, ACT = ACT_, TRAIN = TRAIN_, IDT = IDT_;    // (what launch_variant notes)
    static constexpr bool PERS = PERS_, exists =
        !(PERS_ && PROF_) && !(ACT_ && IDT_) &&                                       // (the kernel's own static_asserts)
        (WPE_ == 4 ? !PROF_ || (CAP_ <= 128 && !ACT_ && !TRAIN_ && !IDT_)            // the phase-cycle diagnostics: the default kernel at 64 / 128 slots
                   : WPE_ == 5 && CAP_ == 128 && PERS_ && !ACT_ && !TRAIN_);          // HOME: 128 slots, the queue form, zero / pool / table
    // as many workgroups as the chip holds at once of the capacity's default queue kernel (each capacity from its own kernel's
    // occupancy: the 256-slot block admits half the 128-slot workgroups per CU); HOME: of its table kernel.  The TRAIN and IDT
    // variants have the default's block.  The ACT variants do not: at 64 slots k_rollout<64, 4, false, true, .., true> has
    // 12 368 B of LDS against the default's 10 240 B -- by the compiler's tables and resident_blocks' granule rule 12 resident
    // workgroups per CU where the grid is sized for 16 (at 128 and 256 slots both come out equal, 8 and 4).  Derived, not
    // measured.
    typedef Rollout12<CAP_, WPE_, false, false, false, WPE_ == 5, true> sized_by;
    static auto kernel() { return k_rollout<CAP_, WPE_, PROF_, ACT_, TRAIN_, IDT_, PERS_>; }
};

// ... and of k_rollout_geo, which takes its arguments in another order: layout x capacity x {default, training outputs, id-indexed
// table, actor, actor + training outputs} x launch form
template <int CAP_, bool FIX4_, int WPE_, bool TRAIN_, bool IDT_, bool PERS_, bool ACT_> struct RolloutGeo {
    static constexpr int CAP = CAP_, WPE = WPE_;
    static constexpr bool GEO = true, PROF = false, ACT = ACT_, TRAIN = TRAIN_, IDT = IDT_;
    static constexpr bool PERS = PERS_, exists =
        !(TRAIN_ && IDT_) && !(ACT_ && IDT_) &&                                       // (the kernel's own static_asserts)
        CAP_ <= 128 && !(PERS_ && TRAIN_ && ACT_) &&                                  // (the 4- / 8-lane layouts: 64 or 128 slots)
        (WPE_ == 4 || (knobs_built && WPE_ == 5 && CAP_ == 128 && !FIX4_ && !TRAIN_ && !IDT_ && !PERS_ && !ACT_));   // (PVE_ROLLOUT_GEO_WPE5)
    // (the variants of one capacity share their register budget; the actor's parameters add 2 KB of LDS: a query of its own)
    typedef RolloutGeo<CAP_, true, 4, false, false, true, ACT_> sized_by;
    static auto kernel() { return k_rollout_geo<CAP_, FIX4_, WPE_, TRAIN_, IDT_, PERS_, ACT_>; }
};

// What a roll-out launcher does with a configuration (Backend::pick_rollout / pick_rollout_geo): launch the variant the flags name
// -- pers: the queue form on as many workgroups as stay resident, else one workgroup per intersection -- or, launch = false,
// answer 1 = no resident kernel: pve_step_many falls back to chunked, then per-tick launches
struct RolloutPick {
    bool launch;
    bool wide;                   // k_rollout: the HOME build (WPE 5); k_rollout_geo: the knob-only 96-VGPR build
    bool prof, act, train, idt, pers;
};

// Workgroups the current device holds at once of kernel variant Q, or -1 (err set): resident workgroups per CU x CUs, cached per
// DEVICE (a process may hold handles on several GPUs, and they need not be the same part) and per queried kernel, hence per
// capacity; filled by the first persistent launch on that device.
template <typename Q> static long long resident_workgroups(std::string &err)
{
    static_assert(Q::exists && Q::PERS, "the grid is sized by a queue kernel the library holds");
    constexpr int MAX_DEV = 64;
    static std::mutex mu;
    static int wgs[MAX_DEV] = {}, n_cu[MAX_DEV] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { err = "hipGetDevice failed"; return -1; }
    std::lock_guard<std::mutex> lock(mu);
    const bool cached = dev >= 0 && dev < MAX_DEV && wgs[dev] > 0;
    int nb = cached ? wgs[dev] : 0, cus = cached ? n_cu[dev] : 0;
    if (!cached) {
        hipDeviceProp_t prop;
        const hipError_t e = resident_blocks(&nb, Q::kernel(), Q::CAP);
        if (e != hipSuccess || nb <= 0 || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
            err = std::string("occupancy query of the persistent roll-out: ") + hipGetErrorString(e);
            return -1;
        }
        cus = prop.multiProcessorCount;
        if (dev >= 0 && dev < MAX_DEV) { wgs[dev] = nb; n_cu[dev] = cus; }
    }
    return (long long)nb * cus;
}

struct Backend : BackendDefaults {
    // the largest capacity pve_create accepts (pve_capi.inc): 256 slots for the 12-lane fast path
    static constexpr int max_capacity = 256;
    static int bad_cap(int cap, std::string &err)
    {
        err = "no kernel for capacity " + std::to_string(cap);
        return -1;
    }
    static int set_device(int dev, std::string &err)
    {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0) { err = "no HIP device visible (libpveenv.so needs an AMD GPU; there is no CPU fallback)"; return -1; }
        if (dev < 0 || dev >= n) { err = "device_id out of range"; return -1; }
        return 0;
    }
    static int enter_device(int dev)
    {
        int prev = -1;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        return prev;
    }
    static void leave_device(int prev)
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    static void *dmalloc(size_t n)
    {
        void *p = nullptr;
        if (hipMalloc(&p, n) != hipSuccess) return nullptr;
        return p;
    }
    static void dfree(void *p) { (void)hipFree(p); }
    static int memset0(void *p, size_t n, void *stream)
    {
        return hipMemsetAsync(p, 0, n, (hipStream_t)stream) == hipSuccess ? 0 : -1;
    }
    // XCDs of the device: the persistent roll-out shards the intersections over them (every shard is worked by one XCD)
    static int n_xcc(int dev)
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess || v <= 0) v = 8;
        return v > QUEUE_MAX_SHARDS ? QUEUE_MAX_SHARDS : v;
    }
    static int d2h(void *dst, const void *src, size_t n, void *stream)
    {
        hipStream_t s = (hipStream_t)stream;
        if (hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
        if (hipStreamSynchronize(s) != hipSuccess) return -1;
        return 0;
    }
    static int sync(void *stream, std::string &err)
    {
        hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) { err = hip_err("hipStreamSynchronize", e); return -1; }
        return 0;
    }
    static int check_launch(std::string &err)
    {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { err = hip_err("kernel launch", e); return -1; }
        return 0;
    }
    template <typename K, typename... A>
    static int launch(K kernel, long long grid, int block, void *stream, std::string &err, const A &...args)
    {
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), 0, (hipStream_t)stream, args...);
        return check_launch(err);
    }
    // THE run-time capacity dispatch: f receives the capacity as std::integral_constant<int, CAP>.  MAX_CAP = 128: a kernel family
    // without a 256-slot build (the 4- / 8-lane layouts)
    template <int MAX_CAP = max_capacity, typename F> static int with_cap(int cap, std::string &err, F f)
    {
        if (cap == 64) return f(std::integral_constant<int, 64>{});
        if (cap == 128) return f(std::integral_constant<int, 128>{});
        if constexpr (MAX_CAP >= 256) if (cap == 256) return f(std::integral_constant<int, 256>{});
        return bad_cap(cap, err);
    }
    static int launch_tick(const Const &c, const Params &P, int cap, void *stream, std::string &err)
    {
        return with_cap(cap, err, [&](auto CAP) {
            const int rc = launch(k_tick<CAP()>, P.n_envs, CAP(), stream, err, c, P);
            if (rc == 0) note_launch(false, NL, CAP(), 0, P.phase_cycles != nullptr, false, P.out.obs_pre || P.out.state_pre, false, false, P.n_envs);
            return rc;
        });
    }
    // the kernel's view of the action source: the pool / table row of the launch's first tick, P.actions = that tick's actions of the
    // pool, the exploration noise (a variant without the actor receives the RolloutArgs part)
    static RolloutArgsNoisy rollout_source(const RolloutArgs &R, const ActionNoise &nz, int cap, Params &P)
    {
        RolloutArgsNoisy Rk;
        (RolloutArgs &)Rk = R;
        Rk.noise = nz;
        if (R.source == 1 || R.source == 3) Rk.pool_tick0 = R.pool_tick0 % R.n_pool;
        P.actions = R.source == 1 ? R.pool + (size_t)Rk.pool_tick0 * (size_t)P.n_envs * (size_t)cap : nullptr;
        return Rk;
    }
    // Launch variant V: one workgroup per intersection, or -- the persistent form (pve_rollout.persistent) -- as many workgroups as
    // the chip holds at once of V::sized_by (the queue needs no more; fewer when the call has fewer items)
    template <typename V, typename C>
    static int launch_variant(const C &c, const Params &P, const RolloutArgsNoisy &Rk, void *stream, std::string &err)
    {
        if constexpr (!V::exists) {
            err = "no such roll-out kernel variant";             // (a pick_rollout* that names a variant its family does not declare)
            return -1;
        } else {
            long long grid = P.n_envs;
            if constexpr (V::PERS) {
                grid = resident_workgroups<typename V::sized_by>(err);
                if (grid < 0) return -1;
                const long long items = (long long)P.n_envs * (Rk.n_full + Rk.n_taper);
                if (const char *g = PVE_KNOB("PVE_PERSISTENT_GRID")) { const long long v = atoll(g); if (v > 0) grid = v; }   // A/B knob
                if (grid > items) grid = items;
            }
            const int rc = launch(V::kernel(), grid, V::CAP, stream, err, c, P, Rk);
            // (pve_debug_last_variant: V's own arguments -- what ran, not what a picker intended)
            if (rc == 0) note_launch(V::GEO, family_of(c), V::CAP, V::WPE, V::PROF, V::ACT, V::TRAIN, V::IDT, V::PERS, grid);
            return rc;
        }
    }
    static int family_of(const Const &) { return NL; }
    static int family_of(const GeoConst &g) { return g.lane_num; }
    // The axes of a configuration, and what rules a resident kernel out in both families: the A/B knobs, and for the closed loop
    // the exact-float32 actor (per-tick launches run it) and a queue without R.actor_actions, through which an intersection's
    // actions go from one item to the next
    static RolloutPick rollout_axes(const Params &P, const RolloutArgs &R)
    {
        static const bool off = PVE_KNOB("PVE_NO_ROLLOUT_KERNEL") != nullptr;   // A/B knob: one launch per tick instead
        static const bool act_off = PVE_KNOB("PVE_NO_ROLLOUT_ACTOR") != nullptr;   // A/B knob: actor + tick launches instead
        RolloutPick v = {};
        v.act = R.source == 2 /* PVE_SRC_ACTOR */; v.idt = R.source == 3; v.pers = R.queue != nullptr;
        v.train = P.out.obs_pre || P.out.state_pre;
        v.launch = !off && !(v.act && (act_off || R.exact_f32 || (v.pers && !R.actor_actions)));
        return v;
    }
    // Is there a resident / persistent k_rollout for this configuration, and which (variant = capacity x action source (pool / zero,
    // actor, id-indexed table) x training outputs x launch form)
    static RolloutPick pick_rollout(int cap, const Params &P, const RolloutArgs &R)
    {
        const RolloutPick none = {};
        RolloutPick v = rollout_axes(P, R);
        if (!v.launch) return none;
        if (P.phase_cycles) {
            // pve_debug_phase_cycles armed.  The phase-cycle diagnostics exist for the default kernel only: every other variant (table,
            // actor, training outputs) answers "no resident kernel" and the caller falls back to per-tick launches, which record the
            // cycles -- except for the table source, which has no per-tick form: pve_step_many refuses it with PVE_ERR_STATE while
            // armed (256 slots: no diagnostics variant of the resident kernel either).  The queue form has none: the chunked launches
            // record the cycles (as the geo path does) -- except in `make trace`, whose per-item timestamps go where the cycles would
            if (v.act) return none;
            if (!v.pers) {
                if (v.train || v.idt || cap == 256) return none;
                v.prof = true;
            }
#ifndef PVE_QUEUE_TRACE
            else return none;
#endif
        }
        // k_rollout<128, 5, ..>: the HOME build of the persistent kernel (128 slots; table, pool and zero sources) -- 96 registers
        // + the 15 280 B block with the carried per-slot fields in LDS homes = 10 workgroups per CU instead of 8, no scratch
        // (pve_tick_core.h: Homes).  Its packed seq_in_lane | id_info[1] word holds arrival cursors < 2^23.  Only the queue form:
        // a plain launch of 4096 workgroups would run as 2560 + 1536.
        // (The training outputs through this block -- k_rollout<128, 5, .., TRAIN, .., PERS>: 94-96 registers -- were measured: 137-141
        //  against 129-131 us per tick; the trainer's roll-out keeps the register build.)
        const bool home_ok = v.pers && !v.act && !v.train && cap == 128 && P.rows < (1 << 23);
        v.wide = PVE_HOME_DEFAULT != 0 && home_ok;
#ifdef PVE_AB_KNOBS
        if (const char *k5 = getenv("PVE_ROLLOUT_WPE5")) v.wide = atoi(k5) != 0 && home_ok;   // A/B knob
#endif
        return v;
    }
    // pve_step_many's launch of a chunk or of the whole call, with the exploration noise of the actor variants (nz.tick0 = the
    // launch's first tick; read by the ACT variants only) -> 0, 1 = no resident kernel for this configuration, -1 (err set)
    static int launch_rollout_noisy(const Const &c, const Params &P_in, const RolloutArgs &R, const ActionNoise &nz, int cap, void *stream,
                                    std::string &err)
    {
        const RolloutPick v = pick_rollout(cap, P_in, R);
        if (!v.launch) return 1;
        Params P = P_in;
        RolloutArgsNoisy Rk = rollout_source(R, nz, cap, P);
#ifdef PVE_QUEUE_TRACE
        if (v.pers) Rk.q_trace = P.phase_cycles;                              // (per-item timestamps: make trace)
#endif
        return with_cap(cap, err, [&](auto CAP) {
            return with_flags([&](auto HOME, auto PROF, auto ACT, auto TRAIN, auto IDT, auto PERS) {
                return launch_variant<Rollout12<CAP(), HOME() ? 5 : 4, PROF(), ACT(), TRAIN(), IDT(), PERS()>>(c, P, Rk, stream, err);
            }, v.wide, v.prof, v.act, v.train, v.idt, v.pers);
        });
    }
    static RolloutPick pick_rollout_geo(const GeoConst &g, int cap, const Params &P, const RolloutArgs &R)
    {
        const RolloutPick none = {};
        RolloutPick v = rollout_axes(P, R);
        // (no phase-cycle diagnostics in k_rollout_geo; the table source without the training outputs)
        if (!v.launch || P.phase_cycles || (v.train && v.idt)) return none;
        // (the closed loop with the training outputs is bound by the state writes: its queue form measured 130 against 128 us per
        //  tick of chunked launches, so it stays on those.  Round 6: the 4-lane <TRAIN, PERS> variant is instantiated -- it
        //  carries 32 spilled registers through the tick and is still 6 % faster than chunked launches: 95.3 vs 101.5 us)
        if (v.pers && v.train && v.act) return none;
#ifdef PVE_AB_KNOBS
        static const bool w5 = getenv("PVE_ROLLOUT_GEO_WPE5") != nullptr;     // A/B knob: 96-VGPR build, 10 workgroups per CU (414 spills)
        v.wide = w5 && cap == 128 && g.lane_num != 4 && !v.train && !v.act && !v.pers && !v.idt;
#endif
        return v;
    }
    static int launch_rollout_geo_noisy(const GeoConst &g, const Params &P_in, const RolloutArgs &R, const ActionNoise &nz, int cap,
                                        void *stream, std::string &err)
    {
        const RolloutPick v = pick_rollout_geo(g, cap, P_in, R);
        if (!v.launch) return 1;
        Params P = P_in;
        const RolloutArgsNoisy Rk = rollout_source(R, nz, cap, P);
        const bool fix4 = g.lane_num == 4;           // (the 4-lane layout's far-conflict path is a kernel of its own)
        return with_cap<128>(cap, err, [&](auto CAP) {
            return with_flags([&](auto FIX4, auto WPE5, auto TRAIN, auto IDT, auto PERS, auto ACT) {
                return launch_variant<RolloutGeo<CAP(), FIX4(), WPE5() ? 5 : 4, TRAIN(), IDT(), PERS(), ACT()>>(g, P, Rk, stream, err);
            }, fix4, v.wide, v.train, v.idt, v.pers, v.act);
        });
    }
    static int launch_tick_geo(const GeoConst &g, const Params &P, int cap, void *stream, std::string &err)
    {
        // (PROF: the diagnostics build, pve_debug_phase_cycles; FIX4: the 4-lane layout's far-conflict path is a kernel of its own)
        return with_cap<128>(cap, err, [&](auto CAP) {
            return with_flags([&](auto PROF, auto FIX4) {
                const int rc = launch(k_tick_geo<CAP(), PROF(), FIX4()>, P.n_envs, CAP(), stream, err, g, P);
                if (rc == 0) note_launch(true, g.lane_num, CAP(), 0, PROF(), false, P.out.obs_pre || P.out.state_pre, false, false, P.n_envs);
                return rc;
            }, P.phase_cycles != nullptr, g.lane_num == 4);
        });
    }
    static int launch_reset_geo(const GeoConst &g, const Params &P, int cap, void *stream, std::string &err)
    {
        return with_cap<128>(cap, err, [&](auto CAP) { return launch(k_reset_geo<CAP()>, (P.n_envs + 63) / 64, 64, stream, err, g, P, 200000); });
    }
    static int launch_compact(const Params &P, int cap, void *stream, std::string &err)
    {
        return with_cap(cap, err, [&](auto CAP) { return launch(k_compact<CAP()>, P.n_envs, CAP(), stream, err, P); });
    }
    static int pack_actor(const float *W, float *flat, unsigned char *packed, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        hipError_t e = hipMemcpyAsync(flat, W, sizeof(float) * AW_TOTAL, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { err = hip_err("hipMemcpyAsync", e); return -1; }
        hipLaunchKernelGGL(k_actor_pack, dim3(1), dim3(256), 0, s, W, packed);
        return check_launch(err);
    }
    static int launch_actor(const float *W, const unsigned char *packed, const void *obs, int mode, const int32_t *meta,
                            double *actions, int n_envs, int cap, void *stream, std::string &err)
    {
        ActionNoise off;
        memset(&off, 0, sizeof(off));
        return launch_actor_noisy(W, packed, obs, mode, meta, nullptr, off, actions, n_envs, cap, stream, err);
    }
    // the actor pass + the exploration noise of pve_set_action_noise (ids = the [n_envs][cap] id field; read when nz.sigma != 0)
    static int launch_actor_noisy(const float *W, const unsigned char *packed, const void *obs, int mode, const int32_t *meta,
                                  const int32_t *ids, const ActionNoise &nz, double *actions, int n_envs, int cap, void *stream,
                                  std::string &err)
    {
        // persistent workgroups of 4 waves (the parameters are staged in LDS once per workgroup): 4 per CU, one wave
        // per intersection at a time (a wave's second intersection, n_envs > 4096: tests/test_gpu_actor_streaming.py)
        static const int wgs = [] { const char *g = PVE_KNOB("PVE_ACTOR_GRID"); const int v = g ? atoi(g) : 0; return v > 0 ? v : 1024; }();
        const int grid = (n_envs + 3) / 4 < wgs ? (n_envs + 3) / 4 : wgs;
        return with_cap(cap, err, [&](auto CAP) {
            return with_flags([&](auto OBS_F32, auto EXACT_F32) {
                typedef std::conditional_t<OBS_F32(), float, double> OBS_T;
                if constexpr (EXACT_F32()) return launch(k_actor_t<CAP(), OBS_T>, grid, 256, stream, err, W, (const OBS_T *)obs, meta, actions, n_envs, ids, nz);
                else return launch(k_actor_h<CAP(), OBS_T>, grid, 256, stream, err, packed, (const OBS_T *)obs, meta, actions, n_envs, ids, nz);
            }, (mode & 1) != 0, (mode & 2) != 0);
        });
    }
    // pve_set_target_networks: the target actor through the actor's own packing kernel, the critic through k_critic_pack
    static int pack_target_networks(const float *actor_w, float *actor_flat, unsigned char *actor_packed, const float *critic_w,
                                    float *critic_flat, unsigned char *critic_packed, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        if (actor_w && pack_actor(actor_w, actor_flat, actor_packed, stream, err) != 0) return -1;
        if (critic_w) {
            hipError_t e = hipMemcpyAsync(critic_flat, critic_w, sizeof(float) * CW_TOTAL, hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) { err = hip_err("hipMemcpyAsync", e); return -1; }
            hipLaunchKernelGGL(k_critic_pack, dim3(1), dim3(256), 0, s, critic_w, critic_packed);
        }
        return check_launch(err);
    }
    // persistent workgroups of 4 waves, every wave walks chunks of 64 rows: as many workgroups as stay resident (LDS: the
    // bootstrap kernel holds both packed networks, 2 per CU; the critic alone 4 per CU), never more than there are chunks
    static int target_q_grid(long long n, int per_cu)
    {   // (mirrored by tests/target_q_walk.py, the host model of the walk behind the tests with several chunks per wave)
        const long long want = (n + 255) / 256, cap = 256LL * per_cu;
        return (int)(want < cap ? want : cap);
    }
    static int launch_critic(const unsigned char *critic_packed, const void *rows, int obs_f32, const float *act7, float *q,
                             long long n, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const int grid = target_q_grid(n, 4);
        if (obs_f32) hipLaunchKernelGGL((k_target_q<float, false>), dim3(grid), dim3(256), 0, s, nullptr, critic_packed, (const float *)rows, act7, nullptr, q, nullptr, n);
        else hipLaunchKernelGGL((k_target_q<double, false>), dim3(grid), dim3(256), 0, s, nullptr, critic_packed, (const double *)rows, act7, nullptr, q, nullptr, n);
        return check_launch(err);
    }
    static int launch_bootstrap_q(const unsigned char *actor_packed, const unsigned char *critic_packed, const void *state, int obs_f32,
                                  const int32_t *flags, float *q, float *act7_out, long long n, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const int grid = target_q_grid(n, 2);
        if (obs_f32) hipLaunchKernelGGL((k_target_q<float, true>), dim3(grid), dim3(256), 0, s, actor_packed, critic_packed, (const float *)state, nullptr, flags, q, act7_out, n);
        else hipLaunchKernelGGL((k_target_q<double, true>), dim3(grid), dim3(256), 0, s, actor_packed, critic_packed, (const double *)state, nullptr, flags, q, act7_out, n);
        return check_launch(err);
    }
    // pve_nstep_scan: one thread per candidate start, then the offsets of the 64-slot groups in one workgroup
    static int launch_nstep_scan(const NstepArgs &A, int block_threads, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const long long n_slots = nstep_groups(A) * NSTEP_GROUP;
        const int block = block_threads > 0 ? block_threads : 256;
        hipLaunchKernelGGL(k_nstep_scan, dim3((unsigned)((n_slots + block - 1) / block)), dim3(block), 0, s, A, n_slots);
        hipLaunchKernelGGL(k_nstep_offsets, dim3(1), dim3(1024), 0, s, A.offsets, nstep_groups(A), A.total);
        return check_launch(err);
    }
    static int launch_nstep_gather(const NstepArgs &A, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const long long n_slots = nstep_groups(A) * NSTEP_GROUP;
        const dim3 grid((unsigned)((n_slots + 255) / 256));
        if (A.obs_f32) hipLaunchKernelGGL(k_nstep_gather<float>, grid, dim3(256), 0, s, A, n_slots);
        else hipLaunchKernelGGL(k_nstep_gather<double>, grid, dim3(256), 0, s, A, n_slots);
        return check_launch(err);
    }
    // pve_replay_append: the copy (grid-stride over the 16-byte pieces of at most min(n_max, capacity) records), then the state
    // update in a launch of its own behind it -- no workgroup of the copy can read the new `written`
    static int launch_replay_append(const ReplayArgs &A, const float *records, const long long *total_dev, long long n_max,
                                    int block_threads, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const int block = block_threads > 0 ? block_threads : 256;
        const long long pieces = (n_max < A.capacity ? n_max : A.capacity) * REPLAY_PIECES, want = (pieces + block - 1) / block;
        const unsigned grid = (unsigned)(want < 16384 ? want : 16384);
        hipLaunchKernelGGL(k_replay_append, dim3(grid), dim3(block), 0, s, A, records, total_dev, n_max);
        hipLaunchKernelGGL(k_replay_append_commit, dim3(1), dim3(64), 0, s, A, total_dev, n_max);
        return check_launch(err);
    }
    // pve_replay_sample: one thread per drawn record, then `draws` and the status word in a launch of their own
    static int launch_replay_sample(const ReplayArgs &A, long long batch, long long n_batches, float *rows, float *act7, float *target,
                                    long long *seq, int block_threads, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const int block = block_threads > 0 ? block_threads : 256;
        const long long n_total = batch * n_batches;
        hipLaunchKernelGGL(k_replay_sample, dim3((unsigned)((n_total + block - 1) / block)), dim3(block), replay_sample_lds(block), s, A, batch,
                           n_total, rows, act7, target, seq);
        hipLaunchKernelGGL(k_replay_sample_commit, dim3(1), dim3(64), 0, s, A, batch, n_batches);
        return check_launch(err);
    }
    // pve_learner_init / pve_learner_step: one workgroup; 153 KB of dynamic LDS need the function attribute (once per device)
    static int launch_learner_init(float *P, const float *actor, const float *critic, const float *tactor, const float *tcritic,
                                   float beta1, float beta2, void *stream, std::string &err)
    {
        return launch(k_learner_init, (LB_TOTAL + 255) / 256, 256, stream, err, P, actor, critic, tactor, tcritic, beta1, beta2);
    }
    // The three kernels that take LEARN_LDS_FLOATS of dynamic LDS get the function attribute once per device -> that device's CU
    // count (cached), or -1 (err set)
    static int learner_setup(std::string &err)
    {
        static std::mutex mu;
        static int n_cu[64] = {};
        int dev = 0, cus = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) { err = hip_err("hipGetDevice", e); return -1; }
        std::lock_guard<std::mutex> lock(mu);
        if (dev >= 0 && dev < 64 && n_cu[dev]) return n_cu[dev];
        for (const void *k : {(const void *)k_learner_step, (const void *)k_learner_slice<true>, (const void *)k_learner_slice<false>}) {
            e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * LEARN_LDS_FLOATS));
            if (e != hipSuccess) { err = hip_err("hipFuncSetAttribute", e); return -1; }
        }
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess || cus <= 0) { err = hip_err("hipDeviceGetAttribute", e); return -1; }
        if (dev >= 0 && dev < 64) n_cu[dev] = cus;
        return cus;
    }
    static int launch_learner_step(const LearnCtx &C, int block_threads, void *stream, std::string &err)
    {
        if (learner_setup(err) < 0) return -1;
        const int block = block_threads > 0 ? block_threads : 1024;
        hipLaunchKernelGGL(k_learner_step, dim3(1), dim3(block), sizeof(float) * LEARN_LDS_FLOATS, (hipStream_t)stream, C);
        return check_launch(err);
    }
    // pve_learner_step_wide: four launches per minibatch (two with PVE_LEARN_CRITIC_ONLY), enqueued in order, no host
    // synchronisation.  groups = 0: one workgroup per slice, at most one per CU.
    static int launch_learner_step_wide(const LearnCtx &C, float *work, int groups, int block_threads, void *stream, std::string &err)
    {
        constexpr size_t lds = sizeof(float) * LEARN_LDS_FLOATS;
        const int cus = learner_setup(err);
        if (cus < 0) return -1;
        const int n_slices = learn_n_slices(C.batch), want = groups > 0 ? groups : cus;
        const int grid = n_slices < want ? n_slices : want, block = block_threads > 0 ? block_threads : 1024;
        const bool with_actor = !(C.H.flags & LEARN_CRITIC_ONLY);
        hipStream_t s = (hipStream_t)stream;
        for (int step = 0; step < C.n_batches; step++) {
            hipLaunchKernelGGL(k_learner_slice<true>, dim3(grid), dim3(block), lds, s, C, work, step, n_slices);
            hipLaunchKernelGGL(k_learner_apply<true>, dim3(1), dim3(block), 0, s, C, (const float *)work, step, n_slices);
            if (with_actor) {
                hipLaunchKernelGGL(k_learner_slice<false>, dim3(grid), dim3(block), lds, s, C, work, step, n_slices);
                hipLaunchKernelGGL(k_learner_apply<false>, dim3(1), dim3(block), 0, s, C, (const float *)work, step, n_slices);
            }
            if (check_launch(err) != 0) return -1;
        }
        return 0;
    }
    // pve_prio_reset: pseq = -1, pstate = 0
    static int launch_prio_reset(const PrioArgs &A, int block_threads, void *stream, std::string &err)
    {
        const int block = block_threads > 0 ? block_threads : 256;
        const long long want = (A.R.capacity + block - 1) / block;
        hipLaunchKernelGGL(k_prio_reset, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(block), 0, (hipStream_t)stream, A);
        return check_launch(err);
    }
    // pve_prio_rank: the keys, then four passes of histogram / scan / scatter over 8-bit digits, keys and payloads ping-pong
    // between the two scratch halves; the last pass writes its payloads to `order`.  The grids cover the capacity: how many
    // records are live is on the device only, a tile past them returns at once.
    static int launch_prio_rank(const PrioArgs &A, int block_threads, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const int block = block_threads > 0 ? block_threads : 256;
        const long long want = (A.R.capacity + block - 1) / block;
        const dim3 tiles((unsigned)prio_tiles(A.R.capacity));
        hipLaunchKernelGGL(k_prio_keys, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(block), 0, s, A);
        for (int pass = 0; pass < PRIO_PASSES; pass++) {
            const int in = pass & 1, out = in ^ 1;
            hipLaunchKernelGGL(k_prio_hist, tiles, dim3(block), 0, s, A, (const uint32_t *)A.keys[in], 8 * pass);
            hipLaunchKernelGGL(k_prio_scan, dim3(PRIO_RADIX), dim3(block), 0, s, A, pass);
            hipLaunchKernelGGL(k_prio_scatter, tiles, dim3(block), 0, s, A, (const uint32_t *)A.keys[in], (const int32_t *)A.vals[in],
                               A.keys[out], pass == PRIO_PASSES - 1 ? A.order : A.vals[out], 8 * pass);
        }
        return check_launch(err);
    }
    // pve_prio_sample: the ranking, one workgroup per minibatch, then pdraws in a launch of its own
    static int launch_prio_sample(const PrioArgs &A, long long n_batches, long long min_live, float alpha_beta, float *rows, float *act7,
                                  float *target, long long *seq, int32_t *rank, float *weight, int block_threads, void *stream,
                                  std::string &err)
    {
        if (launch_prio_rank(A, block_threads, stream, err) != 0) return -1;
        hipStream_t s = (hipStream_t)stream;
        const long long fit = (A.batch + 63) / 64 * 64;
        const int block = block_threads > 0 ? block_threads : (int)(fit < 256 ? fit : 256);
        hipLaunchKernelGGL(k_prio_sample, dim3((unsigned)n_batches), dim3(block), prio_sample_lds(block), s, A, min_live, alpha_beta, rows,
                           act7, target, seq, rank, weight);
        hipLaunchKernelGGL(k_prio_sample_commit, dim3(1), dim3(64), 0, s, A, min_live, n_batches);
        return check_launch(err);
    }
    // pve_prio_update: stamp and zero, then the maximum -- two launches, so that no maximum meets a zeroing
    static int launch_prio_update(const PrioArgs &A, const long long *seq, const float *q, const float *target, long long n,
                                  int block_threads, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const int block = block_threads > 0 ? block_threads : 256;
        const long long want = (n + block - 1) / block;
        const dim3 grid((unsigned)(want < 4096 ? (want > 0 ? want : 1) : 4096));
        hipLaunchKernelGGL(k_prio_update_stamp, grid, dim3(block), 0, s, A, seq, n);
        hipLaunchKernelGGL(k_prio_update_max, grid, dim3(block), 0, s, A, seq, q, target, n);
        return check_launch(err);
    }
    // pve_generate_arrivals: one workgroup per ARR_GROUP environments; the intentions in a launch of their own
    static int launch_generate_arrivals(const ArrivalArgs &A, int block_threads, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const int block = block_threads > 0 ? block_threads : 256;
        hipLaunchKernelGGL(k_gen_arrivals, dim3((unsigned)((A.n_envs + ARR_GROUP - 1) / ARR_GROUP)), dim3(block), 0, s, A);
        if (A.intentions) {
            const long long items = (((long long)A.rows + ARR_INT_ROWS - 1) / ARR_INT_ROWS) * A.n_envs;
            hipLaunchKernelGGL(k_gen_intentions, dim3((unsigned)(items < (1 << 20) ? items : (1 << 20))), dim3(block), 0, s, A);
        }
        return check_launch(err);
    }
    // pve_rollout_stats: the env rows (one wave per (tick, env)), the groups (one workgroup per (tick, group)), the totals
    static int launch_rollout_stats(const StatsArgs &A, int block_threads, void *stream, std::string &err)
    {
        hipStream_t s = (hipStream_t)stream;
        const int block = block_threads > 0 ? block_threads : 256;
        const long long items = (long long)A.n_ticks * A.n_envs, per = block / 64, want = (items + per - 1) / per;
        hipLaunchKernelGGL(k_stats_rows, dim3((unsigned)(want < (1 << 16) ? want : (1 << 16))), dim3(block), 0, s, A);
        // (few workgroups, each walking every chunk of its tick: sixteen waves by default, so that a wave has few chunks in a row)
        hipLaunchKernelGGL(k_stats_groups, dim3((unsigned)A.n_ticks, (unsigned)A.n_groups), dim3(block_threads > 0 ? block_threads : 1024), 0, s, A);
        if (A.totals)
            hipLaunchKernelGGL(k_stats_totals, dim3((unsigned)((A.n_groups * STAT_N + 255) / 256)), dim3(256), 0, s, A);
        return check_launch(err);
    }
    // pve_metrics_groups: one workgroup per group
    static int launch_metrics_groups(const EnvHeader *hd, int n_envs, int cap, const int32_t *group, int n_groups, double *out,
                                     void *stream, std::string &err)
    {
        hipLaunchKernelGGL(k_stats_metrics, dim3((unsigned)n_groups), dim3(STAT_METRIC_THREADS), 0, (hipStream_t)stream, hd, n_envs, cap, group, n_groups, out);
        return check_launch(err);
    }
    static int launch_probe(const Params &P, int cap, int *sink, void *stream, std::string &err)
    {
        return with_cap(cap, err, [&](auto CAP) { return launch(k_probe<CAP()>, P.n_envs, CAP(), stream, err, P, sink); });
    }
    static int launch_reset(const Const &c, const Params &P, int cap, void *stream, std::string &err)
    {
        return with_cap(cap, err, [&](auto CAP) { return launch(k_reset<CAP()>, (P.n_envs + 63) / 64, 64, stream, err, c, P, 200000); });
    }
};
// the product provides every optional group of the contract: a missing or misspelt launcher fails the build here
static_assert(Provides<Backend>::noise, "the HIP backend overrides launch_actor_noisy, launch_rollout_noisy and launch_rollout_geo_noisy");
static_assert(Provides<Backend>::target_q, "the HIP backend overrides pack_target_networks, launch_critic and launch_bootstrap_q");
static_assert(Provides<Backend>::nstep, "the HIP backend overrides launch_nstep_scan and launch_nstep_gather");
static_assert(Provides<Backend>::replay, "the HIP backend overrides launch_replay_append and launch_replay_sample");
static_assert(Provides<Backend>::prio, "the HIP backend overrides launch_prio_reset, launch_prio_rank, launch_prio_sample and launch_prio_update");
static_assert(Provides<Backend>::arrivals, "the HIP backend overrides launch_generate_arrivals");
static_assert(Provides<Backend>::stats, "the HIP backend overrides launch_rollout_stats and launch_metrics_groups");
static_assert(Provides<Backend>::learner, "the HIP backend overrides launch_learner_init and launch_learner_step");
static_assert(Provides<Backend>::learner_wide, "the HIP backend overrides launch_learner_step_wide");

#include "pve_capi.inc"
#endif   // PVE_PROBE_ONE / PVE_PROBE_GEO

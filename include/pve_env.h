/*
 * pve_env.h -- C ABI of libpveenv.so: the MI355X-native batched unsignalised-intersection
 * environment (drop-in for the hot path of Mingtzge/PVE-MCC_for_unsignalized_intersection).
 *
 * The reference has no FFI / plugin interface: its boundary is the Python object surface of
 * `TrafficInteraction` that main.py touches.  Each entry point below names the
 * reference call it replaces ("ref :N" = traffic_interaction_scene.py line N).  The Python host
 * mirror (pve-mcc_for_unsignalized_intersection_amd/traffic_interaction_scene.py and batched.py)
 * binds exactly these symbols through ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no torch / HIP types: device buffers are `void*` device addresses, the stream is a
 *     `void*` holding a hipStream_t (NULL = default stream).
 *   - every function returns PVE_OK (0) or a negative error code; pve_last_error() gives the text.
 *   - all per-vehicle device buffers are caller-allocated, laid out [n_envs][capacity] (row-major),
 *     "slot" = rank of the vehicle in (lane, j) order inside its environment.
 *   - calls on one handle are asynchronous on the handle's stream and must not be issued
 *     concurrently from several host threads.
 */
#ifndef PVE_ENV_H
#define PVE_ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PVE_ABI_VERSION 9
#define PVE_LANES 12          /* physical lanes: lane_num = 4, 8 or 12 (arrays are padded to 12) */
#define PVE_MAX_DIRS 16       /* virtual-lane lists (routes): 12 for lane_num 4 / 12, 16 for lane_num 8 (ref :86, :132, :167) */
#define PVE_OBS_WIDTH 28      /* (o_agent_num + 1) * 4, ref :1295 */
#define PVE_NBR 6             /* ref :1324 hard-codes 6 neighbours */
#define PVE_STATE_ROWS 7
#define PVE_N_METRICS 12

enum {
    PVE_OK = 0,
    PVE_ERR_INVALID = -1,     /* bad argument */
    PVE_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime error (text in pve_last_error) */
    PVE_ERR_STATE = -3,       /* call sequence error (e.g. step before set_arrivals/reset) */
    PVE_ERR_NOMEM = -4
};

/* Constructor arguments of the reference, ref :21-23 (`TrafficInteraction.__init__`), plus
 * args.collision_thr (ref :32).  lane_num = 12 runs the optimised kernel (BASELINE metric); lane_num = 4 or 8
 * (ref :66-145) run the general-geometry kernel.  The 3-lane branch is broken upstream. */
#define PVE_CFG_GENERAL_PATH 0x1   /* flags: use the general-geometry kernel for lane_num = 12 too (cross-checks) */
#define PVE_CFG_OBS_F32      0x2   /* flags: pve_outputs.obs_post and the actor's obs input hold float32 [n_envs][cap][28]
                                      (the type the actor consumes, model_agent_maddpg.py:15; SURVEY.md 8d "FP32 observation
                                      output": 268 instead of 380 algorithmic bytes per slot-step).  Fused ticks only:
                                      obs_pre / state_pre follow the row type (every lane_num); pve_compact(obs) is refused. */
#define PVE_CFG_GEO_SCAN     0x4   /* flags (diagnostics): the general-geometry kernel finds list members by scanning every controlled
                                      vehicle (its fallback when an intersection's lists overflow the LDS entry pool) instead of reading
                                      the per-route lists; results are identical (tested) */
#define PVE_CFG_ACTOR_F32    0x8   /* flags: run the actor as an exact float32 FMA chain (v_mfma_f32_16x16x4_f32, the evaluation order
                                      of csrc/pve_actor.h `actor_canonical`) instead of the default split-half form (every operand
                                      x = hi + lo in float16, three v_mfma_f32_32x32x16_f16 per block, float32 accumulation:
                                      ~1e-6 relative per dot product, 5x less matrix-core time) */
typedef struct pve_config {
    double deltaT;          /* 0.1 */
    double vm, vM;          /* 5, 13   (train(): vm = 6, main.py:230) */
    double am, aM;          /* -3, 3 */
    double v0;              /* 10 */
    double lane_cw;         /* 2.5 */
    double dis_ctl;         /* 150 */
    double collision_thr;   /* 2 (main.py:104) */
    int32_t lane_num;       /* 12 (default), 4 or 8 */
    int32_t flags;          /* PVE_CFG_* */
} pve_config;

/* Per-tick outputs.  Every pointer may be NULL (that output is skipped).  `flags` is written for every slot (0 = the
 * slot held no vehicle); the other per-slot outputs are written only for the slots that held a vehicle at tick start
 * (slots < env_out[PVE_EO_N_PRE]) and are unspecified elsewhere.
 * "pre" arrays are indexed by the slot a vehicle had when the tick started (= the `[lane, j]`
 * the reference reports in `ids`, ref :291); "post" arrays by the slot it has after compaction
 * and spawning (= where the next tick's action for it must be written). */
typedef struct pve_outputs {
    double  *obs_post;      /* [n_envs][cap][28]  (float32 rows with PVE_CFG_OBS_F32) row 0 of the state (ref :1336) of the vehicle now in
                               each slot; zeros for vehicles spawned this tick (ref :380,420) */
    double  *obs_pre;       /* [n_envs][cap][28]  same rows, pre-compaction indexing (`re_state[k][0]`); float32 like obs_post with
                               PVE_CFG_OBS_F32 (lane_num 12) */
    double  *state_pre;     /* [n_envs][cap][7][28] full state incl. neighbour rows (ref :1325-1337), same element type;
                               needs obs_prev_post and obs_pre */
    const double *obs_prev_post; /* obs_post buffer written by the previous tick (stale neighbour rows, ref :1332) */
    double  *reward;        /* [n_envs][cap]  pre; 0 for uncontrolled slots (ref :311-320, 346, 357) */
    int32_t *flags;         /* [n_envs][cap]  pre; PVE_F_* bits | collisions_per_veh << 8 (ref :339) */
    int32_t *lanej;         /* [n_envs][cap]  pre; lane << 16 | j  (the `ids` entry, ref :291) */
    int32_t *nbr;           /* [n_envs][cap][6] pre; lane << 16 | j of the 6 nearest, -1 = none (ref :1391-1405);
                               written for controlled vehicles (PVE_F_CTL) only */
    int32_t *new_slot;      /* [n_envs][cap]  pre -> post slot, -1 if deleted this tick (ref :435-444) */
    int32_t *env_out;       /* [n_envs][PVE_ENV_OUT_N] per-env scalars of this tick, see PVE_EO_* */
} pve_outputs;

/* bits of pve_outputs.flags */
#define PVE_F_ALIVE     0x01  /* slot held a vehicle at tick start */
#define PVE_F_CTL       0x02  /* controlled: appears in `ids`, has reward/obs (ref :282) */
#define PVE_F_DONE      0x04  /* veh["Done"] after this tick (ref :347, 351) */
#define PVE_F_DELETED   0x08  /* in delete_veh (exit or collision, ref :348) */
#define PVE_F_FINISHED  0x10  /* passed the box this tick: reward 5, jerks entry (ref :350-359) */
#define PVE_F_LOCK      0x20  /* veh["lock"] set by the dead-lock scan (ref :1482) */
#define PVE_F_INTENT_SHIFT 6  /* bits 6-7: veh["intention"] (ref :382-394); scene_update emits `ids` in
                                 (lane, intention, j) order (ref :233-275), which differs from slot order for lane_num 4 / 8 */

#define PVE_ENV_OUT_N 8
enum { PVE_EO_N_PRE = 0,      /* vehicles alive at tick start */
       PVE_EO_N_CTL,          /* len(ids) */
       PVE_EO_COLLISIONS,     /* `collisions` of the 9-tuple (ref :337) */
       PVE_EO_LOCK,           /* `lock` of the 9-tuple (ref :365-370) */
       PVE_EO_N_DELETED, PVE_EO_N_FINISHED, PVE_EO_N_SPAWNED,
       PVE_EO_N_POST };       /* vehicles alive after the call */

/* metrics vector of pve_get_metrics (sums over all envs of the handle since reset) */
enum { PVE_M_SLOT_STEPS = 0, PVE_M_ALIVE_STEPS, PVE_M_CTL_STEPS, PVE_M_SPAWNED /* id_seq */,
       PVE_M_PASSED, PVE_M_COLLIDED /* main.py:410-412 count */, PVE_M_LOCKS, PVE_M_SUM_REWARD,
       PVE_M_SUM_JERK /* of passed vehicles */, PVE_M_PASSED_STEPS, PVE_M_OVERFLOW, PVE_M_TICKS };

/* Per-vehicle record for the dict view `env.veh_info[lane][ind]` (ref :396-427, live keys only). */
typedef struct pve_vehicle {
    double p, v, a, jerk, jerk_sum, vir_dis, closer_p;
    int32_t lane, j, id /* id_info[0] */, vnum /* id_info[1] */, seq_in_lane;
    int32_t control, finish, done, collision, step, count, lock, lock_a;
    int32_t vir_header[2];
    int32_t intention, route;
} pve_vehicle;

typedef struct pve_env_info {
    double current_time;                 /* ref :223 */
    int32_t n_alive;
    int32_t lane_count[PVE_LANES];       /* veh_num, ref :206 */
    int32_t veh_rec[PVE_LANES];          /* ref :207 */
    int32_t id_seq, passed_veh, passed_veh_step_total;   /* ref :197-198, 212 */
    int32_t head_valid[PVE_MAX_DIRS], head_lane[PVE_MAX_DIRS], head_j[PVE_MAX_DIRS];  /* virtual_lane_4[d][0][1:3], ref :1517 */
    int32_t overflow;                    /* spawns deferred because the env was full: one per lane and tick.  The rule (fused and split
                                            ticks, every kernel): room = capacity - (vehicles alive when the tick starts) -- the vehicles
                                            this tick deletes free their slots for the NEXT tick only; when more lanes are due than
                                            there is room, the lowest lane indices spawn; a deferred lane keeps its cursor (veh_rec),
                                            takes no id (id_seq) and no intention (intention_re, the 8-lane draw) and is due again on
                                            the next tick */
    int32_t intention_re;                /* ref :42, :387-392 (lane_num 4 / 8) */
} pve_env_info;

typedef struct pve_handle_s *pve_handle;

int pve_abi_version(void);
const char *pve_last_error(void);
void pve_default_config(pve_config *cfg);

/* Bytes of device workspace a handle needs (persistent SoA vehicle state + env headers); 0 for a capacity the library has no
 * kernels for.  pve_workspace_bytes(n, 256) > 0 is how a caller probes for the 256-slot capacity. */
size_t pve_workspace_bytes(int n_envs, int capacity);

/* Replaces `TrafficInteraction(arrive_time, dis_ctl, args, ...)` object creation (ref :21) for
 * n_envs independent intersections with `capacity` (64, 128 or 256) vehicle slots each.  256 slots: lane_num 12 on the fast
 * path only; the 4- / 8-lane layouts and PVE_CFG_GENERAL_PATH at 256 return PVE_ERR_INVALID.
 * workspace: device buffer of pve_workspace_bytes() bytes, or NULL to let the library allocate. */
int pve_create(const pve_config *cfg, int n_envs, int capacity, int device_id,
               void *workspace, void *stream, pve_handle *out);
int pve_destroy(pve_handle h);
int pve_set_stream(pve_handle h, void *stream);

/* Arrival streams `arrive_time` (ref :195, main.py:388-389): DEVICE buffer of float64
 * [n_envs][rows][lane_num] (env_stride_rows = rows) or one shared [rows][lane_num] stream (env_stride_rows = 0).
 * Times beyond the run must be padded with +inf.  The buffer must outlive the handle's use of it. */
int pve_set_arrivals(pve_handle h, const double *arrivals, int rows, int env_stride_rows);

/* lane_num = 8 only: the reference draws each new vehicle's intention with random.randint(0, 1) after reseeding
 * `random` from OS entropy (ref :381, :390), i.e. irreproducibly; here the draws are an input stream like the
 * arrivals: DEVICE int32 [n_envs][rows][8] (or shared, env_stride_rows = 0), entry [veh_rec[lane]][lane] in {0,1}
 * picks intention[lane][draw] (ref :125-134).  Not set = all zeros.  Must be set before pve_reset. */
int pve_set_intentions(pve_handle h, const int32_t *choice, int rows, int env_stride_rows);

/* Constructor warm-up (ref :196-220): zero all state, then advance each env's clock tick by tick
 * (spawning, ref :378) until it holds at least one vehicle. */
int pve_reset(pve_handle h);

/* FUSED TICK = `for lane, ind: env.step(lane, ind, a)` (ref :1501, main.py:398-406) +
 * `env.scene_update()` (ref :222) + `env.delete_vehicle()` (ref :435) for every env.
 * actions: device float64 [n_envs][capacity], indexed by current (post-compaction) slot;
 * entries of uncontrolled / empty slots are ignored (main.py:401 passes 0). */
int pve_step_all(pve_handle h, const double *actions, const pve_outputs *out);

/* Split protocol for the single-env compatibility class (same kernels, three launches):
 *   pve_scene_update   = all step() calls + scene_update(); vehicles marked Done stay in place
 *   pve_compact        = delete_vehicle() */
int pve_scene_update(pve_handle h, const double *actions, const pve_outputs *out);
int pve_compact(pve_handle h, double *obs_post /* optional: rows are moved with the vehicles */);

/* MADDPG actor inference on the device (reference model_agent_maddpg.py:23-49 `actor_network`, called per
 * vehicle with batch 1 from main.py:36-45, 404): for every controlled vehicle
 *   actions[env][slot] = 3*tanh(Dense1(relu(LN(Dense64(relu(LN(Dense64(LN(obs[env][slot]))))))))   (float32; the two dense
 *   layers on the matrix cores with split-half operands unless PVE_CFG_ACTOR_F32, see pve_config.flags),
 * 0 for every other slot (main.py:401).
 * pve_set_actor installs the policy (the reference restores it once per run, main.py:380-384 `saver.restore`): weights =
 * DEVICE float32[PVE_ACTOR_N_WEIGHTS] in the order
 * LayerNorm{gamma[28],beta[28]}, dense{kernel[28][64],bias[64]}, LayerNorm_1{gamma,beta}[64],
 * dense_1{kernel[64][64],bias[64]}, LayerNorm_2{gamma,beta}[64], dense_2{kernel[64],bias[1]} (TF variable
 * layouts, checkpoint names `agent1actor/...`); they are copied into the handle's workspace (flat, and packed for the
 * matrix cores: centered over the output units, split into half pairs, in operand order), so the caller's buffer may be
 * reused afterwards; call it again after every update of the weights.
 * Range of the split-half form.  A half pair hi + lo holds 22 significant bits only while lo is a normal f16 number, i.e. for
 * values in [2^-3, 2^15).  The WEIGHTS are brought there at pack time: each centred dense kernel (and its centred bias) is
 * multiplied by 2^e, e = 0 while its largest entry M is in [2^-3, 2^12], else e = -floor(log2 M) clamped to +-40, and the
 * LayerNorm behind it runs with the variance epsilon 1e-12f * 4^e: exact in float32, and the same function of the weights at
 * every scale a training run passes through (a freshly initialised network, kernels ~ 3e-3, included; e = 0 changes no bit).
 * The ACTIVATIONS are split as they are.  Documented limits: (1) a LayerNorm output must stay below f16's largest number,
 * |gamma| * sqrt(63) + |beta| < 65 504 for LayerNorm_1 and LayerNorm_2 (sqrt(27) for the input LayerNorm); beyond, hi is inf
 * and the action is meaningless.  (2) A row whose input LayerNorm returns values far below 1 -- the all-zero row, or a row
 * whose spread is far below sqrt(1e-12) = 1e-6, while ln0_beta is near 0 as it is right after initialisation -- is contracted
 * with fewer than 22 bits (measured on the CPU model: up to 6e-4 on actions of a freshly initialised actor for rows with a
 * spread of 1e-12; an observation row holds a position, a speed and a route and is nowhere near).  PVE_CFG_ACTOR_F32 has
 * neither limit.  tests/split_half_model.py is the CPU statement of this arithmetic.
 * pve_actor_forward: obs = [n_envs][cap][28] float64 (= obs_post of the previous tick, zeros after reset);
 * actions: [n_envs][cap] float64 out.  `weights` = NULL uses the installed actor; non-NULL = pve_set_actor(weights) first. */
#define PVE_ACTOR_N_WEIGHTS 6393
int pve_set_actor(pve_handle h, const float *weights);
int pve_actor_forward(pve_handle h, const float *weights, const void *obs /* float64, or float32 with PVE_CFG_OBS_F32 */,
                      double *actions);

/* Closed loop on the device, no host round trip: pve_actor_forward(obs_in -> actions) followed by
 * pve_step_all(actions, out) on the same stream (BASELINE config 5).  out->obs_post may be obs_in itself (the tick
 * never reads observations) unless out->state_pre is requested, which needs the previous rows (obs_prev_post). */
int pve_step_all_actor(pve_handle h, const float *weights, const void *obs_in, double *actions,
                       const pve_outputs *out);

/* Exploration noise of the device actor (reference main.py:44, :239: the training loop commands
 * `agent.action(state) + np.random.randn(1) * noise_range` for every controlled vehicle, every tick; the evaluation loops run
 * with noise_range = 0).  Opt-in, host-only state of the handle, in force from the next call:
 *   a_cmd(env, vehicle, tick) = (double) actor_f32(row) + sigma * z(seed, env_global, vehicle_id, tick)
 * for every controlled vehicle (a vehicle spawned at the end of the previous tick, whose row is all zero, included), 0 for every
 * other slot as before (main.py:401); the tick clips a_cmd to [am, aM] as always (ref :1502).  It applies wherever the library
 * runs the actor -- pve_actor_forward (the returned actions are the noisy ones), pve_step_all_actor, pve_step_many(PVE_SRC_ACTOR)
 * in every launch form -- and never to actions the caller supplies (pve_step_all, PVE_SRC_POOL / TABLE / ZERO).
 * z is a pure function of its four arguments (csrc/pve_noise.h; the same numbers whatever the slot, launch form, capacity, chunking
 * or sub-batching):
 *   vehicle_id = the vehicle's id (pve_vehicle.id, state field "id"); tick = ticks the handle has run since pve_reset when the
 *   action is applied (the first tick after pve_reset is tick 0); env_global = env index in the handle + env_offset (a batch cut
 *   into several handles passes each piece its first global index and draws what the uncut batch draws).
 *   Bits: Philox4x32-10 with counter = (vehicle_id, tick mod 2^32, env_global low word, env_global high word) and
 *   key = (seed low word, seed high word); z = sqrt(-2 ln u1) cos(2 pi u2), u = (word + 0.5) 2^-32 from output words 0 and 1,
 *   evaluated in float64 with + - * / sqrt only in the order csrc/pve_noise.h writes down (bit-reproducible on the host:
 *   pve_mcc_amd/noise.py).
 * sigma = 0 switches the noise off (the default; every result is then what it was without this call).  sigma < 0, NaN or inf:
 * PVE_ERR_INVALID; sigma > 0 on a backend without the noisy actor kernels: PVE_ERR_INVALID. */
int pve_set_action_noise(pve_handle h, double sigma, uint64_t seed, int64_t env_offset);

/* Target networks on the device: the critic (reference model_agent_maddpg.py:52-74 `critic_network`) and the bootstrap term of
 * the n-step target (main.py:253-260), for any number of rows per call.  Purely additive to ABI 9: three new symbols, no struct
 * changes, PVE_ABI_VERSION stays 9; a binding detects an older library by the missing symbols.
 *
 * pve_set_target_networks installs a TARGET actor (`agent1_targetactor/...`, layout of pve_set_actor) and / or a critic
 * (`agent1_target_critic/...` for the bootstrap, `agent1_critic/...` for the online Q): DEVICE float32 vectors, copied into the
 * handle's workspace flat and packed like pve_set_actor does.  Either pointer may be NULL (that image is kept); both NULL is
 * PVE_ERR_INVALID.  Independent of pve_set_actor: installing target networks never changes what the acting policy computes.
 * Critic weight order (TF variable layouts): LayerNorm{gamma[28],beta[28]}, dense{kernel[28][64],bias[64]},
 * LayerNorm_1{gamma,beta}[64], dense_1{kernel[71][64],bias[64]} (rows 0..63 hidden, 64 own action, 65..70 the six other actions:
 * model_agent_maddpg.py:66, :82), LayerNorm_2{gamma,beta}[64], dense_2{kernel[64],bias[1]}.
 *
 * pve_critic_forward (main.py:76 `agent.Q(state, action, other_action)`): for each of the n rows
 *   q[i] = dense_2(relu(LN_2(dense_1([relu(LN_1(dense(LN(rows[i])))), act7[i]]))))      act7[i] = own action, six other actions.
 * pve_bootstrap_q (main.py:253-260): a_k = target_actor(state[i][k]) for ALL seven rows k = 0..6 (the all-zero rows of absent
 * neighbours included, as main.py:254-255 does), q[i] = critic(state[i][0], a_0, a_1 .. a_6); act7_out (optional) receives the
 * seven actions.  With `flags` (the pve_outputs.flags block that belongs to the rows) only rows with PVE_F_CTL set and PVE_F_DONE
 * clear are evaluated (main.py:250-251: no bootstrap behind Done; uncontrolled slots have no transition); every other row gets
 * q = 0 and act7_out = 0.  flags = NULL evaluates every row.
 * rows / state have the handle's observation element type (float64, or float32 with PVE_CFG_OBS_F32) and are cast to float32
 * on load, as the graph's placeholders do.  n is any positive count, not tied to n_envs * capacity: one tick's state_pre and
 * flags blocks, or a whole [n_ticks][n_envs][cap] trajectory in one call.  Both calls are asynchronous on the handle's stream
 * and need no pve_reset.  The target networks always run in the split-half matrix-core form (three v_mfma_f32_32x32x16_f16
 * per block, float32 accumulation), with or without PVE_CFG_ACTOR_F32.  The pack-time scale and the two limits stated at
 * pve_set_actor hold for both networks; the critic's second dense kernel is scaled as a whole, its seven action rows included
 * (the actions, |a| <= 3, are activations like the hidden units), and limit (1) reads |gamma| * sqrt(63) + |beta| < 65 504.
 * Errors: null or non-positive arguments PVE_ERR_INVALID; networks not installed PVE_ERR_STATE; a backend without the
 * kernels PVE_ERR_INVALID. */
#define PVE_CRITIC_N_WEIGHTS 6841
int pve_set_target_networks(pve_handle h, const float *target_actor /* PVE_ACTOR_N_WEIGHTS */,
                            const float *critic /* PVE_CRITIC_N_WEIGHTS */);
int pve_critic_forward(pve_handle h, const void *rows /* [n][28] */, const float *act7 /* [n][7] */,
                       float *q /* [n] */, int64_t n);
int pve_bootstrap_q(pve_handle h, const void *state /* [n][7][28] */, const int32_t *flags /* [n] or NULL */,
                    float *q /* [n] */, float *act7_out /* [n][7] or NULL */, int64_t n);

/* N-STEP TRANSITIONS from retained trajectory blocks (reference main.py:243-266).  Additive within ABI 9: two new symbols and two
 * new structs, nothing existing changes; a binding detects an older library by the missing symbols.
 *
 * The reference keeps, per controlled vehicle, a sliding buffer of its last seq_max_step + 1 = 13 ticks.  When the buffer is
 * full or the vehicle is Done it folds the rewards into  r = r_last (+ gamma * Q'(state_next_last) unless Done),
 * r = r_k + gamma * r  backwards through the older entries, and puts ONE transition -- (s0, a, r) of the OLDEST entry -- into
 * the replay buffer.  The learner reads row 0 of s0 (28 numbers, main.py:74), the 7 actions and the target: 36 float32.
 *
 * This is a STATELESS pass over the blocks pve_step_many(trajectory = 1) filled; the handle only supplies n_envs, capacity, the
 * observation element type (PVE_CFG_OBS_F32) and the stream.  It is indexed by a window's START (tick u, env, slot) with
 * PVE_F_CTL set at u and follows the vehicle through new_slot, at most window - 1 links.  A start emits
 *   - a FULL window (`window` entries collected): bootstrapped with q_boot at the closing entry unless that entry is Done;
 *   - a window closed by PVE_F_DONE before it is full ONLY when u is the vehicle's first controlled tick, i.e. its s0 row is all
 *     zero (pve_outputs.obs_post: only a vehicle spawned at the end of the previous tick has one): at Done the reference emits
 *     the oldest buffered entry and drops the younger ones.  mode & PVE_NSTEP_TAIL emits those truncated windows too (the
 *     usual n-step treatment of episode ends);
 *   - nothing when the walk meets a slot without PVE_F_CTL or a -1 link before it closes.
 * Slot-indexed: for lane_num 4 / 8 the reference's `ids` order differs from slot order, which does not matter here.
 *
 * Two segments: `prev` (n_ticks = 0, or >= window; only its last `window` ticks are read) and `cur`, consecutive in time.  A
 * start emits in this call IFF ITS WINDOW CLOSES AT A TICK OF `cur`: starts of `cur` whose walk runs off the end are pending and
 * emit in the next call, when `cur` is passed as `prev`; with prev.n_ticks = 0 the windows that were open before `cur` are lost.
 * Fields of an emitted record: the s0 row = the row the actor consumed at u = obs_post of tick u - 1 at the slot (`obs_first`
 * for the first tick of `cur` when there is no `prev`); the 7 actions = column 2 of the 7 rows of state_pre at u (ref :290);
 * the target in float64: Q' = the float32 of q_boot (pve_bootstrap_q on cur's state_pre / flags) widened to double, then
 * gamma * Q' and every Horner step as separately rounded IEEE operations (no fused multiply-add) -- csrc/pve_nstep.h, bit-equal to
 * pve_mcc_amd/nstep.py.  (The type of the reference's own gamma * Q depends on the NumPy version; this library defines float64.)
 *
 * pve_nstep_scan fills, for the n_cand = min(prev.n_ticks, window - 1) + cur.n_ticks candidate start ticks (tick index relative
 * to cur: -min(..) .. cur.n_ticks - 1), the dense start-indexed `target` (float64) and `code` (int32: entries used in bits 0-7,
 * bit 8 bootstrapped, bit 9 closed by Done; 0 = no transition) [n_cand][n_envs][cap], `offsets` = the index of the first record
 * of every group of 64 slots (int32 [n_cand * n_envs * cap / 64 + 1], the last entry = the count) and `total` (int64, DEVICE).
 * Record order: (tick, env, slot) ascending, whatever the launch geometry (ballot + popcount per wave, no atomics).
 * pve_nstep_gather (same struct, after the scan, same stream) writes the first max_records records in that order:
 * records float32 [max_records][36] = s0 row [28], actions [7], target [1] (cast from the handle's observation type / float64),
 * index int32 [max_records][4] = tick relative to cur (negative: a start in prev), env, slot, code.  `total` always holds the
 * true count.  obs_post / obs_first / records / index must be 16-byte aligned.
 * Errors (PVE_ERR_INVALID): null required pointers, window outside 1 .. 16, gamma NaN or outside [0, 1], 0 < prev.n_ticks <
 * window, cur.n_ticks < 1, max_records < 0, more than 2^31 - 1 candidate slots, a misaligned buffer, a backend without the
 * kernels.  Both calls are asynchronous on the handle's stream and need no pve_reset. */
#define PVE_NSTEP_TAIL 0x1
#define PVE_NSTEP_MAX_WINDOW 16
#define PVE_NSTEP_RECORD 36
typedef struct pve_nstep_segment {
    int32_t n_ticks;
    const void *obs_post;         /* [n_ticks][n_envs][cap][28]   float64, or float32 with PVE_CFG_OBS_F32 */
    const void *state_pre;        /* [n_ticks][n_envs][cap][7][28] same element type */
    const double *reward;         /* [n_ticks][n_envs][cap] */
    const int32_t *flags;         /* [n_ticks][n_envs][cap] */
    const int32_t *new_slot;      /* [n_ticks][n_envs][cap] */
} pve_nstep_segment;
typedef struct pve_nstep {
    double gamma;                 /* main.py:227: tanh((epoch + 6) / 12) * 0.9 */
    int32_t window;               /* seq_max_step + 1 = 13 in the reference */
    int32_t mode;                 /* PVE_NSTEP_* */
    pve_nstep_segment prev, cur;
    const void *obs_first;        /* [n_envs][cap][28]: the rows stored before cur's first tick; read when prev.n_ticks = 0 */
    const float *q_boot;          /* [cur.n_ticks][n_envs][cap] (pve_bootstrap_q) */
    double *target;               /* scan out / gather in */
    int32_t *code;
    int32_t *offsets;
    int64_t *total;
    int64_t max_records;          /* gather */
    float *records;
    int32_t *index;
    int32_t block_threads;        /* 0 = default; diagnostics: threads per workgroup of the scan (a multiple of 64, <= 1024) */
} pve_nstep;
int pve_nstep_scan(pve_handle h, const pve_nstep *ns);
int pve_nstep_gather(pve_handle h, const pve_nstep *ns);

/* REPLAY MEMORY on the device: the uniform store and draw between pve_nstep_gather and pve_critic_forward (reference
 * replay_buffer.py:45-53 `add` and :20-23 `getBatch` with rand_s = True, i.e. `ReplayBuffer(500000, batch_size, learn_start, 50000,
 * rand_s=True)`; main.py:263 `agent1_memory_seq.add(...)`, main.py:50-77 `agent_memory.getBatch(batch_size)` and the split of the batch
 * into obs_batch, the 7 actions and target).  Additive within ABI 9: three new symbols and one new struct, nothing existing changes,
 * PVE_ABI_VERSION stays 9; a binding detects an older library by the missing symbols.
 *
 * RING.  `store` holds `capacity` records of PVE_NSTEP_RECORD = 36 float32 in caller-owned DEVICE memory, `state` is a DEVICE block
 * of PVE_REPLAY_STATE_WORDS int64: state[0] = written (adds ever made = the reference's count()), state[1] = draws (minibatches
 * ever drawn), state[2] = status (live records seen by the latest pve_replay_sample), state[3] reserved.  Record number w (0-based
 * over all adds) lives in slot w mod capacity; the live records are the last L = min(written, capacity), age index a in [0, L) names
 * record written - L + a (0 = the oldest, the left end of the reference's deque).  The reference's deque holds buffer_size - 1
 * entries (num_experiences is incremented before the `<` test, replay_buffer.py:47-49): capacity = 499999 is its 500000.
 * The handle only supplies the device and the stream; one memory belongs to one handle's stream at a time.
 *
 * pve_replay_reset (the reference builds a new ReplayBuffer, main.py:212) zeroes the state block; the store needs no clearing.
 * pve_replay_append (replay_buffer.py:45-53) appends the first n = min(*total_dev, n_max) records of `records` in order; total_dev
 * is a DEVICE int64 (pve_nstep.total, so there is no host synchronisation; negative counts as 0) or NULL for n = n_max.  Of a
 * chunk with n > capacity only the last `capacity` records are written (the others would be overwritten within the same call),
 * `written` grows by n.  records must not overlap the store.
 * pve_replay_sample (replay_buffer.py:20-23, main.py:50-77) draws n_batches minibatches of `batch` distinct live records each --
 * uniform, without replacement within a minibatch -- and writes them split the way pve_critic_forward(rows, act7) takes them:
 *   rows float32 [n_batches][batch][28], act7 float32 [n_batches][batch][7], target float32 [n_batches][batch],
 *   seq int64 [n_batches][batch] = the record numbers w.
 * With fewer than `batch` live records (the reference raises ValueError) it writes seq = -1 and zeros and leaves `draws` alone;
 * otherwise draws grows by n_batches.  Either way state[2] = L, which a caller may read to tell the two apart.
 * THE DRAW (csrc/pve_replay.h, restated in pve_mcc_amd/replay.py; the reference's Mersenne-Twister draw is not reproduced):
 * minibatch number d = draws, draws + 1, .. takes the age indices perm(seed, d, L)(j), j = 0 .. batch - 1, where perm(seed, d, N) is
 * a bijection of [0, N) and a pure function of its arguments (not of the launch geometry, the batch size or n_batches):
 *   b = bit length of N - 1, at least 2, rounded up to even, h = b / 2; an 8-round Feistel network over (L, R) = the high / low h bits,
 *   (L, R) <- (R, L ^ F_r(R)), r = 0 .. 7, with F_r(R) = output word 0, masked to h bits, of Philox4x32-10 with
 *   counter = (R, r, d low word, d high word) and key = (seed low word ^ 0x5245504C, seed high word ^ 0x41594D45)
 *   (the tag keeps these inputs apart from pve_set_action_noise's, whose key is the bare seed); cycle walk: x = j, then
 *   x <- Feistel(x) until x < N.
 * block_threads: 0 = default; diagnostics: threads per workgroup of both kernels (a multiple of 64, <= 1024; same results).
 * Errors (PVE_ERR_INVALID): null pointers, capacity outside 1 .. 2^31 - 1, batch < 1, batch > capacity, n_batches < 1,
 * batch * n_batches > 2^31 - 1, n_max < 0, store / records / rows / act7 not 16-byte aligned (state / total_dev / seq: 8,
 * target: 4), a bad block_threads, a backend without the kernels.  All three calls are asynchronous on the handle's stream and
 * need no pve_reset. */
#define PVE_REPLAY_STATE_WORDS 4
typedef struct pve_replay {
    int64_t capacity;             /* records */
    float *store;                 /* DEVICE [capacity][36] */
    int64_t *state;               /* DEVICE [PVE_REPLAY_STATE_WORDS] */
    uint64_t seed;                /* of the draw */
    int32_t block_threads;
} pve_replay;
int pve_replay_reset(pve_handle h, const pve_replay *rp);
int pve_replay_append(pve_handle h, const pve_replay *rp, const float *records /* [n_max][36] */,
                      const int64_t *total_dev /* DEVICE, or NULL */, int64_t n_max);
int pve_replay_sample(pve_handle h, const pve_replay *rp, int64_t batch, int64_t n_batches, float *rows, float *act7,
                      float *target, int64_t *seq);

/* LEARNER STEP on the device: what the reference runs on a minibatch behind getBatch (main.py:48-84 `train_agent_seq`:
 * model_agent_maddpg.py:85-118 `train_critic`, then `train_actor`, then main.py:19-33 the soft updates of both targets).
 * Additive within ABI 9: two new symbols and one new struct, nothing existing changes, PVE_ABI_VERSION stays 9; a binding
 * detects an older library by the missing symbols.  The arithmetic -- every order of summation, Adam, the tanh -- is stated once
 * in csrc/pve_learn.h, which a host compiler builds as well; the kernel computes that, bit for bit, whatever block_threads.
 *
 * `params` is a caller-owned DEVICE block of PVE_LEARNER_N_FLOATS float32.  Segments (float offsets, each 16-byte aligned):
 *   PVE_LEARNER_ACTOR / _CRITIC / _TARGET_ACTOR / _TARGET_CRITIC   the four networks, in exactly the layouts pve_set_actor and
 *       pve_set_target_networks take: pve_set_actor(h, params + PVE_LEARNER_ACTOR) installs the new policy with no host copy
 *   PVE_LEARNER_M_ACTOR / _V_ACTOR / _M_CRITIC / _V_CRITIC          Adam's moments
 *   PVE_LEARNER_POWERS   beta1^t, beta2^t of the actor's optimizer, then of the critic's
 *   PVE_LEARNER_STEPS    int32: steps taken (+ 3 reserved words)
 *   PVE_LEARNER_GRAD     the gradients of the latest step: critic [6841] (padded to 6844), then actor [6393]
 * pve_learner_init (main.py:203-204) copies the networks in (DEVICE pointers; a NULL target = a copy of the online network),
 * zeroes moments, count and gradients and sets the powers to beta1, beta2.
 * pve_learner_step runs n_batches steps in sequence in ONE launch of one workgroup, on
 *   rows float32 [n_batches][batch][28], act7 float32 [n_batches][batch][7], target float32 [n_batches][batch]
 * (what pve_replay_sample writes).  Per step: 1. critic_loss = mean((target - Q)^2), Adam on the critic; 2. actor_loss =
 * -mean(Q(s, [actor(s), act7[1..6]])) with the UPDATED critic, gradients with respect to the actor only, Adam on the actor;
 * 3. target = c1 * online + c2 * target for both, c1 = float32(1.0 - (double)tau), c2 = float32(tau).  Adam is TF 1.x ApplyAdam
 * in float32 (csrc/pve_learn.h).  losses [n_batches][2] = critic, actor loss of each step, or NULL; grads
 * [n_batches][6841 + 6393] = the gradients each step applied, critic then actor, or NULL.  PVE_LEARN_CRITIC_ONLY skips 2. and the
 * actor's soft update (actor loss and gradients are reported as 0).
 * Not part of the step: td_error / update_priority (main.py:76-79; dead with rand_s = True) are pve_critic_forward on the sampled
 * rows + pve_prio_update (below); the summaries are NOT reproduced.  The reference assigns
 * self.critic_lr after the optimizer is built, which changes nothing there; here both learning rates are read on every call.
 * block_threads: 0 = 1024; else a multiple of 64 up to 1024 (same results).
 * epsilon: any finite float32.  A subnormal value (1e-40f) is honoured as it stands: sqrtf(v) + epsilon is a float32 add with
 * subnormal operands and results kept, as every operation of the step is.  epsilon = 0 is accepted as well; a parameter whose
 * gradient has been exactly zero in every step (m = v = 0: a weight behind a unit that never fires) then takes 0 / 0, and it and
 * its target become NaN.
 * Errors (PVE_ERR_INVALID): null pointers, batch < 1, n_batches < 1, batch * n_batches > 2^31 - 1, params / rows / networks not
 * 16-byte aligned (the others: 4), learning rates, epsilon or tau not finite, tau outside [0, 1], beta outside [0, 1), a bad
 * block_threads, a backend without the kernel.  Both calls are asynchronous on the handle's stream and need no pve_reset. */
#define PVE_LEARNER_ACTOR 0
#define PVE_LEARNER_CRITIC 6396
#define PVE_LEARNER_TARGET_ACTOR 13240
#define PVE_LEARNER_TARGET_CRITIC 19636
#define PVE_LEARNER_M_ACTOR 26480
#define PVE_LEARNER_V_ACTOR 32876
#define PVE_LEARNER_M_CRITIC 39272
#define PVE_LEARNER_V_CRITIC 46116
#define PVE_LEARNER_POWERS 52960
#define PVE_LEARNER_STEPS 52964
#define PVE_LEARNER_GRAD 52968
#define PVE_LEARNER_N_FLOATS 66208
#define PVE_LEARN_CRITIC_ONLY 0x1
typedef struct pve_learner {
    float *params;                /* DEVICE [PVE_LEARNER_N_FLOATS] */
    float actor_lr, critic_lr;    /* reference: 1e-4, 1e-3 */
    float beta1, beta2, epsilon;  /* tf.train.AdamOptimizer's defaults: 0.9, 0.999, 1e-8 */
    float tau;                    /* weight of the OLD target (main.py:30); reference 0.998 */
    int32_t flags;                /* PVE_LEARN_* */
    int32_t block_threads;
} pve_learner;
int pve_learner_init(pve_handle h, const pve_learner *lrn, const float *actor, const float *critic,
                     const float *target_actor /* NULL = actor */, const float *target_critic /* NULL = critic */);
int pve_learner_step(pve_handle h, const pve_learner *lrn, const float *rows, const float *act7, const float *target,
                     int64_t batch, int64_t n_batches, float *losses /* or NULL */, float *grads /* or NULL */);

/* THE WIDE LEARNER STEP: the same step (main.py:48-84) on batches larger than the reference's 128, spread over the chip.
 * Additive within ABI 9: one new symbol, PVE_ABI_VERSION stays 9.  A batch of `batch` rows is ceil(batch / PVE_LEARN_SLICE)
 * slices of 128 rows (the last may be shorter).  Every slice is worked like a batch of pve_learner_step, its sums starting from 0
 * at its first row, with dQ scaled by the WHOLE batch; the gradient of a parameter, and each loss sum, is then partial[0] +
 * partial[1] + ... in ascending slice order, plain float32 adds, and Adam and the soft update follow unchanged
 * (csrc/pve_learn.h, learn_steps_wide: the definition, which a host compiler builds as well).  For batch <= 128 the result is
 * pve_learner_step's bit for bit; for larger batches it is another, equally fixed order of summation: it depends on `batch`
 * alone, not on `groups`, block_threads or the device.
 * Per minibatch four launches on the handle's stream (slice pass and apply for the critic, then for the actor with the updated
 * critic; two with PVE_LEARN_CRITIC_ONLY), no host synchronisation; n_batches steps are enqueued in order.
 * work: caller-owned DEVICE scratch of work_floats >= PVE_LEARNER_WIDE_FLOATS(batch) float32, 16-byte aligned: one row of
 * PVE_LEARNER_WIDE_ROW floats per slice (critic gradients padded to 6844, actor gradients padded to 6396, the two loss sums + 2
 * reserved).  It needs no initialisation: whatever is read was written by the same call.  It must not be shared by calls on
 * different streams.  groups: workgroups of the slice passes; 0 = one per slice, at most one per compute unit.
 * Everything else, and every error, as pve_learner_step; in addition PVE_ERR_INVALID for a null or misaligned work, a work_floats
 * too small and groups < 0. */
#define PVE_LEARN_SLICE 128
#define PVE_LEARNER_WIDE_ROW 13244
#define PVE_LEARNER_WIDE_FLOATS(batch) ((((batch) + 127) / 128) * PVE_LEARNER_WIDE_ROW)
int pve_learner_step_wide(pve_handle h, const pve_learner *lrn, const float *rows, const float *act7, const float *target,
                          int64_t batch, int64_t n_batches, float *work, int64_t work_floats, int32_t groups,
                          float *losses /* or NULL */, float *grads /* or NULL */);

/* RANK-BASED PRIORITISED REPLAY on the device: the memory the reference builds in every run (replay_buffer.py:13-18 constructs
 * rank_based.Experience) and draws from with rand_s = False (replay_buffer.py:24, rank_based.py:148-188 `sample`), with the update
 * main.py:76-79 makes from the target critic (`td_error = |target_Q(obs, act, other) - target|`, `update_priority`).  Additive
 * within ABI 9: five new symbols and one new struct, nothing existing changes, PVE_ABI_VERSION stays 9; a binding detects an older
 * library by the missing symbols.  The specification is csrc/pve_prio.h (host + device), restated in NumPy as
 * PrioritizedReplayModel (pve_mcc_amd/replay.py).  Every integer part is bit-exact; the only floating-point arithmetic is the
 * update's one subtraction (exact IEEE) and the importance weight.
 *
 * `replay` is the ring of pve_replay (reset, appended to and counted through the pve_replay_* calls, unchanged) with
 * capacity = the reference's `size`: rank_based.py:82-99 cycles its index over 1 .. size (e_id = slot + 1, slot = w mod capacity).
 * PRIORITY STORE (caller-owned DEVICE memory): prio uint32 [capacity] = the bit pattern of a non-negative float32; pseq int64
 * [capacity].  The priority of slot s is valid only if pseq[s] is the record number living in s now; otherwise the record is NEW
 * and ranks as +inf (rank_based.py:114-117: a new record gets the heap's maximum).  pstate int64 [PVE_PRIO_STATE_WORDS]:
 * pstate[0] = pdraws (minibatches ever drawn), [1] = live records seen by the latest ranking, [2] = its partition index,
 * [3] = ids ignored by the latest update.
 * pve_prio_reset fills pseq with -1 and zeroes pstate (it does not touch the ring: pve_replay_reset does).
 * pve_prio_rank (binary_heap.py:194-221 `balance_tree` / `priority_to_experience`) writes order int32 [L]: order[r] = the age
 * index of the record of rank r + 1 among the L = min(written, capacity) live records, sorted descending by (priority bits, record
 * number) -- a total order; NEW records first, newest first.  For pairwise distinct priorities this is the reference's
 * priority_to_experience(1 .. L) after rebalance(); the reference's order among ties follows its heap layout and is NOT reproduced.
 * The result is a pure function of the memory's contents (not of block_threads or of what the scratch held).
 * STRATA TABLES, built by the caller as rank_based.py:40-80: part_from int64 [32] (HOST) = for k = 0 .. 31 the smallest L with
 * floor(1.0 * L / size * 32) >= k + 1 (rank_based.py:159; unused trailing entries may be 2^62); the partition index of L is the
 * number of thresholds <= L, partition p >= 1 uses row p - 1 of ends int32 [32][batch + 1] (`strata_ends`: ends[0] = 0,
 * ends[batch] = n_p = p * floor(size / 32)).  `ends` is the DEVICE copy the kernel reads, `ends_host` the same table in HOST memory,
 * which every call validates (each row starts at 0 and is non-decreasing within 0 .. capacity).
 * pve_prio_sample (rank_based.py:148-188) ranks first, always, then draws minibatches d = pdraws, pdraws + 1, ..: stratum j =
 * 0 .. batch - 1 takes  lo = min(ends[j] + 1, ends[j + 1]), hi = max(ends[j] + 1, ends[j + 1])  (rank_based.py:167-172, the swapped
 * randint of degenerate strata included: ranks may repeat within a minibatch),  rank = lo + mulhi32(u, hi - lo + 1)  with u = word 0
 * of Philox4x32-10, counter = (j, 0, d low word, d high word), key = (seed low word ^ 0x5052494F, seed high word ^ 0x52414E4B),
 * clamped to 1 .. L (inactive for tables built as above).  The record is age index order[rank - 1], record number written - L + age.
 * The reference's Mersenne-Twister draw is not reproduced.  Outputs: rows / act7 / target / seq as pve_replay_sample writes them,
 * rank int32 [n_batches][batch], weight float32 [n_batches][batch] = (rank / rank_max)^alpha_beta with rank_max the minibatch's
 * largest rank (rank_based.py:176-182 with the normaliser and partition_max cancelled; alpha_beta = alpha * beta as one float32).
 * With L < min_live, or L below part_from[0], the call is short: seq = -1 and zeros, pdraws unchanged; pstate[1] = L either way.
 * pve_prio_update (main.py:76-79, rank_based.py:138-146) stores p = |q[i] - target[i]| in float32 (|q[i]| when target is NULL; NaN
 * is stored as +inf) as the priority of record seq[i], i < n.  An id outside [written - L, written) -- -1, or a record overwritten
 * since -- is ignored and counted in pstate[3] (the reference would write onto the slot's new occupant).  Of an id named several
 * times in one call the largest p wins; the old value is replaced, not maxed.
 * scratch: caller-owned DEVICE memory of scratch_bytes >= pve_prio_scratch_bytes(capacity), 16-byte aligned, for the ranking; it
 * needs no initialisation and must not be shared by calls on different streams.  pve_prio_scratch_bytes returns 0 for a capacity
 * outside 1 .. 2^31 - 1.  replay.block_threads: diagnostics as in pve_replay (same results).
 * Errors (PVE_ERR_INVALID): what pve_replay_* reject in `replay`; null prio / pseq / order / pstate / scratch / ends / ends_host /
 * part_from / outputs / seq / q; scratch not 16-byte aligned (pseq, pstate, seq: 8; the others: 4; rows and act7: 16); a
 * scratch_bytes too small; batch outside 1 .. capacity; part_from below 1 or decreasing; an `ends_host` row that does not start
 * at 0, decreases or passes capacity; n_batches < 1; batch * n_batches > 2^31 - 1; min_live < 0; alpha_beta negative or not
 * finite; n < 0; a backend without the kernels.  All calls are asynchronous on the handle's stream, none synchronises. */
#define PVE_PRIO_STATE_WORDS 4
#define PVE_PRIO_PARTS 32
typedef struct pve_prio {
    pve_replay replay;            /* the ring; capacity = the reference's `size` */
    uint32_t *prio;               /* DEVICE [capacity] */
    int64_t *pseq;                /* DEVICE [capacity] */
    int32_t *order;               /* DEVICE [capacity] */
    int64_t *pstate;              /* DEVICE [PVE_PRIO_STATE_WORDS] */
    void *scratch;                /* DEVICE [scratch_bytes] */
    int64_t scratch_bytes;
    const int32_t *ends;          /* DEVICE [PVE_PRIO_PARTS][batch + 1] */
    const int32_t *ends_host;     /* HOST   [PVE_PRIO_PARTS][batch + 1], the same table */
    const int64_t *part_from;     /* HOST   [PVE_PRIO_PARTS] */
    int64_t batch;
} pve_prio;
size_t pve_prio_scratch_bytes(int64_t capacity);
int pve_prio_reset(pve_handle h, const pve_prio *pp);
int pve_prio_rank(pve_handle h, const pve_prio *pp);
int pve_prio_sample(pve_handle h, const pve_prio *pp, int64_t n_batches, int64_t min_live, float alpha_beta, float *rows,
                    float *act7, float *target, int64_t *seq, int32_t *rank, float *weight);
int pve_prio_update(pve_handle h, const pve_prio *pp, const int64_t *seq, const float *q, const float *target /* or NULL */,
                    int64_t n);

/* ARRIVAL STREAMS generated on the device: the per-episode input that the reference reads with scipy.io.loadmat (main.py:228-229,
 * :388-389 `arvTimeNewVeh`) and, for the 8-lane layout, the random.randint(0, 1) it draws per arriving vehicle (ref :381, :390),
 * written in place on the handle's stream.  Additive within ABI 9: one new symbol (declared in include/pve_env_arrivals.h) and one
 * new struct, nothing existing changes, PVE_ABI_VERSION stays 9; a binding detects an older library by the missing symbol.  The specification is csrc/pve_arrivals.h
 * (host + device), restated in NumPy as pve_mcc_amd.arrivals.device_arrivals / device_intentions; every implementation is
 * bit-equal to it.
 * arrivals: float64 [n_envs][rows][lane_num] (n_envs and lane_num are the handle's), the layout pve_set_arrivals takes with
 * env_stride_rows = rows.  With env_global = env index + env_offset, row r < rows - 1 and lane l:
 *   w = output word (r & 3) of Philox4x32-10, counter = ((r >> 2) | (l << 28), epoch, env_global low word, env_global high word),
 *   key = (seed low word ^ 0x41525256, seed high word ^ 0x54494D45)  -- apart from the exploration noise (raw seed) and the
 *   prioritised draw (^ 0x5052494F / 0x52414E4B) under one seed;
 *   x = -ln((2 w + 1) 2^-33) in the exact binary64 arithmetic pve_arrivals.h writes down (x in [1.16e-10, 22.874], never 0);
 *   d = mean * x, raised to min_gap_s if below;  t[0] = d[0], t[r] = t[r-1] + d[r]: float64 additions in ascending r.
 * mean = mean_s seconds (3600 / rate in veh/h/lane), or mean_env[env] when mean_env is not NULL (DEVICE memory: its entries must
 * be finite and > 0, which the call cannot check).  Row rows - 1 is +inf in every lane.  A chain is a pure function of (seed,
 * epoch, env_global, l, r): fewer rows give a prefix, a batch cut into pieces with matching env_offset gives the same streams.
 * With min_gap_s = 1, t[r] >= r + 1 exactly, so rows - 1 seconds of run are always covered.
 * intentions (lane_num = 8 only, or NULL): int32 [n_envs][rows][8], entry (e, r, l) = bit (r & 31) of output word ((r >> 5) & 3)
 * of Philox4x32-10 with counter = ((r >> 7) | (l << 28), epoch, env_global low word, env_global high word), key = (seed low word
 * ^ 0x494E5445, seed high word ^ 0x4E54494F); every row, the layout pve_set_intentions takes with env_stride_rows = rows.
 * covered (or NULL): float64 [n_envs], covered[e] = min over lanes of t[e][rows - 2][l]: how far the stream is sure to reach.
 * The call is asynchronous on the handle's stream and never synchronises.  It does NOT install the stream: pve_set_arrivals /
 * pve_set_intentions (which only record pointers) do, before or after.  block_threads: 0 = default; else a multiple of 64 up to
 * 1024 (diagnostics: same results).
 * Errors (PVE_ERR_INVALID): null h / g / arrivals; env_offset < 0; rows outside 2 .. 2^28; mean_env NULL and mean_s not finite or
 * <= 0; min_gap_s negative or not finite; block_threads; intentions with lane_num != 8; arrivals or intentions not 16-byte
 * aligned, covered or mean_env not 8-byte aligned; a backend without the kernels. */
typedef struct pve_arrival_gen {
    uint64_t seed;
    int64_t  env_offset;      /* >= 0 */
    uint32_t epoch;
    int32_t  rows;            /* 2 .. 2^28 */
    double   mean_s;          /* finite, > 0; used when mean_env is NULL */
    const double *mean_env;   /* DEVICE [n_envs] or NULL */
    double   min_gap_s;       /* finite, >= 0 */
    int32_t  block_threads;   /* 0 = default */
} pve_arrival_gen;
/* The prototype of the call is in include/pve_env_arrivals.h, an extension header of its own: this file's list of entry points
 * stays the 44 that bindings and checks of ABI 9 count; entry points added later come in such headers. */

/* MANY TICKS, host out of the loop: the reference's episode loop `for i in range(1000): ... step / scene_update /
 * delete_vehicle` (main.py:397-441) with the action source on the device, as ONE call.  Tick k of the call is exactly
 * pve_step_all() with
 *   PVE_SRC_ZERO   actions = 0 (the zero policy of SURVEY.md 8d)
 *   PVE_SRC_POOL   actions = pool[(pool_tick0 + k) % n_pool], pool = DEVICE float64 [n_pool][n_envs][capacity]
 *   PVE_SRC_TABLE  actions[slot] = table[(pool_tick0 + k) % n_pool][min(id of the vehicle in the slot, table_ids - 1)], table =
 *                  DEVICE float64 [n_pool][table_ids] passed in `pool`: a policy that is a function of (tick, vehicle id), e.g.
 *                  the sin tape of SURVEY.md 8c-ii / BASELINE.md 3, `a = sin(0.37 id + 0.05 tick)`; the vehicle's own thread
 *                  gathers its action (lane_num 12, resident kernel only)
 *   PVE_SRC_ACTOR  actions = pve_actor_forward(actor_weights, observation rows the previous tick stored), i.e. the closed
 *                  loop of main.py:398-441 with the actor of model_agent_maddpg.py:23-49; the first tick reads
 *                  `actor_obs` (zeros after pve_reset, ref :380), later ticks the rows written through out->obs_post,
 *                  which is therefore required (and may be the same buffer as actor_obs when trajectory = 0)
 * and the results are bit-identical to n_ticks separate calls (tested).  The ticks run inside one kernel launch with the
 * intersection state resident on the chip between ticks (k_rollout for lane_num 12, k_rollout_geo for lane_num 4 / 8: no
 * state traffic to HBM, only the per-tick outputs) -- PVE_SRC_ACTOR included: the actor runs inside that kernel on the rows
 * the tick has just stored (with PVE_CFG_ACTOR_F32, or together with the training outputs for lane_num 4 / 8: an actor launch
 * + a tick launch per tick, enqueued from C).
 * trajectory = 0: every tick overwrites the `out` buffers (the last tick's outputs remain; metrics accumulate in the
 * handle as usual); trajectory = 1: every non-NULL `out` buffer holds n_ticks consecutive per-tick blocks
 * ([n_ticks][n_envs][cap]...), the roll-out a trainer consumes.  The training outputs (lane_num 12): obs_pre may be
 * requested in either form; state_pre needs trajectory = 1 (tick k reads the stale neighbour rows from block k - 1 of
 * obs_post, tick 0 from out->obs_prev_post = the rows stored before this call), i.e. a MADDPG trainer gets `re_state` and the
 * 7-action vectors (column 2 of the 7 rows, ref :290) of every tick of the roll-out without leaving the resident kernel. */
enum { PVE_SRC_ZERO = 0, PVE_SRC_POOL = 1, PVE_SRC_ACTOR = 2, PVE_SRC_TABLE = 3 };
typedef struct pve_rollout {
    int32_t n_ticks;
    int32_t source;               /* PVE_SRC_* */
    const double *pool;           /* PVE_SRC_POOL */
    int32_t n_pool, pool_tick0;
    const float *actor_weights;   /* PVE_SRC_ACTOR: NULL = the actor installed by pve_set_actor; else DEVICE float32[PVE_ACTOR_N_WEIGHTS], installed first */
    const void *actor_obs;        /* PVE_SRC_ACTOR: rows the first tick's actor reads (float64, or float32 with PVE_CFG_OBS_F32) */
    double *actor_actions;        /* PVE_SRC_ACTOR: DEVICE scratch float64 [n_envs][capacity] (per-tick launches only: the resident
                                     kernel keeps the actions on the chip and does not touch it) */
    int32_t trajectory;
    int32_t table_ids;            /* PVE_SRC_TABLE: columns of the table (vehicle ids beyond it use the last column) */
    int32_t chunk_ticks;          /* 0: all n_ticks in one launch; > 0: launches of at most chunk_ticks ticks each (same results).
                                     Every workgroup of a launch runs its intersection for all the ticks of the launch, so a
                                     launch lasts as long as its slowest intersection: with several handles stepped on their
                                     own streams, shorter launches let the other handles' workgroups fill the slots that the
                                     fast intersections free (bench.py --chunk). */
    int32_t persistent;           /* 1 (with 0 < chunk_ticks < n_ticks, chunk_ticks <= 255): the whole call is ONE launch of as many
                                     workgroups as the chip holds at once; they pull (intersection, chunk) items from a queue in the
                                     handle's workspace, so nothing waits in launch order for the slowest intersection of a chunk
                                     (the reference's episode loop main.py:397-441 has no such boundary either).  Same results as
                                     persistent = 0.  Eligible: lane_num 12 with every source (ZERO / POOL / TABLE / ACTOR unless
                                     PVE_CFG_ACTOR_F32), with or without trajectory = 1, with or without the training outputs
                                     obs_pre / state_pre; lane_num 4 / 8 with every source (TABLE: without the training outputs, as everywhere for these
                                     layouts); the training outputs through the queue with ZERO / POOL (with ACTOR: the resident
                                     kernel in chunked launches -- that roll-out is bound by its state writes).
                                     Anything else is run as chunked launches (pve_debug_last_launch tells which).
                                     PVE_SRC_ACTOR: `actor_actions` is the hand-off buffer between the items of an intersection
                                     (every item's last tick stores the next actions there, the next item reads them): it must
                                     not alias any other buffer of the call.
                                     A persistent call must run to completion ONCE: its hand-off counters live partly in the
                                     handle (host) and partly in the workspace (device), so it must not be captured into a HIP
                                     graph or replayed; after a failed launch / stream error both sides are reset. */
} pve_rollout;
int pve_step_many(pve_handle h, const pve_rollout *ro, const pve_outputs *out);

/* Host read-back (synchronises the stream). */
int pve_read_env(pve_handle h, int env, pve_env_info *out);
int pve_read_vehicles(pve_handle h, int env, pve_vehicle *out, int max_n, int *n_out);
int pve_get_metrics(pve_handle h, double out[PVE_N_METRICS]);

/* Device views of the persistent per-slot state for zero-copy consumers (actor input masks):
 * field = "p","v","a","jerk","jerk_sum","vir_dis","closer_p" (float64 [n_envs][cap]) or
 * "id","seq","vnum","step","count","meta","hdr" (int32 [n_envs][cap]); meta bit0 = control.
 * Value range of a caller's writes: "seq" (seq_in_lane: the row of the arrival stream the vehicle came from) and "vnum"
 * (id_info[1]) are carried by the 128-slot queue form of pve_step_many in ONE packed word, seq << 8 | vnum, so there
 *   0 <= seq < 2^23   and   0 <= vnum < 256
 * must hold.  The library's own values keep to it: vnum is a lane's vehicle count (at most the capacity), and a stream of
 * rows >= 2^23, whose cursors could pass the range, takes the kernel build that carries the two fields in registers
 * (pve_debug_last_variant: waves_per_simd 4 instead of 5).  Tested at the top of the range, seq = 2^23 - 2 .. 2^23 - 129. */
int pve_state_field(pve_handle h, const char *field, void **dev_ptr, int *elem_bytes);
#define PVE_META_CONTROL 0x1
#define PVE_META_FINISH  0x2
#define PVE_META_DONE    0x4
#define PVE_META_LOCK    0x8

int pve_synchronize(pve_handle h);

/* Diagnostics: accumulate per-phase clock ticks (wall_clock64: the 100 MHz constant clock) of every wave of the tick kernel into a
 * zeroed DEVICE buffer of uint64 [n_envs * capacity/64][16], one row per wave, added to by every armed launch; NULL disables.
 * The kernels write twelve columns (tools/phase_profile.py: PHASES):
 *   0 load, 1 step1, 2 step2+listsA, 3 step3+listsB, 4 build, 5 rank, 6 reward+xy (behind the walk, with the closing barrier),
 *   7 effects, 8 lock, 9 final, 10 state (the state_pre pass: 0 when it is not requested; 12 lanes), 11 walk(merge)
 * and the diagnostics build of the resident roll-out kernel (PHASES_MANY: 0 = the reload barrier, 10 = stage+reload) two more:
 *   12 shader-clock cycles of the launch (clock64), 13 its wall_clock64 ticks (12 / 13 = shader clock in units of 100 MHz);
 * columns 14 and 15 are never written.  Used by tools/phase_profile.py; no effect on results (tested: state, outputs and metrics
 * of an armed batch equal its twin's bit for bit).
 * While armed, the stepping calls launch the diagnostics builds (pve_debug_last_variant: prof = 1): pve_step_all and the 4- / 8-lane
 * ticks as usual; pve_step_many with PVE_SRC_ZERO / PVE_SRC_POOL, 64 or 128 slots, 12 lanes and no training outputs in the resident
 * kernel (persistent = 1: as chunked launches); every other configuration as one launch per tick -- except PVE_SRC_TABLE, which has
 * no per-tick form and is REFUSED with PVE_ERR_STATE while armed (lane_num 12, 4 and 8; nothing is launched, state and tick count
 * stay as they were; the same call succeeds after pve_debug_phase_cycles(h, NULL)). */
int pve_debug_phase_cycles(pve_handle h, uint64_t *dev_counters16);

/* Diagnostics: what the last stepping call on this handle launched.  (Which kernel variant behind the form: the extension header
 * include/pve_env_debug.h.) */
enum { PVE_LAUNCH_NONE = 0, PVE_LAUNCH_TICK = 1 /* one launch per tick */, PVE_LAUNCH_RESIDENT = 2 /* one k_rollout launch per chunk */,
       PVE_LAUNCH_PERSISTENT = 3 /* ONE launch for the call, items pulled from the work queue */ };
int pve_debug_last_launch(pve_handle h);

/* Diagnostics: the item schedule pve_step_many lays out for a persistent call of n_ticks ticks with items of at most chunk_ticks
 * ticks (the per-episode loop `for i in range(1000)` of main.py:397 cut into queue items): out[0] = ticks per full item, out[1] =
 * full items, out[2] = tapered items behind them, out[3 .. 10] = their lengths, out[11] = items per intersection.  Host only. */
int pve_debug_item_schedule(int n_ticks, int chunk_ticks, int32_t out[12]);

/* Diagnostics: every later pve_step_all / pve_scene_update launch of the 12-lane kernel (k_tick) RETURNS behind phase n
 * (0 load, 1 step1, 2 step2, 3 step3, 4 build, 5 rank, 6 walk + reward, 7 effects, 8 lock) without writing any state (tested: the fourteen state
 * fields, the headers and the metrics are bit-identical behind a truncated launch, for every n and capacity), so that hardware counters of truncated launches on one frozen state attribute instructions and LDS conflicts to phases
 * (tools/phase_counters.sh); n < 0 restores the full tick.  The results of truncated launches are meaningless. */
int pve_debug_stop_phase(pve_handle h, int n);

/* Diagnostics: launch a kernel that performs exactly the tick's state-load pattern over every slot
 * (72 B per slot read: 6 x f64 + 6 x i32) and stores one int per env into dev_sink[n_envs]; a known byte
 * count for calibrating rocprofv3 FETCH_SIZE on this access width. */
int pve_debug_traffic_probe(pve_handle h, int32_t *dev_sink);

#ifdef __cplusplus
}
#endif
#endif /* PVE_ENV_H */

// pve_capi.inc -- the extern "C" entry points of include/pve_env.h, written once against a
// `Backend` (static interface) that the including translation unit defines before this file:
//
//   struct Backend : pve::BackendDefaults {
//     static int   set_device(int dev, std::string &err);
//     static int   enter_device(int dev);  static void leave_device(int prev);   // make dev current, return the previous one
//     static void *dmalloc(size_t n);            static void dfree(void *p);
//     static int   memset0(void *p, size_t n, void *stream);
//     static int   n_xcc(int dev);               // XCDs of the device (shards of the persistent roll-out's queue)
//     static int   d2h(void *dst, const void *src, size_t n, void *stream);   // synchronous
//     static int   sync(void *stream, std::string &err);
//     static int   launch_tick(const pve::Const &, const pve::Params &, int cap, void *stream, std::string &err);
//     static int   launch_compact(const pve::Params &, int cap, void *stream, std::string &err);
//     static int   launch_reset(const pve::Const &, const pve::Params &, int cap, void *stream, std::string &err);
//     static int   launch_tick_geo(const pve::GeoConst &, const pve::Params &, int cap, void *stream, std::string &err);
//     static int   launch_reset_geo(const pve::GeoConst &, const pve::Params &, int cap, void *stream, std::string &err);
//     static int   launch_rollout(const pve::Const &, const pve::Params &, const pve::RolloutArgs &, int cap, void *stream,
//                                 std::string &err);    // 0 = launched, 1 = no resident kernel for this configuration, -1 = error
//     static int   launch_rollout_geo(const pve::GeoConst &, const pve::Params &, const pve::RolloutArgs &, int cap, void *stream,
//                                     std::string &err);    // (both: only a backend without the noisy launchers)
//     static int   pack_actor(const float *W, float *flat, unsigned char *packed, void *stream, std::string &err);   // pve_set_actor
//     static int   launch_actor(const float *flat, const unsigned char *packed, const void *obs, int mode, const int32_t *meta,
//                               double *actions, int n_envs, int cap, void *stream, std::string &err);
//     static int   launch_probe(const pve::Params &, int cap, int32_t *sink, void *stream, std::string &err);   // pve_debug_traffic_probe
//   };
//
// That is the mandatory part.  The optional part -- max_capacity and the launchers of the feature groups -- is declared, with
// bodies that refuse, in pve::BackendDefaults (pve_host.h); pve::Provides says which groups a backend overrides.  This file calls
// the mandatory part as Backend:: and the optional part as Opt:: (pve::Contract<Backend>: Backend itself, or, for a Backend that
// does not derive from the defaults, Backend with the defaults beside it).
// pve_hip.hip supplies the HIP backend (the product, every group); tests/emu and tests/emu_wide host loops used only by the CPU
// tests (no group).

using namespace pve;
typedef Contract<Backend> Opt;

#ifndef PVE_KNOB                 // (A/B knobs of the measurement tooling: compiled in with -DPVE_AB_KNOBS only, see pve_hip.hip)
#define PVE_KNOB(name_) ((const char *)nullptr)
#endif

// Every entry point that launches or copies runs with the handle's device current and restores the caller's device on
// the way out: a process may hold handles on several GPUs, and torch may switch the current device between two calls.
struct DevScope {
    int prev;
    explicit DevScope(int dev) : prev(Backend::enter_device(dev)) {}
    ~DevScope() { Backend::leave_device(prev); }
};

static Params base_params(pve_handle h)
{
    Params P;
    memset(&P, 0, sizeof(P));
    P.headers = (EnvHeader *)(h->ws + h->L.off_headers);
    for (int k = 0; k < NF64; k++) P.f64[k] = (double *)(h->ws + h->L.off_f64[k]);
    for (int k = 0; k < NI32; k++) P.i32[k] = (int32_t *)(h->ws + h->L.off_i32[k]);
    P.arrivals = h->arrivals;
    P.arr_env_stride = h->arr_stride;
    P.rows = h->rows;
    P.n_envs = h->n_envs;
    P.phase_cycles = h->phase_cycles;
    P.stop_phase = h->stop_phase;
    P.choice = h->choice;
    P.choice_env_stride = h->choice_stride;
    P.obs_f32 = (h->cfg.flags & PVE_CFG_OBS_F32) ? 1 : 0;
    P.geo_scan = (h->cfg.flags & PVE_CFG_GEO_SCAN) ? 1 : 0;
    return P;
}

// The persistent roll-out's hand-off state is split between the host (h->q_done_base, baked into the kernel arguments) and the
// device (done[], queue heads, owners).  They move together as long as every launch runs to completion; after a failed
// launch or a stream error both sides start from zero again (q_take would otherwise never wait -- or spin forever).
static int queue_reset(pve_handle h)
{
    h->q_done_base = 0;
    return Backend::memset0(h->ws + h->L.off_queue, sizeof(RolloutQueue) + 4 * (size_t)h->n_envs, h->stream);
}

static void copy_outputs(Params &P, const pve_outputs *out)
{
    if (!out) return;
    P.out.obs_post = out->obs_post; P.out.obs_pre = out->obs_pre; P.out.state_pre = out->state_pre;
    P.out.obs_prev_post = out->obs_prev_post; P.out.reward = out->reward; P.out.flags = out->flags;
    P.out.lanej = out->lanej; P.out.nbr = out->nbr; P.out.new_slot = out->new_slot;
    P.out.env_out = out->env_out;
}

// Item schedule of a persistent call of K ticks with items of at most T ticks -> R.n_ticks / n_full / n_taper / taper.
// The call ENDS with a geometric taper -- items of 4, 7, 12, 20 .. ticks (x 1.65 backwards while they stay below T) -- and the
// ticks in front of it are dealt into the fewest equal items of at most T ticks.  A workgroup's last item is what it is still
// busy with when the queue runs empty, so the items shrink towards the end of the call and the chip drains evenly; items of
// ONE tick are a loss (an item's load and flush are only hidden behind several ticks of compute).  Measured on MI355X,
// 4096 x 128, a 20-tick call, same process, median of 15 (tools/ab_launch_shapes.py, knob build): 11,6,3: 593 us; 12,5,3:
// 591-601; 13,5,2: 593; 9,8,3 (round 4's schedule): 600-630; 6,6,5,3: 602; 17,3: 621; 10,10: 624; 5,5,5,5: 638; 12,5,2,1: 688;
// two stream-pipelined sub-batches in launches of 5: 649-655.  Round 6, the HOME kernel (10 workgroups per CU: 2560 resident for
// 4096 intersections), median of 21: 9,7,4: 564 us; 10,6,4: 568; 8,8,4: 570; 6,6,5,3: 572; 8,7,5: 571; 7,7,6: 576; 13,7: 576; 11,6,3
// (the halving taper of round 5): 577; 12,8: 580; 15,5: 587; 16,4: 594 -- the gentler taper is what the schedule below produces.
static void item_schedule(int K, int T, RolloutArgs &R)
{
    int tail[8], n_tail = 0, body = K;
    if (K >= 8) {
        int rev[8], n_rev = 0, left = K;
        for (int sz = 4; sz < T && n_rev < 4 && left - sz >= sz; sz = (sz * 33 + 19) / 20) { rev[n_rev++] = sz; left -= sz; }   // (4, 7, 12, 20; what stays in front is at least as long)
        for (int k = 0; k < n_rev; k++) tail[k] = rev[n_rev - 1 - k];              // (largest first)
        n_tail = n_rev;
        if (const char *tv = PVE_KNOB("PVE_TAPER_TAIL")) {                       // A/B knob: "3,2", "" = none
            int cand[8], n_cand = 0;
            bool ok = true;
            for (const char *q = tv; *q && n_cand < 6; ) { cand[n_cand++] = atoi(q); while (*q && *q != ',') q++; if (*q) q++; }
            for (int k = 0; k < n_cand; k++) ok = ok && cand[k] >= 1 && cand[k] <= 255;   // (a 0-tick item would flush an unstaged LDS block)
            if (ok) { n_tail = n_cand; for (int k = 0; k < n_cand; k++) tail[k] = cand[k]; }
        }
        body = K;
        for (int k = 0; k < n_tail; k++) body -= tail[k];
        if (body < 1) { n_tail = 0; body = K; }
    }
    const int n_body = (body + T - 1) / T, base = body / n_body, rem = body - base * n_body;
    // (items of base + 1 ticks first, then of base ticks: as a full-item count + taper list the kernel needs equal full
    //  items, so the remainder goes into the taper when it fits, else the full items are T long and the remainder is folded
    //  with one of them into two near-equal items -- never an item of one or two ticks of its own)
    R.n_ticks = rem ? base + 1 : base;
    R.n_full = rem ? rem : n_body;
    int n_taper = 0;
    if (rem) {
        if (n_body - rem + n_tail > 8) {           // too many shorter items for the list: items of T ticks instead
            R.n_ticks = T; R.n_full = body / T;
            const int r = body % T;
            if (r && 2 * r < T && R.n_full > 1 && n_tail + 2 <= 8) {
                R.n_full -= 1;
                R.taper[n_taper++] = (uint8_t)((T + r + 1) / 2); R.taper[n_taper++] = (uint8_t)((T + r) / 2);
            } else if (r) R.taper[n_taper++] = (uint8_t)r;
        } else for (int k = 0; k < n_body - rem; k++) R.taper[n_taper++] = (uint8_t)base;
    }
    for (int k = 0; k < n_tail; k++) R.taper[n_taper++] = (uint8_t)tail[k];
    R.n_taper = n_taper;
}

// 256 slots exist for the 12-lane fast path only (k_tick<256> / k_rollout<256, ..>), and only in a backend that says so; the
// 4- / 8-lane layouts and the general path stop at 128.
static bool capacity_known(int capacity)
{
    return capacity == 64 || capacity == 128 || (capacity == 256 && Opt::max_capacity >= 256);
}

// An optional group the backend does not provide (pve::Provides<Opt>): its entry points validate their arguments first
static int no_kernels(const char *who, const char *what)
{
    return fail(PVE_ERR_INVALID, std::string(who) + ": this backend has no " + what + " kernels");
}

// the handle's noise for a launch whose first action is applied at the handle's current tick
static ActionNoise noise_now(pve_handle h)
{
    ActionNoise nz = h->noise;
    nz.tick0 = (uint32_t)(unsigned long long)h->ticks_since_reset;
    return nz;
}
// pve_step_many's launch of a chunk or of the whole call, with the handle's noise where the backend draws it (read by the actor
// variants only; ticks_since_reset moves with every chunk).  A template only so that `if constexpr` discards the branch a backend
// cannot compile: the HIP backend has the noisy launchers and no launch_rollout / launch_rollout_geo, the emulators the reverse.
template <class B = Opt> static int launch_rollout(pve_handle h, const Params &P, const RolloutArgs &R, std::string &err)
{
    if constexpr (Provides<B>::noise) {
        const ActionNoise nz = noise_now(h);
        return h->geo ? B::launch_rollout_geo_noisy(h->g, P, R, nz, h->cap, h->stream, err)
                      : B::launch_rollout_noisy(h->c, P, R, nz, h->cap, h->stream, err);
    } else
        return h->geo ? B::launch_rollout_geo(h->g, P, R, h->cap, h->stream, err) : B::launch_rollout(h->c, P, R, h->cap, h->stream, err);
}

extern "C" {

int pve_abi_version(void) { return PVE_ABI_VERSION; }
const char *pve_last_error(void) { return last_error_ref().c_str(); }

void pve_default_config(pve_config *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->deltaT = 0.1; cfg->vm = 5; cfg->vM = 13; cfg->am = -3; cfg->aM = 3; cfg->v0 = 10;
    cfg->lane_cw = 2.5; cfg->dis_ctl = 150; cfg->collision_thr = 2; cfg->lane_num = 12;
}

size_t pve_workspace_bytes(int n_envs, int capacity)
{
    if (n_envs <= 0 || !capacity_known(capacity)) return 0;
    return make_layout(n_envs, capacity).total;
}

int pve_create(const pve_config *cfg, int n_envs, int capacity, int device_id, void *workspace,
               void *stream, pve_handle *out)
{
    if (!cfg || !out) return fail(PVE_ERR_INVALID, "pve_create: null argument");
    if (cfg->lane_num != 12 && cfg->lane_num != 8 && cfg->lane_num != 4)
        return fail(PVE_ERR_INVALID, "pve_create: lane_num must be 12, 8 or 4 (the 3-lane branch is broken upstream)");
    if (n_envs <= 0) return fail(PVE_ERR_INVALID, "pve_create: n_envs must be > 0");
    if (!capacity_known(capacity))
        return fail(PVE_ERR_INVALID, Opt::max_capacity >= 256 ? "pve_create: capacity must be 64, 128 or 256"
                                                              : "pve_create: capacity must be 64 or 128");
    if (capacity == 256 && (cfg->lane_num != 12 || (cfg->flags & PVE_CFG_GENERAL_PATH)))
        return fail(PVE_ERR_INVALID, "pve_create: capacity 256 needs lane_num 12 on the fast path (not the 4- / 8-lane layouts, "
                                     "not PVE_CFG_GENERAL_PATH)");
    if (!(cfg->deltaT > 0) || !(cfg->am < 0) || !(cfg->aM > 0) || !(cfg->vM >= cfg->vm))
        return fail(PVE_ERR_INVALID, "pve_create: inconsistent limits (deltaT>0, am<0<aM, vM>=vm required)");
    if (!(fabs(cfg->am) >= 1e-6 && fabs(cfg->am) <= 1e6))
        return fail(PVE_ERR_INVALID, "pve_create: |am| must lie in [1e-6, 1e6] (the brake test divides by it through its reciprocal)");
    std::string err;
    if (Backend::set_device(device_id, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_create: " + err);
    DevScope dev_scope(device_id);                 // (set_device validated it; the caller's current device is restored)
    pve_handle h = new (std::nothrow) pve_handle_s();
    if (!h) return fail(PVE_ERR_NOMEM, "pve_create: out of host memory");
    h->cfg = *cfg;
    h->c = make_const(*cfg);
    h->g = make_geo_const(*cfg);
    h->lane_num = cfg->lane_num;
    h->geo = (cfg->lane_num != 12) || (cfg->flags & PVE_CFG_GENERAL_PATH);
    h->choice = nullptr; h->choice_stride = 0; h->choice_rows = 0;
    h->n_envs = n_envs; h->cap = capacity; h->device = device_id;
    h->L = make_layout(n_envs, capacity);
    h->own_ws = (workspace == nullptr);
    h->ws = (char *)workspace;
    if (h->own_ws) {
        h->ws = (char *)Backend::dmalloc(h->L.total);
        if (!h->ws) { delete h; return fail(PVE_ERR_NOMEM, "pve_create: device allocation failed"); }
    }
    h->arrivals = nullptr; h->rows = 0; h->arr_stride = 0;
    h->stream = stream;
    h->has_arrivals = false; h->is_reset = false; h->ticks_since_reset = 0;
    h->phase_cycles = nullptr;
    h->has_actor = false;
    h->has_tactor = false; h->has_critic = false;
    h->q_done_base = 0;
    h->last_launch_kind = PVE_LAUNCH_NONE;
    memset(&h->last_variant, 0, sizeof(h->last_variant));
    h->stop_phase = -1;
    memset(&h->noise, 0, sizeof(h->noise));
    *out = h;
    return PVE_OK;
}

int pve_destroy(pve_handle h)
{
    if (!h) return PVE_OK;
    DevScope dev_scope(h->device);
    if (h->own_ws && h->ws) Backend::dfree(h->ws);
    delete h;
    return PVE_OK;
}

int pve_set_stream(pve_handle h, void *stream)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_set_stream: null handle");
    h->stream = stream;
    return PVE_OK;
}

int pve_set_arrivals(pve_handle h, const double *arrivals, int rows, int env_stride_rows)
{
    if (!h || !arrivals) return fail(PVE_ERR_INVALID, "pve_set_arrivals: null argument");
    if (rows <= 0) return fail(PVE_ERR_INVALID, "pve_set_arrivals: rows must be > 0");
    if (env_stride_rows != 0 && env_stride_rows < rows)
        return fail(PVE_ERR_INVALID, "pve_set_arrivals: env_stride_rows must be 0 (shared) or >= rows");
    h->arrivals = arrivals; h->rows = rows; h->arr_stride = (long long)env_stride_rows * h->lane_num;
    h->has_arrivals = true; h->is_reset = false;
    return PVE_OK;
}

int pve_set_intentions(pve_handle h, const int32_t *choice, int rows, int env_stride_rows)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_set_intentions: null handle");
    if (h->lane_num != 8) return fail(PVE_ERR_INVALID, "pve_set_intentions: only lane_num = 8 draws intentions (ref :389-390)");
    if (choice && rows <= 0) return fail(PVE_ERR_INVALID, "pve_set_intentions: rows must be > 0");
    if (choice && env_stride_rows != 0 && env_stride_rows < rows)
        return fail(PVE_ERR_INVALID, "pve_set_intentions: env_stride_rows must be 0 (shared) or >= rows");
    h->choice = choice; h->choice_rows = choice ? rows : 0;
    h->choice_stride = (long long)env_stride_rows * h->lane_num;
    h->is_reset = false;
    return PVE_OK;
}

int pve_reset(pve_handle h)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_reset: null handle");
    if (!h->has_arrivals) return fail(PVE_ERR_STATE, "pve_reset: call pve_set_arrivals first");
    if (h->choice && h->choice_rows < h->rows)
        return fail(PVE_ERR_INVALID, "pve_reset: the intention stream has fewer rows than the arrival stream");
    DevScope dev_scope(h->device);
    Params P = base_params(h);
    std::string err;
    const int rc = h->geo ? Backend::launch_reset_geo(h->g, P, h->cap, h->stream, err)
                          : Backend::launch_reset(h->c, P, h->cap, h->stream, err);
    if (rc != 0) return fail(PVE_ERR_NO_DEVICE, "pve_reset: " + err);
    // the persistent roll-out's queue words and per-intersection item counts start from zero
    if (queue_reset(h) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_reset: clearing the roll-out queue failed");
    h->is_reset = true; h->ticks_since_reset = 0;
    return PVE_OK;
}

// bit 0: float32 observation rows; bit 1: exact float32 actor (PVE_CFG_ACTOR_F32)
static int actor_mode(pve_handle h)
{
    return ((h->cfg.flags & PVE_CFG_OBS_F32) ? 1 : 0) | ((h->cfg.flags & PVE_CFG_ACTOR_F32) ? 2 : 0);
}

static int tick_params(pve_handle h, const double *actions, const pve_outputs *out, int mode, const char *who, Params &P)
{
    if (!h) return fail(PVE_ERR_INVALID, std::string(who) + ": null handle");
    if (!h->is_reset) return fail(PVE_ERR_STATE, std::string(who) + ": call pve_set_arrivals + pve_reset first");
    P = base_params(h);
    P.actions = actions;
    P.mode = mode;
    P.mask_uncontrolled = (mode == MODE_FUSED) ? 1 : 0;
    copy_outputs(P, out);
    if (P.out.state_pre && (!P.out.obs_pre || !P.out.obs_prev_post))
        return fail(PVE_ERR_INVALID, std::string(who) + ": state_pre needs obs_pre and obs_prev_post");
    if (P.out.obs_prev_post && P.out.obs_prev_post == P.out.obs_post)
        return fail(PVE_ERR_INVALID, std::string(who) + ": obs_prev_post must not alias obs_post (ping-pong them)");
    return PVE_OK;
}

// pve_debug_last_variant: a stepping call clears the thread's launch note and the handle's record in front of its launches and
// copies the note -- what the backend wrote where it launched -- into the handle behind every launch that succeeded
static void clear_variant(pve_handle h)
{
    memset(&launch_note(), 0, sizeof(pve_launch_variant));
    memset(&h->last_variant, 0, sizeof(h->last_variant));
}
static void commit_variant(pve_handle h)
{
    h->last_variant = launch_note();
    h->last_variant.kind = h->last_launch_kind;
}

static int launch_one_tick(pve_handle h, const Params &P, const char *who)
{
    DevScope dev_scope(h->device);
    std::string err;
    const int rc = h->geo ? Backend::launch_tick_geo(h->g, P, h->cap, h->stream, err)
                          : Backend::launch_tick(h->c, P, h->cap, h->stream, err);
    if (rc != 0) return fail(PVE_ERR_NO_DEVICE, std::string(who) + ": " + err);
    h->ticks_since_reset += 1;
    h->last_launch_kind = PVE_LAUNCH_TICK;
    commit_variant(h);
    return PVE_OK;
}

static int run_tick(pve_handle h, const double *actions, const pve_outputs *out, int mode, const char *who, int launches_before = 0)
{
    Params P;
    const int rc = tick_params(h, actions, out, mode, who, P);
    if (rc != PVE_OK) return rc;
    h->last_launch_kind = PVE_LAUNCH_NONE;
    clear_variant(h);
    launch_note().launches = launches_before;       // (pve_step_all_actor: the actor pass in front of the tick)
    return launch_one_tick(h, P, who);
}

// trajectory roll-outs: the per-tick block of every output buffer
static void shift_outputs(Outputs &o, const Outputs &o0, long long k, long long n_envs, long long cap, bool obs_f32)
{
    const long long s = k * n_envs * cap;
    o = o0;
    if (o0.obs_post) o.obs_post = obs_f32 ? (double *)((float *)o0.obs_post + s * OBSW) : o0.obs_post + s * OBSW;
    if (o0.obs_pre) o.obs_pre = obs_f32 ? (double *)((float *)o0.obs_pre + s * OBSW) : o0.obs_pre + s * OBSW;
    if (o0.state_pre) o.state_pre = obs_f32 ? (double *)((float *)o0.state_pre + s * OBSW * (NNB + 1)) : o0.state_pre + s * OBSW * (NNB + 1);
    if (o0.reward) o.reward = o0.reward + s;
    if (o0.flags) o.flags = o0.flags + s;
    if (o0.lanej) o.lanej = o0.lanej + s;
    if (o0.nbr) o.nbr = o0.nbr + s * NNB;
    if (o0.new_slot) o.new_slot = o0.new_slot + s;
    if (o0.env_out) o.env_out = o0.env_out + k * n_envs * 8;
}

int pve_step_all(pve_handle h, const double *actions, const pve_outputs *out)
{
    return run_tick(h, actions, out, MODE_FUSED, "pve_step_all");
}

int pve_scene_update(pve_handle h, const double *actions, const pve_outputs *out)
{
    return run_tick(h, actions, out, MODE_SCENE, "pve_scene_update");
}

static float *actor_flat(pve_handle h) { return (float *)(h->ws + h->L.off_actor_flat); }
static unsigned char *actor_packed(pve_handle h) { return (unsigned char *)(h->ws + h->L.off_actor_packed); }

// the stand-alone actor pass obs -> actions, with the handle's noise
static int run_actor(pve_handle h, const void *obs, double *actions, std::string &err)
{
    const int32_t *meta = (const int32_t *)(h->ws + h->L.off_i32[I_META]), *ids = (const int32_t *)(h->ws + h->L.off_i32[I_ID]);
    if (h->noise.sigma == 0)                       // (always, on a backend without the noisy kernels: pve_set_action_noise)
        return Backend::launch_actor(actor_flat(h), actor_packed(h), obs, actor_mode(h), meta, actions, h->n_envs, h->cap, h->stream, err);
    return Opt::launch_actor_noisy(actor_flat(h), actor_packed(h), obs, actor_mode(h), meta, ids, noise_now(h), actions, h->n_envs,
                                   h->cap, h->stream, err);
}

int pve_set_actor(pve_handle h, const float *weights)
{
    if (!h || !weights) return fail(PVE_ERR_INVALID, "pve_set_actor: null argument");
    DevScope dev_scope(h->device);
    std::string err;
    if (Backend::pack_actor(weights, actor_flat(h), actor_packed(h), h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_set_actor: " + err);
    h->has_actor = true;
    return PVE_OK;
}

// weights != NULL: install them first (pve_set_actor); NULL: the actor installed earlier
static int use_actor(pve_handle h, const float *weights, const char *who)
{
    if (weights) return pve_set_actor(h, weights);
    if (!h->has_actor) return fail(PVE_ERR_STATE, std::string(who) + ": no actor installed (pve_set_actor, or pass the weights)");
    return PVE_OK;
}

int pve_actor_forward(pve_handle h, const float *weights, const void *obs, double *actions)
{
    if (!h || !obs || !actions) return fail(PVE_ERR_INVALID, "pve_actor_forward: null argument");
    if (!h->is_reset) return fail(PVE_ERR_STATE, "pve_actor_forward: call pve_set_arrivals + pve_reset first");
    const int rc = use_actor(h, weights, "pve_actor_forward");
    if (rc != PVE_OK) return rc;
    DevScope dev_scope(h->device);
    std::string err;
    if (run_actor(h, obs, actions, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_actor_forward: " + err);
    return PVE_OK;
}

int pve_set_target_networks(pve_handle h, const float *target_actor, const float *critic)
{
    if (!h || (!target_actor && !critic)) return fail(PVE_ERR_INVALID, "pve_set_target_networks: null argument (at least one network is needed)");
    if (!Provides<Opt>::target_q) return no_kernels("pve_set_target_networks", "critic / bootstrap");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::pack_target_networks(target_actor, (float *)(h->ws + h->L.off_tactor_flat), (unsigned char *)(h->ws + h->L.off_tactor_packed),
                                  critic, (float *)(h->ws + h->L.off_critic_flat), (unsigned char *)(h->ws + h->L.off_critic_packed),
                                  h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_set_target_networks: " + err);
    if (target_actor) h->has_tactor = true;
    if (critic) h->has_critic = true;
    return PVE_OK;
}

int pve_critic_forward(pve_handle h, const void *rows, const float *act7, float *q, int64_t n)
{
    if (!h || !rows || !act7 || !q) return fail(PVE_ERR_INVALID, "pve_critic_forward: null argument");
    if (n <= 0) return fail(PVE_ERR_INVALID, "pve_critic_forward: n must be > 0");
    if (!Provides<Opt>::target_q) return no_kernels("pve_critic_forward", "critic / bootstrap");
    if (!h->has_critic) return fail(PVE_ERR_STATE, "pve_critic_forward: no critic installed (pve_set_target_networks)");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_critic((const unsigned char *)(h->ws + h->L.off_critic_packed), rows, actor_mode(h) & 1, act7, q, (long long)n,
                           h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_critic_forward: " + err);
    return PVE_OK;
}

int pve_bootstrap_q(pve_handle h, const void *state, const int32_t *flags, float *q, float *act7_out, int64_t n)
{
    if (!h || !state || !q) return fail(PVE_ERR_INVALID, "pve_bootstrap_q: null argument");
    if (n <= 0) return fail(PVE_ERR_INVALID, "pve_bootstrap_q: n must be > 0");
    if (!Provides<Opt>::target_q) return no_kernels("pve_bootstrap_q", "critic / bootstrap");
    if (!h->has_tactor || !h->has_critic)
        return fail(PVE_ERR_STATE, "pve_bootstrap_q: needs a target actor and a critic (pve_set_target_networks)");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_bootstrap_q((const unsigned char *)(h->ws + h->L.off_tactor_packed),
                                (const unsigned char *)(h->ws + h->L.off_critic_packed), state, actor_mode(h) & 1, flags, q, act7_out,
                                (long long)n, h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_bootstrap_q: " + err);
    return PVE_OK;
}

// pve_nstep -> NstepArgs, with every check the two entry points share
static int nstep_args(pve_handle h, const pve_nstep *ns, bool gather, const char *who, NstepArgs &A)
{
    const std::string w(who);
    if (!h || !ns) return fail(PVE_ERR_INVALID, w + ": null argument");
    if (ns->window < 1 || ns->window > PVE_NSTEP_MAX_WINDOW) return fail(PVE_ERR_INVALID, w + ": window must be 1 .. 16");
    if (!(ns->gamma >= 0.0 && ns->gamma <= 1.0)) return fail(PVE_ERR_INVALID, w + ": gamma must lie in [0, 1]");
    if (ns->cur.n_ticks < 1) return fail(PVE_ERR_INVALID, w + ": cur.n_ticks must be > 0");
    if (ns->prev.n_ticks < 0 || (ns->prev.n_ticks > 0 && ns->prev.n_ticks < ns->window))
        return fail(PVE_ERR_INVALID, w + ": prev.n_ticks must be 0 or at least window");
    const pve_nstep_segment *segs[2] = {&ns->cur, &ns->prev};
    for (int k = 0; k < (ns->prev.n_ticks > 0 ? 2 : 1); k++)
        if (!segs[k]->obs_post || !segs[k]->state_pre || !segs[k]->reward || !segs[k]->flags || !segs[k]->new_slot)
            return fail(PVE_ERR_INVALID, w + ": a segment needs obs_post, state_pre, reward, flags and new_slot");
    if (ns->prev.n_ticks == 0 && !ns->obs_first) return fail(PVE_ERR_INVALID, w + ": obs_first is needed when there is no prev segment");
    if (!ns->q_boot || !ns->target || !ns->code || !ns->offsets || !ns->total)
        return fail(PVE_ERR_INVALID, w + ": q_boot, target, code, offsets and total are needed");
    if (gather && (ns->max_records < 0 || (ns->max_records > 0 && (!ns->records || !ns->index))))
        return fail(PVE_ERR_INVALID, w + ": max_records must be >= 0, with records and index");
    if (ns->block_threads < 0 || ns->block_threads > 1024 || ns->block_threads % 64)
        return fail(PVE_ERR_INVALID, w + ": block_threads must be 0 or a multiple of 64 up to 1024");
    const uintptr_t align = (uintptr_t)ns->cur.obs_post | (uintptr_t)ns->cur.state_pre | (uintptr_t)ns->prev.obs_post | (uintptr_t)ns->prev.state_pre |
                            (uintptr_t)ns->obs_first | (gather ? (uintptr_t)ns->records | (uintptr_t)ns->index : 0);
    if (align & 15) return fail(PVE_ERR_INVALID, w + ": obs_post, state_pre, obs_first, records and index must be 16-byte aligned");
    memset(&A, 0, sizeof(A));
    A.gamma = ns->gamma; A.window = ns->window; A.mode = ns->mode; A.n_envs = h->n_envs; A.cap = h->cap;
    A.obs_f32 = (h->cfg.flags & PVE_CFG_OBS_F32) ? 1 : 0;
    A.n_back = ns->prev.n_ticks < ns->window - 1 ? ns->prev.n_ticks : ns->window - 1;
    if ((long long)(A.n_back + ns->cur.n_ticks) * h->n_envs * h->cap > 0x7fffffffLL)
        return fail(PVE_ERR_INVALID, w + ": more than 2^31 - 1 candidate slots in one call (cut the trajectory)");
    for (int k = 0; k < 2; k++) {
        NstepSeg &S = k ? A.prev : A.cur;
        S.n_ticks = segs[k]->n_ticks; S.obs_post = segs[k]->obs_post; S.state_pre = segs[k]->state_pre; S.reward = segs[k]->reward;
        S.flags = segs[k]->flags; S.new_slot = segs[k]->new_slot;
    }
    A.obs_first = ns->obs_first; A.q_boot = ns->q_boot; A.target = ns->target; A.code = ns->code; A.offsets = ns->offsets;
    A.total = (long long *)ns->total; A.max_records = ns->max_records; A.records = ns->records; A.index = ns->index;
    if (!Provides<Opt>::nstep) return no_kernels(who, "n-step");
    return PVE_OK;
}

int pve_nstep_scan(pve_handle h, const pve_nstep *ns)
{
    NstepArgs A;
    const int rc = nstep_args(h, ns, false, "pve_nstep_scan", A);
    if (rc != PVE_OK) return rc;
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_nstep_scan(A, ns->block_threads, h->stream, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_nstep_scan: " + err);
    return PVE_OK;
}

int pve_nstep_gather(pve_handle h, const pve_nstep *ns)
{
    NstepArgs A;
    const int rc = nstep_args(h, ns, true, "pve_nstep_gather", A);
    if (rc != PVE_OK) return rc;
    if (A.max_records == 0) return PVE_OK;
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_nstep_gather(A, h->stream, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_nstep_gather: " + err);
    return PVE_OK;
}

// pve_replay -> ReplayArgs, with the checks the three entry points share
static int replay_args(pve_handle h, const pve_replay *rp, const char *who, ReplayArgs &A)
{
    const std::string w(who);
    if (!h || !rp) return fail(PVE_ERR_INVALID, w + ": null argument");
    if (!rp->store || !rp->state) return fail(PVE_ERR_INVALID, w + ": null store or state");
    if (rp->capacity < 1 || rp->capacity > 0x7fffffffLL) return fail(PVE_ERR_INVALID, w + ": capacity must be 1 .. 2^31 - 1");
    if (rp->block_threads < 0 || rp->block_threads > 1024 || rp->block_threads % 64)
        return fail(PVE_ERR_INVALID, w + ": block_threads must be 0 or a multiple of 64 up to 1024");
    if (((uintptr_t)rp->store & 15) || ((uintptr_t)rp->state & 7))
        return fail(PVE_ERR_INVALID, w + ": store must be 16-byte aligned, state 8-byte aligned");
    A.capacity = rp->capacity; A.store = rp->store; A.state = (long long *)rp->state; A.seed = rp->seed;
    return PVE_OK;
}

int pve_replay_reset(pve_handle h, const pve_replay *rp)
{
    ReplayArgs A;
    const int rc = replay_args(h, rp, "pve_replay_reset", A);
    if (rc != PVE_OK) return rc;
    if (!Provides<Opt>::replay) return no_kernels("pve_replay_reset", "replay");
    DevScope dev_scope(h->device);
    if (Backend::memset0(A.state, sizeof(long long) * REPLAY_STATE_WORDS, h->stream) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_replay_reset: device memset failed");
    return PVE_OK;
}

int pve_replay_append(pve_handle h, const pve_replay *rp, const float *records, const int64_t *total_dev, int64_t n_max)
{
    ReplayArgs A;
    const int rc = replay_args(h, rp, "pve_replay_append", A);
    if (rc != PVE_OK) return rc;
    if (n_max < 0) return fail(PVE_ERR_INVALID, "pve_replay_append: n_max must be >= 0");
    if (n_max > 0 && !records) return fail(PVE_ERR_INVALID, "pve_replay_append: null records");
    if (((uintptr_t)records & 15) || ((uintptr_t)total_dev & 7))
        return fail(PVE_ERR_INVALID, "pve_replay_append: records must be 16-byte aligned, total_dev 8-byte aligned");
    if (!Provides<Opt>::replay) return no_kernels("pve_replay_append", "replay");
    if (n_max == 0) return PVE_OK;
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_replay_append(A, records, (const long long *)total_dev, (long long)n_max, rp->block_threads, h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_replay_append: " + err);
    return PVE_OK;
}

int pve_replay_sample(pve_handle h, const pve_replay *rp, int64_t batch, int64_t n_batches, float *rows, float *act7, float *target,
                      int64_t *seq)
{
    ReplayArgs A;
    const int rc = replay_args(h, rp, "pve_replay_sample", A);
    if (rc != PVE_OK) return rc;
    if (batch < 1 || batch > rp->capacity) return fail(PVE_ERR_INVALID, "pve_replay_sample: batch must be 1 .. capacity");
    if (n_batches < 1 || n_batches > 0x7fffffffLL / batch)
        return fail(PVE_ERR_INVALID, "pve_replay_sample: n_batches must be >= 1 and batch * n_batches <= 2^31 - 1");
    if (!rows || !act7 || !target || !seq) return fail(PVE_ERR_INVALID, "pve_replay_sample: null output");
    if (((uintptr_t)rows & 15) || ((uintptr_t)act7 & 15) || ((uintptr_t)target & 3) || ((uintptr_t)seq & 7))
        return fail(PVE_ERR_INVALID, "pve_replay_sample: rows and act7 must be 16-byte aligned, seq 8-byte, target 4-byte aligned");
    if (!Provides<Opt>::replay) return no_kernels("pve_replay_sample", "replay");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_replay_sample(A, (long long)batch, (long long)n_batches, rows, act7, target, (long long *)seq, rp->block_threads,
                                  h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_replay_sample: " + err);
    return PVE_OK;
}

// pve_prio -> PrioArgs, with the checks the four entry points share
static int prio_args(pve_handle h, const pve_prio *pp, const char *who, PrioArgs &A)
{
    const std::string w(who);
    if (!h || !pp) return fail(PVE_ERR_INVALID, w + ": null argument");
    const int rc = replay_args(h, &pp->replay, who, A.R);
    if (rc != PVE_OK) return rc;
    if (!pp->prio || !pp->pseq || !pp->order || !pp->pstate || !pp->scratch || !pp->ends || !pp->ends_host || !pp->part_from)
        return fail(PVE_ERR_INVALID, w + ": null prio, pseq, order, pstate, scratch, ends, ends_host or part_from");
    if (((uintptr_t)pp->prio & 3) || ((uintptr_t)pp->order & 3) || ((uintptr_t)pp->ends & 3) || ((uintptr_t)pp->pseq & 7) ||
        ((uintptr_t)pp->pstate & 7) || ((uintptr_t)pp->scratch & 15))
        return fail(PVE_ERR_INVALID, w + ": scratch must be 16-byte aligned, pseq and pstate 8-byte, prio, order and ends 4-byte aligned");
    if (pp->scratch_bytes < 0 || (uint64_t)pp->scratch_bytes < (uint64_t)prio_scratch_bytes(A.R.capacity))
        return fail(PVE_ERR_INVALID, w + ": scratch_bytes is below pve_prio_scratch_bytes(capacity)");
    if (pp->batch < 1 || pp->batch > A.R.capacity) return fail(PVE_ERR_INVALID, w + ": batch must be 1 .. capacity");
    for (int k = 0; k < PRIO_PARTS; k++) {
        if (pp->part_from[k] < 1 || (k > 0 && pp->part_from[k] < pp->part_from[k - 1]))
            return fail(PVE_ERR_INVALID, w + ": part_from must be >= 1 and non-decreasing");
        const int32_t *row = pp->ends_host + (size_t)k * (size_t)(pp->batch + 1);
        if (row[0] != 0) return fail(PVE_ERR_INVALID, w + ": every row of ends must start at 0");
        for (int64_t j = 1; j <= pp->batch; j++)
            if (row[j] < row[j - 1] || row[j] > A.R.capacity)
                return fail(PVE_ERR_INVALID, w + ": every row of ends must be non-decreasing within 0 .. capacity");
        A.part_from[k] = pp->part_from[k];
    }
    A.prio = pp->prio; A.pseq = (long long *)pp->pseq; A.order = pp->order; A.pstate = (long long *)pp->pstate;
    A.ends = pp->ends; A.batch = pp->batch;
    prio_carve_scratch(A, pp->scratch);
    return PVE_OK;
}

size_t pve_prio_scratch_bytes(int64_t capacity)
{
    return capacity < 1 || capacity > 0x7fffffffLL ? 0 : prio_scratch_bytes(capacity);
}

int pve_prio_reset(pve_handle h, const pve_prio *pp)
{
    PrioArgs A;
    const int rc = prio_args(h, pp, "pve_prio_reset", A);
    if (rc != PVE_OK) return rc;
    if (!Provides<Opt>::prio) return no_kernels("pve_prio_reset", "prioritised replay");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_prio_reset(A, pp->replay.block_threads, h->stream, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_prio_reset: " + err);
    return PVE_OK;
}

int pve_prio_rank(pve_handle h, const pve_prio *pp)
{
    PrioArgs A;
    const int rc = prio_args(h, pp, "pve_prio_rank", A);
    if (rc != PVE_OK) return rc;
    if (!Provides<Opt>::prio) return no_kernels("pve_prio_rank", "prioritised replay");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_prio_rank(A, pp->replay.block_threads, h->stream, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_prio_rank: " + err);
    return PVE_OK;
}

int pve_prio_sample(pve_handle h, const pve_prio *pp, int64_t n_batches, int64_t min_live, float alpha_beta, float *rows, float *act7,
                    float *target, int64_t *seq, int32_t *rank, float *weight)
{
    PrioArgs A;
    const int rc = prio_args(h, pp, "pve_prio_sample", A);
    if (rc != PVE_OK) return rc;
    if (n_batches < 1 || n_batches > 0x7fffffffLL / pp->batch)
        return fail(PVE_ERR_INVALID, "pve_prio_sample: n_batches must be >= 1 and batch * n_batches <= 2^31 - 1");
    if (min_live < 0) return fail(PVE_ERR_INVALID, "pve_prio_sample: min_live must be >= 0");
    if (!(alpha_beta >= 0.f && alpha_beta <= 3.4028234663852886e38f))
        return fail(PVE_ERR_INVALID, "pve_prio_sample: alpha_beta must be finite and >= 0");
    if (!rows || !act7 || !target || !seq || !rank || !weight) return fail(PVE_ERR_INVALID, "pve_prio_sample: null output");
    if (((uintptr_t)rows & 15) || ((uintptr_t)act7 & 15) || ((uintptr_t)target & 3) || ((uintptr_t)seq & 7) || ((uintptr_t)rank & 3) ||
        ((uintptr_t)weight & 3))
        return fail(PVE_ERR_INVALID, "pve_prio_sample: rows and act7 must be 16-byte aligned, seq 8-byte, target, rank and weight 4-byte aligned");
    if (!Provides<Opt>::prio) return no_kernels("pve_prio_sample", "prioritised replay");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_prio_sample(A, (long long)n_batches, (long long)min_live, alpha_beta, rows, act7, target, (long long *)seq, rank,
                                weight, pp->replay.block_threads, h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_prio_sample: " + err);
    return PVE_OK;
}

int pve_prio_update(pve_handle h, const pve_prio *pp, const int64_t *seq, const float *q, const float *target, int64_t n)
{
    PrioArgs A;
    const int rc = prio_args(h, pp, "pve_prio_update", A);
    if (rc != PVE_OK) return rc;
    if (n < 0) return fail(PVE_ERR_INVALID, "pve_prio_update: n must be >= 0");
    if (n > 0 && (!seq || !q)) return fail(PVE_ERR_INVALID, "pve_prio_update: null seq or q");
    if (((uintptr_t)seq & 7) || ((uintptr_t)q & 3) || ((uintptr_t)target & 3))
        return fail(PVE_ERR_INVALID, "pve_prio_update: seq must be 8-byte aligned, q and target 4-byte aligned");
    if (!Provides<Opt>::prio) return no_kernels("pve_prio_update", "prioritised replay");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_prio_update(A, (const long long *)seq, q, target, (long long)n, pp->replay.block_threads, h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_prio_update: " + err);
    return PVE_OK;
}

// pve_learner -> LearnHyper, with the checks the two entry points share
static int learner_args(pve_handle h, const pve_learner *lrn, const char *who, LearnHyper &H)
{
    const std::string w(who);
    if (!h || !lrn) return fail(PVE_ERR_INVALID, w + ": null argument");
    if (!lrn->params) return fail(PVE_ERR_INVALID, w + ": null params");
    if ((uintptr_t)lrn->params & 15) return fail(PVE_ERR_INVALID, w + ": params must be 16-byte aligned");
    const float big = 3.4028234663852886e38f;
    const float fin[4] = {lrn->actor_lr, lrn->critic_lr, lrn->epsilon, lrn->tau};
    for (int k = 0; k < 4; k++)
        if (!(fin[k] >= -big && fin[k] <= big)) return fail(PVE_ERR_INVALID, w + ": actor_lr, critic_lr, epsilon and tau must be finite");
    if (!(lrn->tau >= 0.f && lrn->tau <= 1.f)) return fail(PVE_ERR_INVALID, w + ": tau must lie in [0, 1]");
    if (!(lrn->beta1 >= 0.f && lrn->beta1 < 1.f) || !(lrn->beta2 >= 0.f && lrn->beta2 < 1.f))
        return fail(PVE_ERR_INVALID, w + ": beta1 and beta2 must lie in [0, 1)");
    if (lrn->flags & ~PVE_LEARN_CRITIC_ONLY) return fail(PVE_ERR_INVALID, w + ": unknown flags");
    if (lrn->block_threads < 0 || lrn->block_threads > 1024 || lrn->block_threads % 64)
        return fail(PVE_ERR_INVALID, w + ": block_threads must be 0 or a multiple of 64 up to 1024");
    H.actor_lr = lrn->actor_lr; H.critic_lr = lrn->critic_lr; H.beta1 = lrn->beta1; H.beta2 = lrn->beta2; H.epsilon = lrn->epsilon;
    H.tau = lrn->tau; H.flags = lrn->flags;
    return PVE_OK;
}

int pve_learner_init(pve_handle h, const pve_learner *lrn, const float *actor, const float *critic, const float *target_actor,
                     const float *target_critic)
{
    LearnHyper H;
    const int rc = learner_args(h, lrn, "pve_learner_init", H);
    if (rc != PVE_OK) return rc;
    if (!actor || !critic) return fail(PVE_ERR_INVALID, "pve_learner_init: null actor or critic");
    if (((uintptr_t)actor | (uintptr_t)critic | (uintptr_t)target_actor | (uintptr_t)target_critic) & 15)
        return fail(PVE_ERR_INVALID, "pve_learner_init: the networks must be 16-byte aligned");
    if (!Provides<Opt>::learner) return no_kernels("pve_learner_init", "learner");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_learner_init(lrn->params, actor, critic, target_actor ? target_actor : actor,
                                 target_critic ? target_critic : critic, H.beta1, H.beta2, h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_learner_init: " + err);
    return PVE_OK;
}

int pve_learner_step(pve_handle h, const pve_learner *lrn, const float *rows, const float *act7, const float *target, int64_t batch,
                     int64_t n_batches, float *losses, float *grads)
{
    LearnCtx C;
    memset(&C, 0, sizeof(C));
    const int rc = learner_args(h, lrn, "pve_learner_step", C.H);
    if (rc != PVE_OK) return rc;
    if (!rows || !act7 || !target) return fail(PVE_ERR_INVALID, "pve_learner_step: null rows, act7 or target");
    if (batch < 1) return fail(PVE_ERR_INVALID, "pve_learner_step: batch must be >= 1");
    if (n_batches < 1 || n_batches > 0x7fffffffLL / batch)
        return fail(PVE_ERR_INVALID, "pve_learner_step: n_batches must be >= 1 and batch * n_batches <= 2^31 - 1");
    if (((uintptr_t)rows & 15) || (((uintptr_t)act7 | (uintptr_t)target | (uintptr_t)losses | (uintptr_t)grads) & 3))
        return fail(PVE_ERR_INVALID, "pve_learner_step: rows must be 16-byte aligned, act7, target, losses and grads 4-byte aligned");
    if (!Provides<Opt>::learner) return no_kernels("pve_learner_step", "learner");
    C.P = lrn->params; C.rows = rows; C.act7 = act7; C.target = target; C.losses = losses; C.grads = grads;
    C.batch = (int)batch; C.n_batches = (int)n_batches;
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_learner_step(C, lrn->block_threads, h->stream, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_learner_step: " + err);
    return PVE_OK;
}

int pve_learner_step_wide(pve_handle h, const pve_learner *lrn, const float *rows, const float *act7, const float *target, int64_t batch,
                          int64_t n_batches, float *work, int64_t work_floats, int32_t groups, float *losses, float *grads)
{
    LearnCtx C;
    memset(&C, 0, sizeof(C));
    const int rc = learner_args(h, lrn, "pve_learner_step_wide", C.H);
    if (rc != PVE_OK) return rc;
    if (!rows || !act7 || !target) return fail(PVE_ERR_INVALID, "pve_learner_step_wide: null rows, act7 or target");
    if (batch < 1) return fail(PVE_ERR_INVALID, "pve_learner_step_wide: batch must be >= 1");
    if (n_batches < 1 || n_batches > 0x7fffffffLL / batch)
        return fail(PVE_ERR_INVALID, "pve_learner_step_wide: n_batches must be >= 1 and batch * n_batches <= 2^31 - 1");
    if (((uintptr_t)rows & 15) || (((uintptr_t)act7 | (uintptr_t)target | (uintptr_t)losses | (uintptr_t)grads) & 3))
        return fail(PVE_ERR_INVALID, "pve_learner_step_wide: rows must be 16-byte aligned, act7, target, losses and grads 4-byte aligned");
    if (!work) return fail(PVE_ERR_INVALID, "pve_learner_step_wide: null work");
    if ((uintptr_t)work & 15) return fail(PVE_ERR_INVALID, "pve_learner_step_wide: work must be 16-byte aligned");
    if (work_floats < (int64_t)PVE_LEARNER_WIDE_FLOATS(batch))
        return fail(PVE_ERR_INVALID, "pve_learner_step_wide: work_floats must be >= PVE_LEARNER_WIDE_FLOATS(batch)");
    if (groups < 0) return fail(PVE_ERR_INVALID, "pve_learner_step_wide: groups must be >= 0");
    if (!Provides<Opt>::learner_wide) return no_kernels("pve_learner_step_wide", "learner");
    C.P = lrn->params; C.rows = rows; C.act7 = act7; C.target = target; C.losses = losses; C.grads = grads;
    C.batch = (int)batch; C.n_batches = (int)n_batches;
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_learner_step_wide(C, work, (int)groups, lrn->block_threads, h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_learner_step_wide: " + err);
    return PVE_OK;
}

// The arrival stream of an episode, generated in place (replaces the loadmat of main.py:228-229 / :388-389 and, for the 8-lane
// layout, the intention draws of ref :381, :390).  It does not install the stream: pve_set_arrivals / pve_set_intentions do.
int pve_generate_arrivals(pve_handle h, const pve_arrival_gen *g, double *arrivals, int32_t *intentions, double *covered)
{
    if (!h || !g || !arrivals) return fail(PVE_ERR_INVALID, "pve_generate_arrivals: null handle, descriptor or arrivals");
    if (g->env_offset < 0) return fail(PVE_ERR_INVALID, "pve_generate_arrivals: env_offset must be >= 0");
    if (g->rows < 2 || g->rows > ARR_MAX_ROWS) return fail(PVE_ERR_INVALID, "pve_generate_arrivals: rows must be 2 .. 2^28");
    if (!g->mean_env && (!(g->mean_s > 0) || g->mean_s > 1.7976931348623157e308))
        return fail(PVE_ERR_INVALID, "pve_generate_arrivals: mean_s must be finite and > 0");
    if (!(g->min_gap_s >= 0) || g->min_gap_s > 1.7976931348623157e308)
        return fail(PVE_ERR_INVALID, "pve_generate_arrivals: min_gap_s must be finite and >= 0");
    if (g->block_threads < 0 || g->block_threads > 1024 || g->block_threads % 64)
        return fail(PVE_ERR_INVALID, "pve_generate_arrivals: block_threads must be 0 or a multiple of 64 up to 1024");
    if (intentions && h->lane_num != 8)
        return fail(PVE_ERR_INVALID, "pve_generate_arrivals: only lane_num = 8 draws intentions (ref :389-390)");
    if (((uintptr_t)arrivals & 15) || ((uintptr_t)intentions & 15) || ((uintptr_t)covered & 7) || ((uintptr_t)g->mean_env & 7))
        return fail(PVE_ERR_INVALID, "pve_generate_arrivals: arrivals and intentions must be 16-byte aligned, covered and mean_env 8-byte");
    if (!Provides<Opt>::arrivals) return no_kernels("pve_generate_arrivals", "arrival generator");
    ArrivalArgs A;
    A.seed = g->seed; A.env_offset = (long long)g->env_offset; A.epoch = g->epoch; A.rows = g->rows; A.n_envs = h->n_envs;
    A.lane_num = h->lane_num; A.mean = g->mean_s; A.mean_env = g->mean_env; A.min_gap = g->min_gap_s; A.arrivals = arrivals;
    A.intentions = intentions; A.covered = covered;
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_generate_arrivals(A, g->block_threads, h->stream, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_generate_arrivals: " + err);
    return PVE_OK;
}

// Roll-out and evaluation statistics (include/pve_env_stats.h; the definition is csrc/pve_stats.h)

size_t pve_stats_scratch_bytes(int n_envs, int n_ticks)
{
    if (n_envs < 1 || n_ticks < 1) return 0;
    return stats_scratch_bytes(n_envs, n_ticks);
}

int pve_rollout_stats(pve_handle h, const pve_stats *d)
{
    if (!h || !d) return fail(PVE_ERR_INVALID, "pve_rollout_stats: null handle or descriptor");
    if (!d->flags || !d->reward || !d->env_out || !d->series || !d->scratch)
        return fail(PVE_ERR_INVALID, "pve_rollout_stats: null flags, reward, env_out, series or scratch");
    if (d->n_ticks < 1) return fail(PVE_ERR_INVALID, "pve_rollout_stats: n_ticks must be >= 1");
    if (d->n_groups < 1 || d->n_groups > STAT_MAX_GROUPS || (!d->group && d->n_groups != 1))
        return fail(PVE_ERR_INVALID, "pve_rollout_stats: n_groups must be 1 .. 1024, and 1 without a group map");
    if (d->block_threads < 0 || d->block_threads > 1024 || d->block_threads % 64)
        return fail(PVE_ERR_INVALID, "pve_rollout_stats: block_threads must be 0 or a multiple of 64 up to 1024");
    if (d->reserved != 0) return fail(PVE_ERR_INVALID, "pve_rollout_stats: reserved must be 0");
    const uintptr_t obs_mask = (h->cfg.flags & PVE_CFG_OBS_F32) ? 3 : 7;
    if (((uintptr_t)d->group & 3) || ((uintptr_t)d->flags & 3) || ((uintptr_t)d->env_out & 3) || ((uintptr_t)d->reward & 7) ||
        ((uintptr_t)d->obs_pre & obs_mask) || ((uintptr_t)d->series & 7) || ((uintptr_t)d->totals & 7) || ((uintptr_t)d->scratch & 7))
        return fail(PVE_ERR_INVALID, "pve_rollout_stats: every block must be aligned to its element type");
    if (h->cap % STAT_LANES) return fail(PVE_ERR_INVALID, "pve_rollout_stats: the capacity must be a multiple of 64");
    if (!Provides<Opt>::stats) return no_kernels("pve_rollout_stats", "statistics");
    StatsArgs A;
    A.n_envs = h->n_envs; A.cap = h->cap; A.n_ticks = d->n_ticks; A.n_groups = d->n_groups;
    A.obs_f32 = (h->cfg.flags & PVE_CFG_OBS_F32) ? 1 : 0;
    A.group = d->group; A.flags = d->flags; A.reward = d->reward; A.obs_pre = d->obs_pre; A.env_out = d->env_out;
    A.series = d->series; A.totals = d->totals; A.scratch = (double *)d->scratch;
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_rollout_stats(A, d->block_threads, h->stream, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_rollout_stats: " + err);
    return PVE_OK;
}

int pve_metrics_groups(pve_handle h, const int32_t *group, int n_groups, double *out)
{
    if (!h || !out) return fail(PVE_ERR_INVALID, "pve_metrics_groups: null handle or out");
    if (n_groups < 1 || n_groups > STAT_MAX_GROUPS || (!group && n_groups != 1))
        return fail(PVE_ERR_INVALID, "pve_metrics_groups: n_groups must be 1 .. 1024, and 1 without a group map");
    if (((uintptr_t)group & 3) || ((uintptr_t)out & 7))
        return fail(PVE_ERR_INVALID, "pve_metrics_groups: group must be 4-byte aligned, out 8-byte");
    if (!Provides<Opt>::stats) return no_kernels("pve_metrics_groups", "statistics");
    DevScope dev_scope(h->device);
    std::string err;
    if (Opt::launch_metrics_groups((const EnvHeader *)(h->ws + h->L.off_headers), h->n_envs, h->cap, group, n_groups, out, h->stream,
                                   err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_metrics_groups: " + err);
    return PVE_OK;
}

int pve_set_action_noise(pve_handle h, double sigma, uint64_t seed, int64_t env_offset)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_set_action_noise: null handle");
    if (!(sigma >= 0) || sigma > 1.7976931348623157e308)
        return fail(PVE_ERR_INVALID, "pve_set_action_noise: sigma must be finite and >= 0");
    if (sigma > 0 && !Provides<Opt>::noise)
        return fail(PVE_ERR_INVALID, "pve_set_action_noise: this backend has no noisy actor kernels (sigma must be 0)");
    h->noise.sigma = sigma; h->noise.seed = seed; h->noise.env_offset = env_offset;
    return PVE_OK;
}

int pve_step_all_actor(pve_handle h, const float *weights, const void *obs_in, double *actions,
                       const pve_outputs *out)
{
    if (out && out->state_pre && out->obs_post && (const void *)out->obs_post == obs_in)
        return fail(PVE_ERR_INVALID, "pve_step_all_actor: with state_pre, out->obs_post must not alias obs_in (ping-pong them)");
    int rc = pve_actor_forward(h, weights, obs_in, actions);
    if (rc != PVE_OK) return rc;
    return run_tick(h, actions, out, MODE_FUSED, "pve_step_all_actor", 1);
}

// What the queue form and the chunked form of pve_step_many hand a roll-out launch alike, for a launch that starts at tick k0 of
// the call (everything else zero): the action source, and the rows the tick in front of the launch stored
static void fill_rollout_args(pve_handle h, const pve_rollout *ro, int k0, const void *actor_obs, const void *prev_rows, RolloutArgs &R)
{
    memset(&R, 0, sizeof(R));
    R.source = ro->source; R.pool = ro->pool; R.n_pool = ro->n_pool;
    R.pool_tick0 = (ro->source == PVE_SRC_POOL || ro->source == PVE_SRC_TABLE) ? (int)(((long long)ro->pool_tick0 + k0) % ro->n_pool) : 0;
    R.table_ids = ro->table_ids;
    R.trajectory = ro->trajectory ? 1 : 0;
    R.actor_packed = actor_packed(h); R.actor_obs = actor_obs;
    R.prev_rows = prev_rows;
}

int pve_step_many(pve_handle h, const pve_rollout *ro, const pve_outputs *out)
{
    const char *who = "pve_step_many";
    if (!h || !ro) return fail(PVE_ERR_INVALID, "pve_step_many: null argument");
    if (ro->n_ticks < 0) return fail(PVE_ERR_INVALID, "pve_step_many: n_ticks must be >= 0");
    if (ro->source != PVE_SRC_ZERO && ro->source != PVE_SRC_POOL && ro->source != PVE_SRC_ACTOR && ro->source != PVE_SRC_TABLE)
        return fail(PVE_ERR_INVALID, "pve_step_many: unknown action source");
    if ((ro->source == PVE_SRC_POOL || ro->source == PVE_SRC_TABLE) && (!ro->pool || ro->n_pool <= 0 || ro->pool_tick0 < 0))
        return fail(PVE_ERR_INVALID, "pve_step_many: PVE_SRC_POOL / PVE_SRC_TABLE need pool, n_pool > 0 and pool_tick0 >= 0");
    if (ro->source == PVE_SRC_TABLE && (ro->table_ids <= 0 || (h->geo && out && (out->obs_pre || out->state_pre))))
        return fail(PVE_ERR_INVALID, "pve_step_many: PVE_SRC_TABLE needs table_ids > 0 (lane_num 4 / 8: no obs_pre / state_pre)");
    if (ro->source == PVE_SRC_ACTOR && (!ro->actor_obs || !ro->actor_actions || !out || !out->obs_post))
        return fail(PVE_ERR_INVALID, "pve_step_many: PVE_SRC_ACTOR needs actor_obs, actor_actions and out->obs_post");
    if (out && out->state_pre && !ro->trajectory)
        return fail(PVE_ERR_INVALID, "pve_step_many: state_pre reads the rows the previous tick stored: trajectory = 1 (every tick its own obs_post block)");
    if (ro->source == PVE_SRC_ACTOR && ro->trajectory && (const void *)out->obs_post == ro->actor_obs)
        return fail(PVE_ERR_INVALID, "pve_step_many: with trajectory = 1 actor_obs must not alias out->obs_post");
    Params P;
    int rc = tick_params(h, nullptr, out, MODE_FUSED, who, P);
    if (rc != PVE_OK) return rc;
    h->last_launch_kind = PVE_LAUNCH_NONE;          // (a call of zero ticks launches nothing)
    clear_variant(h);
    if (ro->n_ticks == 0) return PVE_OK;
    if (ro->source == PVE_SRC_ACTOR) {
        rc = use_actor(h, ro->actor_weights, who);
        if (rc != PVE_OK) return rc;
    }
    DevScope dev_scope(h->device);
    const Outputs o0 = P.out;
    const long long E = h->n_envs, cap = h->cap;
    const bool f32 = P.obs_f32 != 0;
    std::string err;
    // state resident on the chip between the ticks (one launch per chunk); not every configuration has that kernel
    if (ro->chunk_ticks < 0) return fail(PVE_ERR_INVALID, "pve_step_many: chunk_ticks must be >= 0");
    // persistent form: ONE launch, the workgroups pull (intersection, chunk) items from the queue in the workspace
    static const bool pers_off = PVE_KNOB("PVE_NO_PERSISTENT") != nullptr;            // A/B knob
    if (ro->persistent && !pers_off && ro->chunk_ticks > 0 && ro->chunk_ticks <= 255 && ro->n_ticks > ro->chunk_ticks &&
        (ro->source == PVE_SRC_ZERO || ro->source == PVE_SRC_POOL || ro->source == PVE_SRC_TABLE ||
         (ro->source == PVE_SRC_ACTOR && !(actor_mode(h) & 2)))) {
        RolloutArgs R;
        fill_rollout_args(h, ro, 0, ro->actor_obs, o0.obs_prev_post, R);
        item_schedule(ro->n_ticks, ro->chunk_ticks, R);
        R.call_ticks = ro->n_ticks;
        R.actor_actions = ro->actor_actions;
        R.queue = (unsigned *)(h->ws + h->L.off_queue);
        R.n_shards = Backend::n_xcc(h->device);
        R.done_base = h->q_done_base;
        const int rr = launch_rollout(h, P, R, err);
        if (rr < 0) { (void)queue_reset(h); return fail(PVE_ERR_NO_DEVICE, std::string(who) + ": " + err); }
        if (rr == 0) {
            h->q_done_base += (unsigned)(R.n_full + R.n_taper);
            h->ticks_since_reset += ro->n_ticks;
            h->last_launch_kind = PVE_LAUNCH_PERSISTENT;
            commit_variant(h);
            return PVE_OK;
        }
        // (no persistent kernel for this configuration: chunked launches below)
    }
    {
        const int chunk = ro->chunk_ticks > 0 ? ro->chunk_ticks : ro->n_ticks;
        for (int k0 = 0; k0 < ro->n_ticks; k0 += chunk) {
            // the block of the tick before this launch: the rows its first tick's actor reads (the caller's in the first launch)
            // and, with a trajectory, the stale neighbour rows of state_pre
            Outputs prev = o0;
            if (k0 > 0 && ro->trajectory) shift_outputs(prev, o0, k0 - 1, E, cap, f32);
            RolloutArgs R;
            fill_rollout_args(h, ro, k0, k0 > 0 ? prev.obs_post : ro->actor_obs, k0 > 0 && ro->trajectory ? prev.obs_post : o0.obs_prev_post, R);
            R.n_ticks = (ro->n_ticks - k0 < chunk) ? ro->n_ticks - k0 : chunk;
            R.exact_f32 = (actor_mode(h) & 2) ? 1 : 0;
            if (ro->trajectory) shift_outputs(P.out, o0, k0, E, cap, f32);
            const int rr = launch_rollout(h, P, R, err);
            if (rr < 0) return fail(PVE_ERR_NO_DEVICE, std::string(who) + ": " + err);
            if (rr > 0) {
                if (ro->source == PVE_SRC_TABLE)        // (nothing was launched: state and tick count are as before the call)
                    return fail(PVE_ERR_STATE, std::string(who) + (h->phase_cycles
                        ? ": PVE_SRC_TABLE runs in the resident kernel only, which has no phase-cycle build: disarm pve_debug_phase_cycles (NULL) first"
                        : ": PVE_SRC_TABLE runs in the resident kernel only"));
                if (k0 == 0) break;                 // no resident kernel for this configuration: per-tick launches below
                return fail(PVE_ERR_STATE, std::string(who) + ": resident kernel refused a later chunk");
            }
            h->ticks_since_reset += R.n_ticks;
            h->last_launch_kind = PVE_LAUNCH_RESIDENT;
            commit_variant(h);
            if (k0 + R.n_ticks >= ro->n_ticks) return PVE_OK;
        }
        P.out = o0;
    }
    // one launch per tick (two with the actor), enqueued from C: no host round trip between them either
    const void *obs_in = ro->actor_obs;
    for (int k = 0; k < ro->n_ticks; k++) {
        if (ro->trajectory) {
            shift_outputs(P.out, o0, k, E, cap, f32);
            if (k > 0) { Outputs prev; shift_outputs(prev, o0, k - 1, E, cap, f32); P.out.obs_prev_post = prev.obs_post; }
        }
        if (ro->source == PVE_SRC_POOL)
            P.actions = ro->pool + (size_t)(((long long)ro->pool_tick0 + k) % ro->n_pool) * (size_t)(E * cap);
        else if (ro->source == PVE_SRC_ACTOR) {
            if (run_actor(h, obs_in, ro->actor_actions, err) != 0) return fail(PVE_ERR_NO_DEVICE, std::string(who) + ": " + err);
            launch_note().launches += 1;
            P.actions = ro->actor_actions;
            obs_in = P.out.obs_post;
        }
        rc = launch_one_tick(h, P, who);
        if (rc != PVE_OK) return rc;
    }
    return PVE_OK;
}

int pve_compact(pve_handle h, double *obs_post)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_compact: null handle");
    if (!h->is_reset) return fail(PVE_ERR_STATE, "pve_compact: call pve_set_arrivals + pve_reset first");
    if (obs_post && (h->cfg.flags & PVE_CFG_OBS_F32))
        return fail(PVE_ERR_INVALID, "pve_compact: moving observation rows is not available with PVE_CFG_OBS_F32 (fused ticks only)");
    DevScope dev_scope(h->device);
    Params P = base_params(h);
    P.mode = MODE_COMPACT;
    P.out.obs_post = obs_post;
    std::string err;
    if (Backend::launch_compact(P, h->cap, h->stream, err) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_compact: " + err);
    return PVE_OK;
}

int pve_synchronize(pve_handle h)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_synchronize: null handle");
    DevScope dev_scope(h->device);
    std::string err;
    if (Backend::sync(h->stream, err) != 0) {
        (void)queue_reset(h);             // (a persistent launch may have died half-way: host and device counts restart together)
        return fail(PVE_ERR_NO_DEVICE, "pve_synchronize: " + err);
    }
    return PVE_OK;
}

static int fetch_header(pve_handle h, int env, EnvHeader *hd)
{
    DevScope dev_scope(h->device);
    return Backend::d2h(hd, h->ws + h->L.off_headers + sizeof(EnvHeader) * (size_t)env, sizeof(EnvHeader), h->stream);
}

int pve_read_env(pve_handle h, int env, pve_env_info *out)
{
    if (!h || !out) return fail(PVE_ERR_INVALID, "pve_read_env: null argument");
    if (env < 0 || env >= h->n_envs) return fail(PVE_ERR_INVALID, "pve_read_env: env out of range");
    EnvHeader hd;
    if (fetch_header(h, env, &hd) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_read_env: device copy failed");
    out->current_time = hd.current_time;
    out->n_alive = hd.n_alive;
    for (int l = 0; l < NL; l++) {
        out->lane_count[l] = hd.lane_start[l + 1] - hd.lane_start[l];
        out->veh_rec[l] = hd.veh_rec[l];
    }
    for (int d = 0; d < ND; d++) {
        out->head_valid[d] = (hd.head_valid >> d) & 1;
        out->head_lane[d] = out->head_valid[d] ? hd.head_lane[d] : -1;
        out->head_j[d] = out->head_valid[d] ? hd.head_j[d] : -1;
    }
    out->intention_re = hd.intention_re;
    out->id_seq = hd.id_seq; out->passed_veh = hd.passed; out->passed_veh_step_total = hd.passed_step_total;
    out->overflow = hd.overflow;
    return PVE_OK;
}

int pve_read_vehicles(pve_handle h, int env, pve_vehicle *out, int max_n, int *n_out)
{
    if (!h || !n_out) return fail(PVE_ERR_INVALID, "pve_read_vehicles: null argument");
    if (env < 0 || env >= h->n_envs) return fail(PVE_ERR_INVALID, "pve_read_vehicles: env out of range");
    EnvHeader hd;
    if (fetch_header(h, env, &hd) != 0) return fail(PVE_ERR_NO_DEVICE, "pve_read_vehicles: device copy failed");
    const int n = hd.n_alive;
    *n_out = n;
    if (!out || max_n <= 0) return PVE_OK;
    const int m = n < max_n ? n : max_n;
    const int cap = h->cap;
    DevScope dev_scope(h->device);
    static_assert(Opt::max_capacity <= 256, "pve_read_vehicles: the slot rows below hold 256 slots");
    double f[NF64][256];
    int32_t iv[NI32][256];
    if (h->n_envs == 1) {
        // single-env handles (the drop-in compatibility class): the whole workspace is ~11 KB, one copy
        std::string buf(h->L.total, '\0');
        if (Backend::d2h(&buf[0], h->ws, h->L.total, h->stream) != 0)
            return fail(PVE_ERR_NO_DEVICE, "pve_read_vehicles: device copy failed");
        memcpy(&hd, buf.data() + h->L.off_headers, sizeof(EnvHeader));
        for (int k = 0; k < NF64; k++) memcpy(f[k], buf.data() + h->L.off_f64[k], 8 * (size_t)cap);
        for (int k = 0; k < NI32; k++) memcpy(iv[k], buf.data() + h->L.off_i32[k], 4 * (size_t)cap);
    } else {
        for (int k = 0; k < NF64; k++)
            if (Backend::d2h(f[k], h->ws + h->L.off_f64[k] + 8 * (size_t)env * cap, 8 * (size_t)cap, h->stream) != 0)
                return fail(PVE_ERR_NO_DEVICE, "pve_read_vehicles: device copy failed");
        for (int k = 0; k < NI32; k++)
            if (Backend::d2h(iv[k], h->ws + h->L.off_i32[k] + 4 * (size_t)env * cap, 4 * (size_t)cap, h->stream) != 0)
                return fail(PVE_ERR_NO_DEVICE, "pve_read_vehicles: device copy failed");
    }
    for (int s = 0; s < m; s++) {
        pve_vehicle &v = out[s];
        int lane = 0;
        for (int L = 1; L < NL; L++) lane += (s >= hd.lane_start[L]) ? 1 : 0;
        v.p = f[F_P][s]; v.v = f[F_V][s]; v.a = f[F_A][s]; v.jerk = f[F_JERK][s];
        v.jerk_sum = f[F_JERK_SUM][s]; v.vir_dis = f[F_VIR_DIS][s]; v.closer_p = f[F_CLOSER_P][s];
        v.lane = lane; v.j = s - hd.lane_start[lane];
        v.id = iv[I_ID][s]; v.vnum = iv[I_VNUM][s]; v.seq_in_lane = iv[I_SEQ][s];
        const int meta = iv[I_META][s];
        v.control = (meta & M_CONTROL) ? 1 : 0; v.finish = (meta & M_FINISH) ? 1 : 0;
        v.done = (meta & M_DONE) ? 1 : 0; v.collision = (meta >> M_COLL_SHIFT) & M_COLL_MASK;
        v.step = iv[I_STEP][s]; v.count = iv[I_COUNT][s];
        v.lock = (meta & M_LOCK) ? 1 : 0;
        v.lock_a = (meta & M_LOCKA_POS) ? 1 : ((meta & M_LOCKA_NEG) ? -1 : 0);
        const int hw = iv[I_HDR][s];
        v.vir_header[0] = hw < 0 ? -1 : (hw >> 16); v.vir_header[1] = hw < 0 ? -1 : (hw & 0xffff);
        if (h->lane_num == 12) { v.intention = lane % 3; v.route = lane; }            /* ref :393-394, :400 */
        else {
            v.intention = (meta >> M_INT_SHIFT) & M_INT_MASK;                         /* ref :382-392 */
            v.route = h->g.direction[lane][v.intention];                              /* ref :400 */
        }
    }
    return PVE_OK;
}

int pve_get_metrics(pve_handle h, double out[PVE_N_METRICS])
{
    if (!h || !out) return fail(PVE_ERR_INVALID, "pve_get_metrics: null argument");
    const size_t bytes = sizeof(EnvHeader) * (size_t)h->n_envs;
    EnvHeader *hd = (EnvHeader *)malloc(bytes);
    if (!hd) return fail(PVE_ERR_NOMEM, "pve_get_metrics: out of host memory");
    DevScope dev_scope(h->device);
    if (Backend::d2h(hd, h->ws + h->L.off_headers, bytes, h->stream) != 0) {
        free(hd);
        return fail(PVE_ERR_NO_DEVICE, "pve_get_metrics: device copy failed");
    }
    for (int k = 0; k < PVE_N_METRICS; k++) out[k] = 0;
    for (int e = 0; e < h->n_envs; e++) {
        out[PVE_M_SLOT_STEPS] += (double)hd[e].ticks * h->cap;
        out[PVE_M_ALIVE_STEPS] += (double)hd[e].alive_steps;
        out[PVE_M_CTL_STEPS] += (double)hd[e].ctl_steps;
        out[PVE_M_SPAWNED] += hd[e].id_seq;
        out[PVE_M_PASSED] += hd[e].passed;
        out[PVE_M_COLLIDED] += hd[e].collided;
        out[PVE_M_LOCKS] += hd[e].locks;
        out[PVE_M_SUM_REWARD] += hd[e].sum_reward;
        out[PVE_M_SUM_JERK] += hd[e].sum_jerk;
        out[PVE_M_PASSED_STEPS] += hd[e].passed_step_total;
        out[PVE_M_OVERFLOW] += hd[e].overflow;
        out[PVE_M_TICKS] += (double)hd[e].ticks;
    }
    free(hd);
    return PVE_OK;
}

int pve_debug_phase_cycles(pve_handle h, uint64_t *dev_counters16)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_debug_phase_cycles: null handle");
    h->phase_cycles = (unsigned long long *)dev_counters16;
    return PVE_OK;
}

int pve_debug_last_launch(pve_handle h)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_debug_last_launch: null handle");
    return h->last_launch_kind;
}

int pve_debug_last_variant(pve_handle h, pve_launch_variant *out)
{
    if (!h || !out) return fail(PVE_ERR_INVALID, "pve_debug_last_variant: null handle or out");
    *out = h->last_variant;
    return PVE_OK;
}

int pve_debug_item_schedule(int n_ticks, int chunk_ticks, int32_t out[12])
{
    if (!out || n_ticks < 1 || chunk_ticks < 1 || chunk_ticks > 255 || n_ticks <= chunk_ticks)
        return fail(PVE_ERR_INVALID, "pve_debug_item_schedule: needs 0 < chunk_ticks <= 255, chunk_ticks < n_ticks and out");
    RolloutArgs R;
    memset(&R, 0, sizeof(R));
    item_schedule(n_ticks, chunk_ticks, R);
    out[0] = R.n_ticks; out[1] = R.n_full; out[2] = R.n_taper;
    for (int k = 0; k < 8; k++) out[3 + k] = k < R.n_taper ? (int)R.taper[k] : 0;
    out[11] = R.n_full + R.n_taper;
    return PVE_OK;
}

int pve_debug_stop_phase(pve_handle h, int n)
{
    if (!h) return fail(PVE_ERR_INVALID, "pve_debug_stop_phase: null handle");
    h->stop_phase = n < 0 ? -1 : n;
    return PVE_OK;
}

int pve_debug_traffic_probe(pve_handle h, int32_t *dev_sink)
{
    if (!h || !dev_sink) return fail(PVE_ERR_INVALID, "pve_debug_traffic_probe: null argument");
    DevScope dev_scope(h->device);
    Params P = base_params(h);
    std::string err;
    if (Backend::launch_probe(P, h->cap, dev_sink, h->stream, err) != 0)
        return fail(PVE_ERR_NO_DEVICE, "pve_debug_traffic_probe: " + err);
    return PVE_OK;
}

int pve_state_field(pve_handle h, const char *field, void **dev_ptr, int *elem_bytes)
{
    if (!h || !field || !dev_ptr || !elem_bytes) return fail(PVE_ERR_INVALID, "pve_state_field: null argument");
    static const char *fn[NF64] = {"p", "v", "a", "jerk", "jerk_sum", "vir_dis", "closer_p"};
    static const char *in[NI32] = {"id", "seq", "vnum", "step", "count", "meta", "hdr"};
    for (int k = 0; k < NF64; k++)
        if (!strcmp(field, fn[k])) { *dev_ptr = h->ws + h->L.off_f64[k]; *elem_bytes = 8; return PVE_OK; }
    for (int k = 0; k < NI32; k++)
        if (!strcmp(field, in[k])) { *dev_ptr = h->ws + h->L.off_i32[k]; *elem_bytes = 4; return PVE_OK; }
    return fail(PVE_ERR_INVALID, std::string("pve_state_field: unknown field ") + field);
}

}  // extern "C"

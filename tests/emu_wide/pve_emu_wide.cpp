// pve_emu_wide.cpp -- CPU *test* emulator of the 12-lane HIP kernels at 64, 128 and 256 slots (NOT a product path, never
// shipped in libpveenv.so, never selected by the package on its own).
//
// tests/emu/pve_emu.cpp emulates every kernel family at 64 and 128 slots and declares no Backend::max_capacity, so the C ABI
// refuses 256 there.  This library runs the same phase bodies (csrc/pve_tick_core.h) of the 12-lane kernels -- the tick,
// the resident roll-out (chunked launches and the work queue, emulated sequentially), compaction and reset -- for every
// thread t = 0..CAP-1 of a workgroup, phase by phase, behind the same C ABI (csrc/pve_capi.inc) on host memory, and declares
// max_capacity = 256.  At 256 slots it follows the 256-slot kernels' phase order: the training states are written per
// thread (ph_state) instead of the byte-descriptor cooperative write.  The 4- / 8-lane layouts are not emulated here (the
// C ABI refuses them at 256; tests/emu covers them at 64 / 128).
#include <new>
#include <string>
#include <vector>

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_host.h"
#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_tick_core.h"
#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_tick_geo.h"
#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_actor.h"

using namespace pve;

// the training states as the kernels of this capacity write them: descriptors + cooperative write up to 128 slots, per thread at 256
template <int CAP, class T, class OutT>
static void emu_state(const Params &P, const OutT &O, int env, typename T::Sh &sh, std::vector<Regs> &regs)
{
    if constexpr (CAP <= 128) {
        for (int t = 0; t < CAP; t++) T::ph_state_publish(O, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_state_coop(P, O, env, t, sh);
    } else {
        for (int t = 0; t < CAP; t++) T::ph_state(P, O, env, t, sh, regs[t]);
    }
}

template <int CAP> static void emu_tick(const Const &c, const Params &P)
{
    typedef Tick<CAP> T;
    std::vector<Regs> regs(CAP);
    Shared<CAP> *shp = new Shared<CAP>();
    for (int env = 0; env < P.n_envs; env++) {
        Shared<CAP> &sh = *shp;
        memset(&sh, 0, sizeof(sh));
        for (int t = 0; t < CAP; t++) T::ph_load(c, P, env, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_step1(c, P, env, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_step2(c, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_lists_a(c, t, sh);
        for (int t = 0; t < CAP; t++) T::ph_step3(c, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_step3_publish(t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_lists_b(t, sh);
        for (int t = 0; t < CAP; t++) T::ph_build(c, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_rank(t, sh, env);
        for (int t = 0; t < CAP; t++) T::ph_scan(c, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_reward(c, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_effects(c, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_prefetch_arrival(P, env, t, sh, regs[t], NL);
        for (int t = 0; t < CAP; t++) T::ph_lock(c, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_lock2(t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) T::ph_final(c, P, env, t, sh, regs[t]);
        if (P.out.state_pre) emu_state<CAP, T>(P, P.out, env, sh, regs);
    }
    delete shp;
}

// k_rollout (register build, every source but the actor): the resident multi-tick form, phase by phase as the kernel orders them.
// k_base: first tick of this launch / queue item within the call's output blocks
template <int CAP> static void emu_rollout(const Const &c, const Params &P, const RolloutArgs &R, int k_base = 0)
{
    typedef Tick<CAP> T;
    std::vector<Regs> regs(CAP);
    std::vector<FinCarry> fcs(CAP);
    std::vector<HomeRegs> hrs(CAP);
    Shared<CAP> *shp = new Shared<CAP>();
    for (int env = 0; env < P.n_envs; env++) {
        Shared<CAP> &sh = *shp;
        memset(&sh, 0, sizeof(sh));
        int pool_idx = R.pool_tick0;
        const bool idt = R.source == 3;                      // PVE_SRC_TABLE: actions by (tick, vehicle id)
        auto tab = [&](int row, int id) { return R.pool[(size_t)row * (size_t)R.table_ids + (id < 0 ? 0 : (id < R.table_ids ? id : R.table_ids - 1))]; };
        std::vector<double> sp_act(CAP, 0.0);
        for (int t = 0; t < CAP; t++) T::ph_load(c, P, env, t, sh, regs[t]);
        if (idt) for (int t = 0; t < CAP; t++) regs[t].act = regs[t].alive ? tab(pool_idx, regs[t].id) : 0.0;
        for (int k = 0; k < R.n_ticks; k++) {
            const bool last_tick = k + 1 == R.n_ticks;
            for (int w = 0; w < CAP / 64; w++)      // the emulator's vote() ORs bits: start every tick from empty masks
                sh.m_alive[w] = sh.m_ctl[w] = sh.m_del[w] = sh.m_fin[w] = sh.m_ctlnow[w] = sh.m_coll[w] = sh.m_lead[w] = sh.m_spawn[w] = 0;
            sh.emu_scan = 0;
            if (k > 0) for (int t = 0; t < CAP; t++) T::ph_tick_init(c, t, sh, regs[t]);
            for (int t = 0; t < CAP; t++) T::ph_step1(c, P, env, t, sh, regs[t]);
            for (int t = 0; t < CAP; t++) T::ph_step2(c, t, sh, regs[t]);
            for (int t = 0; t < CAP; t++) T::ph_lists_a(c, t, sh);
            for (int t = 0; t < CAP; t++) T::ph_step3(c, t, sh, regs[t], last_tick);
            for (int t = 0; t < CAP; t++) T::ph_step3_publish(t, sh, regs[t]);
            for (int t = 0; t < CAP; t++) T::ph_lists_b(t, sh);
            for (int t = 0; t < CAP; t++) T::ph_build(c, t, sh, regs[t]);
            for (int t = 0; t < CAP; t++) T::ph_rank(t, sh);
            for (int t = 0; t < CAP; t++) T::ph_scan(c, t, sh, regs[t]);
            for (int t = 0; t < CAP; t++) T::ph_reward(c, t, sh, regs[t]);
            int nx = -1;
            if (k + 1 < R.n_ticks) { pool_idx = (pool_idx + 1 == R.n_pool) ? 0 : pool_idx + 1; nx = pool_idx; }
            if (idt) for (int t = 0; t < CAP; t++) regs[t].act_nx = (nx >= 0 && regs[t].alive) ? tab(nx, regs[t].id) : 0.0;
            else for (int t = 0; t < CAP; t++) T::ph_prefetch_action(P, R, env, t, nx, regs[t]);
            for (int t = 0; t < CAP; t++) T::ph_effects(c, t, sh, regs[t]);
            for (int t = 0; t < CAP; t++) T::ph_prefetch_arrival(P, env, t, sh, regs[t], NL);
            if (idt) {                               // first action of the vehicles spawned at the end of this tick
                const unsigned want = (unsigned)(sh.m_spawn[0] & 0xFFFull);
                unsigned sp = 0; int room = CAP - sh.hd.n_alive;
                for (int l = 0; l < NL; l++) if ((want >> l) & 1) { if (room > 0) { sp |= 1u << l; room--; } }
                for (int t = 0; t < NL; t++)
                    sp_act[t] = (((sp >> t) & 1) && nx >= 0) ? tab(nx, sh.hd.id_seq + __builtin_popcount(sp & ((1u << t) - 1u))) : 0.0;
            }
            for (int t = 0; t < CAP; t++) T::ph_lock(c, t, sh, regs[t], last_tick);
            for (int t = 0; t < CAP; t++) T::ph_lock2(t, sh, regs[t], last_tick);
            for (int t = 0; t < CAP; t++) T::ph_keep_prefix(t, sh);
            if (!idt) for (int t = 0; t < CAP; t++) T::ph_park_action(t, sh, regs[t]);
            const Outputs O = T::tick_outputs(P, R, k_base + k);
            for (int t = 0; t < CAP; t++)
                T::template ph_final<true>(c, P, O, env, t, sh, regs[t], fcs[t], k + 1 == R.n_ticks || O.state_pre != nullptr);
            if (idt) for (int t = 0; t < CAP; t++) if (fcs[t].new_slot >= 0) sh.act_next[fcs[t].new_slot] = regs[t].act_nx;
            for (int t = 0; t < CAP; t++) T::ph_home_take(t, sh, regs[t], fcs[t], hrs[t]);
            if (fcs[0].still) {                       // (uniform) nobody moves: the registers carry over
                for (int t = 0; t < CAP; t++) T::ph_stage_header(t, sh, fcs[t]);
                for (int t = 0; t < CAP; t++) T::ph_carry_over(t, sh, regs[t], fcs[t]);
            } else {
                if (O.state_pre) emu_state<CAP, T>(P, O, env, sh, regs);
                for (int t = 0; t < CAP; t++) T::ph_stage(c, t, sh, regs[t], fcs[t]);
                for (int t = 0; t < CAP; t++) T::ph_home_put(t, sh, fcs[t], hrs[t]);
                if (idt) for (int t = 0; t < NL; t++) if (fcs[t].sp_slot >= 0) sh.act_next[fcs[t].sp_slot] = sp_act[t];
                if (k + 1 < R.n_ticks) for (int t = 0; t < CAP; t++) T::ph_reload(t, sh, regs[t]);
            }
        }
        for (int t = 0; t < CAP; t++) T::ph_flush(P, env, t, sh);
    }
    delete shp;
}

template <int CAP> static void emu_compact(const Params &P)
{
    std::vector<CRegs> regs(CAP);
    Shared<CAP> *shp = new Shared<CAP>();
    for (int env = 0; env < P.n_envs; env++) {
        Shared<CAP> &sh = *shp;
        memset(&sh, 0, sizeof(sh));
        for (int t = 0; t < CAP; t++) Tick<CAP>::ph_c_load(P, env, t, sh, regs[t]);
        for (int t = 0; t < CAP; t++) Tick<CAP>::ph_c_store(P, env, t, sh, regs[t]);
    }
    delete shp;
}

// one call per capacity: f(std::integral_constant<int, CAP>)
template <class F> static int by_cap(int cap, F f)
{
    if (cap == 64) f(std::integral_constant<int, 64>());
    else if (cap == 128) f(std::integral_constant<int, 128>());
    else if (cap == 256) f(std::integral_constant<int, 256>());
    else return -1;
    return 0;
}

struct Backend : BackendDefaults {
    static constexpr int max_capacity = 256;
    static int set_device(int, std::string &) { return 0; }
    static int enter_device(int) { return 0; }
    static void leave_device(int) {}
    static void *dmalloc(size_t n) { return calloc(1, n); }
    static void dfree(void *p) { free(p); }
    static int memset0(void *p, size_t n, void *) { memset(p, 0, n); return 0; }
    static int n_xcc(int) { return 1; }
    static int d2h(void *dst, const void *src, size_t n, void *) { memcpy(dst, src, n); return 0; }
    static int sync(void *, std::string &) { return 0; }
    static int launch_tick(const Const &c, const Params &P, int cap, void *, std::string &err)
    {
        if (by_cap(cap, [&](auto k) { emu_tick<decltype(k)::value>(c, P); }) != 0) { err = "no emulated tick for this capacity"; return -1; }
        note_launch(false, NL, cap, 0, false, false, P.out.obs_pre || P.out.state_pre, false, false, 0);
        return 0;
    }
    // the persistent form (R.queue): the items run sequentially, chunk-major -- the item schedule of the kernel's queue
    static int launch_rollout(const Const &c, const Params &P_in, const RolloutArgs &R, int cap, void *, std::string &err)
    {
        if (getenv("PVE_NO_ROLLOUT_KERNEL") || R.source == 2) return 1;
        auto emu = [&](const Params &P, const RolloutArgs &Rk, int kb) {
            return by_cap(cap, [&](auto k) { emu_rollout<decltype(k)::value>(c, P, Rk, kb); });
        };
        Params P = P_in;
        RolloutArgs Rk = R;
        if (!R.queue) {
            if (R.source == 1) {
                Rk.pool_tick0 = R.pool_tick0 % R.n_pool;
                P.actions = R.pool + (size_t)Rk.pool_tick0 * (size_t)P.n_envs * (size_t)cap;
            } else P.actions = nullptr;
            if (R.source == 3) Rk.pool_tick0 = R.pool_tick0 % R.n_pool;
            if (emu(P, Rk, 0) != 0) { err = "no emulated roll-out for this capacity"; return -1; }
            note_launch(false, NL, cap, 0, false, false, P_in.out.obs_pre || P_in.out.state_pre, R.source == 3, false, 0);
            return 0;
        }
        for (int chunk = 0; chunk < R.n_full + R.n_taper; chunk++) {
            int kb, nt;
            rollout_item(R, chunk, kb, nt);
            if (nt < 1 || kb + nt > R.call_ticks) { err = "emulated work queue: inconsistent item schedule"; return -1; }
            Rk.n_ticks = nt;
            Rk.pool_tick0 = (R.source == 1 || R.source == 3) ? (R.pool_tick0 + kb) % R.n_pool : 0;
            P.actions = R.source == 1 ? R.pool + (size_t)Rk.pool_tick0 * (size_t)P.n_envs * (size_t)cap : nullptr;
            if (emu(P, Rk, kb) != 0) { err = "no emulated roll-out for this capacity"; return -1; }
        }
        note_launch(false, NL, cap, 0, false, false, P_in.out.obs_pre || P_in.out.state_pre, R.source == 3, true, 0);
        return 0;
    }
    static int launch_compact(const Params &P, int cap, void *, std::string &err)
    {
        if (by_cap(cap, [&](auto k) { emu_compact<decltype(k)::value>(P); }) != 0) { err = "no emulated compaction for this capacity"; return -1; }
        return 0;
    }
    static int launch_reset(const Const &c, const Params &P, int cap, void *, std::string &err)
    {
        for (int env = 0; env < P.n_envs; env++)
            if (by_cap(cap, [&](auto k) { reset_env<decltype(k)::value>(c, P, env, 200000); }) != 0) { err = "no emulated reset for this capacity"; return -1; }
        return 0;
    }
    // the 4- / 8-lane layouts and the general path: tests/emu
    static int launch_tick_geo(const GeoConst &, const Params &, int, void *, std::string &err) { err = "the wide emulator runs the 12-lane fast path only"; return -1; }
    static int launch_reset_geo(const GeoConst &, const Params &, int, void *, std::string &err) { err = "the wide emulator runs the 12-lane fast path only"; return -1; }
    static int launch_rollout_geo(const GeoConst &, const Params &, const RolloutArgs &, int, void *, std::string &err) { err = "the wide emulator runs the 12-lane fast path only"; return -1; }
    // the canonical float32 evaluation order of csrc/pve_actor.h (what the matrix-core kernel computes)
    static int pack_actor(const float *W, float *flat, unsigned char *, void *, std::string &)
    {
        memcpy(flat, W, sizeof(float) * AW_TOTAL);
        return 0;
    }
    static int launch_actor(const float *W, const unsigned char *, const void *obs_v, int obs_f32, const int32_t *meta,
                            double *actions, int n_envs, int cap, void *, std::string &)
    {
        const double *obs = (const double *)obs_v;
        const float *obsf = (const float *)obs_v;
        for (size_t s = 0; s < (size_t)n_envs * cap; s++) {
            if ((meta[s] & (M_ALIVE | M_CONTROL)) != (M_ALIVE | M_CONTROL)) { actions[s] = 0.0; continue; }
            float x[ACT_IN];
            for (int k = 0; k < ACT_IN; k++) x[k] = (obs_f32 & 1) ? obsf[s * OBSW + k] : (float)obs[s * OBSW + k];
            actions[s] = (double)actor_canonical(W, x);
        }
        return 0;
    }
    static int launch_probe(const Params &, int, int *, void *, std::string &) { return 0; }
};

#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_capi.inc"

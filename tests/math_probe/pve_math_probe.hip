// pve_math_probe.hip -- the tick's small arithmetic helpers (csrc/pve_tick_core.h, pve_tick_geo.h, pve_actor.h), one
// at a time, over caller-supplied arrays.  Test infrastructure only: tests/test_math_probe.py, tests/test_gpu_math_probe.py.
// The last section does the same for the generators' and replay helpers' functions (pve_noise.h, pve_arrivals.h,
// pve_replay.h, pve_prio.h): tests/test_gen_probe.py, tests/test_gpu_gen_probe.py.
//
// One source, two builds (tests/math_probe/Makefile):
//   libpve_math_probe_hip.so   hipcc with the product's HIPFLAGS: every entry point launches ONE one-dimensional,
//                              bounds-checked, element-wise kernel over DEVICE arrays, synchronises and returns the hipError_t
//   libpve_math_probe_host.so  g++ -x c++ with the flags of tests/emu: the entry points loop over HOST arrays (the `#else`
//                              branches of the helpers, i.e. what the CPU emulator executes)
// No logic of its own beyond calling the helper.  Const / GeoConst are built from a pve_config by make_const /
// make_geo_const and read, on the device, through the kernel-argument address-space-4 reference as k_tick reads them, so
// that sel2 / sel4 see scalar-loaded table entries.  lane / m (which select table entries) are scalars of a call and are
// validated on the host before the launch.
//
// Every entry point: int pve_probe_<name>(const pve_config *cfg, const pve_probe_args *a)
//   0 = done; > 0 = hipError_t; < 0 = the arguments were refused (PROBE_E_*), nothing ran.
#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_host.h"
#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_tick_core.h"
#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_tick_geo.h"
#if PVE_DEVICE_CODE
#include "../../pve-mcc_for_unsignalized_intersection_amd/csrc/pve_actor.h"
#endif

using namespace pve;

extern "C" {
typedef struct pve_probe_args {
    long long n;             // elements (one thread / loop iteration each)
    const void *in[6];       // input arrays, n elements each unless an entry point says otherwise
    void *out[3];            // output arrays
    int k[4];                // scalars: lane, m | NW, elements per mask
} pve_probe_args;
}
typedef pve_probe_args ProbeArgs;

enum { PROBE_E_ARGS = -1, PROBE_E_LANE = -2, PROBE_E_DEVICE_ONLY = -3 };

template <class T> PVE_HD const T *in(const PVE_AS4 ProbeArgs &a, int k) { return (const T *)a.in[k]; }
template <class T> PVE_HD T *out(const PVE_AS4 ProbeArgs &a, int k) { return (T *)a.out[k]; }

#if PVE_DEVICE_CODE
typedef __attribute__((address_space(4))) const char *KernargPtr;
template <class CT, class B>
__global__ void k_each(const CT c_arg, const ProbeArgs a_arg)
{
    KernargPtr ka = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const PVE_AS4 CT &c = *(const PVE_AS4 CT *)ka;
    const PVE_AS4 ProbeArgs &a = *(const PVE_AS4 ProbeArgs *)(ka + ((sizeof(CT) + 7) / 8 * 8));
    const long long i = (long long)blockIdx.x * (long long)blockDim.x + (long long)threadIdx.x;
    if (i < a.n) B::f(c, a, i);
}
template <class CT, class B> static int run(const CT &c, const ProbeArgs &a, int block = 256)
{
    if (a.n == 0) return 0;
    const unsigned grid = (unsigned)((a.n + block - 1) / block);
    hipLaunchKernelGGL((k_each<CT, B>), dim3(grid), dim3((unsigned)block), 0, 0, c, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}
#else
template <class CT, class B> static int run(const CT &c, const ProbeArgs &a, int = 0)
{
    for (long long i = 0; i < a.n; i++) B::f(c, a, i);
    return 0;
}
#endif

#define PROBE_F(CT) static PVE_HD void f(const PVE_AS4 CT &c, const PVE_AS4 ProbeArgs &a, long long i)
typedef Tick<64> T64;

// ---------------------------------------------------------------------------------- reward terms
struct B_exp_m2_0 { PROBE_F(Const) { out<double>(a, 0)[i] = exp_m2_0(in<double>(a, 0)[i]); } };
struct B_value_div { PROBE_F(Const) { out<double>(a, 0)[i] = value_div(in<double>(a, 0)[i], in<double>(a, 1)[i]); } };
struct B_reward_coth_term { PROBE_F(Const) { out<double>(a, 0)[i] = reward_coth_term(in<double>(a, 0)[i]); } };
struct B_reward_log_term { PROBE_F(Const) { out<double>(a, 0)[i] = reward_log_term(in<double>(a, 0)[i]); } };
// ---------------------------------------------------------------------------------- clamps
struct B_dmin { PROBE_F(Const) { out<double>(a, 0)[i] = dmin(in<double>(a, 0)[i], in<double>(a, 1)[i]); } };
struct B_dmax { PROBE_F(Const) { out<double>(a, 0)[i] = dmax(in<double>(a, 0)[i], in<double>(a, 1)[i]); } };
struct B_clip_a { PROBE_F(Const) { out<double>(a, 0)[i] = T64::clip_a(c, in<double>(a, 0)[i]); } };
struct B_outcome {       // in: p, v, a, ctl (int) -> out: pn, vn
    PROBE_F(Const) { T64::outcome(c, in<double>(a, 0)[i], in<double>(a, 1)[i], in<double>(a, 2)[i], in<int>(a, 3)[i] != 0, out<double>(a, 0)[i], out<double>(a, 1)[i]); }
};
// ---------------------------------------------------------------------------------- decisions
struct B_div_const { PROBE_F(Const) { out<double>(a, 0)[i] = div_const(in<double>(a, 0)[i], in<double>(a, 1)[i], in<double>(a, 2)[i]); } };
struct B_brake_needed { PROBE_F(Const) { out<int>(a, 0)[i] = brake_needed(c, in<double>(a, 0)[i], in<double>(a, 1)[i], in<double>(a, 2)[i], in<double>(a, 3)[i]); } };
struct B_key_less {      // in: d1, v1, r1 (int), d2, v2, r2 (int)
    PROBE_F(Const) { out<int>(a, 0)[i] = key_less(in<double>(a, 0)[i], in<double>(a, 1)[i], in<int>(a, 2)[i], in<double>(a, 3)[i], in<double>(a, 4)[i], in<int>(a, 5)[i]) ? 1 : 0; }
};
struct B_mul24 { PROBE_F(Const) { out<int>(a, 0)[i] = mul24(in<int>(a, 0)[i], in<int>(a, 1)[i]); } };
struct B_mad24 { PROBE_F(Const) { out<int>(a, 0)[i] = mad24(in<int>(a, 0)[i], in<int>(a, 1)[i], in<int>(a, 2)[i]); } };
// sqrt as ph_reward uses it (the FP64 collision distance)
struct B_sqrt_xy { PROBE_F(Const) { const double dx = in<double>(a, 0)[i], dy = in<double>(a, 1)[i]; out<double>(a, 0)[i] = sqrt(dx * dx + dy * dy); } };
// ---------------------------------------------------------------------------------- geometry (lane = k[0], m = k[1])
struct B_sincos_q1 { PROBE_F(Const) { sincos_q1(in<double>(a, 0)[i], out<double>(a, 0)[i], out<double>(a, 1)[i]); } };
struct B_frcp { PROBE_F(Const) { out<float>(a, 0)[i] = frcp(in<float>(a, 0)[i]); } };
struct B_get_xy { PROBE_F(Const) { get_xy(c, in<double>(a, 0)[i], a.k[0], out<double>(a, 0)[i], out<double>(a, 1)[i]); } };
struct B_get_xy_f32 { PROBE_F(Const) { get_xy_f32(c, in<double>(a, 0)[i], a.k[0], out<float>(a, 0)[i], out<float>(a, 1)[i]); } };
struct B_geo_xy { PROBE_F(GeoConst) { geo_xy(c, in<double>(a, 0)[i], a.k[0], a.k[1], out<double>(a, 0)[i], out<double>(a, 1)[i]); } };
struct B_geo_xy_f32 { PROBE_F(GeoConst) { geo_xy_f32(c, in<double>(a, 0)[i], a.k[0], a.k[1], out<float>(a, 0)[i], out<float>(a, 1)[i]); } };
// ---------------------------------------------------------------------------------- masks
struct B_below_sel { PROBE_F(Const) { out<u64>(a, 0)[i] = below_sel(in<int>(a, 0)[i]); } };
struct B_popc_below { PROBE_F(Const) { out<int>(a, 0)[i] = popc_below(in<u64>(a, 0)[i], in<int>(a, 1)[i]); } };
// in[0]: masks [n_masks][NW]; element i: mask i / k[1], t = i % k[1] (k[1] = values of t per mask).  The words are copied
// first: the product's masks live in LDS or registers, never behind a per-lane global pointer
#define PROBE_MASK_WORDS                                                   \
    u64 w[NW];                                                             \
    const int t = (int)(i % a.k[1]);                                       \
    for (int q = 0; q < NW; q++) w[q] = in<u64>(a, 0)[(i / a.k[1]) * NW + q]
template <int NW> struct B_mask_below { PROBE_F(Const) { PROBE_MASK_WORDS; out<int>(a, 0)[i] = mask_below<NW>(w, t); } };
template <int NW> struct B_mask_prev { PROBE_F(Const) { PROBE_MASK_WORDS; out<int>(a, 0)[i] = mask_prev<NW>(w, t); } };
template <int NW> struct B_mask_count { PROBE_F(Const) { PROBE_MASK_WORDS; (void)t; out<int>(a, 0)[i] = mask_count<NW>(w); } };
// mask_rank: t IS the calling thread (k[1] = 64 NW = the block size of the launch, one mask per block)
template <int NW> struct B_mask_rank { PROBE_F(Const) { PROBE_MASK_WORDS; out<int>(a, 0)[i] = mask_rank<NW>(w, t); } };
// ---------------------------------------------------------------------------------- actor activation (device only)
#if PVE_DEVICE_CODE
struct B_actor_tanh3 { PROBE_F(Const) { out<float>(a, 0)[i] = actor_tanh3(in<float>(a, 0)[i]); } };
#endif

// ---------------------------------------------------------------------------------- argument checks (host)
static int check(const pve_config *cfg, const ProbeArgs *a, int n_in, int n_out)
{
    if (!cfg || !a || a->n < 0 || a->n > (1ll << 30)) return PROBE_E_ARGS;
    if (cfg->lane_num != 12 && cfg->lane_num != 4 && cfg->lane_num != 8) return PROBE_E_ARGS;
    for (int q = 0; q < n_in; q++) if (a->n && !a->in[q]) return PROBE_E_ARGS;
    for (int q = 0; q < n_out; q++) if (a->n && !a->out[q]) return PROBE_E_ARGS;
    return 0;
}
static int check_lane12(const pve_config *cfg, const ProbeArgs *a)
{
    return (cfg->lane_num == 12 && a->k[0] >= 0 && a->k[0] < NL) ? 0 : PROBE_E_LANE;
}
static int check_route(const GeoConst &g, const ProbeArgs *a)
{
    const int lane = a->k[0], m = a->k[1];
    if (lane < 0 || lane >= g.lane_num || m < 0 || m > 2 || g.direction[lane][m] < 0) return PROBE_E_LANE;
    return 0;
}

#define PROBE_EXPORT(name, n_in, n_out)                                                          \
    extern "C" int pve_probe_##name(const pve_config *cfg, const pve_probe_args *a)             \
    {                                                                                            \
        const int bad = check(cfg, a, n_in, n_out);                                              \
        return bad ? bad : run<Const, B_##name>(make_const(*cfg), *a);                           \
    }
PROBE_EXPORT(exp_m2_0, 1, 1)
PROBE_EXPORT(value_div, 2, 1)
PROBE_EXPORT(reward_coth_term, 1, 1)
PROBE_EXPORT(reward_log_term, 1, 1)
PROBE_EXPORT(dmin, 2, 1)
PROBE_EXPORT(dmax, 2, 1)
PROBE_EXPORT(clip_a, 1, 1)
PROBE_EXPORT(outcome, 4, 2)
PROBE_EXPORT(div_const, 3, 1)
PROBE_EXPORT(brake_needed, 4, 1)
PROBE_EXPORT(key_less, 6, 1)
PROBE_EXPORT(mul24, 2, 1)
PROBE_EXPORT(mad24, 3, 1)
PROBE_EXPORT(sqrt_xy, 2, 1)
PROBE_EXPORT(sincos_q1, 1, 2)
PROBE_EXPORT(frcp, 1, 1)
PROBE_EXPORT(below_sel, 1, 1)
PROBE_EXPORT(popc_below, 2, 1)

#define PROBE_EXPORT_XY(name)                                                                    \
    extern "C" int pve_probe_##name(const pve_config *cfg, const pve_probe_args *a)             \
    {                                                                                            \
        int bad = check(cfg, a, 1, 2);                                                           \
        if (!bad) bad = check_lane12(cfg, a);                                                    \
        return bad ? bad : run<Const, B_##name>(make_const(*cfg), *a);                           \
    }
PROBE_EXPORT_XY(get_xy)
PROBE_EXPORT_XY(get_xy_f32)

#define PROBE_EXPORT_GEO(name)                                                                   \
    extern "C" int pve_probe_##name(const pve_config *cfg, const pve_probe_args *a)             \
    {                                                                                            \
        int bad = check(cfg, a, 1, 2);                                                           \
        if (bad) return bad;                                                                     \
        const GeoConst g = make_geo_const(*cfg);                                                 \
        bad = check_route(g, a);                                                                 \
        return bad ? bad : run<GeoConst, B_##name>(g, *a);                                       \
    }
PROBE_EXPORT_GEO(geo_xy)
PROBE_EXPORT_GEO(geo_xy_f32)

// k[0] = NW (1, 2, 4), k[1] = values of t per mask (>= 1); n = n_masks * k[1]
#define PROBE_EXPORT_MASK(name, block_of_nw)                                                     \
    extern "C" int pve_probe_##name(const pve_config *cfg, const pve_probe_args *a)             \
    {                                                                                            \
        const int bad = check(cfg, a, 1, 1);                                                     \
        if (bad) return bad;                                                                     \
        const int NW = a->k[0];                                                                  \
        if (a->k[1] < 1 || a->k[1] > 64 * NW + 1 || a->n % a->k[1] != 0) return PROBE_E_ARGS;   \
        if ((block_of_nw) && a->k[1] != 64 * NW) return PROBE_E_ARGS;                            \
        const Const c = make_const(*cfg);                                                        \
        if (NW == 1) return run<Const, B_##name<1>>(c, *a, (block_of_nw) ? 64 : 256);            \
        if (NW == 2) return run<Const, B_##name<2>>(c, *a, (block_of_nw) ? 128 : 256);           \
        if (NW == 4) return run<Const, B_##name<4>>(c, *a, 256);                                 \
        return PROBE_E_ARGS;                                                                     \
    }
PROBE_EXPORT_MASK(mask_below, 0)
PROBE_EXPORT_MASK(mask_prev, 0)
PROBE_EXPORT_MASK(mask_count, 0)
PROBE_EXPORT_MASK(mask_rank, 1)

extern "C" int pve_probe_actor_tanh3(const pve_config *cfg, const pve_probe_args *a)
{
    const int bad = check(cfg, a, 1, 1);
    if (bad) return bad;
#if PVE_DEVICE_CODE
    return run<Const, B_actor_tanh3>(make_const(*cfg), *a);
#else
    return PROBE_E_DEVICE_ONLY;      // v_exp_f32 / v_rcp_f32: no host form
#endif
}

// ====================================================================================== generators and replay helpers
// csrc/pve_noise.h, pve_arrivals.h, pve_replay.h, pve_prio.h (all reached through pve_host.h), one PVE_HD function per entry
// point: tests/gen_probe_scenarios.py, tests/test_gen_probe.py, tests/test_gpu_gen_probe.py.  Scalars of the helpers that are
// 64 bits wide or vary per element (seed, d, env_global, written, ..) are arrays, so that one call sweeps them; `bool`
// arguments travel as int32.  Four output words are a row of an [n][4] array.  Two helpers have preconditions whose breach
// would not end (replay_perm's walk for j >= N) or would trap the host (a capacity of 0 under `%`), and their arguments lie
// in device memory where the host cannot look before the launch: those elements are answered with all ones instead of a call.
typedef long long i64;
struct B_philox4x32_10 {     // in: counter [n][4], key [n][2] -> out: [n][4]
    PROBE_F(Const) {
        uint32_t w[4];
        for (int q = 0; q < 4; q++) w[q] = in<uint32_t>(a, 0)[4 * i + q];
        philox4x32_10(w, in<uint32_t>(a, 1)[2 * i], in<uint32_t>(a, 1)[2 * i + 1]);
        for (int q = 0; q < 4; q++) out<uint32_t>(a, 0)[4 * i + q] = w[q];
    }
};
struct B_noise_gauss { PROBE_F(Const) { out<double>(a, 0)[i] = noise_gauss(in<uint32_t>(a, 0)[i], in<uint32_t>(a, 1)[i]); } };
struct B_action_noise_z {    // in: seed, env_global, vehicle_id, tick
    PROBE_F(Const) { out<double>(a, 0)[i] = action_noise_z(in<uint64_t>(a, 0)[i], in<int64_t>(a, 1)[i], in<int32_t>(a, 2)[i], in<uint32_t>(a, 3)[i]); }
};
struct B_action_with_noise { // in: a, sigma, seed, env_global, vehicle_id, tick
    PROBE_F(Const) {
        ActionNoise nz = {};
        nz.sigma = in<double>(a, 1)[i]; nz.seed = in<uint64_t>(a, 2)[i];
        out<double>(a, 0)[i] = action_with_noise(in<double>(a, 0)[i], nz, in<int64_t>(a, 3)[i], in<int32_t>(a, 4)[i], in<uint32_t>(a, 5)[i]);
    }
};
struct B_arrival_exp { PROBE_F(Const) { out<double>(a, 0)[i] = arrival_exp(in<uint32_t>(a, 0)[i]); } };
struct B_arrival_gap { PROBE_F(Const) { out<double>(a, 0)[i] = arrival_gap(in<uint32_t>(a, 0)[i], in<double>(a, 1)[i], in<double>(a, 2)[i]); } };
#define PROBE_WORDS(fn)      /* in: seed, epoch, env_global, lane, quad | chunk -> out: [n][4] */                            \
    PROBE_F(Const) {                                                                                                         \
        uint32_t w[4];                                                                                                       \
        fn(in<uint64_t>(a, 0)[i], in<uint32_t>(a, 1)[i], in<i64>(a, 2)[i], in<int>(a, 3)[i], in<uint32_t>(a, 4)[i], w);     \
        for (int q = 0; q < 4; q++) out<uint32_t>(a, 0)[4 * i + q] = w[q];                                                   \
    }
struct B_arrival_words { PROBE_WORDS(arrival_words) };
struct B_intention_words { PROBE_WORDS(intention_words) };
struct B_intention_bit {     // in: words [n][4], r
    PROBE_F(Const) {
        uint32_t w[4];
        for (int q = 0; q < 4; q++) w[q] = in<uint32_t>(a, 0)[4 * i + q];
        out<int32_t>(a, 0)[i] = intention_bit(w, in<int>(a, 1)[i]);
    }
};
struct B_replay_half_bits { PROBE_F(Const) { out<int>(a, 0)[i] = replay_half_bits(in<uint32_t>(a, 0)[i]); } };
struct B_replay_feistel {    // in: seed, d, h (1 .. 16), x
    PROBE_F(Const) {
        const int h = in<int>(a, 2)[i];
        out<uint32_t>(a, 0)[i] = (h >= 1 && h <= 16) ? replay_feistel(in<uint64_t>(a, 0)[i], in<uint64_t>(a, 1)[i], h, in<uint32_t>(a, 3)[i]) : ~0u;
    }
};
struct B_replay_perm {       // in: seed, d, N (1 .. 2^31 - 1), j (< N)
    PROBE_F(Const) {
        const uint32_t N = in<uint32_t>(a, 2)[i], j = in<uint32_t>(a, 3)[i];
        out<uint32_t>(a, 0)[i] = (N <= 0x7FFFFFFFu && j < N) ? replay_perm(in<uint64_t>(a, 0)[i], in<uint64_t>(a, 1)[i], N, j) : ~0u;
    }
};
struct B_replay_append_plan {        // in: written, has_total (int), total, n_max, capacity (>= 1) -> out: (n, skip, start) [n][3]
    PROBE_F(Const) {
        const i64 capacity = in<i64>(a, 4)[i];
        ReplayPlan P = {-1, -1, -1};
        if (capacity >= 1) P = replay_append_plan(in<i64>(a, 0)[i], in<int>(a, 1)[i] != 0, in<i64>(a, 2)[i], in<i64>(a, 3)[i], capacity);
        out<i64>(a, 0)[3 * i] = P.n; out<i64>(a, 0)[3 * i + 1] = P.skip; out<i64>(a, 0)[3 * i + 2] = P.start;
    }
};
struct B_replay_append_slot {        // in: the plan's start, capacity, q
    PROBE_F(Const) {
        ReplayPlan P = {0, 0, in<i64>(a, 0)[i]};
        out<i64>(a, 0)[i] = replay_append_slot(P, in<i64>(a, 1)[i], in<i64>(a, 2)[i]);
    }
};
struct B_prio_key { PROBE_F(Const) { out<uint32_t>(a, 0)[i] = prio_key(in<int>(a, 0)[i] != 0, in<uint32_t>(a, 1)[i]); } };
struct B_prio_partition {    // in: part_from [32] (one table per call), L
    PROBE_F(Const) { const i64 *part_from = in<i64>(a, 0); out<int>(a, 0)[i] = prio_partition(part_from, in<i64>(a, 1)[i]); }
};
struct B_prio_draw_rank {    // in: ends [k[1]][k[0] + 1], seed, d, L; element i: row i / k[0], stratum i % k[0]
    PROBE_F(Const) {
        const i64 bsz = a.k[0];
        out<int32_t>(a, 0)[i] = prio_draw_rank(in<int32_t>(a, 0) + (i / bsz) * (bsz + 1), in<uint64_t>(a, 1)[i], in<uint64_t>(a, 2)[i], (uint32_t)(i % bsz), in<i64>(a, 3)[i]);
    }
};
struct B_prio_weight { PROBE_F(Const) { out<float>(a, 0)[i] = prio_weight(in<int32_t>(a, 0)[i], in<int32_t>(a, 1)[i], in<float>(a, 2)[i]); } };
struct B_prio_update_bits { PROBE_F(Const) { out<uint32_t>(a, 0)[i] = prio_update_bits(in<float>(a, 0)[i], in<int>(a, 1)[i] != 0, in<float>(a, 2)[i]); } };
struct B_prio_update_slot { PROBE_F(Const) { out<i64>(a, 0)[i] = prio_update_slot(in<i64>(a, 0)[i], in<i64>(a, 1)[i], in<i64>(a, 2)[i]); } };

PROBE_EXPORT(philox4x32_10, 2, 1)
PROBE_EXPORT(noise_gauss, 2, 1)
PROBE_EXPORT(action_noise_z, 4, 1)
PROBE_EXPORT(action_with_noise, 6, 1)
PROBE_EXPORT(arrival_exp, 1, 1)
PROBE_EXPORT(arrival_gap, 3, 1)
PROBE_EXPORT(arrival_words, 5, 1)
PROBE_EXPORT(intention_words, 5, 1)
PROBE_EXPORT(intention_bit, 2, 1)
PROBE_EXPORT(replay_half_bits, 1, 1)
PROBE_EXPORT(replay_feistel, 4, 1)
PROBE_EXPORT(replay_perm, 4, 1)
PROBE_EXPORT(replay_append_plan, 5, 1)
PROBE_EXPORT(replay_append_slot, 3, 1)
PROBE_EXPORT(prio_key, 2, 1)
PROBE_EXPORT(prio_partition, 2, 1)
PROBE_EXPORT(prio_weight, 3, 1)
PROBE_EXPORT(prio_update_bits, 3, 1)
PROBE_EXPORT(prio_update_slot, 3, 1)

// k[0] = bsz (strata per row, >= 1), k[1] = rows of the table; n <= rows * bsz
extern "C" int pve_probe_prio_draw_rank(const pve_config *cfg, const pve_probe_args *a)
{
    const int bad = check(cfg, a, 4, 1);
    if (bad) return bad;
    if (a->k[0] < 1 || a->k[1] < 1 || a->n > (long long)a->k[0] * a->k[1]) return PROBE_E_ARGS;
    return run<Const, B_prio_draw_rank>(make_const(*cfg), *a);
}

extern "C" int pve_probe_is_device(void) { return PVE_DEVICE_CODE; }

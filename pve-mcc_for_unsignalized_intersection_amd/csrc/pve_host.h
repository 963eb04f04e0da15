// pve_host.h -- backend-independent host side of the C ABI (handle, constants, layout).
// Included by pve_hip.hip (product, HIP backend) and by the CPU test emulators (tests/emu, tests/emu_wide).
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <type_traits>

#include "../../include/pve_env.h"
#include "../../include/pve_env_arrivals.h"
#include "../../include/pve_env_stats.h"
#include "../../include/pve_env_debug.h"
#include "pve_types.h"
#include "pve_nstep.h"
#include "pve_replay.h"
#include "pve_prio.h"
#include "pve_arrivals.h"
#include "pve_stats.h"
#include "pve_learn.h"

namespace pve {

// the replay memory stores the n-step pass's records, and its state block is the public one
static_assert(REPLAY_REC == NSTEP_REC && REPLAY_REC == PVE_NSTEP_RECORD, "pve_replay.h and pve_nstep.h / pve_env.h disagree on the record");
static_assert(REPLAY_STATE_WORDS == PVE_REPLAY_STATE_WORDS, "pve_replay.h and pve_env.h disagree on the state block");
static_assert(sizeof(long long) == sizeof(int64_t), "the state block is int64");
// the specification headers are also built alone and do not read the public ones: their constants are held to them here
static_assert(STAT_N == PVE_STAT_N && STAT_MAX_GROUPS == PVE_STAT_MAX_GROUPS && STAT_N_METRICS == PVE_N_METRICS &&
              (int)STAT_ENV_TICKS == PVE_STAT_ENV_TICKS && (int)STAT_ALIVE == PVE_STAT_ALIVE && (int)STAT_SPAWNED == PVE_STAT_SPAWNED &&
              (int)STAT_FINISHED == PVE_STAT_FINISHED && (int)STAT_DELETED == PVE_STAT_DELETED && (int)STAT_COLLISIONS == PVE_STAT_COLLISIONS &&
              (int)STAT_LOCK == PVE_STAT_LOCK && (int)STAT_CTL == PVE_STAT_CTL && (int)STAT_COLLIDED == PVE_STAT_COLLIDED &&
              (int)STAT_DONE == PVE_STAT_DONE && (int)STAT_SUM_REWARD == PVE_STAT_SUM_REWARD &&
              (int)STAT_SUM_REWARD_SQ == PVE_STAT_SUM_REWARD_SQ && (int)STAT_SUM_V == PVE_STAT_SUM_V && (int)STAT_SUM_A == PVE_STAT_SUM_A &&
              STAT_F_CTL == PVE_F_CTL && STAT_F_DONE == PVE_F_DONE, "pve_stats.h and the public headers disagree on the columns");
static_assert(((STAT_EO_OF_COLUMN >> 0) & 7) == PVE_EO_N_PRE && ((STAT_EO_OF_COLUMN >> 4) & 7) == PVE_EO_N_SPAWNED &&
              ((STAT_EO_OF_COLUMN >> 8) & 7) == PVE_EO_N_FINISHED && ((STAT_EO_OF_COLUMN >> 12) & 7) == PVE_EO_N_DELETED &&
              ((STAT_EO_OF_COLUMN >> 16) & 7) == PVE_EO_COLLISIONS && ((STAT_EO_OF_COLUMN >> 20) & 7) == PVE_EO_LOCK,
              "pve_stats.h and pve_env.h disagree on env_out");
static_assert(LEARN_SLICE == PVE_LEARN_SLICE && LW_ROW == PVE_LEARNER_WIDE_ROW && LW_ROW % 4 == 0 &&
              PVE_LEARNER_WIDE_FLOATS(1) == LW_ROW && PVE_LEARNER_WIDE_FLOATS(128) == LW_ROW && PVE_LEARNER_WIDE_FLOATS(129) == 2 * LW_ROW,
              "the wide step's workspace (include/pve_env.h PVE_LEARNER_WIDE_*)");
static_assert(LB_ACTOR == PVE_LEARNER_ACTOR && LB_CRITIC == PVE_LEARNER_CRITIC && LB_TACTOR == PVE_LEARNER_TARGET_ACTOR &&
              LB_TCRITIC == PVE_LEARNER_TARGET_CRITIC && LB_M_ACTOR == PVE_LEARNER_M_ACTOR && LB_V_ACTOR == PVE_LEARNER_V_ACTOR &&
              LB_M_CRITIC == PVE_LEARNER_M_CRITIC && LB_V_CRITIC == PVE_LEARNER_V_CRITIC && LB_POWERS == PVE_LEARNER_POWERS &&
              LB_STEPS == PVE_LEARNER_STEPS && LB_GRAD == PVE_LEARNER_GRAD && LB_TOTAL == PVE_LEARNER_N_FLOATS &&
              LRN_ACTOR_W == PVE_ACTOR_N_WEIGHTS && LRN_CRITIC_W == PVE_CRITIC_N_WEIGHTS && LEARN_CRITIC_ONLY == PVE_LEARN_CRITIC_ONLY,
              "the learner's block layout (include/pve_env.h PVE_LEARNER_*)");

// Geometry and limits exactly as the reference constructor derives them
// (ref traffic_interaction_scene.py:21-45, :148-152, :153-166, :182-186; libm = CPython's math).
inline Const make_const(const pve_config &cfg)
{
    Const c;
    memset(&c, 0, sizeof(c));
    const double cw = cfg.lane_cw, dc = cfg.dis_ctl;
    c.deltaT = cfg.deltaT; c.dt2 = pow(cfg.deltaT, 2);
    c.vm = cfg.vm; c.vM = cfg.vM; c.am = cfg.am; c.aM = cfg.aM; c.v0 = cfg.v0;
    c.abs_am = fabs(cfg.am); c.two_abs_am = 2 * fabs(cfg.am);
    c.inv_abs_am = 1.0 / c.abs_am; c.inv_two_abs_am = 1.0 / c.two_abs_am;
    c.aM_minus_am = cfg.aM - cfg.am;
    c.inv_dt = 1.0 / cfg.deltaT; c.inv_span = 1.0 / (cfg.aM - cfg.am);
    c.collision_thr = cfg.collision_thr; c.lock_mean_thr = cfg.collision_thr + 3;
    c.exit_p = -dc + (double)((NL + 1) / 2) * cw;
    c.cw = cw;
    const double approach = dc - 6 * cw;
    c.inbox[0] = 3.1415 / 2 * 7 * cw; c.inbox[1] = 12 * cw; c.inbox[2] = 3.1415 / 2 * cw;
    for (int m = 0; m < 3; m++) c.spawn_p[m] = 0 + approach + c.inbox[m];
    const double pi = 3.141592653589793;
    const double cita = (2 * sqrt(10.0) - 6) * cw;
    const double alpha = atan((6 * cw + cita) / (3 * cw));
    const double beta = pi / 2 - alpha;
    const double gama = atan((sqrt(13.0) * cw) / (6 * cw));
    const double _gama = pi / 2 - gama;
    // ego = left turn (ref :771-799): delta = p1 - A + B, vd = C + delta
    c.vdA[0][0] = 6 * cw;          c.vdB[0][0] = cita;  c.vdC[0][0] = alpha * 7 * cw;
    c.vdA[0][1] = gama * 7 * cw;   c.vdB[0][1] = 0;     c.vdC[0][1] = _gama * 7 * cw;
    c.vdA[0][2] = _gama * 7 * cw;  c.vdB[0][2] = 0;     c.vdC[0][2] = gama * 7 * cw;
    c.vdA[0][3] = 6 * cw;          c.vdB[0][3] = -cita; c.vdC[0][3] = beta * 7 * cw;
    // ego = straight (ref :733-766)
    c.vdA[1][0] = 3 * cw;          c.vdB[1][0] = 0;     c.vdC[1][0] = 9 * cw;
    c.vdA[1][1] = beta * 7 * cw;   c.vdB[1][1] = 0;     c.vdC[1][1] = 6 * cw + cita;
    c.vdA[1][2] = alpha * 7 * cw;  c.vdB[1][2] = 0;     c.vdC[1][2] = 6 * cw - cita;
    c.vdA[1][3] = 9 * cw;          c.vdB[1][3] = 0;     c.vdC[1][3] = 3 * cw;
    for (int k = 0; k < 4; k++) {
        double ang = 3.141593 / 2 * (double)k;            // ref :1251
        c.rot_cos[k] = cos(ang); c.rot_sin[k] = sin(ang);
    }
    c.arc_k = 3.141593;
    static const int8_t l2l[NL][4] = {
        {10, 3, 9, 7}, {10, 6, 3, 4}, {-1, -1, -1, -1},
        {1, 6, 0, 10}, {1, 9, 6, 7},  {-1, -1, -1, -1},
        {4, 9, 3, 1},  {4, 0, 9, 10}, {-1, -1, -1, -1},
        {7, 0, 6, 4},  {7, 3, 0, 1},  {-1, -1, -1, -1}};
    for (int i = 0; i < NL; i++)
        for (int k = 0; k < 4; k++) c.l2l[i][k] = l2l[i][k];
    for (int i = 0; i < NL; i++)
        for (int k = 0; k < 4; k++) {
            c.l2l_inv[i][k] = -1;
            int o = l2l[i][k];
            if (o < 0) continue;
            for (int q = 0; q < 4; q++) if (l2l[o][q] == i) c.l2l_inv[i][k] = (int8_t)q;
        }
    return c;
}

// General geometry: constructor tables of the 4- / 8-lane branches (ref :66-145), get_virtual_distance as a table
// (ref :453-660), get_p as canonical path + quarter turns (ref :896-1249).  lane_num = 12 re-expresses make_const's
// tables in the same form (used to cross-check the general kernel against the fast path).
inline GeoConst make_geo_const(const pve_config &cfg)
{
    GeoConst g;
    memset(&g, 0, sizeof(g));
    g.base = make_const(cfg);
    Const &c = g.base;
    const int LN = cfg.lane_num;
    const double cw = cfg.lane_cw, dc = cfg.dis_ctl;
    g.lane_num = LN;
    memset(g.l2l, -1, sizeof(g.l2l));
    memset(g.direction, -1, sizeof(g.direction));
    memset(g.tab.dir_lane, 0, sizeof(g.tab.dir_lane));
    auto set = [&](int ty, int k, double A, double B, double C, double C2) {
        g.tab.vd[ty][k][0] = A; g.tab.vd[ty][k][1] = B; g.tab.vd[ty][k][2] = C; g.tab.vd[ty][k][3] = C2;
    };
    if (LN == 4) {
        g.dir_num = 12; g.tmod = 3; g.RL = 3; g.H = 2 * cw;
        const double approach = dc - 2 * cw;                                     // ref :69-71
        c.inbox[0] = 3.1415 / 2 * 3 * cw; c.inbox[1] = 4 * cw; c.inbox[2] = 3.1415 / 2 * cw;
        for (int m = 0; m < 3; m++) c.spawn_p[m] = 0 + approach + c.inbox[m];
        static const int8_t l2l[12][7] = {                                       // ref :74-87
            {10, 6, 9, 3, 7, 4, 8}, {10, 6, 3, 4, 9, 5, -1}, {6, 10, -1, -1, -1, -1, -1},
            {1, 9, 0, 6, 10, 7, 11}, {1, 9, 6, 7, 0, 8, -1}, {9, 1, -1, -1, -1, -1, -1},
            {4, 0, 3, 9, 1, 10, 2},  {4, 0, 9, 10, 3, 11, -1}, {0, 4, -1, -1, -1, -1, -1},
            {7, 3, 6, 0, 4, 1, 5},   {7, 3, 0, 1, 6, 2, -1},  {3, 7, -1, -1, -1, -1, -1}};
        for (int d = 0; d < 12; d++) for (int k = 0; k < 7; k++) g.l2l[d][k] = l2l[d][k];
        static const int8_t dir[4][3] = {{6, 7, 8}, {0, 1, 2}, {9, 10, 11}, {3, 4, 5}};   // ref :88-93
        for (int i = 0; i < 4; i++) for (int k = 0; k < 3; k++) g.direction[i][k] = dir[i][k];
        static const int8_t turn[4] = {0, 2, 1, 3};                              // ref :897, :939, :981, :1022
        for (int i = 0; i < 4; i++) g.turn[i] = turn[i];
        const double alpha = atan((4 - sqrt(2.0)) / (4 + sqrt(2.0)));            // ref :94-98
        const double _alpha = atan((4 + sqrt(2.0)) / (4 - sqrt(2.0)));
        const double beta = atan(2 / sqrt(5.0)), _beta = atan(sqrt(5.0) / 2);
        const double gama = atan(1.0 / 2 * sqrt(2.0));
        const double half = 0.5 * 3.1415, q = 1.5 * 3.1415 * cw, cg = cos(gama);
        auto F = [&](double x) { return (q * x) / half; };                       // 1.5*3.1415*cw*x/(0.5*3.1415)
        auto G = [&](double x) { return q * (x / half); };                       // (1.5*3.1415)*cw*(x/(0.5*3.1415))
        set(0, 0, 4 * cw - 3 * cw * cg, 0, 3 * cw * (0.5 * 3.1415 - gama), 0);   // ref :455-459
        set(0, 1, G(_alpha), 0, G(alpha), 0);                                    // ref :476-480
        set(0, 2, F(beta), 0, F(_beta), 0);                                      // ref :466-470
        set(0, 3, F(_beta), 0, F(beta), 0);                                      // ref :471-475
        set(0, 4, 3 * cw * cg, 0, G(gama), 0);                                   // ref :481-485
        set(1, 0, cw, 0, 3 * cw, 0);                                             // ref :497-516
        set(1, 1, F(gama), 0, 3 * cw * cg, 0);
        set(1, 2, F(0.5 * 3.1415 - gama), 0, 4 * cw - 3 * cw * cg, 0);
        set(1, 3, 3 * cw, 0, cw, 0);
        g.fix_d = (_alpha - alpha) * 3 * cw;                                     // ref :1304
        g.fix_hi = _alpha * 3 * cw; g.fix_lo = alpha * 3 * cw;                   // ref :1309, :1316
    } else if (LN == 8) {
        g.dir_num = 16; g.tmod = 4; g.RL = 5; g.H = 4 * cw;
        const double approach = dc - 4 * cw;                                     // ref :103-105
        c.inbox[0] = 3.1415 / 2 * 5 * cw; c.inbox[1] = 8 * cw; c.inbox[2] = 3.1415 / 2 * cw;
        for (int m = 0; m < 3; m++) c.spawn_p[m] = 0 + approach + c.inbox[m];
        static const int8_t l2l[16][7] = {                                       // ref :107-124
            {14, 4, 13, 12, 9, 10, 5}, {14, 13, 8, 4, 5, 6, 12}, {14, 13, 8, 4, 5, 6, 7}, {14, -1, -1, -1, -1, -1, -1},
            {2, 8, 1, 0, 13, 14, 9},   {2, 1, 12, 8, 9, 10, 0},  {2, 1, 12, 8, 9, 10, 11}, {2, -1, -1, -1, -1, -1, -1},
            {6, 12, 5, 4, 1, 2, 13},   {6, 5, 0, 12, 13, 14, 4}, {6, 5, 0, 12, 13, 14, 15}, {6, -1, -1, -1, -1, -1, -1},
            {10, 0, 9, 8, 5, 6, 1},    {10, 9, 4, 0, 1, 2, 8},   {10, 9, 4, 0, 1, 2, 3},   {10, -1, -1, -1, -1, -1, -1}};
        for (int d = 0; d < 16; d++) for (int k = 0; k < 7; k++) g.l2l[d][k] = l2l[d][k];
        static const int8_t dir[8][3] = {{0, 1, -1}, {-1, 2, 3}, {4, 5, -1}, {-1, 6, 7},
                                         {8, 9, -1}, {-1, 10, 11}, {12, 13, -1}, {-1, 14, 15}};   // ref :135-144
        for (int i = 0; i < 8; i++) for (int k = 0; k < 3; k++) g.direction[i][k] = dir[i][k];
        static const int8_t turn[4] = {2, 3, 0, 1};                              // lane pairs, ref :1062-1249
        for (int i = 0; i < 8; i++) g.turn[i] = turn[i / 2];
        const double s24 = sqrt(24.0);
        set(0, 0, 8 * cw - s24 * cw, 0, atan(s24) * 5 * cw, 0);                  // ref :540-575
        set(0, 1, atan(3.0 / 4) * 5 * cw, 0, atan(4.0 / 3) * 5 * cw, 0);
        set(0, 2, 4 * cw, 0, atan(4.0 / 3) * 5 * cw, 0);
        set(0, 3, atan(4.0 / 3) * 5 * cw, 0, atan(3.0 / 4) * 5 * cw, 0);
        set(0, 4, 4 * cw, 0, atan(3.0 / 4) * 5 * cw, 0);
        set(0, 5, s24 * cw, 0, atan(1 / s24) * 5 * cw, 0);
        set(1, 0, 3 * cw, 0, 7 * cw, 0);                                         // ref :578-613
        set(1, 1, 3 * cw, 0, 5 * cw, 0);
        set(1, 2, atan(3.0 / 4) * 5 * cw, 0, 4 * cw, 0);
        set(1, 3, atan(4.0 / 3) * 5 * cw, 0, 4 * cw, 0);
        set(1, 4, 5 * cw, 0, 3 * cw, 0);
        set(1, 5, 5 * cw, 0, cw, 0);
        set(2, 0, cw, 0, 7 * cw, 0);                                             // ref :615-652
        set(2, 1, cw, 0, 5 * cw, 0);
        set(2, 2, atan(1 / s24) * 5 * cw, 0, s24 * cw, 0);
        set(2, 3, atan(s24) * 5 * cw, 0, 8 * cw, s24 * cw);                      // abs(d) + 8cw - sqrt(24)cw, ref :634
        set(2, 4, 7 * cw, 0, 3 * cw, 0);
        set(2, 5, 7 * cw, 0, cw, 0);
    } else {
        g.dir_num = 12; g.tmod = 3; g.RL = 7; g.H = 6 * cw;
        for (int d = 0; d < 12; d++) for (int k = 0; k < 4; k++) g.l2l[d][k] = c.l2l[d][k];
        for (int i = 0; i < 12; i++) g.direction[i][i % 3] = (int8_t)i;          // ref :168-181
        for (int m = 0; m < 2; m++) for (int k = 0; k < 4; k++) set(m, k, c.vdA[m][k], c.vdB[m][k], c.vdC[m][k], 0);
    }
    c.exit_p = -dc + (double)((LN + 1) / 2) * cw;                                // ref :341-342
    for (int i = 0; i < LN; i++)
        for (int m = 0; m < 3; m++)
            if (g.direction[i][m] >= 0) { g.tab.dir_lane[g.direction[i][m]] = (int8_t)i; g.tab.dir_index[g.direction[i][m]] = (int8_t)m; }
    // membership tables of the virtual-lane lists (ref :240-270): which routes can appear in list d, and where
    memset(g.tab.pos, -1, sizeof(g.tab.pos));
    memset(g.tab.mroutes, 0, sizeof(g.tab.mroutes));
    memset(g.tab.lroutes, 0, sizeof(g.tab.lroutes));
    for (int d = 0; d < ND; d++) {
        g.tab.opp[d] = g.l2l[d][1];
        if (d >= g.dir_num) continue;
        for (int q = 0; q < MAXK; q++) if (g.l2l[d][q] >= 0) g.tab.pos[d][g.l2l[d][q]] = (int8_t)q;
        unsigned mr = 0;
        const int li = g.tab.dir_lane[d];
        for (int q = 0; q < 3; q++) if (g.direction[li][q] >= 0) mr |= 1u << g.direction[li][q];
        for (int q = 0; q < MAXK; q++) if (g.l2l[d][q] >= 0) mr |= 1u << g.l2l[d][q];
        g.tab.mroutes[d] = (uint16_t)mr;
    }
    for (int d = 0; d < g.dir_num; d++)
        for (int rt = 0; rt < ND; rt++) if ((g.tab.mroutes[d] >> rt) & 1u) g.tab.lroutes[rt] |= (uint16_t)(1u << d);
    memset(g.tab.lst, 0, sizeof(g.tab.lst));
    for (int rt = 0; rt < ND; rt++) {
        int n = 0;
        for (int d = 0; d < g.dir_num; d++) if ((g.tab.lroutes[rt] >> d) & 1u) g.tab.lst[rt][n++] = (int8_t)d;
        g.tab.nl[rt] = (int8_t)n;
        g.tab.ninv[rt] = (uint16_t)(n ? (32768 + n - 1) / n : 0);
    }
    for (int d = 0; d < ND; d++) g.tab.dty[d] = (int8_t)(d % g.tmod);
    for (int m = 0; m < 3; m++) g.tab.inbox[m] = c.inbox[m];
    g.turn_pk = 0; g.dir_pk[0] = g.dir_pk[1] = g.dir_pk[2] = 0;
    for (int i = 0; i < NL; i++) {
        g.turn_pk |= (unsigned long long)(g.turn[i] & 15) << (4 * i);
        for (int m = 0; m < 3; m++) g.dir_pk[m] |= (unsigned long long)((g.direction[i][m] + 1) & 31) << (5 * i);
    }
    return g;
}

inline std::string &last_error_ref()
{
    static thread_local std::string e;
    return e;
}
inline int fail(int code, const std::string &msg)
{
    last_error_ref() = msg;
    return code;
}

// What a stepping call launched (pve_debug_last_variant, include/pve_env_debug.h).  A backend notes every tick / roll-out launch
// WHERE IT LAUNCHES (note_launch: the template arguments of the kernel, not what a picker intended); pve_capi.inc clears the note in
// front of a stepping call and copies it into the handle behind it.  Per thread, like the error text: calls on one handle are not
// concurrent.
inline pve_launch_variant &launch_note()
{
    static thread_local pve_launch_variant v;
    return v;
}
inline void note_launch(bool geo, int family, int cap, int waves_per_simd, bool prof, bool actor, bool train, bool table, bool pers,
                        long long grid)
{
    pve_launch_variant &v = launch_note();
    const int32_t n = v.launches + 1;
    memset(&v, 0, sizeof(v));
    v.family = family; v.capacity = cap; v.waves_per_simd = waves_per_simd;
    v.prof = prof; v.actor = actor; v.train = train; v.table = table; v.persistent = pers; v.geo = geo;
    v.grid = (int32_t)(grid > 0x7fffffffLL ? 0x7fffffffLL : grid);
    v.launches = n;
}

// THE OPTIONAL PART OF THE BACKEND CONTRACT (the mandatory part: the comment at the head of pve_capi.inc).  A backend derives from
// BackendDefaults and overrides, group by group, the launchers it has kernels for; what it leaves alone refuses, and the entry
// points of that group validate their arguments and then answer "this backend has no ... kernels" (Provides, below).
struct BackendDefaults {
    static constexpr int max_capacity = 128;   // the largest capacity it runs: 256 slots exist for the 12-lane fast path only
    // all three or none: launch_actor / launch_rollout / launch_rollout_geo + the exploration noise of pve_set_action_noise
    // (ActionNoise::tick0 = first tick; ids = the [n_envs][cap] id field).  A backend with them needs no launch_rollout[_geo].
    static int launch_actor_noisy(const float *, const unsigned char *, const void *, int, const int32_t *, const int32_t *,
                                  const ActionNoise &, double *, int, int, void *, std::string &) { return -1; }
    static int launch_rollout_noisy(const Const &, const Params &, const RolloutArgs &, const ActionNoise &, int, void *, std::string &) { return -1; }
    static int launch_rollout_geo_noisy(const GeoConst &, const Params &, const RolloutArgs &, const ActionNoise &, int, void *,
                                        std::string &) { return -1; }
    // all three or none: pve_set_target_networks / pve_critic_forward / pve_bootstrap_q (csrc/pve_critic.h; a NULL weight pointer
    // of pack_target_networks = keep that image)
    static int pack_target_networks(const float *, float *, unsigned char *, const float *, float *, unsigned char *, void *,
                                    std::string &) { return -1; }
    static int launch_critic(const unsigned char *, const void *, int, const float *, float *, long long, void *, std::string &) { return -1; }
    static int launch_bootstrap_q(const unsigned char *, const unsigned char *, const void *, int, const int32_t *, float *, float *,
                                  long long, void *, std::string &) { return -1; }
    // both or none: pve_nstep_scan / pve_nstep_gather (csrc/pve_nstep.h)
    static int launch_nstep_scan(const NstepArgs &, int, void *, std::string &) { return -1; }
    static int launch_nstep_gather(const NstepArgs &, void *, std::string &) { return -1; }
    // both or none: pve_replay_reset / _append / _sample (csrc/pve_replay.h)
    static int launch_replay_append(const ReplayArgs &, const float *, const long long *, long long, int, void *, std::string &) { return -1; }
    static int launch_replay_sample(const ReplayArgs &, long long, long long, float *, float *, float *, long long *, int, void *,
                                    std::string &) { return -1; }
    // all four or none: pve_prio_reset / _rank / _sample / _update (csrc/pve_prio.h); launch_prio_sample ranks first
    static int launch_prio_reset(const PrioArgs &, int, void *, std::string &) { return -1; }
    static int launch_prio_rank(const PrioArgs &, int, void *, std::string &) { return -1; }
    static int launch_prio_sample(const PrioArgs &, long long, long long, float, float *, float *, float *, long long *, int32_t *, float *,
                                  int, void *, std::string &) { return -1; }
    static int launch_prio_update(const PrioArgs &, const long long *, const float *, const float *, long long, int, void *,
                                  std::string &) { return -1; }
    // pve_generate_arrivals (csrc/pve_arrivals.h)
    static int launch_generate_arrivals(const ArrivalArgs &, int, void *, std::string &) { return -1; }
    // both or none: pve_rollout_stats / pve_metrics_groups (csrc/pve_stats.h)
    static int launch_rollout_stats(const StatsArgs &, int, void *, std::string &) { return -1; }
    static int launch_metrics_groups(const EnvHeader *, int, int, const int32_t *, int, double *, void *, std::string &) { return -1; }
    // both or none: pve_learner_init / pve_learner_step (csrc/pve_learn.h)
    static int launch_learner_init(float *, const float *, const float *, const float *, const float *, float, float, void *,
                                   std::string &) { return -1; }
    static int launch_learner_step(const LearnCtx &, int, void *, std::string &) { return -1; }
    // pve_learner_step_wide (learn_steps_wide)
    static int launch_learner_step_wide(const LearnCtx &, float *, int, int, void *, std::string &) { return -1; }
};

// Does backend B provide an optional group: it overrides every launcher of it.  (An override with another signature hides the
// default, and the comparison of the two pointer types does not compile.)
#define PVE_OVERRIDES(f_) (&B::f_ != &BackendDefaults::f_)
template <class B> struct Provides {
    static constexpr bool noise = PVE_OVERRIDES(launch_actor_noisy) && PVE_OVERRIDES(launch_rollout_noisy) && PVE_OVERRIDES(launch_rollout_geo_noisy);
    static constexpr bool target_q = PVE_OVERRIDES(pack_target_networks) && PVE_OVERRIDES(launch_critic) && PVE_OVERRIDES(launch_bootstrap_q);
    static constexpr bool nstep = PVE_OVERRIDES(launch_nstep_scan) && PVE_OVERRIDES(launch_nstep_gather);
    static constexpr bool replay = PVE_OVERRIDES(launch_replay_append) && PVE_OVERRIDES(launch_replay_sample);
    static constexpr bool prio = PVE_OVERRIDES(launch_prio_reset) && PVE_OVERRIDES(launch_prio_rank) && PVE_OVERRIDES(launch_prio_sample) &&
                                 PVE_OVERRIDES(launch_prio_update);
    static constexpr bool arrivals = PVE_OVERRIDES(launch_generate_arrivals);
    static constexpr bool stats = PVE_OVERRIDES(launch_rollout_stats) && PVE_OVERRIDES(launch_metrics_groups);
    static constexpr bool learner = PVE_OVERRIDES(launch_learner_init) && PVE_OVERRIDES(launch_learner_step);
    static constexpr bool learner_wide = PVE_OVERRIDES(launch_learner_step_wide);
};
#undef PVE_OVERRIDES

// How pve_capi.inc reaches the optional part: through the backend itself where it derives from BackendDefaults.  A Backend that
// does not (an emulator source older than BackendDefaults, built against this directory) has none of the optional launchers: it
// gets the defaults beside it and keeps a max_capacity of its own where it declares one.  Nothing here knows a feature.
template <class B, class = void> struct OwnCapacity { static constexpr int value = BackendDefaults::max_capacity; };
template <class B> struct OwnCapacity<B, decltype((void)B::max_capacity)> { static constexpr int value = B::max_capacity; };
template <class B> struct BesideDefaults : BackendDefaults, B { static constexpr int max_capacity = OwnCapacity<B>::value; };
template <class B> using Contract = std::conditional_t<std::is_base_of<BackendDefaults, B>::value, B, BesideDefaults<B>>;

}  // namespace pve

struct pve_handle_s {
    pve::Const c;
    pve::GeoConst g;                  // general-geometry path (lane_num 4 / 8, or 12 with PVE_CFG_GENERAL_PATH)
    bool geo;
    int lane_num;
    const int32_t *choice;
    long long choice_stride;
    int choice_rows;
    pve_config cfg;
    int n_envs, cap, device;
    pve::Layout L;
    char *ws;
    bool own_ws;
    const double *arrivals;
    int rows;
    long long arr_stride;
    void *stream;
    bool has_arrivals, is_reset;
    long long ticks_since_reset;
    unsigned long long *phase_cycles;
    bool has_actor;                   // pve_set_actor installed an actor in the workspace
    int stop_phase;                   // pve_debug_stop_phase (diagnostics), -1 = off
    unsigned q_done_base;             // persistent roll-out: items completed per intersection since pve_reset (cumulative)
    int last_launch_kind;             // PVE_LAUNCH_*: what the last stepping call launched (pve_debug_last_launch)
    pve_launch_variant last_variant;  // ... and which kernel variant, as the backend noted it at the launch (pve_debug_last_variant)
    bool has_tactor, has_critic;      // pve_set_target_networks installed a target actor / a critic in the workspace
    pve::ActionNoise noise;           // pve_set_action_noise (sigma = 0: off); tick0 is filled in per launch
};

/* pve_env_debug.h -- extension of the C ABI of pve_env.h (libpveenv.so, ABI 9): which kernel variant the last stepping call
 * launched.  pve_debug_last_launch (pve_env.h) tells the launch FORM -- one launch per tick, one per chunk, one for the call; the
 * library holds several kernels behind each form (the register build and the HOME build of the 128-slot queue kernel, the
 * phase-cycle diagnostics builds, the table / actor / training-output variants, the 4- / 8-lane kernels), and this call names
 * the one that ran.  A library older than this header lacks the symbol. */
#ifndef PVE_ENV_DEBUG_H
#define PVE_ENV_DEBUG_H

#include "pve_env.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The record is written where the launch happens, from the template arguments of the kernel that was launched -- not from what
 * the selection rules intended.  It describes the LAST tick or roll-out kernel launch of the last stepping call (pve_step_all,
 * pve_scene_update, pve_step_all_actor, pve_step_many) on the handle; every launch of one call has the same variant except `grid`
 * of a shorter last chunk.  All zero (kind = PVE_LAUNCH_NONE) before the first call, after a call of zero ticks and after a
 * stepping call whose launch failed or was refused (a call rejected for its arguments leaves the record as it was). */
typedef struct pve_launch_variant {
    int32_t kind;             /* PVE_LAUNCH_*: what pve_debug_last_launch returns */
    int32_t family;           /* lanes of the layout the kernel serves: 12, or 4 / 8 */
    int32_t capacity;         /* slots per intersection of the kernel: 64, 128 or 256 */
    int32_t waves_per_simd;   /* roll-out kernels: the occupancy the kernel is built for -- 4 = the register build, 5 = the HOME build
                                 of the 128-slot queue kernel (or the knob-only wide 8-lane build); 0 for per-tick launches and for
                                 a backend without waves */
    int32_t prof;             /* 1 = a phase-cycle diagnostics build (roll-out), or a tick launched with pve_debug_phase_cycles armed */
    int32_t actor;            /* 1 = the actor runs inside the roll-out kernel (0 for per-tick launches: the actor is a launch of its own) */
    int32_t train;            /* 1 = the roll-out kernel with the training outputs obs_pre / state_pre; per-tick: they were requested */
    int32_t table;            /* 1 = the roll-out kernel that gathers PVE_SRC_TABLE actions by vehicle id */
    int32_t persistent;       /* 1 = the queue form of the roll-out kernel */
    int32_t geo;              /* 1 = the general-geometry kernels (lane_num 4 / 8, or 12 with PVE_CFG_GENERAL_PATH) */
    int32_t grid;             /* workgroups of the last launch (0: a backend without workgroups) */
    int32_t launches;         /* launches the call enqueued: tick and roll-out kernels, plus the actor passes between per-tick launches */
    int32_t reserved[4];      /* 0 */
} pve_launch_variant;

/* Host only: waits for nothing, launches nothing.  Errors (PVE_ERR_INVALID): null handle or out. */
int pve_debug_last_variant(pve_handle h, pve_launch_variant *out);

#ifdef __cplusplus
}
#endif
#endif /* PVE_ENV_DEBUG_H */

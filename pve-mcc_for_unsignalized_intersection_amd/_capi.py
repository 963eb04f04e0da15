"""ctypes binding of libpveenv.so (include/pve_env.h).

The library is the hand-written HIP implementation; there is NO CPU fallback: if the shared
object is missing or no AMD GPU is visible the calls fail loudly (PveError).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libpveenv.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)

DIR_NUM = {4: 12, 8: 16, 12: 12}     # virtual-lane lists per layout (ref :86, :132, :167)
# Every integer macro and enumerator of include/*.h, once: an upper-case integer here is the header's name with or without its
# PVE_ prefix, and position k of a name tuple is the enumerator PVE_EO_<NAME> / PVE_M_<NAME> / PVE_LAUNCH_<NAME> (and
# PVE_STAT_<NAME>: stats.STAT_NAMES) of value k.  tests/test_binding_contract.py holds both directions to the headers.
ABI_VERSION = 9
PVE_OK, PVE_ERR_INVALID, PVE_ERR_NO_DEVICE, PVE_ERR_STATE, PVE_ERR_NOMEM = 0, -1, -2, -3, -4
PVE_LANES, PVE_MAX_DIRS, PVE_OBS_WIDTH, PVE_NBR, PVE_STATE_ROWS, PVE_N_METRICS, PVE_ENV_OUT_N = 12, 16, 28, 6, 7, 12, 8
CFG_GENERAL_PATH, CFG_OBS_F32, CFG_GEO_SCAN, CFG_ACTOR_F32 = 0x1, 0x2, 0x4, 0x8
PVE_ACTOR_N_WEIGHTS, PVE_CRITIC_N_WEIGHTS = 6393, 6841
NSTEP_TAIL, NSTEP_MAX_WINDOW, NSTEP_RECORD = 0x1, 16, 36
REPLAY_STATE_WORDS = 4
PRIO_STATE_WORDS, PRIO_PARTS = 4, 32
# float offsets of the learner block's segments (pve_mcc_amd/learner.py)
LEARNER_ACTOR, LEARNER_CRITIC, LEARNER_TARGET_ACTOR, LEARNER_TARGET_CRITIC = 0, 6396, 13240, 19636
LEARNER_M_ACTOR, LEARNER_V_ACTOR, LEARNER_M_CRITIC, LEARNER_V_CRITIC = 26480, 32876, 39272, 46116
LEARNER_POWERS, LEARNER_STEPS, LEARNER_GRAD, LEARNER_N_FLOATS = 52960, 52964, 52968, 66208
LEARN_CRITIC_ONLY, LEARN_SLICE, LEARNER_WIDE_ROW = 0x1, 128, 13244
SRC_ZERO, SRC_POOL, SRC_ACTOR, SRC_TABLE = 0, 1, 2, 3
PVE_STAT_N, PVE_STAT_MAX_GROUPS = 14, 1024
LAUNCH_NONE, LAUNCH_TICK, LAUNCH_RESIDENT, LAUNCH_PERSISTENT = 0, 1, 2, 3      # pve_debug_last_launch
LAUNCH_NAMES = ("none", "tick", "resident", "persistent")                      # ... as batched.last_launch() reports them

F_ALIVE, F_CTL, F_DONE, F_DELETED, F_FINISHED, F_LOCK = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
F_INTENT_SHIFT = 6
META_CONTROL, META_FINISH, META_DONE, META_LOCK = 0x1, 0x2, 0x4, 0x8
METRIC_NAMES = ("slot_steps", "alive_steps", "ctl_steps", "spawned", "passed", "collided", "locks",
                "sum_reward", "sum_jerk", "passed_steps", "overflow", "ticks")
ENV_OUT_NAMES = ("n_pre", "n_ctl", "collisions", "lock", "n_deleted", "n_finished", "n_spawned", "n_post")


class PveError(RuntimeError):
    pass


class PveConfig(C.Structure):
    _fields_ = [("deltaT", C.c_double), ("vm", C.c_double), ("vM", C.c_double), ("am", C.c_double),
                ("aM", C.c_double), ("v0", C.c_double), ("lane_cw", C.c_double), ("dis_ctl", C.c_double),
                ("collision_thr", C.c_double), ("lane_num", C.c_int32), ("flags", C.c_int32)]


class PveOutputs(C.Structure):
    _fields_ = [("obs_post", C.c_void_p), ("obs_pre", C.c_void_p), ("state_pre", C.c_void_p),
                ("obs_prev_post", C.c_void_p), ("reward", C.c_void_p), ("flags", C.c_void_p),
                ("lanej", C.c_void_p), ("nbr", C.c_void_p), ("new_slot", C.c_void_p), ("env_out", C.c_void_p)]


class PveRollout(C.Structure):
    _fields_ = [("n_ticks", C.c_int32), ("source", C.c_int32), ("pool", C.c_void_p), ("n_pool", C.c_int32),
                ("pool_tick0", C.c_int32), ("actor_weights", C.c_void_p), ("actor_obs", C.c_void_p),
                ("actor_actions", C.c_void_p), ("trajectory", C.c_int32), ("table_ids", C.c_int32), ("chunk_ticks", C.c_int32),
                ("persistent", C.c_int32)]


class PveNstepSegment(C.Structure):
    _fields_ = [("n_ticks", C.c_int32), ("obs_post", C.c_void_p), ("state_pre", C.c_void_p), ("reward", C.c_void_p),
                ("flags", C.c_void_p), ("new_slot", C.c_void_p)]


class PveNstep(C.Structure):
    _fields_ = [("gamma", C.c_double), ("window", C.c_int32), ("mode", C.c_int32), ("prev", PveNstepSegment),
                ("cur", PveNstepSegment), ("obs_first", C.c_void_p), ("q_boot", C.c_void_p), ("target", C.c_void_p),
                ("code", C.c_void_p), ("offsets", C.c_void_p), ("total", C.c_void_p), ("max_records", C.c_int64),
                ("records", C.c_void_p), ("index", C.c_void_p), ("block_threads", C.c_int32)]


class PveReplay(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("store", C.c_void_p), ("state", C.c_void_p), ("seed", C.c_uint64),
                ("block_threads", C.c_int32)]


class PvePrio(C.Structure):
    _fields_ = [("replay", PveReplay), ("prio", C.c_void_p), ("pseq", C.c_void_p), ("order", C.c_void_p), ("pstate", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64), ("ends", C.c_void_p), ("ends_host", C.c_void_p),
                ("part_from", C.c_void_p), ("batch", C.c_int64)]


class PveArrivalGen(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("env_offset", C.c_int64), ("epoch", C.c_uint32), ("rows", C.c_int32), ("mean_s", C.c_double),
                ("mean_env", C.c_void_p), ("min_gap_s", C.c_double), ("block_threads", C.c_int32)]


class PveStats(C.Structure):
    _fields_ = [("n_ticks", C.c_int32), ("n_groups", C.c_int32), ("block_threads", C.c_int32), ("reserved", C.c_int32),
                ("group", C.c_void_p), ("flags", C.c_void_p), ("reward", C.c_void_p), ("obs_pre", C.c_void_p), ("env_out", C.c_void_p),
                ("series", C.c_void_p), ("totals", C.c_void_p), ("scratch", C.c_void_p)]


class PveLaunchVariant(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "family", "capacity", "waves_per_simd", "prof", "actor", "train", "table",
                                         "persistent", "geo", "grid", "launches")] + [("reserved", C.c_int32 * 4)]


class PveLearner(C.Structure):
    _fields_ = [("params", C.c_void_p), ("actor_lr", C.c_float), ("critic_lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("epsilon", C.c_float), ("tau", C.c_float), ("flags", C.c_int32), ("block_threads", C.c_int32)]


class PveVehicle(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("p", "v", "a", "jerk", "jerk_sum", "vir_dis", "closer_p")] + \
               [(n, C.c_int32) for n in ("lane", "j", "id", "vnum", "seq_in_lane", "control", "finish", "done",
                                         "collision", "step", "count", "lock", "lock_a")] + \
               [("vir_header", C.c_int32 * 2), ("intention", C.c_int32), ("route", C.c_int32)]


class PveEnvInfo(C.Structure):
    _fields_ = [("current_time", C.c_double), ("n_alive", C.c_int32), ("lane_count", C.c_int32 * 12),
                ("veh_rec", C.c_int32 * 12), ("id_seq", C.c_int32), ("passed_veh", C.c_int32),
                ("passed_veh_step_total", C.c_int32), ("head_valid", C.c_int32 * 16),
                ("head_lane", C.c_int32 * 16), ("head_j", C.c_int32 * 16), ("overflow", C.c_int32),
                ("intention_re", C.c_int32)]


vp, cint, i32, i64, u64, f32, f64 = C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
P = C.POINTER
# THE TABLE of entry points, by the header that declares them: name -> (restype, argtypes).  _declare, load_library's missing-symbol
# check and the EXPORTS* tuples are read from it; tests/test_binding_contract.py holds it (and the structures and constants
# above) to the four headers with the C++ compiler.  A new entry point is one row here.
PROTOTYPES = {
    "pve_env.h": {
        "pve_abi_version": (cint, []),
        "pve_last_error": (C.c_char_p, []),
        "pve_default_config": (None, [P(PveConfig)]),
        "pve_workspace_bytes": (C.c_size_t, [cint, cint]),
        "pve_create": (cint, [P(PveConfig), cint, cint, cint, vp, vp, P(vp)]),
        "pve_destroy": (cint, [vp]),
        "pve_set_stream": (cint, [vp, vp]),
        "pve_set_arrivals": (cint, [vp, vp, cint, cint]),
        "pve_reset": (cint, [vp]),
        "pve_step_all": (cint, [vp, vp, P(PveOutputs)]),
        "pve_scene_update": (cint, [vp, vp, P(PveOutputs)]),
        "pve_compact": (cint, [vp, vp]),
        "pve_read_env": (cint, [vp, cint, P(PveEnvInfo)]),
        "pve_read_vehicles": (cint, [vp, cint, P(PveVehicle), cint, P(cint)]),
        "pve_get_metrics": (cint, [vp, P(f64)]),
        "pve_state_field": (cint, [vp, C.c_char_p, P(vp), P(cint)]),
        "pve_synchronize": (cint, [vp]),
        "pve_debug_phase_cycles": (cint, [vp, vp]),
        "pve_actor_forward": (cint, [vp, vp, vp, vp]),
        "pve_step_all_actor": (cint, [vp, vp, vp, vp, P(PveOutputs)]),
        "pve_debug_traffic_probe": (cint, [vp, vp]),
        "pve_set_intentions": (cint, [vp, vp, cint, cint]),
        "pve_step_many": (cint, [vp, P(PveRollout), P(PveOutputs)]),
        "pve_set_actor": (cint, [vp, vp]),
        "pve_debug_stop_phase": (cint, [vp, cint]),
        "pve_debug_last_launch": (cint, [vp]),
        "pve_debug_item_schedule": (cint, [cint, cint, P(i32)]),
        "pve_set_action_noise": (cint, [vp, f64, u64, i64]),
        "pve_set_target_networks": (cint, [vp, vp, vp]),
        "pve_critic_forward": (cint, [vp, vp, vp, vp, i64]),
        "pve_bootstrap_q": (cint, [vp, vp, vp, vp, vp, i64]),
        "pve_nstep_scan": (cint, [vp, P(PveNstep)]),
        "pve_nstep_gather": (cint, [vp, P(PveNstep)]),
        "pve_replay_reset": (cint, [vp, P(PveReplay)]),
        "pve_replay_append": (cint, [vp, P(PveReplay), vp, vp, i64]),
        "pve_replay_sample": (cint, [vp, P(PveReplay), i64, i64, vp, vp, vp, vp]),
        "pve_learner_init": (cint, [vp, P(PveLearner), vp, vp, vp, vp]),
        "pve_learner_step": (cint, [vp, P(PveLearner), vp, vp, vp, i64, i64, vp, vp]),
        "pve_learner_step_wide": (cint, [vp, P(PveLearner), vp, vp, vp, i64, i64, vp, i64, i32, vp, vp]),
        "pve_prio_scratch_bytes": (C.c_size_t, [i64]),
        "pve_prio_reset": (cint, [vp, P(PvePrio)]),
        "pve_prio_rank": (cint, [vp, P(PvePrio)]),
        "pve_prio_sample": (cint, [vp, P(PvePrio), i64, i64, f32, vp, vp, vp, vp, vp, vp]),
        "pve_prio_update": (cint, [vp, P(PvePrio), vp, vp, vp, i64]),
    },
    # extension headers: entry points added within ABI 9 behind pve_env.h's own
    "pve_env_arrivals.h": {"pve_generate_arrivals": (cint, [vp, P(PveArrivalGen), vp, vp, vp])},
    "pve_env_stats.h": {                           # roll-out and evaluation statistics by group (csrc/pve_stats.h)
        "pve_stats_scratch_bytes": (C.c_size_t, [cint, cint]),
        "pve_rollout_stats": (cint, [vp, P(PveStats)]),
        "pve_metrics_groups": (cint, [vp, vp, cint, vp]),
    },
    # which kernel variant the last stepping call launched
    "pve_env_debug.h": {"pve_debug_last_variant": (cint, [vp, P(PveLaunchVariant)])},
}
EXPORTS, EXPORTS_EXT, EXPORTS_STATS, EXPORTS_DEBUG = (tuple(PROTOTYPES[h]) for h in (
    "pve_env.h", "pve_env_arrivals.h", "pve_env_stats.h", "pve_env_debug.h"))


def _declare(L):
    # (_declare also dresses libraries that load_library has not vetted -- the tests' emulators, which may be builds of sources
    #  older than include/pve_env_debug.h: the diagnostics hook is declared where it exists, and last_variant() says so where not)
    for header, group in PROTOTYPES.items():
        for name, (restype, argtypes) in group.items():
            if header != "pve_env_debug.h" or hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = restype, argtypes
    return L


_cached = None


def load_library(path=None):
    """Load libpveenv.so (built in-tree by __graft_entry__.build() / `make -C csrc`)."""
    global _cached
    if path is None and _cached is not None:
        return _cached
    p = path or os.environ.get("PVE_LIBRARY_PATH") or LIB_PATH   # env override: profiling builds
    if not os.path.isfile(p):
        raise PveError("%s not found: build the HIP library first (python -c 'import __graft_entry__ as g; "
                       "g.build()' or make -C %s/csrc). There is no CPU fallback." % (p, _HERE))
    dll = C.CDLL(p)
    missing = [n for group in PROTOTYPES.values() for n in group if not hasattr(dll, n)]
    if missing:       # (the target-network entry points were added within ABI 9: an older build lacks the symbols)
        raise PveError("%s is an older build: it lacks %s (rebuild it)" % (p, ", ".join(missing)))
    L = _declare(dll)
    if L.pve_abi_version() != ABI_VERSION:
        raise PveError("ABI mismatch: library %d, binding %d" % (L.pve_abi_version(), ABI_VERSION))
    if path is None:
        _cached = L
    return L


def check(L, rc, what=""):
    if rc != 0:
        msg = L.pve_last_error()
        raise PveError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))

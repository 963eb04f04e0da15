"""ctypes wrapper of the CPU oracle (oracle/pve_oracle.c).  TEST INFRASTRUCTURE ONLY.

Allowed importers: tests/, tests/golden/gen_golden.py, __graft_entry__.smoke(),
bench.py's cpu_baseline leg.  The product package must never import this module.
What it shares with oracle/oracle_geo.py lives in oracle/ctypes_env.py.
"""
import ctypes as C
import functools

import numpy as np

from . import ctypes_env
from .ctypes_env import DP, IP, LP, VP


class PvoParams(C.Structure):
    _fields_ = ctypes_env.PARAM_FIELDS


def build(force=False):
    return ctypes_env.build("libpve_oracle.so", force)


def _extras(L, sig):
    sig(VP, [DP, C.c_int, C.POINTER(PvoParams), C.c_int], "create")
    sig(C.c_int, [VP], "peak_alive")
    sig(C.c_int, [VP, IP], "lane_counts")
    sig(C.c_int, [VP, IP, DP, DP], "export_vehicles")
    sig(C.c_int, [VP, C.c_double, C.c_int, DP], "get_p")
    sig(C.c_long, [VP, C.c_int, C.c_int, C.c_double, C.c_int, LP], "run")
    sig(C.c_long, [C.POINTER(VP), IP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, DP, C.c_int, C.c_int, C.c_int, LP], "run_many")


@functools.lru_cache(maxsize=None)
def lib():
    return ctypes_env.load("libpve_oracle.so", "pvo_", PvoParams, _extras)


class OracleEnv(ctypes_env.CtypesEnv):
    """Single environment; same call protocol as the reference object
    (ctor warm-up, step, scene_update, delete_vehicle).
    capacity: the slots of a batched env.  None = unbounded, as the reference.  Otherwise a spawn is deferred when the
    intersection is full: room = capacity - (vehicles alive at tick start) -- this tick's deletions free nothing until the
    next tick -- the lowest due lanes are granted, a deferred lane keeps its cursor, id and everything else and is due
    again on the next tick; `overflow` counts the deferred lanes of every tick."""
    PREFIX, Params = "pvo_", PvoParams
    lane_num = dir_num = 12

    def __init__(self, arrive_time, capacity=None, **params):
        prm = self._params(lib(), params)
        arr = np.ascontiguousarray(arrive_time, dtype=np.float64)
        assert arr.ndim == 2 and arr.shape[1] == 12
        self._arr = arr
        self._h = self._c.create(arr.ctypes.data_as(DP), arr.shape[0], C.byref(prm), 0)
        self._bound(capacity)

    @property
    def peak_alive(self):
        """most vehicles alive at the start of a tick of run() (the slots a capacity-bound build would need)"""
        return self._c.peak_alive(self._h)

    def lane_counts(self):
        out = np.zeros(12, np.int32)
        self._c.lane_counts(self._h, out.ctypes.data_as(IP))
        return out

    def get_p(self, p, lane):
        out = np.zeros(2, np.float64)
        self._c.get_p(self._h, float(p), int(lane), out.ctypes.data_as(DP))
        return out

    def run(self, ticks, policy=0, amp=1.0, tick0=0):
        """Timing loop entirely in C (GIL released by ctypes). -> (alive_steps, ctl_steps)"""
        ctl = C.c_long(0)
        alive = self._c.run(self._h, int(ticks), int(policy), float(amp), int(tick0), C.byref(ctl))
        self.tick_no += ticks
        return int(alive), int(ctl.value)


def run_many(envs, env_index, n_threads, ticks, policy=1, amp=1.0, tick0=0, pool=None):
    """bench.py's cpu_baseline on all host cores: `envs` (OracleEnv objects) dealt to n_threads POSIX threads inside ONE C call
    (pvo_run_many) -- no Python, no GIL in the timed loop.  pool: [n_pool, n_envs_total, cap] float64 (env_index[i] = the row of
    envs[i] in it) for the slot-indexed tape, None for policy 0 (zero) / 1 (a = amp sin(0.37 id + 0.05 tick)).
    -> (alive_steps, ctl_steps)"""
    L = lib()
    hs = (C.c_void_p * len(envs))(*[e._h for e in envs])
    idx = np.ascontiguousarray(env_index, dtype=np.int32)
    ctl = C.c_long(0)
    if pool is not None:
        pool = np.ascontiguousarray(pool, dtype=np.float64)
        pp, n_pool, n_tot, cap = pool.ctypes.data_as(C.POINTER(C.c_double)), pool.shape[0], pool.shape[1], pool.shape[2]
    else:
        pp, n_pool, n_tot, cap = None, 0, 0, 0
    alive = L.pvo_run_many(hs, idx.ctypes.data_as(C.POINTER(C.c_int)), len(envs), int(n_threads), int(ticks), int(policy), float(amp),
                           int(tick0), pp, n_pool, cap, n_tot, C.byref(ctl))
    if alive < 0:
        raise MemoryError("pvo_run_many")
    for e in envs:
        e.tick_no += ticks
    return int(alive), int(ctl.value)

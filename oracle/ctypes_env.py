"""What the ctypes wrappers of the two CPU oracles share (oracle/oracle.py: pvo_*, 12 lanes; oracle/oracle_geo.py: pvg_*,
4 / 8 / 12 lanes): building and declaring a library, and the environment's call protocol.  TEST INFRASTRUCTURE ONLY.

A wrapper module supplies the symbol prefix, its parameter struct, the signatures only its library has, the constructor and
whatever else is its own."""
import ctypes as C
import os
import subprocess

import numpy as np

from .record import VEH_I_COLS, VEH_F_COLS

_HERE = os.path.dirname(os.path.abspath(__file__))
VP, IP, DP, LP = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_long)
PARAM_FIELDS = [(n, C.c_double) for n in ("deltaT", "vm", "vM", "am", "aM", "v0", "lane_cw", "dis_ctl", "collision_thr")]


def build(library, force=False):
    """`make` the library -> its path.  oracle/Makefile names the sources, so whether it is stale is make's question."""
    subprocess.check_call(["make", "-C", _HERE, "-s"] + (["-B"] if force else []) + [library])
    return os.path.join(_HERE, library)


def load(library, prefix, params, extras):
    """The CDLL of `library` with the signatures both oracles have (under `prefix`) and extras(L, sig), where
    sig(restype, argtypes, *names) declares the prefixed names."""
    L = C.CDLL(build(library))

    def sig(restype, argtypes, *names):
        for name in names:
            fn = getattr(L, prefix + name)
            fn.restype, fn.argtypes = restype, argtypes
    sig(C.c_int, [C.POINTER(params)], "default_params")
    sig(C.c_int, [VP], "destroy", "scene_update", "delete_vehicle", "n_ctl", "collisions", "lock", "n_jerks", "n_deleted",
        "ref_would_raise", "n_alive", "overflow", "tick_deferred")
    sig(C.c_int, [VP, C.c_int, C.c_int, C.c_double], "step")
    sig(C.c_int, [VP, DP], "tick_actions")
    sig(IP, [VP], "ids", "nbr", "coll_pv", "deleted")
    sig(DP, [VP], "reward", "state", "jerks")
    sig(C.c_int, [VP, C.c_int], "set_capacity")
    sig(C.c_uint, [VP], "deferred_lanes")
    sig(C.c_double, [VP], "time")
    sig(C.c_int, [VP, IP], "export_env")
    sig(C.c_int, [VP, C.c_int, C.c_int, C.c_double, DP], "get_virtual_distance")
    sig(C.c_long, [VP, C.c_int, DP, C.c_int, C.c_int, C.c_int, LP], "run_pool")
    extras(L, sig)
    return L


class Calls:
    """The entry points of a library without their prefix: Calls(L, "pvo_").n_alive is L.pvo_n_alive"""

    def __init__(self, L, prefix):
        self._L, self._prefix = L, prefix

    def __getattr__(self, name):
        fn = getattr(self._L, self._prefix + name)
        setattr(self, name, fn)
        return fn


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros((0,), dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class CtypesEnv:
    """Single environment; same call protocol as the reference object (ctor warm-up, step, scene_update, delete_vehicle).
    A subclass sets PREFIX and Params, lane_num and dir_num (class or instance), and creates the handle in its constructor
    between _params() and _bound()."""
    PREFIX, Params = None, None
    VEHICLE_EXTRAS = ()               # blocks of export_vehicles after veh_i, veh_f, obs0: (snapshot key, columns), int32
    ENV_EXTRAS = ()                   # ints of export_env between the three counters and veh_num

    def _params(self, L, params):
        self._L, self._c = L, Calls(L, self.PREFIX)
        prm = self.Params()
        self._c.default_params(C.byref(prm))
        for k, v in params.items():
            if not hasattr(prm, k):
                raise TypeError("unknown parameter %s" % k)
            setattr(prm, k, float(v))
        return prm

    def _bound(self, capacity):
        self.capacity = None if capacity is None else int(capacity)
        if capacity is not None and self._c.set_capacity(self._h, int(capacity)) != 0:
            raise ValueError("capacity must be at least one slot per lane")
        self.tick_no = 0

    def __del__(self):
        if getattr(self, "_h", None):
            self._c.destroy(self._h)
            self._h = None

    # -- reference-shaped calls
    def step(self, lane, ind, a):
        self._c.step(self._h, int(lane), int(ind), float(a))

    def scene_update(self):
        self._c.scene_update(self._h)

    def delete_vehicle(self):
        self._c.delete_vehicle(self._h)

    # -- views
    @property
    def n_alive(self):
        return self._c.n_alive(self._h)

    @property
    def current_time(self):
        return self._c.time(self._h)

    @property
    def overflow(self):
        """spawns deferred so far, one per lane and tick (0 for an unbounded env)"""
        return self._c.overflow(self._h)

    @property
    def ref_would_raise(self):
        return self._c.ref_would_raise(self._h)

    def vehicles(self):
        n = self.n_alive
        out = (np.zeros((n, len(VEH_I_COLS)), np.int32), np.zeros((n, len(VEH_F_COLS)), np.float64), np.zeros((n, 28), np.float64)) \
            + tuple(np.zeros((n, cols), np.int32) for _, cols in self.VEHICLE_EXTRAS)
        if n:
            self._c.export_vehicles(self._h, *[a.ctypes.data_as(IP if a.dtype == np.int32 else DP) for a in out])
        return out

    def alive_view(self):
        vi, _vf, obs0 = self.vehicles()[:3]
        return vi[:, 2].astype(np.int64), vi[:, 5].copy(), obs0

    def get_virtual_distance(self, lane1, lane2, p1):
        vd = C.c_double(0.0)
        ok = self._c.get_virtual_distance(self._h, lane1, lane2, float(p1), C.byref(vd))
        return (vd.value if ok else None)

    # -- one caller-protocol tick -> canonical record (snapshot before delete), then compaction
    def tick(self, actions, want_state=False):
        actions = np.ascontiguousarray(actions, dtype=np.float64)
        assert actions.shape[0] == self.n_alive
        self._c.tick_actions(self._h, actions.ctypes.data_as(DP))
        rec = self.snapshot(want_state)
        self._c.delete_vehicle(self._h)
        self.tick_no += 1
        return rec

    def snapshot(self, want_state=False):
        c, h = self._c, self._h
        Cn = c.n_ctl(h)
        nl, nd_ = self.lane_num, self.dir_num
        rec = dict(tick=self.tick_no, time=c.time(h))
        rec["ids"] = _arr(c.ids(h), Cn * 2, np.int32).reshape(Cn, 2)
        rec["nbr"] = _arr(c.nbr(h), Cn * 12, np.int32).reshape(Cn, 6, 2)
        rec["reward"] = _arr(c.reward(h), Cn, np.float64)
        st = _arr(c.state(h), Cn * 196, np.float64).reshape(Cn, 7, 28)
        rec["obs0"] = np.ascontiguousarray(st[:, 0, :])
        rec["state"] = st if want_state else None
        rec["act7"] = np.ascontiguousarray(st[:, :, 2]) if want_state else None
        rec["coll_pv"] = _arr(c.coll_pv(h), Cn, np.int32)
        rec["collisions"] = c.collisions(h)
        rec["lock"] = c.lock(h)
        nj = c.n_jerks(h)
        rec["jerks"] = _arr(c.jerks(h), nj, np.float64)
        nd = c.n_deleted(h)
        rec["deleted"] = _arr(c.deleted(h), nd * 2, np.int32).reshape(nd, 2)
        veh = self.vehicles()
        rec["veh_i"], rec["veh_f"] = veh[:2]
        for (key, _), block in zip(self.VEHICLE_EXTRAS, veh[3:]):
            rec[key] = block
        k = 3 + len(self.ENV_EXTRAS)
        ev = np.zeros(k + 2 * nl + 3 * nd_, np.int32)
        c.export_env(h, ev.ctypes.data_as(IP))
        rec["id_seq"], rec["passed"], rec["passed_step_total"] = int(ev[0]), int(ev[1]), int(ev[2])
        # capacity bound: deferrals so far / of this tick / this tick's deferred lanes as a mask (all 0 when unbounded)
        rec["overflow"], rec["deferred"] = c.overflow(h), c.tick_deferred(h)
        rec["deferred_lanes"] = int(c.deferred_lanes(h))
        for i, key in enumerate(self.ENV_EXTRAS):
            rec[key] = int(ev[3 + i])
        rec["veh_num"] = ev[k:k + nl].copy()
        rec["veh_rec"] = ev[k + nl:k + 2 * nl].copy()
        rec["heads"] = ev[k + 2 * nl:].reshape(nd_, 3).copy()
        return rec

    def run_pool(self, ticks, pool, tick0=0):
        """Timing loop entirely in C with a per-slot action pool [n_pool, cap] (bench.py cpu_baseline; see pvo_run_pool).
        -> (alive_steps, ctl_steps)"""
        pool = np.ascontiguousarray(pool, dtype=np.float64)
        ctl = C.c_long(0)
        alive = self._c.run_pool(self._h, int(ticks), pool.ctypes.data_as(DP), pool.shape[0], pool.shape[1], int(tick0), C.byref(ctl))
        self.tick_no += ticks
        return int(alive), int(ctl.value)

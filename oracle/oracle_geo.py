"""ctypes wrapper of the general-geometry CPU oracle (oracle/pve_oracle_geo.c; lane_num 4 / 8 / 12).
TEST INFRASTRUCTURE ONLY -- same import rules as oracle/oracle.py, the same base (oracle/ctypes_env.py).
"""
import ctypes as C
import functools

import numpy as np

from . import ctypes_env
from .ctypes_env import DP, IP, VP

DIR_NUM = {4: 12, 8: 16, 12: 12}


class PvgParams(C.Structure):
    _fields_ = ctypes_env.PARAM_FIELDS


def build(force=False):
    return ctypes_env.build("libpve_oracle_geo.so", force)


def _extras(L, sig):
    sig(VP, [DP, IP, C.c_int, C.c_int, C.POINTER(PvgParams)], "create")
    sig(C.c_int, [VP], "lane_num", "dir_num")
    sig(C.c_int, [VP, IP, DP, DP, IP], "export_vehicles")
    sig(C.c_int, [VP, C.c_double, C.c_int, C.c_int, DP], "get_p")


@functools.lru_cache(maxsize=None)
def lib():
    return ctypes_env.load("libpve_oracle_geo.so", "pvg_", PvgParams, _extras)


class OracleGeoEnv(ctypes_env.CtypesEnv):
    """Single environment of `lane_num` physical lanes; same call protocol as the reference object.
    `choice` ([rows, lane_num] of 0/1) replaces the reference's random.randint(0, 1) draws (8-lane).
    capacity: the slots of a batched env (None = unbounded, as the reference); the deferral rule of OracleEnv.  A deferred
    spawn draws no intention: `intention_re` and the 8-lane `choice` cursor stay where they are."""
    PREFIX, Params = "pvg_", PvgParams
    VEHICLE_EXTRAS = (("intent", 2),)
    ENV_EXTRAS = ("intention_re",)

    def __init__(self, arrive_time, lane_num, choice=None, capacity=None, **params):
        prm = self._params(lib(), params)
        arr = np.ascontiguousarray(arrive_time, dtype=np.float64)
        assert arr.ndim == 2 and arr.shape[1] == lane_num
        ch = None
        if choice is not None:
            ch = np.ascontiguousarray(choice, dtype=np.int32)
            assert ch.shape == arr.shape
        self.lane_num = int(lane_num)
        self.dir_num = DIR_NUM[self.lane_num]
        self._h = self._c.create(arr.ctypes.data_as(DP), ch.ctypes.data_as(IP) if ch is not None else None,
                                 arr.shape[0], self.lane_num, C.byref(prm))
        if not self._h:
            raise ValueError("lane_num must be 4, 8 or 12")
        self._bound(capacity)

    def get_p(self, p, lane, intention):
        out = np.zeros(2, np.float64)
        self._c.get_p(self._h, float(p), int(lane), int(intention), out.ctypes.data_as(DP))
        return out

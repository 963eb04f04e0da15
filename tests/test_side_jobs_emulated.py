"""CPU parity of the side jobs of the HOME block (csrc/pve_tick_core.h, Shared<128, false, true>::SIDE): thread
t works the dead-lock walk (LOCK) and the single-precision position (BUILD) of dense vehicle t ^ 64 and the stale head (WALK)
of lane t ^ 64, from LDS alone.  The emulator (PVE_EMU_HOME = 1) runs the same phase bodies; every roll-out through the work
queue must equal single ticks of k_tick bit for bit, on shapes where each job decides something -- asserted from the metrics.
(The emulator runs the threads of a phase one after the other: a race between the two waves is not something it can see;
the hazard table in DESIGN.md 3.2 is the argument for that.)"""
import ctypes as C

from tests import side_jobs_scenarios as S
from tests.hip_adapter import emulator_lib

BACKEND = "emu"


def _passes():
    lib = emulator_lib()
    lib.pve_emu_max_passes.restype = C.c_int
    return int(lib.pve_emu_max_passes())


def test_side_jobs_dense_vehicles_all_in_the_first_wave(monkeypatch):
    monkeypatch.setenv("PVE_EMU_HOME", "1")
    st = S.run(BACKEND, S.WAVE0, n_envs=3)
    print(st)
    assert st["max_alive"] <= 64, st                      # (alive <= 64: the controlled ones are threads 0..63 for sure)
    assert st["locks"] > 0 and st["collided"] > 0, st     # the walk found cycles; the xy32 pre-filter let pairs through


def test_side_jobs_controlled_count_crosses_64(monkeypatch):
    monkeypatch.setenv("PVE_EMU_HOME", "1")
    st = S.run(BACKEND, S.CROSSING, n_envs=3)
    print(st)
    assert st["locks"] > 0 and st["collided"] > 0, st
    n_ctl = S.controlled_per_tick(BACKEND, S.CROSSING, n_envs=3)
    print("controlled per tick: min %d, max %d, ticks > 64: %d of %d" % (n_ctl.min(), n_ctl.max(), (n_ctl > 64).sum(), n_ctl.size))
    assert (n_ctl > 64).any() and ((n_ctl > 0) & (n_ctl <= 64)).any(), "the controlled count must lie on both sides of 64"
    assert int(n_ctl.sum()) == int(st["ctl_steps"]), "the trajectory call is not the run the metrics are of"


def test_side_jobs_more_than_64_controlled_throughout(monkeypatch):
    monkeypatch.setenv("PVE_EMU_HOME", "1")
    _passes()
    st = S.run(BACKEND, S.FULL, n_envs=2)
    print(st)
    assert st["locks"] > 0, st
    assert st["mean_ctl"] > 64 and st["overflow"] > 0, st
    assert _passes() >= 2, "a full intersection must overflow the 304-entry pool (the heads per group of lists)"

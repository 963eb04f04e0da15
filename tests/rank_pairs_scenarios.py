"""RANK on pairs of list entries (csrc/pve_tick_core.h, ph_rank_pairs): the 128-slot queue kernel against the sequential oracle.

Four streams, each run as `prefill` un-retained ticks followed by <= 60 ticks whose retained blocks (flags, lanej, nbr, reward,
env_out, new_slot and the observation rows) are held to the oracle's record of EVERY tick -- ints exact, floats at
oracle.record.close 1e-9, the bars of tests/bounded_scenarios.py, whose comparators do the work -- then the header and the
persistent state field by field.  All of it through pve_step_many(source="table", persistent=True, chunk=...): the HOME build
of the queue kernel on the GPU, the same phase bodies on the emulator (PVE_EMU_HOME=1 / 2).

  TRAFFIC    4 envs from an empty intersection at 1100 veh/h/lane: the lists grow through the lengths 0, 1, 2, 3, ...
  SYMMETRIC  lanes that spawn in the same tick and a zero tape: vehicles with equal distances in the lists they share, filed in
             different pairs and waves (two neighbours of a list never tie in traffic: that case is driven by the emulator's RANK
             probe, tests/test_rank_pairs_emulated.py)
  QUANTISED  a tape quantised to 1 m/s^2 at 1600 veh/h/lane: vehicles that share a spawn tick keep exactly equal or
             one-ulp-apart distances for many ticks (the 12-lane counterpart of the 8-lane one-ulp regression stream)
  FULL       3000 veh/h/lane, vm = 3 m/s, a braking tape: > 80 controlled vehicles, more list entries than the pool holds,
             i.e. the multi-pass RANK (ph_rank<true>), against CAPACITY-BOUND oracles through the deferred spawns
"""
import collections
import contextlib
import functools

import numpy as np

from oracle.record import close
from tests import bounded_scenarios as B
from tests import native, scenarios
from tests.hip_adapter import _np, state_snapshot


def diag_emulator_lib():
    """The CPU test emulator built with RANK's counters (PVE_EMU_DIAG) and the RANK probe (tests/emu_diag): the very sources of
    tests/emu, one more translation unit around them."""
    return native.load_emulator("emu_diag", "libpveenv_emu_diag.so")


@contextlib.contextmanager
def diag_emulator():
    """backend "emu" runs on the diagnostics build inside this block"""
    from tests import hip_adapter
    saved, hip_adapter._emu = hip_adapter._emu, diag_emulator_lib()
    try:
        yield hip_adapter._emu
    finally:
        hip_adapter._emu = saved


Case = collections.namedtuple("Case", "name scn prefill ticks chunk arrivals")

LANE_GROUPS = ((0, 3, 6, 9), (1, 4, 7, 10), (2, 5, 8, 11))


def _case(name, n_envs, prefill, ticks, chunk, rate, seed, arrivals=None, **kw):
    return Case(name, B.Scn(12, 128, n_envs, prefill + ticks, rate, seed, tape="table", **kw), prefill, ticks, chunk, arrivals)


TRAFFIC = _case("traffic", 4, 0, 60, 7, 1100.0, 311)
SYMMETRIC = _case("symmetric", 4, 0, 60, 9, 1100.0, 313, arrivals="symmetric", lo=0.0, hi=0.0)
QUANTISED = _case("quantised", 6, 120, 60, 11, 1600.0, 3110, quantize=1.0)
FULL = _case("full", 2, 250, 60, 8, 3000.0, 191, lo=-3.0, hi=-2.0, cfg=(("vm", 3.0), ("collision_thr", 0.01)))
CASES = {c.name: c for c in (TRAFFIC, SYMMETRIC, QUANTISED, FULL)}


@functools.lru_cache(maxsize=None)
def oracle_run(case):
    """The (capacity-bound) oracle's record of every tick of every env of a case: computed once, shared, never modified."""
    scn = case.scn
    run = B.scenario_inputs(scn)
    if case.arrivals == "symmetric":
        run.arr = scenarios.symmetric_arrivals(scn.n_envs, gap_s=3.4, rows=40, lane_groups=[list(g) for g in LANE_GROUPS])
    oracles = B.make_oracles(run)
    run.recs = []
    for t in range(scn.ticks):
        row = []
        for e, o in enumerate(oracles):
            vid, ctl, _ = o.alive_view()
            pre = o.snapshot()
            rec = o.tick(B._actions(run, t, e, vid, ctl))
            rec = {k: rec[k] for k in B._KEEP if k in rec}
            rec.update(tick=t, n_pre=len(vid), id_seq_pre=pre["id_seq"], veh_rec_pre=pre["veh_rec"])
            row.append(rec)
        run.recs.append(row)
    run.final = [o.vehicles() for o in oracles]
    run.overflow = [o.overflow for o in oracles]
    run.max_ctl = max(len(r["ids"]) for row in run.recs[case.prefill:] for r in row)
    run.collisions = sum(r["collisions"] for row in run.recs for r in row)
    return run


def equal_distance_pairs(run, case):
    """Retained ticks in which two controlled vehicles of one env hold the same (position, speed) on lanes of one symmetry
    group: they share every list they both enter, with equal virtual distances."""
    n = 0
    for row in run.recs[case.prefill:]:
        for r in row:
            vi, vf = r["veh_i"], r["veh_f"]
            ctl = vi[:, 5] != 0
            key = np.stack([vi[ctl, 0] % 3, vf[ctl, 0].view(np.int64), vf[ctl, 1].view(np.int64)], -1)
            n += int(len(key) - len(np.unique(key, axis=0)) > 0)
    return n


def check_queue_kernel_vs_oracle(backend, case):
    scn = case.scn
    run = oracle_run(case)
    outs = ("obs_post", "reward", "flags", "nbr", "env_out", "new_slot", "lanej")
    b = B._batch(run, backend, outs)
    if case.prefill:
        b.step_many(case.prefill, source="table", chunk=case.chunk * 3, persistent=True)
        b.synchronize()
        for e in range(scn.n_envs):
            B.compare_header(run.recs[case.prefill - 1][e], b.read_env(e), "%s: after the prefill, env %d" % (case.name, e), 12)
    traj = b.step_many(case.ticks, source="table", trajectory=True, chunk=case.chunk, persistent=True)
    b.synchronize()
    assert b.last_launch() == "persistent", b.last_launch()
    host = {k: _np(traj[k][:case.ticks]) for k in outs}
    for k in range(case.ticks):
        for e in range(scn.n_envs):
            B.compare_tick(run.recs[case.prefill + k][e], {x: v[k, e] for x, v in host.items()},
                           "%s: tick %d env %d" % (case.name, case.prefill + k, e), rows="post")
    for e in range(scn.n_envs):
        B.compare_header(run.recs[-1][e], b.read_env(e), "%s: after the last tick, env %d" % (case.name, e), 12)
        _info, vi, vf = state_snapshot(b, e)
        ovi, ovf = run.final[e][0], run.final[e][1]
        assert np.array_equal(vi[:, :13], ovi[:, :13]), "%s: final state ints, env %d" % (case.name, e)
        assert close(ovf[:, :5], vf[:, :5], 1e-9), "%s: final state floats, env %d" % (case.name, e)
    assert b.metrics()["overflow"] == sum(run.overflow)
    return run

"""The three traffic shapes on which the side jobs of the 128-slot HOME block (csrc/pve_tick_core.h, DESIGN.md 3.2: the
dead-lock walk, the single-precision positions and the stale list heads of dense vehicle / lane c are worked by thread
c ^ 64) can go wrong, shared by the CPU test (tests/test_side_jobs_emulated.py) and its GPU twin (tests/test_gpu_side_jobs.py).
Every roll-out must equal single ticks of k_tick bit for bit (scenarios.check_step_many); what makes a shape bite is asserted
from the metrics it returns (ref traffic_interaction_scene.py:322-334 collision test, :365-370 and :1469-1499 dead-lock scan,
:1517 stale heads)."""
import numpy as np
import torch

from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import scenarios
from tests.hip_adapter import _np, make_batch

# (a) every dense vehicle in the first wave (the rule at the headline load): all side jobs run in the second wave
WAVE0 = dict(source="table", seed=281, chunks=(20, 9, 33, 50), trajectory_chunk=14)
# (b) the controlled count crosses 64 back and forth: side jobs in both waves, and in neither lane set twice
CROSSING = dict(source="table", seed=7, rate=1800.0, chunks=(150, 40, 7, 60, 90), trajectory_chunk=10)
# (c) a full intersection, > 64 controlled throughout, more list entries than the pool holds: the heads per group of lists
FULL = dict(source="table", seed=191, rate=3000.0, cfg=dict(vm=3.0, collision_thr=0.01), act_lo=-3.0, act_hi=-2.0,
            chunks=(250, 40, 7, 60), trajectory_chunk=10)


def run(backend, shape, n_envs):
    """check_step_many through the work queue; the metrics plus `mean_ctl` = controlled vehicles per intersection and tick"""
    st = scenarios.check_step_many(backend, n_envs=n_envs, persistent=True, waves=5 if backend == "hip" else None, **shape)
    st["mean_ctl"] = st["ctl_steps"] / st["ticks"]
    return st


def controlled_per_tick(backend, shape, n_envs):
    """len(ids) of every (tick, intersection) of the shape's run, from the env_out blocks of ONE trajectory call on the same
    arrival streams and action table (scenarios.check_step_many draws the pool, then the table, from the shape's seed)"""
    ticks = sum(shape["chunks"]) + shape["trajectory_chunk"]
    arr = synthetic_arrivals(n_envs, rate=shape.get("rate", 1100.0), horizon_s=ticks * 0.1 + 30, seed=shape["seed"])
    b = make_batch(arr, n_envs, 128, backend, outputs=("flags", "env_out"), **shape.get("cfg", {}))
    b.reset()
    rng = np.random.default_rng(shape["seed"])
    lo, hi = shape.get("act_lo", -3.0), shape.get("act_hi", 3.0)
    rng.uniform(lo, hi, size=(5, n_envs, 128))
    b.set_action_table(torch.as_tensor(rng.uniform(lo, hi, size=(23, 150))))
    traj = b.step_many(ticks, source="table", trajectory=True, chunk=ticks // 3 + 1, persistent=True)
    b.synchronize()
    assert b.last_launch() == "persistent", b.last_launch()
    if backend == "hip":                                    # (the side jobs live in the HOME build)
        assert b.last_variant()["waves_per_simd"] == 5, b.last_variant()
    return _np(traj["env_out"])[:, :, 1]

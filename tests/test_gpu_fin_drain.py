"""-m gpu: the resident tick consumes its prefetches (next action, the spawn's first action, the next arrival time) in front of
FIN's first output store and parks them in LDS (k_rollout<.., NODRAIN / PARK>) -- a value parked in a wrong cell,
moved to a wrong slot or read back too late shows as a wrong action, a wrong arrival time or a wrong first action of a spawned
vehicle within a few ticks.  A persistent call of 23 ticks in items of 6 (three full items and a tail of 5; every sixth tick is an
item's last, whose act_next[] cells hold the jerks), every tick's outputs in trajectory form, bit for bit against single ticks of
k_tick; once at the bench load and once with the intersection full (deferred spawns: the late gather of the spawn's action)."""
import numpy as np
import pytest
import torch

from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import scenarios
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
BACKEND = "hip"
N_ENVS, TICKS, ITEM = 8, 23, 6
OUTS = ("obs_post", "reward", "flags", "nbr", "new_slot", "env_out", "lanej")
# a rate that fills the intersection (with slow, braking vehicles: cf. test_gpu_home_block.py) and the ticks after which it is
# just full: on the emulator, 19 / 20 of the 23 ticks behind them have both a spawn and a deferred spawn (64 / 128 slots)
FULL = {64: (1500.0, 120), 128: (3000.0, 140), 256: (3000.0, 280)}
FULL_CFG = dict(vm=3.0, collision_thr=0.01)


def _same_outputs(o1, o2, what):
    f = _np(o1["flags"])
    assert np.array_equal(f, _np(o2["flags"])), what + ": flags"
    alive, ctl = (f & 1) != 0, (f & 2) != 0
    for k in ("reward", "new_slot", "lanej"):
        assert np.array_equal(_np(o1[k])[alive], _np(o2[k])[alive]), what + ": " + k
    assert np.array_equal(_np(o1["nbr"])[ctl], _np(o2["nbr"])[ctl]), what + ": nbr"
    assert np.array_equal(_np(o1["env_out"]), _np(o2["env_out"])), what + ": env_out"


def _trajectory_in_items(source, capacity, full):
    rate, prefill = FULL[capacity] if full else (1100.0, 60)
    cfg = FULL_CFG if full else {}
    lo, hi = (-3.0, -2.0) if full else (-3.0, 3.0)
    seed = 311 + capacity + (7 if full else 0)
    rng = np.random.default_rng(seed)
    arr = synthetic_arrivals(N_ENVS, rate=rate, horizon_s=(prefill + TICKS) * 0.1 + 30, seed=seed)
    one = make_batch(arr, N_ENVS, capacity, BACKEND, outputs=OUTS, **cfg)
    many = make_batch(arr, N_ENVS, capacity, BACKEND, outputs=OUTS, **cfg)
    one.reset(); many.reset()
    n_pool = 5
    pool = torch.as_tensor(rng.uniform(lo, hi, size=(n_pool, N_ENVS, capacity))).to(one.device)
    if source == "pool":
        many.set_action_pool(pool)
    else:
        table = torch.as_tensor(rng.uniform(lo, hi, size=(23, 150)))
        one.set_action_table(table); many.set_action_table(table)

    def single():
        return one.step(one.actions_from_table()) if source == "table" else one.step(pool[one.ticks % n_pool])

    for _ in range(prefill):
        single()
    many.step_many(prefill, source=source)                  # (one plain launch of the resident kernel)
    assert many.last_launch() == "resident" and many.last_variant()["waves_per_simd"] == 4
    scenarios.batches_equal(one, many, "after the prefill")
    traj = many.step_many(TICKS, source=source, trajectory=True, chunk=ITEM, persistent=True)
    assert many.last_launch() == "persistent"
    assert many.last_variant()["waves_per_simd"] == (5 if capacity == 128 else 4)      # (128 slots: the HOME build)
    spawned = 0
    for k in range(TICKS):
        o1 = single()
        _same_outputs(o1, {n: traj[n][k] for n in traj}, "tick %d" % k)
        post_ctl = (_np(one.state_field("meta")) & 1) != 0
        assert np.array_equal(_np(one.obs)[post_ctl], _np(traj["obs_post"][k])[post_ctl]), "observation rows, tick %d" % k
        spawned += int(_np(o1["env_out"])[:, 6].sum())
    scenarios.batches_equal(one, many, "after the persistent call")
    m1, m2 = one.metrics(), many.metrics()
    assert m1 == m2, (m1, m2)
    assert m1["ctl_steps"] > 0 and spawned > 0, (m1, spawned)
    return dict(m1, max_alive=int(max(one.read_env(e).n_alive for e in range(N_ENVS))))


@pytest.mark.parametrize("source", ["table", "pool"])
@pytest.mark.parametrize("capacity", [128, 64, 256])
def test_gpu_items_of_six_equal_single_ticks(source, capacity):
    _trajectory_in_items(source, capacity, full=False)


@pytest.mark.parametrize("source", ["table", "pool"])
@pytest.mark.parametrize("capacity", [128, 64, 256])
def test_gpu_items_of_six_equal_single_ticks_full_intersection(source, capacity):
    st = _trajectory_in_items(source, capacity, full=True)
    if capacity <= 128:                                     # (256 slots: dense traffic only, the lanes do not carry enough to fill them)
        assert st["max_alive"] == capacity and st["overflow"] > 0, st


@pytest.mark.parametrize("source", ["table", "pool"])
def test_gpu_items_of_six_through_check_step_many(source):
    """the suite's own comparison (state, headers, rows, last-tick outputs, trajectory, metrics): calls of 17 ticks and a
    trajectory call of 11, both in items of 6"""
    scenarios.check_step_many(BACKEND, source, n_envs=N_ENVS, chunks=(40, 17, 17), trajectory_chunk=11, seed=313, persistent=True, waves=5)

"""Scenarios of the 256-slot capacity (12-lane fast path), shared by the CPU file (wide emulator, tests/emu_wide) and the
`-m gpu` file (k_tick<256> / k_rollout<256, ..>)."""
import types

import numpy as np
import torch

from oracle.oracle import OracleEnv
from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import scenarios
from tests.hip_adapter import SplitEnv, _np, make_batch

# The dense scenario: a Poisson stream at 2200 veh/h/lane and a braking tape (every controlled vehicle asks for -3 m/s^2, the
# lower bound, so it crawls through at vm).  Oracle peaks of the 4 envs over 350 ticks: 174, 200, 187, 177 vehicles alive at
# once -- above 128 from tick 177 .. 203 on, well below 256.
DENSE_RATE, DENSE_SEED, DENSE_ENVS, DENSE_TICKS = 2200.0, 2561, 4, 350


def dense_arrivals(n_envs=DENSE_ENVS):
    return synthetic_arrivals(n_envs, rate=DENSE_RATE, horizon_s=DENSE_TICKS * 0.1 + 30.0, seed=DENSE_SEED)


def brake_policy(t, veh_id, control, obs0=None):
    return np.where(np.asarray(control) != 0, -3.0, 0.0)


def dense_case(env, ticks=DENSE_TICKS):
    """GoldenCase-shaped view of env `env` of the dense stream (what the scenarios.check_* helpers read)."""
    return types.SimpleNamespace(name="dense256_e%d" % env, arrive=np.ascontiguousarray(dense_arrivals()[env]), ctor={},
                                 ticks=ticks, policy=brake_policy)


def oracle_peak(arr, ticks=DENSE_TICKS):
    o = OracleEnv(arr)
    peak = 0
    for _ in range(ticks):
        vid, ctl, _ = o.alive_view()
        o.tick(brake_policy(0, vid, ctl))
        peak = max(peak, o.n_alive)
    return peak


def check_dense_split(backend, env, ticks=DENSE_TICKS):
    """Split protocol at 256 slots vs the oracle: every tick, every field at 1e-9, no deferred spawn."""
    b = scenarios.check_split_vs_oracle(dense_case(env, ticks), backend, ticks, capacity=256, tol=1e-9)
    assert b.metrics()["overflow"] == 0
    return b


# The full scenario: the same stream seed at 5000 veh/h/lane with the braking tape fills all 256 slots (env 0: from tick 265 on,
# 464 deferred spawns in 350 ticks, 61 collisions, 198 dead-locks on the oracle side).
FULL_RATE = 5000.0


def full_case(env, ticks=DENSE_TICKS):
    arr = synthetic_arrivals(env + 1, rate=FULL_RATE, horizon_s=DENSE_TICKS * 0.1 + 30.0, seed=DENSE_SEED)[env]
    return types.SimpleNamespace(name="full256_e%d" % env, arrive=np.ascontiguousarray(arr), ctor={}, ticks=ticks, policy=brake_policy)


def check_full_split(backend, env=0, ticks=DENSE_TICKS):
    """Split protocol at 256 slots through a FULL intersection against the capacity-bound oracle: every tick, every field at
    1e-9, the grants / cursors / id counter / deferral count every tick, metrics()["overflow"] == the oracle's count > 0."""
    b = scenarios.check_split_vs_oracle(full_case(env, ticks), backend, ticks, capacity=256, tol=1e-9, bounded=True)
    assert b.metrics()["overflow"] > 0
    return b


def check_dense_fused(backend, env, ticks=DENSE_TICKS):
    scenarios.check_fused_equals_split(dense_case(env, ticks), backend, ticks, capacity=256)


def check_dense_overflows_128(backend, env, ticks=DENSE_TICKS):
    """The same stream and tape at 128 slots defers spawns: the scenario lies beyond the old capacity."""
    case = dense_case(env, ticks)
    b = make_batch(case.arrive, 1, 128, backend)
    e = SplitEnv(b)
    for t in range(ticks):
        vid, ctl, obs = e.alive_view()
        e.tick(brake_policy(t, vid, ctl))
    assert b.metrics()["overflow"] > 0


def check_dense_step_many(backend, source, persistent=False, chunks=(1, 9, 60, 120, 40), trajectory_chunk=12):
    """pve_step_many at 256 slots on the dense stream (braking-heavy pool) == single ticks, bit for bit."""
    scenarios.check_step_many(backend, source, n_envs=DENSE_ENVS, capacity=256, seed=DENSE_SEED, chunks=chunks,
                              trajectory_chunk=trajectory_chunk, arrivals=dense_arrivals(), persistent=persistent,
                              act_lo=-3.0, act_hi=-1.0)


def check_dense_training_rows(backend, persistent=False, chunk=0, source="pool", calls=(120, 60, 90, 60)):
    """obs_pre / state_pre of trajectory roll-outs at 256 slots vs the oracle at every tick (the per-thread state write)."""
    scenarios.check_step_many_state_rows(backend, n_envs=2, capacity=256, rate=DENSE_RATE, calls=calls, seed=DENSE_SEED,
                                         chunk=chunk, source=source, persistent=persistent)


STATE_FIELDS = scenarios.STATE_F + scenarios.STATE_I


def check_capacity_equivalence(backend, n_envs=4, ticks=300, rate=900.0, seed=4321):
    """On a stream that never exceeds 128 alive, a 128 handle and a 256 handle compute the same: every per-slot field of
    slots < 128, empty slots above, headers, outputs and metrics."""
    rng = np.random.default_rng(seed)
    arr = synthetic_arrivals(n_envs, rate=rate, horizon_s=ticks * 0.1 + 30.0, seed=seed)
    outs = ("obs_post", "reward", "flags", "nbr", "new_slot", "env_out", "lanej")
    b1 = make_batch(arr, n_envs, 128, backend, outputs=outs)
    b2 = make_batch(arr, n_envs, 256, backend, outputs=outs)
    b1.reset()
    b2.reset()
    peak = 0
    for t in range(ticks):
        a = rng.uniform(-3, 3, size=(n_envs, 128))
        a2 = np.zeros((n_envs, 256))
        a2[:, :128] = a
        o1 = b1.step(torch.as_tensor(a).to(b1.device))
        o2 = b2.step(torch.as_tensor(a2).to(b2.device))
        for k in outs:
            x1, x2 = _np(o1[k]), _np(o2[k])
            if x1.ndim >= 2 and x1.shape[1] == 128:
                assert np.array_equal(x1, x2[:, :128]), "output %s differs at tick %d" % (k, t)
            else:
                assert np.array_equal(x1, x2), "output %s differs at tick %d" % (k, t)
        for e in range(n_envs):
            peak = max(peak, b2.read_env(e).n_alive)
    assert 0 < peak <= 128
    for k in STATE_FIELDS:
        s1, s2 = _np(b1.state_field(k)), _np(b2.state_field(k))
        assert np.array_equal(s1, s2[:, :128]), "state field %s differs" % k
    # slots 128 .. 255 never held a vehicle: never alive, no id
    assert np.all(_np(b2.state_field("meta"))[:, 128:] == 0) and np.all(_np(b2.state_field("id"))[:, 128:] == -1)
    for e in range(n_envs):
        h1, h2 = b1.read_env(e), b2.read_env(e)
        for f, _t in h1._fields_:
            v1, v2 = getattr(h1, f), getattr(h2, f)
            v1 = list(v1) if hasattr(v1, "__len__") else v1
            v2 = list(v2) if hasattr(v2, "__len__") else v2
            assert v1 == v2, "header %s differs (env %d)" % (f, e)
    m1, m2 = b1.metrics(), b2.metrics()
    for k in m1:                                  # (slot_steps counts ticks x capacity)
        assert (m2[k] == 2 * m1[k]) if k == "slot_steps" else (m2[k] == m1[k]), "metric %s: %r vs %r" % (k, m1[k], m2[k])
    return peak

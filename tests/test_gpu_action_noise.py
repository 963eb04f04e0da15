"""Exploration noise of the device actor on the GPU (pve_set_action_noise / BatchedIntersections.set_exploration): the kernels
add exactly float64(actor) + sigma * noise.action_noise(...), every launch form commands the same bits, the tick consumes them
(sequential oracle), a batch cut into pieces draws what the uncut batch draws, and noise off is the deterministic actor."""
import math

import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from oracle.record import close
from pve_mcc_amd import PipelinedIntersections, noise
from pve_mcc_amd.arrivals import synthetic_arrivals, synthetic_intentions
from tests.hip_adapter import _np, make_batch, state_snapshot
from tests.scenarios import batches_equal

pytestmark = pytest.mark.gpu
BACKEND = "hip"
OUTS = ("obs_post", "reward", "flags", "nbr", "new_slot", "env_out", "lanej")
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
RATE = {12: 1000.0, 8: 1300.0, 4: 1500.0}


def bits(x):
    return np.ascontiguousarray(_np(x), np.float64).view(np.uint64)


def new_batch(n_envs, capacity, lane_num=12, ticks=200, seed=5, rate=None, outputs=OUTS, **kw):
    rate = rate or RATE[lane_num] * (1.0 if capacity >= 128 else 0.5)
    arr = synthetic_arrivals(n_envs, rate=rate, horizon_s=ticks * 0.1 + 30, seed=seed, lane_num=lane_num)
    geo = {}
    if lane_num != 12:
        geo = dict(lane_num=lane_num,
                   intentions=synthetic_intentions(n_envs, arr.shape[1], seed=seed, lane_num=lane_num) if lane_num == 8 else None)

    def make():
        b = make_batch(arr, n_envs, capacity, BACKEND, outputs=outputs, **geo, **kw)
        b.reset()
        b.set_actor(flat_weights(load_weights()))
        return b
    return make, arr, geo.get("intentions")


def expected_actions(b, a_clean, sigma, seed, env_offset):
    """a_clean + sigma z for the controlled slots of the batch's current state, 0 elsewhere (NumPy restatement)."""
    ids = _np(b.state_field("id")).astype(np.int64)
    ctl = _np(b.control_mask()).astype(bool)
    env = np.arange(b.n_envs)[:, None] + env_offset
    z = noise.action_noise(seed, env, np.where(ctl, ids, 0), b.ticks)
    return np.where(ctl, _np(a_clean) + sigma * z, 0.0), ctl


# ------------------------------------------------------------------ 5. act() adds exactly the restated noise
@pytest.mark.parametrize("capacity,kw", [(64, {}), (128, {}), (256, {}), (128, dict(obs_dtype=torch.float32)),
                                         (128, dict(actor_f32=True)), (256, dict(obs_dtype=torch.float32, actor_f32=True))])
def test_gpu_act_adds_the_restated_noise(capacity, kw):
    make, _, _ = new_batch(6, capacity, ticks=120, rate=1000.0 if capacity >= 128 else 600.0, **kw)
    b = make()
    b.step_many(90, source="actor")
    sigma, seed, off = 0.2, 0xC0FFEE1234567, 3
    for _ in range(3):
        a_clean = b.act().clone()
        b.set_exploration(sigma, seed=seed, env_offset=off)
        a_noisy = b.act().clone()
        want, ctl = expected_actions(b, a_clean, sigma, seed, off)
        assert ctl.sum() >= 5 * b.n_envs
        assert np.array_equal(bits(a_noisy), want.view(np.uint64)), "act() with noise != act() + sigma * action_noise"
        assert np.all(_np(a_noisy)[~ctl] == 0) and np.any(_np(a_noisy)[ctl] != _np(a_clean)[ctl])
        b.step_with_actor()                       # (the noisy closed loop moves on; the next round draws another tick's noise)
        b.set_exploration(0.0)


# ------------------------------------------------------------------ 6. every launch form commands the same bits
def same_outputs(o1, o2, what, train=False):
    f = _np(o1["flags"])
    assert np.array_equal(f, _np(o2["flags"])), what + ": flags"
    alive, ctl = (f & 1) != 0, (f & 2) != 0
    for k in ("reward", "new_slot"):
        assert np.array_equal(_np(o1[k])[alive], _np(o2[k])[alive]), what + ": " + k
    assert np.array_equal(_np(o1["nbr"])[ctl], _np(o2["nbr"])[ctl]), what + ": nbr"
    assert np.array_equal(_np(o1["env_out"]), _np(o2["env_out"])), what + ": env_out"
    if train:
        for k in ("obs_pre", "state_pre"):
            assert np.array_equal(_np(o1[k])[ctl], _np(o2[k])[ctl]), what + ": " + k


FORMS = [("single launch", dict(chunk=0), "resident"), ("chunked", dict(chunk=7), "resident"),
         ("persistent", dict(chunk=7, persistent=True), "persistent")]


@pytest.mark.parametrize("lane_num,capacity,train,kw", [
    (12, 64, False, {}), (12, 128, False, dict(obs_dtype=torch.float32)), (12, 256, False, {}),
    (4, 64, False, {}), (4, 128, False, dict(obs_dtype=torch.float32)), (8, 128, False, {}),
    (12, 128, True, dict(obs_dtype=torch.float32)), (4, 128, True, dict(obs_dtype=torch.float32)),
    (12, 128, False, dict(actor_f32=True))])
def test_gpu_launch_forms_agree_with_noise(lane_num, capacity, train, kw):
    """step_with_actor() x n == step_many(source="actor") in one launch == chunked == the persistent queue, bit for bit on
    every persistent field, header and output, with sigma = 0.5 on a stream dense enough to spawn, finish and compact."""
    calls = (60, 45, 95)
    n_envs = 12
    make, _, _ = new_batch(n_envs, capacity, lane_num, ticks=sum(calls), seed=40 + lane_num, outputs=TRAIN_OUTS if train else OUTS, **kw)
    sigma, seed, off = 0.5, 20250213, 1000
    one = make()
    others = [(name, make(), args, launch) for name, args, launch in FORMS]
    for b in [one] + [o[1] for o in others]:
        b.set_exploration(sigma, seed=seed, env_offset=off)
    exact = bool(kw.get("actor_f32"))
    clipped = noisy = 0
    for n in calls:
        ticks = []
        for _ in range(n):
            o = one.step_with_actor()
            a = _np(one._actor_actions)
            clipped += int((np.abs(a) > 3.0).sum())
            noisy += int((a != 0).sum())
            if train:
                ticks.append({k: v.clone() for k, v in o.items()})
        assert one.last_launch() == "tick"
        for name, b, args, launch in others:
            what = "%s, lane_num %d x %d, call of %d" % (name, lane_num, capacity, n)
            o2 = b.step_many(n, source="actor", trajectory=train, **args)
            b.synchronize()
            # (the exact-float32 actor has no resident kernel; the 4- / 8-lane closed loop with the training outputs runs
            #  its queue form as chunked launches)
            want = "tick" if exact else ("resident" if (launch == "persistent" and train and lane_num != 12) else launch)
            assert b.last_launch() == want, (what, b.last_launch(), want)
            batches_equal(one, b, what)
            if train:
                for k in range(n):
                    same_outputs(ticks[k], {x: o2[x][k] for x in o2}, what + ", tick %d" % k, train=True)
            else:
                same_outputs(o, o2, what)
    m = one.metrics()
    for _, b, _, _ in others:
        assert b.metrics() == m
    # not an idle intersection: vehicles spawned, finished (so the slots were compacted under them), and the noise pushed
    # commanded actions beyond [am, aM] = [-3, 3], where the tick clips them
    assert m["spawned"] >= 10 * n_envs and m["passed"] >= n_envs and m["overflow"] == 0, m
    assert clipped >= 10 and noisy >= 1000, (clipped, noisy)


# ------------------------------------------------------------------ 7. the tick consumed what the actor produced
@pytest.mark.parametrize("lane_num", [12, 4])
def test_gpu_noisy_actions_drive_the_oracle(lane_num):
    from oracle.oracle import OracleEnv
    from oracle.oracle_geo import OracleGeoEnv
    n_envs, ticks = 4, 150
    make, arr, _ = new_batch(n_envs, 128, lane_num, ticks=ticks, seed=60 + lane_num)
    b = make()
    b.set_exploration(0.5, seed=77, env_offset=9)
    oracles = [OracleEnv(arr[e]) if lane_num == 12 else OracleGeoEnv(arr[e], lane_num) for e in range(n_envs)]
    n_ctl = 0
    for t in range(ticks):
        acts = _np(b.act()).copy()                # the noisy action buffer of this tick
        out = b.step_with_actor()
        assert np.array_equal(bits(b._actor_actions), acts.view(np.uint64)), "the tick's actions are the ones act() returned"
        rew, flags, lanej = _np(out["reward"]), _np(out["flags"]).astype(np.int64), _np(out["lanej"]).astype(np.int64)
        for e, o in enumerate(oracles):
            n = o.n_alive
            _vid, ctlm, _ = o.alive_view()
            assert np.all(acts[e, :n][ctlm == 0] == 0) and np.all(acts[e, n:] == 0)
            rec = o.tick(acts[e, :n])
            f = flags[e, :n]
            if lane_num == 12:
                ctl = np.flatnonzero((f & 2) != 0)
            else:
                order = np.lexsort((lanej[e, :n] & 0xFFFF, (f >> 6) & 3, lanej[e, :n] >> 16))
                ctl = order[((f & 2) != 0)[order]]
            assert len(ctl) == len(rec["ids"]), "controlled set: tick %d env %d" % (t, e)
            assert close(rec["reward"], rew[e, ctl], 1e-9), "reward: tick %d env %d" % (t, e)
            n_ctl += len(ctl)
    for e, o in enumerate(oracles):
        _info, vi, vf = state_snapshot(b, e)
        ovi, ovf = o.vehicles()[:2]
        assert np.array_equal(vi[:, :13], ovi[:, :13]), "state ints, env %d" % e
        assert close(ovf[:, :5], vf[:, :5], 1e-9), "state floats, env %d" % e
    assert n_ctl >= 10 * ticks


# ------------------------------------------------------------------ 8. cutting the batch changes nothing
def test_gpu_cut_batches_draw_the_same_noise():
    E, cap, ticks = 10, 128, 90
    arr = synthetic_arrivals(E, rate=1000.0, horizon_s=ticks * 0.1 + 30, seed=8)
    w = flat_weights(load_weights())
    sigma, seed = 0.5, 31337

    def prep(b, **kw):
        b.reset()
        b.set_actor(w)
        b.set_exploration(sigma, **kw)
        return b
    whole = prep(make_batch(arr, E, cap, BACKEND, outputs=OUTS), seed=seed)
    halves = [prep(make_batch(arr[k * 5:(k + 1) * 5], 5, cap, BACKEND, outputs=OUTS), seed=seed, env_offset=5 * k) for k in range(2)]
    pipe = prep(PipelinedIntersections(E, cap, arr, n_sub=2, outputs=OUTS), seed=seed)
    assert [s.exploration for s in pipe.subs] == [(sigma, seed, 0), (sigma, seed, 5)]
    other_seed = prep(make_batch(arr, E, cap, BACKEND, outputs=OUTS), seed=seed + 1)
    shifted = prep(make_batch(arr, E, cap, BACKEND, outputs=OUTS), seed=seed, env_offset=1)
    # the first tick's actions (reset() leaves every intersection with its first vehicle on the road)
    a0, a1, a2 = (_np(b.act()).copy() for b in (whole, other_seed, shifted))
    ctl = _np(whole.control_mask()).astype(bool)
    assert ctl.sum() >= E and np.all(a0[ctl] != 0)
    assert np.all(a0[ctl] != a1[ctl]), "another seed draws other noise"
    assert np.all(a0[ctl] != a2[ctl]), "env_offset + 1 draws the neighbour's noise"
    assert np.array_equal(a0[:5].view(np.uint64), bits(halves[0].act())) and np.array_equal(a0[5:].view(np.uint64), bits(halves[1].act()))
    whole.step_many(ticks, source="actor", chunk=9)
    for b in halves:
        b.step_many(ticks, source="actor")
    pipe.step_many(ticks, source="actor", chunk=9)
    pipe.synchronize()
    for k in range(2):
        for name in ("p", "v", "a", "jerk_sum", "vir_dis", "id", "seq", "step", "count", "meta"):
            x = _np(whole.state_field(name))[5 * k:5 * k + 5]
            assert np.array_equal(x, _np(halves[k].state_field(name))), "two batches: %s of piece %d" % (name, k)
            assert np.array_equal(x, _np(pipe.subs[k].state_field(name))), "pipelined: %s of piece %d" % (name, k)
    # (the counters; the float sums sum_reward / sum_jerk are added over the environments in another order when the batch is cut)
    m, pm, hm = whole.metrics(), pipe.metrics(), [b.metrics() for b in halves]
    assert m["ctl_steps"] > 20 * E
    for k in ("spawned", "passed", "collided", "locks", "ctl_steps", "alive_steps", "passed_steps", "overflow", "ticks"):
        assert m[k] == pm[k] == hm[0][k] + hm[1][k], k


# ------------------------------------------------------------------ 9. noise off is the deterministic closed loop
def test_gpu_noise_off_equals_a_fresh_batch():
    make, _, _ = new_batch(8, 128, ticks=120, seed=9)
    fresh, b = make(), make()
    b.set_exploration(0.2, seed=4, env_offset=2)
    b.set_exploration(0)
    for x in (fresh, b):
        for _ in range(20):
            x.step_with_actor()
        x.step_many(50, source="actor")
        x.step_many(50, source="actor", chunk=8, persistent=True)
    batches_equal(fresh, b, "noise switched off again")
    assert fresh.metrics() == b.metrics() and fresh.metrics()["ctl_steps"] > 0
    assert np.array_equal(bits(fresh.act()), bits(b.act()))


# ------------------------------------------------------------------ 10. the device's own numbers are standard normal
def test_gpu_device_noise_statistics():
    n_envs, ticks, sigma = 128, 200, 0.2
    make, _, _ = new_batch(n_envs, 128, ticks=ticks, seed=10)
    b = make()
    zs = []
    for t in range(ticks):
        b.set_exploration(0.0)
        a_clean = _np(b.act()).copy()
        b.set_exploration(sigma, seed=2025)
        b.step_with_actor()
        ctl = a_clean != 0
        zs.append(((_np(b._actor_actions) - a_clean)[ctl]) / sigma)
    z = np.concatenate(zs)
    N = len(z)
    mean, var = float(z.mean()), float(z.var())
    print("device noise: N %d  mean %.3e (bound %.3e)  var - 1 %.3e (bound %.3e)" % (N, mean, 5 / math.sqrt(N), var - 1, 5 * math.sqrt(2.0 / N)))
    assert N >= 100000
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1) <= 5 * math.sqrt(2.0 / N)

"""The split-half actor and critic kernels (k_actor_pack / k_actor_h / actor_tile32 inside k_rollout, k_critic_pack / k_target_q) on
weights a training run produces: every weight set and row family of tests/split_half_scenarios.py, against float64 NumPy
(pve_mcc_amd/critic.py) and against the CPU model of the half-pair arithmetic (tests/split_half_model.py), within the bars
stated in split_half_scenarios.py -- none of them taken from a device.  The rest of the suite holds these kernels to a reference
on ONE weight set each (the shipped checkpoint, the three networks of critic_graph.npz); the dense kernels of a freshly
initialised network are 100 to 400 times smaller, and without the power-of-two scale of k_*_pack the half pairs lose their low
halves there (tests/test_split_half_model.py shows that on the CPU).

Every test runs on 8 intersections x 128 slots or on a few thousand explicit rows and prints the maxima it measured before it
asserts ("split-half |" lines: profiles/split_half_weights.txt is made of them)."""
import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights
from pve_mcc_amd import _capi, critic
from pve_mcc_amd import learner as LN
from tests import actor_scenarios as A
from tests import split_half_model as M
from tests import split_half_scenarios as S
from tests import target_q_walk as TQ
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
BACKEND = "hip"
N_ENVS = 8
FIELDS = ("p", "v", "a", "jerk_sum", "vir_dis", "closer_p", "id", "step", "count", "meta")
OFF_SCALE = ("fresh-first-layer-0", "w1-x2^-10", "learned-fresh-64")      # weight sets whose pack-time factor is not 1

_planted = {}


def planted(**cfg):
    """one filled batch per configuration (8 x 128, shipped weights for the filling), shared: act() is stateless"""
    key = tuple(sorted(cfg.items(), key=str))
    if key not in _planted:
        _planted[key] = A.planted_batch(BACKEND, N_ENVS, **cfg)
        assert len(_planted[key][1]) >= 20 * N_ENVS
    return _planted[key]


def report(entry, name, family, spread, model, dev64, dev_model, bar):
    print("split-half | %-12s | %-36s | %-13s | spread %.3e | model %s | device %.3e | device-model %s | bar %.3e"
          % (entry, name, family, spread, "%.3e" % model if model is not None else "    -    ", dev64,
             "%.3e" % dev_model if dev_model is not None else "    -    ", bar))


# ------------------------------------------------------------------ 1. act(): k_actor_h on every weight set and row family
@pytest.mark.parametrize("name", list(S.actor_sets()))
def test_gpu_act_on_every_weight_set(name):
    w = S.actor_sets()[name]
    rows, family, names = S.all_actor_rows()
    b, slots = planted()
    b.set_actor(flat_weights(w))
    a = A.actions_of_planted_rows(b, slots, rows)                       # (asserts: uncontrolled slots are exactly 0)
    a64 = critic.actor_forward(w, rows, np.float64)
    a32 = critic.actor_forward(w, rows, np.float32).astype(np.float64)
    am = M.actor_split(w, rows).astype(np.float64)
    assert np.all(np.isfinite(a))
    bad = []
    for i, fam in enumerate(names):
        m = family == i
        spread = float(np.abs(a32[m] - a64[m]).max())
        bar = S.actor_bar(name, fam, spread)
        d64, dm, mm = (float(np.abs(x[m] - y[m]).max()) for x, y in ((a, a64), (a, am), (am, a64)))
        report("act", name, fam, spread, mm, d64, dm, bar)
        if not (d64 <= bar and dm <= bar):
            bad.append((fam, d64, dm, bar))
    assert not bad, bad


# ------------------------------------------------------------------ 2. the control: k_actor_t, the float32 chain, on the same sets
@pytest.mark.parametrize("name", list(S.actor_sets()))
def test_gpu_actor_f32_control(name):
    """PVE_CFG_ACTOR_F32 has no half pairs and no pack-time scale: within 3 x spread_a(W) of float64 on the rows under test (all
    four families together) -- the sets and the bars are sound on the device."""
    w = S.actor_sets()[name]
    rows, family, names = S.all_actor_rows()
    b, slots = planted(actor_f32=True)
    b.set_actor(flat_weights(w))
    a = A.actions_of_planted_rows(b, slots, rows)
    a64, spread = S.ref_actions(w, rows)
    worst = float(np.abs(a - a64).max())
    report("act f32", name, "all", spread, None, worst, None, 3.0 * spread)
    assert worst <= 3.0 * spread


# ------------------------------------------------------------------ 3. the all-zero row: act(), and the packed PV_A0 of the roll-out
def filled_pair(w, obs_dtype, seed=41):
    """two batches in the same filled state with the actor `w` installed"""
    pair = [A.planted_batch(BACKEND, N_ENVS, seed=seed, obs_dtype=obs_dtype, weights=w)[0] for _ in range(2)]
    for k in FIELDS:
        assert torch.equal(pair[0].state_field(k), pair[1].state_field(k)), k
    return pair


@pytest.mark.parametrize("name", ("fresh-0", "fresh-first-layer-0", "w1-x2^-10"))
def test_gpu_zero_row_and_first_action_of_a_spawned_vehicle(name):
    w = S.actor_sets()[name]
    zero = S.actor_rows()["zero"]
    b, slots = planted()
    b.set_actor(flat_weights(w))
    a0 = A.actions_of_planted_rows(b, slots, zero)[0]
    a64, spread = S.ref_actions(w, zero)
    bar = S.actor_bar(name, "zero", spread)
    am = float(M.actor_split(w, zero)[0])
    report("act zero", name, "zero", spread, abs(am - a64[0]), abs(a0 - a64[0]), abs(a0 - am), bar)
    assert abs(a0 - a64[0]) <= bar and abs(a0 - am) <= bar
    # the roll-out gives a vehicle it spawns the PACKED action of the all-zero row (PV_A0, computed by k_actor_pack with the tile)
    # for the tick after; the two-call form computes that action from the vehicle's (all-zero) row: same bits, on these weights
    x, y = filled_pair(w, torch.float32)
    seen = same = 0
    for rep in range(12):
        x.step_many(2, source="actor")
        y.step_many(1, source="actor")
        spawned = np.argwhere(_np(y.control_mask()) & ~_np(y.obs).any(axis=2))      # controlled, all-zero row: spawned by this tick
        ids = _np(y.state_field("id"))[spawned[:, 0], spawned[:, 1]]
        y.step_many(1, source="actor")
        for k in FIELDS:
            assert torch.equal(x.state_field(k), y.state_field(k)), (rep, k)
        idx, acc, ctl = _np(x.state_field("id")), _np(x.state_field("a")), _np(x.control_mask())
        for (e, _), v in zip(spawned, ids):
            at = np.flatnonzero((idx[e] == v) & ctl[e])
            if len(at) == 1:                                                         # (still there after its first tick)
                seen += 1
                same += int(np.float64(acc[e, at[0]]).tobytes() == np.float64(a0).tobytes())
    print("split-half | spawned      | %-36s | %d vehicles spawned under the roll-out, %d of them took exactly act(zero row) = %.9g"
          % (name, seen, same, a0))
    assert seen >= 5 and same >= 0.5 * seen, (seen, same)


# ------------------------------------------------------------------ 4. fused against two launches, off the shipped scale
@pytest.mark.parametrize("obs_dtype", (torch.float32, torch.float64))
@pytest.mark.parametrize("name", OFF_SCALE)
def test_gpu_fused_rollout_equals_two_launches(name, obs_dtype):
    """20 ticks of step_with_actor() (k_actor_h, then the tick) against step_many(20, source="actor") (the tile inside k_rollout):
    the state is bit-equal -- the existing shipped-weights statement, on weights whose scale factor is not 1."""
    w = S.actor_sets()[name]
    assert M.Packed(w).e != [0, 0]
    x, y = filled_pair(w, obs_dtype)
    for _ in range(20):
        x.step_with_actor()
    y.step_many(20, source="actor")
    for k in FIELDS:
        assert torch.equal(x.state_field(k), y.state_field(k)), k
    assert torch.equal(x.obs, y.obs)
    assert x.metrics() == y.metrics() and x.metrics()["ctl_steps"] > 20 * 10 * N_ENVS


# ------------------------------------------------------------------ 5. critic_q: k_target_q<.., false> on every critic weight set
_critic_batch = []


def critic_batch():
    if not _critic_batch:
        from pve_mcc_amd.arrivals import synthetic_arrivals
        arr = synthetic_arrivals(N_ENVS, rate=1000.0, horizon_s=60.0, seed=5)
        _critic_batch.append(make_batch(arr, N_ENVS, 128, BACKEND, outputs=("obs_post", "reward", "flags", "env_out"),
                                        obs_dtype=torch.float32))
    return _critic_batch[0]


@pytest.mark.parametrize("name", list(S.critic_sets()))
def test_gpu_critic_q_on_every_weight_set(name):
    w = S.critic_sets()[name]
    rows, act7 = S.critic_rows()
    b = critic_batch()
    b.set_target_networks(critic=w)
    q = _np(b.critic_q(torch.as_tensor(np.array(rows)), torch.as_tensor(np.array(act7)))).astype(np.float64)
    b.synchronize()
    q64, spread = S.ref_q(w, rows, act7)
    qm = M.critic_split(w, rows, act7).astype(np.float64)
    bar = S.critic_bar(name, spread)
    d64, dm = float(np.abs(q - q64).max()), float(np.abs(q - qm).max())
    report("critic_q", name, "rows", spread, float(np.abs(qm - q64).max()), d64, dm, bar)
    assert np.all(np.isfinite(q)) and d64 <= bar and dm <= bar


# ------------------------------------------------------------------ 6. bootstrap_q: target actor x target critic
def check_bootstrap(b, label, aw, cw, st, flags):
    """bootstrap_q(state, flags) of the installed pair against float64 NumPy and the model on the evaluated rows.  States whose
    row 0 is all zero are a family of their own: the critic's input LayerNorm returns ln0_beta there, which is ~1e-6 right after
    initialisation -- limit (2) of include/pve_env.h, an activation in f16's subnormal range -- so their Q bar is 2 x the CPU
    model's own maximum on them where that exceeds the standard bar (split_half_scenarios.MODEL_BARS has the same rule)."""
    ev = TQ.evaluated(flags)
    q, a7 = b.bootstrap_q(torch.as_tensor(np.array(st)), torch.as_tensor(flags))
    b.synchronize()
    q, a7 = _np(q), _np(a7)
    assert np.all(q[~ev].view(np.uint32) == 0) and np.all(a7[~ev].view(np.uint32) == 0), "excluded rows must be exactly 0"
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(a7))
    q64, a64, q_bar, a_bar, info = S.ref_bootstrap(aw, cw, st[ev])
    qm, am = M.bootstrap_split(aw, cw, st[ev])
    da, dam, ma = (float(np.abs(x - y).max()) for x, y in ((a7[ev], a64), (a7[ev], am), (am, a64)))
    report("bootstrap a7", label, "states", info["spread_a"], ma, da, dam, a_bar)
    assert da <= a_bar and dam <= a_bar
    zero0 = ~st[ev][:, 0].any(axis=1)
    assert 1 <= zero0.sum() < len(zero0) // 2
    for fam, m in (("row 0 not zero", ~zero0), ("row 0 all zero", zero0)):
        dq, dqm, mq = (float(np.abs(x[m] - y[m]).max()) for x, y in ((q[ev], q64), (q[ev], qm), (qm, q64)))
        bar = max(q_bar, 2.0 * mq) if fam == "row 0 all zero" else q_bar
        report("bootstrap q", label, fam, info["spread_q"], mq, dq, dqm, bar)
        assert dq <= bar and dqm <= bar, (fam, dq, dqm, bar, info)


def bootstrap_flags(n):
    """every 5th row uncontrolled, every 7th behind Done: the accepted rows of a 64-row chunk make one full tile and a partial one"""
    f = np.full(n, _capi.F_ALIVE | _capi.F_CTL, np.int32)
    f[::5] = _capi.F_ALIVE
    f[3::7] |= _capi.F_DONE
    return f


@pytest.mark.parametrize("name", list(S.bootstrap_pairs()))
def test_gpu_bootstrap_q_on_target_pairs(name):
    aw, cw = S.bootstrap_pairs()[name]
    st = S.bootstrap_states()
    flags = bootstrap_flags(len(st))
    walk = TQ.walk(len(st), TQ.evaluated(flags), TQ.BOOT_PER_CU)
    # more than one tile per wave: a full tile inside the chunk's loop, the left-over rows in the pass behind the last chunk
    assert max(len(t) for t in walk.tiles) >= 2 and walk.partial_tiles >= 1 and walk.max_pending > 32
    b = critic_batch()
    b.set_target_networks(actor=aw, critic=cw)
    check_bootstrap(b, name, aw, cw, st, flags)


# ------------------------------------------------------------------ 7. after install(): the learner's own weights, held to a reference
def test_gpu_install_after_a_learner_step_vs_numpy():
    """One Learner.step on a block of freshly initialised networks, install(), then act() and bootstrap_q() against float64 NumPy
    ON THE READ-BACK WEIGHTS: what test_gpu_install_equals_weights_copied_through_the_host (two device paths, bit for bit)
    leaves out."""
    from tests import learner_scenarios as LS
    b, slots = A.planted_batch(BACKEND, N_ENVS, seed=43, obs_dtype=torch.float32)
    fa, fc = LN.flat_weights(S.fresh(1), False), LN.flat_weights(S.fresh(1, True), True)
    lrn = LN.Learner(b, fa, fc, **LS.HYPER)
    lrn.step(*(torch.as_tensor(x).to(b.device) for x in LS.minibatches(64, 1, seed=21)))
    lrn.install()
    aw, taw, tcw = (LN.unflat_weights(_np(x).copy(), c) for x, c in ((lrn.actor_weights, False), (lrn.target_actor_weights, False),
                                                                     (lrn.target_critic_weights, True)))
    assert not np.array_equal(aw["w1"], S.fresh(1)["w1"]) and not np.array_equal(tcw["w2"], S.fresh(1, True)["w2"])
    assert M.Packed(aw).e != [0, 0] and M.Packed(tcw).e != [0, 0]
    rows = S.actor_rows()["graph"]
    a = A.actions_of_planted_rows(b, slots, rows)
    a64, spread = S.ref_actions(aw, rows)
    am = M.actor_split(aw, rows).astype(np.float64)
    bar = S.action_bar(spread)
    d64, dm = float(np.abs(a - a64).max()), float(np.abs(a - am).max())
    report("act", "installed after one step", "graph", spread, float(np.abs(am - a64).max()), d64, dm, bar)
    assert d64 <= bar and dm <= bar
    st = S.bootstrap_states()
    check_bootstrap(b, "installed after one step", taw, tcw, st, bootstrap_flags(len(st)))

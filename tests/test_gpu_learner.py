"""The learner step on the GPU (pve_learner_init / pve_learner_step, k_learner_step) against a g++ build of the same header
(tests/learner_host, held to LearnerModel and to autograd in tests/test_learner.py): the whole parameter block, the losses and
the gradients, bit for bit.  Then its use: install() against weights copied through the host, and one pass of roll-out ->
n-step transitions -> replay memory -> sample -> step."""
import functools

import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from pve_mcc_amd import Learner, PveError, ReplayMemory
from pve_mcc_amd import learner as LN
from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import learner_scenarios as S
from tests.critic_scenarios import load_critic_golden
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
GAMMA0 = float(np.tanh(6.0 / 12.0) * 0.9)
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
_batch = {}


def batch():
    """one small float32 handle: the learner only takes the device and the stream from it"""
    if "b" not in _batch:
        arr = synthetic_arrivals(3, rate=500.0, horizon_s=20.0, seed=3)
        _batch["b"] = make_batch(arr, 3, 64, "hip", outputs=("obs_post", "flags"), obs_dtype=torch.float32)
    return _batch["b"]


def dev(x, b):
    return torch.as_tensor(np.ascontiguousarray(x)).to(b.device)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def device_learner(b, zero_units=False, warmed=False, threads=0):
    lrn = Learner(b, *S.nets(zero_units), block_threads=threads, **S.HYPER)
    if warmed:
        lrn.load_state_dict({"params": torch.from_numpy(S.warmed_block(zero_units).copy())})
    return lrn


@functools.lru_cache(maxsize=None)
def host_run(bsz, n, warmed, zero_units, critic_only=False):
    """the host build on the scenario's minibatches -> (inputs, block after, losses, grads); computed once, read-only"""
    P = S.warmed_block(zero_units).copy() if warmed else S.host_block(S.nets(zero_units))
    inp = S.minibatches(bsz, n, seed=7 * bsz + n)
    losses, grads = S.host_step(P, *inp, critic_only=critic_only)
    for a in inp + (P, losses, grads):
        a.setflags(write=False)
    return inp, P, losses, grads


def check_block(lrn, P, what):
    got = _np(lrn.params)
    if not np.array_equal(S.bits32(got), S.bits32(P)):
        names = ("actor", "critic", "target_actor", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic", "powers", "steps", "grad")
        offs = (LN.ACTOR, LN.CRITIC, LN.TARGET_ACTOR, LN.TARGET_CRITIC, LN.M_ACTOR, LN.V_ACTOR, LN.M_CRITIC, LN.V_CRITIC, LN.POWERS, LN.STEPS,
                LN.GRAD, LN.N_FLOATS)
        bad = {n: int((S.bits32(got[a:z]) != S.bits32(P[a:z])).sum()) for n, a, z in zip(names, offs[:-1], offs[1:])}
        raise AssertionError("%s: the block differs from the host build's: words per segment %s" % (what, bad))


# ------------------------------------------------------------------ 1. the kernel == the host build, bit for bit
@pytest.mark.parametrize("bsz", [1, 63, 64, 65, 128, 200])
def test_gpu_step_equals_the_host_build(bsz):
    """1, 3 and 17 minibatches, 256 and 1024 threads; fresh and warmed state with the fixture's and the exact-zero-ReLU networks
    at 3 minibatches, fresh / fixture and warmed / exact-zero at 1 and 17.  Every minibatch of 3 rows or more holds the all-zero
    rows.  Sub-blocks: 64 rows in the critic step, 32 in the actor step (63, 65 and 200 leave ragged tails; 128 and 200 run both loops
    past their first iteration)."""
    b = batch()
    for n in (1, 3, 17):
        combos = ((False, False), (True, False), (False, True), (True, True)) if n == 3 else ((False, False), (True, True))
        for warmed, zero_units in combos:
            inp, P, losses, grads = host_run(bsz, n, warmed, zero_units)
            rows, act7, target = (dev(x, b) for x in inp)
            for threads in (256, 1024):
                what = "batch %d, %d minibatches, %d threads, warmed %s, zero units %s" % (bsz, n, threads, warmed, zero_units)
                lrn = device_learner(b, zero_units, warmed, threads)
                if not warmed:
                    check_block(lrn, S.host_block(S.nets(zero_units)), what + " (init)")
                got_l, got_g = lrn.step(rows, act7, target, losses=True, grads=True)
                assert got_l.shape == (n, 2) and got_g.shape == (n, LN.N_GRADS)
                assert np.array_equal(S.bits32(_np(got_l)), S.bits32(losses)), what
                assert np.array_equal(S.bits32(_np(got_g)), S.bits32(grads)), what
                check_block(lrn, P, what)
                assert lrn.steps() == n + (5 if warmed else 0)
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(grads))


def test_gpu_default_geometry_and_optional_outputs():
    """block_threads = 0 (1024), a single [batch, ..] minibatch, no losses / grads asked for: the same block"""
    b = batch()
    inp, P, _, _ = host_run(65, 1, True, False)
    lrn = device_learner(b, warmed=True)
    assert lrn.step(*(dev(x[0], b) for x in inp)) == (None, None)
    check_block(lrn, P, "defaults")
    with pytest.raises(PveError, match="block_threads"):
        device_learner(b, threads=96)
    with pytest.raises(PveError, match="float32"):
        lrn.step(dev(inp[0].astype(np.float64), b), dev(inp[1], b), dev(inp[2], b))
    with pytest.raises(PveError, match="needed"):
        lrn.step(dev(inp[0], b), dev(inp[1][:, :-1], b), dev(inp[2], b))


def test_gpu_three_minibatches_equal_three_calls():
    b = batch()
    rows, act7, target = (dev(x, b) for x in S.minibatches(37, 3, seed=5))
    one, three = device_learner(b, warmed=True), device_learner(b, warmed=True)
    l3, g3 = three.step(rows, act7, target, losses=True, grads=True)
    for k in range(3):
        l1, g1 = one.step(rows[k], act7[k], target[k], losses=True, grads=True)
        assert same_bits(l1[0], l3[k]) and same_bits(g1[0], g3[k])
    assert same_bits(one.params, three.params)


@pytest.mark.parametrize("warmed", [False, True])
def test_gpu_critic_only(warmed):
    b = batch()
    inp, P, losses, grads = host_run(50, 3, warmed, False, critic_only=True)
    lrn = device_learner(b, warmed=warmed, threads=512)
    before = lrn.params.clone()
    got_l, got_g = lrn.step(*(dev(x, b) for x in inp), losses=True, grads=True, critic_only=True)
    check_block(lrn, P, "critic only")
    assert np.array_equal(S.bits32(_np(got_l)), S.bits32(losses)) and np.array_equal(S.bits32(_np(got_g)), S.bits32(grads))
    for o, n in ((LN.ACTOR, 6396), (LN.TARGET_ACTOR, 6396), (LN.M_ACTOR, 6396), (LN.V_ACTOR, 6396), (LN.POWERS, 2), (LN.GRAD_ACTOR, 6396)):
        assert same_bits(lrn.params[o:o + n], before[o:o + n])
    assert not same_bits(lrn.critic_weights, before[LN.CRITIC:LN.CRITIC + LN.N_CRITIC])
    # the flag belongs to the call: the next full step moves the actor
    lrn.step(*(dev(x[:1], b) for x in inp))
    assert not same_bits(lrn.actor_weights, before[LN.ACTOR:LN.ACTOR + LN.N_ACTOR])


def test_gpu_state_dict_round_trip():
    b = batch()
    inp, P, _, _ = host_run(64, 3, False, False)
    lrn = device_learner(b)
    lrn.step(*(dev(x[:2], b) for x in inp))
    twin = device_learner(b, zero_units=True)
    twin.load_state_dict(lrn.state_dict())
    for l in (lrn, twin):
        l.step(*(dev(x[2:], b) for x in inp))
        check_block(l, P, "state_dict")


# ------------------------------------------------------------------ 2. install(): the block's segments feed set_actor / set_target_networks
def test_gpu_install_equals_weights_copied_through_the_host():
    g = load_critic_golden()
    E = 3
    arr = synthetic_arrivals(E, rate=1300.0, horizon_s=45.0, seed=11)
    results = []
    for through_host in (False, True):
        b = make_batch(arr, E, 128, "hip", outputs=TRAIN_OUTS)
        b.reset()
        b.set_actor(flat_weights(load_weights()))
        b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
        b.step_many(150, source="actor", trajectory=True)
        lrn = device_learner(b)
        lrn.step(*(dev(x, b) for x in S.minibatches(64, 4, seed=9)))
        if through_host:
            b.set_actor(_np(lrn.actor_weights).copy())
            b.set_target_networks(_np(lrn.target_actor_weights).copy(), _np(lrn.target_critic_weights).copy())
        else:
            lrn.install()
        b.step_many(2, source="actor", trajectory=True)
        q, a7 = b.bootstrap_q()
        results.append((b.act().clone(), q.clone(), a7.clone(), lrn.actor_weights.clone()))
        b.synchronize()
    (act0, q0, a70, w0), (act1, q1, a71, w1) = results
    assert same_bits(w0, w1) and not np.array_equal(_np(w0), S.fixture().actor)
    assert same_bits(act0, act1) and same_bits(q0, q1) and same_bits(a70, a71)
    assert (act0 != 0).any() and (q0 != 0).any()


# ------------------------------------------------------------------ 3. one pass: roll-out -> n-step -> memory -> sample -> step
def rollout(with_learner):
    g = load_critic_golden()
    E = 3
    arr = synthetic_arrivals(E, rate=1300.0, horizon_s=45.0, seed=11)
    b = make_batch(arr, E, 128, "hip", outputs=TRAIN_OUTS)
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
    b.set_exploration(0.2, seed=77)
    b.step_many(250, source="actor", trajectory=True)            # (to steady state: vehicles take ~150 ticks to cross)
    sets = [b.alloc_trajectory(20), b.alloc_trajectory(20)]
    mem = ReplayMemory(b, buffer_size=301, batch_size=64, seed=77)
    lrn = device_learner(b) if with_learner else None
    kept, samples, learned = [], [], []
    prev = None
    for call in range(2):
        t = b.step_many(20, source="actor", trajectory=sets[call])
        rec, idx, total = b.nstep_transitions(GAMMA0, prev=prev, max_records=E * 128 * 20)
        mem.add(rec, total)
        rows, act7, target, seq = mem.sample(2, check=False)
        samples.append((rows, act7, target, seq))
        if lrn is not None:
            learned.append(lrn.step(rows, act7, target, losses=True, grads=True))
        prev = t
        kept.append(({k: v.clone() for k, v in t.items()}, rec.clone(), idx.clone(), total.clone()))
    b.synchronize()
    fields = {f: b.state_field(f).clone() for f in ("p", "v", "a", "id", "meta", "step")}
    return kept, samples, learned, fields, lrn


def test_gpu_rollout_to_learner_step():
    kept, samples, learned, fields, lrn = rollout(True)
    kept0, samples0, _, fields0, _ = rollout(False)
    # no bit of the roll-out differs from the same roll-out without a learner
    for (t, rec, idx, total), (t0, rec0, idx0, total0) in zip(kept, kept0):
        for k in t:
            assert same_bits(t[k], t0[k]), k
        n = int(total)
        assert n == int(total0) and n > 0 and torch.equal(idx[:n], idx0[:n]) and same_bits(rec[:n], rec0[:n])
    for f in fields:
        assert torch.equal(fields[f], fields0[f]), f
    for s, s0 in zip(samples, samples0):
        for x, y in zip(s, s0):
            assert same_bits(x, y)
    # the learner equals the host build on the sampled tensors
    P = S.host_block(S.nets())
    for (rows, act7, target, seq), (got_l, got_g) in zip(samples, learned):
        assert (_np(seq) >= 0).all() and rows.shape == (2, 64, 28)
        losses, grads = S.host_step(P, _np(rows), _np(act7), _np(target))
        assert np.array_equal(S.bits32(_np(got_l)), S.bits32(losses)) and np.array_equal(S.bits32(_np(got_g)), S.bits32(grads))
    check_block(lrn, P, "roll-out")
    assert lrn.steps() == 4 and np.all(np.isfinite(P))

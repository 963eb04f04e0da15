"""The wide learner step on the GPU (pve_learner_step_wide: k_learner_slice / k_learner_apply, Learner.step_wide) against the g++
build of the same header (tests/learner_wide_host, held to learn_steps, to the stated combine and to LearnerModel in
tests/test_learner_wide.py): the whole parameter block, the losses and the gradients, bit for bit -- whatever the grid, the threads
and the workspace's earlier contents.  Then its use behind the replay memory."""
import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from pve_mcc_amd import Learner, PveError, ReplayMemory
from pve_mcc_amd import learner as LN
from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import learner_scenarios as S
from tests import learner_wide_scenarios as W
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


def check_block(lrn, P, what, nan_ok=False):
    """the device block against the host build's, bit for bit, no NaN in either; nan_ok (family D of the range only): equal NaN
    masks, every other word bit-equal (learner_scenarios.same_words).  Differences are reported per segment."""
    S.check_words(_np(lrn.params), P, what + ": the block", nan_ok=nan_ok)


# ------------------------------------------------------------------ 1. the kernels == the host build, bit for bit
# (batch, minibatches, threads, warmed, zero-unit networks): every value of every axis occurs; every minibatch holds the all-zero
# rows in each slice of 3 rows or more.  1: a single row; 128: one full slice; 129: a second slice of one row; 300: a last slice of
# 44 rows (less than one critic sub-block of 64, more than one actor sub-block of 32); 449: 3 slices + 65 rows (one row past a
# critic sub-block); 1024: 8 full slices.
CASES = [(1, 1, 256, False, False), (1, 3, 1024, True, True), (128, 3, 256, True, False), (129, 1, 1024, False, True),
         (129, 3, 256, True, True), (300, 3, 1024, False, False), (300, 1, 256, True, True), (449, 3, 256, False, True),
         (449, 1, 1024, True, False), (1024, 1, 1024, False, False), (1024, 3, 256, True, True)]


@pytest.mark.parametrize("bsz,n,threads,warmed,zero_units", CASES)
def test_gpu_wide_step_equals_the_host_build(bsz, n, threads, warmed, zero_units):
    b = batch()
    inp, P, losses, grads = W.host_run(bsz, n, warmed, zero_units)
    what = "batch %d, %d minibatches, %d threads, warmed %s, zero units %s" % (bsz, n, threads, warmed, zero_units)
    lrn = device_learner(b, zero_units, warmed, threads)
    got_l, got_g = lrn.step_wide(*(dev(x, b) for x in inp), losses=True, grads=True)
    assert got_l.shape == (n, 2) and got_g.shape == (n, LN.N_GRADS)
    assert np.array_equal(S.bits32(_np(got_l)), S.bits32(losses)), what
    assert np.array_equal(S.bits32(_np(got_g)), S.bits32(grads)), what
    check_block(lrn, P, what)
    assert lrn.steps() == n + (5 if warmed else 0) and np.all(np.isfinite(P)) and np.all(np.isfinite(grads))


# ------------------------------------------------------------------ 1b. the same across the float32 range (learner_scenarios: A .. F)
@pytest.mark.parametrize("name", list(S.RANGE_CASES))
def test_gpu_wide_range_equals_the_host_build(name):
    """The cases of tests/test_gpu_learner.py through the slice and apply kernels: 130 rows (two slices, the second of 2 rows) and
    300 rows (three, the last of 44), two grids each (one workgroup per slice; one or two workgroups walking the slices), 256 and
    1024 threads.  Family C here: three minibatches from the long run's state at step 850 (b1p subnormal, moving) and at step
    1 100 (its fixed point).  D alone may hold NaN: equal NaN masks, every other word bit-equal."""
    b = batch()
    c = S.range_case(name)
    for bsz, threads, groups in ((130, 256, 0), (130, 1024, 1), (300, 1024, 0), (300, 256, 2)):
        inp, P, losses, grads = W.range_run(name, bsz)
        what = "%s, batch %d, %d threads, groups %d" % (name, bsz, threads, groups)
        lrn = Learner(b, *S.range_networks(name), block_threads=threads, **c["hyper"])
        lrn.load_state_dict({"params": torch.from_numpy(S.range_start(name).copy())})
        got_l, got_g = lrn.step_wide(*(dev(x, b) for x in inp), losses=True, grads=True, groups=groups)
        S.check_words(_np(got_l), losses, what + ": losses", nan_ok=c["nan_ok"])
        S.check_words(_np(got_g), grads, what + ": grads", nan_ok=c["nan_ok"])
        check_block(lrn, P, what, nan_ok=c["nan_ok"])
        assert lrn.steps() == int(P[LN.STEPS:LN.STEPS + 1].view(np.int32)[0])
        print("%s: equal to the host build (%d subnormal words, %d NaN, %d infinities in block and gradients)"
              % (what, S.count_subnormal(P[:LN.STEPS]) + S.count_subnormal(grads), S.count_nan(P) + S.count_nan(grads),
                 int(np.isinf(P).sum() + np.isinf(grads).sum())))


# ------------------------------------------------------------------ 2. up to one slice: the existing kernel's bits
@pytest.mark.parametrize("bsz", [1, 64, 128])
def test_gpu_one_slice_equals_step(bsz):
    b = batch()
    rows, act7, target = (dev(x, b) for x in S.minibatches(bsz, 3, seed=60 + bsz))
    old, new = device_learner(b, warmed=True), device_learner(b, warmed=True)
    l1, g1 = old.step(rows, act7, target, losses=True, grads=True)
    l2, g2 = new.step_wide(rows, act7, target, losses=True, grads=True)
    assert same_bits(l1, l2) and same_bits(g1, g2) and same_bits(old.params, new.params)
    assert new.steps() == 8


# ------------------------------------------------------------------ 3. no bit depends on the grid
def test_gpu_grid_independence():
    """640 rows = 5 slices: one workgroup per slice (0 and 5), one workgroup walking all five (1), two walking 3 and 2 (2)"""
    b = batch()
    inp, P, losses, grads = W.host_run(640, 2, True, False)
    rows, act7, target = (dev(x, b) for x in inp)
    for groups in (0, 1, 2, 5):
        lrn = device_learner(b, warmed=True)
        got_l, got_g = lrn.step_wide(rows, act7, target, losses=True, grads=True, groups=groups)
        assert np.array_equal(S.bits32(_np(got_l)), S.bits32(losses)) and np.array_equal(S.bits32(_np(got_g)), S.bits32(grads)), groups
        check_block(lrn, P, "groups %d" % groups)
    with pytest.raises(PveError, match="groups"):
        lrn.step_wide(rows, act7, target, groups=-1)


# ------------------------------------------------------------------ 4. minibatches per call, critic only
def test_gpu_three_minibatches_equal_three_calls():
    b = batch()
    rows, act7, target = (dev(x, b) for x in W.minibatches(300, 3, seed=5))
    one, three = device_learner(b, warmed=True), device_learner(b, warmed=True)
    l3, g3 = three.step_wide(rows, act7, target, losses=True, grads=True)
    for k in range(3):
        l1, g1 = one.step_wide(rows[k], act7[k], target[k], losses=True, grads=True)
        assert same_bits(l1[0], l3[k]) and same_bits(g1[0], g3[k])
    assert same_bits(one.params, three.params)


@pytest.mark.parametrize("warmed", [False, True])
def test_gpu_critic_only(warmed):
    b = batch()
    inp, P, losses, grads = W.host_run(300, 3, warmed, False, critic_only=True)
    lrn = device_learner(b, warmed=warmed, threads=512)
    before = lrn.params.clone()
    got_l, got_g = lrn.step_wide(*(dev(x, b) for x in inp), losses=True, grads=True, critic_only=True)
    check_block(lrn, P, "critic only")
    assert np.array_equal(S.bits32(_np(got_l)), S.bits32(losses)) and np.array_equal(S.bits32(_np(got_g)), S.bits32(grads))
    for o, n in ((LN.ACTOR, 6396), (LN.TARGET_ACTOR, 6396), (LN.M_ACTOR, 6396), (LN.V_ACTOR, 6396), (LN.POWERS, 2), (LN.GRAD_ACTOR, 6396)):
        assert same_bits(lrn.params[o:o + n], before[o:o + n])
    assert not same_bits(lrn.critic_weights, before[LN.CRITIC:LN.CRITIC + LN.N_CRITIC])
    assert bool((got_g[:, LN.N_CRITIC:] == 0).all()) and bool((got_l[:, 1] == 0).all()) and lrn.steps() == 3 + (5 if warmed else 0)
    # the flag belongs to the call: the next full step moves the actor
    lrn.step_wide(*(dev(x[:1], b) for x in inp))
    assert not same_bits(lrn.actor_weights, before[LN.ACTOR:LN.ACTOR + LN.N_ACTOR])


# ------------------------------------------------------------------ 5. the workspace needs no initialisation
def test_gpu_workspace_full_of_nan_changes_no_bit():
    b = batch()
    inp, P, losses, grads = W.host_run(300, 3, True, True)
    lrn = device_learner(b, zero_units=True, warmed=True)
    with b._own_stream():
        lrn._wide_work = torch.full((LN.wide_floats(300) + 8,), float("nan"), dtype=torch.float32, device=b.device)
    work = lrn._wide_work
    got_l, got_g = lrn.step_wide(*(dev(x, b) for x in inp), losses=True, grads=True)
    assert lrn._wide_work is work                                  # (the cached workspace was large enough: it is the one used)
    assert np.array_equal(S.bits32(_np(got_l)), S.bits32(losses)) and np.array_equal(S.bits32(_np(got_g)), S.bits32(grads))
    check_block(lrn, P, "NaN workspace")
    assert bool(torch.isnan(work[LN.wide_floats(300):]).all())     # nothing was written behind the batch's rows
    # a larger batch grows it, a smaller one keeps it
    lrn.step_wide(*(dev(x, b) for x in W.minibatches(449, 1, seed=1)))
    assert lrn._wide_work is not work and lrn._wide_work.numel() == LN.wide_floats(449)
    grown = lrn._wide_work
    lrn.step_wide(*(dev(x, b) for x in W.minibatches(129, 1, seed=1)))
    assert lrn._wide_work is grown


# ------------------------------------------------------------------ 6. the two entry points on one block
def test_gpu_wide_and_narrow_steps_interleave():
    b = batch()
    big, small = W.minibatches(300, 1, seed=21), S.minibatches(100, 1, seed=22)
    big2 = W.minibatches(449, 1, seed=23)
    P = S.warmed_block().copy()
    ref = [W.host_step_wide(P, *big), S.host_step(P, *small), W.host_step_wide(P, *big2)]
    lrn = device_learner(b, warmed=True)
    got = [lrn.step_wide(*(dev(x, b) for x in big), losses=True, grads=True), lrn.step(*(dev(x, b) for x in small), losses=True, grads=True),
           lrn.step_wide(*(dev(x, b) for x in big2), losses=True, grads=True)]
    for (l, g), (rl, rg) in zip(got, ref):
        assert np.array_equal(S.bits32(_np(l)), S.bits32(rl)) and np.array_equal(S.bits32(_np(g)), S.bits32(rg))
    check_block(lrn, P, "step_wide, step, step_wide")
    assert lrn.steps() == 8


# ------------------------------------------------------------------ 7. from the pipeline: roll-out -> n-step -> memory -> sample -> step_wide
def test_gpu_rollout_to_wide_step():
    g = load_critic_golden()
    E = 3
    arr = synthetic_arrivals(E, rate=1300.0, horizon_s=45.0, seed=11)
    b = make_batch(arr, E, 128, "hip", outputs=TRAIN_OUTS)
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
    b.set_exploration(0.2, seed=77)
    b.step_many(250, source="actor", trajectory=True)            # (to steady state: vehicles take ~150 ticks to cross)
    traj = b.alloc_trajectory(20)
    b.step_many(20, source="actor", trajectory=traj)
    rec, idx, total = b.nstep_transitions(GAMMA0, max_records=E * 128 * 20)
    mem = ReplayMemory(b, buffer_size=2001, batch_size=512, seed=77)
    mem.add(rec, total)
    rows, act7, target, seq = mem.sample(2, check=False)
    lrn = device_learner(b)
    got_l, got_g = lrn.step_wide(rows, act7, target, losses=True, grads=True)
    assert rows.shape == (2, 512, 28) and (_np(seq) >= 0).all() and int(total) > 0
    P = S.host_block(S.nets())
    losses, grads = W.host_step_wide(P, _np(rows), _np(act7), _np(target))
    assert np.array_equal(S.bits32(_np(got_l)), S.bits32(losses)) and np.array_equal(S.bits32(_np(got_g)), S.bits32(grads))
    check_block(lrn, P, "roll-out")
    assert lrn.steps() == 2 and np.all(np.isfinite(P))
    # the batch then acts with those weights
    lrn.install()
    assert torch.equal(b._actor_w, lrn.actor_weights) and not np.array_equal(_np(lrn.actor_weights), S.fixture().actor)
    b.step_many(2, source="actor", trajectory=True)
    b.synchronize()
    assert bool(torch.isfinite(b.act()).all()) and bool((b.act() != 0).any())

"""The learner step on the GPU (pve_learner_init / pve_learner_step, k_learner_step) against a g++ build of the same header
(tests/learner_host, held to LearnerModel and to autograd in tests/test_learner.py): the whole parameter block, the losses and
the gradients, bit for bit -- on the fixture's magnitudes and across the float32 range (subnormal gradients, moments and beta
powers, overflow, hyper-parameters at the ends of their ranges: tests/learner_scenarios.py, families A .. F).  Then its use:
install() against weights copied through the host, and one pass of roll-out -> n-step transitions -> replay memory -> sample ->
step."""
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


def check_block(lrn, P, what, nan_ok=False):
    """the device block against the host build's, bit for bit, no NaN in either; nan_ok (family D of the range only): equal NaN
    masks, every other word bit-equal (learner_scenarios.same_words).  Differences are reported per segment."""
    S.check_words(_np(lrn.params), P, what + ": the block", nan_ok=nan_ok)


def range_learner(b, name, threads):
    """a Learner at the start of a case of learner_scenarios.RANGE_CASES, with the case's hyper-parameters: a fresh state comes
    from pve_learner_init (and is compared), any other is loaded"""
    c = S.range_case(name)
    lrn = Learner(b, *S.range_networks(name), block_threads=threads, **c["hyper"])
    if c["warmed"] or c["long"]:
        lrn.load_state_dict({"params": torch.from_numpy(S.range_start(name).copy())})
    else:
        check_block(lrn, S.range_start(name), name + " (init)")
    return lrn


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


# ------------------------------------------------------------------ 1b. the same across the float32 range (learner_scenarios: A .. F)
@pytest.mark.parametrize("name", list(S.RANGE_CASES))
def test_gpu_range_equals_the_host_build(name):
    """Subnormal gradients and moments (A), the state of a long run with a subnormal b1p (C), overflow (D), hyper-parameters at the
    ends of their ranges (E), squares that underflow in the input LayerNorm (F): block, losses and gradients bit for bit at 256
    and 1024 threads.  tests/test_learner.py asserts that the host results are in the regime.  D alone may hold NaN: there the
    NaN masks are equal and every other word, infinities included, is bit-equal."""
    b = batch()
    c = S.range_case(name)
    inp, P, losses, grads = S.range_run(name)
    rows, act7, target = (dev(x, b) for x in inp)
    for threads in (256, 1024):
        what = "%s, %d threads" % (name, threads)
        lrn = range_learner(b, name, threads)
        got_l, got_g = lrn.step(rows, act7, target, losses=True, grads=True)
        S.check_words(_np(got_l), losses, what + ": losses", nan_ok=c["nan_ok"])
        S.check_words(_np(got_g), grads, what + ": grads", nan_ok=c["nan_ok"])
        check_block(lrn, P, what, nan_ok=c["nan_ok"])
        assert lrn.steps() == int(P[LN.STEPS:LN.STEPS + 1].view(np.int32)[0])
        print("%s: equal to the host build (%d subnormal words, %d NaN, %d infinities in block and gradients)"
              % (what, S.count_subnormal(P[:LN.STEPS]) + S.count_subnormal(grads), S.count_nan(P) + S.count_nan(grads),
                 int(np.isinf(P).sum() + np.isinf(grads).sum())))


def test_gpu_long_run_equals_the_host_build():
    """Family C: 1 100 steps of batch 2 in 22 calls of 50 minibatches.  The block after call 17 (step 850: b1p subnormal and still
    moving) and after call 22 (step 1 100: b1p at its fixed point of 4 quanta) equals the host build's; then the policy of that
    state is installed: act() equals the act() of the same weights copied through the host."""
    b = batch()
    rows, act7, target = (dev(x, b) for x in S.long_run_inputs())
    host = S.long_run()
    lrn = device_learner(b)
    for call in range(S.LONG_STEPS // S.LONG_CALL):
        a = call * S.LONG_CALL
        lrn.step(rows[a:a + S.LONG_CALL], act7[a:a + S.LONG_CALL], target[a:a + S.LONG_CALL])
        if a + S.LONG_CALL in (S.LONG_MOVING, S.LONG_STEPS):
            check_block(lrn, host[a + S.LONG_CALL], "long run, step %d" % (a + S.LONG_CALL))
            print("long run, step %d: equal to the host build, b1p %.6e" % (a + S.LONG_CALL, host[a + S.LONG_CALL][LN.POWERS]))
    assert lrn.steps() == S.LONG_STEPS and _np(lrn.params)[LN.POWERS] == S.B1P_FIXED_POINT
    state = {"params": torch.from_numpy(_np(lrn.params).copy())}
    g = load_critic_golden()
    arr = synthetic_arrivals(3, rate=1300.0, horizon_s=45.0, seed=11)
    acts = []
    for through_host in (False, True):
        e = make_batch(arr, 3, 64, "hip", outputs=TRAIN_OUTS)
        e.reset()
        e.set_actor(flat_weights(load_weights()))
        e.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
        e.step_many(150, source="actor", trajectory=True)
        there = device_learner(e)
        there.load_state_dict(state)
        if through_host:
            e.set_actor(_np(there.actor_weights).copy())
        else:
            there.install()
        acts.append(e.act().clone())
        e.synchronize()
    assert same_bits(acts[0], acts[1]) and bool((acts[0] != 0).any()) and bool(torch.isfinite(acts[0]).all())
    assert not np.array_equal(_np(lrn.actor_weights), S.fixture().actor)


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

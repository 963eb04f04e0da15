"""The binding's gateway and its stream rule on the GPU: the shortest sequence that crosses every kind of call -- actor, tick,
target networks, critic, bootstrap Q, roll-out, n-step transitions, replay memory, learner -- on a batch with a side stream of
its own, on a batch that follows a current side stream, and on a batch on the default stream: the same bits everywhere.  What
the rule protects is the order of every kernel against the torch work (allocations, fills, copies) around it; the batch with
its own stream is where act() used to re-bind the stream.  The refusals of tensors on the wrong device type are here too (the
CPU suite has no second device type): tests/test_binding_gateway.py holds the other refusals."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from pve_mcc_amd import Learner, PrioritizedReplayMemory, PveError, ReplayMemory
from pve_mcc_amd.arrivals import synthetic_arrivals
from pve_mcc_amd.batched import BatchedIntersections
from tests import learner_scenarios as LS
from tests.critic_scenarios import load_critic_golden

pytestmark = pytest.mark.gpu
OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
GAMMA = float(np.tanh(6.0 / 12.0) * 0.9)


def make(stream):
    arr = synthetic_arrivals(4, rate=1500.0, horizon_s=40.0, seed=11)
    return BatchedIntersections(4, 64, arr, device="cuda", outputs=OUTS, stream=stream)


@functools.lru_cache(maxsize=None)
def run(mode):
    """The sequence on a 4-environment, 64-slot batch -> every output as host bytes.  mode: "own" (the batch has a side
    stream, torch's current stream is the default one), "current" (no stream of its own, everything inside a side stream's
    context) or "default".  Inputs go in as host arrays: the calls upload them on the stream the kernels run on.  The test's
    own reads of views that a later call overwrites are fenced on both sides (a caller's duty: outputs belong to the batch's
    stream); nothing else in the sequence waits."""
    side = torch.cuda.Stream() if mode != "default" else None
    g = load_critic_golden()
    res = {}

    def copy_of(view):
        b.synchronize()
        c = view.clone()
        torch.cuda.synchronize()
        return c
    with torch.cuda.stream(side) if mode == "current" else contextlib.nullcontext():
        b = make(side if mode == "own" else None)
        torch.cuda.synchronize()                             # (the constructor's fills and uploads ran on the current stream)
        b.reset()
        torch.cuda.synchronize()                             # (... and so does reset()'s zeroing of the views)
        b.set_actor(flat_weights(load_weights()))
        for _ in range(100):                                # (traffic: controlled vehicles in every environment)
            b.step_with_actor()
        res["act"] = copy_of(b.act())
        res["reward"] = copy_of(b.step_with_actor()["reward"])
        b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
        act7 = np.linspace(-3.0, 3.0, 4 * 64 * 7, dtype=np.float32).reshape(4, 64, 7)
        res["critic_q"] = b.critic_q(b.obs, act7)
        res["boot_q"], res["boot_act7"] = b.bootstrap_q()
        tr = b.step_many(4, trajectory=True)
        res["traj_reward"], res["traj_flags"] = tr["reward"], tr["flags"]
        rec, idx, total = b.nstep_transitions(GAMMA, window=2)
        res["records"], res["index"] = rec, idx
        assert total == rec.shape[0] >= 4, total
        mem = ReplayMemory(b, buffer_size=total + 1, batch_size=4, seed=3)
        mem.add(rec)
        rows, a7, target, seq = mem.sample(1)
        res["rows"], res["sampled_act7"], res["target"], res["seq"] = rows, a7, target, seq
        lrn = Learner(b, *LS.nets(), **LS.HYPER)
        res["losses"], res["grads"] = lrn.step(rows, a7, target, losses=True, grads=True)
        res["params"] = lrn.params
        b.synchronize()
    torch.cuda.synchronize()
    assert int((res["act"] != 0).sum()) > 0 and lrn.steps() == 1
    return {k: v.cpu().numpy().tobytes() for k, v in res.items()}


@pytest.mark.parametrize("mode", ["own", "current"])
def test_gpu_every_kind_of_call_on_a_side_stream_equals_the_default_stream(mode):
    got, want = run(mode), run("default")
    assert sorted(got) == sorted(want) and len(want) == 16
    for k in want:
        assert got[k] == want[k], k


def refused(message, fn, *args, **kw):
    with pytest.raises(PveError) as e:
        fn(*args, **kw)
    assert str(e.value) == message, str(e.value)


def test_gpu_tensors_on_the_wrong_device_type_are_refused():
    b = make(None)
    b.reset()
    tr = b.step_many(2, trajectory=True)
    b.synchronize()
    dev = tr["flags"].device
    rows, act7 = torch.zeros(3, 28, dtype=torch.float64), torch.zeros(3, 7)
    refused("out must be a contiguous float32 device tensor of 3 elements", b.critic_q, rows, act7, out=torch.zeros(3))
    refused("actions_out must be a contiguous float32 device tensor of 21 elements", b.bootstrap_q, torch.zeros(3, 7, 28), actions_out=torch.zeros(3, 7))
    refused("out must be a contiguous float64 device tensor of shape (2, 1, 14)", b.rollout_stats, tr, out=torch.zeros(2, 1, 14, dtype=torch.float64))
    refused("totals must be a contiguous float64 device tensor of shape (1, 14)", b.rollout_stats, tr, totals=torch.zeros(1, 14, dtype=torch.float64))
    refused("out must be a contiguous float64 device tensor of shape (1, 12)", b.metrics_by_group, out=torch.zeros(1, 12, dtype=torch.float64))
    refused("rollout_stats: flags must be a torch.int32 device tensor of shape (2, 4, 64)", b.rollout_stats, dict(tr, flags=tr["flags"].cpu()))
    refused("nstep_transitions: cur['reward'] must be a torch.float64 device tensor of shape (2, 4, 64)", b.nstep_transitions, GAMMA,
            cur=dict(tr, reward=tr["reward"].cpu()), q=torch.zeros(2, 4, 64))
    mem = ReplayMemory(b, buffer_size=17, batch_size=4)
    refused("ReplayMemory.add: records are on cpu, the memory is on %s" % dev, mem.add, torch.zeros(5, 36))
    pm = PrioritizedReplayMemory(b, buffer_size=320, batch_size=8, learn_start=0, steps=1000)
    seq, q = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, device=dev)
    word = "PrioritizedReplayMemory.update_priority: %s must be a %s tensor on " + str(dev) + " with seq's element count"
    refused(word % ("seq", "torch.int64"), pm.update_priority, seq.cpu(), q)
    refused(word % ("q", "torch.float32"), pm.update_priority, seq, q.cpu())
    refused(word % ("target", "torch.float32"), pm.update_priority, seq, q, q.cpu())
    lrn = Learner(b, *LS.nets(), **LS.HYPER)
    r, a, t = (torch.zeros(s, device=dev) for s in ((1, 4, 28), (1, 4, 7), (1, 4)))
    for method in ("step", "step_wide"):
        fn = getattr(lrn, method)
        refused("Learner.%s: rows must be a float32 tensor on %s" % (method, dev), fn, r.cpu(), a, t)
        refused("Learner.%s: target must be a float32 tensor on %s" % (method, dev), fn, r, a, t.cpu())
        refused("Learner.%s: losses must be a contiguous float32 device tensor [1, 2]" % method, fn, r, a, t, losses=torch.zeros(1, 2))
        refused("Learner.%s: grads must be a contiguous float32 device tensor [1, 13234]" % method, fn, r, a, t, grads=torch.zeros(1, 13234))
    b.synchronize()
    assert lrn.steps() == 0

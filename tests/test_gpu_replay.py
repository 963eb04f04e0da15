"""The replay memory on the GPU (pve_replay_append / pve_replay_sample; csrc/pve_replay.h) against ReplayModel
(pve_mcc_amd/replay.py, pinned to the reference's ReplayBuffer and to its own specification in tests/test_replay.py).  Nothing
is arithmetic: rings, rows, actions and targets are compared as uint32 bit patterns, record numbers and state as int64."""
import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from pve_mcc_amd import PveError, ReplayMemory, ReplayModel
from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import replay_scenarios as S
from tests.critic_scenarios import load_critic_golden
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
GAMMA0 = float(np.tanh(6.0 / 12.0) * 0.9)
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
_batch = {}


def batch():
    """one small float32 handle: the memory only takes the device and the stream from it (and critic_q its row type)"""
    if "b" not in _batch:
        arr = synthetic_arrivals(3, rate=500.0, horizon_s=20.0, seed=3)
        _batch["b"] = make_batch(arr, 3, 64, "hip", outputs=("obs_post", "flags"), obs_dtype=torch.float32)
    return _batch["b"]


def dev(x, b):
    return torch.as_tensor(np.ascontiguousarray(x)).to(b.device)


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


class LibrarySpy:
    """the loaded library with one entry point's arguments recorded on the way through"""

    def __init__(self, lib, name):
        self.lib, self.name, self.calls = lib, name, []

    def __getattr__(self, attr):
        fn = getattr(self.lib, attr)
        if attr != self.name:
            return fn

        def recorded(*args):
            self.calls.append(args)
            return fn(*args)
        return recorded


def check_ring(mem, model):
    state = _np(mem.state)
    assert state.dtype == np.int64 and (int(state[0]), int(state[1])) == (model.written, model.draws), (state, model.written, model.draws)
    assert np.array_equal(S.bits32(_np(mem.store)), S.bits32(model.store))
    assert mem.count() == model.count() and mem.live() == model.live()


def check_sample(got, want):
    for g, w in zip(got[:3], want[:3]):
        assert tuple(g.shape) == w.shape and g.dtype == torch.float32 and g.is_contiguous()
        assert np.array_equal(S.bits32(_np(g)), S.bits32(w))
    assert got[3].dtype == torch.int64 and np.array_equal(_np(got[3]), want[3])


# ------------------------------------------------------------------ 1. append
@pytest.mark.parametrize("capacity", [7, 64, 319, 4099])
def test_gpu_append(capacity):
    b = batch()
    chunks = S.append_chunks(capacity) + ([5000] if capacity == 4099 else [])      # (5000 into 4099: several workgroups, a wrap inside)
    for threads in (64, 256, 1024):
        mem = ReplayMemory(b, buffer_size=capacity + 1, batch_size=1, block_threads=threads)
        model = ReplayModel(buffer_size=capacity + 1, batch_size=1)
        fed = 0
        for n in chunks:                                    # total = NULL: all of the chunk
            rec = S.payload(n, fed)
            mem.add(dev(rec, b))
            model.add(rec)
            fed += n
            check_ring(mem, model)
        # a device-side count below, equal to and above n_max (and a negative one)
        for n_max, total in ((50, 20), (50, 50), (50, 70), (50, -3), (capacity + 9, capacity + 3), (2 * capacity + 1, 5 * capacity)):
            rec = S.payload(n_max, fed)
            mem.add(dev(rec, b), total=torch.tensor(total, dtype=torch.int64, device=b.device))
            model.add(rec, total=total)
            fed += n_max
            check_ring(mem, model)
        assert model.count() > 5 * capacity
        mem.reset()
        model.reset()
        assert mem.count() == 0 and mem.live() == 0
        rec = S.payload(3)
        mem.add(dev(rec, b))
        model.add(rec)
        assert np.array_equal(S.bits32(_np(mem.store)[:3]), S.bits32(rec)) and mem.count() == 3
    with pytest.raises(PveError, match="block_threads"):
        ReplayMemory(b, buffer_size=capacity + 1, batch_size=1, block_threads=96).add(dev(S.payload(1), b))


# ------------------------------------------------------------------ 2. sample
@pytest.mark.parametrize("bsz", [1, 63, 64, 65, 128, 1024])
def test_gpu_sample(bsz):
    b = batch()
    capacity = 4099 if bsz > 128 else 319
    for threads in (64, 256, 1024):                         # (the same model every time: the result does not depend on the geometry)
        mem = ReplayMemory(b, buffer_size=capacity + 1, batch_size=bsz, seed=(1 << 33) + 5, block_threads=threads)
        model = ReplayModel(buffer_size=capacity + 1, batch_size=bsz, seed=(1 << 33) + 5)
        fed = 0

        def feed(n):
            nonlocal fed
            rec = S.payload(n, fed)
            mem.add(dev(rec, b))
            model.add(rec)
            fed += n
        if bsz > 1:
            feed(bsz - 1)                                   # L < batch: nothing is drawn
            got = mem.sample(3, check=False)
            check_sample(got, model.sample(3, check=False))
            assert (_np(got[3]) == -1).all() and int(mem.state[2]) == bsz - 1 == model.status
            with pytest.raises(PveError, match="fewer"):
                mem.sample()
            check_ring(mem, model)                          # (draws unchanged)
            feed(1)
        else:
            got = mem.sample(2, check=False)
            assert (_np(got[3]) == -1).all() and int(mem.state[2]) == 0
            feed(1)
        got = mem.sample()                                  # L == batch: every live record exactly once
        check_sample(got, model.sample())
        assert np.array_equal(np.sort(_np(got[3])[0]), np.arange(bsz)) and int(mem.state[2]) == bsz
        feed(capacity - bsz - 1)                            # not yet wrapped (one slot still empty)
        for wrapped in (False, True):
            for n_batches in (1, 3, 17):
                got = mem.sample(n_batches)
                want = model.sample(n_batches)
                check_sample(got, want)
                seq = _np(got[3])
                assert all(len(set(row.tolist())) == bsz for row in seq)
                assert seq.min() >= model.written - model.live() and seq.max() < model.written
                rec = np.concatenate([_np(got[0]), _np(got[1]), _np(got[2])[..., None]], axis=-1).reshape(-1, 36)
                assert np.array_equal(S.bits32(rec), S.bits32(S.payload_of(seq)))      # (the drawn records ARE those numbers)
            check_ring(mem, model)
            if not wrapped:
                feed(capacity // 2 + 3)
                assert model.written > capacity
    # sample(3) = three sample(1) calls
    twin = ReplayMemory(b, buffer_size=capacity + 1, batch_size=bsz, seed=(1 << 33) + 5)
    twin.store.copy_(mem.store)
    twin.state.copy_(mem.state)
    three = mem.sample(3)
    for k in range(3):
        one = twin.sample(1)
        for x, y in zip(three, one):
            assert same_bits(x[k], y[0])
    assert torch.equal(mem.state, twin.state)


# ------------------------------------------------------------------ 3. use: the sampled tensors feed critic_q without a copy
def test_gpu_sampled_batches_feed_the_critic():
    g = load_critic_golden()
    b = batch()
    b.set_target_networks(critic=g.weights["target_critic"])
    n = 700
    rec = np.concatenate([g.given_rows[:n], g.given_act7[:n], np.arange(n, dtype=np.float32)[:, None]], axis=1).astype(np.float32)
    mem = ReplayMemory(b, buffer_size=512, batch_size=128, seed=4)
    model = ReplayModel(buffer_size=512, batch_size=128, seed=4)
    mem.add(dev(rec, b))
    model.add(rec)
    rows, act7, target, seq = mem.sample(5)
    want = model.sample(5)
    check_sample((rows, act7, target, seq), want)
    # no copy on the way into pve_critic_forward: the pointers critic_q hands to the library are the sampled tensors' own
    spy = LibrarySpy(b.lib, "pve_critic_forward")
    b.lib = spy
    b._fns.pop("pve_critic_forward", None)                   # (the gateway keeps the entry points it has bound: look this one up anew)
    try:
        q = b.critic_q(rows, act7)
    finally:
        b.lib = spy.lib
        b._fns.pop("pve_critic_forward", None)
    assert len(spy.calls) == 1
    _, rows_ptr, act7_ptr, q_ptr, n_rows = spy.calls[0]      # (the gateway passes addresses as plain integers)
    assert (rows_ptr, act7_ptr, q_ptr, n_rows) == (rows.data_ptr(), act7.data_ptr(), q.data_ptr(), 5 * 128)
    q_model = b.critic_q(dev(want[0], b), dev(want[1], b))
    assert q.shape == (5, 128) and torch.equal(q.view(torch.int32), q_model.view(torch.int32))
    assert torch.isfinite(q).all() and q.std() > 0


# ------------------------------------------------------------------ 4. a real noisy closed-loop roll-out, two chained calls
def rollout(with_memory):
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
    mem = ReplayMemory(b, buffer_size=301, batch_size=64, seed=77) if with_memory else None       # (same seed as the noise: the tag)
    kept, samples = [], []
    prev = None
    for call in range(2):
        t = b.step_many(20, source="actor", trajectory=sets[call])
        rec, idx, total = b.nstep_transitions(GAMMA0, prev=prev, max_records=E * 128 * 20)
        if mem is not None:
            mem.add(rec, total)
            samples.append(mem.sample(2, check=False))
        prev = t
        kept.append(({k: v.clone() for k, v in t.items()}, rec.clone(), idx.clone(), total.clone()))
    b.synchronize()
    fields = {f: b.state_field(f).clone() for f in ("p", "v", "a", "id", "meta", "step")}
    return kept, samples, fields, mem


def test_gpu_real_rollout_into_the_memory():
    kept, samples, fields, mem = rollout(True)
    kept0, _, fields0, _ = rollout(False)
    # no bit of the roll-out's outputs differs from the same roll-out without the memory
    for (t, rec, idx, total), (t0, rec0, idx0, total0) in zip(kept, kept0):
        for k in t:
            assert same_bits(t[k], t0[k]), k
        n = int(total)
        assert n == int(total0) and torch.equal(idx[:n], idx0[:n]) and same_bits(rec[:n], rec0[:n])
    for f in fields:
        assert torch.equal(fields[f], fields0[f]), f
    # the memory equals the model fed from the copied-back records
    model = ReplayModel(buffer_size=301, batch_size=64, seed=77)
    totals = []
    for (t, rec, idx, total), got in zip(kept, samples):
        model.add(_np(rec), total=int(total))
        totals.append(int(total))
        check_sample(got, model.sample(2, check=False))
    print("transitions per call: %s, capacity 300" % totals)
    assert totals[0] > 0 and sum(totals) > 300 and totals[1] < 3 * 128 * 20          # (wrapped; the count cuts the chunk short)
    check_ring(mem, model)
    assert (_np(samples[1][3]) >= 0).all() and model.draws >= 2

"""The rank-based prioritised memory on the GPU (pve_prio_reset / _rank / _sample / _update; csrc/pve_prio.h) against
PrioritizedReplayModel (pve_mcc_amd/replay.py, pinned to the recorded reference and to its own rules in tests/test_prio_replay.py):
order, seq, rank, rows, prio, pseq and pstate bit for bit; the importance weight against the float64 expression at 1e-5 relative
(tests/prio_scenarios.py: WEIGHT_BAR)."""
import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from pve_mcc_amd import Learner, PrioritizedReplayMemory, PrioritizedReplayModel, PveError, replay
from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import prio_scenarios as S
from tests.critic_scenarios import load_critic_golden
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
GAMMA0 = float(np.tanh(6.0 / 12.0) * 0.9)
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
_batch = {}
_worst = {"weight": 0.0}


def batch():
    """one small float32 handle: the memory only takes the device and the stream from it (and critic_q its row type)"""
    if "b" not in _batch:
        arr = synthetic_arrivals(3, rate=500.0, horizon_s=20.0, seed=3)
        _batch["b"] = make_batch(arr, 3, 64, "hip", outputs=("obs_post", "flags"), obs_dtype=torch.float32)
    return _batch["b"]


def dev(x, b):
    return torch.as_tensor(np.ascontiguousarray(x)).to(b.device)


def pair(capacity, bsz, threads=0, **kw):
    kw = dict(dict(learn_start=0, steps=1000, seed=(1 << 33) + 5), **kw)
    mem = PrioritizedReplayMemory(batch(), buffer_size=capacity, batch_size=bsz, block_threads=threads, **kw)
    return mem, PrioritizedReplayModel(buffer_size=capacity, batch_size=bsz, **kw)


def feed(mem, model, n, zeros=False):
    rec = np.zeros((n, 36), np.float32) if zeros else S.payload(n, model.written)
    mem.add(dev(rec, mem.batch))
    model.add(rec)


def update(mem, model, seq, q, target=None):
    b = mem.batch
    mem.update_priority(dev(seq, b), dev(q, b), None if target is None else dev(target, b))
    model.update_priority(seq, q, target)


def check_store(mem, model, order=True):
    assert np.array_equal(_np(mem.prio).view(np.uint32), model.prio) and np.array_equal(_np(mem.pseq), model.pseq)
    assert np.array_equal(_np(mem.pstate), model.pstate), (_np(mem.pstate), model.pstate)
    assert int(mem.state[0]) == model.written and np.array_equal(S.bits32(_np(mem.store)), S.bits32(model.store))
    if order:
        L = model.live()
        assert np.array_equal(_np(mem.order)[:L], model.order[:L])


def check_sample(got, want, ab):
    for g, w in zip(got[:3], want[:3]):
        assert tuple(g.shape) == w.shape and g.dtype == torch.float32 and g.is_contiguous()
        assert np.array_equal(S.bits32(_np(g)), S.bits32(w))
    assert got[3].dtype == torch.int64 and np.array_equal(_np(got[3]), want[3])
    assert got[4].dtype == torch.int32 and np.array_equal(_np(got[4]), want[4])
    weight = _np(got[5]).astype(np.float64)
    assert got[5].dtype == torch.float32 and weight.shape == want[5].shape
    if (want[3] < 0).all():
        assert not weight.any()
        return
    w64 = replay.prio_weights(want[4], np.float32(ab))
    rel = float(np.abs(weight / w64 - 1).max())
    _worst["weight"] = max(_worst["weight"], rel)
    assert rel <= S.WEIGHT_BAR, rel


# ------------------------------------------------------------------ 1. the ranking: live counts x key patterns
@pytest.mark.parametrize("pattern", S.PATTERNS)
@pytest.mark.parametrize("live", S.LIVE_COUNTS)
def test_gpu_rank(live, pattern):
    capacity, written = S.geometry(live)
    threads = (0, 64, 256, 1024)[(S.LIVE_COUNTS.index(live) + S.PATTERNS.index(pattern)) % 4]
    mem, model = pair(capacity, 2, threads)
    rng = np.random.default_rng(live)
    feed(mem, model, written, zeros=True)
    assert model.live() == live
    ids, q = S.pattern_update(pattern, model.live_seq(), rng)
    if len(ids):
        update(mem, model, ids, q)
    mem.scratch.fill_(0x5A5A5A5A)                            # (whatever the scratch holds)
    mem.order.fill_(-7)
    order = _np(mem.rank())
    want = model.rank()
    assert np.array_equal(order[:live], want) and (order[live:] == -7).all()
    assert np.array_equal(np.sort(order[:live]), np.arange(live))
    check_store(mem, model)
    assert int(mem.pstate[replay.PLIVE]) == live and mem.count() == written
    if live >= 4097 and pattern == "digits":                 # the same memory under every workgroup size
        for t in (64, 256, 1024):
            twin = PrioritizedReplayMemory(batch(), buffer_size=capacity, batch_size=2, learn_start=0, steps=1000, block_threads=t)
            for name in ("store", "state", "prio", "pseq", "pstate"):
                getattr(twin, name).copy_(getattr(mem, name))
            assert np.array_equal(_np(twin.rank())[:live], want), t
    with pytest.raises(PveError, match="block_threads"):
        PrioritizedReplayMemory(batch(), buffer_size=capacity, batch_size=2, learn_start=0, steps=1000, block_threads=96).rank()


# ------------------------------------------------------------------ 2. the draw at every partition boundary
@pytest.mark.parametrize("threads", [64, 256, 1024])
@pytest.mark.parametrize("capacity,bsz", [(320, 8), (4096, 128)])
def test_gpu_sample_at_partition_boundaries(capacity, bsz, threads):
    mem, model = pair(capacity, bsz, threads)
    rng = np.random.default_rng(capacity + threads)
    lives = [int(x) for x in np.unique(np.concatenate([model.part_from, model.part_from - 1]))]
    assert lives[-1] == capacity and lives[0] == model.min_live - 1 and len(lives) == 64
    seen_parts = set()
    for i, live in enumerate(lives):
        feed(mem, model, live - model.live())
        n_batches, beta = (1, 3, 40)[i % 3], (0.5, 0.77, 1.0)[i % 3]
        ab = model._alpha_beta(beta, ValueError)
        got = mem.sample(n_batches, beta=beta, check=False)
        want = model.sample(n_batches, beta=beta, check=False)
        check_sample(got, want, ab)
        check_store(mem, model)
        seen_parts.add(int(model.pstate[replay.PPART]))
        if live < model.min_live:
            assert (want[3] == -1).all() and model.pstate[replay.PDRAWS] == 0
            with pytest.raises(PveError, match="fewer"):
                mem.sample(beta=beta)
            continue
        seq = want[3].ravel()
        pick = rng.integers(0, len(seq), max(len(seq) // 2, 1))      # priorities for half of what was drawn, some ids twice
        update(mem, model, seq[pick], rng.normal(0, 2, len(pick)).astype(np.float32), want[2].ravel()[pick])
        check_store(mem, model, order=False)
    assert seen_parts == set(range(33)) and model.pstate[replay.PDRAWS] > 0
    # wrap-around appends between update and sample, capacity not dividing the adds; then sample(3) = three sample(1) calls
    oldest = model.written - capacity + np.arange(5)          # (overwritten by the appends below: stale ids)
    feed(mem, model, capacity // 3 + 1)
    ids = np.concatenate([want[3].ravel(), oldest, [-1]])
    update(mem, model, ids, rng.normal(0, 2, len(ids)).astype(np.float32))
    assert model.pstate[replay.PIGNORED] > 0 and model.written % capacity != 0
    check_sample(mem.sample(3, beta=0.9), model.sample(3, beta=0.9), model._alpha_beta(0.9, ValueError))
    check_store(mem, model)
    twin = PrioritizedReplayMemory(batch(), buffer_size=capacity, batch_size=bsz, learn_start=0, steps=1000, seed=(1 << 33) + 5)
    for name in ("store", "state", "prio", "pseq", "pstate"):
        getattr(twin, name).copy_(getattr(mem, name))
    three = mem.sample(3, beta=0.9)
    for k in range(3):
        one = twin.sample(1, beta=0.9)
        for x, y in zip(three, one):
            assert torch.equal(x[k].contiguous().view(torch.uint8), y[0].contiguous().view(torch.uint8))
    assert torch.equal(mem.pstate, twin.pstate)
    mem.reset()
    model.reset()
    check_store(mem, model, order=False)
    assert mem.count() == 0 and (_np(mem.pseq) == -1).all()


# ------------------------------------------------------------------ 3. one large update: duplicates, stale ids, -1
@pytest.mark.parametrize("threads", [0, 64, 1024])
def test_gpu_update_4096_ids(threads):
    mem, model = pair(4096, 128, threads)
    feed(mem, model, 4096 + 1500, zeros=True)
    rng = np.random.default_rng(threads)
    seq, q, target = S.messy_update(model.written, 4096, 4096, rng)
    live = (seq >= model.written - 4096) & (seq < model.written)
    assert (seq == -1).any() and (seq[~live] >= 0).any() and len(np.unique(seq[live])) < int(live.sum())
    update(mem, model, seq, q, target)
    check_store(mem, model, order=False)
    assert model.pstate[replay.PIGNORED] == int((~live).sum()) > 0
    update(mem, model, seq[::3], q[::3])                     # no target: |q|; the old values are replaced, not maxed
    check_store(mem, model, order=False)
    check_sample(mem.sample(2, beta=1.0), model.sample(2, beta=1.0), model._alpha_beta(1.0, ValueError))
    check_store(mem, model)


# ------------------------------------------------------------------ 4. the weight at the reference's size
def test_gpu_weight_at_500000():
    """capacity 500 000 full (zero records, all NEW): ranks reach 500 000; the device's float32 weight against the float64
    expression on the ranks the device returned.  The largest deviation of this module's runs is printed for profiles/."""
    mem = PrioritizedReplayMemory(batch(), buffer_size=500000, batch_size=128, learn_start=0, steps=1000, seed=3)
    b = mem.batch
    mem.add(torch.zeros(500000, 36, dtype=torch.float32, device=b.device))
    worst = 0.0
    for beta in (0.5, 1.0):
        ab = mem._alpha_beta(beta, PveError)
        rows, act7, target, seq, rank, weight = mem.sample(64, beta=beta)
        rank, weight, seq = _np(rank), _np(weight).astype(np.float64), _np(seq)
        want = replay.prio_draw_ranks(3, int(mem.pstate[replay.PDRAWS]) - 64 + np.arange(64, dtype=np.uint64), mem.ends[31], 500000)
        assert np.array_equal(rank, want) and rank.max() > 450000
        assert np.array_equal(seq, 500000 - rank.astype(np.int64))              # all NEW: rank r is the r-th newest
        worst = max(worst, float(np.abs(weight / replay.prio_weights(rank, ab) - 1).max()))
    _worst["weight"] = max(_worst["weight"], worst)
    print("PRIO_WEIGHT max relative deviation, ranks to 500000: %.3e; all tests of this module so far: %.3e (bar %.0e)"
          % (worst, _worst["weight"], S.WEIGHT_BAR))
    assert worst <= S.WEIGHT_BAR


# ------------------------------------------------------------------ 5. the closed loop
def test_gpu_closed_loop():
    """roll-out -> nstep_transitions -> add -> sample -> critic_q -> update_priority -> sample -> Learner.step; the model is fed
    the device's records and q, copied back; the second sample is bit-equal."""
    from tests import learner_scenarios as LS
    g = load_critic_golden()
    E = 3
    arr = synthetic_arrivals(E, rate=1300.0, horizon_s=45.0, seed=11)
    b = make_batch(arr, E, 128, "hip", outputs=TRAIN_OUTS)
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
    b.set_exploration(0.2, seed=77)
    b.step_many(250, source="actor", trajectory=True)
    bq = batch()
    bq.set_target_networks(critic=g.weights["target_critic"])
    kw = dict(buffer_size=320, batch_size=8, seed=77, learn_start=20, steps=5000)
    mem, model = PrioritizedReplayMemory(b, **kw), PrioritizedReplayModel(**kw)
    sets = [b.alloc_trajectory(20), b.alloc_trajectory(20)]
    prev, totals = None, []
    for call in range(3):
        t = b.step_many(20, source="actor", trajectory=sets[call % 2])
        rec, idx, total = b.nstep_transitions(GAMMA0, prev=prev, max_records=300)
        mem.add(rec, total)
        model.add(_np(rec), total=int(total))
        totals.append(min(int(total), 300))
        prev = t
        beta = model.beta_at(model.count())
        ab = model._alpha_beta(beta, ValueError)
        rows, act7, target, seq, rank, weight = mem.sample(4, beta=beta, check=False)
        check_sample((rows, act7, target, seq, rank, weight), model.sample(4, beta=beta, check=False), ab)
        if model.live() < model.min_live:
            continue
        q = bq.critic_q(rows, act7)
        mem.update_priority(seq, q, target)
        model.update_priority(_np(seq), _np(q), _np(target))
        check_store(mem, model, order=False)
        second = mem.sample(4, beta=beta)
        check_sample(second, model.sample(4, beta=beta), ab)
        check_store(mem, model)
    print("transitions per call: %s into capacity 320" % totals)
    assert sum(totals) > 320 and model.pstate[replay.PDRAWS] >= 8 and int((model.pseq >= 0).sum()) > 16
    assert len(np.unique(model.prio[model.pseq >= 0])) > 16 and torch.isfinite(q).all()
    lrn = Learner(b, *LS.nets(), **LS.HYPER)
    losses, _ = lrn.step(second[0], second[1], second[2], losses=True, grads=True)
    assert lrn.steps() == 4 and bool(torch.isfinite(losses).all()) and bool(torch.isfinite(lrn.params).all())

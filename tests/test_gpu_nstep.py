"""The n-step transition pass on the GPU (pve_nstep_scan / pve_nstep_gather; csrc/pve_nstep.h) against its NumPy restatement
(pve_mcc_amd/nstep.py, pinned to the reference's own bookkeeping in tests/test_nstep.py).  Everything is exact: code and
index equal, targets and records bit-equal.  The pass is stateless, so most cases run on the hand-made trajectories of
tests/nstep_scenarios.py; one case is a real closed-loop roll-out."""
import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from pve_mcc_amd import PveError, _capi, nstep
from pve_mcc_amd.arrivals import synthetic_arrivals
from pve_mcc_amd.batched import PipelinedIntersections
from tests import nstep_scenarios as S
from tests.critic_scenarios import load_critic_golden
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
GAMMA0 = float(np.tanh(6.0 / 12.0) * 0.9)
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
E = 3
_batches = {}


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def bits32(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def batch(cap, f32, n_envs=E):
    """One small handle per (capacity, row type): the pass only takes n_envs, capacity, the row type and the stream from it"""
    if (cap, f32, n_envs) not in _batches:
        arr = synthetic_arrivals(n_envs, rate=500.0, horizon_s=20.0, seed=3)
        _batches[cap, f32, n_envs] = make_batch(arr, n_envs, cap, "hip", outputs=("obs_post", "flags"),
                                                obs_dtype=torch.float32 if f32 else torch.float64)
    return _batches[cap, f32, n_envs]


def dev(seg, b):
    return {k: torch.as_tensor(np.ascontiguousarray(v)).to(b.device) for k, v in seg.items()}


def run_both(b, tr, a, n, prev_from, window=13, tail=False, gamma=GAMMA0, **kw):
    """the device pass and nstep.py over ticks a .. a + n - 1 of a trajectory (prev = ticks prev_from .. a - 1)"""
    cur = S.blocks(tr, a, a + n)
    prev = None if prev_from is None else S.blocks(tr, prev_from, a)
    first, q = S.obs_before(tr, a), tr.q[a:a + n]
    rec, idx, total = b.nstep_transitions(gamma, window=window, cur=dev(cur, b), prev=None if prev is None else dev(prev, b),
                                          obs_first=None if prev is not None else torch.as_tensor(first).to(b.device),
                                          q=torch.as_tensor(q).to(b.device), tail=tail, **kw)
    target, code, _ = (_np(x) for x in b._nstep_last)
    b.synchronize()
    want_t, want_c, n_back = nstep.scan(cur, gamma, window, prev=prev, obs_first=first, q=q, tail=tail)
    want_rec, want_idx = nstep.records(cur, want_t, want_c, n_back, prev=prev, obs_first=first)
    return (_np(rec), _np(idx), total, target, code), (want_rec, want_idx, want_t, want_c)


def check(got, want):
    rec, idx, total, target, code = got
    want_rec, want_idx, want_t, want_c = want
    assert np.array_equal(code, want_c)
    assert np.array_equal(bits(target)[want_c != 0], bits(want_t)[want_c != 0])
    assert int(total) == len(want_rec) and rec.shape == want_rec.shape and idx.shape == want_idx.shape
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(bits32(rec), bits32(want_rec))
    return len(want_rec)


# ------------------------------------------------------------------ 1. hand-made trajectories, every capacity and row type
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("cap", [64, 128, 256])
def test_gpu_hand_made(cap, f32):
    tr = S.make_trajectory(60, E=E, K=cap, seed=4, f32=f32)
    b = batch(cap, f32)
    for n in (1, 12, 13, 14, 40):
        m0 = check(*run_both(b, tr, 0, n, None))                # from the first tick, nothing in front
        m1 = check(*run_both(b, tr, 20, n, 0))                  # windows reaching back into prev
        m2 = check(*run_both(b, tr, 20, n, 5, tail=True))
        print("cap %d f32 %d n_ticks %2d: %d / %d / %d records" % (cap, f32, n, m0, m1, m2))
        assert m1 > 0 and m2 >= m1 and (m0 > 0 or n < 13)


@pytest.mark.parametrize("window", [1, 16, 2])
def test_gpu_windows(window):
    tr = S.make_trajectory(60, E=E, K=128, seed=4)
    b = batch(128, False)
    for tail in (False, True):
        assert check(*run_both(b, tr, 17, 23, 0, window=window, tail=tail, gamma=0.8)) > 0
        assert check(*run_both(b, tr, 0, 23, None, window=window, tail=tail, gamma=1.0)) > 0


# ------------------------------------------------------------------ 1b. k_nstep_offsets with runs of more than one group
@pytest.mark.parametrize("n,ragged", [(40, False), (5, True)])
def test_gpu_offsets_with_runs_of_several_groups(n, ragged):
    """k_nstep_offsets is ONE workgroup of 1024 threads, each owning per = ceil(n_groups / 1024) consecutive group counts; up
    to 1024 groups (every case above) per == 1.  67 intersections x 64 slots, ticks 20 .. 20 + n - 1 with 12 candidate ticks in
    front: 52 x 67 = 3484 groups (per = 4, threads 871 and up own nothing) and 17 x 67 = 1139 (per = 2, the last owning
    thread's run is cut short by n_groups, 454 threads own nothing)."""
    E67, cap = 67, 64
    tr = S.make_trajectory(60, E=E67, K=cap, seed=4)
    b = batch(cap, False, E67)
    got, want = run_both(b, tr, 20, n, 0)
    offsets = _np(b._nstep_last[2]).astype(np.int64)
    b.synchronize()
    M = check(got, want)
    n_groups = (12 + n) * E67 * cap // 64
    per = (n_groups + 1023) // 1024
    owners = (n_groups + per - 1) // per
    print("n_ticks %d: %d groups, per %d, %d threads without a group, %d records" % (n, n_groups, per, 1024 - owners, M))
    assert offsets.shape == (n_groups + 1,)
    assert per >= 2 and owners < 1024 and (n_groups % per != 0) == ragged
    counts = (got[4] != 0).reshape(n_groups, 64).sum(axis=1)
    assert counts.max() > 1 and (counts == 0).any() and M > 1024
    assert np.array_equal(offsets[:-1], np.cumsum(counts) - counts) and offsets[n_groups] == M == int(got[2])


# ------------------------------------------------------------------ 2. the cut-off
def test_gpu_max_records_and_total():
    tr = S.make_trajectory(60, E=E, K=128, seed=4, f32=True)
    b = batch(128, True)
    got, want = run_both(b, tr, 20, 20, 0)
    M = check(got, want)
    assert M > 300
    for m in (0, 1, 63, M // 2 + 1, M, M + 7):
        (rec, idx, total, _, _), _ = run_both(b, tr, 20, 20, 0, max_records=m)
        assert torch.is_tensor(total) and int(total) == M              # the true count, beyond the cut-off too
        k = min(m, M)
        assert rec.shape == (m, 36) and np.array_equal(bits32(rec[:k]), bits32(want[0][:k])) and np.array_equal(idx[:k], want[1][:k])


# ------------------------------------------------------------------ 3. the record order does not depend on the launch geometry
def test_gpu_order_is_independent_of_the_launch_geometry():
    tr = S.make_trajectory(60, E=E, K=64, seed=4)
    b = batch(64, False)
    base, want = run_both(b, tr, 20, 33, 0)
    assert check(base, want) > 0
    for threads in (64, 128, 512, 1024):
        got, _ = run_both(b, tr, 20, 33, 0, block_threads=threads)
        check(got, want)
    with pytest.raises(PveError):
        run_both(b, tr, 20, 33, 0, block_threads=96)


def test_gpu_argument_errors():
    tr = S.make_trajectory(60, E=E, K=64, seed=4)
    b = batch(64, False)
    for kw in (dict(window=0), dict(window=17), dict(gamma=1.01), dict(gamma=float("nan"))):
        with pytest.raises(PveError):
            run_both(b, tr, 20, 10, 0, **kw)
    with pytest.raises(PveError, match="window"):
        run_both(b, tr, 20, 10, 12)                              # 0 < n_prev < window
    with pytest.raises(PveError, match="trajectory"):
        b.nstep_transitions(0.8)                                 # nothing stepped yet


# ------------------------------------------------------------------ 4. one real roll-out, two chained calls
def test_gpu_real_rollout_chained():
    g = load_critic_golden()
    arr = synthetic_arrivals(E, rate=1300.0, horizon_s=45.0, seed=11)
    b = make_batch(arr, E, 64, "hip", outputs=TRAIN_OUTS)
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
    b.set_exploration(0.2, seed=77)
    b.step_many(250, source="actor", trajectory=True)            # (to steady state: vehicles take ~150 ticks to cross)
    sets = [b.alloc_trajectory(20), b.alloc_trajectory(20)]
    t1 = b.step_many(20, source="actor", trajectory=sets[0])
    first = b._last_traj[3].clone()
    q1, _ = b.bootstrap_q()
    r1, i1, n1 = b.nstep_transitions(GAMMA0)                     # prev=None: the windows open before the call are lost
    keep1 = {k: v.clone() for k, v in t1.items()}
    t2 = b.step_many(20, source="actor", trajectory=sets[1])
    q2, _ = b.bootstrap_q()
    keep2 = {k: v.clone() for k, v in t2.items()}
    fields = {f: b.state_field(f).clone() for f in ("p", "v", "a", "id", "meta", "step")}
    r2, i2, n2 = b.nstep_transitions(GAMMA0, prev=t1)
    r2t, i2t, n2t = b.nstep_transitions(GAMMA0, prev=t1, q=q2, tail=True)
    b.synchronize()
    # nothing the roll-out produced changed by a bit
    for keep, t in ((keep1, t1), (keep2, t2)):
        for k in keep:
            assert torch.equal(keep[k], t[k]), k
    for f in fields:
        assert torch.equal(fields[f], b.state_field(f)), f
    c1 = {k: _np(t1[k]) for k in nstep.KEYS}
    c2 = {k: _np(t2[k]) for k in nstep.KEYS}
    w1 = nstep.nstep_transitions(c1, GAMMA0, 13, obs_first=_np(first), q=_np(q1))
    w2 = nstep.nstep_transitions(c2, GAMMA0, 13, prev=c1, q=_np(q2))
    w2t = nstep.nstep_transitions(c2, GAMMA0, 13, prev=c1, q=_np(q2), tail=True)
    for (r, i, n), w, what in (((r1, i1, n1), w1, "first"), ((r2, i2, n2), w2, "second"), ((r2t, i2t, n2t), w2t, "second, tail")):
        print("%s call: %d transitions" % (what, w[2]))
        assert n == w[2] > 0 and np.array_equal(_np(i), w[1]) and np.array_equal(bits32(_np(r)), bits32(w[0]))
    done2 = (w2[1][:, 3] & nstep.DONE) != 0
    crossing = w2[1][:, 0] < 0
    flags = np.concatenate([c1["flags"], c2["flags"]])
    assert ((flags & _capi.F_DONE) != 0).sum() > 0 and done2.sum() > 0           # vehicles finish inside the two calls
    assert crossing.sum() > 0 and (w2[1][:, 0] >= 0).sum() > 0 and w2t[2] > w2[2]
    # steady state: one transition per controlled vehicle and tick of the second call that is 12 ticks old
    closes = (w2[1][:, 0] + (w2[1][:, 3] & 0xFF) - 1)
    assert closes.min() == 0 and closes.max() == 19
    # the stamps: a trajectory that is not the call right before cur is refused, and so is a stale cur
    with pytest.raises(PveError, match="right before"):
        b.nstep_transitions(GAMMA0, prev=t2)
    b.step_with_actor()
    with pytest.raises(PveError, match="latest"):
        b.nstep_transitions(GAMMA0)


def test_gpu_pipelined_matches_one_batch():
    g = load_critic_golden()
    arr = synthetic_arrivals(4, rate=1300.0, horizon_s=30.0, seed=12)
    results = []
    for make in (lambda: make_batch(arr, 4, 64, "hip", outputs=TRAIN_OUTS),
                 lambda: PipelinedIntersections(4, 64, arr, n_sub=2, device="cuda", outputs=TRAIN_OUTS)):
        b = make()
        b.reset()
        b.set_actor(flat_weights(load_weights()))
        b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
        b.step_many(150, source="actor", trajectory=True)
        t1 = b.step_many(15, source="actor", trajectory=True)
        b.nstep_transitions(0.8)
        b.step_many(15, source="actor", trajectory=True)
        rec, idx, total = b.nstep_transitions(0.8, prev=t1)
        b.synchronize()
        rec, idx = _np(rec), _np(idx)
        order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
        results.append((rec[order], idx[order], int(total)))
    (r0, i0, n0), (r1, i1, n1) = results
    assert n0 == n1 > 0 and np.array_equal(i0, i1) and np.array_equal(bits32(r0), bits32(r1))
    assert set(i1[:, 1]) == {0, 1, 2, 3}

"""The training side on the 4- / 8-lane layouts (and, by vehicle identity, on 12 lanes) on the GPU.

1. tests/nstep_identity_scenarios.py on the kernels, every scenario in both launch forms: the transitions of the device pass
   against the reference's per-vehicle buffers fed from the oracle (B), bit-equal to nstep.py on the read-back blocks, and
   independent of what the ring of trajectory buffers held before (C).  tests/test_nstep_identity.py runs the same bodies on the
   CPU emulator and pins the model to the reference's own fixture.
2. bootstrap_q and the closed loop over a geo roll-out's own state_pre / flags: what test_gpu_bootstrap_over_a_trajectory,
   test_gpu_real_rollout_chained and test_gpu_rollout_to_learner_step check for 12 lanes, for the shipped checkpoint's layout
   (lane_num 4, vm = 6, 128 slots, float32 rows) and for 8 lanes.

Bars: tests/test_gpu_critic.py's for the actions and Q (ACTION_TOL, boot_bar), the scenario module's for the rows and targets.
Every test prints what it measured before it asserts; profiles/nstep_layouts.txt holds one run's figures."""
import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from pve_mcc_amd import ReplayMemory, ReplayModel, _capi, critic, nstep
from pve_mcc_amd.arrivals import synthetic_arrivals, synthetic_intentions
from tests import learner_scenarios as LS
from tests import nstep_identity_scenarios as N
from tests.critic_scenarios import load_critic_golden
from tests.hip_adapter import _np, make_batch
from tests.parity_util import GoldenCase
from tests.test_gpu_critic import ACTION_TOL, boot_bar
from tests.test_gpu_learner import check_block, device_learner
from tests.test_gpu_replay import check_sample

pytestmark = pytest.mark.gpu
GAMMA0 = N.GAMMA0
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
E, CAP, PREFILL, TICKS, CALLS = 3, 128, 250, 20, 3
# the closed-loop rates of check_step_many_geo_actor at 128 slots
LAYOUTS = {4: dict(rate=1500.0, seed=191, ctor="geo_g4_rand_vm6"), 8: dict(rate=1300.0, seed=192, ctor=None)}


# ------------------------------------------------------------------ 1. identity and the dirty ring, every scenario
@pytest.mark.parametrize("form", sorted(N.LAUNCH_FORMS))
@pytest.mark.parametrize("name", sorted(N.SCENARIOS))
def test_gpu_identity_and_dirty_ring(name, form):
    clean = N.rollout(name, "hip", **N.LAUNCH_FORMS[form])
    N.check_identity(name, "hip", clean)
    dirty = N.rollout(name, "hip", dirty=True, **N.LAUNCH_FORMS[form])
    left = N.check_dirty(name, clean, dirty)
    print("%s %s: elements still holding the fill: %s" % (name, form, left))


# ------------------------------------------------------------------ 2. bootstrap_q and the closed loop on a geo roll-out
def closed_loop(lane_num, train):
    """prefill, then three chained closed-loop calls into a ring of two buffer sets; train: the target networks are installed
    and every call is followed by bootstrap_q() and nstep_transitions(), the last one by memory -> sample -> learner step"""
    lay = LAYOUTS[lane_num]
    g = load_critic_golden()
    cfg = dict(GoldenCase(lay["ctor"]).ctor) if lay["ctor"] else {}
    arr = synthetic_arrivals(E, rate=lay["rate"], horizon_s=(PREFILL + CALLS * TICKS) * 0.1 + 30, seed=lay["seed"], lane_num=lane_num)
    ch = synthetic_intentions(E, arr.shape[1], seed=lay["seed"], lane_num=lane_num) if lane_num == 8 else None
    b = make_batch(arr, E, CAP, "hip", outputs=TRAIN_OUTS, obs_dtype=torch.float32, lane_num=lane_num, intentions=ch, **cfg)
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    if train:
        b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
    b.set_exploration(0.2, seed=77)
    prev = b.step_many(PREFILL, source="actor", trajectory=True)               # (to steady state)
    b.synchronize()
    prev_host = {k: _np(prev[k][-N.WINDOW:]).copy() for k in TRAIN_OUTS}
    ring = [b.alloc_trajectory(TICKS), b.alloc_trajectory(TICKS)]
    calls, closing = [], None
    for i in range(CALLS):
        t = b.step_many(TICKS, source="actor", trajectory=ring[i & 1])
        b.synchronize()
        c = dict(blocks={k: _np(t[k]).copy() for k in TRAIN_OUTS}, prev=prev_host)
        if train:
            q, a7 = b.bootstrap_q()
            rec, idx, total = b.nstep_transitions(GAMMA0, prev=prev, max_records=E * CAP * TICKS)      # (total: a device tensor)
            b.synchronize()
            c.update(q=_np(q), a7=_np(a7), rec=_np(rec)[:int(total)], idx=_np(idx)[:int(total)], total=int(total))
            if i == CALLS - 1:
                mem = ReplayMemory(b, buffer_size=301, batch_size=64, seed=77)
                lrn = device_learner(b)
                mem.add(rec, total)
                sample = mem.sample(2, check=False)
                learned = lrn.step(*sample[:3], losses=True, grads=True)
                b.synchronize()
                closing = (sample, learned, lrn)
        calls.append(c)
        prev, prev_host = t, c["blocks"]
    fields = {f: _np(b.state_field(f)).copy() for f in N.STATE_FIELDS}
    return calls, fields, closing


@pytest.mark.parametrize("lane_num", [4, 8])
def test_gpu_bootstrap_and_closed_loop_on_a_geo_rollout(lane_num):
    g = load_critic_golden()
    calls, fields, (sample, learned, lrn) = closed_loop(lane_num, True)
    n_ev = n_done = n_rec = 0
    worst_a = worst_q = 0.0
    for i, c in enumerate(calls):
        state, flags = c["blocks"]["state_pre"], c["blocks"]["flags"]
        assert c["q"].shape == (TICKS, E, CAP) and c["a7"].shape == (TICKS, E, CAP, 7)
        ev = (flags & (_capi.F_CTL | _capi.F_DONE)) == _capi.F_CTL
        n_ev += int(ev.sum())
        n_done += int(((flags & _capi.F_CTL) != 0).sum() - ev.sum())
        # the oracle side: float64 NumPy on the read-back rows
        q64, a64 = critic.bootstrap_q(g.weights["target_actor"], g.weights["target_critic"], state, flags, dtype=np.float64)
        assert np.all(np.isfinite(q64)) and np.all(np.isfinite(a64))
        assert not N.bits(c["q"])[~ev].any() and not N.bits(c["a7"])[~ev].any(), "rows that are not (CTL and not Done) must hold zero bits"
        worst_a = max(worst_a, float(np.abs(c["a7"].astype(np.float64) - a64).max()))
        worst_q = max(worst_q, float(np.abs(c["q"].astype(np.float64) - q64).max()))
        # the pass with its default q == nstep.py on the read-back blocks, fed the device's q
        w_rec, w_idx, w_total = nstep.nstep_transitions(c["blocks"], GAMMA0, N.WINDOW, prev=c["prev"], q=c["q"])
        assert c["total"] == w_total > 0 and np.array_equal(c["idx"], w_idx) and N.same_bits(c["rec"], w_rec), "call %d" % i
        n_rec += w_total
    print("lane_num %d closed loop: %d evaluated rows, %d controlled rows behind Done, %d transitions; "
          "max |a - numpy f64| = %.3e (bar %.1e), max |q - numpy f64| = %.3e (bar %.3e)"
          % (lane_num, n_ev, n_done, n_rec, worst_a, ACTION_TOL, worst_q, boot_bar(g)))
    assert n_ev >= 200 and n_done >= 1
    assert worst_a <= ACTION_TOL and worst_q <= boot_bar(g)
    # installing the target networks and running the passes changes no bit of the roll-out or of the state
    calls0, fields0, _ = closed_loop(lane_num, False)
    for c, c0 in zip(calls, calls0):
        for k in TRAIN_OUTS:
            assert N.same_bits(c["blocks"][k], c0["blocks"][k]), k
    for f in fields:
        assert N.same_bits(fields[f], fields0[f]), f
    # the closing pass: memory -> sample == ReplayModel, learner step == the host build
    model = ReplayModel(buffer_size=301, batch_size=64, seed=77)
    model.add(calls[-1]["rec"], total=calls[-1]["total"])
    check_sample(sample, model.sample(2, check=False))
    rows, act7, target, seq = sample
    assert (_np(seq) >= 0).all() and rows.shape == (2, 64, 28)
    P = LS.host_block(LS.nets())
    losses, grads = LS.host_step(P, _np(rows), _np(act7), _np(target))
    got_l, got_g = learned
    assert np.array_equal(LS.bits32(_np(got_l)), LS.bits32(losses)) and np.array_equal(LS.bits32(_np(got_g)), LS.bits32(grads))
    check_block(lrn, P, "lane_num %d roll-out" % lane_num)
    assert lrn.steps() == 2 and np.all(np.isfinite(P))

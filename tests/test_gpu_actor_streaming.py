"""The two-launch actor (k_actor_h / k_actor_t, csrc/pve_actor.h) beyond one intersection per wave.  launch_actor_t
(csrc/pve_hip.hip) starts min(ceil(n_envs / 4), 1024) workgroups of 4 waves, one wave per intersection at a time, so
`for (; env < n_envs; env += stride)` runs a second time only above 4096 intersections.  At 4096 + 13 the waves of workgroups
0 .. 3 take a second intersection (the last of the four workgroups only one): the flags prefetched one intersection ahead, the
wave's reused slot list in LDS and the `env` handed to the exploration noise are exercised there.

Intersections are independent, so the expected actions are those of small batches over the same arrival streams, stepped
identically (bit for bit; tests/test_gpu_parity.py relies on the same independence); the NumPy restatements of the actor and of
the noise are the second, kernel-independent reference."""
import numpy as np
import pytest
import torch

from oracle.actor_np import actor_forward, flat_weights, load_weights
from pve_mcc_amd import noise
from pve_mcc_amd.arrivals import synthetic_arrivals
from tests.actor_scenarios import ACTION_TOL
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
N_ENVS, TICKS = 4096 + 13, 120
RANGES = ((0, 16), (N_ENVS - 16, N_ENVS))
M_CONTROL, M_ALIVE = 0x1, 0x80                    # csrc/pve_types.h
# planted occupancies (global env -> "all" slots controlled / "none"): the wave of env e < 13 also takes env 4096 + e, so each
# pair below hands a wave a long slot list followed by a short one, or the reverse, or an intersection without any
PLANTED = {2: "all", 4096 + 5: "all", 7: "none", 4096 + 4: "none"}


def bits(x):
    return np.ascontiguousarray(_np(x) if torch.is_tensor(x) else x, np.float64).view(np.uint64)


def stepped(arr, lo, hi, cap, table, **kw):
    """the batch of environments lo .. hi - 1 after TICKS ticks under the action table, with the planted occupancies"""
    b = make_batch(arr[lo:hi], hi - lo, cap, "hip", outputs=("obs_post", "reward", "flags", "env_out"), **kw)
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    b.set_action_table(table)
    b.step_many(TICKS, source="table")
    meta = b.state_field("meta")
    for env, what in PLANTED.items():
        if lo <= env < hi:
            if what == "all":
                meta[env - lo] |= M_ALIVE | M_CONTROL
            else:
                meta[env - lo] &= ~M_CONTROL
    return b


@pytest.mark.parametrize("actor_f32", [False, True])
@pytest.mark.parametrize("cap,dtype,rate", [(64, torch.float64, 700.0), (256, torch.float32, 1000.0)])
def test_gpu_actor_second_intersection_per_wave(cap, dtype, rate, actor_f32):
    assert (N_ENVS + 3) // 4 > 1024 and N_ENVS - 4096 < 16          # the geometry: a second iteration in 13 waves
    arr = synthetic_arrivals(N_ENVS, rate=rate, horizon_s=TICKS * 0.1 + 30, seed=515)
    tick, vid = np.arange(TICKS)[:, None], np.arange(512)[None, :]
    table = torch.as_tensor(np.sin(0.37 * vid + 0.05 * tick).astype(np.float32).astype(np.float64))
    kw = dict(obs_dtype=dtype, actor_f32=actor_f32)
    big = stepped(arr, 0, N_ENVS, cap, table, **kw)
    small = [stepped(arr, lo, hi, cap, table, **kw) for lo, hi in RANGES]
    assert big.metrics()["overflow"] == 0
    for (lo, hi), s in zip(RANGES, small):                            # the same state on both sides
        for f in ("id", "meta", "p", "v"):
            assert torch.equal(big.state_field(f)[lo:hi], s.state_field(f)), f
        assert torch.equal(big.obs[lo:hi], s.obs)
    meta = _np(big.state_field("meta"))
    ctl = (meta & (M_ALIVE | M_CONTROL)) == (M_ALIVE | M_CONTROL)
    per_env = ctl.sum(axis=1)
    in_ranges = np.concatenate([per_env[lo:hi] for lo, hi in RANGES])
    print("cap %d, %s rows, actor_f32 %s: %d controlled vehicles in %d intersections (%d without any), %d / %d in the compared ranges"
          % (cap, dtype, actor_f32, ctl.sum(), N_ENVS, (per_env == 0).sum(), in_ranges.sum(), (in_ranges == 0).sum()))
    assert in_ranges.sum() >= 200 and (in_ranges == 0).sum() >= 1 and (in_ranges == cap).sum() >= 1
    assert (per_env > 0).mean() >= 0.95 and per_env[4096:].sum() >= 100
    w = load_weights()
    a_np = actor_forward(w, _np(big.obs[4096:])).astype(np.float64)
    sigma, seed = 0.2, 0xFEED5EED
    for noisy in (False, True):
        for b, off in [(big, 0)] + [(s, lo) for s, (lo, _) in zip(small, RANGES)]:
            b.set_exploration(sigma if noisy else 0.0, seed=seed, env_offset=off)
        a = _np(big.act()).copy()
        big.synchronize()
        for (lo, hi), s in zip(RANGES, small):
            assert np.array_equal(bits(a[lo:hi]), bits(s.act())), "envs %d .. %d, noise %s: act() differs from the small batch" % (lo, hi - 1, noisy)
        assert np.all(bits(a[~ctl]) == 0), "uncontrolled slots must be exactly 0.0"
        if not noisy:
            a_clean = a
            worst = float(np.abs(a[4096:] - a_np)[ctl[4096:]].max())
            print("envs 4096 .. %d: max |a - numpy actor| = %.3e on %d controlled slots (bar %.1e)" % (N_ENVS - 1, worst, ctl[4096:].sum(), ACTION_TOL))
            assert worst <= ACTION_TOL
        else:
            # the noise of the second iteration is drawn for the global env index: float64(actor) + sigma * z, restated
            ids = _np(big.state_field("id")).astype(np.int64)
            env = np.arange(N_ENVS)[:, None]
            z = noise.action_noise(seed, env, np.where(ctl, ids, 0), big.ticks)
            want = np.where(ctl, a_clean + sigma * z, 0.0)
            assert np.array_equal(bits(a), bits(want)), "act() with noise != act() + sigma * action_noise(seed, env, id, tick)"
            assert np.any(a[ctl] != a_clean[ctl])

"""The statistics kernels (csrc/pve_stats.h: k_stats_rows, k_stats_groups, k_stats_totals, k_stats_metrics) against the NumPy
model (pve_mcc_amd.stats) bit for bit: the raw entry point on the synthetic blocks of tests/test_rollout_stats.py, whatever the
workgroup size; rollout_stats over real roll-outs of every kernel family into dirty rings, its column sums against metrics();
metrics_by_group; totals accumulated over calls with no synchronisation in between; the pipelined batch."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights, load_weights
from pve_mcc_amd import _capi, stats as ST
from pve_mcc_amd.arrivals import synthetic_arrivals, synthetic_intentions
from pve_mcc_amd.batched import BatchedIntersections, PipelinedIntersections
from tests import metrics_ref
from tests.test_rollout_stats import SHAPES, group_map, synthetic_blocks

pytestmark = pytest.mark.gpu
COL = ST.COL
GUARD = 256
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
E, T, PREFILL = 5, 21, 250                                  # (250 ticks: to steady state, vehicles leave the box)
GROUPS5 = np.array([0, 2, 0, 2, 7], np.int32)             # group 1 empty, the last environment out of range


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def filled(nbytes):
    return torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")


def on_device(a):
    return torch.as_tensor(np.ascontiguousarray(a).view(np.uint8).ravel()).cuda()


_handles = {}


def handle(n_envs, cap, f32):
    key = (n_envs, cap, f32)
    if key not in _handles:
        _handles[key] = BatchedIntersections(n_envs, cap, None, device="cuda", outputs=("obs_post",),
                                             obs_dtype=torch.float32 if f32 else torch.float64)
    return _handles[key]


def raw_stats(b, blk, T_, G, groups, with_obs, block_threads, totals0):
    """pve_rollout_stats on device copies of the blocks into 0xFF-filled buffers -> (series, totals, scratch); guards and the
    inputs are checked"""
    n_envs = b.n_envs
    names = ["flags", "reward", "env_out"] + (["obs_pre"] if with_obs else [])
    dev = {k: on_device(blk[k]) for k in names}
    before = {k: v.clone() for k, v in dev.items()}
    g = on_device(groups) if groups is not None else None
    series, scratch, tot = filled(8 * T_ * G * 14), filled(8 * T_ * n_envs * 14), filled(8 * G * 14)
    tot[:8 * G * 14] = on_device(totals0)
    st = _capi.PveStats(n_ticks=T_, n_groups=G, block_threads=block_threads, reserved=0, group=g.data_ptr() if g is not None else None,
                        flags=dev["flags"].data_ptr(), reward=dev["reward"].data_ptr(),
                        obs_pre=dev["obs_pre"].data_ptr() if with_obs else None, env_out=dev["env_out"].data_ptr(),
                        series=series.data_ptr(), totals=tot.data_ptr(), scratch=scratch.data_ptr())
    assert b.lib.pve_stats_scratch_bytes(n_envs, T_) == 8 * T_ * n_envs * 14
    b._bind_stream()
    rc = b.lib.pve_rollout_stats(b._h, C.byref(st))
    assert rc == 0, b.lib.pve_last_error()
    b.synchronize()
    for buf, used in ((series, 8 * T_ * G * 14), (scratch, 8 * T_ * n_envs * 14), (tot, 8 * G * 14)):
        assert bool((buf[used:] == 0xFF).all()), "guard region written"
    for k in names:
        assert torch.equal(dev[k], before[k]), "input block %s modified" % k

    def f64(buf, shape):
        return buf[:8 * int(np.prod(shape))].cpu().numpy().view(np.float64).reshape(shape)
    return f64(series, (T_, G, 14)), f64(tot, (G, 14)), f64(scratch, (T_, n_envs, 14))


# ------------------------------------------------------------------ 1. the raw entry point on synthetic blocks
# (the CPU test's 36 shapes, and 4101 environments: 65 chunks, one more than the chunks that wait in LDS at a time)
@pytest.mark.parametrize("part", [0, 1, 2, "two_batches"])
def test_kernels_equal_the_numpy_model_bit_for_bit(part):
    shapes = [(64, 4101, 2, True, True, 3)] if part == "two_batches" else SHAPES[part::3]
    for k, (cap, n_envs, T_, f32, with_obs, G) in enumerate(shapes):
        blk = synthetic_blocks(T_, n_envs, cap, f32, seed=500 + 7 * k + (0 if isinstance(part, str) else part))
        groups = group_map(n_envs, G)
        model_in = dict(blk) if with_obs else {n: v for n, v in blk.items() if n != "obs_pre"}
        rows = ST.env_rows(model_in)
        want = ST.group_rows(rows, groups, G)
        tot0 = np.arange(G * 14, dtype=np.float64).reshape(G, 14) * 0.37
        want_tot = ST.add_totals(tot0, want)
        b = handle(n_envs, cap, f32)
        for block in (0, 64, 1024):
            got, got_tot, got_rows = raw_stats(b, blk, T_, G, groups, with_obs, block, tot0)
            what = (cap, n_envs, T_, f32, with_obs, G, block)
            assert np.array_equal(bits(got_rows), bits(rows)), what
            assert np.array_equal(bits(got), bits(want)), what
            assert np.array_equal(bits(got_tot), bits(want_tot)), what
            assert np.all(np.isfinite(got)), what


# ------------------------------------------------------------------ 2. real roll-outs of every kernel family
ROLLOUTS = {"l12_c64": dict(lane_num=12, cap=64, rate=700.0), "l12_c128": dict(lane_num=12, cap=128, rate=1400.0),
            "l12_c128_queue": dict(lane_num=12, cap=128, rate=1400.0, persistent=True, chunk=7),
            "l12_c256": dict(lane_num=12, cap=256, rate=2600.0), "l4_c128": dict(lane_num=4, cap=128, rate=1500.0),
            "l8_c128": dict(lane_num=8, cap=128, rate=1300.0)}


def dirty(traj):
    for t in traj.values():
        t.view(torch.uint8).fill_(0xFF)
    return traj


def training_batch(lane_num, cap, rate, seed):
    arr = synthetic_arrivals(E, rate=rate, horizon_s=(PREFILL + 4 * T) * 0.1 + 30, seed=seed, lane_num=lane_num)
    ch = synthetic_intentions(E, arr.shape[1], seed=seed, lane_num=lane_num) if lane_num == 8 else None
    b = BatchedIntersections(E, cap, arr, device="cuda", outputs=TRAIN_OUTS, obs_dtype=torch.float32, lane_num=lane_num, intentions=ch)
    b.reset()
    return b


def check_rollout(b, traj, m0, what):
    """rollout_stats on the blocks the last call filled against the model on their copies, and against the metrics() deltas"""
    g = torch.as_tensor(GROUPS5).cuda()
    series = b.rollout_stats(groups=g, n_groups=3)
    rows_dev = b._stats_rows                                   # (the kernels' scratch of that call)
    one = b.rollout_stats(traj)
    m1 = b.metrics()                                           # (synchronises)
    blk = {k: traj[k][:T].cpu().numpy() for k in ("flags", "reward", "env_out", "obs_pre")}
    rows = ST.env_rows(blk)
    assert np.array_equal(bits(rows_dev.cpu().numpy()), bits(rows)), what
    assert np.array_equal(bits(series.cpu().numpy()), bits(ST.group_rows(rows, GROUPS5, 3))), what
    assert np.array_equal(bits(one.cpu().numpy()), bits(ST.group_rows(rows))), what
    assert np.all(np.isfinite(rows)) and np.all(series.cpu().numpy()[:, 1] == 0)
    tot = ST.add_totals(np.zeros((1, 14)), one.cpu().numpy())[0]
    for col, key in (("alive", "alive_steps"), ("ctl", "ctl_steps"), ("spawned", "spawned"), ("finished", "passed"),
                     ("collided", "collided"), ("lock", "locks"), ("env_ticks", "ticks")):
        assert tot[COL[col]] == m1[key] - m0[key], (what, col, tot[COL[col]], m1[key] - m0[key])
    ctl = (blk["flags"] & 2) != 0
    bar = metrics_ref.REL_BAR * float(np.maximum(1.0, np.abs(blk["reward"][ctl])).sum())
    dev = abs(tot[COL["sum_reward"]] - (m1["sum_reward"] - m0["sum_reward"]))
    print("rollout stats %s: ctl %d, collided %d, finished %d, sum_reward %.6f vs metrics() delta: deviation %.3e, bar %.3e"
          % (what, tot[COL["ctl"]], tot[COL["collided"]], tot[COL["finished"]], tot[COL["sum_reward"]], dev, bar))
    assert dev <= bar, what
    assert tot[COL["ctl"]] > 0, what
    return tot


@pytest.mark.parametrize("source", ["actor", "pool"])
@pytest.mark.parametrize("name", sorted(ROLLOUTS))
def test_real_rollouts_into_dirty_rings(name, source):
    cfg = dict(ROLLOUTS[name])
    launch = dict(persistent=cfg.pop("persistent", False), chunk=cfg.pop("chunk", 0))
    b = training_batch(seed=300 + len(name), **cfg)
    if source == "actor":
        b.set_actor(flat_weights(load_weights()))
        b.set_exploration(0.3, seed=5)
    else:
        pool = np.random.default_rng(4).uniform(-3, 3, size=(16, E, cfg["cap"])).astype(np.float32).astype(np.float64)
        b.set_action_pool(torch.as_tensor(pool))
    pre = b.alloc_trajectory(50)
    for _ in range(PREFILL // 50):
        b.step_many(50, source=source, trajectory=pre)
    ring = dirty(b.alloc_trajectory(T + 2))                    # (longer than the call: the blocks behind it keep the fill)
    m0 = b.metrics()
    traj = b.step_many(T, source=source, trajectory=ring, **launch)
    if launch["persistent"]:
        assert b.last_launch() == "persistent"
    tot = check_rollout(b, {k: v[:T] for k, v in traj.items()}, m0, "%s %s" % (name, source))
    assert tot[COL["finished"]] > 0 and tot[COL["spawned"]] > 0 and tot[COL["deleted"]] > 0, (name, source, tot)   # (reach)
    # the single-tick views (T = 1): the last tick of the call
    last = b.rollout_stats(b.out).cpu().numpy()
    assert last.shape == (1, 1, 14)
    assert np.array_equal(bits(last), bits(ST.rollout_stats({k: traj[k][T - 1].cpu().numpy() for k in ("flags", "reward", "env_out", "obs_pre")})))


# ------------------------------------------------------------------ 3. metrics_by_group
def test_metrics_by_group_partitions_metrics():
    arr = synthetic_arrivals(E, rate=1400.0, horizon_s=70.0, seed=41)
    b = BatchedIntersections(E, 128, arr, device="cuda", outputs=("obs_post", "reward", "flags", "env_out"))
    b.reset()
    b.set_action_pool(torch.zeros(1, E, 128, dtype=torch.float64))
    b.step_many(400, source="pool")
    one = b.metrics_by_group()
    three = b.metrics_by_group(torch.as_tensor(GROUPS5).cuda(), 3)
    rest = b.metrics_by_group(np.array([1, 1, 1, 1, 0], np.int32), 1)            # the environment GROUPS5 leaves out
    m = b.metrics()
    want = np.array([m[k] for k in _capi.METRIC_NAMES])
    one, three, rest = one.cpu().numpy(), three.cpu().numpy(), rest.cpu().numpy()
    assert one.shape == (1, 12) and three.shape == (3, 12)
    assert np.array_equal(bits(one[0]), bits(want)), (one, want)
    hd = ST.headers_of(b)
    assert np.array_equal(bits(three), bits(ST.metrics_groups(hd, 128, GROUPS5, 3)))
    print("metrics_by_group: %s" % {k: m[k] for k in ("ctl_steps", "passed", "collided", "sum_reward", "sum_jerk")})
    assert np.all(three[1] == 0) and m["ctl_steps"] > 0 and m["sum_reward"] != 0
    ints = [k for k, n in enumerate(_capi.METRIC_NAMES) if n not in ("sum_reward", "sum_jerk")]
    assert np.array_equal(three.sum(0)[ints] + rest[0][ints], want[ints])
    for k in (7, 8):
        assert abs(three[:, k].sum() + rest[0, k] - want[k]) <= 1e-12 * max(1.0, abs(want[k]))


# ------------------------------------------------------------------ 4. totals over calls, no synchronisation in between
def test_totals_accumulate_without_a_synchronisation():
    b = training_batch(12, 128, 1400.0, seed=42)
    pool = np.random.default_rng(9).uniform(-3, 3, size=(16, E, 128)).astype(np.float32).astype(np.float64)
    b.set_action_pool(torch.as_tensor(pool))
    b.step_many(PREFILL, source="pool", trajectory=True)
    ring = [dirty(b.alloc_trajectory(T)), dirty(b.alloc_trajectory(T))]
    g = torch.as_tensor(GROUPS5).cuda()
    totals = torch.zeros(3, 14, dtype=torch.float64, device="cuda")
    kept = []
    for i in range(3):
        traj = b.step_many(T, source="pool", trajectory=ring[i & 1])
        b.rollout_stats(groups=g, n_groups=3, totals=totals)
        kept.append({k: traj[k].clone() for k in ("flags", "reward", "env_out", "obs_pre")})    # (device copies: no wait)
    got = totals.cpu().numpy()                                                                  # the one read
    want = np.zeros((3, 14))
    for blk in kept:
        want = ST.add_totals(want, ST.rollout_stats({k: v.cpu().numpy() for k, v in blk.items()}, GROUPS5, 3))
    assert np.array_equal(bits(got), bits(want))
    assert want[0, COL["ctl"]] > 0 and want[2, COL["env_ticks"]] == 2 * 3 * T
    s = ST.summaries(totals)
    assert np.isnan(s["reward_mean"][1]) and np.isfinite(s["reward_std"][0]) and 0.0 <= s["collision_rate"][0]


# ------------------------------------------------------------------ 5. the pipelined batch
def test_pipelined_rollout_stats_is_the_sum_of_its_sub_batches():
    arr = synthetic_arrivals(E, rate=1400.0, horizon_s=(PREFILL + T) * 0.1 + 30, seed=43)
    pipe = PipelinedIntersections(E, 128, arr, n_sub=2, device="cuda", outputs=TRAIN_OUTS, obs_dtype=torch.float32)
    pipe.reset()
    pool = np.random.default_rng(10).uniform(-3, 3, size=(16, E, 128)).astype(np.float32).astype(np.float64)
    pipe.set_action_pool(pool)
    pipe.step_many(PREFILL, source="pool", trajectory=True)
    trajs = pipe.step_many(T, source="pool", trajectory=True)
    totals = torch.full((3, 14), 0.5, dtype=torch.float64, device="cuda")
    g_dev = torch.zeros(E, dtype=torch.int32, device="cuda").add_(torch.as_tensor(GROUPS5).cuda())    # made on the current stream, just now
    out = torch.full((T, 3, 14), -1.0, dtype=torch.float64, device="cuda")
    series = pipe.rollout_stats(groups=g_dev, n_groups=3, out=out, totals=totals)
    assert series is out
    mg = pipe.metrics_by_group(g_dev, 3, out=torch.empty(3, 12, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    want = None
    for k, tr in enumerate(trajs):
        lo, hi = pipe.bounds[k], pipe.bounds[k + 1]
        s = ST.rollout_stats({n: tr[n].cpu().numpy() for n in ("flags", "reward", "env_out", "obs_pre")}, GROUPS5[lo:hi], 3)
        want = s if want is None else want + s
    assert np.array_equal(bits(series.cpu().numpy()), bits(want))
    assert np.array_equal(bits(totals.cpu().numpy()), bits(ST.add_totals(np.full((3, 14), 0.5), want)))
    assert want[:, 0, COL["ctl"]].sum() > 0
    m = pipe.metrics()
    ints = [k for k, n in enumerate(_capi.METRIC_NAMES) if n not in ("sum_reward", "sum_jerk")]
    rest = pipe.metrics_by_group(np.array([1, 1, 1, 1, 0], np.int32), 1).cpu().numpy()
    assert np.array_equal(mg.cpu().numpy().sum(0)[ints] + rest[0][ints], np.array([m[k] for k in _capi.METRIC_NAMES])[ints])


# ------------------------------------------------------------------ 6. evaluate_rates: batch_test()'s densities in one batch
def test_evaluate_rates_reports_one_line_per_density():
    from pve_mcc_amd import evaluate as EV
    ticks, n = 130, 2
    res = EV.evaluate_rates([1200.0, 300.0], flat_weights(load_weights()), ticks=ticks, envs_per_rate=n, capacity=128, seed=5, chunk=50)
    assert [r["rate"] for r in res] == [1200.0, 300.0] and all(r["n_envs"] == n and r["ticks"] == ticks for r in res)
    for r in res:
        print(EV.rate_line(r))
        assert r["vehicles"] > 0 and np.isfinite(r["reward_mean"]) and r["reward_std"] >= 0 and r["v_mean"] > 0
        assert EV.rate_line(r).startswith("vehicle number %d  collisions occurred number %d collisions rate " % (r["vehicles"], r["collisions"]))
    assert res[0]["vehicles"] > res[1]["vehicles"]                # the denser streams spawn more
    # the same batch evaluated in one piece: the groups partition it
    both = BatchedIntersections(2 * n, 128, None, device="cuda", outputs=("obs_post", "reward", "flags", "env_out"))
    both.generate_arrivals(np.repeat([1200.0, 300.0], n), horizon_s=ticks * 0.1 + 30.0, seed=5)
    both.set_actor(flat_weights(load_weights()))
    both.reset()
    both.step_many(ticks, source="actor")
    m = both.metrics()
    assert m["spawned"] == sum(r["vehicles"] for r in res) and m["collided"] == sum(r["collisions"] for r in res)

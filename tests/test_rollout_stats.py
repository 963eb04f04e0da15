"""Roll-out and evaluation statistics by group on the CPU (csrc/pve_stats.h, pve_rollout_stats / pve_metrics_groups): a g++ build
of the header against the NumPy restatement (pve_mcc_amd.stats) bit for bit, the model fed from emulator roll-outs against
what the oracle's records say on their own, the column sums against metrics(), totals across calls, summaries(), the grouped
metrics, and the C ABI's argument checks through the emulator, which has no such kernels and says so.  The kernels are held
to the model in tests/test_gpu_rollout_stats.py."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from pve_mcc_amd import _capi, stats as ST
from pve_mcc_amd.batched import BatchedIntersections
from tests import metrics_ref, metrics_scenarios as MS, native
from tests.hip_adapter import emulator_lib, make_batch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCENARIOS = ("l12_c64", "l12_c128_five", "l12_c256", "l4_c128", "l8_c128")
STAT_OUTS = ("obs_post", "obs_pre", "reward", "flags", "new_slot", "env_out")
COL = ST.COL


def _declare(lib):
    vp = C.c_void_p
    lib.stats_rollout_host.restype = None
    lib.stats_rollout_host.argtypes = [C.c_int] * 5 + [vp] * 8
    lib.stats_metrics_groups_host.restype = None
    lib.stats_metrics_groups_host.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.stats_header_bytes.restype = C.c_int
    lib.stats_scratch_bytes_host.restype = C.c_size_t
    lib.stats_scratch_bytes_host.argtypes = [C.c_longlong, C.c_longlong]
    return lib


def host():
    return native.load("stats_host", "libstats_host.so", _declare)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ synthetic blocks (shared with tests/test_gpu_rollout_stats.py)
def synthetic_blocks(T, E, cap, f32, seed):
    """Blocks as a roll-out leaves them, and worse: every float of a slot without F_CTL holds the 0xFF pattern (a NaN), dead
    slots have flags 0, rewards hold the reference's event values (+-20, -10, 5) between values whose sum depends on the
    order (magnitudes from 1e-9 to 1e9)."""
    rng = np.random.default_rng(seed)
    n_alive = rng.integers(0, cap + 1, size=(T, E))
    if E > 1:
        n_alive[:, 0] = cap                                     # a full environment ...
        n_alive[:, -1] = 0                                      # ... and an empty one
    slot = np.arange(cap)[None, None, :]
    alive = slot < n_alive[..., None]
    ctl = alive & (rng.random((T, E, cap)) < 0.7)
    flags = np.where(alive, 1, 0).astype(np.int32)
    flags |= np.where(ctl, 2, 0).astype(np.int32)
    flags |= np.where(alive & (rng.random((T, E, cap)) < 0.2), 4, 0).astype(np.int32)                 # DONE, also on uncontrolled slots
    flags |= (np.where(alive & (rng.random((T, E, cap)) < 0.15), rng.integers(1, 4, size=(T, E, cap)), 0) << 8).astype(np.int32)
    flags |= np.where(alive, rng.integers(0, 4, size=(T, E, cap)) << 6, 0).astype(np.int32)
    events = np.array([20.0, -20.0, -10.0, 5.0])
    r = rng.standard_normal((T, E, cap)) * 10.0 ** rng.integers(-9, 10, size=(T, E, cap))
    pick = rng.random((T, E, cap)) < 0.3
    r = np.where(pick, events[rng.integers(0, 4, size=(T, E, cap))], r)
    reward = np.empty((T, E, cap))
    reward.view(np.uint8)[:] = 0xFF
    reward[ctl] = r[ctl]
    odt = np.float32 if f32 else np.float64
    obs = np.empty((T, E, cap, 28), odt)
    obs.view(np.uint8)[:] = 0xFF
    obs[ctl] = (rng.standard_normal((int(ctl.sum()), 28)) * 7.0).astype(odt)
    env_out = rng.integers(0, 300, size=(T, E, 8)).astype(np.int32)
    env_out[..., 0] = n_alive
    return dict(flags=flags, reward=reward, obs_pre=obs, env_out=env_out)


def group_map(E, G):
    """Non-contiguous assignment; with G = 3 group 1 stays empty and (E > 2) one environment carries an id out of range."""
    if G == 1:
        return None
    g = np.where(np.arange(E) % 3 == 1, 2, 0).astype(np.int32)
    if E > 2:
        g[E // 2] = 7 if E % 2 else -1
    return g


SHAPES = [(cap, E, T, f32, with_obs, G)
          for (cap, E, T), (f32, with_obs, G) in zip(itertools.product((64, 128, 256), (1, 5, 17), (1, 2, 7, 21)),
                                                     itertools.cycle([(True, True, 1), (False, True, 3), (True, False, 3),
                                                                      (False, False, 1), (True, True, 3)]))]


def host_rollout(blk, E, cap, T, f32, with_obs, G, groups, totals=None):
    """(series, totals, scratch) of the g++ build into 0xFF-filled buffers with guards behind them"""
    def buf(n):
        a = np.empty(n + 8)
        a.view(np.uint8)[:] = 0xFF
        return a
    series, scratch = buf(T * G * 14), buf(T * E * 14)
    tot = buf(G * 14)
    if totals is not None:
        tot[:G * 14] = np.asarray(totals).ravel()
    obs = np.ascontiguousarray(blk["obs_pre"]) if with_obs else None
    host().stats_rollout_host(E, cap, T, G, int(f32), groups.ctypes.data if groups is not None else None, blk["flags"].ctypes.data,
                              blk["reward"].ctypes.data, obs.ctypes.data if with_obs else None, blk["env_out"].ctypes.data,
                              series.ctypes.data, tot.ctypes.data if totals is not None else None, scratch.ctypes.data)
    for a in (series, scratch, tot):
        assert np.all(a.view(np.uint8)[-64:] == 0xFF), "guard"
    return series[:-8].reshape(T, G, 14), tot[:-8].reshape(G, 14), scratch[:-8].reshape(T, E, 14)


# ------------------------------------------------------------------ 1. the g++ build of the header against the NumPy model
def test_host_build_equals_the_numpy_model_bit_for_bit():
    assert host().stats_header_bytes() == ST.HEADER_DTYPE.itemsize == 408
    assert host().stats_scratch_bytes_host(4096, 20) == 4096 * 20 * 14 * 8
    order_seen = 0
    for k, (cap, E, T, f32, with_obs, G) in enumerate(SHAPES):
        blk = synthetic_blocks(T, E, cap, f32, seed=100 + k)
        groups = group_map(E, G)
        model_in = dict(blk) if with_obs else {n: v for n, v in blk.items() if n != "obs_pre"}
        rows = ST.env_rows(model_in)
        want = ST.group_rows(rows, groups, G)
        tot0 = np.arange(G * 14, dtype=np.float64).reshape(G, 14) * 0.37
        got, got_tot, got_rows = host_rollout(blk, E, cap, T, f32, with_obs, G, groups, totals=tot0)
        what = (cap, E, T, f32, with_obs, G)
        assert np.array_equal(bits(got_rows), bits(rows)), what
        assert np.array_equal(bits(got), bits(want)), what
        assert np.array_equal(bits(got_tot), bits(ST.add_totals(tot0, want))), what
        assert np.all(np.isfinite(got)), what                                  # no 0xFF pattern reached a sum
        if not with_obs:
            assert np.all(got[..., COL["sum_v"]] == 0) and np.all(got[..., COL["sum_a"]] == 0)
        # the definition's plain meaning, column by column
        ctl = (blk["flags"] & 2) != 0
        member = np.ones(E, bool) if groups is None else None
        for g in range(G):
            m = member if groups is None else groups == g
            assert np.array_equal(got[:, g, COL["env_ticks"]], np.full(T, m.sum()))
            assert np.array_equal(got[:, g, COL["ctl"]], ctl[:, m].sum((1, 2)))
            assert np.array_equal(got[:, g, COL["collided"]], (ctl & ((blk["flags"] >> 8) > 0))[:, m].sum((1, 2)))
            assert np.array_equal(got[:, g, COL["done"]], (ctl & ((blk["flags"] & 4) != 0))[:, m].sum((1, 2)))
            for col, src in (("alive", 0), ("spawned", 6), ("finished", 5), ("deleted", 4), ("collisions", 2), ("lock", 3)):
                assert np.array_equal(got[:, g, COL[col]], blk["env_out"][:, m, src].sum(1)), (what, col)
            r = np.where(ctl, blk["reward"], 0.0)[:, m]
            for t in range(T):
                exact = math.fsum(r[t].ravel())
                scale = float(np.abs(r[t]).sum()) + 1.0
                assert abs(got[t, g, COL["sum_reward"]] - exact) <= 1e-12 * scale, what
                # the same terms added in the reverse order: another float64 on some case, so an order change is visible here
                rev = 0.0
                for x in r[t].ravel()[::-1]:
                    rev += x
                order_seen += int(rev != got[t, g, COL["sum_reward"]])
        if G == 3:
            assert np.all(got[:, 1] == 0), "the empty group"
            if E > 2:                                                          # the environment with an id out of range is in no group
                assert got[:, :, COL["env_ticks"]].sum() == T * (E - 1)
    assert len(SHAPES) == 36 and order_seen > 0


# ------------------------------------------------------------------ 2. emulator roll-outs against the oracle's records
_runs = {}


def emulator_run(name):
    """One scenario through the CPU emulator with step_many(trajectory=True) from the pool, call by call; the oracle's tick
    records of the same run.  -> (per-call block dicts as NumPy, records[t][e], metrics() after every call, batch)"""
    if name in _runs:
        return _runs[name]
    ref = MS.reference(name)
    spec = ref.spec
    E, K, L = len(spec.envs), spec.capacity, spec.lane_num
    oracles = [MS.make_oracle(ref.arr[e], L, choice=None if ref.choice is None else ref.choice[e], **ref.cfg) for e in range(E)]
    recs = []
    for t in range(sum(spec.calls)):
        row = []
        for e, o in enumerate(oracles):
            n = o.n_alive
            row.append(o.tick(ref.actions[t, e, :n]))
        recs.append(row)
    if K == 256:                                     # (the 256-slot scenarios run on the wide emulator, tests/emu_wide)
        from tests.test_capacity256 import wide_lib
        lib = wide_lib()
    else:
        lib = emulator_lib()
    kw = dict(ref.cfg)
    if L != 12:
        kw.update(lane_num=L, intentions=ref.choice)
    b = BatchedIntersections(E, K, ref.arr, device="cpu", outputs=STAT_OUTS, _lib=lib, **kw)
    b.reset()
    b.set_action_pool(torch.as_tensor(ref.actions))
    calls, mets = [], [b.metrics()]
    for n in spec.calls:
        tr = b.step_many(n, source="pool", trajectory=True)
        calls.append({k: v.numpy().copy() for k, v in tr.items()})
        mets.append(b.metrics())
    _runs[name] = (calls, recs, mets, b)
    return _runs[name]


@pytest.mark.parametrize("name", SCENARIOS)
def test_emulator_rollout_against_the_oracle_records(name):
    calls, recs, _mets, _b = emulator_run(name)
    t0, worst = 0, 0.0
    for blk in calls:
        series = ST.rollout_stats(blk)
        rows = ST.env_rows(blk)
        T, E = rows.shape[:2]
        for t in range(T):
            for e in range(E):
                rec, x = recs[t0 + t][e], rows[t, e]
                assert x[COL["ctl"]] == len(rec["ids"]) and x[COL["collisions"]] == rec["collisions"] and x[COL["lock"]] == rec["lock"]
                assert x[COL["collided"]] == int((np.asarray(rec["coll_pv"]) > 0).sum()), (name, t0 + t, e)
                for col, terms in (("sum_reward", rec["reward"]), ("sum_v", np.asarray(rec["obs0"]).reshape(-1, 28)[:, 1]),
                                   ("sum_a", np.asarray(rec["obs0"]).reshape(-1, 28)[:, 2])):
                    terms = [float(v) for v in terms]
                    bar = metrics_ref.REL_BAR * sum(max(1.0, abs(v)) for v in terms)
                    dev = abs(x[COL[col]] - math.fsum(terms))
                    worst = max(worst, dev / bar if bar else 0.0)
                    assert dev <= bar, (name, col, t0 + t, e, dev, bar)
            assert np.array_equal(series[t, 0], ST.group_rows(rows[t:t + 1])[0, 0])
        t0 += T
    print("rollout stats %s: worst deviation of a per-(tick, env) float sum from the oracle's: %.2e of its bar" % (name, worst))


def test_scenarios_reach_what_the_columns_count():
    """From the oracle's side alone: a collided vehicle, a finished one, a lock and an environment that stays empty."""
    stats = [s for name in SCENARIOS for s in MS.reference(name).stats]
    assert sum(s["collided"] for s in stats) > 0 and sum(s["locks"] for s in stats) > 0
    assert any(s["peak"] == 0 for s in stats), "an environment that stays empty"
    fin = sum(int(MS.reference(name).snaps[sum(MS.SPECS[name].calls)][0]["passed"]) for name in SCENARIOS)
    assert fin > 0


# ------------------------------------------------------------------ 3. column sums over a run against metrics()
@pytest.mark.parametrize("name", SCENARIOS)
def test_column_sums_equal_the_metrics_deltas(name):
    calls, recs, mets, _b = emulator_run(name)
    ref = MS.reference(name)
    tot = np.zeros(14)
    for blk in calls:
        tot = ST.add_totals(tot[None], ST.rollout_stats(blk))[0]
    first, last = mets[0], mets[-1]
    for col, key in (("alive", "alive_steps"), ("ctl", "ctl_steps"), ("spawned", "spawned"), ("finished", "passed"),
                     ("collided", "collided"), ("lock", "locks")):
        assert tot[COL[col]] == last[key] - first[key], (name, col)
    assert tot[COL["env_ticks"]] == last["ticks"] - first["ticks"]
    bar = ref.snaps[sum(ref.spec.calls)][1]["sum_reward"]
    assert abs(tot[COL["sum_reward"]] - (last["sum_reward"] - first["sum_reward"])) <= bar, name


# ------------------------------------------------------------------ 4. totals across calls, summaries()
def test_totals_over_two_calls_and_summaries():
    a, b = synthetic_blocks(7, 17, 128, True, 5), synthetic_blocks(2, 17, 128, True, 6)
    groups = group_map(17, 3)
    s_a, s_b = ST.rollout_stats(a, groups, 3), ST.rollout_stats(b, groups, 3)
    z = np.zeros((3, 14))
    two = ST.add_totals(ST.add_totals(z, s_a), s_b)
    both = ST.add_totals(z, np.concatenate([s_a, s_b]))
    assert np.array_equal(bits(two), bits(both))
    _, h1, _ = host_rollout(a, 17, 128, 7, True, True, 3, groups, totals=z)
    _, h2, _ = host_rollout(b, 17, 128, 2, True, True, 3, groups, totals=h1)
    assert np.array_equal(bits(h2), bits(two))
    # a hand-made row: 4 controlled vehicles with rewards 1, 2, 3, 6 -> mean 3, population variance 3.5; v 2.5, a -0.5
    row = np.zeros(14)
    row[COL["ctl"]], row[COL["sum_reward"]], row[COL["sum_reward_sq"]] = 4, 12.0, 50.0
    row[COL["sum_v"]], row[COL["sum_a"]], row[COL["spawned"]], row[COL["collided"]] = 10.0, -2.0, 8, 2
    row[COL["collisions"]], row[COL["lock"]] = 3, 1
    s = ST.summaries(np.stack([row, np.zeros(14)]))
    assert s["reward_mean"][0] == 3.0 and s["reward_std"][0] == math.sqrt(3.5) == np.std([1.0, 2.0, 3.0, 6.0])
    assert s["v_mean"][0] == 2.5 and s["acc_mean"][0] == -0.5 and s["collision_rate"][0] == 0.25
    assert s["collisions"][0] == 3 and s["collided"][0] == 2 and s["lock"][0] == 1
    for k in ("reward_mean", "reward_std", "v_mean", "acc_mean", "collision_rate"):          # the empty group: nan, no exception
        assert np.isnan(s[k][1]), k
    assert s["collisions"][1] == 0 and ST.summaries(torch.as_tensor(two))["lock"].shape == (3,)
    assert ST.STAT_NAMES[10:] == ("sum_reward", "sum_reward_sq", "sum_v", "sum_a") and len(ST.STAT_NAMES) == _capi.PVE_STAT_N


# ------------------------------------------------------------------ 5. the grouped metrics
def test_metrics_groups_model_partitions_and_one_group_is_metrics():
    _calls, _recs, mets, b = emulator_run("l12_c128_five")
    hd = ST.headers_of(b)
    E, K = b.n_envs, b.capacity
    one = ST.metrics_groups(hd, K)
    assert one.shape == (1, 12)
    want = np.array([mets[-1][k] for k in _capi.METRIC_NAMES])
    assert np.array_equal(bits(one[0]), bits(want)), "one group is metrics(), float sums included"
    groups = np.array([2, 0, 2, 5, 0], np.int32)                                # group 1 empty, env 3 out of range
    three = ST.metrics_groups(hd, K, groups, 3)
    assert np.all(three[1] == 0)
    solo = ST.metrics_groups(hd, K, np.array([1, 1, 1, 0, 1], np.int32), 1)     # env 3 alone
    ints = [k for k, n in enumerate(_capi.METRIC_NAMES) if n not in ("sum_reward", "sum_jerk")]
    assert np.array_equal(three.sum(0)[ints] + solo[0][ints], one[0][ints])
    for k in (7, 8):
        assert abs(three[:, k].sum() + solo[0, k] - one[0, k]) <= 1e-12 * max(1.0, abs(one[0, k]))
    # the g++ build of the header's loop on the same headers
    raw = np.frombuffer(hd.tobytes(), np.uint8).copy()
    for g_map, G in ((None, 1), (groups, 3)):
        out = np.empty(G * 12 + 8)
        out.view(np.uint8)[:] = 0xFF
        host().stats_metrics_groups_host(raw.ctypes.data, E, K, g_map.ctypes.data if g_map is not None else None, G, out.ctypes.data)
        assert np.all(out.view(np.uint8)[-64:] == 0xFF)
        assert np.array_equal(bits(out[:-8].reshape(G, 12)), bits(ST.metrics_groups(hd, K, g_map, G)))


# ------------------------------------------------------------------ 6. the C ABI on a backend without the kernels
def test_entry_points_on_the_emulator():
    lib = emulator_lib()
    assert _capi.EXPORTS_STATS == ("pve_stats_scratch_bytes", "pve_rollout_stats", "pve_metrics_groups")
    # (that the header declares exactly EXPORTS_STATS, the version, PVE_STAT_* and pve_stats' layout: tests/test_binding_contract.py)
    assert _capi.EXPORTS_EXT == ("pve_generate_arrivals",)
    assert lib.pve_abi_version() == _capi.ABI_VERSION
    ext = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pve_env_stats.h")).read(), flags=re.S)
    assert "int pve_rollout_stats(pve_handle h, const pve_stats *st);" in ext
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pve_env.h")).read(), flags=re.S)
    assert not any(n in main for n in _capi.EXPORTS_STATS)
    product = _capi.load_library()
    assert all(hasattr(product, n) and hasattr(lib, n) for n in _capi.EXPORTS_STATS)
    assert not set(_capi.EXPORTS_STATS) & set(_capi.EXPORTS + _capi.EXPORTS_EXT)
    assert lib.pve_stats_scratch_bytes(4096, 20) == 4096 * 20 * 14 * 8 and lib.pve_stats_scratch_bytes(0, 5) == 0
    assert product.pve_stats_scratch_bytes(17, 3) == 17 * 3 * 14 * 8 and lib.pve_stats_scratch_bytes(5, -1) == 0
    b = make_batch(np.full((4, 12), np.inf), 3, 64, "emu", outputs=("obs_post", "obs_pre", "reward", "flags", "env_out"))
    b32 = make_batch(np.full((4, 12), np.inf), 3, 64, "emu", outputs=("obs_post", "obs_pre", "reward", "flags", "env_out"),
                     obs_dtype=torch.float32)
    keep = []

    def P(n, dt, off=0):
        raw = np.zeros(n * np.dtype(dt).itemsize + 32, np.uint8)
        keep.append(raw)
        return raw.ctypes.data + (-raw.ctypes.data) % 16 + off

    T = 2
    ptr = dict(group=P(3, np.int32), flags=P(T * 3 * 64, np.int32), reward=P(T * 3 * 64, np.float64), obs_pre=P(T * 3 * 64 * 28, np.float64),
               env_out=P(T * 3 * 8, np.int32), series=P(T * 3 * 14, np.float64), totals=P(3 * 14, np.float64), scratch=P(T * 3 * 14, np.float64))

    def run(h=b._h, desc=True, **kw):
        d = dict(n_ticks=T, n_groups=3, block_threads=0, reserved=0, **ptr)
        d.update(kw)
        return lib.pve_rollout_stats(h, C.byref(_capi.PveStats(**d)) if desc else None)

    bad = [(dict(h=None), b"null"), (dict(desc=False), b"null"), (dict(flags=None), b"null"), (dict(reward=None), b"null"),
           (dict(env_out=None), b"null"), (dict(series=None), b"null"), (dict(scratch=None), b"null"),
           (dict(n_ticks=0), b"n_ticks"), (dict(n_ticks=-3), b"n_ticks"), (dict(n_groups=0), b"n_groups"),
           (dict(n_groups=1025), b"n_groups"), (dict(group=None), b"n_groups"), (dict(block_threads=100), b"block_threads"),
           (dict(block_threads=2048), b"block_threads"), (dict(block_threads=-64), b"block_threads"), (dict(reserved=1), b"reserved"),
           (dict(group=ptr["group"] + 2), b"aligned"), (dict(flags=ptr["flags"] + 2), b"aligned"), (dict(reward=ptr["reward"] + 4), b"aligned"),
           (dict(obs_pre=ptr["obs_pre"] + 4), b"aligned"), (dict(env_out=ptr["env_out"] + 1), b"aligned"),
           (dict(series=ptr["series"] + 4), b"aligned"), (dict(totals=ptr["totals"] + 4), b"aligned"),
           (dict(scratch=ptr["scratch"] + 4), b"aligned"), (dict(h=b32._h, obs_pre=ptr["obs_pre"] + 2), b"aligned")]
    for kw, word in bad:
        assert run(**kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    for kw in (dict(), dict(obs_pre=None), dict(totals=None), dict(group=None, n_groups=1), dict(n_groups=1024), dict(block_threads=1024),
               dict(block_threads=64), dict(h=b32._h, obs_pre=ptr["obs_pre"] + 4)):
        assert run(**kw) == -1 and b"this backend has no statistics kernels" in lib.pve_last_error(), (kw, lib.pve_last_error())
    out = P(3 * 12, np.float64)
    for args, word in (((None, ptr["group"], 3, out), b"null"), ((b._h, ptr["group"], 3, None), b"null"), ((b._h, ptr["group"], 0, out), b"n_groups"),
                       ((b._h, ptr["group"], 1025, out), b"n_groups"), ((b._h, None, 2, out), b"n_groups"),
                       ((b._h, ptr["group"] + 2, 3, out), b"aligned"), ((b._h, ptr["group"], 3, out + 4), b"aligned")):
        assert lib.pve_metrics_groups(*args) == -1 and word in lib.pve_last_error(), (args, lib.pve_last_error())
    for args in ((b._h, ptr["group"], 3, out), (b._h, None, 1, out)):
        assert lib.pve_metrics_groups(*args) == -1 and b"this backend has no statistics kernels" in lib.pve_last_error()
    # the Python methods ask the backend and pass its refusal on
    b.reset()
    b.step_many(2, source="zero", trajectory=True)
    with pytest.raises(_capi.PveError, match="no statistics kernels"):
        b.rollout_stats()
    with pytest.raises(_capi.PveError, match="no statistics kernels"):
        b.rollout_stats(b.out, groups=[0, 1, 0])
    with pytest.raises(_capi.PveError, match="no statistics kernels"):
        b.metrics_by_group([0, 1, 1], 2)
    with pytest.raises(_capi.PveError, match="n_groups"):
        b.rollout_stats(n_groups=2)
    with pytest.raises(_capi.PveError, match="lack the reward"):
        make_batch(np.full((4, 12), np.inf), 3, 64, "emu", outputs=("obs_post", "flags", "env_out")).rollout_stats()
    from pve_mcc_amd.batched import PipelinedIntersections
    pipe = PipelinedIntersections(4, 64, np.full((4, 12), np.inf), n_sub=2, device="cpu", _lib=lib,
                                  outputs=("obs_post", "reward", "flags", "env_out"))
    with pytest.raises(_capi.PveError, match="no statistics kernels"):
        pipe.rollout_stats(groups=[0, 1, 1, 0])
    with pytest.raises(_capi.PveError, match="no statistics kernels"):
        pipe.metrics_by_group()

"""Parity under NON-DEFAULT constructor arguments -- every field of `pve_config` the C ABI exposes (include/pve_env.h), i.e.
`TrafficInteraction(arrive_time, dis_ctl, args, deltaT, vm, vM, am, aM, v0, ..., lane_cw)` + `args.collision_thr`
(ref traffic_interaction_scene.py:21-23, :32; callers only ever pass vm = 6: main.py:230).  The host derives the geometry
(lane_info, exit_p, the virtual-distance table) from lane_cw / dis_ctl and the exact constant divisions of the brake test from
|am|, so each argument is moved on its own and all of them together, under a pseudo-random +-3 tape that provokes collisions
and dead-locks:
  * live reference <-> C oracle, every tick, every field, 1e-12            (-m reference: build container only)
  * C oracle <-> the kernels' phase bodies on the CPU emulator, 1e-9      (CPU)
  * C oracle <-> the HIP kernels through the C ABI, 1e-9                  (-m gpu); + pve_step_many == single ticks
  * the committed fixture tests/golden/s1000_rand_kw.npz (all arguments together, generated from the live reference by
    tests/golden/gen_golden.py) is replayed by the CASE_NAMES-parametrised golden tests of the oracle / emulator / GPU suites.

The 4- and 8-lane layouts (second half of this file; the shipped checkpoint was trained with lane_num = 4 and vm = 6:
model_data/baseline/args.txt) derive much more from the arguments, in code the 12-lane kernels do not run: the general-geometry
constants of make_geo_const (csrc/pve_host.h: H, inbox, spawn_p, exit_p, the whole virtual-distance table of both layouts, the
4-lane far-conflict constants fix_d / fix_hi / fix_lo of TickGeo::walk_merge4), get_xy's division by rl * lane_cw, the float32
collision pre-filter, the lock test.  The same ladder for lane_num 4 and 8:
  * live reference <-> OracleGeoEnv, every tick, every field, intent and intention_re included, 1e-12      (-m reference)
  * OracleGeoEnv's geometry at lane_cw = 3, dis_ctl = 120 <-> tests/golden/geometry_geo_kw.npz             (test_oracle_geo.py)
  * OracleGeoEnv <-> the emulated phases / k_tick_geo (split protocol, both capacities), 1e-9              (CPU / -m gpu)
  * fused ticks on a batch, k_rollout_geo in every form (pool / table source, resident / work queue, the closed loop with the
    actor inside, the training outputs) with every argument moved, and the closed loop with vm = 6        (CPU twins / -m gpu)
  * the fixtures geo_g4_rand_kw / geo_g8_rand_kw / geo_g4_rand_vm6 (tests/golden/gen_golden_geo.py) are replayed by the
    GEO_CASE_NAMES-parametrised golden tests of the oracle / emulator / GPU suites; geo_g4_rand_vm6 by the drop-in class too."""
import os

import numpy as np
import pytest
import torch

from oracle.oracle import OracleEnv
from oracle.record import compare_records, get_policy
from tests import scenarios
from tests.parity_util import GOLDEN_DIR

ALL_KW = {"dis_ctl": 120, "lane_cw": 3, "collision_thr": 3, "vM": 15, "v0": 9, "am": -2.5, "aM": 2.5, "deltaT": 0.2, "vm": 6}
VARIANTS = [
    ("dis_ctl", {"dis_ctl": 120}),
    ("lane_cw", {"lane_cw": 3}),
    ("collision_thr", {"collision_thr": 3}),
    ("speeds", {"vM": 15, "v0": 9}),
    ("accel", {"am": -2.5, "aM": 2.5}),
    ("deltaT", {"deltaT": 0.2}),
    ("all", ALL_KW),
    ("vm6", {"vm": 6}),                                   # what every caller passes (main.py:230): the trained configuration
    ("accel_asym", {"am": -3.7, "aM": 1.3}),              # |am| != aM: the brake test's constant divisions (|am|, aM - am)
]
TICKS = 300


def stream(name="1000"):
    """the reference's own 1000 / 200 veh/h streams (data files committed under tests/golden/streams, read by the product's reader)"""
    from pve_mcc_amd.arrivals import load_arrival_mat
    return np.ascontiguousarray(load_arrival_mat(os.path.join(GOLDEN_DIR, "streams", "arvTimeNewVeh_new_%s_12.mat" % name)), np.float64)


class KwCase:
    """what scenarios.check_split_vs_oracle needs of a golden case, without a fixture"""

    def __init__(self, name, kw, ticks=TICKS, stream_name="1000"):
        self.name = "kw_" + name
        self.arrive = stream(stream_name)
        self.ctor = dict(kw)
        self.policy = get_policy("rand3")
        self.ticks = ticks


@pytest.mark.reference
@pytest.mark.parametrize("name,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_oracle_vs_live_reference_under_ctor_kwargs(name, kw):
    from tests.golden import ref_harness as rh
    arr = rh.load_stream("1000")
    policy = get_policy("rand3")
    ref = rh.RefRunner(arr, policy, want_state=True, **kw)
    orc = OracleEnv(arr, **kw)
    coll = locks = 0
    for t in range(TICKS):
        vid, ctl, obs0 = ref.alive_view()
        vid2, ctl2, obs02 = orc.alive_view()
        assert np.array_equal(vid, vid2) and np.array_equal(ctl, ctl2)
        assert np.allclose(obs0, obs02, rtol=0, atol=1e-12)
        acts = policy(t, vid, ctl, obs0)
        ra = ref.tick(acts)
        rb = orc.tick(acts, want_state=True)
        compare_records(ra, rb, tol=1e-12, label="kw_" + name)
        coll += rb["collisions"]; locks += rb["lock"]
    assert orc.ref_would_raise == 0
    assert coll > 0 and locks > 0, "the tape must provoke collisions and dead-locks (%d, %d)" % (coll, locks)


@pytest.mark.parametrize("name,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_emulated_kernels_vs_oracle_under_ctor_kwargs(name, kw):
    scenarios.check_split_vs_oracle(KwCase(name, kw), "emu", ticks=TICKS)


def test_emulated_step_many_under_ctor_kwargs():
    """the resident loop (and, PVE_EMU_HOME, the HOME block) with every argument moved: == single ticks"""
    scenarios.check_step_many("emu", "table", n_envs=3, chunks=(1, 7, 40, 3, 60), trajectory_chunk=12, seed=201, cfg=ALL_KW)
    os.environ["PVE_EMU_HOME"] = "1"
    try:
        scenarios.check_step_many("emu", "pool", n_envs=3, chunks=(9, 40, 33), trajectory_chunk=12, seed=202, cfg=ALL_KW, persistent=True)
    finally:
        del os.environ["PVE_EMU_HOME"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_gpu_kernels_vs_oracle_under_ctor_kwargs(name, kw):
    scenarios.check_split_vs_oracle(KwCase(name, kw), "hip", ticks=TICKS)
    if name in ("accel", "all"):                       # the capacity-64 kernels too (their own instantiation of every phase;
        # the 200 veh/h stream: the 1000 one needs more than 64 slots)
        scenarios.check_split_vs_oracle(KwCase(name, kw, ticks=400, stream_name="200"), "hip", ticks=400, capacity=64)


@pytest.mark.gpu
@pytest.mark.parametrize("source,persistent", [("table", True), ("pool", True), ("zero", False), ("table", False)])
def test_gpu_step_many_under_ctor_kwargs(source, persistent):
    """k_rollout (plain / queue form; the HOME build for the 128-slot queue form) with every argument moved == single ticks of
    k_tick, which the test above holds to the oracle"""
    scenarios.check_step_many("hip", source, n_envs=5, chunks=(1, 7, 40, 3, 60), trajectory_chunk=12, seed=203, cfg=ALL_KW,
                              persistent=persistent)


# ---------------------------------------------------------------- the 4- / 8-lane layouts (general-geometry kernels)
GEO_LANES = (4, 8)
GEO_PARAMS = [(ln, name, kw) for ln in GEO_LANES for name, kw in VARIANTS]
GEO_IDS = ["%d-%s" % (ln, name) for ln, name, _ in GEO_PARAMS]
# capacity 64 (its own instantiation of every phase): the 4-lane stream below peaks under 64 vehicles in these variants
GEO_CAP64 = [(name, kw) for name, kw in VARIANTS if name in ("accel", "accel_asym", "vm6", "all")]
# veh/h/lane of the batched tests under ALL_KW: deltaT = 0.2 and dis_ctl = 120 change the density, so these were chosen on the
# oracle alone (300 ticks, 8 envs: peak 40 / 50 / 68 vehicles alive, hundreds of collisions and dead-locks, no deferred spawn)
GEO_RATE = {(4, 64): 1500.0, (4, 128): 3000.0, (8, 128): 1600.0}
GEO_SHAPES = [(4, 128), (8, 128), (4, 64)]


def test_all_kw_is_what_the_fixture_generator_used():
    from tests.golden.gen_golden_geo import ALL_KW as generator_kw
    assert generator_kw == ALL_KW


class GeoKwCase:
    """what scenarios.check_geo_vs_oracle needs of a golden case, without a fixture: the synthetic stream (and the 8-lane
    intention draws) of tests/golden/gen_golden_geo.py, mean gap 1.2 s, seed 900 + lane_num"""

    def __init__(self, lane_num, name, kw, ticks=TICKS):
        from tests.golden.gen_golden_geo import make_stream
        self.name = "geo%d_kw_%s" % (lane_num, name)
        self.lane_num = lane_num
        self.arrive, self.choice = make_stream(lane_num, 400, 1.2, 900 + lane_num)
        self.ctor = dict(kw)
        self.policy = get_policy("rand3")
        self.ticks = ticks


@pytest.mark.reference
@pytest.mark.parametrize("lane_num,name,kw", GEO_PARAMS, ids=GEO_IDS)
def test_geo_oracle_vs_live_reference_under_ctor_kwargs(lane_num, name, kw):
    from oracle.oracle_geo import OracleGeoEnv
    from tests.golden import ref_harness as rh
    case = GeoKwCase(lane_num, name, kw)
    ref = rh.GeoRefRunner(case.arrive, lane_num, case.policy, choice=case.choice, want_state=True, **kw)
    try:
        orc = OracleGeoEnv(case.arrive, lane_num, choice=case.choice, **kw)
        coll = locks = 0
        for t in range(TICKS):
            vid, ctl, obs0 = ref.alive_view()
            vid2, ctl2, obs02 = orc.alive_view()
            assert np.array_equal(vid, vid2) and np.array_equal(ctl, ctl2)
            assert np.allclose(obs0, obs02, rtol=0, atol=1e-12)
            acts = case.policy(t, vid, ctl, obs0)
            ra = ref.tick(acts)
            rb = orc.tick(acts, want_state=True)
            compare_records(ra, rb, tol=1e-12, label=case.name)
            assert np.array_equal(ra["intent"], rb["intent"]), "intent differs at tick %d" % t
            assert ra["intention_re"] == rb["intention_re"], "intention_re differs at tick %d" % t
            coll += rb["collisions"]; locks += rb["lock"]
    finally:
        ref.close()
    assert orc.ref_would_raise == 0
    assert coll > 0 and locks > 0, "the tape must provoke collisions and dead-locks (%d, %d)" % (coll, locks)


@pytest.mark.parametrize("name", ["geo_g4_rand_kw", "geo_g8_rand_kw", "geo_g4_rand_vm6"])
def test_geo_kw_fixtures_record_collisions_and_dead_locks(name):
    """the fixtures carry their constructor arguments and did provoke what they are for, without the harness's crash guard"""
    from tests.parity_util import GoldenCase
    from oracle.record import DIGEST_I_COLS
    case = GoldenCase(name)
    assert case.ctor == ({"vm": 6} if name.endswith("vm6") else ALL_KW) and case.meta["policy"] == "rand3"
    assert case.lane_num == (8 if "g8" in name else 4) and 300 <= case.ticks <= 600
    assert int(case.z["guard_hits"]) == 0
    coll = int(case.dig_i[:, DIGEST_I_COLS.index("collisions")].sum())
    locks = int(case.dig_i[:, DIGEST_I_COLS.index("lock")].sum())
    assert coll > 0 and locks > 0, (coll, locks)


def geo_tick_vs_oracle(backend, lane_num, name, kw):
    """(a) the tick kernel, split protocol, single env, 300 ticks, every field of every tick at 1e-9"""
    scenarios.check_geo_vs_oracle(GeoKwCase(lane_num, name, kw), backend, ticks=TICKS, capacity=128)


def geo_fuzz_all_kw(backend, lane_num, cap):
    """(b) fused ticks on a batch of 8 under ALL_KW, one continuous and one quantised tape (exact ties); 4 x 128 is
    TickGeo::walk_merge4 with the far-conflict constants of lane_cw = 3"""
    for quantize, seed in ((None, 300), (1.0, 301)):
        coll, lock = scenarios.check_geo_fuzz_vs_oracle(backend, lane_num, n_envs=8, capacity=cap, ticks=300, rate=GEO_RATE[lane_num, cap],
                                                        seed=seed + lane_num + cap, quantize=quantize, cfg=ALL_KW)
        print("fused ticks under ALL_KW, %d lanes x %d slots, quantize %s: %d collisions, %d dead-locks" % (lane_num, cap, quantize, coll, lock))
        assert coll > 0 and lock > 0, (coll, lock)          # (overflow == 0 is asserted by the helper)


def geo_step_many_all_kw(backend, lane_num, cap, source, persistent):
    """(c) k_rollout_geo[<.., IDT>][<.., PERS>] == single ticks of k_tick_geo under ALL_KW, bit for bit"""
    m = scenarios.check_step_many_geo(backend, lane_num, n_envs=9, capacity=cap, chunks=(1, 7, 40, 25), trajectory_chunk=12,
                                      rate=GEO_RATE[lane_num, cap], source=source, persistent=persistent, cfg=ALL_KW, seed=310 + lane_num)
    print("roll-out under ALL_KW, %d lanes x %d slots, %s, persistent=%s: %s" % (
        lane_num, cap, source, persistent, {k: int(m[k]) for k in ("ctl_steps", "collided", "locks", "overflow")}))
    assert m["collided"] > 0 and m["locks"] > 0 and m["overflow"] == 0, m


def geo_closed_loop(backend, lane_num, dtype, persistent, cfg):
    """(d) the closed loop (actor inside k_rollout_geo<.., ACT[, PERS]>) == actor launch + tick, after the two-launch form was
    held to the oracle for 60 ticks; 4 lanes x 128 slots with float32 rows is the shipped checkpoint's layout"""
    m = scenarios.check_step_many_geo_actor(backend, lane_num, n_envs=12, capacity=128, chunks=(1, 9, 30, 4, 45), obs_dtype=dtype,
                                            persistent=persistent, oracle_ticks=60, cfg=cfg)
    print("closed loop, %d lanes, persistent=%s, %s: %s" % (lane_num, persistent, sorted(cfg), {k: int(m[k]) for k in ("ctl_steps", "collided", "locks")}))


def geo_training_outputs(backend, lane_num, dtype):
    """(e) the training outputs of the roll-out through the work queue (k_rollout_geo<.., TRAIN, PERS>) under ALL_KW: 7 x 28
    states and 7-action vectors of every tick against the oracle"""
    n = scenarios.check_step_many_state_rows(backend, n_envs=12, capacity=128, calls=(30, 17, 40), chunk=7, lane_num=lane_num, persistent=True,
                                             obs_dtype=dtype, min_ctl_per_tick=1, rate=GEO_RATE[lane_num, 128], cfg=ALL_KW, seed=320 + lane_num)
    print("training outputs under ALL_KW, %d lanes: %d controlled vehicle-ticks" % (lane_num, n))


def geo_closed_loop_training(backend, lane_num, dtype):
    """the closed loop WITH the training outputs (k_rollout_geo<.., TRAIN, .., ACT>) under ALL_KW == actor launch + tick"""
    scenarios.check_closed_loop_state_rows(backend, n_envs=12, capacity=128, calls=(30, 17, 40), chunk=7, lane_num=lane_num, obs_dtype=dtype,
                                           rate=GEO_RATE[lane_num, 128], cfg=ALL_KW, seed=330 + lane_num,
                                           want_launch=("resident",))


CLOSED_LOOP = [(ln, dt, pers, cname) for cname in ("vm6", "all") for ln, dt in ((4, torch.float32), (8, torch.float64)) for pers in (False, True)]
STEP_MANY = [(ln, cap, src, pers) for ln, cap in GEO_SHAPES for src in ("pool", "table") for pers in (False, True)]
CFGS = {"vm6": {"vm": 6}, "all": ALL_KW}


# ---- CPU: the emulated twins, same shapes
@pytest.mark.parametrize("lane_num,name,kw", GEO_PARAMS, ids=GEO_IDS)
def test_emulated_geo_kernels_vs_oracle_under_ctor_kwargs(lane_num, name, kw):
    geo_tick_vs_oracle("emu", lane_num, name, kw)


@pytest.mark.parametrize("name,kw", GEO_CAP64, ids=[v[0] for v in GEO_CAP64])
def test_emulated_geo_kernels_vs_oracle_under_ctor_kwargs_capacity_64(name, kw):
    scenarios.check_geo_vs_oracle(GeoKwCase(4, name, kw), "emu", ticks=TICKS, capacity=64)


@pytest.mark.parametrize("lane_num,cap", [(4, 64), (4, 128), (8, 128)])
def test_emulated_geo_fused_ticks_under_ctor_kwargs(lane_num, cap):
    geo_fuzz_all_kw("emu", lane_num, cap)


@pytest.mark.parametrize("lane_num,cap,source,persistent", STEP_MANY)
def test_emulated_geo_step_many_under_ctor_kwargs(lane_num, cap, source, persistent):
    geo_step_many_all_kw("emu", lane_num, cap, source, persistent)


@pytest.mark.parametrize("lane_num,dtype,persistent,cfg", CLOSED_LOOP)
def test_emulated_geo_closed_loop_under_ctor_kwargs(lane_num, dtype, persistent, cfg):
    geo_closed_loop("emu", lane_num, dtype, persistent, CFGS[cfg])


@pytest.mark.parametrize("lane_num,dtype", [(4, torch.float32), (8, torch.float64)])
def test_emulated_geo_training_outputs_under_ctor_kwargs(lane_num, dtype):
    geo_training_outputs("emu", lane_num, dtype)
    geo_closed_loop_training("emu", lane_num, dtype)


# ---- the HIP kernels
@pytest.mark.gpu
@pytest.mark.parametrize("lane_num,name,kw", GEO_PARAMS, ids=GEO_IDS)
def test_gpu_geo_kernels_vs_oracle_under_ctor_kwargs(lane_num, name, kw):
    """k_tick_geo<128, ..> (4 lanes: FIX4) against the oracle with each argument moved on its own and all together"""
    geo_tick_vs_oracle("hip", lane_num, name, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", GEO_CAP64, ids=[v[0] for v in GEO_CAP64])
def test_gpu_geo_kernels_vs_oracle_under_ctor_kwargs_capacity_64(name, kw):
    scenarios.check_geo_vs_oracle(GeoKwCase(4, name, kw), "hip", ticks=TICKS, capacity=64)


@pytest.mark.gpu
@pytest.mark.parametrize("lane_num,cap", [(4, 64), (4, 128), (8, 128)])
def test_gpu_geo_fused_ticks_under_ctor_kwargs(lane_num, cap):
    geo_fuzz_all_kw("hip", lane_num, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("lane_num,cap,source,persistent", STEP_MANY)
def test_gpu_geo_step_many_under_ctor_kwargs(lane_num, cap, source, persistent):
    geo_step_many_all_kw("hip", lane_num, cap, source, persistent)


@pytest.mark.gpu
@pytest.mark.parametrize("lane_num,dtype,persistent,cfg", CLOSED_LOOP)
def test_gpu_geo_closed_loop_under_ctor_kwargs(lane_num, dtype, persistent, cfg):
    geo_closed_loop("hip", lane_num, dtype, persistent, CFGS[cfg])


@pytest.mark.gpu
@pytest.mark.parametrize("lane_num,dtype", [(4, torch.float32), (8, torch.float64)])
def test_gpu_geo_training_outputs_under_ctor_kwargs(lane_num, dtype):
    geo_training_outputs("hip", lane_num, dtype)
    geo_closed_loop_training("hip", lane_num, dtype)

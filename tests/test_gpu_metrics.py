"""-m gpu: the metrics vector (pve_get_metrics) of every kernel family against the reference accumulator (tests/metrics_ref.py).
On the device sum_reward / sum_jerk come out of the block reductions (DPP trees per wave, one partial per wave in LDS, the
ballot skip of the sparse form, thread 0's sum in FIN) and the counters out of two code shapes (accumulated in LDS across the
ticks of an item, or written to the header every tick); the emulator runs neither.  The scenarios, their reach conditions and
the CPU twin: tests/metrics_scenarios.py, tests/test_metrics.py.  Every float comparison prints its measured deviation.

Largest deviation seen on an MI355X, as a fraction of the bar 1e-9 x sum(max(1, |term|)) (sum_reward / sum_jerk):
  k_tick, k_rollout (12 lanes; step, split, pool, table, zero; register and HOME builds, queue)   4.4e-7 / 0
  k_tick_geo, k_rollout_geo (4 lanes | 8 lanes)                                                   6.2e-7 | 5.3e-7 / 0
  closed loop (two-launch form, resident, queue; with and without noise)                          1.1e-7 / 1.7e-7
  golden digests summed (s1000_rand_kw, s1200_sin1, geo_g8_rand_kw; fused ticks)                  6.9e-7 / 0
i.e. absolute deviations of 1e-12 .. 1e-11 on sums of 1e3 .. 1e5; every counter exact."""
import os

import pytest
import torch

from tests import metrics_scenarios as S

pytestmark = pytest.mark.gpu
BACKEND = "hip"
QUEUE = dict(persistent=True, launch="persistent")


# ------------------------------------------------------------------ k_tick / k_tick_geo: fused and split, every width
@pytest.mark.parametrize("form", ["step", "split"])
@pytest.mark.parametrize("name", ["l12_c64", "l12_c128", "l12_c256", "l4_c64", "l4_c128", "l8_c64", "l8_c128"])
def test_gpu_tick_metrics(name, form):
    S.check_open_loop(BACKEND, name, form)


# ------------------------------------------------------------------ full intersections: `overflow` against capacity-bound oracles
@pytest.mark.parametrize("form,kw", [("step", {}), ("split", {}), ("pool", dict(launch="resident")), ("pool", dict(chunk=7, **QUEUE)),
                                     ("table", dict(chunk=1, **QUEUE))])
@pytest.mark.parametrize("name", sorted(S.FULL_SPECS))
def test_gpu_metrics_full_intersections(name, form, kw):
    """overflowing bursts, one per kernel family (12 lanes at 64 slots and at the HOME build's 128, 4 lanes, 8 lanes): all twelve
    sums through the deferred spawns, `overflow` = the bounded oracles' deferral counts, the float sums at their usual bars"""
    S.check_open_loop(BACKEND, name, form, **kw)


def test_gpu_tick_metrics_float32_rows():
    S.check_open_loop(BACKEND, "l12_c128", "step", obs_dtype=torch.float32)


# ------------------------------------------------------------------ k_rollout / k_rollout_geo through step_many
@pytest.mark.parametrize("kw", [dict(launch="resident"), dict(chunk=1, **QUEUE), dict(chunk=7, **QUEUE)])
@pytest.mark.parametrize("name", ["l12_c64", "l12_c256", "l4_c64", "l4_c128", "l8_c64", "l8_c128"])
def test_gpu_rollout_metrics(name, kw):
    S.check_open_loop(BACKEND, name, "pool", **kw)


@pytest.mark.parametrize("name,source", [("l12_c128", "pool"), ("l12_c128", "table"), ("l12_c128_zero", "zero")])
@pytest.mark.parametrize("chunk", [1, 7])
def test_gpu_home_kernel_metrics(name, source, chunk):
    """the HOME build: the queue form at 128 slots"""
    S.check_open_loop(BACKEND, name, source, chunk=chunk, waves=5, **QUEUE)


def test_gpu_rollout_metrics_register_build_128():
    S.check_open_loop(BACKEND, "l12_c128", "pool", launch="resident", waves=4)
    S.check_open_loop(BACKEND, "l12_c128", "table", chunk=7, launch="resident", waves=4)


@pytest.mark.parametrize("kw", [dict(launch="resident"), dict(chunk=7, **QUEUE)])
def test_gpu_rollout_metrics_training_outputs(kw):
    S.check_open_loop(BACKEND, "l12_c128", "pool", outputs=S.TRAIN_OUTS, **kw)


@pytest.mark.parametrize("name", ["l4_c128_kw", "l8_c64_kw"])
def test_gpu_geo_metrics_constructor_arguments(name):
    S.check_open_loop(BACKEND, name, "step")
    S.check_open_loop(BACKEND, name, "pool", chunk=7, **QUEUE)


# ------------------------------------------------------------------ closed loop: the device's own actions drive the oracle
@pytest.mark.parametrize("lane_num,capacity,kw", [(12, 128, {}), (12, 256, {}), (12, 128, dict(noisy=True)),
                                                  (4, 128, dict(cfg=dict(vm=6.0)))])
def test_gpu_closed_loop_metrics(lane_num, capacity, kw):
    S.check_closed_loop(BACKEND, lane_num, capacity, **kw)
    S.check_closed_loop(BACKEND, lane_num, capacity, chunk=7, persistent=True, **kw)


# ------------------------------------------------------------------ a batch of very different populations; reset()
def test_gpu_batch_of_five_and_reset():
    S.check_open_loop(BACKEND, "l12_c128_five", "step", replay=True)
    S.check_open_loop(BACKEND, "l12_c128_five", "pool", chunk=7, replay=True, **QUEUE)


def test_gpu_batch_of_five_pipelined():
    S.check_open_loop(BACKEND, "l12_c128_five", "pool", chunk=7, pipelined=2)


# ------------------------------------------------------------------ the reference's own arithmetic, no oracle in between
@pytest.mark.parametrize("name", ["s1000_rand_kw", "s1200_sin1", "geo_g8_rand_kw"])
def test_gpu_metrics_equal_golden_digests(name):
    S.check_golden_anchor(BACKEND, name, ticks=400)


# ------------------------------------------------------------------ evaluate() on the device
def test_gpu_evaluate_protocol():
    """pve_mcc_amd.evaluate.evaluate on the shipped 1000 stream, 1000 ticks, on the device: the bars the project holds for this
    closed loop (tests/actor_scenarios.py: 323 vehicles, no collision, |passed - 281| <= 3, |pT-m - 12.294| < 0.15, no
    overflow), reward_mean within 2 % of SURVEY App. D's 1.30294 (the drift bar for sum_reward between the split-half and the
    exact actor).  jerk_mean has no bar in the project: it is held to the value the same call returns through the emulator
    (208.799) at three times the measured relative deviation and not below 1 %.
    Measured on an MI355X: vehicles 323, passed 281, collisions 0, lock_num 548, pT_m 12.294302, reward_mean 1.3029424,
    jerk_mean 208.799278: 1.3e-6 (relative) off 208.799, which is the rounding of that printed figure.  Three times that is
    4e-6, so the bar is the 1 % floor.  The figures are printed."""
    from oracle.actor_np import load_weights
    from pve_mcc_amd.arrivals import load_arrival_mat, pad_stream
    from pve_mcc_amd.evaluate import evaluate
    from tests.parity_util import GOLDEN_DIR
    arr = pad_stream(load_arrival_mat(os.path.join(GOLDEN_DIR, "streams", "arvTimeNewVeh_new_1000_12.mat")))
    res = evaluate(arr, load_weights(), ticks=1000)
    rel_jerk = abs(res["jerk_mean"] - 208.799) / 208.799
    print("evaluate() on the device: %r; jerk_mean off 208.799 by %.3e (relative)" % (res, rel_jerk))
    assert res["vehicles"] == 323 and res["collisions"] == 0 and res["overflow"] == 0
    assert abs(res["passed"] - 281) <= 3
    assert abs(res["pT_m"] - 12.294) < 0.15
    assert abs(res["reward_mean"] - 1.30294) <= 0.02 * 1.30294
    assert rel_jerk <= 0.01

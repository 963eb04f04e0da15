"""The arrival generator's kernels (csrc/pve_arrivals.h: k_gen_arrivals, k_gen_intentions) against the NumPy model
(pve_mcc_amd.arrivals.device_arrivals / device_intentions) bit for bit, and generate_arrivals as the input of roll-outs."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import pve_mcc_amd
from pve_mcc_amd import _capi, arrivals as AR, distributed
from tests import scenarios

pytestmark = pytest.mark.gpu

TILE, GROUP = 64, 4                      # ARR_TILE, ARR_GROUP of csrc/pve_arrivals.h
GUARD = 256                              # bytes behind every buffer that must keep their fill
# the shapes of the CPU test (tests/test_arrivals_device.py) and rows around the tile: one tile, several, a partial last one, a last
# tile that holds the padding row alone (T + 1, 2T + 1); 1 / 5 / 17 environments: a partial group, one full + partial, four + partial
ROWS = (2, 3, 5, 6, 33, 130, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 2 * TILE + 3)
VARIANTS = [dict(min_gap=1.0), dict(min_gap=0.0, env_offset=3, epoch=1),
            dict(min_gap=0.0, env_offset=(1 << 32) - 2, epoch=(1 << 32) - 1, seed=0xFEDCBA9876543210),
            dict(min_gap=1.0, rate=3600.0 / 1e-3, epoch=1), dict(min_gap=0.5, rate=3600.0 / 1e6, seed=77, env_offset=(1 << 32) - 2)]


def filled(nbytes):
    return torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")


def raw_generate(b, rows, rate, seed=0, epoch=0, env_offset=0, min_gap=1.0, block_threads=0, intentions=False):
    """pve_generate_arrivals into 0xFF-filled buffers -> (arrivals, intentions or None, covered) as NumPy; the guards are checked"""
    E, ln = b.n_envs, b.lane_num
    n = E * rows * ln
    arr, ch, cov = filled(8 * n), filled(4 * n) if intentions else None, filled(8 * E)
    g = _capi.PveArrivalGen(seed=int(seed) & 0xFFFFFFFFFFFFFFFF, env_offset=env_offset, epoch=epoch & 0xFFFFFFFF, rows=rows, mean_s=1.0,
                            mean_env=None, min_gap_s=min_gap, block_threads=block_threads)
    mean = None
    if np.ndim(rate) > 0:
        mean = torch.as_tensor(AR.device_mean(rate, E)).cuda()
        g.mean_env = mean.data_ptr()
    else:
        g.mean_s = 3600.0 / float(rate)
    b._bind_stream()
    rc = b.lib.pve_generate_arrivals(b._h, C.byref(g), C.c_void_p(arr.data_ptr()), C.c_void_p(ch.data_ptr()) if intentions else None,
                                     C.c_void_p(cov.data_ptr()))
    assert rc == 0, b.lib.pve_last_error()
    b.synchronize()
    for buf, used in ((arr, 8 * n), (ch, 4 * n), (cov, 8 * E)):
        if buf is not None:
            assert bool((buf[used:] == 0xFF).all()), "guard region written"
    return (arr[:8 * n].cpu().numpy().view(np.float64).reshape(E, rows, ln),
            ch[:4 * n].cpu().numpy().view(np.int32).reshape(E, rows, ln) if intentions else None, cov[:8 * E].cpu().numpy().view(np.float64))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def blank(n_envs, lane_num, capacity=64, **kw):
    return pve_mcc_amd.BatchedIntersections(n_envs, capacity, None, device="cuda", lane_num=lane_num, **kw)


@pytest.mark.parametrize("lane_num", [4, 8, 12])
def test_kernels_equal_the_numpy_model_bit_for_bit(lane_num):
    variants = itertools.cycle(VARIANTS)
    blocks = itertools.cycle([0, 64, 1024, 192])
    for n_envs in (1, 5, 17):
        b = blank(n_envs, lane_num, outputs=("obs_post",))
        for rows in ROWS:
            kw = dict(next(variants))
            rate = kw.pop("rate", None)
            per_env = (rows + n_envs) % 2 == 1
            if per_env:
                rate = np.linspace(200.0, 1200.0, n_envs) if rate is None else np.full(n_envs, rate)
            elif rate is None:
                rate = 1100.0
            want_a = AR.device_arrivals(n_envs, rows, lane_num, rate, **kw)
            want_c = AR.device_intentions(n_envs, rows, **{k: v for k, v in kw.items() if k != "min_gap"})
            for block in (next(blocks), next(blocks)):
                a, c, cov = raw_generate(b, rows, rate, block_threads=block, intentions=lane_num == 8, **kw)
                what = (n_envs, rows, lane_num, block, kw)
                assert np.array_equal(bits(a), bits(want_a)), what
                assert np.array_equal(bits(cov), bits(AR.device_covered(want_a))), what
                if lane_num == 8:
                    assert np.array_equal(c, want_c), what
        b.close()


def test_headline_rows_and_intentions_past_one_philox_call():
    """432 rows (the 600 s episode at 1100 veh/h/lane): seven tiles, the last partial; 300 rows of intentions: three Philox calls per
    (env, lane), the last partial; without `covered`."""
    b = blank(9, 8, outputs=("obs_post",))
    cov = b.generate_arrivals(1100.0, horizon_s=600.0, seed=12345, epoch=7, env_offset=5)
    assert cov is None and tuple(b.arrivals.shape) == (9, 432, 8) and tuple(b.intentions.shape) == (9, 432, 8)
    assert np.array_equal(bits(b.arrivals.cpu().numpy()), bits(AR.device_arrivals(9, 432, 8, 1100.0, seed=12345, epoch=7, env_offset=5)))
    assert np.array_equal(b.intentions.cpu().numpy(), AR.device_intentions(9, 432, seed=12345, epoch=7, env_offset=5))


def rollout(b, ticks=64, pool=None):
    if pool is not None:
        b.set_action_pool(pool)
    b.reset()
    return b.step_many(ticks)


def assert_same_rollout(b1, out1, b2, out2, what):
    torch.cuda.synchronize()
    assert set(out1) == set(out2)
    for k in out1:
        assert torch.equal(out1[k].view(torch.uint8), out2[k].view(torch.uint8)), "%s: output %s differs" % (what, k)
    scenarios.batches_equal(b1, b2, what)
    assert b1.metrics() == b2.metrics() and b1.metrics()["alive_steps"] > 0, what


@pytest.mark.parametrize("lane_num,rate", [(12, 1100.0), (8, 1500.0)])
def test_generated_episode_equals_the_uploaded_model_stream(lane_num, rate):
    """generate -> reset -> step_many(64) against a batch fed device_arrivals through set_arrivals; then the next epoch into the same
    buffers with no synchronisation in between, against a fresh batch on the model's stream of that epoch."""
    E, cap, outputs = 4, 128, ("obs_post", "reward", "flags", "lanej", "env_out", "new_slot")
    rows = AR.default_rows(rate, 40.0)
    pool = np.random.default_rng(5).uniform(-2, 2, size=(7, E, cap)).astype(np.float32).astype(np.float64)
    g = blank(E, lane_num, cap, outputs=outputs)
    g.set_action_pool(pool)
    ptr = None
    outs = []
    for epoch in (3, 4):                                     # (enqueued back to back: the second generation overwrites the first's buffers)
        cov = g.generate_arrivals(rate, rows=rows, seed=21, epoch=epoch, covered=True)
        assert ptr in (None, g.arrivals.data_ptr())
        ptr = g.arrivals.data_ptr()
        g.reset()
        outs.append(({k: v.clone() for k, v in g.step_many(64).items()}, cov))
        if epoch == 3:
            snap = pve_mcc_amd.BatchedIntersections(E, cap, AR.device_arrivals(E, rows, lane_num, rate, seed=21, epoch=3), device="cuda",
                                                    lane_num=lane_num, outputs=outputs,
                                                    intentions=AR.device_intentions(E, rows, seed=21, epoch=3) if lane_num == 8 else None)
            assert_same_rollout(g, outs[0][0], snap, rollout(snap, pool=pool), "epoch 3, %d lanes" % lane_num)
    want = AR.device_arrivals(E, rows, lane_num, rate, seed=21, epoch=4)
    fresh = pve_mcc_amd.BatchedIntersections(E, cap, want, device="cuda", lane_num=lane_num, outputs=outputs,
                                             intentions=AR.device_intentions(E, rows, seed=21, epoch=4) if lane_num == 8 else None)
    assert_same_rollout(g, outs[1][0], fresh, rollout(fresh, pool=pool), "epoch 4, %d lanes" % lane_num)
    assert np.array_equal(bits(g.arrivals.cpu().numpy()), bits(want))
    assert np.array_equal(bits(outs[1][1].cpu().numpy()), bits(AR.device_covered(want)))
    assert np.array_equal(bits(outs[0][1].cpu().numpy()), bits(AR.device_covered(AR.device_arrivals(E, rows, lane_num, rate, seed=21, epoch=3))))


def test_regeneration_without_a_synchronisation_between_the_launches():
    """Two generations into the same buffers and a roll-out enqueued with nothing read in between: the epoch + 1 stream rules."""
    E, cap, rate, outputs = 4, 128, 1100.0, ("obs_post", "reward", "flags", "env_out")
    rows = AR.default_rows(rate, 40.0)
    g = blank(E, 12, cap, outputs=outputs)
    g.generate_arrivals(rate, rows=rows, seed=2, epoch=0)
    g.reset()
    g.step_many(64)
    g.generate_arrivals(rate, rows=rows, seed=2, epoch=1)
    g.reset()
    out = g.step_many(64)
    fresh = pve_mcc_amd.BatchedIntersections(E, cap, AR.device_arrivals(E, rows, 12, rate, seed=2, epoch=1), device="cuda", outputs=outputs)
    assert_same_rollout(g, out, fresh, rollout(fresh), "regenerated")


def test_pipelined_sub_batches_equal_one_batch():
    E, cap, rows = 5, 128, 100
    rate = np.array([200.0, 1200.0, 700.0, 1100.0, 450.0])
    outputs = ("obs_post", "reward", "flags", "env_out")
    pipe = pve_mcc_amd.PipelinedIntersections(E, cap, None, n_sub=2, outputs=outputs)
    cov = pipe.generate_arrivals(rate, rows=rows, seed=11, epoch=2, covered=True)
    one = blank(E, 12, cap, outputs=outputs)
    cov1 = one.generate_arrivals(rate, rows=rows, seed=11, epoch=2, covered=True)
    pipe.reset()
    pipe.step_many(40)
    one.reset()
    one.step_many(40)
    pipe.synchronize()
    one.synchronize()
    want = AR.device_arrivals(E, rows, 12, rate, seed=11, epoch=2)
    assert np.array_equal(bits(torch.cat([s.arrivals for s in pipe.subs]).cpu().numpy()), bits(want))
    assert np.array_equal(bits(one.arrivals.cpu().numpy()), bits(want))
    assert torch.equal(torch.cat(cov), cov1) and np.array_equal(bits(cov1.cpu().numpy()), bits(AR.device_covered(want)))
    for k in scenarios.STATE_F + scenarios.STATE_I:
        assert torch.equal(torch.cat([s.state_field(k) for s in pipe.subs]), one.state_field(k)), k
    assert pipe.metrics() == one.metrics() and one.metrics()["alive_steps"] > 0


def test_mixed_rates_in_one_batch_and_shards():
    """Half the batch at 200, half at 1200 veh/h/lane; the rate as an array, as a device tensor, and cut into shards."""
    E, ln = 6, 12
    rate = np.array([200.0] * 3 + [1200.0] * 3)
    rows = AR.default_rows(rate, 60.0)
    assert rows == AR.default_rows(1200.0, 60.0)
    want = AR.device_arrivals(E, rows, ln, rate, seed=3)
    b = blank(E, ln, outputs=("obs_post",))
    b.generate_arrivals(rate, horizon_s=60.0, seed=3)
    assert np.array_equal(bits(b.arrivals.cpu().numpy()), bits(want))
    cov = b.generate_arrivals(torch.as_tensor(rate).cuda(), rows=rows, seed=3, covered=True)
    assert np.array_equal(bits(b.arrivals.cpu().numpy()), bits(want)) and np.array_equal(bits(cov.cpu().numpy()), bits(AR.device_covered(want)))
    slow, fast = want[:3, :-1], want[3:, :-1]
    assert slow[:, -1].min() > 3.0 * fast[:, -1].max()                         # (mean gaps 18 s and 3 s)
    for rank in range(2):
        lo, hi = distributed.shard_range(E, rank, 2)
        s = blank(hi - lo, ln, outputs=("obs_post",))
        distributed.generate_shard_arrivals(s, rate, E, rank, 2, horizon_s=60.0, seed=3)
        assert np.array_equal(bits(s.arrivals.cpu().numpy()), bits(want[lo:hi]))

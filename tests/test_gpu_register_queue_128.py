"""-m gpu: the two builds of the 128-slot queue kernel on either side of the `rows` boundary, and the HOME build's packed word at
the top of its range.

k_rollout<128, 5, .., PERS> (HOME: the carried per-slot fields in LDS homes) packs seq_in_lane << 8 | id_info[1] into one word,
which holds arrival cursors below 2^23; a stream of rows >= 2^23 takes the register build k_rollout<128, 4, .., PERS> instead.
Since HOME became the default nothing launched that kernel for the zero, pool and table sources.  Here one SHARED stream
[rows, 12] of +inf with the first rows of a 1100 veh/h/lane stream in front (805 MB at rows = 2^23, alive for one test at a
time) sends the same call to either build -- last_variant() says which, as literals -- and both are held, bit for bit, to one
launch per tick and to the HOME run of the same first rows in a short stream.  Then the packed word: seq = 2^23 - 2 - slot
written into every live slot of a HOME run comes back unchanged."""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import launch_matrix_scenarios as lm
from tests import scenarios
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
BACKEND = "hip"
N_ENVS, CAP, CHUNKS, ITEM = 5, 128, (20, 9, 33), 7
OUTS = ("obs_post", "reward", "flags", "nbr", "new_slot", "env_out", "lanej")
BOUNDARY = 1 << 23

_shared = {}


def _inputs():
    """the short stream, the action tape and the table: computed once, never written"""
    if not _shared:
        rng = np.random.default_rng(823)
        _shared["arr"] = synthetic_arrivals(1, rate=1100.0, horizon_s=sum(CHUNKS) * 0.1 + 30, seed=823)[0]
        _shared["pool"] = torch.as_tensor(rng.uniform(-3, 3, size=(5, N_ENVS, CAP)))
        _shared["table"] = torch.as_tensor(rng.uniform(-3, 3, size=(7, 40)))
    return _shared["arr"], _shared["pool"], _shared["table"]


def _batch(arr, source):
    _arr, pool, table = _inputs()
    b = make_batch(arr, N_ENVS, CAP, BACKEND, outputs=OUTS)
    b.reset()
    if source == "table":
        b.set_action_table(table)
    if source == "pool":
        b.set_action_pool(pool)
    return b


def _single(b, source):
    if source == "table":
        return b.step(b.actions_from_table())
    return b.step(b._pool[b.ticks % b._pool.shape[0]] if source == "pool" else None)


def _long_stream(rows):
    """[rows, 12] of +inf on the device, the short stream in front"""
    arr = _inputs()[0]
    long = torch.full((rows, 12), float("inf"), dtype=torch.float64, device="cuda")
    long[:arr.shape[0]] = torch.as_tensor(arr).to(long.device)
    return long


def _variant(source, waves):
    return dict(kind="persistent", family=12, capacity=128, waves_per_simd=waves, prof=0, actor=0, train=0,
                table=int(source == "table"), persistent=1, geo=0, launches=1)


@pytest.mark.parametrize("source", ["zero", "pool", "table"])
@pytest.mark.parametrize("rows,waves", [(BOUNDARY, 4), (BOUNDARY - 1, 5)], ids=["rows-2^23-register", "rows-2^23-1-home"])
def test_gpu_queue_kernel_128_on_either_side_of_the_rows_boundary(rows, waves, source):
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    long = _long_stream(rows)
    case = lm.Case(12, CAP, source, False, True, False, False)
    tick, queue, home = _batch(long, source), _batch(long, source), _batch(_inputs()[0], source)
    n_ctl = 0
    for n in CHUNKS:
        for _ in range(n):
            o1 = _single(tick, source)
        outs = {}
        for name, b, w in (("long stream", queue, waves), ("short stream", home, 5)):
            outs[name] = b.step_many(n, source=source, chunk=ITEM, persistent=True)
            b.synchronize()
            v = b.last_variant()
            grid = v.pop("grid")
            assert b.last_launch() == "persistent" and v == _variant(source, w), (name, rows, source, v)
            sched = (C.c_int32 * 12)()                        # (one workgroup per item: far fewer than the chip holds)
            assert b.lib.pve_debug_item_schedule(n, ITEM, sched) == 0 and grid == N_ENVS * sched[11] <= 6 * N_ENVS, (name, grid)
        assert tick.last_variant()["kind"] == "tick" and tick.last_variant()["waves_per_simd"] == 0
        for name, b in (("long stream", queue), ("short stream", home)):
            what = "%s, rows %d, %s, call of %d ticks" % (name, rows, source, n)
            n_ctl += lm._same_tick(case, o1, outs[name], tick, b.obs, what)
            scenarios.batches_equal(tick, b, what)
            assert tick.metrics() == b.metrics(), what
    m = tick.metrics()
    assert n_ctl > 0 and m["ctl_steps"] > 0 and m["overflow"] == 0 and m["ticks"] == N_ENVS * sum(CHUNKS), m
    peak = torch.cuda.max_memory_allocated() / 2.0 ** 20
    for b in (tick, queue, home):
        b.close()
    del long, tick, queue, home
    torch.cuda.empty_cache()
    print("rows %d, %s: %.2f s wall, peak %.0f MiB of device memory" % (rows, source, time.time() - t0, peak))


def test_gpu_home_packed_word_at_the_top_of_its_range():
    """seq << 8 | vnum with seq = 2^23 - 2 - slot (2^23 - 2 .. 2^23 - 129: the largest values the word holds) in every live slot:
    the HOME queue kernel carries them as the per-tick kernel does -- seq, vnum and id of every live slot -- while the vehicles
    spawned during the run carry their real arrival cursor."""
    arr = _inputs()[0]
    Snapshot = collections.namedtuple("Snapshot", "seq vnum id alive")

    def live(b):
        n = np.array([b.read_env(e).n_alive for e in range(N_ENVS)])
        alive = np.arange(CAP)[None, :] < n[:, None]
        return Snapshot(*(np.where(alive, _np(b.state_field(k)), -1) for k in ("seq", "vnum", "id")), alive)

    tick, queue = _batch(arr, "table"), _batch(arr, "table")
    for _ in range(120):                                   # (traffic first: ~40 vehicles per intersection)
        _single(tick, "table")
    queue.step_many(120, source="table", chunk=25, persistent=True)
    queue.synchronize()
    assert queue.last_variant()["waves_per_simd"] == 5
    top = (BOUNDARY - 2 - torch.arange(CAP, dtype=torch.int32, device=tick.device))[None, :].expand(N_ENVS, CAP)
    before = live(tick)
    assert before.alive.sum() >= 10 * N_ENVS
    for b in (tick, queue):
        mask = torch.as_tensor(before.alive).to(b.device)
        b.state_field("seq")[mask] = top[mask]
        b.synchronize()
    assert live(queue).seq.max() == BOUNDARY - 2
    n_spawned0 = tick.metrics()["spawned"]
    for n in (20, 9):
        for _ in range(n):
            _single(tick, "table")
        queue.step_many(n, source="table", chunk=ITEM, persistent=True)
        queue.synchronize()
        v = queue.last_variant()
        assert (v["kind"], v["waves_per_simd"], v["table"], v["persistent"]) == ("persistent", 5, 1, 1), v
        s1, s2 = live(tick), live(queue)
        for k in ("seq", "vnum", "id"):
            assert np.array_equal(getattr(s1, k), getattr(s2, k)), (k, n)
        scenarios.batches_equal(tick, queue, "packed word at the top of its range, call of %d ticks" % n)
    # survivors still carry the written values; the vehicles spawned since carry cursors of the short stream
    assert (s2.seq >= BOUNDARY - 2 - CAP).sum() >= 5 * N_ENVS and s2.seq.max() <= BOUNDARY - 2
    fresh = s2.alive & (s2.seq < BOUNDARY - 2 - CAP)
    assert tick.metrics()["spawned"] > n_spawned0 and fresh.sum() > 0 and s2.seq[fresh].max() < arr.shape[0]
    assert (s2.vnum[s2.alive] >= 0).all() and (s2.vnum[s2.alive] < 256).all()
    tick.close(); queue.close()

"""The launch matrix of pve_step_many: every combination of layout x capacity x action source x training outputs x launch
form the API accepts, each on a tiny batch.  A case asserts WHICH path ran (last_launch() and last_variant() against literal tables: a backend
that picks a valid but wrong kernel variant, or quietly falls back, fails here) and holds every requested output and the final
state bit-equal to the same ticks run one launch per tick.  Shared by the CPU file (the emulators, their own table) and the
`-m gpu` file."""
import collections

import numpy as np
import torch

from pve_mcc_amd.arrivals import synthetic_arrivals, synthetic_intentions
from tests.hip_adapter import _np, make_batch
from tests.scenarios import batches_equal

# 5 intersections: fewer than the 8 XCD shards of the work queue, so shards are adopted; 11 ticks in chunks of 4: items 4 + 4 + 3
N_ENVS, N_TICKS, CHUNK = 5, 11, 4
SOURCES = ("zero", "pool", "table", "actor")
# arrival rates [veh/h/lane]: the defaults of scenarios.check_step_many / check_step_many_geo / check_step_many_geo_actor
RATE = {12: lambda cap, src: 1100.0,
        8: lambda cap, src: 1300.0 if src == "actor" else 1500.0,
        4: lambda cap, src: (1500.0 if cap == 128 else 1000.0) if src == "actor" else (1800.0 if cap == 128 else 1200.0)}

Case = collections.namedtuple("Case", "lane_num capacity source train persistent obs_f32 actor_f32")


def case_id(c):
    return "l%d-c%d-%s-%s-%s-%s%s" % (c.lane_num, c.capacity, c.source, "train" if c.train else "plain",
                                      "queue" if c.persistent else "resident", "f32" if c.obs_f32 else "f64",
                                      "-exactf32" if c.actor_f32 else "")


def refused(lane_num, source, train):
    """PVE_SRC_TABLE with the training outputs on the 4- / 8-lane layouts: PVE_ERR_INVALID (check_refusal)"""
    return lane_num != 12 and source == "table" and train


def matrix():
    cases = []
    for lane_num, caps in ((12, (64, 128, 256)), (4, (64, 128)), (8, (64, 128))):
        for ci, cap in enumerate(caps):
            for si, source in enumerate(SOURCES):
                for train in (False, True):
                    for persistent in (False, True):
                        if not refused(lane_num, source, train):      # (float32 rows in half the cases, balanced over every axis)
                            cases.append(Case(lane_num, cap, source, train, persistent, (ci + si + train + persistent) % 2 == 1, False))
    # the exact float32 actor (PVE_CFG_ACTOR_F32), one case per kernel family
    cases.append(Case(12, 128, "actor", False, False, True, True))
    cases.append(Case(4, 128, "actor", False, True, False, True))
    return cases


# last_launch() on the GPU by (12-lane family?, source, training outputs, persistent form asked for); the exact float32 actor
# runs as "tick" everywhere.  (The 4- / 8-lane closed loop with the training outputs has no queue kernel: chunked launches.)
GPU_TABLE = {
    (True, "zero", False, False): "resident", (True, "zero", False, True): "persistent",
    (True, "zero", True, False): "resident", (True, "zero", True, True): "persistent",
    (True, "pool", False, False): "resident", (True, "pool", False, True): "persistent",
    (True, "pool", True, False): "resident", (True, "pool", True, True): "persistent",
    (True, "table", False, False): "resident", (True, "table", False, True): "persistent",
    (True, "table", True, False): "resident", (True, "table", True, True): "persistent",
    (True, "actor", False, False): "resident", (True, "actor", False, True): "persistent",
    (True, "actor", True, False): "resident", (True, "actor", True, True): "persistent",
    (False, "zero", False, False): "resident", (False, "zero", False, True): "persistent",
    (False, "zero", True, False): "resident", (False, "zero", True, True): "persistent",
    (False, "pool", False, False): "resident", (False, "pool", False, True): "persistent",
    (False, "pool", True, False): "resident", (False, "pool", True, True): "persistent",
    (False, "table", False, False): "resident", (False, "table", False, True): "persistent",
    (False, "actor", False, False): "resident", (False, "actor", False, True): "persistent",
    (False, "actor", True, False): "resident", (False, "actor", True, True): "resident",
}


def expected_gpu(c):
    return "tick" if c.actor_f32 else GPU_TABLE[(c.lane_num == 12, c.source, c.train, c.persistent)]


# last_variant() on the GPU, as literals (never computed from the picker's rules), by the key of GPU_TABLE:
# (waves_per_simd at 128 slots, waves_per_simd at every other capacity, actor, train, table).  5 = the HOME build of the queue
# kernel: exactly 12 lanes, 128 slots, queue form, zero / pool / table, no training outputs.  4 = the register build.
# The 4- / 8-lane closed loop with the training outputs through the queue runs as chunked launches of the resident kernel.
GPU_VARIANTS = {
    (True, "zero", False, False): (4, 4, 0, 0, 0), (True, "zero", False, True): (5, 4, 0, 0, 0),
    (True, "zero", True, False): (4, 4, 0, 1, 0), (True, "zero", True, True): (4, 4, 0, 1, 0),
    (True, "pool", False, False): (4, 4, 0, 0, 0), (True, "pool", False, True): (5, 4, 0, 0, 0),
    (True, "pool", True, False): (4, 4, 0, 1, 0), (True, "pool", True, True): (4, 4, 0, 1, 0),
    (True, "table", False, False): (4, 4, 0, 0, 1), (True, "table", False, True): (5, 4, 0, 0, 1),
    (True, "table", True, False): (4, 4, 0, 1, 1), (True, "table", True, True): (4, 4, 0, 1, 1),
    (True, "actor", False, False): (4, 4, 1, 0, 0), (True, "actor", False, True): (4, 4, 1, 0, 0),
    (True, "actor", True, False): (4, 4, 1, 1, 0), (True, "actor", True, True): (4, 4, 1, 1, 0),
    (False, "zero", False, False): (4, 4, 0, 0, 0), (False, "zero", False, True): (4, 4, 0, 0, 0),
    (False, "zero", True, False): (4, 4, 0, 1, 0), (False, "zero", True, True): (4, 4, 0, 1, 0),
    (False, "pool", False, False): (4, 4, 0, 0, 0), (False, "pool", False, True): (4, 4, 0, 0, 0),
    (False, "pool", True, False): (4, 4, 0, 1, 0), (False, "pool", True, True): (4, 4, 0, 1, 0),
    (False, "table", False, False): (4, 4, 0, 0, 1), (False, "table", False, True): (4, 4, 0, 0, 1),
    (False, "actor", False, False): (4, 4, 1, 0, 0), (False, "actor", False, True): (4, 4, 1, 0, 0),
    (False, "actor", True, False): (4, 4, 1, 1, 0), (False, "actor", True, True): (4, 4, 1, 1, 0),
}
# workgroups of a queue launch = N_ENVS x items per intersection = 5 x pve_debug_item_schedule(11, 4)[11] = 15 (far below what
# the chip holds); launches of a call: 1 for the queue, 1 for the plain resident form (chunk = 0), ceil(11 / 4) = 3 where the
# queue form was asked for and chunked launches ran, 11 per-tick launches (22 with the actor pass in front of each)
QUEUE_GRID, CHUNKED_LAUNCHES = 15, 3


def expected_gpu_variant(c):
    """the whole record of last_variant() for a case on the GPU"""
    kind = expected_gpu(c)
    v = dict(kind=kind, family=c.lane_num, capacity=c.capacity, geo=int(c.lane_num != 12), prof=0, grid=N_ENVS)
    if kind == "tick":           # (the exact float32 actor: an actor launch and a tick launch per tick)
        v.update(waves_per_simd=0, actor=0, train=int(c.train), table=0, persistent=0, launches=2 * N_TICKS)
        return v
    w128, w, actor, train, table = GPU_VARIANTS[(c.lane_num == 12, c.source, c.train, c.persistent)]
    v.update(waves_per_simd=w128 if c.capacity == 128 else w, actor=actor, train=train, table=table,
             persistent=int(kind == "persistent"))
    if kind == "persistent":
        v.update(grid=QUEUE_GRID, launches=1)
    else:
        v.update(launches=CHUNKED_LAUNCHES if c.persistent else 1)
    return v


def expected_emulated_variant(c):
    """what the emulators know of their own table: the kind, the layout, the capacity and the flags -- no waves, no workgroups, and
    the actor source as per-tick launches"""
    kind = expected_emulated(c)
    v = dict(kind=kind, family=c.lane_num, capacity=c.capacity, geo=int(c.lane_num != 12), prof=0, actor=0, train=int(c.train),
             table=int(c.source == "table" and kind != "tick"), persistent=int(kind == "persistent"), waves_per_simd=0, grid=0)
    v["launches"] = {"tick": N_TICKS * (2 if c.source == "actor" else 1), "persistent": 1,
                     "resident": CHUNKED_LAUNCHES if c.persistent else 1}[kind]
    return v


def expected_emulated(c):
    """The emulators run the actor source as per-tick launches; every other row is the GPU's."""
    return "tick" if c.source == "actor" else expected_gpu(c)


_shared = {}


def _inputs(c):
    """arrival stream (+ intentions), action tape, table and actor weights of a case's (layout, capacity, source kind): computed
    once, shared by the cases, never written"""
    key = (c.lane_num, c.capacity, c.source == "actor")
    if key not in _shared:
        seed = 7100 + c.lane_num
        arr = synthetic_arrivals(N_ENVS, rate=RATE[c.lane_num](c.capacity, c.source), horizon_s=N_TICKS * 0.1 + 30, seed=seed,
                                 lane_num=c.lane_num)
        ch = synthetic_intentions(N_ENVS, arr.shape[1], seed=seed, lane_num=c.lane_num) if c.lane_num == 8 else None
        rng = np.random.default_rng(seed)
        pool = torch.as_tensor(rng.uniform(-3, 3, size=(3, N_ENVS, c.capacity)))
        table = torch.as_tensor(rng.uniform(-3, 3, size=(5, 40)))          # (few columns: later ids share the last)
        _shared[key] = (arr, ch, pool, table)
    if "w" not in _shared:
        from oracle.actor_np import flat_weights, load_weights
        _shared["w"] = flat_weights(load_weights())
    return _shared[key] + (_shared["w"],)


def _batches(backend, c):
    arr, ch, pool, table, w = _inputs(c)
    outs = ("obs_post", "reward", "flags", "nbr", "new_slot", "env_out", "lanej") + (("obs_pre", "state_pre") if c.train else ())
    kw = dict(outputs=outs, obs_dtype=torch.float32 if c.obs_f32 else torch.float64)
    if c.lane_num != 12:
        kw.update(lane_num=c.lane_num, intentions=ch)
    if c.actor_f32:
        kw["actor_f32"] = True
    one = make_batch(arr, N_ENVS, c.capacity, backend, **kw)
    many = make_batch(arr, N_ENVS, c.capacity, backend, **kw)
    pool = pool.to(one.device)
    for b in (one, many):
        b.reset()
        if c.source == "actor":
            b.set_actor(w)
        if c.source == "table":
            b.set_action_table(table)
    if c.source == "pool":
        many.set_action_pool(pool)
    return one, many, pool


def _same_tick(c, o1, o2, one, obs2, what):
    """every requested output of one tick: flags and env_out whole, per-slot outputs where a vehicle is, rows where one is controlled"""
    f = _np(o1["flags"])
    assert np.array_equal(f, _np(o2["flags"])), what + ": flags"
    alive, ctl = (f & 1) != 0, (f & 2) != 0
    for k in ("reward", "new_slot", "lanej"):
        assert np.array_equal(_np(o1[k])[alive], _np(o2[k])[alive]), what + ": " + k
    for k in ("nbr",) + (("obs_pre", "state_pre") if c.train else ()):
        assert np.array_equal(_np(o1[k])[ctl], _np(o2[k])[ctl]), what + ": " + k
    assert np.array_equal(_np(o1["env_out"]), _np(o2["env_out"])), what + ": env_out"
    post_ctl = (_np(one.state_field("meta")) & 1) != 0
    assert np.array_equal(_np(one.obs)[post_ctl], _np(obs2)[post_ctl]), what + ": obs_post"
    return int(ctl.sum())


def run_case(backend, c, want, want_variant=None):
    one, many, pool = _batches(backend, c)

    def single():
        if c.source == "actor":
            return one.step_with_actor()
        if c.source == "table":
            return one.step(one.actions_from_table())
        return one.step(pool[one.ticks % pool.shape[0]] if c.source == "pool" else None)

    what = case_id(c)
    chunk = CHUNK if c.persistent else 0
    # (the training outputs need a trajectory roll-out: state_pre reads the rows the previous tick stored)
    res = many.step_many(N_TICKS, source=c.source, trajectory=c.train, chunk=chunk, persistent=c.persistent)
    many.synchronize()
    assert many.last_launch() == want, "%s: launched as %r, expected %r" % (what, many.last_launch(), want)
    if want_variant is not None:
        got = many.last_variant()
        assert got == want_variant, "%s: launched %r, expected %r" % (what, got, want_variant)
        if want_variant["kind"] == "persistent" and backend == "hip":         # (the grid literal against the library's own schedule)
            import ctypes as C
            sched = (C.c_int32 * 12)()
            assert many.lib.pve_debug_item_schedule(N_TICKS, CHUNK, sched) == 0 and N_ENVS * sched[11] == QUEUE_GRID == got["grid"]
    n_ctl = 0
    for k in range(N_TICKS):
        o1 = single()
        if c.train:
            n_ctl += _same_tick(c, o1, {n: res[n][k] for n in res}, one, res["obs_post"][k], "%s, tick %d" % (what, k))
        else:
            n_ctl += int(((_np(o1["flags"]) & 2) != 0).sum())
    one.synchronize()
    _same_tick(c, o1, res if not c.train else {n: res[n][N_TICKS - 1] for n in res}, one, many.obs, what + ", last tick")
    assert many.ticks == one.ticks == N_TICKS
    batches_equal(one, many, what)
    m1, m2 = one.metrics(), many.metrics()
    assert m1 == m2, (what, m1, m2)
    assert n_ctl >= N_TICKS and m1["overflow"] == 0, (what, n_ctl, m1)        # (vehicles were controlled; nothing deferred)
    one.close(); many.close()


def check_refusal(backend, lane_num):
    from pve_mcc_amd._capi import PveError
    c = Case(lane_num, 64, "table", True, False, False, False)
    _one, many, _pool = _batches(backend, c)
    try:
        many.step_many(N_TICKS, source="table", trajectory=True)
    except PveError as e:
        assert "(-1)" in str(e) and "PVE_SRC_TABLE" in str(e), str(e)          # (-1 = PVE_ERR_INVALID)
        return
    raise AssertionError("PVE_SRC_TABLE with the training outputs accepted for lane_num %d" % lane_num)

"""-m gpu: the measuring instruments -- pve_debug_phase_cycles, pve_debug_stop_phase, pve_debug_traffic_probe -- held to what
include/pve_env.h promises of them.

pve_debug_phase_cycles reroutes kernel selection and launches code that exists for it alone (k_rollout<64|128, 4, PROF = true, ..>,
k_tick_geo<CAP, PROF = true, FIX4>): an armed batch must compute what its never-armed twin computes, bit for bit, take the route
the header states (last_launch() / last_variant() against literals), refuse the table source with a message that names the hook,
and its counters must behave as the code says (no measured number is asserted: only signs, monotonicity, the guard rows and two
bounds that follow from the clocks).  pve_debug_stop_phase must leave the state alone behind a truncated launch, whatever the
phase and the capacity; pve_debug_traffic_probe must write n_envs zeros and nothing else."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from pve_mcc_amd._capi import PveError
from pve_mcc_amd.arrivals import synthetic_arrivals, synthetic_intentions
from pve_mcc_amd.batched import ALL_OUTPUTS, DEFAULT_OUTPUTS
from tests import launch_matrix_scenarios as lm
from tests import scenarios
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
BACKEND = "hip"
N_ENVS, GUARD = 5, 3
STATE_FIELDS = ("p", "v", "a", "jerk", "jerk_sum", "vir_dis", "closer_p", "id", "seq", "vnum", "step", "count", "meta", "hdr")
LAYOUTS = [(12, 64), (12, 128), (12, 256), (4, 64), (4, 128), (8, 64), (8, 128)]

_shared = {}


def _inputs(lane_num, cap):
    """arrival stream (+ intentions), action tape and table of a (layout, capacity): computed once, never written"""
    key = (lane_num, cap)
    if key not in _shared:
        seed = 9300 + lane_num
        arr = synthetic_arrivals(N_ENVS, rate=lm.RATE[lane_num](cap, "zero"), horizon_s=90.0, seed=seed, lane_num=lane_num)
        ch = synthetic_intentions(N_ENVS, arr.shape[1], seed=seed, lane_num=lane_num) if lane_num == 8 else None
        rng = np.random.default_rng(seed + cap)
        _shared[key] = (arr, ch, torch.as_tensor(rng.uniform(-3, 3, size=(3, N_ENVS, cap))), torch.as_tensor(rng.uniform(-3, 3, size=(5, 40))))
    return _shared[key]


def _twins(lane_num, cap, outputs, prefill=150, n=2):
    """n batches on the same inputs, `prefill` ticks into the stream (never armed so far)"""
    arr, ch, pool, table = _inputs(lane_num, cap)
    kw = dict(outputs=outputs)
    if lane_num != 12:
        kw.update(lane_num=lane_num, intentions=ch)
    bs = [make_batch(arr, N_ENVS, cap, BACKEND, **kw) for _ in range(n)]
    for b in bs:
        b.reset()
        b.set_action_pool(pool)
        b.set_action_table(table)
        if prefill and "state_pre" in outputs:              # (state_pre needs a trajectory roll-out: single ticks instead)
            for _ in range(prefill):
                b.step(None)
        elif prefill:
            b.step_many(prefill, source="zero", chunk=25, persistent=True)
    return bs + [bs[0]._pool]


def _arm(b):
    """a zeroed counter buffer with GUARD rows of 0xFF.. behind it, armed"""
    rows = N_ENVS * b.capacity // 64
    buf = torch.zeros(rows + GUARD, 16, dtype=torch.int64, device=b.device)
    buf[rows:] = -1
    b.synchronize()
    assert b.lib.pve_debug_phase_cycles(b._h, C.c_void_p(buf.data_ptr())) == 0
    return buf


def _disarm(b):
    b.synchronize()
    assert b.lib.pve_debug_phase_cycles(b._h, None) == 0


def _counters(buf):
    c = _np(buf)
    assert (c[-GUARD:] == -1).all(), "guard rows written"
    return c[:-GUARD]


def _same_outputs(o1, o2, b1, what):
    """every output of one call: flags and env_out whole, per-slot outputs where a vehicle is, rows where one is controlled"""
    f = _np(o1["flags"])
    assert np.array_equal(f, _np(o2["flags"])), what + ": flags"
    alive, ctl = (f & 1) != 0, (f & 2) != 0
    post_ctl = (_np(b1.state_field("meta")) & 1) != 0
    assert set(o1) == set(o2)
    for k in o1:
        mask = {"flags": None, "env_out": None, "reward": alive, "new_slot": alive, "lanej": alive, "obs_post": post_ctl}.get(k, ctl)
        x, y = _np(o1[k]), _np(o2[k])
        assert np.array_equal(x, y) if mask is None else np.array_equal(x[mask], y[mask]), "%s: %s" % (what, k)
    return int(ctl.sum())


def _equal(armed, twin, what):
    scenarios.batches_equal(twin, armed, what)
    assert armed.metrics() == twin.metrics(), what


def _snapshot(b):
    b.synchronize()
    env = []
    for e in range(b.n_envs):
        i = b.read_env(e)
        env.append([list(getattr(i, f)) if hasattr(getattr(i, f), "__len__") else getattr(i, f) for f, _ in i._fields_])
    return {k: _np(b.state_field(k)).copy() for k in STATE_FIELDS}, env, b.metrics()


def _same_snapshot(s1, s2, what):
    for k in STATE_FIELDS:                                  # (whole [n_envs, capacity] arrays, the slots without a vehicle included)
        assert np.array_equal(s1[0][k], s2[0][k], equal_nan=True), "%s: state field %s written" % (what, k)
    assert s1[1] == s2[1], "%s: header written" % what
    assert s1[2] == s2[2], "%s: metrics moved" % what


def _tick_variant(lane_num, cap, prof, train, launches=1):
    return dict(kind="tick", family=lane_num, capacity=cap, waves_per_simd=0, prof=prof, actor=0, train=train, table=0, persistent=0,
                geo=int(lane_num != 12), grid=N_ENVS, launches=launches)


# ------------------------------------------------------------------ pve_debug_phase_cycles: one launch per tick
@pytest.mark.parametrize("lane_num,cap", LAYOUTS, ids=["l%d-c%d" % lc for lc in LAYOUTS])
def test_gpu_armed_step_equals_twin_and_counts(lane_num, cap):
    """step() with every output (state_pre included), K = 12 launches, twice; then disarmed"""
    K = 12
    armed, twin, pool = _twins(lane_num, cap, ALL_OUTPUTS)
    buf = _arm(armed)
    t0 = time.perf_counter()                                # (_arm synchronised: nothing armed runs before t0)
    n_ctl = 0
    for k in range(K):
        o1, o2 = twin.step(pool[k % 3]), armed.step(pool[k % 3])
        n_ctl += _same_outputs(o1, o2, twin, "l%d c%d tick %d" % (lane_num, cap, k))
        _equal(armed, twin, "l%d c%d tick %d" % (lane_num, cap, k))
        assert armed.last_launch() == "tick" and armed.last_variant() == _tick_variant(lane_num, cap, 1, 1)
        assert twin.last_variant() == _tick_variant(lane_num, cap, 0, 1)
    armed.synchronize()
    host_s = time.perf_counter() - t0
    assert n_ctl > 0
    c1 = _counters(buf)
    assert (c1[:, 12:] == 0).all(), "a per-tick launch writes columns 0 .. 11 only"
    assert (c1[:, :12] >= 0).all() and (c1[:, :12].sum(1) > 0).all(), "every wave row counts"
    # wall_clock64 is the 100 MHz constant clock: no wave can have spent more ticks in its K launches than the host saw pass
    assert c1[:, :12].sum(1).max() <= 1e8 * host_s, (c1[:, :12].sum(1).max(), host_s)
    if lane_num == 12:
        assert c1[:, 10].sum() > 0, "state_pre was requested: column 10 counts its pass"
    for k in range(K, 2 * K):                                # the counters accumulate
        twin.step(pool[k % 3]); armed.step(pool[k % 3])
    c2 = _counters(buf)
    assert (c2 >= c1).all() and (c2[:, :12].sum(1) > c1[:, :12].sum(1)).all() and (c2[:, 12:] == 0).all()
    _disarm(armed)
    for k in range(2 * K, 2 * K + 3):
        o1, o2 = twin.step(pool[k % 3]), armed.step(pool[k % 3])
        assert armed.last_variant() == _tick_variant(lane_num, cap, 0, 1)
    armed.synchronize()
    assert np.array_equal(_np(buf)[:-GUARD], c2), "disarmed ticks wrote the counters"
    _same_outputs(o1, o2, twin, "disarmed")
    _equal(armed, twin, "l%d c%d after disarming" % (lane_num, cap))
    armed.close(); twin.close()


@pytest.mark.parametrize("cap", [64, 128, 256])
def test_gpu_armed_step_without_state_pre_leaves_column_10(cap):
    armed, twin, pool = _twins(12, cap, DEFAULT_OUTPUTS)
    buf = _arm(armed)
    for k in range(12):
        o1, o2 = twin.step(pool[k % 3]), armed.step(pool[k % 3])
        _same_outputs(o1, o2, twin, "c%d tick %d" % (cap, k))
    assert armed.last_variant() == _tick_variant(12, cap, 1, 0)
    _equal(armed, twin, "c%d" % cap)
    c = _counters(buf)
    assert (c[:, 10] == 0).all() and (c[:, 12:] == 0).all() and (c[:, :12].sum(1) > 0).all()
    armed.close(); twin.close()


# ------------------------------------------------------------------ pve_debug_phase_cycles: pve_step_many
@pytest.mark.parametrize("persistent", [False, True], ids=["plain", "queue-asked"])
@pytest.mark.parametrize("source", ["zero", "pool"])
@pytest.mark.parametrize("cap", [64, 128])
def test_gpu_armed_step_many_runs_the_diagnostics_build_of_the_resident_kernel(cap, source, persistent):
    """zero / pool, no training outputs, 64 / 128 slots: k_rollout<CAP, 4, PROF = true, ..> -- one launch, or chunked launches where
    the queue form was asked for (it has no diagnostics build); the twin takes the queue"""
    n, chunk = 21, (6 if persistent else 0)
    armed, twin, _pool = _twins(12, cap, DEFAULT_OUTPUTS + ("lanej",))
    buf = _arm(armed)
    for call in range(2):
        o1 = twin.step_many(n, source=source, chunk=chunk, persistent=persistent)
        o2 = armed.step_many(n, source=source, chunk=chunk, persistent=persistent)
        armed.synchronize(); twin.synchronize()
        assert armed.last_launch() == "resident"
        assert armed.last_variant() == dict(kind="resident", family=12, capacity=cap, waves_per_simd=4, prof=1, actor=0, train=0, table=0,
                                            persistent=0, geo=0, grid=N_ENVS, launches=4 if persistent else 1)
        vt = twin.last_variant()
        assert (vt["kind"], vt["prof"], vt["waves_per_simd"]) == (("persistent", 0, 5 if cap == 128 else 4) if persistent else ("resident", 0, 4))
        _same_outputs(o1, o2, twin, "c%d %s call %d" % (cap, source, call))
        _equal(armed, twin, "c%d %s call %d" % (cap, source, call))
        c = _counters(buf)
        assert (c[:, 14:] == 0).all() and (c[:, :14] >= 0).all()
        assert (c[:, 13] > 0).all() and (c[:, 12] > 0).all(), "both clocks of the launch"
        assert (c[:, :12].sum(1) <= c[:, 13]).all(), "the phases lie inside the launch"
        assert (c[:, 12] <= 30 * c[:, 13]).all(), "a shader clock above 3 GHz"
        if call:
            assert (c >= c_first).all() and (c[:, 13] > c_first[:, 13]).all()
        c_first = c
    armed.close(); twin.close()


FALLBACKS = [  # (layout, capacity, source, training outputs, queue form asked): every one runs as one launch per tick while armed
    (12, 256, "zero", False, False), (12, 256, "pool", False, True), (12, 64, "pool", True, False), (12, 128, "zero", True, True),
    (12, 128, "actor", False, False), (12, 64, "actor", False, True), (4, 64, "zero", False, False), (4, 128, "pool", False, True),
    (8, 64, "pool", False, False), (8, 128, "zero", True, True), (8, 128, "actor", False, False)]


@pytest.mark.parametrize("lane_num,cap,source,train,persistent", FALLBACKS,
                         ids=["l%d-c%d-%s-%s-%s" % (f[0], f[1], f[2], "train" if f[3] else "plain", "queue" if f[4] else "resident") for f in FALLBACKS])
def test_gpu_armed_step_many_falls_back_to_armed_ticks(lane_num, cap, source, train, persistent):
    n, chunk = 13, (5 if persistent else 0)
    armed, twin, _pool = _twins(lane_num, cap, DEFAULT_OUTPUTS + (("obs_pre",) if train else ()))
    if source == "actor":
        from oracle.actor_np import flat_weights, load_weights
        w = flat_weights(load_weights())
        armed.set_actor(w); twin.set_actor(w)
    buf = _arm(armed)
    o1 = twin.step_many(n, source=source, chunk=chunk, persistent=persistent)
    o2 = armed.step_many(n, source=source, chunk=chunk, persistent=persistent)
    armed.synchronize(); twin.synchronize()
    assert armed.last_launch() == "tick"
    assert armed.last_variant() == _tick_variant(lane_num, cap, 1, int(train), launches=n * (2 if source == "actor" else 1))
    vt = twin.last_variant()
    assert vt["kind"] in ("resident", "persistent") and vt["prof"] == 0, vt
    what = "l%d c%d %s" % (lane_num, cap, source)
    assert _same_outputs(o1, o2, twin, what) > 0
    _equal(armed, twin, what)
    c = _counters(buf)
    assert (c[:, 12:] == 0).all() and (c[:, 10] == 0).all() and (c[:, :12].sum(1) > 0).all()
    armed.close(); twin.close()


@pytest.mark.parametrize("lane_num", [12, 4, 8])
@pytest.mark.parametrize("persistent", [False, True], ids=["plain", "queue"])
def test_gpu_armed_table_source_is_refused_and_runs_after_disarming(lane_num, persistent):
    armed, twin, _pool = _twins(lane_num, 128, DEFAULT_OUTPUTS)
    buf = _arm(armed)
    before, ticks = _snapshot(armed), armed.ticks
    with pytest.raises(PveError) as e:
        armed.step_many(11, source="table", chunk=4 if persistent else 0, persistent=persistent)
    assert "(-3)" in str(e.value) and "pve_debug_phase_cycles" in str(e.value) and "PVE_SRC_TABLE" in str(e.value), str(e.value)
    assert armed.last_launch() == "none" and armed.last_variant()["launches"] == 0 and armed.ticks == ticks
    _same_snapshot(before, _snapshot(armed), "refused call")
    assert (_counters(buf) == 0).all()
    _disarm(armed)
    o2 = armed.step_many(11, source="table", chunk=4 if persistent else 0, persistent=persistent)
    o1 = twin.step_many(11, source="table", chunk=4 if persistent else 0, persistent=persistent)
    v = armed.last_variant()
    assert (v["kind"], v["table"], v["prof"]) == ("persistent" if persistent else "resident", 1, 0) and v == twin.last_variant()
    _same_outputs(o1, o2, twin, "l%d table after disarming" % lane_num)
    _equal(armed, twin, "l%d table after disarming" % lane_num)
    armed.close(); twin.close()


# ------------------------------------------------------------------ pve_debug_stop_phase
@pytest.mark.parametrize("cap", [64, 128, 256])
def test_gpu_truncated_tick_writes_no_state(cap):
    """one truncated step() behind every phase n = 0 .. 8 on a steady-state batch (a full tick between them moves the state on):
    the fourteen state fields, every header and the metrics are bit-identical behind it"""
    b, pool = _twins(12, cap, DEFAULT_OUTPUTS, prefill=250, n=1)
    assert b.metrics()["alive_steps"] > 0
    for n in range(9):
        before = _snapshot(b)
        assert (before[0]["meta"] & 1).sum() >= N_ENVS, "vehicles are controlled"
        assert b.lib.pve_debug_stop_phase(b._h, n) == 0
        b.step(pool[n % 3])
        _same_snapshot(before, _snapshot(b), "capacity %d, stop behind phase %d" % (cap, n))
        assert b.last_variant() == _tick_variant(12, cap, 0, 0)
        assert b.lib.pve_debug_stop_phase(b._h, -1) == 0
        b.step(pool[(n + 1) % 3])
        after = _snapshot(b)
        assert after[2]["ticks"] == before[2]["ticks"] + N_ENVS and after[1] != before[1], "the full tick is a tick again"
    b.close()


@pytest.mark.parametrize("cap", [64, 128, 256])
def test_gpu_alternating_full_and_truncated_ticks_equal_the_full_ticks(cap):
    """the pattern of tools/phase_probe.py: full tick, truncated tick, full tick, .. against a twin that ran the full ticks only"""
    probe, twin, pool = _twins(12, cap, DEFAULT_OUTPUTS, prefill=250)
    for k in range(8):
        probe.lib.pve_debug_stop_phase(probe._h, -1)
        o2, o1 = probe.step(pool[k % 3]), twin.step(pool[k % 3])
        _same_outputs(o1, o2, twin, "round %d" % k)
        probe.lib.pve_debug_stop_phase(probe._h, k)          # (behind phases 0 .. 7 in turn)
        probe.step(pool[(k + 1) % 3])
    probe.lib.pve_debug_stop_phase(probe._h, -1)
    _same_snapshot(_snapshot(twin), _snapshot(probe), "capacity %d after 8 rounds" % cap)
    o2, o1 = probe.step(pool[0]), twin.step(pool[0])
    _same_outputs(o1, o2, twin, "the tick behind the rounds")
    _equal(probe, twin, "capacity %d, the tick behind the rounds" % cap)
    probe.close(); twin.close()


# ------------------------------------------------------------------ pve_debug_traffic_probe
@pytest.mark.parametrize("cap", [64, 128, 256])
def test_gpu_traffic_probe_writes_one_zero_per_intersection(cap):
    b, _pool = _twins(12, cap, DEFAULT_OUTPUTS, prefill=100, n=1)
    before = _snapshot(b)
    sink = torch.full((N_ENVS + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=b.device)
    b.synchronize()
    assert b.lib.pve_debug_traffic_probe(b._h, C.c_void_p(sink.data_ptr())) == 0
    b.synchronize()
    s = _np(sink)
    assert (s[:N_ENVS] == 0).all(), "no slot's state sums to 12345.678"
    assert (s[N_ENVS:] == 0x5A5A5A5A).all(), "the probe wrote past n_envs"
    _same_snapshot(before, _snapshot(b), "traffic probe")
    assert b.last_variant()["kind"] == "persistent", "the probe is no stepping call: the record is the prefill's"
    b.close()

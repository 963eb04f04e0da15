"""The n-step transition pass, CPU side: the fixture recorded from the unmodified reference with main.py:243-266's own buffers
(tests/golden/gen_nstep_golden.py -> tests/golden/nstep_ref.npz), the NumPy restatement pve_mcc_amd/nstep.py, csrc/pve_nstep.h
through a g++ host shim (tests/nstep_host), hand-made trajectories (tests/nstep_scenarios.py), one roll-out of the CPU emulator,
and the two C ABI entry points on the emulator (which has no n-step kernels and must say so).  The kernels are checked in
tests/test_gpu_nstep.py.  Everything here is exact: targets are compared as float64 bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

from pve_mcc_amd import PveError, _capi, nstep
from tests import native
from tests import nstep_scenarios as S
from tests.hip_adapter import _np, emulator_lib, make_batch
from tests.parity_util import GOLDEN_DIR

GAMMA0 = float(np.tanh(6.0 / 12.0) * 0.9)            # main.py:227 at epoch 0


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _signatures(L):
    L.nstep_scan_host.restype = C.c_longlong
    L.nstep_scan_host.argtypes = [C.c_double] + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 8
    return L


def shim():
    """csrc/pve_nstep.h compiled by g++ (tests/nstep_host), built and loaded by tests/native.py."""
    return native.load("nstep_host", "libnstep_host.so", _signatures)


def shim_scan(cur, gamma, window=13, prev=None, obs_first=None, q=None, tail=False):
    keep = []

    def P(x, dt):
        if x is None:
            return None
        a = np.ascontiguousarray(x, dt)
        keep.append(a)
        return a.ctypes.data
    n_cur, E, K = cur["flags"].shape
    n_prev = 0 if prev is None else prev["flags"].shape[0]
    odt = cur["obs_post"].dtype
    n_back = min(n_prev, window - 1)
    target = np.full((n_back + n_cur, E, K), np.nan)
    code = np.full((n_back + n_cur, E, K), -1, np.int32)
    p = prev or {}
    total = shim().nstep_scan_host(float(gamma), window, nstep.TAIL if tail else 0, E, K, int(odt == np.float32),
                                   n_prev, P(p.get("obs_post"), odt), P(p.get("reward"), np.float64), P(p.get("flags"), np.int32),
                                   P(p.get("new_slot"), np.int32),
                                   n_cur, P(cur["obs_post"], odt), P(cur["reward"], np.float64), P(cur["flags"], np.int32),
                                   P(cur["new_slot"], np.int32), P(obs_first, odt), P(q, np.float32), target.ctypes.data, code.ctypes.data)
    assert total == np.count_nonzero(code)
    return target, code, n_back


def run_pass(tr, gamma, window, a=0, b=None, prev_from=None, tail=False):
    """nstep.py over ticks a .. b - 1 of a hand-made trajectory (prev = ticks prev_from .. a - 1) -> dict keyed by the ABSOLUTE
    start tick, and the records"""
    b = tr.T if b is None else b
    prev = None if prev_from is None else S.blocks(tr, prev_from, a)
    rec, idx, total = nstep.nstep_transitions(S.blocks(tr, a, b), gamma, window, prev=prev, obs_first=S.obs_before(tr, a), q=tr.q[a:b], tail=tail)
    assert total == len(rec) == len(idx)
    tgt, code, n_back = nstep.scan(S.blocks(tr, a, b), gamma, window, prev=prev, obs_first=S.obs_before(tr, a), q=tr.q[a:b], tail=tail)
    c, e, s = nstep.order(code)
    return S.as_dict(idx, lambda i: tgt[c[i], e[i], s[i]], tick0=a), rec, idx


def same(got, want):
    assert set(got) == set(want), (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    for k in want:
        assert got[k][1:] == want[k][1:], (k, got[k], want[k])
        assert bits(got[k][0]) == bits(want[k][0]), (k, got[k], want[k])


# ------------------------------------------------------------------ 1. the fixture recorded from the reference
def test_fixture_vs_numpy_restatement():
    z, cur = S.load_reference_fixture()
    T, K, window = int(z["T"]), int(z["K"]), int(z["window"])
    assert window == 13 and T > 2 * window and z["q"].dtype == np.float32 and z["q"].shape == (T, 1, K)
    gammas = z["gammas"]
    assert bits(gammas[0]) == bits(GAMMA0) and gammas[1] == 0.8
    ids = z["ids"]                                   # vehicle id of every (tick, slot), -1 = empty
    n_done = n_boot = 0
    for gi, gamma in enumerate(gammas):
        rec, idx, total = nstep.nstep_transitions(cur, gamma, window, obs_first=z["obs_first"], q=z["q"])
        tgt, code, n_back = nstep.scan(cur, gamma, window, obs_first=z["obs_first"], q=z["q"])
        assert n_back == 0 and total == len(z["em_tick"]) > 0
        # multiset of (emitting tick, vehicle id) -> row, actions, target
        got = {}
        for i, (t, e, s, c) in enumerate(idx.tolist()):
            key = (t + (c & 0xFF) - 1, int(ids[t, 0, s]))
            assert key not in got
            row = (z["obs_first"][0, s] if t == 0 else cur["obs_post"][t - 1, 0, s])
            got[key] = (row, cur["state_pre"][t, 0, s, :, 2], tgt[t, 0, s], c)
            assert np.array_equal(rec[i, :28], row.astype(np.float32)) and np.array_equal(rec[i, 28:35], got[key][1].astype(np.float32))
            assert rec[i, 35] == np.float32(tgt[t, 0, s])
        want = {(int(t), int(v)): i for i, (t, v) in enumerate(zip(z["em_tick"], z["em_id"]))}
        assert set(got) == set(want)
        for key, i in want.items():
            row, act, target, c = got[key]
            assert np.array_equal(bits(row), bits(z["em_row"][i])), key
            assert np.array_equal(bits(act), bits(z["em_act"][i])), key
            assert bits(target) == bits(z["em_target"][gi, i]), (key, target, z["em_target"][gi, i])
            n_done += bool(c & nstep.DONE)
            n_boot += bool(c & nstep.BOOT)
    assert n_done > 0 and n_boot > 0                       # windows closed by Done and bootstrapped windows both occur in the run


# ------------------------------------------------------------------ 2. hand-made trajectories: every case present
@pytest.mark.parametrize("window", [13, 1, 16, 5])
def test_hand_made_cases(window):
    tr = S.make_trajectory(40)
    gamma = GAMMA0
    got, rec, idx = run_pass(tr, gamma, window)
    want = S.expected(tr, gamma, window)
    same(got, want)
    got_tail, _, _ = run_pass(tr, gamma, window, tail=True)
    same(got_tail, S.expected(tr, gamma, window, tail=True))
    codes = idx[:, 3]
    n, boot, done = codes & 0xFF, (codes & nstep.BOOT) != 0, (codes & nstep.DONE) != 0
    close = idx[:, 0] + n - 1
    assert np.count_nonzero(boot & (n == window)) > 0                      # a full window that is bootstrapped
    assert np.count_nonzero(done & (n == window)) > 0                      # Done at entry `window`: no bootstrap
    assert not np.any(boot & done) and np.all(boot | done)
    assert np.count_nonzero(done & (n == 1)) > 0                           # Done at entry 1
    assert np.count_nonzero(close == 0) > 0 and np.count_nonzero(close == tr.T - 1) > 0    # closing on the first / last tick
    if window > 1:
        short = done & (n < window)
        assert np.count_nonzero(short) > 0                                 # a fresh vehicle that dies before the window fills
        assert len(got_tail) > len(got) and set(got) < set(got_tail)       # its younger starts: dropped by default, emitted with tail
        younger = set(got_tail) - set(got)
        assert all(got_tail[k][3] and got_tail[k][1] < window for k in younger)
    # the ingredients: permuted slots, uncontrolled slots, -1 links without Done
    alive = tr.flags != 0
    moved = alive & (tr.new_slot >= 0) & (tr.new_slot != np.arange(tr.K)[None, None, :])
    assert moved.sum() > 0.9 * (alive & (tr.new_slot >= 0)).sum()
    assert np.count_nonzero(alive & ((tr.flags & S.F_CTL) == 0)) > 0
    assert np.count_nonzero(((tr.flags & (S.F_CTL | S.F_DONE)) == S.F_CTL) & (tr.new_slot < 0)) > 0
    # a start behind an uncontrolled slot or a broken link emits nothing
    tgt, code, _ = nstep.scan(S.blocks(tr), gamma, window, obs_first=tr.obs_first, q=tr.q, tail=True)
    assert not code[(tr.flags & S.F_CTL) == 0].any()
    if window > 1:
        broken = ((tr.flags & (S.F_CTL | S.F_DONE)) == S.F_CTL) & (tr.new_slot < 0)
        assert not code[broken].any()


def test_records_layout():
    tr = S.make_trajectory(14, f32=True)
    got, rec, idx = run_pass(tr, 0.8, 13)
    assert rec.dtype == np.float32 and rec.shape[1] == 36 and idx.dtype == np.int32 and len(rec) > 0
    order = idx[:, 0].astype(np.int64) * tr.E * tr.K + idx[:, 1] * tr.K + idx[:, 2]
    assert np.all(np.diff(order) > 0)                                      # (tick, env, slot) ascending
    for i, (t, e, s, c) in enumerate(idx.tolist()):
        assert np.array_equal(rec[i, :28], S.obs_before(tr, t)[e, s]) and np.array_equal(rec[i, 28:35], tr.state_pre[t, e, s, :, 2])
        assert rec[i, 35] == np.float32(got[(t, e, s)][0])


# ------------------------------------------------------------------ 3. windows that cross calls
def test_chained_calls():
    tr = S.make_trajectory(40, seed=2)
    gamma, window = GAMMA0, 13
    whole, _, _ = run_pass(tr, gamma, window)
    a, _, _ = run_pass(tr, gamma, window, 0, 14)
    b, _, _ = run_pass(tr, gamma, window, 14, 27, prev_from=0)
    c, _, _ = run_pass(tr, gamma, window, 27, 40, prev_from=14)
    assert a and b and c
    assert not (set(a) & set(b)) and not (set(b) & set(c)) and not (set(a) & set(c))      # a pending start emits exactly once
    union = dict(a)
    union.update(b)
    union.update(c)
    same(union, whole)
    # pending starts of the first call: they are in the second call's records, with negative ticks there
    pending = [k for k in b if k[0] < 14]
    assert pending and all(k not in a for k in pending)
    same(b, S.expected(tr, gamma, window, lo=14, hi=27))
    # without prev the windows open before the call are lost, nothing else
    lost, _, _ = run_pass(tr, gamma, window, 14, 27)
    assert set(lost) < set(b) and all(k[0] >= 14 for k in lost)
    assert {k for k in b if k[0] >= 14 and b[k][1] == window} <= set(lost)
    with pytest.raises(ValueError):
        run_pass(tr, gamma, window, 14, 27, prev_from=4)                   # 0 < n_prev < window
    # only the last `window` ticks of prev are read
    long_prev, _, _ = run_pass(tr, gamma, window, 27, 40, prev_from=0)
    same(long_prev, c)


# ------------------------------------------------------------------ 4. the header's own routine, compiled by g++
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("window,tail", [(13, False), (13, True), (1, False), (16, True), (4, False)])
def test_host_build_is_bit_equal(window, tail, f32):
    tr = S.make_trajectory(40, seed=3, f32=f32)
    n = 0
    for a, b, p in ((0, 40, None), (16, 30, 0), (20, 21, 3), (20, 40, None)):
        kw = dict(prev=None if p is None else S.blocks(tr, p, a), obs_first=S.obs_before(tr, a), q=tr.q[a:b], tail=tail)
        t0, c0, nb0 = nstep.scan(S.blocks(tr, a, b), GAMMA0, window, **kw)
        t1, c1, nb1 = shim_scan(S.blocks(tr, a, b), GAMMA0, window, **kw)
        assert nb0 == nb1 and np.array_equal(c0, c1) and np.array_equal(bits(t0), bits(t1))
        n += np.count_nonzero(c0)
    assert n > 0


def test_fold_is_not_contracted():
    """one bootstrapped window whose fused and separately rounded folds differ"""
    rng = np.random.RandomState(11)
    K, window = 64, 13
    cur = dict(obs_post=np.ones((window, 1, K, 28)), state_pre=np.zeros((window, 1, K, 7, 28)), reward=rng.uniform(-2, 5, (window, 1, K)),
               flags=np.full((window, 1, K), 3, np.int32), new_slot=np.tile(np.arange(K, dtype=np.int32), (window, 1, 1)))
    q = rng.uniform(-20, 20, (window, 1, K)).astype(np.float32)
    tgt, code, _ = nstep.scan(cur, GAMMA0, window, obs_first=np.ones((1, K, 28)), q=q)
    assert np.all(code[0] == (window | nstep.BOOT)) and not code[1:].any()
    from fractions import Fraction
    fused = []
    for s in range(K):                                                     # every step rounded ONCE (what an FMA would give)
        r = float(Fraction(float(cur["reward"][-1, 0, s])) + Fraction(GAMMA0) * Fraction(float(q[-1, 0, s])))
        for k in range(window - 2, -1, -1):
            r = float(Fraction(float(cur["reward"][k, 0, s])) + Fraction(GAMMA0) * Fraction(r))
        fused.append(r)
    assert np.count_nonzero(bits(np.array(fused)) != bits(tgt[0, 0])) > 0
    t1, c1, _ = shim_scan(cur, GAMMA0, window, obs_first=np.ones((1, K, 28)), q=q)
    assert np.array_equal(bits(t1), bits(tgt))


# ------------------------------------------------------------------ 5. one roll-out of the CPU emulator
def test_emulator_rollout():
    from pve_mcc_amd.arrivals import synthetic_arrivals
    arr = synthetic_arrivals(2, rate=1100.0, horizon_s=60.0, seed=9)
    b = make_batch(arr, 2, 64, "emu", outputs=("obs_post", "obs_pre", "state_pre", "reward", "flags", "new_slot", "env_out"))
    b.reset()
    first = _np(b.obs).copy()
    traj = b.step_many(30, source="zero", trajectory=True)
    cur = {k: _np(traj[k]).copy() for k in nstep.KEYS}
    q = np.random.RandomState(5).uniform(-10, 10, cur["flags"].shape).astype(np.float32)
    assert not first.any()
    t0, c0, _ = nstep.scan(cur, GAMMA0, 13, obs_first=first, q=q)
    t1, c1, _ = shim_scan(cur, GAMMA0, 13, obs_first=first, q=q)
    assert np.array_equal(c0, c1) and np.array_equal(bits(t0), bits(t1))
    ctl = (cur["flags"] & S.F_CTL) != 0
    assert np.count_nonzero(c0) > 0 and ctl[:18].sum() > 0
    # steady state: every controlled vehicle and tick whose window fits starts one transition, nothing else does
    fits = np.zeros_like(ctl)
    fits[:18] = ctl[:18]
    full = (c0 & 0xFF) == 13
    assert np.array_equal(full & ~((c0 & nstep.DONE) != 0), (c0 & nstep.BOOT) != 0)
    alive_to_end = fits & (c0 != 0)
    assert alive_to_end.sum() >= 0.9 * fits.sum() and not c0[~ctl].any()
    rec, idx = nstep.records(cur, t0, c0, 0, obs_first=first)
    # a vehicle's s0 row carries what the previous tick stored for it: first controlled tick = all zero
    fresh = ~rec[:, :28].any(axis=1)
    assert fresh.any() and not fresh.all()
    # the Python layer asks the backend, which has no kernels
    with pytest.raises(PveError, match="backend"):
        b.nstep_transitions(GAMMA0, q=torch.as_tensor(q))


# ------------------------------------------------------------------ 6. the C ABI on a backend without the kernels
def test_entry_points_on_the_emulator():
    from pve_mcc_amd.arrivals import synthetic_arrivals
    from pve_mcc_amd.batched import BatchedIntersections, PipelinedIntersections
    lib = emulator_lib()
    for name in ("pve_nstep_scan", "pve_nstep_gather"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert lib.pve_abi_version() == _capi.ABI_VERSION
    for cls in (BatchedIntersections, PipelinedIntersections):
        assert callable(getattr(cls, "nstep_transitions"))
    b = make_batch(synthetic_arrivals(2, rate=500.0, horizon_s=20.0, seed=1), 2, 64, "emu", outputs=("obs_post", "reward", "flags", "env_out"))
    tr = S.make_trajectory(14, E=2)
    keep = []

    def P(x, dt):
        a = np.ascontiguousarray(x, dt)
        if a.ctypes.data % 16:                       # (the ABI wants 16-byte aligned rows)
            raw = np.zeros(a.nbytes + 16, np.uint8)
            o = (-raw.ctypes.data) % 16
            raw[o:o + a.nbytes] = a.view(np.uint8).ravel()
            keep.append(raw)
            return raw.ctypes.data + o
        keep.append(a)
        return a.ctypes.data

    def make(**kw):
        ns = _capi.PveNstep()
        ns.gamma, ns.window, ns.mode = 0.8, 13, 0
        for seg in (ns.cur, ns.prev):
            seg.n_ticks = 14
            seg.obs_post, seg.state_pre = P(tr.obs_post, np.float64), P(tr.state_pre, np.float64)
            seg.reward, seg.flags, seg.new_slot = P(tr.reward, np.float64), P(tr.flags, np.int32), P(tr.new_slot, np.int32)
        ns.prev.n_ticks = 0
        ns.obs_first, ns.q_boot = P(tr.obs_first, np.float64), P(tr.q, np.float32)
        ns.target, ns.code = P(np.zeros((14, 2, 64)), np.float64), P(np.zeros((14, 2, 64)), np.int32)
        ns.offsets, ns.total = P(np.zeros(29), np.int32), P(np.zeros(1), np.int64)
        ns.max_records, ns.records, ns.index = 10, P(np.zeros((10, 36)), np.float32), P(np.zeros((10, 4)), np.int32)
        for k, v in kw.items():
            obj, _, f = k.rpartition("__")
            setattr(getattr(ns, obj) if obj else ns, f, v)
        return ns
    bad = [(dict(window=0), b"window"), (dict(window=17), b"window"), (dict(gamma=float("nan")), b"gamma"), (dict(gamma=1.5), b"gamma"),
           (dict(gamma=-0.1), b"gamma"), (dict(prev__n_ticks=5), b"prev.n_ticks"), (dict(prev__n_ticks=-1), b"prev.n_ticks"),
           (dict(cur__n_ticks=0), b"cur.n_ticks"), (dict(cur__flags=None), b"segment"), (dict(cur__state_pre=None), b"segment"),
           (dict(prev__n_ticks=13, prev__new_slot=None), b"segment"), (dict(obs_first=None), b"obs_first"), (dict(q_boot=None), b"q_boot"),
           (dict(target=None), b"q_boot"), (dict(total=None), b"q_boot"), (dict(block_threads=100), b"block_threads"),
           (dict(obs_first=P(tr.obs_first, np.float64) + 8), b"aligned")]
    for kw, word in bad:
        for fn in (lib.pve_nstep_scan, lib.pve_nstep_gather):
            rc = fn(b._h, C.byref(make(**kw)))
            assert rc == -1 and word in lib.pve_last_error(), (kw, rc, lib.pve_last_error())
    for kw, word in ((dict(max_records=-1), b"max_records"), (dict(records=None), b"max_records"), (dict(index=None), b"max_records")):
        assert lib.pve_nstep_gather(b._h, C.byref(make(**kw))) == -1 and word in lib.pve_last_error()
    assert lib.pve_nstep_scan(None, C.byref(make())) == -1 and b"null" in lib.pve_last_error()
    assert lib.pve_nstep_scan(b._h, None) == -1 and b"null" in lib.pve_last_error()
    # valid arguments: the emulator has no n-step kernels and says so
    for fn in (lib.pve_nstep_scan, lib.pve_nstep_gather):
        assert fn(b._h, C.byref(make())) == -1 and b"backend has no n-step kernels" in lib.pve_last_error()
    # the Python layer's own checks
    with pytest.raises(PveError, match="trajectory"):
        b.nstep_transitions(0.8)

"""The MADDPG critic and the bootstrap Q, CPU side: the fixture decoded from the reference's own graph
(tests/golden/gen_critic_golden.py -> tests/golden/critic_graph.npz), the NumPy restatement pve_mcc_amd/critic.py, the canonical
float32 order of csrc/pve_critic.h through a g++ host shim (tests/critic_host), and the three C ABI entry points through the
CPU test emulator (which has no critic kernels and must say so).  The kernels are checked in tests/test_gpu_critic.py.

Bars: spread_critic = max |graph float32 - graph float64| on the fixture's rows is the graph's own float32 round-off; a float32
evaluation in another order lies within one spread of the real value, hence within two of the graph's float64 value (a float32
result itself rounds to half an ulp of |Q| <= 148: 7.6e-6, well inside)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pve_mcc_amd import PveError, _capi, critic
from tests import native
from tests.critic_scenarios import load_critic_golden
from tests.hip_adapter import _np, emulator_lib, make_batch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _signatures(L):
    L.critic_canonical_many.argtypes = [C.c_void_p] * 4 + [C.c_longlong]
    L.bootstrap_canonical_many.argtypes = [C.c_void_p] * 5 + [C.c_longlong]
    return L


def shim():
    """csrc/pve_critic.h compiled by g++ (tests/critic_host), built and loaded by tests/native.py."""
    return native.load("critic_host", "libcritic_host.so", _signatures)


def flat_actor(w):
    return np.concatenate([np.asarray(w[k], np.float32).ravel() for k in critic.KEYS])


# ------------------------------------------------------------------ 1. what the decoded file says
def test_fixture_description():
    g = load_critic_golden()
    assert 1100 <= g.n <= 1400 and g.states.shape == (g.n, 7, 28) and g.states.dtype == np.float32
    assert (g.kinds == "closed_loop").sum() >= 900 and (g.kinds == "shaped").sum() == 280
    absent = (~g.states[g.kinds == "shaped"].any(axis=2)).sum(axis=1)
    assert sorted(set(absent)) == [0, 1, 2, 3, 4, 5, 6]                 # 0 .. 6 absent neighbours
    deg = g.states[g.kinds == "degenerate"]
    assert len(deg) == 2 and not deg[0, 0].any() and deg[0, 1:].any() and not deg[1].any()
    for net, scope, ph in (("critic", "agent1_critic", ("Placeholder", "Placeholder_1", "Placeholder_2")),
                           ("target_critic", "agent1_target_critic", ("Placeholder_5", "Placeholder_6", "Placeholder_7"))):
        d = g.meta[net]
        assert d["output"] == scope + "/dense_2/BiasAdd" and "ConcatV2" in d["ops"] and "Tanh" not in d["ops"]
        assert (d["state"], d["action"], d["other_action"]) == ph
        assert [d["placeholders"][p] for p in ph] == [[-1, 28], [-1, 1], [-1, 6]]
        # model_agent_maddpg.py:82 own action then the other actions; :66 hidden units then the actions
        assert d["concat"][d["concat_outer"]] == dict(inputs=[ph[1], ph[2]], axis=1)
        assert d["concat"][d["concat_inner"]] == dict(inputs=[scope + "/Relu", d["concat_outer"]], axis=-1)
        assert sorted(d["epsilon"].values()) == [float(np.float32(1e-12))] * 3
        shapes = {k[len(scope) + 1:]: v for k, v in d["variables"].items()}
        assert shapes["dense/kernel"] == [28, 64] and shapes["dense_1/kernel"] == [71, 64] and shapes["dense_2/kernel"] == [64, 1]
        assert critic.flat_critic_weights(g.weights[net]).size == _capi.PVE_CRITIC_N_WEIGHTS == 6841
    assert g.meta["target_actor"]["output"] == "agent1_targetactor/Mul"
    assert flat_actor(g.weights["target_actor"]).size == _capi.PVE_ACTOR_N_WEIGHTS
    # the recorded spreads are what the recorded values say; the issue's orders of magnitude hold
    s_c = max(np.abs(g.critic_q_f32 - g.critic_q_f64).max(), np.abs(g.target_q_f32 - g.target_q_f64).max())
    assert s_c == g.spread_critic and np.abs(g.boot_q_f32 - g.boot_q_f64).max() == g.spread_bootstrap
    assert 1e-4 < g.spread_critic < 1e-3 and 1e-4 < g.spread_bootstrap < 2e-3 and 5 < g.sens < 30
    assert g.boot_q_f64.min() < -100 and g.boot_q_f64.max() > 20


# ------------------------------------------------------------------ 2. the NumPy restatement
def test_numpy_restatement_vs_graph():
    g = load_critic_golden()
    w, tw, aw = g.weights["critic"], g.weights["target_critic"], g.weights["target_actor"]
    q64 = critic.critic_forward(w, g.given_rows, g.given_act7, np.float64)
    q32 = critic.critic_forward(w, g.given_rows, g.given_act7, np.float32)
    e64, e32 = np.abs(q64 - g.critic_q_f64).max(), np.abs(q32.astype(np.float64) - g.critic_q_f64).max()
    print("critic.py vs graph float64: float64 %.3e, float32 %.3e (bar %.3e)" % (e64, e32, 2 * g.spread_critic))
    assert q32.dtype == np.float32 and e64 <= 1e-9 and e32 <= 2 * g.spread_critic
    bq64, ba64 = critic.bootstrap_q(aw, tw, g.states, dtype=np.float64)
    # (the graph feeds the target actor's actions back through float32 placeholders; critic.py keeps them in float64)
    assert np.abs(ba64 - g.boot_act7_f64).max() <= 1e-9
    assert np.abs(bq64 - g.boot_q_f64).max() <= g.sens * 2.0 ** -23 * 3.0 * 2      # |a| <= 3 rounded to float32, both ways
    bq32, ba32 = critic.bootstrap_q(aw, tw, g.states, dtype=np.float32)
    assert np.abs(bq32.astype(np.float64) - g.boot_q_f64).max() <= 2 * g.spread_bootstrap
    # flags: only controlled rows that are not Done are evaluated
    flags = np.array([0, 1, 3, 7, 3 | 0x20, 1 | 4], np.int32)[np.arange(g.n) % 6]
    mq, ma = critic.bootstrap_q(aw, tw, g.states, flags, dtype=np.float32)
    ev = (flags == 3) | (flags == (3 | 0x20))
    assert np.all(mq[~ev] == 0) and np.all(ma[~ev] == 0)
    # (a BLAS product of fewer rows may round differently: float32 round-off, not bit equality)
    assert np.abs(mq[ev] - bq32[ev]).max() <= 2 * g.spread_bootstrap and np.abs(ma[ev] - ba32[ev]).max() <= 5e-4
    assert critic.bootstrap_q(aw, tw, g.states.reshape(10, -1, 7, 28), dtype=np.float32)[0].shape == (10, g.n // 10)


# ------------------------------------------------------------------ 3. the canonical float32 order of csrc/pve_critic.h
def test_critic_canonical_vs_graph():
    g = load_critic_golden()
    L = shim()
    assert L.critic_n_weights() == 6841
    w = critic.flat_critic_weights(g.weights["critic"])
    rows, a7 = np.ascontiguousarray(g.given_rows, np.float32), np.ascontiguousarray(g.given_act7, np.float32)
    q = np.empty(len(rows), np.float32)
    L.critic_canonical_many(w.ctypes.data, rows.ctypes.data, a7.ctypes.data, q.ctypes.data, len(rows))
    err = np.abs(q.astype(np.float64) - g.critic_q_f64).max()
    print("critic_canonical vs graph float64: %.3e (bar %.3e)" % (err, 2 * g.spread_critic))
    assert err <= 2 * g.spread_critic
    # the composition in the canonical orders (actor_canonical x 7, critic_canonical) against the graph's bootstrap
    aw, tw = flat_actor(g.weights["target_actor"]), critic.flat_critic_weights(g.weights["target_critic"])
    st = np.ascontiguousarray(g.states, np.float32)
    bq, ba = np.empty(g.n, np.float32), np.empty((g.n, 7), np.float32)
    L.bootstrap_canonical_many(aw.ctypes.data, tw.ctypes.data, st.ctypes.data, bq.ctypes.data, ba.ctypes.data, g.n)
    ea, eq = np.abs(ba - g.boot_act7_f64).max(), np.abs(bq - g.boot_q_f64).max()
    print("canonical bootstrap vs graph float64: actions %.3e, q %.3e" % (ea, eq))
    assert ea <= 5e-4 and eq <= 2 * g.spread_bootstrap


# ------------------------------------------------------------------ 4. exports, header, binding
def test_exports_header_and_binding_agree():
    lib = emulator_lib()
    header = open(os.path.join(ROOT, "include", "pve_env.h")).read()
    assert lib.pve_abi_version() == _capi.ABI_VERSION          # (version and constants against the header: tests/test_binding_contract.py)
    assert "main.py:253-260" in header and "PVE_ABI_VERSION stays 9" in header
    for name in ("pve_set_target_networks", "pve_critic_forward", "pve_bootstrap_q"):
        assert name in _capi.EXPORTS and hasattr(lib, name) and ("int %s(pve_handle h" % name) in header
    assert lib.pve_critic_forward.argtypes[-1] is C.c_int64 and lib.pve_bootstrap_q.argtypes[-1] is C.c_int64
    from pve_mcc_amd import BatchedIntersections, PipelinedIntersections
    for cls in (BatchedIntersections, PipelinedIntersections):
        for m in ("set_target_networks", "critic_q", "bootstrap_q"):
            assert callable(getattr(cls, m))
    # the workspace holds one more actor and one critic, flat and packed
    assert lib.pve_workspace_bytes(2, 64) >= 2 * (25600 + 26880) + 27364 + 30736


# ------------------------------------------------------------------ 5. the entry points on a backend without the kernels
def closed_loop(b, ticks):
    rewards = [_np(b.step_with_actor()["reward"]).copy() for _ in range(ticks)]
    acts = _np(b.act()).copy()
    fields = {k: _np(b.state_field(k)).copy() for k in ("p", "v", "a", "id", "meta", "step", "count")}
    return rewards, acts, fields, b.metrics()


def test_entry_points_on_the_emulator():
    from oracle.actor_np import flat_weights, load_weights
    from pve_mcc_amd.arrivals import synthetic_arrivals
    g = load_critic_golden()
    lib = emulator_lib()
    arr = synthetic_arrivals(2, rate=1000.0, horizon_s=40.0, seed=5)
    outs = ("obs_post", "reward", "flags", "env_out")
    plain, b = (make_batch(arr, 2, 64, "emu", outputs=outs) for _ in range(2))
    for x in (plain, b):
        x.reset()
        x.set_actor(flat_weights(load_weights()))
    st = np.zeros((3, 7, 28))
    a7, q = np.zeros((3, 7), np.float32), np.zeros(3, np.float32)
    aw, cw = flat_actor(g.weights["target_actor"]), critic.flat_critic_weights(g.weights["target_critic"])
    P = lambda x: x.ctypes.data                                              # noqa: E731
    # argument validation comes first
    for call, word in ((lambda: lib.pve_set_target_networks(None, P(aw), P(cw)), b"null"),
                     (lambda: lib.pve_set_target_networks(b._h, None, None), b"at least one"),
                     (lambda: lib.pve_critic_forward(None, P(st), P(a7), P(q), 3), b"null"),
                     (lambda: lib.pve_critic_forward(b._h, None, P(a7), P(q), 3), b"null"),
                     (lambda: lib.pve_critic_forward(b._h, P(st), None, P(q), 3), b"null"),
                     (lambda: lib.pve_critic_forward(b._h, P(st), P(a7), None, 3), b"null"),
                     (lambda: lib.pve_critic_forward(b._h, P(st), P(a7), P(q), 0), b"n must be > 0"),
                     (lambda: lib.pve_critic_forward(b._h, P(st), P(a7), P(q), -4), b"n must be > 0"),
                     (lambda: lib.pve_bootstrap_q(None, P(st), None, P(q), None, 3), b"null"),
                     (lambda: lib.pve_bootstrap_q(b._h, None, None, P(q), None, 3), b"null"),
                     (lambda: lib.pve_bootstrap_q(b._h, P(st), None, None, None, 3), b"null"),
                     (lambda: lib.pve_bootstrap_q(b._h, P(st), None, P(q), P(a7), 0), b"n must be > 0")):
        rc = call()
        assert rc == -1 and word in lib.pve_last_error(), (rc, lib.pve_last_error())
    # the emulator has no critic / bootstrap kernels: PVE_ERR_INVALID, and the message says why
    for call in (lambda: lib.pve_set_target_networks(b._h, P(aw), P(cw)), lambda: lib.pve_set_target_networks(b._h, None, P(cw)),
                 lambda: lib.pve_critic_forward(b._h, P(st), P(a7), P(q), 3),
                 lambda: lib.pve_bootstrap_q(b._h, P(st), None, P(q), P(a7), 3)):
        assert call() == -1 and b"backend has no critic / bootstrap kernels" in lib.pve_last_error()
    assert not q.any() and not a7.any()
    with pytest.raises(PveError, match="backend"):
        b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
    with pytest.raises(PveError, match="backend"):
        b.bootstrap_q(torch.zeros(3, 7, 28, dtype=torch.float64))
    with pytest.raises(PveError, match="backend"):
        b.critic_q(torch.zeros(3, 28, dtype=torch.float64), torch.zeros(3, 7))
    with pytest.raises(PveError):
        b.set_target_networks()
    with pytest.raises(PveError, match="state_pre"):
        b.bootstrap_q()                                                      # this batch has no state_pre output
    with pytest.raises(PveError, match="6841"):
        b.set_target_networks(critic=np.zeros(6393, np.float32))
    # the acting policy is what it was
    r0, a0, f0, m0 = closed_loop(plain, 40)
    r1, a1, f1, m1 = closed_loop(b, 40)
    assert m0 == m1 and m0["ctl_steps"] > 0 and np.array_equal(a0.view(np.uint64), a1.view(np.uint64)) and a0.any()
    for x, y in zip(r0, r1):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    for k in f0:
        assert np.array_equal(f0[k], f1[k]), k

"""The learner step without a GPU.  Three links of one chain (the fourth, kernel == host build bit for bit, is
tests/test_gpu_learner.py):
  1. LearnerModel(float64) -- the hand-written backward pass -- against torch autograd in float64 on networks built from torch ops;
  2. a g++ build of csrc/pve_learn.h (tests/learner_host) against LearnerModel(float64), step by step with teacher forcing, to
     the bar of tests/learner_scenarios.py (three times the float32 model's own spread);
  3. Adam and the soft update of the host build against a NumPy float32 restatement, bit for bit.
Plus the direction of a step, the critic-only mode, the C ABI's argument checks and the refusal of the CPU emulators, which
have no learner kernels and say so."""
import ctypes as C

import numpy as np
import pytest

from pve_mcc_amd import Learner, LearnerModel, PveError, _capi
from pve_mcc_amd import learner as LN
from tests import learner_scenarios as S
from tests.hip_adapter import emulator_lib, make_batch

ROOT = S.ROOT


# ------------------------------------------------------------------ 0. layout and the tanh of the header
def test_layout_is_the_headers():
    out = np.zeros(16, np.int32)
    S.shim().learner_host_layout(S._ptr(out))
    assert out.tolist()[:14] == [LN.ACTOR, LN.CRITIC, LN.TARGET_ACTOR, LN.TARGET_CRITIC, LN.M_ACTOR, LN.V_ACTOR, LN.M_CRITIC, LN.V_CRITIC,
                                 LN.POWERS, LN.STEPS, LN.GRAD, LN.N_FLOATS, LN.N_ACTOR, LN.N_CRITIC]
    # learner.py takes the offsets from _capi's LEARNER_*, which tests/test_binding_contract.py holds to the header's macros
    for name, v in (("ACTOR", LN.ACTOR), ("CRITIC", LN.CRITIC), ("TARGET_ACTOR", LN.TARGET_ACTOR), ("TARGET_CRITIC", LN.TARGET_CRITIC),
                    ("M_ACTOR", LN.M_ACTOR), ("V_ACTOR", LN.V_ACTOR), ("M_CRITIC", LN.M_CRITIC), ("V_CRITIC", LN.V_CRITIC),
                    ("POWERS", LN.POWERS), ("STEPS", LN.STEPS), ("GRAD", LN.GRAD), ("N_FLOATS", LN.N_FLOATS)):
        assert v == getattr(_capi, "LEARNER_" + name)
        assert v % 4 == 0                                        # every segment starts 16-byte aligned
    assert LN.CRITIC_ONLY == _capi.LEARN_CRITIC_ONLY == 1


def test_tanh3_of_the_header():
    """learn_tanh3 is a rational function of + - * / and fmaf: within 4e-7 of 3 tanh(z) relative, odd, bounded by 3 (so
    the derivative is never negative), exactly 0 at 0, and its derivative is 3 (1 - (a / 3)^2) of the forward value."""
    z = np.sort(np.concatenate([np.linspace(-12, 12, 400001), np.random.default_rng(0).normal(0, 1, 100000),
                                [0.0, -0.0, 1e-30, -1e-30, 9.0, -9.0, 50.0, -50.0, 1e30, -1e30]]).astype(np.float32))
    a, d = np.zeros_like(z), np.zeros_like(z)
    S.shim().learner_host_tanh3(S._ptr(z), len(z), S._ptr(a), S._ptr(d))
    ref = 3 * np.tanh(z.astype(np.float64))
    rel = np.abs(a - ref) / np.maximum(np.abs(ref), 1e-300)
    assert rel.max() <= 4e-7, rel.max()
    assert np.all(np.abs(a) <= 3.0) and np.all(a[z == 0] == 0) and np.all(d >= 0) and np.all(a[np.abs(z) >= 9] == 3 * np.sign(z[np.abs(z) >= 9]))
    za, nz = np.zeros_like(z), np.ascontiguousarray(-z)
    S.shim().learner_host_tanh3(S._ptr(nz), len(z), S._ptr(za), S._ptr(d))
    assert np.array_equal(S.bits32(za), S.bits32(-a))
    t = a / np.float32(3)
    assert np.array_equal(S.bits32(d), S.bits32(np.float32(3) * (np.float32(1) - t * t)))


# ------------------------------------------------------------------ 1. the semantics against an independent derivation
def _torch_net(w, rows, act7=None):
    import torch

    def ln(x, g, b):
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        return (x - mean) / torch.sqrt(var + float(np.float32(1e-12))) * g + b

    x = ln(rows, w["ln0_gamma"], w["ln0_beta"])
    x = torch.relu(ln(x @ w["w1"] + w["b1"], w["ln1_gamma"], w["ln1_beta"]))
    if act7 is not None:
        x = torch.cat([x, act7], dim=-1)
    x = torch.relu(ln(x @ w["w2"] + w["b2"], w["ln2_gamma"], w["ln2_beta"]))
    z = (x @ w["w3"] + w["b3"])[..., 0]
    return z if act7 is not None else 3.0 * torch.tanh(z)


@pytest.mark.parametrize("zero_units", [False, True])
@pytest.mark.parametrize("batch", [1, 5, 128])
def test_model_gradients_equal_autograd(batch, zero_units):
    """LearnerModel(float64): both losses and their gradients == torch autograd in float64, the actor loss differentiated
    through the critic; to 1e-9 of each tensor's largest magnitude."""
    import torch
    a, c, _, _ = S.nets(zero_units)
    rows, act7, target = (x[0] for x in S.minibatches(batch, 1, seed=10 + batch))
    m = LearnerModel(a, c, dtype=np.float64, **S.HYPER)
    t64 = lambda x: torch.tensor(np.asarray(x, np.float64))                  # noqa: E731
    wa = {k: t64(v).requires_grad_(True) for k, v in LN.unflat_weights(a, False).items()}
    wc = {k: t64(v).requires_grad_(True) for k, v in LN.unflat_weights(c, True).items()}
    R, A, T = t64(rows), t64(act7), t64(target)
    # critic loss
    loss_c = ((T - _torch_net(wc, R, A)) ** 2).mean()
    gc = torch.autograd.grad(loss_c, [wc[k] for k in LN.KEYS])
    got_l, got_g = m.critic_gradients(rows, act7, target)
    assert abs(got_l - loss_c.item()) <= 1e-9 * abs(loss_c.item())
    for (k, v), ref in zip(LN.unflat_weights(got_g, True).items(), gc):
        assert S.rel_dev(v, ref.numpy()) <= 1e-9, ("critic", k)
    # actor loss, through the critic
    act = torch.cat([_torch_net(wa, R)[:, None], A[:, 1:]], dim=-1)
    loss_a = -_torch_net(wc, R, act).mean()
    ga = torch.autograd.grad(loss_a, [wa[k] for k in LN.KEYS])
    got_l, got_g = m.actor_gradients(rows, act7)
    assert abs(got_l - loss_a.item()) <= 1e-9 * abs(loss_a.item())
    for (k, v), ref in zip(LN.unflat_weights(got_g, False).items(), ga):
        assert np.abs(ref.numpy()).max() > 0 and S.rel_dev(v, ref.numpy()) <= 1e-9, ("actor", k)


# ------------------------------------------------------------------ 2. the header against the semantics
def test_recorded_spread_is_current():
    """The figure behind the bar, measured again: the float32 model's spread stays below the bar derived from the record"""
    worst, where = S.measure_f32_spread()
    print("LearnerModel(float32) against float64: %.3e at %s (recorded %.3e)" % (worst, where, S.F32_SPREAD_MEASURED))
    assert worst <= S.HEADER_BAR


@pytest.mark.parametrize("label,zero_units,batch,n_steps,seed", S.header_batches())
def test_host_build_follows_the_model(label, zero_units, batch, n_steps, seed):
    """Teacher forcing: before every step the model takes the host build's whole state, so Adam's sensitivity to the sign of
    tiny gradients does not accumulate; gradients (per tensor) and losses within HEADER_BAR of LearnerModel(float64)."""
    P = S.host_block(S.nets(zero_units))
    rows, act7, target = S.minibatches(batch, n_steps, seed=seed)
    worst = 0.0
    for s in range(n_steps):
        l64, g64 = S.model(P, np.float64).step(rows[s], act7[s], target[s])
        lh, gh = S.host_step(P, rows[s], act7[s], target[s])
        got, ref = S.split_grads(gh[0]), S.split_grads(g64)
        for k in got:
            d = S.rel_dev(got[k], ref[k])
            worst = max(worst, d)
            assert d <= S.HEADER_BAR, (label, s, k, d)
        for j in range(2):
            d = S.rel_dev(lh[0][j], l64[j])
            worst = max(worst, d)
            assert d <= S.HEADER_BAR, (label, s, "loss", j, d)
        assert int(P[LN.STEPS:LN.STEPS + 1].view(np.int32)[0]) == s + 1
    print("%s: host build against LearnerModel(float64), worst tensor %.3e (bar %.3e)" % (label, worst, S.HEADER_BAR))


def test_zero_units_give_exact_zeros():
    """the exact-zero scenario is what it says: the zeroed LayerNorm units output exactly 0, ReLU passes nothing back through
    them, so the rows of the next dense kernel they feed get an exactly zero gradient"""
    P = S.host_block(S.nets(True))
    _, g = S.host_step(P, *S.minibatches(128, 1, seed=2))
    d = S.split_grads(g[0])
    for net in ("critic", "actor"):
        assert np.all(d[net + "/w2"][[3, 17, 40]] == 0) and np.all(d[net + "/w3"][[0, 31, 63]] == 0)
        assert np.any(d[net + "/w2"][[4, 18, 41]] != 0)


# ------------------------------------------------------------------ 3. Adam and the soft update, bit for bit
@pytest.mark.parametrize("critic_only", [False, True])
def test_adam_and_soft_update_are_exact(critic_only):
    """Given the host build's own gradients, a NumPy float32 line-by-line restatement reproduces w, m, v, the powers and the
    targets bit for bit, over 6 steps from a state with non-zero moments (every operation is correctly rounded in both)."""
    P = S.warmed_block().copy()
    rows, act7, target = S.minibatches(64, 6, seed=21)
    h = S.HYPER
    seg = {"critic": (LN.CRITIC, LN.TARGET_CRITIC, LN.M_CRITIC, LN.V_CRITIC, LN.POWERS + 2, LN.N_CRITIC, h["critic_lr"]),
           "actor": (LN.ACTOR, LN.TARGET_ACTOR, LN.M_ACTOR, LN.V_ACTOR, LN.POWERS, LN.N_ACTOR, h["actor_lr"])}
    for s in range(6):
        before = P.copy()
        _, g = S.host_step(P, rows[s], act7[s], target[s], critic_only=critic_only)
        grads = {"critic": g[0, :LN.N_CRITIC], "actor": g[0, LN.N_CRITIC:]}
        for net, (ow, ot, om, ov, op, n, lr) in seg.items():
            if net == "actor" and critic_only:
                for o, k in ((ow, n), (ot, n), (om, n), (ov, n), (op, 2)):
                    assert np.array_equal(S.bits32(P[o:o + k]), S.bits32(before[o:o + k]))
                assert np.all(grads["actor"] == 0)
                continue
            w, m, v, b1p, b2p = LN.adam_update(before[ow:ow + n], before[om:om + n], before[ov:ov + n], grads[net], lr, before[op],
                                               before[op + 1], h["beta1"], h["beta2"], h["epsilon"], np.float32)
            tgt = LN.soft_update(w, before[ot:ot + n], h["tau"], np.float32)
            for name, got, ref in (("w", P[ow:ow + n], w), ("m", P[om:om + n], m), ("v", P[ov:ov + n], v), ("target", P[ot:ot + n], tgt),
                                   ("powers", P[op:op + 2], np.array([b1p, b2p], np.float32))):
                assert ref.dtype == np.float32 and np.array_equal(S.bits32(got), S.bits32(ref)), (s, net, name)
            assert np.array_equal(S.bits32(P[LN.GRAD + (0 if net == "critic" else 6844):][:n]), S.bits32(grads[net]))


def test_steps_in_one_call_equal_single_calls():
    rows, act7, target = S.minibatches(37, 3, seed=5)
    P1, P2 = S.warmed_block().copy(), S.warmed_block().copy()
    l1, g1 = S.host_step(P1, rows, act7, target)
    for s in range(3):
        l2, g2 = S.host_step(P2, rows[s], act7[s], target[s])
        assert np.array_equal(S.bits32(l1[s]), S.bits32(l2[0])) and np.array_equal(S.bits32(g1[s]), S.bits32(g2[0]))
    assert np.array_equal(S.bits32(P1), S.bits32(P2))


@pytest.mark.parametrize("bsz", [1, 5, 7, 36, 128])
def test_sub_block_sizes_change_no_bit(bsz):
    """the header built with sub-blocks of 7 / 5 rows instead of 64 / 32 (ragged tails at other places): the same block, losses
    and gradients, bit for bit"""
    sub = S.shim("liblearner_host_sub.so")
    out = np.zeros(16, np.int32)
    sub.learner_host_layout(S._ptr(out))
    assert out.tolist()[14:] == [7, 5]
    S.shim().learner_host_layout(S._ptr(out))
    assert out.tolist()[14:] == [64, 32]
    rows, act7, target = S.minibatches(bsz, 3, seed=50 + bsz)
    P1, P2 = S.warmed_block(True).copy(), S.warmed_block(True).copy()
    l1, g1 = S.host_step(P1, rows, act7, target)
    l2, g2 = S.host_step(P2, rows, act7, target, lib=sub)
    assert np.array_equal(S.bits32(l1), S.bits32(l2)) and np.array_equal(S.bits32(g1), S.bits32(g2))
    assert np.array_equal(S.bits32(P1), S.bits32(P2))


# ------------------------------------------------------------------ 4. direction, critic-only mode
def test_twenty_steps_lower_the_critic_loss():
    P = S.host_block(S.nets())
    rows, act7, target = S.minibatches(128, 1, seed=31)
    losses = [S.host_step(P, rows, act7, target)[0][0] for _ in range(20)]
    print("critic loss over 20 steps on one minibatch: %.6f -> %.6f; actor loss %.6f -> %.6f"
          % (losses[0][0], losses[-1][0], losses[0][1], losses[-1][1]))
    assert losses[-1][0] < losses[0][0]


@pytest.mark.parametrize("warmed", [False, True])
def test_critic_only_leaves_the_actor_alone(warmed):
    P = S.warmed_block().copy() if warmed else S.host_block(S.nets())
    before = P.copy()
    losses, grads = S.host_step(P, *S.minibatches(50, 3, seed=41), critic_only=True)
    for o, n in ((LN.ACTOR, 6396), (LN.TARGET_ACTOR, 6396), (LN.M_ACTOR, 6396), (LN.V_ACTOR, 6396), (LN.POWERS, 2), (LN.GRAD_ACTOR, 6396)):
        assert np.array_equal(S.bits32(P[o:o + n]), S.bits32(before[o:o + n]))
    for o, n in ((LN.CRITIC, LN.N_CRITIC), (LN.TARGET_CRITIC, LN.N_CRITIC), (LN.M_CRITIC, LN.N_CRITIC), (LN.V_CRITIC, LN.N_CRITIC), (LN.POWERS + 2, 2)):
        assert not np.array_equal(S.bits32(P[o:o + n]), S.bits32(before[o:o + n]))
    assert np.all(losses[:, 1] == 0) and np.all(grads[:, LN.N_CRITIC:] == 0) and np.all(losses[:, 0] > 0)
    # the critic's half of the step is the full step's
    Q = before.copy()
    l2, g2 = S.host_step(Q, *[x[:1] for x in S.minibatches(50, 3, seed=41)])
    assert np.array_equal(S.bits32(l2[0, 0]), S.bits32(losses[0, 0])) and np.array_equal(S.bits32(g2[0, :LN.N_CRITIC]), S.bits32(grads[0, :LN.N_CRITIC]))


# ------------------------------------------------------------------ 5. the C ABI on a backend without the kernel
def _emulators():
    from tests import rank_pairs_scenarios, test_capacity256
    return {"emu": emulator_lib, "emu_wide": test_capacity256.wide_lib, "emu_diag": rank_pairs_scenarios.diag_emulator_lib}


def test_entry_points_on_the_emulator():
    from pve_mcc_amd.arrivals import synthetic_arrivals
    lib = emulator_lib()
    for name in ("pve_learner_init", "pve_learner_step"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert lib.pve_abi_version() == _capi.ABI_VERSION
    b = make_batch(synthetic_arrivals(2, rate=500.0, horizon_s=20.0, seed=1), 2, 64, "emu", outputs=("obs_post", "flags"))
    keep = []

    def P(n, off=0):
        raw = np.zeros(n * 4 + 32, np.uint8)
        keep.append(raw)
        return raw.ctypes.data + (-raw.ctypes.data) % 16 + off

    batch, nb = 8, 3
    params, actor, critic = P(LN.N_FLOATS), P(LN.N_ACTOR), P(LN.N_CRITIC)
    rows, act7, target, losses, grads = P(nb * batch * 28), P(nb * batch * 7), P(nb * batch), P(nb * 2), P(nb * LN.N_GRADS)

    def lr(**kw):
        r = _capi.PveLearner()
        r.params, r.flags, r.block_threads = params, 0, 0
        for k, v in S.HYPER.items():
            setattr(r, k, v)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def init(r=None, h=b._h, nets=(actor, critic, None, None)):
        return lib.pve_learner_init(h, C.byref(r) if r is not None else None, *nets)

    def step(r=None, h=b._h, inp=(rows, act7, target), batch=batch, nb=nb, out=(losses, grads)):
        return lib.pve_learner_step(h, C.byref(r) if r is not None else None, *inp, batch, nb, *out)

    inf, nan = float("inf"), float("nan")
    shared = [(dict(params=None), b"null params"), (dict(params=params + 4), b"aligned"), (dict(actor_lr=inf), b"finite"),
              (dict(actor_lr=nan), b"finite"), (dict(critic_lr=-inf), b"finite"), (dict(critic_lr=nan), b"finite"),
              (dict(epsilon=nan), b"finite"), (dict(epsilon=inf), b"finite"), (dict(tau=nan), b"finite"), (dict(tau=inf), b"finite"),
              (dict(tau=-0.001), b"tau"), (dict(tau=1.001), b"tau"), (dict(beta1=1.0), b"beta"), (dict(beta2=-0.5), b"beta"),
              (dict(beta1=nan), b"beta"), (dict(flags=2), b"flags"), (dict(block_threads=100), b"block_threads"),
              (dict(block_threads=2048), b"block_threads"), (dict(block_threads=-64), b"block_threads")]
    for kw, word in shared:
        for fn in (init, step):
            assert fn(lr(**kw)) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    for fn in (lambda: init(lr(), h=None), lambda: init(None), lambda: step(lr(), h=None), lambda: step(None)):
        assert fn() == -1 and b"null" in lib.pve_last_error()
    for kw, word in ((dict(nets=(None, critic, None, None)), b"null actor or critic"), (dict(nets=(actor, None, None, None)), b"null actor or critic"),
                     (dict(nets=(actor + 4, critic, None, None)), b"aligned"), (dict(nets=(actor, critic + 8, None, None)), b"aligned"),
                     (dict(nets=(actor, critic, actor + 4, None)), b"aligned"), (dict(nets=(actor, critic, None, critic + 4)), b"aligned")):
        assert init(lr(), **kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    for kw, word in ((dict(inp=(None, act7, target)), b"null rows"), (dict(inp=(rows, None, target)), b"null rows"),
                     (dict(inp=(rows, act7, None)), b"null rows"), (dict(batch=0), b"batch"), (dict(batch=-3), b"batch"),
                     (dict(nb=0), b"n_batches"), (dict(nb=-1), b"n_batches"), (dict(batch=1 << 20, nb=1 << 12), b"n_batches"),
                     (dict(inp=(rows + 4, act7, target)), b"aligned"), (dict(inp=(rows, act7 + 2, target)), b"aligned"),
                     (dict(inp=(rows, act7, target + 1)), b"aligned"), (dict(out=(losses + 2, grads)), b"aligned"),
                     (dict(out=(losses, grads + 3)), b"aligned")):
        assert step(lr(), **kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    # valid arguments: no learner kernels here, and the library says so (optional pointers NULL, the extremes of every range)
    for fn in (lambda: init(lr()), lambda: init(lr(), nets=(actor, critic, actor, critic)), lambda: step(lr()),
               lambda: step(lr(), out=(None, None)), lambda: step(lr(flags=1, block_threads=1024, tau=0.0), batch=1, nb=1),
               lambda: step(lr(tau=1.0, beta1=0.0, block_threads=64), inp=(rows, act7 + 4, target + 4))):
        assert fn() == -1 and b"backend has no learner kernels" in lib.pve_last_error(), lib.pve_last_error()
    # the Python class asks the backend
    a, c, _, _ = S.nets()
    with pytest.raises(PveError, match="backend"):
        Learner(b, a, c)
    with pytest.raises(ValueError, match="weights"):
        Learner(b, a[:-1], c)


@pytest.mark.parametrize("which", ["emu", "emu_wide", "emu_diag"])
def test_every_emulator_refuses(which):
    """each CPU emulator exports both symbols, validates, and refuses valid calls with PVE_ERR_INVALID"""
    from pve_mcc_amd.arrivals import synthetic_arrivals
    from pve_mcc_amd.batched import BatchedIntersections
    lib = _emulators()[which]()
    assert hasattr(lib, "pve_learner_init") and hasattr(lib, "pve_learner_step")
    b = BatchedIntersections(1, 64, synthetic_arrivals(1, rate=500.0, horizon_s=20.0, seed=1), device="cpu", outputs=("obs_post",), _lib=lib)
    raw = np.zeros(LN.N_FLOATS * 4 + 32, np.uint8)
    p = raw.ctypes.data + (-raw.ctypes.data) % 16
    r = _capi.PveLearner()
    r.params = p
    for k, v in S.HYPER.items():
        setattr(r, k, v)
    assert lib.pve_learner_init(b._h, C.byref(r), p, p, None, None) == -1 and b"backend has no learner kernels" in lib.pve_last_error()
    assert lib.pve_learner_step(b._h, C.byref(r), p, p, p, 4, 2, None, None) == -1 and b"backend has no learner kernels" in lib.pve_last_error()
    assert lib.pve_learner_step(b._h, C.byref(r), p, p, p, 0, 2, None, None) == -1 and b"batch" in lib.pve_last_error()
    assert not np.any(raw)                                        # nothing was written

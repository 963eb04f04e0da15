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


# ------------------------------------------------------------------ 4b. the float32 range (learner_scenarios: families A .. F)
# First that every scenario IS in the regime it is named for (on the host build; a scenario that never leaves the normal range
# proves nothing), then what can be said there without a GPU.  tests/test_gpu_learner.py holds the kernel to these host results.
SUB = "liblearner_host_sub.so"


def _subnormal_words(P, grads):
    seg = S.segments(P)
    return dict(grads=S.count_subnormal(grads), **{k: S.count_subnormal(seg[k]) for k in ("m_actor", "v_actor", "m_critic", "v_critic")})


@pytest.mark.parametrize("name", [n for n in S.RANGE_CASES if n[0] == "A"])
def test_family_a_is_subnormal(name):
    """scaled heads: thousands of subnormal words in the gradients and in Adam's moments, everything finite; from a fresh state and
    from one with non-zero moments alike"""
    s = S.range_case(name)["s"]
    _, P, losses, grads = S.range_run(name)
    n = _subnormal_words(P, grads)
    print("%s: subnormal words %s of %d non-zero gradient words" % (name, n, int((grads != 0).sum())))
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(grads)) and np.all(np.isfinite(losses))
    if s in (62, 70):
        assert n["grads"] >= 1000
    if s == 62:
        assert n["v_critic"] >= 1000
    if s == 100:
        assert n["m_critic"] >= 1000 and n["v_actor"] >= 100
    if S.range_case(name)["warmed"]:
        start = S.segments(S.range_start(name))
        # (non-zero moments, powers below beta; at s = 100 every g * g underflows to zero during the warm-up, and v with it)
        assert all(np.any(start[k] != 0) for k in ("m_actor", "m_critic")) and start["powers"][0] < S.HYPER["beta1"]
        assert all(np.any(start[k] != 0) == (s < 100) for k in ("v_actor", "v_critic"))
        assert np.array_equal(S.bits32(start["critic"][:LN.N_CRITIC]), S.bits32(S.range_networks(name)[1]))    # (the scaled head is still there)


def test_family_c_reaches_the_fixed_point_of_b1p():
    """1 100 steps of batch 2: b1p *= 0.9f is subnormal and moving at step 850 and sits at 4 quanta at step 1 100, where
    0.9f * 4 quanta rounds back to 4; calls of 50 minibatches == one call of 1 100 == the sub-block build"""
    L = S.long_run()
    P = L[S.LONG_STEPS]
    for k in (S.LONG_MOVING, S.LONG_MOVING + S.LONG_CALL, S.LONG_STEPS):
        print("step %4d: b1p %.6e (%d quanta), b2p %.6f" % (k, L[k][LN.POWERS], S.bits32(L[k][LN.POWERS:LN.POWERS + 1])[0], L[k][LN.POWERS + 1]))
    assert S.bits32(P[LN.POWERS:LN.POWERS + 1])[0] == S.bits32(S.B1P_FIXED_POINT) == 4 and P[LN.POWERS + 2] == S.B1P_FIXED_POINT
    assert np.float32(S.HYPER["beta1"]) * S.B1P_FIXED_POINT == S.B1P_FIXED_POINT
    assert int(P[LN.STEPS:LN.STEPS + 1].view(np.int32)[0]) == S.LONG_STEPS and all(np.all(np.isfinite(b)) for b in L.values())
    moving, later = L[S.LONG_MOVING][LN.POWERS], L[S.LONG_MOVING + S.LONG_CALL][LN.POWERS]
    assert S.B1P_FIXED_POINT < later < moving < S.TINY
    one, sub = S.long_run(call=S.LONG_STEPS), S.long_run(lib=SUB)
    assert np.array_equal(S.bits32(one[S.LONG_STEPS]), S.bits32(P))
    for k in (S.LONG_MOVING, S.LONG_STEPS):
        assert np.array_equal(S.bits32(sub[k]), S.bits32(L[k])), k


@pytest.mark.parametrize("name", [n for n in S.RANGE_CASES if n[0] in "CEF"])
def test_range_cases_stay_finite_and_keep_their_bits_across_builds(name):
    """C (three minibatches of 65 rows from the long run's state), E and F: the block stays finite; the sub-block build and three
    single calls give the same bits"""
    c = S.range_case(name)
    inp, P, losses, grads = S.range_run(name)
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(grads)) and np.all(np.isfinite(losses)), name
    _, P2, l2, g2 = S.range_run(name, lib=SUB)
    assert np.array_equal(S.bits32(P), S.bits32(P2)) and np.array_equal(S.bits32(losses), S.bits32(l2)) and np.array_equal(S.bits32(grads), S.bits32(g2))
    Q = S.range_start(name).copy()
    for k in range(c["n"]):
        l1, g1 = S.host_step(Q, *(x[k] for x in inp), **c["hyper"])
        assert np.array_equal(S.bits32(l1[0]), S.bits32(losses[k])) and np.array_equal(S.bits32(g1[0]), S.bits32(grads[k]))
    assert np.array_equal(S.bits32(Q), S.bits32(P))
    if c["long"]:
        assert 0 < S.range_start(name)[LN.POWERS] < S.TINY and 0 < P[LN.POWERS] < S.TINY


def test_family_e_hyper_parameters_do_what_they_say():
    """each end of a range is visible in the block, so the bit-equality of tests/test_gpu_learner.py says that the kernel received it"""
    seg = {n: (S.segments(S.range_start(n)), S.segments(S.range_run(n)[1])) for n in S.RANGE_CASES if n[0] == "E"}
    for net in ("actor", "critic"):
        a, z = seg["E-tau-1"]
        assert np.array_equal(S.bits32(z["target_" + net]), S.bits32(a["target_" + net])) and not np.array_equal(z[net], a[net])
        a, z = seg["E-tau-0"]
        assert np.array_equal(S.bits32(z["target_" + net]), S.bits32(z[net])) and not np.array_equal(z[net], a[net])
    a, z = seg["E-beta1-0"]
    assert a["powers"][0] > 0 and z["powers"][0] == 0 and z["powers"][2] == 0 and z["powers"][1] > 0
    a, z = seg["E-lr-0-1"]
    assert np.array_equal(S.bits32(z["actor"]), S.bits32(a["actor"])) and np.any(z["m_actor"] != a["m_actor"])
    assert np.abs(z["critic"] - a["critic"]).max() > 0.5                                   # (critic_lr = 1: Adam's steps are of order 1)
    # epsilon = 1e-40 is a float32 subnormal and is honoured: the zero-gradient weights of the exact-zero-ReLU networks divide
    # 0 by sqrt(v) + 1e-40 and stay; with epsilon = 0 they divide 0 by 0 (include/pve_env.h says so)
    assert 0 < np.float32(1e-40) < S.TINY
    name = "E-epsilon-1e-40"
    a, z = seg[name]
    dead = (z["v_critic"] == 0) & (z["m_critic"] == 0)
    assert dead.sum() >= 64 and np.array_equal(S.bits32(z["critic"][dead]), S.bits32(a["critic"][dead]))
    Q = S.range_start(name).copy()
    S.host_step(Q, *S.range_inputs(name), want=False, **dict(S.range_case(name)["hyper"], epsilon=0.0))
    print("epsilon = 0 on the exact-zero-ReLU networks: %d NaN words in the block" % S.count_nan(Q))
    assert S.count_nan(Q) > 0 and S.count_nan(S.range_run(name)[1]) == 0


def test_family_f_underflows_inside_the_input_layernorm():
    """the observable: `r0`, the rstd of the input LayerNorm that LearnerModel's tape exposes (learner_scenarios.underflowed_input_rows)"""
    rows = S.range_inputs("F-tiny-rows")[0]
    n = S.underflowed_input_rows(rows)
    print("F-tiny-rows: %d of %d rows have d * d underflowed to zero in the input LayerNorm" % (n, rows.shape[0] * rows.shape[1]))
    assert n >= 1 and S.underflowed_input_rows(S.minibatches(65, 2, seed=9)[0]) == 0


def test_same_words():
    """the comparison tests/test_gpu_learner.py uses where NaN occurs: equal NaN masks, every other word bit-equal"""
    w = lambda *bits: np.array(bits, np.uint32).view(np.float32)                         # noqa: E731
    qnan, xnan, snan, inf, ninf = 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000
    assert S.is_nan_word(np.array([qnan, xnan, snan, inf, ninf, 0, 1], np.uint32)).tolist() == [True, True, True, False, False, False, False]
    assert S.same_words(w(qnan, inf, 1, 0), w(xnan, inf, 1, 0)) and S.same_words(w(snan), w(qnan))
    assert not S.same_words(w(qnan, inf), w(qnan, ninf))                                 # an infinity keeps its sign
    assert not S.same_words(w(qnan, 5), w(5, qnan)) and not S.same_words(w(qnan), w(inf)) and not S.same_words(w(0), w(0x80000000))
    assert not S.same_words(w(1), w(2)) and not S.same_words(w(1, 2), w(1)) and S.same_words(w(4), w(4))
    S.check_words(w(qnan, 7), w(xnan, 7), "nan_ok", nan_ok=True)
    for got, ref, ok in ((w(qnan, 7), w(xnan, 7), False), (w(qnan, 7), w(qnan, 8), True), (w(3, 7), w(3, 8), False)):
        with pytest.raises(AssertionError):
            S.check_words(got, ref, "differs", nan_ok=ok)


def test_family_d_overflows_and_keeps_its_words_across_builds():
    """targets x 2^60: the critic loss is +inf in minibatch 0, the block holds NaN and infinities; the sub-block build gives the
    same words (same_words: x86 gives every NaN as 0xFFC00000, so here the bits are equal as well)"""
    _, P, losses, grads = S.range_run("D-overflow")
    print("D-overflow: %d NaN words and %d infinities in the block, losses %s" % (S.count_nan(P), int(np.isinf(P).sum()), losses.tolist()))
    assert losses[0, 0] == np.inf and S.count_nan(P) >= 1 and int(np.isinf(P).sum()) >= 1
    _, P2, l2, g2 = S.range_run("D-overflow", lib=SUB)
    assert S.same_words(P, P2) and S.same_words(losses, l2) and S.same_words(grads, g2)
    assert not S.same_words(P, S.range_start("D-overflow"))


# ---- B. below the underflow the header is exactly scale-equivariant
@pytest.mark.parametrize("library", [None, SUB])
@pytest.mark.parametrize("s", [20, 40])
def test_scaled_head_is_exactly_equivariant(s, library):
    """w3, b3 of the critic and the targets times 2^-s: Q, dQ and the gradients of w3 and b3 carry 2^-s, every critic gradient
    upstream (dQ * w3 first) 2^-2s, the critic loss 2^-2s -- exactly, every operation of the header being a correctly rounded
    + - * / fmaf or sqrtf on operands scaled by a power of two, as long as nothing leaves the normal range.  First minibatch of a
    call only: Adam is not scale-equivariant (epsilon; sqrt(v)), so the second minibatch meets another critic.
    The actor side: the actor loss is -mean Q of the UPDATED critic, which is linear in (w3, b3), so it and every actor gradient
    carry 2^-s exactly IF the two critics are the same function up to the head's scale.  Behind Adam's step with the reference's
    critic_lr they are not (w -= m alpha / (sqrt(v) + epsilon) moves the scaled and the unscaled critic differently), so the
    exponent is asserted with critic_lr = 0, which leaves both critics where they were (w -= 0 / (..) is exact)."""
    lib = S.shim(library) if library else None
    res = {}
    for e in (0, s):
        for lr in (S.HYPER["critic_lr"], 0.0):
            P = S.host_block(S.scaled_head(e))
            res[e, lr] = S.host_step(P, *S.scaled_minibatches(65, 1, 5, e), lib=lib, critic_lr=lr)
    scaled = lambda x, k: np.ldexp(x, -k * s).astype(np.float32)                          # noqa: E731
    for lr in (S.HYPER["critic_lr"], 0.0):
        (l0, g0), (ls, gs) = res[0, lr], res[s, lr]
        a, b = S.split_grads(g0[0]), S.split_grads(gs[0])
        for k in a:
            if k.startswith("critic/"):
                assert np.any(a[k] != 0) and np.array_equal(S.bits32(b[k]), S.bits32(scaled(a[k], 1 if k in ("critic/w3", "critic/b3") else 2))), (k, lr)
            elif lr == 0.0:
                assert np.any(a[k] != 0) and np.array_equal(S.bits32(b[k]), S.bits32(scaled(a[k], 1))), k
        assert np.array_equal(S.bits32(ls[0, 0]), S.bits32(scaled(l0[0, 0], 2)))
        if lr == 0.0:
            assert np.array_equal(S.bits32(ls[0, 1]), S.bits32(scaled(l0[0, 1], 1)))


# ---- A at s = 62 and 70, F: the header against the semantics, by the rule of section 2
def test_recorded_subnormal_spread_is_current():
    """the figure behind SUBNORMAL_BAR, measured again (the one behind HEADER_BAR: test_recorded_spread_is_current, which
    measures on these scenarios too)"""
    worst, where = S.measure_f32_spread(subnormal=True)
    print("LearnerModel(float32) against float64, tensors with a subnormal largest entry: %.3e at %s (recorded %.3e)"
          % (worst, where, S.F32_SPREAD_SUBNORMAL_MEASURED))
    assert where is not None and worst <= S.SUBNORMAL_BAR
    worst, where = S.measure_f32_spread([b[0] for b in S.range_header_batches()])
    print("LearnerModel(float32) against float64 on the range scenarios, all other tensors: %.3e at %s (recorded %.3e)"
          % (worst, where, S.F32_SPREAD_MEASURED))
    assert worst <= S.F32_SPREAD_MEASURED                      # below the record: it needs no constant of its own


@pytest.mark.parametrize("label", [b[0] for b in S.range_header_batches()])
def test_host_build_follows_the_model_in_the_range(label):
    """as test_host_build_follows_the_model: gradients (per tensor) and losses within HEADER_BAR of LearnerModel(float64) -- within
    SUBNORMAL_BAR for a tensor whose largest entry is itself subnormal (learner_scenarios.header_bar)"""
    networks, (rows, act7, target) = S.header_inputs(label)
    P = S.host_block(networks)
    worst = {False: 0.0, True: 0.0}
    for s in range(len(rows)):
        l64, g64 = S.model(P, np.float64).step(rows[s], act7[s], target[s])
        lh, gh = S.host_step(P, rows[s], act7[s], target[s])
        got, ref = S.split_grads(gh[0]), S.split_grads(g64)
        got.update(critic_loss=lh[0][0], actor_loss=lh[0][1])
        ref.update(critic_loss=l64[0], actor_loss=l64[1])
        for k in got:
            d, sub = S.rel_dev(got[k], ref[k]), S.is_subnormal_tensor(ref[k])
            worst[sub] = max(worst[sub], d)
            assert d <= S.header_bar(ref[k]), (label, s, k, d)
    print("%s: host build against LearnerModel(float64), worst tensor %.3e (bar %.3e); with a subnormal largest entry %.3e (bar %.3e)"
          % (label, worst[False], S.HEADER_BAR, worst[True], S.SUBNORMAL_BAR))


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

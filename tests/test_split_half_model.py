"""The split-half evaluation on the CPU: tests/split_half_model.py (the NumPy statement of `k_actor_pack` / `actor_tile32` and of
`k_critic_pack` / `critic_tile32`) against float64 NumPy on every weight set and row family of tests/split_half_scenarios.py,
within the bars stated there.  tests/test_gpu_split_half.py holds the kernels to the same bars and to this model.

The loss this file was written to see.  WITHOUT the pack-time scale (`scaled=False`: what the kernels did before it) the model's
max |a - a_float64| on the well-conditioned rows of actor_graph.npz, against the bar min(3 x spread + T, ACTION_TOL):
    fresh-0                      1.9e-6   bar 1.7e-6        w1-x2^-3     8.6e-4   bar 5.0e-4
    fresh-first-layer-0 / 1 / 2  1.9e-3 / 1.8e-3 / 1.0e-3   bars 9.8e-5 / 1.1e-4 / 5.4e-5
    fresh-second-layer-0 / 1 / 2 4.7e-6 / 1.4e-4 / 8.7e-5   bars 2.5e-6 / 1.4e-5 / 6.7e-6
    w1-x2^-10    1.5e-1   bar 5.0e-4        w2-x2^-7     7.3e-4   bar 5.0e-4
    w1-x2^-16    2.7      bar 2.3e-4        w2-x2^-14    1.1e-1   bar 5.0e-4
and on Q (bar 3 x spread_q): fresh-0 3.6e-7 (1.9e-8), fresh-first-layer-0 2.0e-2 (1.1e-3), fresh-second-layer-0 4.0e-3 (6.3e-4),
w1-x2^-10 4.6e-2, w1-x2^-16 4.2, w2-x2^-7 1.4e-3, w2-x2^-14 3.3e-1 (all 1.0e-3 .. 1.1e-3).  test_unscaled_model_misses_the_bars
keeps that statement alive: the bars do see the defect.  WITH the scale every one of these is inside its bar.

Families whose bar is 2 x the model's own maximum (split_half_scenarios.MODEL_BARS): rows whose LayerNorm_0 output is far below 1
-- the all-zero row and rows with a spread far below sqrt(1e-12) leave only ln0_beta, and a freshly initialised beta is 0 to 1e-5.
That activation is a B operand: it is split at run time, in f16's subnormal range, and the pack-time scale of the KERNELS cannot
reach it.  The recorded maxima are this model's, never a device's."""
import struct

import numpy as np
import pytest

from oracle.actor_np import load_weights
from pve_mcc_amd import critic as CR
from tests import split_half_model as M
from tests import split_half_scenarios as S
from tests.actor_scenarios import ACTION_TOL, load_graph_golden
from tests.critic_scenarios import load_critic_golden


# ------------------------------------------------------------------ 1. the shipped weights: the model is the kernel the suite knows
def test_model_on_shipped_weights():
    rows, kinds, a32, a64, meta, well = load_graph_golden()
    a = M.actor_split(load_weights(), rows[well]).astype(np.float64)
    worst = float(np.abs(a - a64[well]).max())
    print("actor model vs graph float64 on %d rows: %.3e (bar %.1e)" % (well.sum(), worst, ACTION_TOL))
    assert worst <= ACTION_TOL
    g = load_critic_golden()
    n = g.n
    for net, ra, want in (("critic", (g.given_rows, g.given_act7), g.critic_q_f64),
                          ("target_critic", (g.states[:, 0], g.boot_act7_f64.astype(np.float32)), g.target_q_f64)):
        q = M.critic_split(g.weights[net], *ra).astype(np.float64)
        worst = float(np.abs(q - want).max())
        print("%s model vs graph float64 on %d rows: %.3e (bar %.3e)" % (net, len(q), worst, 2 * g.spread_critic))
        assert worst <= 2 * g.spread_critic
    q, a7 = M.bootstrap_split(g.weights["target_actor"], g.weights["target_critic"], g.states)
    assert np.abs(a7 - g.boot_act7_f64).max() <= ACTION_TOL and q.shape == (n,)
    assert np.abs(q - g.boot_q_f64).max() <= 3 * g.spread_critic + g.sens * ACTION_TOL


# ------------------------------------------------------------------ 2. every weight set, every row family
@pytest.mark.parametrize("name", list(S.actor_sets()))
def test_actor_model_within_bars(name):
    w = S.actor_sets()[name]
    rows, family, names = S.all_actor_rows()
    a64 = CR.actor_forward(w, rows, np.float64)
    a32 = CR.actor_forward(w, rows, np.float32).astype(np.float64)
    a = M.actor_split(w, rows).astype(np.float64)
    assert np.all(np.isfinite(a))
    for i, fam in enumerate(names):
        m = family == i
        spread, worst = float(np.abs(a32[m] - a64[m]).max()), float(np.abs(a[m] - a64[m]).max())
        bar = S.actor_bar(name, fam, spread)
        print("actor %-30s %-13s spread %.3e  model %.3e  bar %.3e%s" % (name, fam, spread, worst, bar,
                                                                        "  (2 x model)" if ("actor", name, fam) in S.MODEL_BARS else ""))
        assert worst <= bar, (name, fam)
        S.check_model_bar_needed("actor", name, fam, worst, S.action_bar(spread))


@pytest.mark.parametrize("name", list(S.critic_sets()))
def test_critic_model_within_bars(name):
    w = S.critic_sets()[name]
    rows, act7 = S.critic_rows()
    q64, spread = S.ref_q(w, rows, act7)
    q = M.critic_split(w, rows, act7).astype(np.float64)
    worst = float(np.abs(q - q64).max())
    bar = S.critic_bar(name, spread)
    print("critic %-30s spread %.3e  model %.3e  bar %.3e  max |Q| %.3e" % (name, spread, worst, bar, np.abs(q64).max()))
    assert np.all(np.isfinite(q)) and worst <= bar
    S.check_model_bar_needed("critic", name, "rows", worst, S.q_bar(spread))


@pytest.mark.parametrize("name", list(S.bootstrap_pairs()))
def test_bootstrap_model_within_bars(name):
    aw, cw = S.bootstrap_pairs()[name]
    st = S.bootstrap_states()
    q64, a64, q_bar, a_bar, info = S.ref_bootstrap(aw, cw, st)
    q, a7 = M.bootstrap_split(aw, cw, st)
    worst_a, worst_q = float(np.abs(a7 - a64).max()), float(np.abs(q - q64).max())
    print("bootstrap %-36s actions %.3e (bar %.3e)  q %.3e (bar %.3e)  %s" % (name, worst_a, a_bar, worst_q, q_bar, info))
    assert worst_a <= a_bar and worst_q <= q_bar


# ------------------------------------------------------------------ 3. the bars see the defect the scale removes
LOST_WITHOUT_SCALE = ("fresh-0", "fresh-first-layer-0", "fresh-first-layer-1", "fresh-first-layer-2", "fresh-second-layer-0",
                      "w1-x2^-3", "w1-x2^-10", "w1-x2^-16", "w2-x2^-7", "w2-x2^-14")
LOST_WITHOUT_SCALE_CRITIC = ("fresh-0", "fresh-first-layer-0", "fresh-second-layer-0", "w1-x2^-10", "w1-x2^-16", "w2-x2^-7",
                             "w2-x2^-14")


def test_unscaled_model_misses_the_bars():
    """The packing without the scale rule (e = 0, the literal 1e-12) is outside the bars on the freshly initialised and the
    rescaled sets, inside them with the rule: reverting the rule alone turns this file red on exactly these sets."""
    rows = S.actor_rows()["graph"]
    for name in LOST_WITHOUT_SCALE:
        w = S.actor_sets()[name]
        a64, spread = S.ref_actions(w, rows)
        with np.errstate(all="ignore"):
            lost = float(np.abs(M.actor_split(w, rows, scaled=False) - a64).max())
        kept = float(np.abs(M.actor_split(w, rows) - a64).max())
        print("actor %-24s without the scale %.3e, with it %.3e, bar %.3e" % (name, lost, kept, S.action_bar(spread)))
        assert kept <= S.action_bar(spread) < lost, name
    rows, act7 = S.critic_rows()
    for name in LOST_WITHOUT_SCALE_CRITIC:
        w = S.critic_sets()[name]
        q64, spread = S.ref_q(w, rows, act7)
        lost = float(np.abs(M.critic_split(w, rows, act7, scaled=False) - q64).max())
        kept = float(np.abs(M.critic_split(w, rows, act7) - q64).max())
        print("critic %-24s without the scale %.3e, with it %.3e, bar %.3e" % (name, lost, kept, S.q_bar(spread)))
        assert kept <= S.q_bar(spread) < lost, name
    # hi overflows f16 without the scale: not a loss of bits but inf in the operands -- NaN out of the LayerNorm, which the
    # ReLU's fmaxf turns into 0: every row gets the same, wrong action
    base, rows = load_weights(), S.actor_rows()["graph"][:256]
    for layer, e in ((1, 18), (2, 16)):
        k, b = "w%d" % layer, "b%d" % layer
        w = dict(base, **{k: base[k] * np.float32(2.0 ** e), b: base[b] * np.float32(2.0 ** e)})
        a64, spread = S.ref_actions(w, rows)
        with np.errstate(all="ignore"):
            lost = M.actor_split(w, rows, scaled=False)
        assert np.ptp(lost) == 0 and np.abs(lost - a64).max() > 0.5, (layer, e)
        assert np.abs(M.actor_split(w, rows) - a64).max() <= S.action_bar(spread), (layer, e)


# ------------------------------------------------------------------ 4. the scale rule
def test_scale_rule():
    g = load_critic_golden()
    for w in (load_weights(), g.weights["critic"], g.weights["target_critic"], g.weights["target_actor"]):
        p = M.Packed(w)
        assert p.e == [0, 0] and all(e.tobytes() == np.float32(1e-12).tobytes() for e in p.eps)
    two = lambda e: np.float32(2.0) ** np.float32(e)                   # noqa: E731
    below = lambda x: np.nextafter(np.float32(x), np.float32(0))       # noqa: E731
    above = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))  # noqa: E731
    assert M.pack_exponent(0.0) == 0
    assert M.pack_exponent(two(-3)) == 0 and M.pack_exponent(two(12)) == 0 and M.pack_exponent(1.0) == 0
    assert M.pack_exponent(below(two(-3))) == 4 and M.pack_exponent(above(two(12))) == -12
    assert M.pack_exponent(3e-3) == 9 and M.pack_exponent(two(-40)) == 40 and M.pack_exponent(two(-41)) == 40
    assert M.pack_exponent(two(60)) == -40 and M.pack_exponent(np.float32(1e-45)) == 40
    for m in np.float32(2.0) ** np.random.default_rng(1).uniform(-40, 40, 500).astype(np.float32):
        e = M.pack_exponent(m)
        assert e == 0 and two(-3) <= m <= two(12) or 1.0 <= float(m) * 2.0 ** e < 2.0, (m, e)
    # the epsilon that goes with it is an exact, normal float32 for every e the rule can give
    for e in (-40, -12, 9, 40):
        eps = np.float32(np.float32(1e-12) * np.float32(4.0) ** np.float32(e))
        assert float(eps) == float(np.float32(1e-12)) * 4.0 ** e and eps > np.finfo(np.float32).tiny
    # and the packed operands of a scaled set: the largest |hi| in [1, 2], every operand finite
    for name in ("fresh-0", "w1-x2^-16", "w2-x2^12"):
        p = M.Packed(S.actor_sets()[name])
        for e, kh in zip(p.e, p.kh):
            assert np.all(np.isfinite(kh)) and (e == 0 or 1.0 <= np.abs(kh).max() <= 2.0), (name, e)


# ------------------------------------------------------------------ 5. the split itself
def half_of(x):
    """float -> the nearest f16 value (ties to even), by the C library's conversion through struct: independent of NumPy's"""
    try:
        return struct.unpack("<e", struct.pack("<e", float(x)))[0]
    except OverflowError:
        return float(np.copysign(np.inf, x))


def test_split_keeps_22_bits_while_lo_is_normal():
    r = np.random.default_rng(3)
    x = (r.uniform(1, 2, 20000) * 2.0 ** r.integers(-3, 15, 20000) * r.choice([-1, 1], 20000)).astype(np.float32)
    x = np.concatenate([x, np.float32([0.125, -0.125, 32767.998, 1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 + 2.0 ** -21])])
    assert np.abs(x).min() >= 2.0 ** -3 and np.abs(x).max() < 2.0 ** 15
    hi, lo = M.split(x)
    rel = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x) / np.abs(x)
    print("hi + lo vs x on |x| in [2^-3, 2^15): max relative %.3e (2^-22 = %.3e)" % (rel.max(), 2.0 ** -22))
    assert rel.max() <= 2.0 ** -22
    # below 2^-3 the claim fails, which is why the rule scales: at 3e-3 only ~14 bits are left
    y = (x * np.float32(2.0 ** -9)).astype(np.float32)
    hi, lo = M.split(y)
    assert (np.abs(hi.astype(np.float64) + lo.astype(np.float64) - y) / np.abs(y)).max() > 2.0 ** -16


def test_split_definition_on_subnormal_and_overflowing_inputs():
    xs = np.float32([0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 3e-8, 5.97e-8, 6.1e-5, 6.103e-5, 2.0 ** -14, 1e-3, 3e-3,
                     65504.0, 65519.9, 65520.0, 1e5, -7e4, 3.4e38, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1e-30, -1e-10])
    hi, lo = M.split(xs)
    for x, h, l in zip(xs, hi, lo):
        want_h = half_of(x)
        assert float(h) == want_h and np.signbit(h) == np.signbit(np.float32(want_h)), x
        if np.isinf(want_h):
            assert np.isinf(l) and np.sign(l) == -np.sign(want_h), x          # x - inf: the pair is lost, hi + lo = NaN
        else:
            d = np.float32(x) - np.float32(want_h)                            # exact in float32
            assert float(d) == float(x) - want_h and float(l) == half_of(d), x

"""Weight sets, rows and bars for the split-half actor and critic, shared by tests/test_split_half_model.py (CPU: the NumPy model of
tests/split_half_model.py) and tests/test_gpu_split_half.py (the kernels).  Everything is generated from seeds and from fixtures
already committed (actor_66.npz, actor_graph.npz, critic_graph.npz).

Why these sets: the kernels multiply f16 half pairs, x = hi + lo, and the pair holds 22 bits only while lo is a normal f16
number.  The shipped checkpoint (dense kernels up to 0.44 and 1.25) is the one scale the rest of the suite visits; the reference
initialises every dense kernel with uniform(-3e-3, 3e-3) (model_agent_maddpg.py:29-41, :61-73), two to three orders of magnitude
below it, and training moves through everything in between.  LayerNorm makes each dense layer scale-invariant, so float32 and
float64 do not care -- the half pairs do, and k_*_pack's power-of-two scale (split_half_model.pack_exponent) is what makes them not.

Bars (none of them taken from what the kernels or the model return):
  actions:   min(3 x spread_a(W) + T, ACTION_TOL).  spread_a(W) = max |float32 NumPy - float64 NumPy| of the SAME weights on the rows
             under test: two float32 evaluations in different orders lie within one spread of the real value each, the third spread
             is for the 2^-22 half pairs.  T = ACTOR_TANH3_BAR (tests/math_probe_scenarios.py, profiles/math_probe.txt) covers the
             v_exp / v_rcp head, which a NumPy float32 evaluation does not contain.
  Q:         3 x spread_q(W), likewise.
  bootstrap: 3 x spread_q(W) + sens(W) x the action bar; sens(W) = max sum_k |dQ/da_k|, float64 central differences, h = 1e-3:
             the definition tests/golden/gen_critic_golden.py records in the fixture."""
import functools

import numpy as np

from oracle.actor_np import load_weights
from pve_mcc_amd import critic as CR
from pve_mcc_amd import learner as LN
from pve_mcc_amd.critic import KEYS
from tests.actor_scenarios import ACTION_TOL, load_graph_golden
from tests.critic_scenarios import load_critic_golden
from tests.math_probe_scenarios import ACTOR_TANH3_BAR

INIT = 3e-3                                     # model_agent_maddpg.py: every dense kernel ~ uniform(-3e-3, 3e-3), biases 0
FRESH_SEEDS = (0, 1, 2)
ACTOR_W1_EXP, ACTOR_W2_EXP = (-3, -10, -16, 12), (-7, -14, 12)
GAMMA_EXP = {False: 12, True: 10}               # ln1_gamma x 2^e inside |gamma| sqrt(63) + |beta| < 65 504 (include/pve_env.h):
#                                                 the actor's largest ln1_gamma is 1.83 (59 350 at 2^12), the critics' 4.83 (39 300 at 2^10)


def _copy(w):
    return {k: np.array(w[k], np.float32) for k in KEYS}


def fresh(seed, critic=False):
    """the reference's initialisation: dense kernels U(+-3e-3), biases 0, gammas 1, betas 0"""
    r = np.random.default_rng(7000 + 10 * seed + int(critic))
    k2 = 71 if critic else 64
    u = lambda *s: r.uniform(-INIT, INIT, s).astype(np.float32)        # noqa: E731
    one, zero = lambda n: np.ones(n, np.float32), lambda n: np.zeros(n, np.float32)   # noqa: E731
    return dict(ln0_gamma=one(28), ln0_beta=zero(28), w1=u(28, 64), b1=zero(64), ln1_gamma=one(64), ln1_beta=zero(64),
                w2=u(k2, 64), b2=zero(64), ln2_gamma=one(64), ln2_beta=zero(64), w3=u(64, 1), b3=zero(1))


def _with(base, **repl):
    w = _copy(base)
    for k, v in repl.items():
        w[k] = np.asarray(v, np.float32)
    return w


def _scaled(base, layer, e):
    s = np.float32(2.0) ** np.float32(e)
    return _with(base, **{"w%d" % layer: base["w%d" % layer] * s, "b%d" % layer: base["b%d" % layer] * s})


@functools.lru_cache(maxsize=None)
def learned():
    """{(start, steps): {"actor" | "target_actor" | "critic" | "target_critic": dict}}: LearnerModel (float32 NumPy) for 4 and for 64
    steps on minibatches of 32 from the learner tests' fixture, once from learner_scenarios.nets(), once from fresh networks"""
    from tests import learner_scenarios as LS
    rows, act7, target = LS.minibatches(32, 64, seed=5)
    out = {}
    for start in ("fixture", "fresh"):
        if start == "fixture":
            a, c, ta, tc = LS.nets()
        else:
            a, c = LN.flat_weights(fresh(0), False), LN.flat_weights(fresh(0, True), True)
            ta, tc = a.copy(), c.copy()
        m = LN.LearnerModel(a, c, ta, tc, dtype=np.float32, **LS.HYPER)
        for s in range(64):
            m.step(rows[s], act7[s], target[s])
            if s + 1 in (4, 64):
                out[(start, s + 1)] = {k: _copy(LN.unflat_weights(m.net[k].astype(np.float32), "critic" in k)) for k in m.net}
    return out


def _family(base, critic, w1_exp, w2_exp, fresh_seeds):
    sets = {}
    for s in fresh_seeds:
        f = fresh(s, critic)
        sets["fresh-%d" % s] = f
        sets["fresh-first-layer-%d" % s] = _with(base, w1=f["w1"], b1=f["b1"])
        sets["fresh-second-layer-%d" % s] = _with(base, w2=f["w2"], b2=f["b2"])
    for e in w1_exp:
        sets["w1-x2^%d" % e] = _scaled(base, 1, e)
    for e in w2_exp:
        sets["w2-x2^%d" % e] = _scaled(base, 2, e)
    k2 = base["w2"].shape[0]
    sets["offset"] = _with(base, w2=base["w2"] + np.linspace(-8, 8, k2, dtype=np.float32)[:, None])
    sets["dead-most"] = _with(base, ln1_beta=base["ln1_beta"] - np.float32(3))
    sets["dead-all"] = _with(base, ln1_beta=base["ln1_beta"] - np.float32(30))
    sets["gamma-x2^%d" % GAMMA_EXP[critic]] = _with(base, ln1_gamma=base["ln1_gamma"] * np.float32(2.0 ** GAMMA_EXP[critic]))
    return sets


@functools.lru_cache(maxsize=None)
def actor_sets():
    """name -> weight dict, in a fixed order"""
    base = load_weights()
    sets = {"shipped": _copy(base)}
    sets.update(_family(base, False, ACTOR_W1_EXP, ACTOR_W2_EXP, FRESH_SEEDS))
    for (start, steps), nets in learned().items():
        sets["learned-%s-%d" % (start, steps)] = nets["actor"]
        sets["learned-%s-%d-target" % (start, steps)] = nets["target_actor"]
    return sets


@functools.lru_cache(maxsize=None)
def critic_sets():
    g = load_critic_golden()
    sets = {"critic": _copy(g.weights["critic"]), "target_critic": _copy(g.weights["target_critic"])}
    fam = _family(g.weights["target_critic"], True, ACTOR_W1_EXP, ACTOR_W2_EXP, FRESH_SEEDS)
    sets.update(fam)
    for (start, steps), nets in learned().items():
        sets["learned-%s-%d-target" % (start, steps)] = nets["target_critic"]
    return sets


# ---------------------------------------------------------------------------------- rows
@functools.lru_cache(maxsize=None)
def actor_rows():
    """name -> float32 [n, 28]: the well-conditioned rows of actor_graph.npz, the same x 2^-16 and x 2^16, the all-zero row"""
    rows, kinds, a32, a64, meta, well = load_graph_golden()
    base = np.ascontiguousarray(rows[well & (np.abs(rows).max(axis=1) > 0)], np.float32)
    out = {"graph": base, "graph-x2^-16": base * np.float32(2.0 ** -16), "graph-x2^16": base * np.float32(2.0 ** 16),
           "zero": np.zeros((1, 28), np.float32)}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def all_actor_rows():
    r = actor_rows()
    names = list(r)
    rows = np.concatenate([r[k] for k in names])
    family = np.concatenate([np.full(len(r[k]), i) for i, k in enumerate(names)])
    rows.setflags(write=False)
    return rows, family, names


@functools.lru_cache(maxsize=None)
def critic_rows():
    """(rows [n, 28], act7 [n, 7]): row 0 of the fixture's states with `given_act7` (both action sets), then every 4th row with all
    actions at +3, at -3 and alternating"""
    g = load_critic_golden()
    sub = g.states[::4, 0]
    alt = np.where(np.arange(7) % 2 == 0, 3.0, -3.0).astype(np.float32)
    rows = np.concatenate([g.given_rows, sub, sub, sub]).astype(np.float32)
    act7 = np.concatenate([g.given_act7, np.full((len(sub), 7), 3, np.float32), np.full((len(sub), 7), -3, np.float32),
                           np.broadcast_to(alt, (len(sub), 7))]).astype(np.float32)
    rows.setflags(write=False)
    act7.setflags(write=False)
    return rows, act7


@functools.lru_cache(maxsize=None)
def bootstrap_states():
    """float32 [n, 7, 28]: every second state of the fixture (absent neighbours and the two degenerate states at its end included)"""
    g = load_critic_golden()
    st = np.ascontiguousarray(np.concatenate([g.states[::2], g.states[-2:]]), np.float32)
    st.setflags(write=False)
    return st


def bootstrap_pairs():
    """name -> (target actor, target critic)"""
    a, c, L = actor_sets(), critic_sets(), learned()
    return {"fresh": (a["fresh-0"], c["fresh-0"]),
            "learned": (L[("fresh", 64)]["target_actor"], L[("fresh", 64)]["target_critic"]),
            "fresh-first-layer x rescaled critic": (a["fresh-first-layer-0"], c["w1-x2^-10"])}


# ---------------------------------------------------------------------------------- references and bars
def ref_actions(w, rows):
    """(float64 actions, spread_a) on these rows"""
    with np.errstate(over="ignore", invalid="ignore"):
        a64 = CR.actor_forward(w, rows, np.float64)
        a32 = CR.actor_forward(w, rows, np.float32)
    return a64, float(np.abs(a32.astype(np.float64) - a64).max())


def action_bar(spread):
    return min(3.0 * spread + ACTOR_TANH3_BAR, ACTION_TOL)


# Families whose bar is 2 x the maximum of the CPU model (tests/split_half_model.py, with the scale rule), because the model itself
# exceeds 3 x spread there: (kind, weight set, row family) -> the model's max |. - float64|, recorded from tests/test_split_half_model.py.
#   * x 2^-16 rows and all-zero rows on fresh networks: 48 of the graph rows have a spread of 1e-7, 1e-12 after the scaling, far
#     below sqrt(epsilon) = 1e-6, so LayerNorm_0 returns ~1e-6 (+ ln0_beta, which is 0 to 2e-5 there): an ACTIVATION in f16's subnormal
#     range, split at run time; the pack-time scale of the kernels does not reach it, and a fresh b1 = 0 does not mask it;
#   * learned-fixture-64-target: e = 0 for both layers (the half pairs are the shipped ones'), the model is 3.06 x the spread of
#     this one float32 evaluation: the margin of a bar built on ONE float32 order, not a loss of the half pairs.
MODEL_BARS = {
    ("actor", "fresh-0", "graph-x2^-16"): 5.883e-4,
    ("actor", "fresh-1", "graph-x2^-16"): 4.809e-4,
    ("actor", "fresh-2", "graph-x2^-16"): 3.483e-4,
    ("actor", "learned-fresh-4-target", "graph-x2^-16"): 4.471e-6,
    ("actor", "learned-fixture-64-target", "graph"): 1.260e-4,
    ("actor", "learned-fixture-64-target", "graph-x2^16"): 1.260e-4,
    ("critic", "learned-fresh-4-target", "rows"): 7.395e-8,
}


def actor_bar(name, family, spread):
    """the bar of one actor weight set on one row family: min(3 x spread + T, ACTION_TOL), or 2 x the model's recorded maximum"""
    rec = MODEL_BARS.get(("actor", name, family))
    return action_bar(spread) if rec is None else 2.0 * rec


def critic_bar(name, spread):
    rec = MODEL_BARS.get(("critic", name, "rows"))
    return q_bar(spread) if rec is None else 2.0 * rec


def check_model_bar_needed(kind, name, family, model_max, standard_bar):
    """a MODEL_BARS entry must be what the model gives (not more) and must be needed (the model is over the standard bar)"""
    rec = MODEL_BARS.get((kind, name, family))
    if rec is not None:
        assert standard_bar < model_max <= rec * 1.002, (kind, name, family, model_max, rec, standard_bar)


def ref_q(w, rows, act7):
    """(float64 Q, spread_q)"""
    q64 = CR.critic_forward(w, rows, act7, np.float64)
    q32 = CR.critic_forward(w, rows, act7, np.float32)
    return q64, float(np.abs(q32.astype(np.float64) - q64).max())


def q_bar(spread):
    return 3.0 * spread


def sensitivity(w, rows, act7, h=1e-3):
    """max over rows of sum_k |dQ/da_k|: float64 central differences on float32-rounded displaced actions (gen_critic_golden.py)"""
    a7 = np.asarray(act7, np.float32)
    total = np.zeros(len(rows))
    for k in range(7):
        up, dn = a7.copy(), a7.copy()
        up[:, k] += np.float32(h)
        dn[:, k] -= np.float32(h)
        dq = CR.critic_forward(w, rows, up, np.float64) - CR.critic_forward(w, rows, dn, np.float64)
        total += np.abs(dq / (up[:, k].astype(np.float64) - dn[:, k].astype(np.float64)))
    return float(total.max())


def ref_bootstrap(actor_w, critic_w, state):
    """float64 (q, act7) and the bars (q_bar, a_bar) of the composition"""
    q64, a64 = CR.bootstrap_q(actor_w, critic_w, state, dtype=np.float64)
    _, spread_a = ref_actions(actor_w, state)
    a_bar = action_bar(spread_a)
    q32 = CR.critic_forward(critic_w, state[:, 0], a64, np.float32)
    spread_q = float(np.abs(q32.astype(np.float64) - q64).max())
    sens = sensitivity(critic_w, state[:, 0], a64)
    return q64, a64, q_bar(spread_q) + sens * a_bar, a_bar, dict(spread_a=spread_a, spread_q=spread_q, sens=sens)

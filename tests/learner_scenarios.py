"""Inputs, scenarios and the host build of csrc/pve_learn.h (tests/learner_host) shared by tests/test_learner.py and
tests/test_gpu_learner.py.  Everything comes from fixtures already committed: the online critic, the target critic and the target
actor, row 0 of every state, `given_act7` and `target_q_f32` (as the targets) from tests/golden/critic_graph.npz, the online actor
from tests/golden/actor_66.npz."""
import ctypes as C
import functools
import os

import numpy as np

from pve_mcc_amd import learner as LN
from pve_mcc_amd.critic import KEYS
from tests import native
from tests.critic_scenarios import load_critic_golden
from tests.parity_util import GOLDEN_DIR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HYPER = dict(actor_lr=1e-4, critic_lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, tau=0.998)       # the reference's run

# ---------------------------------------------------------------------------------- the bar of "the header against the semantics"
# The host build's gradients and losses are compared with LearnerModel(float64) on the same float32 inputs, per tensor, as
# max |difference| / max |tensor|.  The bar is THREE times the largest such figure of LearnerModel(float32) against
# LearnerModel(float64) -- the margin DESIGN §13 gives its own spread -- over the batches of header_batches() below (20 teacher-forced
# steps from the fixture weights on batches of 128 with the all-zero rows, and one step each on the exact-zero-ReLU networks and on
# batches of 1 and 5): the two float32 evaluations differ only in the order of their sums, so they scatter around the
# real-valued result alike.  Measured by measure_f32_spread(): 6.31e-4, on the critic's dense_2 bias gradient at step 10 of the
# teacher-forced run -- that gradient is 2 mean(Q - target), a sum that cancels as the bias settles, which is where float32 shows; the
# host build's own figure against float64 on the same batches is 3.2e-4, on the same tensor.
F32_SPREAD_MEASURED = 6.31e-4
HEADER_BAR = 3 * F32_SPREAD_MEASURED


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def shim(name="liblearner_host.so"):
    """csrc/pve_learn.h compiled by g++ (tests/learner_host), built and loaded by tests/native.py.
    "liblearner_host_sub.so" is the same header with sub-blocks of 7 / 5 rows instead of 64 / 32."""
    return native.load("learner_host", name, _signatures)


def _signatures(L):
    vp = C.c_void_p
    L.learner_host_layout.restype = None
    L.learner_host_layout.argtypes = [vp]
    L.learner_host_init.restype = None
    L.learner_host_init.argtypes = [vp, vp, vp, vp, vp, C.c_float, C.c_float]
    L.learner_host_step.restype = None
    L.learner_host_step.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.learner_host_tanh3.restype = None
    L.learner_host_tanh3.argtypes = [vp, C.c_longlong, vp, vp]
    return L


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


class Fixture:
    pass


@functools.lru_cache(maxsize=None)
def fixture():
    g = load_critic_golden()
    f = Fixture()
    z = np.load(os.path.join(GOLDEN_DIR, "actor_66.npz"))
    f.actor = LN.flat_weights({k: z[k] for k in KEYS}, False)
    f.critic = LN.flat_weights(g.weights["critic"], True)
    f.target_critic = LN.flat_weights(g.weights["target_critic"], True)
    f.target_actor = LN.flat_weights(g.weights["target_actor"], False)
    f.rows = np.ascontiguousarray(g.states[:, 0], np.float32)
    f.act7 = np.ascontiguousarray(g.given_act7[:g.n], np.float32)
    f.target = np.ascontiguousarray(g.target_q_f32, np.float32)
    f.zero_rows = np.nonzero(np.abs(f.rows).sum(axis=1) == 0)[0]
    assert len(f.zero_rows) >= 2                                   # the fixture's degenerate states
    for a in (f.actor, f.critic, f.target_critic, f.target_actor, f.rows, f.act7, f.target):
        a.setflags(write=False)
    return f


def nets(zero_units=False):
    """(actor, critic, target_actor, target_critic), flat float32.  zero_units: gamma = beta = 0 on some units of LayerNorm_1 and
    LayerNorm_2 of the critic and the actor (targets too), so that ReLU sees exact zeros there."""
    f = fixture()
    out = [f.actor.copy(), f.critic.copy(), f.target_actor.copy(), f.target_critic.copy()]
    if zero_units:
        for w, crit in zip(out, (False, True, False, True)):
            d = LN.unflat_weights(w, crit)
            for k, units in (("ln1", (3, 17, 40)), ("ln2", (0, 31, 63))):
                d[k + "_gamma"][list(units)] = 0
                d[k + "_beta"][list(units)] = 0
    return out


def minibatches(batch, n_batches, seed=0, zero_rows=True):
    """(rows [n, batch, 28], act7 [n, batch, 7], target [n, batch]) drawn from the fixture; with zero_rows every minibatch of 3 rows
    or more holds the fixture's all-zero rows (at positions 1 and batch - 1)."""
    f = fixture()
    r = np.random.default_rng(1000 + seed)
    idx = np.stack([r.choice(len(f.rows), batch, replace=False) for _ in range(n_batches)])
    if zero_rows and batch >= 3:
        idx[:, 1], idx[:, batch - 1] = f.zero_rows[0], f.zero_rows[1]
    return np.ascontiguousarray(f.rows[idx]), np.ascontiguousarray(f.act7[idx]), np.ascontiguousarray(f.target[idx])


def hyper_array(**kw):
    h = dict(HYPER, **kw)
    return np.array([h[k] for k in ("actor_lr", "critic_lr", "beta1", "beta2", "epsilon", "tau")], np.float32)


def host_block(networks, beta1=HYPER["beta1"], beta2=HYPER["beta2"]):
    """pve_learner_init of the host build -> float32 [N_FLOATS]"""
    P = np.zeros(LN.N_FLOATS, np.float32)
    a, c, ta, tc = [np.ascontiguousarray(w, np.float32) if w is not None else None for w in networks]
    shim().learner_host_init(_ptr(P), _ptr(a), _ptr(c), _ptr(ta), _ptr(tc), np.float32(beta1), np.float32(beta2))
    return P


def host_step(P, rows, act7, target, critic_only=False, want=True, lib=None, **hyper):
    """pve_learner_step of the host build, in place on P -> (losses [n, 2], grads [n, 13234]) (None with want=False)"""
    rows, act7, target = (np.ascontiguousarray(x, np.float32) for x in (rows, act7, target))
    if rows.ndim == 2:
        rows, act7, target = rows[None], act7[None], target[None]
    n, B = rows.shape[:2]
    assert act7.shape == (n, B, 7) and target.shape == (n, B) and P.dtype == np.float32 and P.size == LN.N_FLOATS
    losses = np.zeros((n, 2), np.float32) if want else None
    grads = np.zeros((n, LN.N_GRADS), np.float32) if want else None
    h = hyper_array(**hyper)
    (lib or shim()).learner_host_step(_ptr(P), _ptr(h), LN.CRITIC_ONLY if critic_only else 0, _ptr(rows), _ptr(act7), _ptr(target), B, n,
                             _ptr(losses), _ptr(grads))
    return losses, grads


@functools.lru_cache(maxsize=None)
def warmed_block(zero_units=False):
    """A state that has taken 5 steps on batches of 32 (non-zero moments, powers below beta); read-only"""
    P = host_block(nets(zero_units))
    host_step(P, *minibatches(32, 5, seed=77), want=False)
    P.setflags(write=False)
    return P


def split_grads(g):
    """one row of `grads` -> {"critic/<key>": array, "actor/<key>": array}"""
    out = {}
    for name, crit, part in (("critic", True, g[:LN.N_CRITIC]), ("actor", False, g[LN.N_CRITIC:])):
        for k, v in LN.unflat_weights(part, crit).items():
            out[name + "/" + k] = v
    return out


def rel_dev(a, ref):
    """max |a - ref| / max |ref| (0 for an all-zero reference that is met exactly)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    d = np.abs(a - ref).max()
    return 0.0 if d == 0 else d / top


def header_batches():
    """(label, zero_units, batch, n_steps, seed): what the header is held to the semantics on, and the bar is measured on"""
    return (("fixture-128", False, 128, 20, 1), ("zero-units-128", True, 128, 1, 2), ("batch-1", False, 1, 1, 3),
            ("batch-5", False, 5, 1, 4))


def model(block, dtype):
    m = LN.LearnerModel(np.zeros(LN.N_ACTOR, np.float32), np.zeros(LN.N_CRITIC, np.float32), dtype=dtype, **HYPER)
    m.load_block(block)
    return m


def measure_f32_spread():
    """The figure behind HEADER_BAR: LearnerModel(float32) against LearnerModel(float64), teacher-forced along the host build's
    trajectory, worst tensor of gradients and losses -> (figure, where)"""
    worst, where = 0.0, None
    for label, zu, batch, n, seed in header_batches():
        P = host_block(nets(zu))
        rows, act7, target = minibatches(batch, n, seed=seed)
        for s in range(n):
            m32, m64 = model(P, np.float32), model(P, np.float64)
            l32, g32 = m32.step(rows[s], act7[s], target[s])
            l64, g64 = m64.step(rows[s], act7[s], target[s])
            a, b = split_grads(g32), split_grads(g64)
            for k in a:
                d = rel_dev(a[k], b[k])
                if d > worst:
                    worst, where = d, (label, s, k)
            for j, k in enumerate(("critic_loss", "actor_loss")):
                d = rel_dev(l32[j], l64[j])
                if d > worst:
                    worst, where = d, (label, s, k)
            host_step(P, rows[s], act7[s], target[s], want=False)
    return worst, where

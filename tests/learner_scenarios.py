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
#
# The scenarios of the float32 range (range_header_batches() below: subnormal gradients at s = 62 and 70, tiny input rows) are held
# to the same rule and measured by the same function.  On every tensor whose largest entry (in float64) is a NORMAL float32 the
# spread there is 2.66e-5 (critic/ln0_gamma, F-tiny-rows; 2.09e-5 at s = 62, critic/w1), the host build's own figure 4.8e-5: below
# the record above, which therefore stays the bar.  A tensor whose largest entry is itself SUBNORMAL is another matter: at N quanta
# (N x 2^-149) every rounding of its chain costs up to 1 / (2 N) of that entry, whichever order the sums take.  At s = 70 the
# critic's gradients upstream of dense_2 carry 2^-140, their tensors peak at 2 000 .. 490 000 quanta, and
# measure_f32_spread(subnormal=True) gives 9.87e-3 on critic/ln1_gamma (10 921 quanta; LearnerModel(float32) is off by 108 quanta
# there and so, to the digit, is the host build).  That figure is larger, so such tensors get a constant of their own, with the same
# factor 3; no tensor with a normal largest entry is judged by it.  The host build stays below it, so no absolute allowance is needed.
F32_SPREAD_MEASURED = 6.31e-4
HEADER_BAR = 3 * F32_SPREAD_MEASURED
F32_SPREAD_SUBNORMAL_MEASURED = 9.87e-3
SUBNORMAL_BAR = 3 * F32_SPREAD_SUBNORMAL_MEASURED
SMALLEST_NORMAL = 2.0 ** -126


def is_subnormal_tensor(ref):
    """the tensor's largest entry is a subnormal float32 (and not zero)"""
    return 0 < np.abs(np.asarray(ref, np.float64)).max() < SMALLEST_NORMAL


def header_bar(ref):
    """the bar of one tensor (or loss) of LearnerModel(float64)"""
    return SUBNORMAL_BAR if is_subnormal_tensor(ref) else HEADER_BAR


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


def header_inputs(label):
    """a label of header_batches() or range_header_batches() -> (networks, (rows, act7, target))"""
    for lab, zu, batch, n, seed in header_batches():
        if lab == label:
            return nets(zu), minibatches(batch, n, seed=seed)
    for lab, s, tiny, batch, n, seed in range_header_batches():
        if lab == label:
            inp = tiny_row_minibatches(batch, n, seed, e=tiny) if tiny else scaled_minibatches(batch, n, seed, s)
            return scaled_head(s), inp
    raise KeyError(label)


def measure_f32_spread(batches=None, subnormal=False):
    """The figure behind HEADER_BAR: LearnerModel(float32) against LearnerModel(float64), teacher-forced along the host build's
    trajectory, worst tensor of gradients and losses -> (figure, where).  batches: the labels to measure on; by default those of
    header_batches() and of range_header_batches().  subnormal: over the tensors whose largest entry is a subnormal float32 (the
    figure behind SUBNORMAL_BAR) instead of over all others."""
    worst, where = 0.0, None
    for label in batches or [b[0] for b in header_batches() + range_header_batches()]:
        networks, (rows, act7, target) = header_inputs(label)
        P = host_block(networks)
        n = len(rows)
        for s in range(n):
            m32, m64 = model(P, np.float32), model(P, np.float64)
            l32, g32 = m32.step(rows[s], act7[s], target[s])
            l64, g64 = m64.step(rows[s], act7[s], target[s])
            a, b = split_grads(g32), split_grads(g64)
            a.update(critic_loss=l32[0], actor_loss=l32[1])
            b.update(critic_loss=l64[0], actor_loss=l64[1])
            for k in a:
                d = rel_dev(a[k], b[k])
                if d > worst and is_subnormal_tensor(b[k]) == subnormal:
                    worst, where = d, (label, s, k)
            host_step(P, rows[s], act7[s], target[s], want=False)
    return worst, where


# ---------------------------------------------------------------------------------- the float32 range: families A .. F
# What the bit-for-bit statement (kernel == host build) is held to beyond the fixture's magnitudes: subnormal gradients and moments
# (A), the exactly scale-equivariant range below them (B), the state of a long run, whose beta1 power is subnormal and then sits at
# a fixed point (C), overflow to inf and NaN (D), hyper-parameters at the ends of their ranges (E) and inputs whose squares underflow
# inside the first LayerNorm (F).  tests/test_learner.py asserts on the host build that every scenario is in the regime it is named
# for; profiles/learner_range.txt keeps the counts.
QUANTUM = np.float32(2.0 ** -149)                                  # the smallest positive float32
TINY = np.float32(SMALLEST_NORMAL)                                 # the smallest positive NORMAL float32
B1P_FIXED_POINT = np.float32(4) * QUANTUM                          # where b1p *= 0.9f stays: 0.9f * 4 quanta rounds back to 4
LONG_STEPS, LONG_CALL, LONG_BATCH = 1100, 50, 2                    # family C: 22 calls of 50 minibatches of 2 rows
LONG_MOVING = 850                                                  # ... at step 850 b1p is subnormal and still moving


def is_nan_word(w):
    w = np.asarray(w, np.uint32)
    return ((w & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((w & np.uint32(0x007FFFFF)) != 0)


def same_words(a, b):
    """What "bit for bit" means once NaN occurs: the same words are NaN in both, and every other word -- infinities with their sign,
    zeros with theirs, subnormals -- is bit-equal.  A NaN's sign and payload are the one thing a correctly rounding device may have
    differently from an x86 host (whose default NaN is 0xFFC00000), and nothing reads them."""
    a, b = bits32(a), bits32(b)
    if a.shape != b.shape:
        return False
    na, nb = is_nan_word(a), is_nan_word(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def count_nan(a):
    return int(is_nan_word(bits32(a)).sum())


def count_subnormal(a):
    a = np.asarray(a, np.float32)
    return int(((a != 0) & (np.abs(a) < TINY)).sum())


SEGMENTS = ("actor", "critic", "target_actor", "target_critic", "m_actor", "v_actor", "m_critic", "v_critic", "powers", "steps", "grad")


def segments(P):
    """the block -> {segment name: view}"""
    offs = (LN.ACTOR, LN.CRITIC, LN.TARGET_ACTOR, LN.TARGET_CRITIC, LN.M_ACTOR, LN.V_ACTOR, LN.M_CRITIC, LN.V_CRITIC, LN.POWERS, LN.STEPS,
            LN.GRAD, LN.N_FLOATS)
    return {n: P[a:z] for n, a, z in zip(SEGMENTS, offs[:-1], offs[1:])}


def check_words(got, ref, what, nan_ok=False):
    """`got` (a block, losses or gradients) against the host build's.  Bit-equality; with nan_ok (family D only) same_words, else
    neither side may hold a NaN.  A block that differs is reported per segment: differing words and the first of them."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not nan_ok:
        assert count_nan(got) == 0 and count_nan(ref) == 0, "%s: NaN words: %d here, %d in the host build" % (what, count_nan(got), count_nan(ref))
    if np.array_equal(bits32(got), bits32(ref)) or (nan_ok and same_words(got, ref)):
        return
    g, r = bits32(got).ravel(), bits32(ref).ravel()
    bad = (g != r) & ~(is_nan_word(g) & is_nan_word(r)) if nan_ok else g != r
    parts = segments(np.arange(LN.N_FLOATS)) if g.size == LN.N_FLOATS else {"all": np.arange(g.size)}
    rep = {}
    for name, idx in parts.items():
        k = int(bad[idx].sum())
        if k:
            j = int(idx[np.flatnonzero(bad[idx])[0]])
            rep[name] = "%d words, first at %d (+%d): %08x, host %08x" % (k, j, j - int(idx[0]), g[j], r[j])
    raise AssertionError("%s: differs from the host build's: %s" % (what, rep))


def scaled_head(s, zero_units=False):
    """The four networks with w3 and b3 of the critic and of the target critic multiplied by 2^-s (exact in float32: asserted).  Q,
    and with scaled_minibatches the targets, dQ and the gradients of w3 / b3 then carry 2^-s, every gradient upstream 2^-2s, the
    critic loss 2^-2s.  s = 62 and 70 put thousands of gradient and second-moment words below 2^-126; s = 80 and beyond let the
    upstream gradients underflow to zero altogether, so that no bar relative to LearnerModel(float64) means anything there (the
    deviation is 1.0): s = 100 is held to bit-equality between builds and with the kernels only."""
    out = nets(zero_units)
    f = np.float32(np.ldexp(1.0, -s))
    for w in (out[1], out[3]):
        d = LN.unflat_weights(w, True)
        for k in ("w3", "b3"):
            was = d[k].copy()
            d[k] *= f
            assert np.array_equal(bits32(np.ldexp(d[k], s)), bits32(was)), (k, s)
    return out


def _scale_exact(x, e):
    y = np.ldexp(x, e).astype(np.float32)
    assert np.all(np.isfinite(y)) and np.array_equal(bits32(np.ldexp(y, -e).astype(np.float32)), bits32(x)), e
    return np.ascontiguousarray(y)


def scaled_minibatches(batch, n_batches, seed, s, wide=False):
    """the fixture minibatches with the targets multiplied by 2^-s, exactly (s = -60: family D's overflow)"""
    if wide:
        from tests import learner_wide_scenarios as W
        rows, act7, target = W.minibatches(batch, n_batches, seed=seed)
    else:
        rows, act7, target = minibatches(batch, n_batches, seed=seed)
    return rows, act7, _scale_exact(target, -s)


def tiny_row_minibatches(batch, n_batches, seed, wide=False, e=120):
    """family F: the rows of every second sample (0, 2, ..) multiplied by 2^-e: d = x - mean is of order 1e-36 there, d * d
    underflows to zero inside the input LayerNorm and rstd is 1 / sqrtf(1e-12f)."""
    rows, act7, target = scaled_minibatches(batch, n_batches, seed, 0, wide)
    rows = rows.copy()
    rows[:, ::2] = np.ldexp(rows[:, ::2], -e).astype(np.float32)          # (features that land on subnormals are rounded: fine here)
    return rows, act7, target


def underflowed_input_rows(rows):
    """family F's observable: the LayerNorm statistic `r0` (rstd of the input LayerNorm) that LearnerModel's tape exposes, in float32.
    Counts the rows that are not constant and whose rstd is nevertheless exactly 1 / sqrt(1e-12f): every d * d of such a row
    underflowed to zero (or to a subnormal that 1e-12f absorbs; either way the products left the normal range)."""
    w = LN.unflat_weights(fixture().critic, True)
    x = np.asarray(rows, np.float32).reshape(-1, 28)
    r0 = LN.net_forward(w, x, np.zeros((len(x), 7), np.float32), np.float32)["r0"][:, 0]
    d = x - x.mean(axis=1, keepdims=True, dtype=np.float32)
    small = np.abs(d).max(axis=1)
    return int(((small > 0) & (small * small < TINY) & (r0 == np.float32(1.0) / np.sqrt(np.float32(1e-12)))).sum())


# name -> what the case is.  s: scaled_head / scaled_minibatches; warmed: the start has taken 5 steps of batch 32 (A: on the scaled
# problem itself; E: warmed_block); long: the start is the block after that many steps of family C; nan_ok: family D alone.
# (batch, minibatches, seed) are those of Learner.step; the wide step runs the same cases at batches of 130 and 300.
RANGE_CASES = {
    "A-s62": dict(s=62, batch=65, n=3, seed=5), "A-s62-warmed": dict(s=62, warmed=True, batch=65, n=3, seed=5),
    "A-s70": dict(s=70, batch=65, n=3, seed=5), "A-s70-warmed": dict(s=70, warmed=True, batch=65, n=3, seed=5),
    "A-s100": dict(s=100, batch=65, n=3, seed=5), "A-s100-warmed": dict(s=100, warmed=True, batch=65, n=3, seed=5),
    "C-step850": dict(long=LONG_MOVING, batch=65, n=3, seed=6), "C-step1100": dict(long=LONG_STEPS, batch=65, n=3, seed=6),
    "D-overflow": dict(s=-60, head=False, batch=65, n=2, seed=8, nan_ok=True),
    "E-epsilon-1e-40": dict(zero_units=True, warmed=True, batch=37, n=3, seed=5, hyper=dict(epsilon=1e-40)),
    "E-tau-0": dict(warmed=True, batch=37, n=3, seed=5, hyper=dict(tau=0.0)),
    "E-tau-1": dict(warmed=True, batch=37, n=3, seed=5, hyper=dict(tau=1.0)),
    "E-beta1-0": dict(warmed=True, batch=37, n=3, seed=5, hyper=dict(beta1=0.0)),
    "E-lr-0-1": dict(warmed=True, batch=37, n=3, seed=5, hyper=dict(actor_lr=0.0, critic_lr=1.0)),
    "F-tiny-rows": dict(tiny=120, batch=65, n=2, seed=9),
}


def range_case(name):
    c = dict(s=0, head=True, zero_units=False, warmed=False, long=0, tiny=0, nan_ok=False, hyper={})
    c.update(RANGE_CASES[name])
    c["family"] = name[0]
    c["hyper"] = dict(HYPER, **c["hyper"])
    return c


def range_networks(name):
    c = range_case(name)
    return scaled_head(c["s"] if c["head"] else 0, c["zero_units"])


def range_inputs(name, batch=None, wide=False):
    """the minibatches of a case (at the case's own batch, or at `batch`; wide: drawn as learner_wide_scenarios draws them)"""
    c = range_case(name)
    batch = batch or c["batch"]
    if c["tiny"]:
        return tiny_row_minibatches(batch, c["n"], c["seed"], wide, c["tiny"])
    return scaled_minibatches(batch, c["n"], c["seed"], c["s"], wide)


@functools.lru_cache(maxsize=None)
def range_start(name):
    """the block a case starts from; read-only"""
    c = range_case(name)
    if c["long"]:
        P = long_run()[c["long"]].copy()
    elif c["warmed"] and c["family"] == "A":
        # warmed_block's 5 steps of batch 32, on the scaled problem itself, with critic_lr = 0: moments and powers move, the critic
        # stays.  With the reference's critic_lr Adam's step on w3 is lr g / epsilon, some 1e5 times the scaled head itself, the
        # critic loss grows 1e11-fold per step and after 5 steps nothing is subnormal any more (measured: 0 words at s = 62, 70 and
        # 100, and a flushing build was bit-equal there: such a start tests nothing of this family).
        P = host_block(range_networks(name))
        host_step(P, *scaled_minibatches(32, 5, 77, c["s"]), want=False, critic_lr=0.0)
    elif c["warmed"]:
        P = warmed_block(c["zero_units"]).copy()
    else:
        P = host_block(range_networks(name))
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def range_run(name, lib=None):
    """the host build (lib: another library name) on a case -> (inputs, block after, losses, grads); computed once, read-only"""
    c = range_case(name)
    P = range_start(name).copy()
    inp = range_inputs(name)
    losses, grads = host_step(P, *inp, lib=shim(lib) if lib else None, **c["hyper"])
    for a in inp + (P, losses, grads):
        a.setflags(write=False)
    return inp, P, losses, grads


@functools.lru_cache(maxsize=None)
def long_run_inputs():
    inp = minibatches(LONG_BATCH, LONG_STEPS, seed=9)
    for a in inp:
        a.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def long_run(call=LONG_CALL, lib=None):
    """family C on the host build: LONG_STEPS steps of batch 2 from the fixture networks in calls of `call` minibatches ->
    {steps taken: block} after every call; read-only"""
    rows, act7, target = long_run_inputs()
    P = host_block(nets())
    out = {}
    for a in range(0, LONG_STEPS, call):
        host_step(P, rows[a:a + call], act7[a:a + call], target[a:a + call], want=False, lib=shim(lib) if lib else None)
        out[min(a + call, LONG_STEPS)] = P.copy()
        out[min(a + call, LONG_STEPS)].setflags(write=False)
    return out


def range_header_batches():
    """(label, s, exponent of the tiny rows, batch, n_steps, seed): the scenarios of the float32 range on which the host build is ALSO held to
    LearnerModel(float64) by HEADER_BAR, and on which measure_f32_spread() measures beside header_batches().  s = 62 and 70: the
    subnormal gradients of family A (one step each from the scaled networks); tiny rows: family F.  Not s = 80, 100: see
    scaled_head()."""
    return (("A-s62", 62, False, 65, 1, 5), ("A-s70", 70, False, 65, 1, 5), ("F-tiny-rows", 0, 120, 65, 1, 9))

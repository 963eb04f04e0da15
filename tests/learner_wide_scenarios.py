"""Inputs and the host build of the WIDE learner step (csrc/pve_learn.h learn_steps_wide; tests/learner_wide_host) shared by
tests/test_learner_wide.py and tests/test_gpu_learner_wide.py.  Networks, warmed blocks and the fixture are those of
tests/learner_scenarios.py; only the minibatches are drawn here, because a wide batch is larger than the fixture (drawn with
replacement then) and every SLICE of it carries the fixture's all-zero rows."""
import ctypes as C
import functools

import numpy as np

from pve_mcc_amd import learner as LN
from tests import learner_scenarios as S
from tests import native

SLICE, ROW = LN.SLICE, LN.WIDE_ROW
ROW_CRITIC, ROW_ACTOR, ROW_LOSS = 0, 6844, 13240          # a slice's row of the workspace (csrc/pve_learn.h LW_*)

# ---------------------------------------------------------------------------------- the bar of "the wide header against the semantics"
# Built as learner_scenarios.HEADER_BAR is: the wide host build's gradients and losses are compared with LearnerModel(float64) on the
# same float32 inputs, per tensor, with learner_scenarios.rel_dev; the bar is THREE times the largest such figure of
# LearnerModel(float32) against LearnerModel(float64) over wide_batches() below (batches of 129, 300 and 1 024 rows, 5 teacher-forced
# steps each along the wide host build's trajectory from the fixture weights).  Measured by measure_f32_spread_wide(): 2.71e-4
# (recorded rounded to 2.70e-4), on the critic's dense_2 bias gradient (critic/b3) at step 4 of the 300-row run -- the same tensor
# that sets HEADER_BAR, 2 mean(Q - target), a sum that cancels as the bias settles; the wide host build's own figure against float64
# on the same batches is 8.1e-5 (actor/ln0_gamma, step 1 of the 1 024-row run).
F32_SPREAD_WIDE_MEASURED = 2.70e-4
WIDE_BAR = 3 * F32_SPREAD_WIDE_MEASURED


def shim(name="liblearner_wide_host.so"):
    """learn_steps_wide compiled by g++ (tests/learner_wide_host), built and loaded by tests/native.py.
    "liblearner_wide_host_sub.so" is the same header with sub-blocks of 7 / 5 rows instead of 64 / 32."""
    return native.load("learner_wide_host", name, _signatures)


def _signatures(L):
    vp = C.c_void_p
    L.learner_wide_host_layout.restype = None
    L.learner_wide_host_layout.argtypes = [vp]
    L.learner_wide_host_step.restype = None
    L.learner_wide_host_step.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.learner_wide_host_partials.restype = C.c_int
    L.learner_wide_host_partials.argtypes = [vp]
    return L


def n_slices(batch):
    return (batch + SLICE - 1) // SLICE


def minibatches(batch, n_batches, seed=0, zero_rows=True):
    """(rows [n, batch, 28], act7 [n, batch, 7], target [n, batch]) drawn from the fixture, with replacement where it has fewer rows
    than the batch; with zero_rows every slice of 3 rows or more holds the fixture's all-zero rows (at its positions 1 and last)."""
    f = S.fixture()
    r = np.random.default_rng(5000 + seed)
    idx = np.stack([r.choice(len(f.rows), batch, replace=batch > len(f.rows)) for _ in range(n_batches)])
    if zero_rows:
        for s in range(n_slices(batch)):
            a, z = s * SLICE, min(batch, s * SLICE + SLICE)
            if z - a >= 3:
                idx[:, a + 1], idx[:, z - 1] = f.zero_rows[0], f.zero_rows[1]
    return np.ascontiguousarray(f.rows[idx]), np.ascontiguousarray(f.act7[idx]), np.ascontiguousarray(f.target[idx])


def host_step_wide(P, rows, act7, target, critic_only=False, want=True, lib=None, **hyper):
    """pve_learner_step_wide of the host build, in place on P -> (losses [n, 2], grads [n, 13234]) (None with want=False)"""
    rows, act7, target = (np.ascontiguousarray(x, np.float32) for x in (rows, act7, target))
    if rows.ndim == 2:
        rows, act7, target = rows[None], act7[None], target[None]
    n, B = rows.shape[:2]
    assert act7.shape == (n, B, 7) and target.shape == (n, B) and P.dtype == np.float32 and P.size == LN.N_FLOATS
    losses = np.zeros((n, 2), np.float32) if want else None
    grads = np.zeros((n, LN.N_GRADS), np.float32) if want else None
    h = S.hyper_array(**hyper)
    (lib or shim()).learner_wide_host_step(S._ptr(P), S._ptr(h), LN.CRITIC_ONLY if critic_only else 0, S._ptr(rows), S._ptr(act7),
                                           S._ptr(target), B, n, S._ptr(losses), S._ptr(grads))
    return losses, grads


def partial_rows(lib=None):
    """the per-slice rows of the workspace after the latest step of the latest host_step_wide -> float32 [n_slices, ROW]"""
    lib = lib or shim()
    out = np.zeros((lib.learner_wide_host_partials(None), ROW), np.float32)
    assert lib.learner_wide_host_partials(S._ptr(out)) == out.shape[0]
    return out


def combine(parts):
    """the stated combine on float32 [n_slices, k]: acc = p[0]; acc = acc + p[s], slices ascending -> float32 [k]"""
    parts = np.asarray(parts)
    assert parts.dtype == np.float32
    acc = parts[0].copy()
    for s in range(1, parts.shape[0]):
        acc = acc + parts[s]
    assert acc.dtype == np.float32
    return acc


@functools.lru_cache(maxsize=None)
def host_run(bsz, n, warmed, zero_units, critic_only=False):
    """the wide host build on the scenario's minibatches -> (inputs, block after, losses, grads); computed once, read-only"""
    P = S.warmed_block(zero_units).copy() if warmed else S.host_block(S.nets(zero_units))
    inp = minibatches(bsz, n, seed=7 * bsz + n)
    losses, grads = host_step_wide(P, *inp, critic_only=critic_only)
    for a in inp + (P, losses, grads):
        a.setflags(write=False)
    return inp, P, losses, grads


@functools.lru_cache(maxsize=None)
def range_run(name, bsz, lib=None):
    """the wide host build (lib: another library name) on a case of learner_scenarios.RANGE_CASES at a batch of bsz rows: the
    case's networks, start block, hyper-parameters and number of minibatches, the minibatches drawn as minibatches() above draws
    them -> (inputs, block after, losses, grads); computed once, read-only"""
    c = S.range_case(name)
    P = S.range_start(name).copy()
    inp = S.range_inputs(name, bsz, wide=True)
    losses, grads = host_step_wide(P, *inp, lib=shim(lib) if lib else None, **c["hyper"])
    for a in inp + (P, losses, grads):
        a.setflags(write=False)
    return inp, P, losses, grads


def wide_batches():
    """(batch, n_steps, seed): what the wide header is held to the semantics on, and its bar is measured on"""
    return ((129, 5, 11), (300, 5, 12), (1024, 5, 13))


def measure_f32_spread_wide():
    """The figure behind WIDE_BAR: LearnerModel(float32) against LearnerModel(float64), teacher-forced along the wide host build's
    trajectory, worst tensor of gradients and losses -> (figure, where)"""
    worst, where = 0.0, None
    for batch, n, seed in wide_batches():
        P = S.host_block(S.nets())
        rows, act7, target = minibatches(batch, n, seed=seed)
        for s in range(n):
            l32, g32 = S.model(P, np.float32).step(rows[s], act7[s], target[s])
            l64, g64 = S.model(P, np.float64).step(rows[s], act7[s], target[s])
            a, b = S.split_grads(g32), S.split_grads(g64)
            for k in a:
                d = S.rel_dev(a[k], b[k])
                if d > worst:
                    worst, where = d, (batch, s, k)
            for j, k in enumerate(("critic_loss", "actor_loss")):
                d = S.rel_dev(l32[j], l64[j])
                if d > worst:
                    worst, where = d, (batch, s, k)
            host_step_wide(P, rows[s], act7[s], target[s], want=False)
    return worst, where

"""The wide learner step (csrc/pve_learn.h learn_steps_wide, pve_learner_step_wide) without a GPU, on a g++ build of the header
(tests/learner_wide_host):
  1. a batch of one slice (<= 128 rows) is learn_steps, bit for bit;
  2. beyond that the combine is the stated one: a NumPy float32 `acc = p[0]; acc = acc + p[s]` over the per-slice rows gives the
     gradients and the loss sums, and Adam's NumPy restatement gives the block from them;
  3. no bit depends on the sub-block sizes;
  4. gradients and losses follow LearnerModel(float64) to a bar built like learner_scenarios.HEADER_BAR;
  5. the C ABI's argument checks, through the CPU emulators, which have no learner kernels and say so.
The kernels against this host build: tests/test_gpu_learner_wide.py."""
import ctypes as C

import numpy as np
import pytest

from pve_mcc_amd import _capi
from pve_mcc_amd import learner as LN
from tests import learner_scenarios as S
from tests import learner_wide_scenarios as W
from tests.hip_adapter import emulator_lib, make_batch


def test_layout_is_the_headers():
    out = np.zeros(8, np.int32)
    W.shim().learner_wide_host_layout(S._ptr(out))
    assert out.tolist()[:7] == [LN.SLICE, LN.WIDE_ROW, W.ROW_CRITIC, W.ROW_ACTOR, W.ROW_LOSS, 64, 32]
    W.shim("liblearner_wide_host_sub.so").learner_wide_host_layout(S._ptr(out))
    assert out.tolist()[5:7] == [7, 5]
    # (_capi's LEARN_SLICE and LEARNER_WIDE_ROW against the header's macros: tests/test_binding_contract.py)
    assert (LN.SLICE, LN.WIDE_ROW) == (_capi.LEARN_SLICE, _capi.LEARNER_WIDE_ROW)
    assert LN.WIDE_ROW % 4 == 0 and LN.WIDE_ROW == 6844 + 6396 + 4
    assert [LN.wide_floats(b) for b in (1, 128, 129, 256, 257)] == [LN.WIDE_ROW * k for k in (1, 1, 2, 2, 3)]


@pytest.mark.parametrize("library", ["liblearner_wide_host.so", "liblearner_wide_host_sub.so"])
def test_host_build_is_stale_after_any_file_it_reads(library):
    """tests/learner_wide_host/Makefile keeps the rule of tests/native.mk (tests/test_native_build.py, which lists the older
    directories): the library is rebuilt after a change of any file its translation unit reads"""
    from tests import test_native_build as NB
    NB.test_library_is_stale_after_any_file_it_reads("learner_wide_host", library, library)


# ------------------------------------------------------------------ 1. one slice is the existing definition
@pytest.mark.parametrize("critic_only", [False, True])
@pytest.mark.parametrize("warmed,zero_units", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("bsz", [1, 5, 64, 127, 128])
def test_one_slice_is_learn_steps(bsz, warmed, zero_units, critic_only):
    inp = S.minibatches(bsz, 3, seed=90 + bsz)
    P1 = S.warmed_block(zero_units).copy() if warmed else S.host_block(S.nets(zero_units))
    P2 = P1.copy()
    l1, g1 = S.host_step(P1, *inp, critic_only=critic_only)
    l2, g2 = W.host_step_wide(P2, *inp, critic_only=critic_only)
    assert np.array_equal(S.bits32(l1), S.bits32(l2)) and np.array_equal(S.bits32(g1), S.bits32(g2))
    assert np.array_equal(S.bits32(P1), S.bits32(P2))
    assert np.all(np.isfinite(P2)) and int(P2[LN.STEPS:LN.STEPS + 1].view(np.int32)[0]) == 3 + (5 if warmed else 0)


# ------------------------------------------------------------------ 2. the combine is the stated one
@pytest.mark.parametrize("critic_only", [False, True])
@pytest.mark.parametrize("bsz", [129, 300, 449])
def test_combine_is_the_stated_one(bsz, critic_only):
    h = S.HYPER
    P = S.warmed_block().copy()
    before = P.copy()
    rows, act7, target = W.minibatches(bsz, 1, seed=bsz)
    losses, grads = W.host_step_wide(P, rows, act7, target, critic_only=critic_only)
    parts = W.partial_rows()
    assert parts.shape == (W.n_slices(bsz), W.ROW)
    gc = W.combine(parts[:, W.ROW_CRITIC:W.ROW_CRITIC + LN.N_CRITIC])
    assert np.array_equal(S.bits32(gc), S.bits32(grads[0, :LN.N_CRITIC]))
    assert np.array_equal(S.bits32(gc), S.bits32(P[LN.GRAD:LN.GRAD + LN.N_CRITIC]))
    sums = W.combine(parts[:, W.ROW_LOSS:W.ROW_LOSS + 2])
    assert np.array_equal(S.bits32(sums[0] / np.float32(bsz)), S.bits32(losses[0, 0]))
    if critic_only:
        ga = np.zeros(LN.N_ACTOR, np.float32)
        assert np.all(np.isnan(parts[:, W.ROW_ACTOR:W.ROW_LOSS])) and np.isnan(sums[1])        # the actor pass never ran
        assert np.array_equal(S.bits32(losses[0, 1]), S.bits32(np.float32(0)))
        assert np.array_equal(S.bits32(P[LN.GRAD_ACTOR:LN.GRAD_ACTOR + 6396]), S.bits32(before[LN.GRAD_ACTOR:LN.GRAD_ACTOR + 6396]))
    else:
        ga = W.combine(parts[:, W.ROW_ACTOR:W.ROW_ACTOR + LN.N_ACTOR])
        assert np.array_equal(S.bits32(-(sums[1] / np.float32(bsz))), S.bits32(losses[0, 1]))
        assert np.array_equal(S.bits32(ga), S.bits32(P[LN.GRAD_ACTOR:LN.GRAD_ACTOR + LN.N_ACTOR]))
    assert np.array_equal(S.bits32(ga), S.bits32(grads[0, LN.N_CRITIC:]))
    # a slice's partial is not the whole sum: the combine did add something
    assert W.n_slices(bsz) > 1 and not np.array_equal(S.bits32(parts[0, :LN.N_CRITIC]), S.bits32(gc))
    # the block from the combined gradients: Adam and the soft update, restated in NumPy float32
    seg = {"critic": (LN.CRITIC, LN.TARGET_CRITIC, LN.M_CRITIC, LN.V_CRITIC, LN.POWERS + 2, LN.N_CRITIC, h["critic_lr"], gc),
           "actor": (LN.ACTOR, LN.TARGET_ACTOR, LN.M_ACTOR, LN.V_ACTOR, LN.POWERS, LN.N_ACTOR, h["actor_lr"], ga)}
    for net, (ow, ot, om, ov, op, n, lr, g) in seg.items():
        if net == "actor" and critic_only:
            for o, k in ((ow, n), (ot, n), (om, n), (ov, n), (op, 2)):
                assert np.array_equal(S.bits32(P[o:o + k]), S.bits32(before[o:o + k]))
            continue
        w, m, v, b1p, b2p = LN.adam_update(before[ow:ow + n], before[om:om + n], before[ov:ov + n], g, lr, before[op], before[op + 1],
                                           h["beta1"], h["beta2"], h["epsilon"], np.float32)
        tgt = LN.soft_update(w, before[ot:ot + n], h["tau"], np.float32)
        for name, got, ref in (("w", P[ow:ow + n], w), ("m", P[om:om + n], m), ("v", P[ov:ov + n], v), ("target", P[ot:ot + n], tgt),
                               ("powers", P[op:op + 2], np.array([b1p, b2p], np.float32))):
            assert ref.dtype == np.float32 and np.array_equal(S.bits32(got), S.bits32(ref)), (net, name)
    assert int(P[LN.STEPS:LN.STEPS + 1].view(np.int32)[0]) == 6


def test_a_wide_batch_is_another_order_than_learn_steps():
    """what the documents say: beyond 128 rows the wide step is NOT learn_steps bit for bit (a different, fixed order), though the
    same step within float32 rounding"""
    inp = W.minibatches(300, 1, seed=3)
    P1, P2 = S.host_block(S.nets()), S.host_block(S.nets())
    l1, g1 = S.host_step(P1, *inp)
    l2, g2 = W.host_step_wide(P2, *inp)
    assert not np.array_equal(S.bits32(g1), S.bits32(g2))
    for k, v in S.split_grads(g1[0]).items():
        assert S.rel_dev(S.split_grads(g2[0])[k], v) <= W.WIDE_BAR, k


def test_steps_in_one_call_equal_single_calls():
    rows, act7, target = W.minibatches(300, 3, seed=5)
    P1, P2 = S.warmed_block().copy(), S.warmed_block().copy()
    l1, g1 = W.host_step_wide(P1, rows, act7, target)
    for s in range(3):
        l2, g2 = W.host_step_wide(P2, rows[s], act7[s], target[s])
        assert np.array_equal(S.bits32(l1[s]), S.bits32(l2[0])) and np.array_equal(S.bits32(g1[s]), S.bits32(g2[0]))
    assert np.array_equal(S.bits32(P1), S.bits32(P2))


# ------------------------------------------------------------------ 3. no dependence on the sub-block sizes
@pytest.mark.parametrize("bsz", [129, 300, 1024])
def test_sub_block_sizes_change_no_bit(bsz):
    sub = W.shim("liblearner_wide_host_sub.so")
    rows, act7, target = W.minibatches(bsz, 2, seed=50 + bsz)
    P1, P2 = S.warmed_block(True).copy(), S.warmed_block(True).copy()
    l1, g1 = W.host_step_wide(P1, rows, act7, target)
    p1 = W.partial_rows()
    l2, g2 = W.host_step_wide(P2, rows, act7, target, lib=sub)
    p2 = W.partial_rows(sub)
    assert np.array_equal(S.bits32(l1), S.bits32(l2)) and np.array_equal(S.bits32(g1), S.bits32(g2))
    assert np.array_equal(S.bits32(P1), S.bits32(P2))
    used = np.r_[0:LN.N_CRITIC, W.ROW_ACTOR:W.ROW_ACTOR + LN.N_ACTOR, W.ROW_LOSS:W.ROW_LOSS + 2]
    assert np.array_equal(S.bits32(p1[:, used]), S.bits32(p2[:, used])) and np.all(np.isfinite(p1[:, used]))


# ------------------------------------------------------------------ 3b. the float32 range (learner_scenarios: families A .. F)
WIDE_SUB = "liblearner_wide_host_sub.so"


def test_long_run_state_in_calls_and_across_builds():
    """family C for the wide build: 40 steps of 130 rows (two slices, the second of 2 rows) from the state of step 850 of the long
    run, where b1p is subnormal and still moving: one call == calls of 10 == the sub-block build"""
    start = S.long_run()[S.LONG_MOVING]
    rows, act7, target = W.minibatches(130, 40, seed=17)
    blocks = []
    for call, lib in ((40, None), (10, None), (40, W.shim(WIDE_SUB))):
        P = start.copy()
        for a in range(0, 40, call):
            W.host_step_wide(P, rows[a:a + call], act7[a:a + call], target[a:a + call], want=False, lib=lib)
        blocks.append(P)
    P = blocks[0]
    print("wide, steps 850 .. 890: b1p %.6e -> %.6e" % (start[LN.POWERS], P[LN.POWERS]))
    assert S.B1P_FIXED_POINT < P[LN.POWERS] < start[LN.POWERS] < S.TINY and np.all(np.isfinite(P))
    assert int(P[LN.STEPS:LN.STEPS + 1].view(np.int32)[0]) == S.LONG_MOVING + 40
    assert np.array_equal(S.bits32(blocks[1]), S.bits32(P)) and np.array_equal(S.bits32(blocks[2]), S.bits32(P))


@pytest.mark.parametrize("name", list(S.RANGE_CASES))
def test_range_cases_keep_their_words_across_builds(name):
    """every case of the range at 130 rows: finite (D: NaN and infinities, compared by same_words), and the same words from the
    sub-block build; family A keeps its thousands of subnormal words at this batch"""
    c = S.range_case(name)
    _, P, losses, grads = W.range_run(name, 130)
    _, P2, l2, g2 = W.range_run(name, 130, lib=WIDE_SUB)
    for what, a, b in (("block", P, P2), ("losses", losses, l2), ("grads", grads, g2)):
        S.check_words(a, b, "%s, %s of the sub-block build" % (name, what), nan_ok=c["nan_ok"])
    if c["nan_ok"]:
        assert losses[0, 0] == np.inf and S.count_nan(P) >= 1 and int(np.isinf(P).sum()) >= 1
    else:
        assert np.all(np.isfinite(P)) and np.all(np.isfinite(grads)) and np.all(np.isfinite(losses))
    if c["family"] == "A":
        n = S.count_subnormal(grads) + S.count_subnormal(P[:LN.STEPS])
        print("%s at 130 rows: %d subnormal words in the gradients and the block" % (name, n))
        assert n >= 1000


# ------------------------------------------------------------------ 4. the wide header against the semantics
def test_recorded_spread_is_current():
    """The figure behind the bar, measured again: the float32 model's spread stays below the bar derived from the record"""
    worst, where = W.measure_f32_spread_wide()
    print("LearnerModel(float32) against float64 on the wide batches: %.3e at %s (recorded %.3e)" % (worst, where, W.F32_SPREAD_WIDE_MEASURED))
    assert worst <= W.WIDE_BAR


@pytest.mark.parametrize("batch,n_steps,seed", W.wide_batches())
def test_wide_host_build_follows_the_model(batch, n_steps, seed):
    """Teacher forcing as in tests/test_learner.py: before every step the model takes the host build's whole state; gradients (per
    tensor) and losses within WIDE_BAR of LearnerModel(float64)."""
    P = S.host_block(S.nets())
    rows, act7, target = W.minibatches(batch, n_steps, seed=seed)
    worst, where = 0.0, None
    for s in range(n_steps):
        l64, g64 = S.model(P, np.float64).step(rows[s], act7[s], target[s])
        lh, gh = W.host_step_wide(P, rows[s], act7[s], target[s])
        got, ref = S.split_grads(gh[0]), S.split_grads(g64)
        for k in got:
            d = S.rel_dev(got[k], ref[k])
            if d > worst:
                worst, where = d, (s, k)
            assert d <= W.WIDE_BAR, (batch, s, k, d)
        for j in range(2):
            d = S.rel_dev(lh[0][j], l64[j])
            if d > worst:
                worst, where = d, (s, "loss %d" % j)
            assert d <= W.WIDE_BAR, (batch, s, "loss", j, d)
        assert int(P[LN.STEPS:LN.STEPS + 1].view(np.int32)[0]) == s + 1
    print("batch %d: wide host build against LearnerModel(float64), worst tensor %.3e at %s (bar %.3e)" % (batch, worst, where, W.WIDE_BAR))


# ------------------------------------------------------------------ 5. the C ABI on a backend without the kernels
def test_entry_point_on_the_emulator():
    from pve_mcc_amd.arrivals import synthetic_arrivals
    lib = emulator_lib()
    assert "pve_learner_step_wide" in _capi.EXPORTS and hasattr(lib, "pve_learner_step_wide") and lib.pve_abi_version() == _capi.ABI_VERSION
    b = make_batch(synthetic_arrivals(2, rate=500.0, horizon_s=20.0, seed=1), 2, 64, "emu", outputs=("obs_post", "flags"))
    keep = []

    def P(n, off=0):
        raw = np.zeros(n * 4 + 32, np.uint8)
        keep.append(raw)
        return raw.ctypes.data + (-raw.ctypes.data) % 16 + off

    batch, nb = 200, 3                                      # two slices
    need = LN.wide_floats(batch)
    assert need == 2 * LN.WIDE_ROW
    params = P(LN.N_FLOATS)
    rows, act7, target, losses, grads = P(nb * batch * 28), P(nb * batch * 7), P(nb * batch), P(nb * 2), P(nb * LN.N_GRADS)
    work = P(need)

    def lr(**kw):
        r = _capi.PveLearner()
        r.params, r.flags, r.block_threads = params, 0, 0
        for k, v in S.HYPER.items():
            setattr(r, k, v)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def step(r=None, h=b._h, inp=(rows, act7, target), batch=batch, nb=nb, work=work, floats=need, groups=0, out=(losses, grads)):
        return lib.pve_learner_step_wide(h, C.byref(r) if r is not None else None, *inp, batch, nb, work, floats, groups, *out)

    inf, nan = float("inf"), float("nan")
    # every check shared with pve_learner_step
    shared = [(dict(params=None), b"null params"), (dict(params=params + 4), b"aligned"), (dict(actor_lr=inf), b"finite"),
              (dict(actor_lr=nan), b"finite"), (dict(critic_lr=-inf), b"finite"), (dict(critic_lr=nan), b"finite"),
              (dict(epsilon=nan), b"finite"), (dict(epsilon=inf), b"finite"), (dict(tau=nan), b"finite"), (dict(tau=inf), b"finite"),
              (dict(tau=-0.001), b"tau"), (dict(tau=1.001), b"tau"), (dict(beta1=1.0), b"beta"), (dict(beta2=-0.5), b"beta"),
              (dict(beta1=nan), b"beta"), (dict(flags=2), b"flags"), (dict(block_threads=100), b"block_threads"),
              (dict(block_threads=2048), b"block_threads"), (dict(block_threads=-64), b"block_threads")]
    for kw, word in shared:
        assert step(lr(**kw)) == -1 and word in lib.pve_last_error() and b"pve_learner_step_wide" in lib.pve_last_error(), (kw, lib.pve_last_error())
    for fn in (lambda: step(lr(), h=None), lambda: step(None)):
        assert fn() == -1 and b"null" in lib.pve_last_error()
    for kw, word in ((dict(inp=(None, act7, target)), b"null rows"), (dict(inp=(rows, None, target)), b"null rows"),
                     (dict(inp=(rows, act7, None)), b"null rows"), (dict(batch=0), b"batch"), (dict(batch=-3), b"batch"),
                     (dict(nb=0), b"n_batches"), (dict(nb=-1), b"n_batches"), (dict(batch=1 << 20, nb=1 << 12), b"n_batches"),
                     (dict(inp=(rows + 4, act7, target)), b"aligned"), (dict(inp=(rows, act7 + 2, target)), b"aligned"),
                     (dict(inp=(rows, act7, target + 1)), b"aligned"), (dict(out=(losses + 2, grads)), b"aligned"),
                     (dict(out=(losses, grads + 3)), b"aligned"),
                     # the wide step's own
                     (dict(work=None), b"null work"), (dict(work=work + 4), b"work must be 16-byte aligned"),
                     (dict(work=work + 8), b"work must be 16-byte aligned"), (dict(floats=need - 1), b"work_floats"),
                     (dict(floats=LN.WIDE_ROW), b"work_floats"), (dict(floats=0), b"work_floats"), (dict(floats=-need), b"work_floats"),
                     (dict(batch=129, floats=LN.WIDE_ROW), b"work_floats"), (dict(groups=-1), b"groups"), (dict(groups=-(1 << 31)), b"groups")):
        assert step(lr(), **kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    # valid arguments: no learner kernels here, and the library says so (optional pointers NULL, the extremes of every range)
    for fn in (lambda: step(lr()), lambda: step(lr(), out=(None, None)), lambda: step(lr(), floats=need + 1, groups=1),
               lambda: step(lr(), groups=(1 << 31) - 1), lambda: step(lr(), batch=128, floats=LN.WIDE_ROW),
               lambda: step(lr(flags=1, block_threads=1024, tau=0.0), batch=1, nb=1, floats=LN.WIDE_ROW),
               lambda: step(lr(tau=1.0, beta1=0.0, block_threads=64), inp=(rows, act7 + 4, target + 4))):
        assert fn() == -1 and b"pve_learner_step_wide: this backend has no learner kernels" in lib.pve_last_error(), lib.pve_last_error()
    assert not any(np.any(raw) for raw in keep)                   # nothing was written


@pytest.mark.parametrize("which", ["emu", "emu_wide", "emu_diag"])
def test_every_emulator_refuses(which):
    """each CPU emulator exports the symbol, validates, and refuses valid calls with PVE_ERR_INVALID"""
    from pve_mcc_amd.arrivals import synthetic_arrivals
    from pve_mcc_amd.batched import BatchedIntersections
    from tests import rank_pairs_scenarios, test_capacity256
    lib = {"emu": emulator_lib, "emu_wide": test_capacity256.wide_lib, "emu_diag": rank_pairs_scenarios.diag_emulator_lib}[which]()
    assert hasattr(lib, "pve_learner_step_wide")
    b = BatchedIntersections(1, 64, synthetic_arrivals(1, rate=500.0, horizon_s=20.0, seed=1), device="cpu", outputs=("obs_post",), _lib=lib)
    raw = np.zeros(LN.N_FLOATS * 4 + 32, np.uint8)
    p = raw.ctypes.data + (-raw.ctypes.data) % 16
    r = _capi.PveLearner()
    r.params = p
    for k, v in S.HYPER.items():
        setattr(r, k, v)
    assert lib.pve_learner_step_wide(b._h, C.byref(r), p, p, p, 4, 2, p, LN.WIDE_ROW, 0, None, None) == -1 \
        and b"backend has no learner kernels" in lib.pve_last_error()
    assert lib.pve_learner_step_wide(b._h, C.byref(r), p, p, p, 4, 2, p, LN.WIDE_ROW - 1, 0, None, None) == -1 and b"work_floats" in lib.pve_last_error()
    assert lib.pve_learner_step_wide(b._h, C.byref(r), p, p, p, 4, 2, None, LN.WIDE_ROW, 0, None, None) == -1 and b"null work" in lib.pve_last_error()
    assert not np.any(raw)                                        # nothing was written

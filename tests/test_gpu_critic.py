"""The critic and the bootstrap Q on the GPU (pve_set_target_networks / pve_critic_forward / pve_bootstrap_q; csrc/pve_critic.h)
against the reference's own graph (tests/golden/critic_graph.npz).

Bars (none of them taken from what the kernels return):
  Q alone:    3 x spread_critic.  spread_critic = max |graph float32 - graph float64| on the fixture's rows (3.06e-4): two float32
              evaluations in different orders each lie within one spread of the real value, the third spread is for the 2^-22
              split-half operands.
  bootstrap:  3 x spread_critic + sens x ACTION_TOL.  ACTION_TOL (5e-4) is the action error the project already accepts for the
              device actor; sens = max sum_k |dQ/da_k| of the reference's target critic (15.6) pushes it through to Q.
Every test prints the maximum it measured before it asserts.

Section 6 runs k_target_q beyond one 64-row chunk per wave (the pending ring across chunks; tests/target_q_walk.py is the host
model of that walk and builds the inputs, tests/test_target_q_walk.py shows on the CPU that they reach the ring's paths)."""
import numpy as np
import pytest
import torch

from oracle.actor_np import flat_weights
from pve_mcc_amd import _capi, critic
from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import actor_scenarios as A
from tests import target_q_walk as TQ
from tests.critic_scenarios import load_critic_golden
from tests.hip_adapter import _np, make_batch

pytestmark = pytest.mark.gpu
ACTION_TOL = A.ACTION_TOL
ROW_COUNTS = (1, 31, 32, 33, 65, 4 * 64 + 1)
DTYPES = (torch.float32, torch.float64)
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")


def q_bar(g):
    return 3.0 * g.spread_critic


def boot_bar(g):
    return 3.0 * g.spread_critic + g.sens * ACTION_TOL


def bits32(x):
    return np.ascontiguousarray(_np(x) if torch.is_tensor(x) else x, np.float32).view(np.uint32)


_batches = {}


def batch(obs_dtype, target="target_critic"):
    """One small batch per row type with the fixture's target networks installed (shared: the calls under test are stateless)"""
    key = (obs_dtype, target)
    if key not in _batches:
        g = load_critic_golden()
        arr = synthetic_arrivals(4, rate=1000.0, horizon_s=60.0, seed=5)
        b = make_batch(arr, 4, 128, "hip", outputs=("obs_post", "reward", "flags", "env_out"), obs_dtype=obs_dtype)
        b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights[target])
        _batches[key] = b
    return _batches[key]


def pick(n_total, n):
    """n row indices spread over the fixture (the degenerate states at its end included once n allows)"""
    return np.unique(np.linspace(0, n_total - 1, n).round().astype(np.int64)) if n > 1 else np.array([n_total - 2])


# ------------------------------------------------------------------ 1. critic_q vs graph float64
@pytest.mark.parametrize("obs_dtype", DTYPES)
@pytest.mark.parametrize("n", ROW_COUNTS + (None,))
def test_gpu_critic_q_vs_graph(n, obs_dtype):
    g = load_critic_golden()
    b = batch(obs_dtype, "critic")
    idx = np.arange(len(g.given_rows)) if n is None else pick(len(g.given_rows), n)
    assert n is None or len(idx) == n
    q = _np(b.critic_q(torch.as_tensor(g.given_rows[idx]), torch.as_tensor(g.given_act7[idx])))
    b.synchronize()
    assert q.shape == (len(idx),) and q.dtype == np.float32
    worst = float(np.abs(q.astype(np.float64) - g.critic_q_f64[idx]).max())
    print("critic_q, %d rows, %s: max |q - graph f64| = %.3e (bar %.3e)" % (len(idx), obs_dtype, worst, q_bar(g)))
    assert worst <= q_bar(g)


# ------------------------------------------------------------------ 2. bootstrap_q composition
@pytest.mark.parametrize("obs_dtype", DTYPES)
@pytest.mark.parametrize("n", ROW_COUNTS + (None,))
def test_gpu_bootstrap_q_composition(n, obs_dtype):
    g = load_critic_golden()
    b = batch(obs_dtype)
    idx = np.arange(g.n) if n is None else pick(g.n, n)
    st = torch.as_tensor(g.states[idx])
    q, a7 = b.bootstrap_q(st)
    q2 = b.critic_q(st[:, 0], a7)
    b.synchronize()
    qn, an = _np(q), _np(a7)
    assert qn.shape == (len(idx),) and an.shape == (len(idx), 7)
    worst_a = float(np.abs(an.astype(np.float64) - g.boot_act7_f64[idx]).max())
    worst_q = float(np.abs(qn.astype(np.float64) - g.boot_q_f64[idx]).max())
    print("bootstrap_q, %d rows, %s: max |a - graph| = %.3e (bar %.1e), max |q - graph f64| = %.3e (bar %.3e)"
          % (len(idx), obs_dtype, worst_a, ACTION_TOL, worst_q, boot_bar(g)))
    assert worst_a <= ACTION_TOL
    assert worst_q <= boot_bar(g)
    # the critic half of the bootstrap IS the critic kernel: no tolerance
    assert np.array_equal(bits32(q2), bits32(q)), "critic_q(state[:, 0], act7_out) != bootstrap_q's q"


# ------------------------------------------------------------------ 3. the target actor inside the bootstrap is the acting actor
@pytest.mark.parametrize("obs_dtype", DTYPES)
def test_gpu_bootstrap_actor_is_the_acting_actor(obs_dtype):
    g = load_critic_golden()
    arr = synthetic_arrivals(4, rate=1000.0, horizon_s=60.0, seed=6)
    b = make_batch(arr, 4, 128, "hip", outputs=("obs_post", "reward", "flags", "env_out"), obs_dtype=obs_dtype)
    b.reset()
    b.set_actor(flat_weights(g.weights["target_actor"]))
    b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
    b.step_many(90, source="actor")
    slots = np.argwhere(_np(b.control_mask()))
    assert len(slots) >= 20
    idx = pick(g.n, 300)
    _, a7 = b.bootstrap_q(torch.as_tensor(g.states[idx]))
    a7 = _np(a7)
    a_act = A.actions_of_planted_rows(b, slots, g.states[idx, 0])
    assert np.array_equal(a_act.view(np.uint64), a7[:, 0].astype(np.float64).view(np.uint64)), "act() != act7_out[:, 0]"
    zero_rows = ~g.states[idx].any(axis=2)                        # [n, 7]: absent neighbours
    assert zero_rows[:, 1:].sum() >= 100
    a_zero = A.actions_of_planted_rows(b, slots, np.zeros((1, 28), np.float32))[0]
    assert np.all(a7[zero_rows].astype(np.float64).view(np.uint64) == np.float64(a_zero).view(np.uint64))


# ------------------------------------------------------------------ 4. masking
@pytest.mark.parametrize("obs_dtype", DTYPES)
def test_gpu_bootstrap_masking_and_bounds(obs_dtype):
    g = load_critic_golden()
    b = batch(obs_dtype)
    n = 4 * 64 + 1
    idx = pick(g.n, n)
    st = torch.as_tensor(g.states[idx])
    rng = np.random.default_rng(4)
    flags = rng.choice(np.array([0, _capi.F_ALIVE, _capi.F_ALIVE | _capi.F_CTL, _capi.F_ALIVE | _capi.F_CTL | _capi.F_DONE,
                                 _capi.F_ALIVE | _capi.F_CTL | _capi.F_LOCK | (3 << 8), _capi.F_ALIVE | _capi.F_DONE | _capi.F_DELETED],
                                np.int32), n)
    flags[64:128] = _capi.F_ALIVE                                  # a whole chunk without an evaluated row
    ev = ((flags & (_capi.F_CTL | _capi.F_DONE)) == _capi.F_CTL)
    assert 40 <= ev.sum() <= n - 100
    sent_q, sent_a = np.float32(-12345.5), np.float32(777.25)
    qbuf = torch.full((n + 64,), float(sent_q), dtype=torch.float32, device=b.device)
    abuf = torch.full(((n + 64) * 7,), float(sent_a), dtype=torch.float32, device=b.device)
    q_all, a_all = b.bootstrap_q(st)
    b.bootstrap_q(st, torch.as_tensor(flags), out=qbuf[:n], actions_out=abuf[:n * 7].view(n, 7))
    b.synchronize()
    q, a7 = _np(qbuf), _np(abuf)
    assert np.all(q[n:] == sent_q) and np.all(a7[n * 7:] == sent_a), "wrote behind q[n] / act7_out[n]"
    q, a7 = q[:n], a7[:n * 7].reshape(n, 7)
    assert np.all(bits32(q[~ev]) == 0) and np.all(bits32(a7[~ev]) == 0), "masked rows must be exactly 0"
    assert np.array_equal(bits32(q[ev]), bits32(_np(q_all)[ev])) and np.array_equal(bits32(a7[ev]), bits32(_np(a_all)[ev]))
    # the same rows with flags = NULL are evaluated
    assert np.abs(_np(q_all).astype(np.float64) - g.boot_q_f64[idx]).max() <= boot_bar(g)
    assert np.all(_np(q_all)[~ev] != 0)
    # no output buffer for the actions
    qbuf2 = torch.full((n + 64,), float(sent_q), dtype=torch.float32, device=b.device)
    rc = b.lib.pve_bootstrap_q(b._h, st.to(b.device, b.obs_dtype).contiguous().data_ptr(), None, qbuf2.data_ptr(), None, n)
    b.synchronize()
    assert rc == 0 and np.array_equal(bits32(qbuf2[:n]), bits32(q_all)) and np.all(_np(qbuf2)[n:] == sent_q)


def test_gpu_target_network_errors():
    g = load_critic_golden()
    arr = synthetic_arrivals(2, rate=500.0, horizon_s=30.0, seed=5)
    b = make_batch(arr, 2, 64, "hip", outputs=("obs_post", "flags"))
    L, dev = b.lib, b.device
    st = torch.zeros(3, 7, 28, dtype=torch.float64, device=dev)
    q = torch.zeros(3, dtype=torch.float32, device=dev)
    a = torch.zeros(3, 7, dtype=torch.float32, device=dev)
    assert L.pve_bootstrap_q(b._h, st.data_ptr(), None, q.data_ptr(), None, 3) == -3          # PVE_ERR_STATE
    assert L.pve_critic_forward(b._h, st.data_ptr(), a.data_ptr(), q.data_ptr(), 3) == -3
    b.set_target_networks(critic=g.weights["critic"])
    assert L.pve_critic_forward(b._h, st.data_ptr(), a.data_ptr(), q.data_ptr(), 3) == 0      # no pve_reset needed
    assert L.pve_bootstrap_q(b._h, st.data_ptr(), None, q.data_ptr(), None, 3) == -3          # still no target actor
    b.set_target_networks(actor=g.weights["target_actor"])
    assert L.pve_bootstrap_q(b._h, st.data_ptr(), None, q.data_ptr(), None, 3) == 0
    for bad in (0, -5):
        assert L.pve_bootstrap_q(b._h, st.data_ptr(), None, q.data_ptr(), None, bad) == -1
        assert L.pve_critic_forward(b._h, st.data_ptr(), a.data_ptr(), q.data_ptr(), bad) == -1
    assert L.pve_bootstrap_q(b._h, None, None, q.data_ptr(), None, 3) == -1
    assert L.pve_critic_forward(b._h, st.data_ptr(), None, q.data_ptr(), 3) == -1
    assert L.pve_set_target_networks(b._h, None, None) == -1
    b.synchronize()


# ------------------------------------------------------------------ 5. integration: a roll-out's own state_pre / flags
def test_gpu_bootstrap_over_a_trajectory():
    from oracle.actor_np import load_weights
    g = load_critic_golden()
    arr = synthetic_arrivals(4, rate=1300.0, horizon_s=40.0, seed=11)

    def rollout(install):
        b = make_batch(arr, 4, 64, "hip", outputs=TRAIN_OUTS)
        b.reset()
        b.set_actor(flat_weights(load_weights()))
        if install:
            b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
        b.set_exploration(0.2, seed=77)
        for _ in range(250):                                      # (to steady state: vehicles take ~150 ticks to cross)
            b.step_with_actor()
        traj = b.step_many(30, source="actor", trajectory=True)
        b.synchronize()
        return b, traj
    b, traj = rollout(True)
    q, a7 = b.bootstrap_q()
    b.synchronize()
    assert tuple(q.shape) == (30, 4, 64) and tuple(a7.shape) == (30, 4, 64, 7)
    state, flags = _np(traj["state_pre"]), _np(traj["flags"])
    ev = (flags & (_capi.F_CTL | _capi.F_DONE)) == _capi.F_CTL
    n_done = int(((flags & _capi.F_CTL) != 0).sum() - ev.sum())
    print("trajectory: %d evaluated rows, %d controlled rows behind Done" % (ev.sum(), n_done))
    assert ev.sum() >= 200 and n_done >= 1
    # the oracle side: float64 NumPy on the read-back rows (no NaN), and float32 NumPy within its own spread of it
    q64, a64 = critic.bootstrap_q(g.weights["target_actor"], g.weights["target_critic"], state, flags, dtype=np.float64)
    assert np.all(np.isfinite(q64)) and np.all(np.isfinite(a64))
    qd, ad = _np(q).astype(np.float64), _np(a7).astype(np.float64)
    assert np.all(bits32(_np(q))[~ev] == 0) and np.all(bits32(_np(a7))[~ev] == 0)
    worst_a, worst_q = float(np.abs(ad - a64).max()), float(np.abs(qd - q64).max())
    print("trajectory: max |a - numpy f64| = %.3e, max |q - numpy f64| = %.3e (bar %.3e)" % (worst_a, worst_q, boot_bar(g)))
    assert worst_a <= ACTION_TOL and worst_q <= boot_bar(g)
    # installing the target networks changes no bit of the roll-out
    b0, traj0 = rollout(False)
    for k in traj:
        assert torch.equal(traj[k], traj0[k]), k
    for f in ("p", "v", "a", "id", "meta", "step"):
        assert torch.equal(b.state_field(f), b0.state_field(f)), f


# ------------------------------------------------------------------ 6. more than one chunk per wave: the pending ring across chunks
SENT_Q, SENT_A = np.float32(-12345.5), np.float32(777.25)


def big_bootstrap_inputs(b, g, n):
    """(state [n, 7, 28] built ON the device from the uploaded fixture, flags, row map, evaluated mask) of the big call"""
    idx, flags = TQ.row_map(n, g.n), TQ.bootstrap_flags(n)
    fixture = torch.as_tensor(g.states).to(b.device, b.obs_dtype)
    big = fixture.index_select(0, torch.as_tensor(idx).to(b.device))
    return big, torch.as_tensor(flags).to(b.device), idx, TQ.evaluated(flags)


def sentinel_buffers(b, n):
    return (torch.full((n + 64,), float(SENT_Q), dtype=torch.float32, device=b.device),
            torch.full(((n + 64) * 7,), float(SENT_A), dtype=torch.float32, device=b.device))


@pytest.mark.parametrize("obs_dtype,n", [(torch.float32, TQ.N_BOOT_F32), (torch.float64, TQ.N_BOOT_F64)])
def test_gpu_bootstrap_many_chunks_per_wave(obs_dtype, n):
    """Three chunks per wave at 512 workgroups, chunk densities 0.25 .. 1: rows carried into the next chunk, ring writes across
    index 127 -> 0, a 95-entry backlog, tiles mixing rows of two chunks, left-overs flushed behind a chunk that accepted nothing.
    Expected: the kernel's own one-chunk-per-wave results on the fixture's rows (the path pinned to the graph above), bit for
    bit -- each vehicle is its own column of the matrix products, so its tile company does not matter (section 4 asserts the
    same between masked and unmasked runs) -- and, independently of the kernel, the graph in float64 within the bars above."""
    g = load_critic_golden()
    b = batch(obs_dtype)
    assert TQ.target_q_grid(g.n, TQ.BOOT_PER_CU) * 4 * 64 >= g.n and TQ.target_q_grid(n, TQ.BOOT_PER_CU) * 4 * 64 * 2 < n
    q_small, a_small = b.bootstrap_q(torch.as_tensor(g.states))           # flags = None, one chunk per wave
    q_small, a_small = _np(q_small), _np(a_small)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    big, flags, idx, ev = big_bootstrap_inputs(b, g, n)
    qbuf, abuf = sentinel_buffers(b, n)
    b.bootstrap_q(big, flags, out=qbuf[:n], actions_out=abuf[:n * 7].view(n, 7))
    # the same call without an output buffer for the actions (the raw entry point, as in section 4)
    qbuf2 = torch.full((n + 64,), float(SENT_Q), dtype=torch.float32, device=b.device)
    rc = b.lib.pve_bootstrap_q(b._h, big.data_ptr(), flags.data_ptr(), qbuf2.data_ptr(), None, n)
    b.synchronize()
    held = (torch.cuda.max_memory_allocated() - base) / 1e6
    q, a7, q2 = _np(qbuf), _np(abuf), _np(qbuf2)
    del big, qbuf, abuf, qbuf2
    print("bootstrap_q, %d rows, %s, grid %d: %.0f MB on the device, %d evaluated rows (%.3f); walk %s"
          % (n, obs_dtype, TQ.target_q_grid(n, TQ.BOOT_PER_CU), held, ev.sum(), ev.mean(), TQ.counters(TQ.bootstrap_walk(n))))
    assert np.all(q[n:] == SENT_Q) and np.all(a7[n * 7:] == SENT_A), "wrote behind q[n] / act7_out[n]"
    q, a7 = q[:n], a7[:n * 7].reshape(n, 7)
    assert np.all(bits32(q[~ev]) == 0) and np.all(bits32(a7[~ev]) == 0), "masked rows must be exactly 0"
    wrong_q = np.flatnonzero(ev & (bits32(q) != bits32(q_small[idx])))
    wrong_a = np.flatnonzero(ev & (bits32(a7) != bits32(a_small[idx])).any(axis=1))
    assert len(wrong_q) == 0 and len(wrong_a) == 0, "rows %s / %s (chunks %s) differ from the one-chunk call" % (
        wrong_q[:8], wrong_a[:8], np.unique(np.concatenate([wrong_q, wrong_a]) // 64)[:8])
    worst_a = float(np.abs(a7.astype(np.float64) - g.boot_act7_f64[idx])[ev].max())
    worst_q = float(np.abs(q.astype(np.float64) - g.boot_q_f64[idx])[ev].max())
    print("bootstrap_q, %d rows, %s: max |a - graph| = %.3e (bar %.1e), max |q - graph f64| = %.3e (bar %.3e)"
          % (n, obs_dtype, worst_a, ACTION_TOL, worst_q, boot_bar(g)))
    assert worst_a <= ACTION_TOL and worst_q <= boot_bar(g)
    assert rc == 0 and np.array_equal(bits32(q2[:n]), bits32(q)) and np.all(q2[n:] == SENT_Q), "actions_out = NULL changes q"


@pytest.mark.parametrize("obs_dtype", DTYPES)
def test_gpu_critic_q_many_chunks_per_wave(obs_dtype):
    """The critic alone (flags = NULL: whole chunks only) at 2 x 262 144 + 3 x 64 + 17 rows: 4 waves of the 1024 workgroups take
    a third chunk (their ring wraps with it), the last chunk is partial."""
    g = load_critic_golden()
    b = batch(obs_dtype, "critic")
    n = TQ.N_CRITIC
    idx = TQ.row_map(n, len(g.given_rows), seed=12)
    q_small = _np(b.critic_q(torch.as_tensor(g.given_rows), torch.as_tensor(g.given_act7)))
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx_dev = torch.as_tensor(idx).to(b.device)
    rows = torch.as_tensor(g.given_rows).to(b.device, b.obs_dtype).index_select(0, idx_dev)
    acts = torch.as_tensor(g.given_act7).to(b.device).index_select(0, idx_dev)
    qbuf, _ = sentinel_buffers(b, n)
    b.critic_q(rows, acts, out=qbuf[:n])
    b.synchronize()
    held = (torch.cuda.max_memory_allocated() - base) / 1e6
    q = _np(qbuf)
    del rows, acts, qbuf
    print("critic_q, %d rows, %s, grid %d: %.0f MB on the device; walk %s"
          % (n, obs_dtype, TQ.target_q_grid(n, TQ.CRITIC_PER_CU), held, TQ.counters(TQ.critic_walk(n))))
    assert np.all(q[n:n + 64] == SENT_Q), "wrote behind q[n]"
    q = q[:n]
    wrong = np.flatnonzero(bits32(q) != bits32(q_small[idx]))
    assert len(wrong) == 0, "rows %s (chunks %s) differ from the one-chunk call" % (wrong[:8], np.unique(wrong // 64)[:8])
    worst = float(np.abs(q.astype(np.float64) - g.critic_q_f64[idx]).max())
    print("critic_q, %d rows, %s: max |q - graph f64| = %.3e (bar %.3e)" % (n, obs_dtype, worst, q_bar(g)))
    assert worst <= q_bar(g)

"""The training side on the layouts a user trains on, held to the oracle by VEHICLE IDENTITY: one scenario body for the CPU
emulator ("emu": tests/test_nstep_identity.py) and the HIP kernels ("hip": tests/test_gpu_nstep_layouts.py).

A roll-out as check_step_many_state_rows builds it (synthetic arrivals, the 8-lane intention stream, actions from
set_action_pool) so that the sequential oracle replays it exactly: a prefill, then CALLS chained step_many calls of TICKS ticks
into a ring of TWO alloc_trajectory(TICKS) sets, every call followed by nstep_transitions(prev = the previous call's dict,
q = a fixed pseudo-random tensor).

  B  identity: the oracle's controlled vehicles of every tick, keyed by vehicle id, feed tests/nstep_by_vehicle.py (the
     reference's own per-vehicle buffers, pinned to tests/golden/nstep_ref.npz).  Every record of the pass is turned into
     (closing tick, vehicle id) through the lanej block at its START slot; the two sides must hold the same keys, codes, s0 rows,
     7-action vectors and targets.  For lane_num 4 / 8 the vehicles are processed and listed in (lane, intention, j) order, the
     pass walks slots: this is the check that the difference does not matter.
  C  dirty buffers: the same roll-out a second time with every tensor of the ring filled with byte 0xFF beforehand (-1 in the
     int blocks, NaN in the rows and rewards); every DEFINED position, every record and the handle's state must be bit-equal,
     and the fill must survive somewhere outside them (the definedness contract of alloc_trajectory, in a test).

Bars (none taken from what the code under test returns): rows stored as float64 1e-9, as float32 2e-6 relative (the bars of
check_step_many_state_rows); the float64 target window x 1e-9 x max(1, |target|): the rewards, held to the oracle at 1e-9 by the
parity suite, enter with weights gamma^k <= 1, and q is the same tensor on both sides."""
import functools

import numpy as np
import torch

from oracle.oracle import OracleEnv
from oracle.record import close
from pve_mcc_amd import _capi, critic, nstep
from pve_mcc_amd.arrivals import synthetic_arrivals, synthetic_intentions
from tests.critic_scenarios import load_critic_golden
from tests.hip_adapter import _np, make_batch
from tests.nstep_by_vehicle import VehicleBuffers
from tests.parity_util import GoldenCase

GAMMA0 = float(np.tanh(6.0 / 12.0) * 0.9)            # main.py:227 at epoch 0
WINDOW, E, TICKS, CALLS, N_POOL = 13, 3, 20, 4, 7
OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "lanej", "new_slot", "env_out")
STATE_FIELDS = ("p", "v", "a", "id", "meta", "step")
F_ALIVE, F_CTL, F_DONE = _capi.F_ALIVE, _capi.F_CTL, _capi.F_DONE

# name -> lane_num, capacity, rate (veh/h/lane), float32 rows, prefill ticks, seed; "ctor": the fixture whose constructor
# arguments the batch and the oracles get (geo_g4_rand_vm6: vm = 6, the shipped checkpoint's)
SCENARIOS = {
    "g4_c64_f64": dict(lane_num=4, capacity=64, rate=1200.0, f32=False, prefill=220, seed=181),
    "g4_c64_f32": dict(lane_num=4, capacity=64, rate=1200.0, f32=True, prefill=220, seed=181),
    "g4_c128_vm6_f32": dict(lane_num=4, capacity=128, rate=1800.0, f32=True, prefill=220, seed=182, ctor="geo_g4_rand_vm6"),
    "g8_c128_f64": dict(lane_num=8, capacity=128, rate=1500.0, f32=False, prefill=220, seed=183),
    "g8_c128_f32": dict(lane_num=8, capacity=128, rate=1500.0, f32=True, prefill=220, seed=183),
    # (12 lanes x 1100 veh/h bring 3.7 vehicles per second and nobody leaves before tick ~150: 64 slots hold the first 180 ticks)
    "g12_c64_f64": dict(lane_num=12, capacity=64, rate=1100.0, f32=False, prefill=95, seed=184),
    "g12_c256_f32": dict(lane_num=12, capacity=256, rate=1100.0, f32=True, prefill=220, seed=184),
}
LAUNCH_FORMS = {"one_launch": dict(chunk=0, persistent=False), "queue": dict(chunk=7, persistent=True)}


def bits(x):
    a = np.ascontiguousarray(x)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(bits(x), bits(y))


class Bag:
    pass


@functools.lru_cache(maxsize=None)
def inputs(name):
    """What both sides are given: arrivals, intentions, constructor arguments, the action pool, q of every measured call"""
    sc = SCENARIOS[name]
    x = Bag()
    x.name, x.lane_num, x.capacity, x.f32, x.prefill = name, sc["lane_num"], sc["capacity"], sc["f32"], sc["prefill"]
    x.total = x.prefill + CALLS * TICKS
    rng = np.random.default_rng(sc["seed"])
    x.arr = synthetic_arrivals(E, rate=sc["rate"], horizon_s=x.total * 0.1 + 30, seed=sc["seed"], lane_num=x.lane_num)
    x.choice = synthetic_intentions(E, x.arr.shape[1], seed=sc["seed"], lane_num=x.lane_num) if x.lane_num == 8 else None
    x.cfg = dict(GoldenCase(sc["ctor"]).ctor) if "ctor" in sc else {}
    x.pool = rng.uniform(-3, 3, size=(N_POOL, E, x.capacity)).astype(np.float32).astype(np.float64)
    x.q = rng.uniform(-20.0, 20.0, size=(CALLS, TICKS, E, x.capacity)).astype(np.float32)
    for a in (x.pool, x.q):
        a.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------------- the oracle side
@functools.lru_cache(maxsize=None)
def oracle_trace(name):
    """The sequential oracle over the whole roll-out, once per scenario and read-only: per (tick, env) the vehicle id behind
    every (lane, j) and the controlled vehicles in PROCESSING order with the row the tick stored for them, their 7 actions,
    reward and Done; and the vacuity conditions that do not involve the pass at all."""
    x = inputs(name)
    if x.lane_num == 12:
        oracles = [OracleEnv(x.arr[e], **x.cfg) for e in range(E)]
    else:
        from oracle.oracle_geo import OracleGeoEnv
        oracles = [OracleGeoEnv(x.arr[e], x.lane_num, choice=None if x.choice is None else x.choice[e], **x.cfg) for e in range(E)]
    tr = Bag()
    tr.vid_of, tr.ctl, tr.n_alive = {}, {}, np.zeros((x.total, E), np.int64)
    tr.unordered = 0                       # (tick, env) whose processing order is not ascending slot order, measured calls
    slots_seen, moves, was_ctl = {}, 0, [set() for _ in range(E)]
    for t in range(x.total):
        for e, o in enumerate(oracles):
            vi = o.vehicles()[0]
            na = len(vi)
            lane, j, vid, ctlm = vi[:, 0], vi[:, 1], vi[:, 2].astype(np.int64), vi[:, 5]
            assert na <= x.capacity, "the scene outgrows the capacity: tick %d env %d" % (t, e)
            tr.n_alive[t, e] = na
            acts = np.where(ctlm != 0, x.pool[t % N_POOL, e, :na], 0.0)
            rec = o.tick(acts, want_state=True)
            slot_of = {(int(l), int(k)): s for s, (l, k) in enumerate(zip(lane, j))}
            tr.vid_of[t, e] = {lj: int(vid[s]) for lj, s in slot_of.items()}
            done_of = {int(r[2]): bool(r[7]) for r in rec["veh_i"]}
            rows = []
            for c, (l, k) in enumerate(rec["ids"].tolist()):
                v = tr.vid_of[t, e][l, k]
                rows.append((l, k, v, rec["obs0"][c].copy(), rec["act7"][c].copy(), float(rec["reward"][c]), done_of[v]))
            tr.ctl[t, e] = rows
            now = {r[2] for r in rows}
            # a vehicle is controlled from its first tick on: one that was not controlled at the previous tick was spawned then
            assert not (now - was_ctl[e]) & set(tr.vid_of.get((t - 1, e), {}).values()), (t, e)
            was_ctl[e] = now
            if t >= x.prefill:
                order = [slot_of[l, k] for l, k, *_ in rows]
                tr.unordered += int(any(a > b for a, b in zip(order, order[1:])))
                for s, v in enumerate(vid.tolist()):
                    seen = slots_seen.setdefault((e, v), [])
                    moves += int(bool(seen) and seen[-1] != s)
                    seen.append(s)
    tr.moves = moves
    survivors = [s for s in slots_seen.values() if len(s) > 1]
    tr.moved_share = sum(len(set(s)) > 1 for s in survivors) / max(1, len(survivors))
    assert all(o.overflow == 0 for o in oracles)
    return tr


def reference_transitions(name, lanej_calls):
    """Model A fed from the oracle alone -- rows, actions, rewards, Done -- with q read at the slot where the device's lanej block
    shows the vehicle's (lane, j) at that tick -> {(closing tick, env, vehicle id): Emission}"""
    x, tr = inputs(name), oracle_trace(name)
    out = {}
    for e in range(E):
        model = VehicleBuffers(GAMMA0, WINDOW)
        last = {}
        for t in range(x.total):
            ci, k = divmod(t - x.prefill, TICKS) if t >= x.prefill else (-1, 0)
            now = {}
            for l, j, v, row, act7, reward, done in tr.ctl[t, e]:
                q = 0.0                                                       # (a window that closes in the prefill is not looked at)
                if ci >= 0:
                    lj = lanej_calls[ci][k, e, :tr.n_alive[t, e]]
                    at = np.nonzero(lj == ((l << 16) | j))[0]
                    assert len(at) == 1, "lanej: (lane %d, j %d) at tick %d env %d is in %d slots" % (l, j, t, e, len(at))
                    q = x.q[ci, k, e, at[0]]
                model.feed(t, v, last.get(v, np.zeros(28)), act7, reward, q, done)
                now[v] = row
            last = now
        for (t, v, _), em in model.emitted().items():
            if t >= x.prefill:
                out[t, e, v] = em
    return out


def vacuity(name, want, tr):
    """The conditions against a vacuous pass, on the reference side alone -> the counts"""
    x = inputs(name)
    n = dict(transitions=len(want),
             crossing=sum(1 for (t, e, v), em in want.items() if (t - em.entries + 1 - x.prefill) // TICKS < (t - x.prefill) // TICKS),
             done=sum(1 for em in want.values() if em.done), fresh=sum(1 for em in want.values() if not em.row.any()),
             moved_share=tr.moved_share, moves=tr.moves, unordered=tr.unordered)
    assert n["transitions"] >= 300 and n["crossing"] >= 20 and n["done"] >= 3 and n["fresh"] >= 5, n
    assert n["moved_share"] >= 0.9 or n["moves"] >= 50, n
    assert x.lane_num == 12 or n["unordered"] >= 1, n
    return n


# ---------------------------------------------------------------------------------------------------- the device side
def fill_ff(ring):
    for traj in ring:
        for tns in traj.values():
            tns.view(torch.uint8).fill_(0xFF)


def rollout(name, backend, chunk=0, persistent=False, dirty=False):
    """-> per measured call: every block copied to the host, records / index / total / dense target and code, bootstrap Q; the
    last 13 ticks of the prefill; the state fields after the last call"""
    x = inputs(name)
    kw = dict(lane_num=x.lane_num, intentions=x.choice) if x.lane_num != 12 else {}
    b = make_batch(x.arr, E, x.capacity, backend, outputs=OUTS, obs_dtype=torch.float32 if x.f32 else torch.float64, **kw, **x.cfg)
    b.reset()
    b.set_action_pool(torch.as_tensor(x.pool.copy()))
    g = load_critic_golden()
    if backend == "hip":
        b.set_target_networks(actor=g.weights["target_actor"], critic=g.weights["target_critic"])
    prev = b.step_many(x.prefill, source="pool", trajectory=True)
    b.synchronize()
    res = Bag()
    res.prefill = {k: _np(prev[k][-WINDOW:]).copy() for k in OUTS}
    ring = [b.alloc_trajectory(TICKS), b.alloc_trajectory(TICKS)]
    if dirty:
        fill_ff(ring)
    res.calls = []
    prev_host = res.prefill
    for ci in range(CALLS):
        traj = b.step_many(TICKS, source="pool", trajectory=ring[ci & 1], chunk=chunk, persistent=persistent)
        b.synchronize()
        want_launch = "persistent" if (persistent and 0 < chunk < TICKS) else "resident"
        assert b.last_launch() == want_launch, (b.last_launch(), want_launch)
        c = Bag()
        c.blocks = {k: _np(traj[k]).copy() for k in OUTS}
        q = x.q[ci]
        if backend == "hip":
            qb, _ = b.bootstrap_q()
            rec, idx, total = b.nstep_transitions(GAMMA0, window=WINDOW, prev=prev, q=torch.as_tensor(q.copy()).to(b.device))
            target, code = b._nstep_last[0], b._nstep_last[1]
            b.synchronize()
            c.q_boot, c.rec, c.idx, c.total, c.target, c.code = _np(qb), _np(rec), _np(idx), int(total), _np(target), _np(code)
        else:           # the emulator has no n-step or target-network kernels: their NumPy restatements on the read-back blocks
            c.q_boot, _ = critic.bootstrap_q(g.weights["target_actor"], g.weights["target_critic"], c.blocks["state_pre"], c.blocks["flags"])
            c.target, c.code, n_back = nstep.scan(c.blocks, GAMMA0, WINDOW, prev=prev_host, q=q)
            c.rec, c.idx = nstep.records(c.blocks, c.target, c.code, n_back, prev=prev_host)
            c.total = len(c.rec)
        res.calls.append(c)
        prev, prev_host = traj, c.blocks
    res.fields = {f: _np(b.state_field(f)).copy() for f in STATE_FIELDS}
    res.overflow = b.metrics()["overflow"]
    return res


# ---------------------------------------------------------------------------------------------------- B: identity
def check_identity(name, backend, res):
    x, tr = inputs(name), oracle_trace(name)
    want = reference_transitions(name, [c.blocks["lanej"] for c in res.calls])
    counts = vacuity(name, want, tr)
    assert res.overflow == 0
    tol = 2e-6 if x.f32 else 1e-9
    worst = dict(row=0.0, act7=0.0, target=0.0)
    got_keys = set()
    prev = res.prefill
    for ci, c in enumerate(res.calls):
        start = x.prefill + ci * TICKS
        assert c.total == len(c.rec) == len(c.idx)
        n_back = c.code.shape[0] - TICKS
        assert n_back == WINDOW - 1
        for i, (u, e, s, code) in enumerate(c.idx.tolist()):
            lj = int(c.blocks["lanej"][u, e, s]) if u >= 0 else int(prev["lanej"][u, e, s])       # (u < 0: counted from prev's end)
            n = code & 0xFF
            key = (start + u + n - 1, e, tr.vid_of[start + u, e][lj >> 16, lj & 0xFFFF])
            assert key not in got_keys, "emitted twice: %r" % (key,)
            got_keys.add(key)
            assert key in want, "call %d: a transition the reference does not have: %r (start tick %d slot %d code %#x)" % (ci, key, u, s, code)
            assert start <= key[0] < start + TICKS
            em = want[key]
            assert (n, bool(code & nstep.BOOT), bool(code & nstep.DONE)) == (em.entries, em.boot, em.done), (key, hex(code), em)
            row32, act32 = em.row.astype(np.float32), em.act7.astype(np.float32)
            assert close(row32, c.rec[i, :28], tol), ("s0 row", key, row32, c.rec[i, :28])
            assert close(act32, c.rec[i, 28:35], tol), ("act7", key, act32, c.rec[i, 28:35])
            dense = float(c.target[u + n_back, e, s])
            bar = WINDOW * 1e-9 * max(1.0, abs(float(em.target)))
            assert abs(dense - float(em.target)) <= bar, ("target", key, dense, em.target)
            assert c.rec[i, 35] == np.float32(dense)
            worst["row"] = max(worst["row"], float(np.max(np.abs(row32.astype(np.float64) - c.rec[i, :28]) / np.maximum(1.0, np.abs(row32)))))
            worst["act7"] = max(worst["act7"], float(np.max(np.abs(act32.astype(np.float64) - c.rec[i, 28:35]) / np.maximum(1.0, np.abs(act32)))))
            worst["target"] = max(worst["target"], abs(dense - float(em.target)) / max(1.0, abs(float(em.target))))
        missing = {k for k in want if start <= k[0] < start + TICKS} - got_keys
        assert not missing, "call %d: %d transitions of the reference are missing, e.g. %r" % (ci, len(missing), sorted(missing)[:3])
        if backend == "hip":            # the exact layer: the kernels == nstep.py on the read-back blocks
            w_t, w_c, nb = nstep.scan(c.blocks, GAMMA0, WINDOW, prev=prev, q=x.q[ci])
            w_rec, w_idx = nstep.records(c.blocks, w_t, w_c, nb, prev=prev)
            assert np.array_equal(c.code, w_c) and np.array_equal(bits(c.target)[w_c != 0], bits(w_t)[w_c != 0])
            assert np.array_equal(c.idx, w_idx) and same_bits(c.rec, w_rec)
        prev = c.blocks
    assert got_keys == set(want)
    line = ("%s %s: %d transitions, %d crossing, %d Done, %d fresh starts, %.0f%% moved / %d moves, %d unordered (tick, env); "
            "max row %.2e / act7 %.2e (bar %.0e), target %.2e (bar %.1e)"
            % (name, backend, counts["transitions"], counts["crossing"], counts["done"], counts["fresh"], 100 * counts["moved_share"],
               counts["moves"], counts["unordered"], worst["row"], worst["act7"], tol, worst["target"], WINDOW * 1e-9))
    print(line)
    return line


# ---------------------------------------------------------------------------------------------------- C: dirty buffers
def check_dirty(name, clean, dirty):
    """run 2 (ring filled with 0xFF) against run 1 (ring as alloc_trajectory returns it), same handles otherwise"""
    cat = lambda r, k: np.concatenate([c.blocks[k] for c in r.calls])                   # noqa: E731
    f1, f2 = cat(clean, "flags"), cat(dirty, "flags")
    assert np.array_equal(f1, f2), "flags"
    assert np.array_equal(cat(clean, "env_out"), cat(dirty, "env_out")), "env_out"
    alive, ctl = (f1 & F_ALIVE) != 0, (f1 & F_CTL) != 0
    for k in ("reward", "lanej", "new_slot"):
        assert np.array_equal(bits(cat(clean, k)[alive]), bits(cat(dirty, k)[alive])), k
    for k in ("nbr", "obs_pre", "state_pre"):
        assert np.array_equal(bits(cat(clean, k)[ctl]), bits(cat(dirty, k)[ctl])), k
    nxt = ctl[1:]                                            # the rows the NEXT tick's controlled vehicles were given
    assert np.array_equal(bits(cat(clean, "obs_post")[:-1][nxt]), bits(cat(dirty, "obs_post")[:-1][nxt])), "obs_post"
    for ci, (a, b) in enumerate(zip(clean.calls, dirty.calls)):
        assert a.total == b.total and np.array_equal(a.idx, b.idx) and same_bits(a.rec, b.rec), "records of call %d" % ci
        assert same_bits(a.q_boot, b.q_boot), "bootstrap_q of call %d" % ci
        assert not np.isnan(b.rec).any() and not np.isnan(b.q_boot).any(), "NaN in call %d" % ci
    for f in STATE_FIELDS:
        assert same_bits(clean.fields[f], dirty.fields[f]), f
    # the fill reached memory the kernels skip: what the ring holds at the end (the last two calls) still shows it outside the
    # defined positions, where run 1 shows the zeros of alloc_trajectory or an earlier tick's values
    last = lambda r, k: np.concatenate([c.blocks[k] for c in r.calls[-2:]])             # noqa: E731
    fl = last(dirty, "flags")
    undefined = dict(reward=(fl & F_ALIVE) == 0, new_slot=(fl & F_ALIVE) == 0, state_pre=(fl & F_CTL) == 0,
                     obs_post=np.concatenate([(fl[1:] & F_CTL) == 0, np.zeros_like(fl[:1], bool)]))
    left = {}
    for k, where in undefined.items():
        u2, u1 = bits(last(dirty, k))[where], bits(last(clean, k))[where]
        left[k] = int((u2 == np.iinfo(u2.dtype).max).sum())
        assert left[k] > 0, "no element of %s still holds the fill" % k
        assert not np.array_equal(u1, u2) and (k == "new_slot" or not (u1 == np.iinfo(u1.dtype).max).any()), k
    return left

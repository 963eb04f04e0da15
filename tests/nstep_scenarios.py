"""Hand-made trajectories for the n-step transition pass, shared by tests/test_nstep.py and tests/test_gpu_nstep.py.

`make_trajectory` plays a toy population through [T, E, K] blocks of the shape step_many(trajectory=...) returns: vehicles are
spawned into free slots (all-zero observation row, as ref :380), live a random number of ticks, are moved to a NEW RANDOM
slot every tick (new_slot is a permutation), some are uncontrolled, some vanish through a -1 link without Done, one is Done
at its very first tick.  Alongside, the reference's own bookkeeping (main.py:243-266: a per-vehicle buffer, emit the oldest
entry when the buffer holds `window` entries or the vehicle is Done) is restated with plain Python floats: `expected` maps
(start tick, env, start slot) -> (target, entries, bootstrapped, done)."""
import functools
import os

import numpy as np

F_ALIVE, F_CTL, F_DONE, F_DELETED = 0x01, 0x02, 0x04, 0x08


class Traj:
    pass


def _row(rng, dtype):
    r = rng.uniform(-1.0, 1.0, 28)
    r[1] = rng.uniform(5.0, 13.0)                  # a live vehicle's row holds its speed >= vm > 0 (ref :1336)
    return r.astype(dtype)


@functools.lru_cache(maxsize=None)
def make_trajectory(T, E=3, K=64, seed=0, f32=False, fill=0.6):
    rng = np.random.RandomState(seed * 1000 + T * 7 + K + (1 if f32 else 0))
    dt = np.float32 if f32 else np.float64
    tr = Traj()
    tr.T, tr.E, tr.K, tr.dtype = T, E, K, dt
    tr.obs_post = np.zeros((T, E, K, 28), dt)
    tr.state_pre = rng.uniform(-3.0, 3.0, (T, E, K, 7, 28)).astype(dt)
    tr.reward = np.zeros((T, E, K), np.float64)
    tr.flags = np.zeros((T, E, K), np.int32)
    tr.new_slot = np.full((T, E, K), -1, np.int32)
    tr.obs_first = np.zeros((E, K, 28), dt)
    tr.q = rng.uniform(-20.0, 20.0, (T, E, K)).astype(np.float32)
    tr.life = []                                   # (env, first tick, first slot, ticks lived, controlled, ended by Done)
    for e in range(E):
        veh = {}                                   # slot -> dict(ctl, left, vanish, born, slot0, n)

        def spawn(slot, t, fresh):
            u = rng.rand()
            left = 1 if u < 0.08 else int(rng.randint(1, 31))
            veh[slot] = dict(ctl=rng.rand() > 0.15, left=left, vanish=rng.rand() < 0.08, born=t, slot0=slot, n=0)
            return veh[slot]
        for slot in rng.permutation(K)[:int(fill * K)]:
            spawn(int(slot), 0, True)
            if rng.rand() < 0.5:                   # half of the initial population is older than the trajectory
                tr.obs_first[e, slot] = _row(rng, dt)
        for t in range(T):
            nxt, free = {}, list(rng.permutation(K))
            for slot in sorted(veh):
                v = veh[slot]
                v["n"] += 1
                v["left"] -= 1
                dies = v["left"] == 0
                f = F_ALIVE | (F_CTL if v["ctl"] else 0)
                if v["ctl"]:
                    tr.reward[t, e, slot] = rng.uniform(-2.0, 5.0)
                if dies:
                    f |= F_DELETED | (0 if v["vanish"] else F_DONE)
                    tr.life.append((e, v["born"], v["slot0"], v["n"], v["ctl"], not v["vanish"]))
                else:
                    to = int(free.pop())
                    tr.new_slot[t, e, slot] = to
                    nxt[to] = v
                    tr.obs_post[t, e, to] = _row(rng, dt)
                tr.flags[t, e, slot] = f
            veh = nxt
            for slot in free:                      # spawns: an all-zero row (ref :380)
                if len(veh) < int(fill * K) and rng.rand() < 0.5:
                    spawn(int(slot), t + 1, True)
    for a in (tr.obs_post, tr.state_pre, tr.reward, tr.flags, tr.new_slot, tr.obs_first, tr.q):
        a.setflags(write=False)
    return tr


def blocks(tr, a=0, b=None):
    """ticks a .. b - 1 as a segment dict"""
    b = tr.T if b is None else b
    return dict(obs_post=tr.obs_post[a:b], state_pre=tr.state_pre[a:b], reward=tr.reward[a:b], flags=tr.flags[a:b],
                new_slot=tr.new_slot[a:b])


def obs_before(tr, a):
    """the rows stored before tick a"""
    return tr.obs_first if a == 0 else tr.obs_post[a - 1]


def expected(tr, gamma, window, tail=False, first=0, lo=0, hi=None):
    """The reference's buffers (main.py:243-266) over ticks first .. hi - 1, buffers empty at `first`; the transitions whose
    emitting tick lies in lo .. hi - 1 -> {(start tick, env, start slot): (target, entries, bootstrapped, done)}."""
    hi = tr.T if hi is None else hi
    gamma = float(gamma)
    out = {}
    for e in range(tr.E):
        buf = {}                                   # current slot -> list of (tick, slot, reward)

        def emit(b, t, slot, done, key_from):
            if done:
                r = b[-1][2]
            else:
                r = b[-1][2] + gamma * float(np.float64(tr.q[t, e, slot]))
            for ent in reversed(b[:-1]):
                r = ent[2] + gamma * r
            if lo <= t < hi:
                out[(b[0][0], e, b[0][1])] = (r, len(b), not done, done)
        for t in range(first, hi):
            nxt = {}
            for slot in range(tr.K):
                f = int(tr.flags[t, e, slot])
                if not f & F_CTL:
                    continue
                b = buf.get(slot, []) + [(t, slot, float(tr.reward[t, e, slot]))]
                done = bool(f & F_DONE)
                if done or len(b) >= window:
                    # a buffer that never filled is emitted at Done from the vehicle's first controlled tick only: the row
                    # in front of it is all zero (older vehicles lost the head of their buffer before tick `first`)
                    if len(b) >= window or tail or not obs_before(tr, b[0][0])[e, b[0][1]].any():
                        emit(b, t, slot, done, 0)
                    if done and tail:
                        for k in range(1, len(b)):
                            emit(b[k:], t, slot, True, k)
                    b = b[1:]
                to = int(tr.new_slot[t, e, slot])
                if to >= 0 and not done:
                    nxt[to] = b
            buf = nxt
    return out


def as_dict(index, target_of, tick0=0):
    """records of a pass -> {(absolute start tick, env, slot): (target, entries, bootstrapped, done)}"""
    out = {}
    for i, (t, e, s, c) in enumerate(np.asarray(index).tolist()):
        key = (t + tick0, e, s)
        assert key not in out, "start emitted twice: %r" % (key,)
        out[key] = (target_of(i), c & 0xFF, bool(c & 0x100), bool(c & 0x200))
    return out


def load_reference_fixture():
    """tests/golden/nstep_ref.npz (tests/golden/gen_nstep_golden.py: the unmodified reference under main.py:243-266's own
    buffers) -> (the file, the run's per-tick outputs as a segment dict [T, 1, K, ...])"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nstep_ref.npz"))
    T, K = int(z["T"]), int(z["K"])
    obs_post = np.zeros((T, 1, K, 28))
    state_pre = np.zeros((T, 1, K, 7, 28))
    obs_post[z["row_t"], 0, z["row_slot"]] = z["row_val"]
    state_pre[z["ctl_t"], 0, z["ctl_slot"], :, 2] = z["ctl_col2"]
    return z, dict(obs_post=obs_post, state_pre=state_pre, reward=z["reward"], flags=z["flags"], new_slot=z["new_slot"])

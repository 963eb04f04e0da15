"""NumPy restatement of the n-step transition pass (csrc/pve_nstep.h; reference main.py:243-266): the walk through new_slot,
the emit rule and the float64 backward Horner fold, for every candidate start at once.  Bit-equal to the device pass and to a
g++ build of the header by construction: every float64 operation below is one separately rounded NumPy operation, in the
header's order.

A segment is a dict of arrays with the leading shape [n_ticks, n_envs, cap]: obs_post [.., 28], state_pre [.., 7, 28] (float64
or float32), reward (float64), flags, new_slot (int32) -- what step_many(trajectory=...) returns, copied to the host.
Slot-indexed: for lane_num 4 / 8 the reference's `ids` order differs from slot order, which does not matter here.
"""
import numpy as np

F_CTL, F_DONE = 0x02, 0x04
TAIL = 0x1
MAX_WINDOW = 16
BOOT, DONE = 0x100, 0x200
RECORD = 36
KEYS = ("obs_post", "state_pre", "reward", "flags", "new_slot")


def _segments(cur, prev, window):
    n_cur = int(np.asarray(cur["flags"]).shape[0])
    n_prev = 0 if prev is None else int(np.asarray(prev["flags"]).shape[0])
    if not 1 <= window <= MAX_WINDOW:
        raise ValueError("window must be 1 .. 16")
    if n_cur < 1:
        raise ValueError("cur needs at least one tick")
    if 0 < n_prev < window:
        raise ValueError("prev must hold 0 or at least `window` ticks")
    return n_cur, n_prev


def scan(cur, gamma, window=13, prev=None, obs_first=None, q=None, tail=False):
    """-> (target float64 [n_cand, n_envs, cap], code int32 [n_cand, n_envs, cap], n_back): start-indexed, candidate tick c is
    tick c - n_back relative to cur.  code: entries used in bits 0-7, bit 8 bootstrapped, bit 9 closed by Done; 0 = none.
    q: float32 [n_ticks, n_envs, cap], the bootstrap Q of cur's ticks (bootstrap_q on cur's state_pre / flags)."""
    gamma = np.float64(gamma)
    if not (0.0 <= gamma <= 1.0):
        raise ValueError("gamma must lie in [0, 1]")
    n_cur, n_prev = _segments(cur, prev, window)
    n_back = min(n_prev, window - 1)
    if n_prev == 0 and obs_first is None:
        raise ValueError("obs_first is needed when there is no prev segment")

    def cat(key):
        c = np.asarray(cur[key])
        return c if n_prev == 0 else np.concatenate([np.asarray(prev[key])[n_prev - window:], c])
    flags, reward, new_slot = cat("flags"), cat("reward").astype(np.float64, copy=False), cat("new_slot")
    off = flags.shape[0] - n_cur                       # index of cur's tick 0 in the concatenated blocks
    rows = cat("obs_post") if n_prev else np.concatenate([np.asarray(obs_first)[None], np.asarray(cur["obs_post"])])
    roff = off - 1 if n_prev else 0                    # the s0 row of a start at tick t: rows[t + roff]
    _, E, K = flags.shape
    n_cand = n_back + n_cur
    t = np.broadcast_to(np.arange(-n_back, n_cur, dtype=np.int64)[:, None, None], (n_cand, E, K))
    env = np.broadcast_to(np.arange(E)[None, :, None], (n_cand, E, K))
    slot0 = np.broadcast_to(np.arange(K)[None, None, :], (n_cand, E, K))
    s = slot0.copy()
    s_last = s.copy()
    walking = np.ones((n_cand, E, K), bool)
    bad = np.zeros_like(walking)
    done = np.zeros_like(walking)
    n = np.zeros((n_cand, E, K), np.int32)
    r = np.zeros((window, n_cand, E, K), np.float64)
    for k in range(window):
        tk = t + k
        pend = walking & (tk >= n_cur)                 # pending: closes in a later call
        bad |= pend
        walking = walking & ~pend
        ti = np.where(walking, tk + off, 0)
        f = flags[ti, env, s]
        lost = walking & ((f & F_CTL) == 0)            # not (or no longer) a controlled vehicle
        bad |= lost
        walking = walking & ~lost
        r[k] = np.where(walking, reward[ti, env, s], 0.0)
        n = np.where(walking, k + 1, n).astype(np.int32)
        s_last = np.where(walking, s, s_last)
        d = walking & ((f & F_DONE) != 0)
        done |= d
        walking = walking & ~d
        if k + 1 < window:
            nxt = new_slot[ti, env, s]
            broken = walking & ((nxt < 0) | (nxt >= K))
            bad |= broken
            walking = walking & ~broken
            s = np.where(walking, nxt, s)
    t_close = t + n - 1
    ok = ~bad & (n > 0) & (t_close >= 0)
    full = n == window
    if not tail:
        fresh = ~(rows[np.where(ok, t + roff, 0), env, slot0] != 0).any(axis=-1)     # all-zero s0 row: first controlled tick
        ok &= full | fresh
    boot = ok & ~done
    qq = np.zeros((n_cand, E, K), np.float64)
    if boot.any():
        if q is None:
            raise ValueError("q is needed: a window of this trajectory is bootstrapped")
        qq = np.where(boot, np.asarray(q, np.float32)[np.where(boot, t_close, 0), env, s_last].astype(np.float64), 0.0)
    acc = np.zeros((n_cand, E, K), np.float64)
    for k in range(window - 1, -1, -1):
        gq = gamma * qq
        last = np.where(boot, r[k] + gq, r[k])
        ga = gamma * acc
        acc = np.where(k == n - 1, last, np.where(k < n - 1, r[k] + ga, acc))
    code = np.where(ok, n | np.where(boot, BOOT, 0) | np.where(done, DONE, 0), 0).astype(np.int32)
    target = np.where(ok, acc, 0.0)
    return target, code, n_back


def order(code):
    """Candidate indices (c, env, slot) of the records, in record order: (tick, env, slot) ascending."""
    return np.nonzero(code)


def records(cur, target, code, n_back, prev=None, obs_first=None):
    """-> (records float32 [M, 36] = s0 row [28], actions [7], target [1]; index int32 [M, 4] = tick relative to cur, env,
    slot, code)"""
    c, env, slot = order(code)
    t = c.astype(np.int64) - n_back
    M = len(c)
    rec = np.zeros((M, RECORD), np.float32)
    idx = np.stack([t, env, slot, code[c, env, slot]], axis=1).astype(np.int32).reshape(M, 4)
    n_prev = 0 if prev is None else int(np.asarray(prev["flags"]).shape[0])
    for i in range(M):
        ti, e, sl = int(t[i]), int(env[i]), int(slot[i])
        if ti > 0:
            row = np.asarray(cur["obs_post"])[ti - 1, e, sl]
        elif n_prev:
            row = np.asarray(prev["obs_post"])[n_prev + ti - 1, e, sl]
        else:
            row = np.asarray(obs_first)[e, sl]
        st = np.asarray(cur["state_pre"])[ti, e, sl] if ti >= 0 else np.asarray(prev["state_pre"])[n_prev + ti, e, sl]
        rec[i, :28] = row.astype(np.float32)
        rec[i, 28:35] = st[:, 2].astype(np.float32)            # column 2 of the 7 rows (ref :290)
        rec[i, 35] = np.float32(target[c[i], e, sl])
    return rec, idx


def nstep_transitions(cur, gamma, window=13, prev=None, obs_first=None, q=None, tail=False):
    """The whole pass -> (records, index, total)."""
    target, code, n_back = scan(cur, gamma, window, prev=prev, obs_first=obs_first, q=q, tail=tail)
    rec, idx = records(cur, target, code, n_back, prev=prev, obs_first=obs_first)
    return rec, idx, len(rec)

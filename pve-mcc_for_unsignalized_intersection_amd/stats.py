"""Roll-out and evaluation statistics by group of environments: the NumPy restatement of csrc/pve_stats.h (the definition),
bit for bit, and `summaries`, the quantities the reference watches while it trains (main.py:286-304), keeps its best
checkpoint by (main.py:315-328) and prints when it evaluates (main.py:413-415, :576-581).

The device pass is BatchedIntersections.rollout_stats / metrics_by_group (pve_rollout_stats / pve_metrics_groups)."""
import numpy as np

from . import _capi

STAT_NAMES = ("env_ticks", "alive", "spawned", "finished", "deleted", "collisions", "lock", "ctl", "collided", "done",
              "sum_reward", "sum_reward_sq", "sum_v", "sum_a")
STAT_N = len(STAT_NAMES)
COL = {n: k for k, n in enumerate(STAT_NAMES)}
# env_out index of the columns alive .. lock
_EO_OF_COLUMN = (0, 6, 5, 4, 2, 3)
_LANES = 64

# EnvHeader (csrc/pve_types.h): the per-environment header at the start of a handle's workspace
HEADER_DTYPE = np.dtype([("current_time", "<f8"), ("sum_reward", "<f8"), ("sum_jerk", "<f8"), ("next_arr", "<f8", (12,)),
                         ("alive_steps", "<i8"), ("ctl_steps", "<i8"), ("ticks", "<i8"), ("n_alive", "<i4"),
                         ("lane_start", "<i4", (13,)), ("veh_rec", "<i4", (12,)), ("id_seq", "<i4"), ("passed", "<i4"),
                         ("passed_step_total", "<i4"), ("head_valid", "<i4"), ("head_lane", "<i4", (16,)), ("head_j", "<i4", (16,)),
                         ("collided", "<i4"), ("locks", "<i4"), ("overflow", "<i4"), ("intention_re", "<i4")], align=True)


def _tree64(v):
    """tree64 of the header over the LAST axis (64 entries): neighbours first, v[l] = v[l] + v[l + w] for l a multiple of
    2 w, w = 1 .. 32."""
    assert v.shape[-1] == _LANES
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def env_rows(traj):
    """The per-(tick, env) rows [T, E, 14] (the scratch block of pve_rollout_stats).  traj: dict with flags [T, E, cap],
    reward, env_out [T, E, 8] and optionally obs_pre [T, E, cap, 28] (float64 or float32); [E, ...] blocks count as T = 1."""
    flags, reward, env_out = _np(traj["flags"]), _np(traj["reward"]), _np(traj["env_out"])
    obs = _np(traj["obs_pre"]) if traj.get("obs_pre") is not None else None
    if flags.ndim == 2:
        flags, reward, env_out = flags[None], reward[None], env_out[None]
        obs = obs[None] if obs is not None else None
    T, E, cap = flags.shape
    assert cap % _LANES == 0 and reward.shape == (T, E, cap) and env_out.shape == (T, E, 8) and reward.dtype == np.float64
    ctl = (flags & _capi.F_CTL) != 0
    x = np.zeros((T, E, STAT_N))
    x[..., COL["env_ticks"]] = 1.0
    for k, src in enumerate(_EO_OF_COLUMN):
        x[..., 1 + k] = env_out[..., src]
    x[..., COL["ctl"]] = ctl.sum(-1)
    x[..., COL["collided"]] = (ctl & ((flags >> 8) > 0)).sum(-1)
    x[..., COL["done"]] = (ctl & ((flags & _capi.F_DONE) != 0)).sum(-1)
    with np.errstate(all="ignore"):
        r = np.where(ctl, reward, 0.0)                       # a select: what a dead slot holds never reaches a sum
        vals = [r, r * r]
        for c in (1, 2):
            vals.append(np.where(ctl, obs[..., c].astype(np.float64), 0.0) if obs is not None else np.zeros_like(r))
    for k, v in enumerate(vals):
        v = v.reshape(T, E, cap // _LANES, _LANES)
        p = np.zeros((T, E, _LANES))
        for j in range(cap // _LANES):
            p = p + v[:, :, j, :]
        x[..., COL["sum_reward"] + k] = _tree64(p)
    return x


def group_rows(rows, groups=None, n_groups=1):
    """series [T, G, 14] of the env rows [T, E, 14]: chunks of 64 environments, tree64 per chunk, chunks in ascending order.
    An environment whose id is outside [0, G) is counted in no group."""
    T, E, _ = rows.shape
    g_of = np.zeros(E, np.int64) if groups is None else _np(groups).astype(np.int64)
    assert g_of.shape == (E,)
    chunks = (E + _LANES - 1) // _LANES
    pad = np.zeros((T, chunks * _LANES, STAT_N))
    pad[:, :E] = rows
    gp = np.full(chunks * _LANES, -1, np.int64)
    gp[:E] = g_of
    series = np.zeros((T, n_groups, STAT_N))
    for g in range(n_groups):
        m = np.where((gp == g)[None, :, None], pad, 0.0).reshape(T, chunks, _LANES, STAT_N)
        q = _tree64(np.moveaxis(m, 2, -1))                   # [T, chunks, 14]
        s = np.zeros((T, STAT_N))
        for j in range(chunks):
            s = s + q[:, j]
        series[:, g] = s
    return series


def add_totals(totals, series):
    """totals [G, 14] + series[t] for t ascending (what a call with `totals` does on the device); returns the new totals."""
    tot = np.array(totals, np.float64, copy=True)
    for t in range(series.shape[0]):
        tot = tot + series[t]
    return tot


def rollout_stats(traj, groups=None, n_groups=1):
    """series [T, G, 14] float64 of retained roll-out blocks, bit-equal to pve_rollout_stats (csrc/pve_stats.h)."""
    return group_rows(env_rows(traj), groups, n_groups)


def headers_of(batch):
    """The EnvHeaders of a batch as a structured array [n_envs] (a host copy of the start of its workspace; for tests and
    tools -- the device path is metrics_by_group)."""
    n = batch.n_envs * HEADER_DTYPE.itemsize
    return np.frombuffer(batch.workspace[:n].cpu().numpy().tobytes(), dtype=HEADER_DTYPE)


def metrics_groups(headers, capacity, groups=None, n_groups=1):
    """out [G, 12] float64 (the order of _capi.METRIC_NAMES) from the headers, bit-equal to pve_metrics_groups: integer sums
    converted once; sum_reward / sum_jerk added in ascending environment index."""
    E = len(headers)
    g_of = np.zeros(E, np.int64) if groups is None else _np(groups).astype(np.int64)
    out = np.zeros((n_groups, _capi.PVE_N_METRICS))
    for g in range(n_groups):
        h = headers[g_of == g]
        ticks = int(h["ticks"].astype(np.int64).sum())
        out[g] = [ticks * capacity, int(h["alive_steps"].sum()), int(h["ctl_steps"].sum()), int(h["id_seq"].astype(np.int64).sum()),
                  int(h["passed"].astype(np.int64).sum()), int(h["collided"].astype(np.int64).sum()), int(h["locks"].astype(np.int64).sum()),
                  0.0, 0.0, int(h["passed_step_total"].astype(np.int64).sum()), int(h["overflow"].astype(np.int64).sum()), ticks]
        sr = sj = np.float64(0.0)
        for r, j in zip(h["sum_reward"], h["sum_jerk"]):
            sr, sj = sr + r, sj + j
        out[g, 7], out[g, 8] = sr, sj
    return out


def summaries(x):
    """The reference's quantities from series / totals ([..., 14], array or tensor): a dict of arrays of the leading shape.
    v_mean, acc_mean (main.py:290, :294), reward_mean, reward_std (np.mean / np.std of main.py:413-415: the population
    standard deviation) are over controlled vehicles; collisions (main.py:287), collided (main.py:276-278), collision_rate =
    collided / spawned (main.py:315) and lock follow.  An empty denominator gives nan."""
    x = _np(x).astype(np.float64)
    assert x.shape[-1] == STAT_N
    with np.errstate(all="ignore"):
        n = np.where(x[..., COL["ctl"]] > 0, x[..., COL["ctl"]], np.nan)
        mean = x[..., COL["sum_reward"]] / n
        var = np.maximum(x[..., COL["sum_reward_sq"]] / n - mean * mean, 0.0)
        spawned = np.where(x[..., COL["spawned"]] > 0, x[..., COL["spawned"]], np.nan)
        return dict(v_mean=x[..., COL["sum_v"]] / n, acc_mean=x[..., COL["sum_a"]] / n, reward_mean=mean, reward_std=np.sqrt(var),
                    collisions=x[..., COL["collisions"]], collided=x[..., COL["collided"]],
                    collision_rate=x[..., COL["collided"]] / spawned, lock=x[..., COL["lock"]],
                    ctl=x[..., COL["ctl"]], spawned=x[..., COL["spawned"]], finished=x[..., COL["finished"]])

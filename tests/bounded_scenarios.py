"""Full intersections: the kernels against CAPACITY-BOUND oracles, through every deferred spawn.

The sequential oracles (oracle/pve_oracle.c, oracle/pve_oracle_geo.c) spawn without limit, as the reference does; built with
`capacity=` they defer the spawns a batched env of that many slots has no room for, by the rule of ph_final (csrc/pve_tick_core.h,
csrc/pve_tick_geo.h):

  room = capacity - (vehicles alive at tick start)   -- this tick's deletions free nothing until the next tick;
  more lanes due than room: the lowest lane indices are granted;
  a deferred lane keeps its cursor (veh_rec), draws no intention, gets no id and is due again on the next tick;
  `overflow` grows by the number of deferred lanes per tick.

tests/test_oracle_bounded.py pins that rule to the unbounded oracle and to the live reference (a bounded run == an unbounded run
on the arrival stream rewritten to the grant times).  Here one bounded oracle run per scenario (computed once, shared by the
tests that need it) is the record every launch form is held to: ints exact, floats at oracle.record.close 1e-9.

A scenario's action tape is indexed by (tick, slot) (a pool of n_pool entries: what pve_step_many(PVE_SRC_POOL) reads) or by
(tick, vehicle id) (PVE_SRC_TABLE), so the oracle runs ahead of the backend and the scenario's non-vacuity -- deferrals in every
env, partial grants, deferrals in ticks that also delete, a lane starved for 3 ticks, collisions, dead-locks -- is asserted from
the oracle alone before a backend is judged.
"""
import collections
import functools

import numpy as np
import torch

from oracle.oracle import OracleEnv
from oracle.oracle_geo import OracleGeoEnv
from oracle.record import close, compare_records
from pve_mcc_amd import _capi
from pve_mcc_amd.arrivals import synthetic_arrivals, synthetic_intentions
from tests.hip_adapter import SplitEnv, _np, make_batch, state_snapshot

EO = {n: i for i, n in enumerate(_capi.ENV_OUT_NAMES)}

_Scn = collections.namedtuple("Scn", "lane_num capacity n_envs ticks rate seed tape lo hi quantize n_pool cfg min_gap")


def Scn(lane_num, capacity, n_envs, ticks, rate, seed, tape="pool", lo=-3.0, hi=3.0, quantize=None, n_pool=16, cfg=(), min_gap=1.0):
    """tape: "pool" = actions by (tick % n_pool, slot), "table" = by (tick % 23, min(id, 149)); uniform in [lo, hi], rounded to
    float32, optionally quantised (exact ties).  cfg: constructor arguments as a tuple of (name, value) pairs.
    min_gap: the shortest headway of a lane's arrivals in seconds (synthetic_arrivals clips at 1 s: four lanes cannot fill
    128 slots at that)."""
    return _Scn(lane_num, capacity, n_envs, ticks, rate, seed, tape, lo, hi, quantize, n_pool, tuple(cfg), min_gap)


# Streams chosen on the CPU (oracle alone) so that every condition of _non_vacuity holds; tests/test_oracle_bounded.py lists the
# counts.  12 lanes: the 12-lane oracle and the fast path / PVE_CFG_GENERAL_PATH; 4 / 8 lanes: the general-geometry oracle.
S12_64 = Scn(12, 64, 3, 300, 1500.0, 7)
S12_64_Q = Scn(12, 64, 3, 300, 1500.0, 7, quantize=0.5)
S12_64_TABLE = Scn(12, 64, 3, 300, 1500.0, 7, tape="table")
S12_128 = Scn(12, 128, 3, 400, 6000.0, 7)
S12_128_TABLE = Scn(12, 128, 3, 400, 6000.0, 7, tape="table")
S12_256 = Scn(12, 256, 3, 350, 5000.0, 2561, lo=-3.0, hi=-1.0)        # (cap256_scenarios' stream seed, a braking tape)
S4_64 = Scn(4, 64, 3, 300, 7200.0, 9, min_gap=0.5)
S4_128 = Scn(4, 128, 3, 300, 18000.0, 9, min_gap=0.2, cfg=(("collision_thr", 1.0),))   # (four lanes fill 128 slots only at short headways)
S8_64 = Scn(8, 64, 3, 300, 3000.0, 9)
S8_128 = Scn(8, 128, 3, 350, 6000.0, 9)


class OracleRun:
    """arr / ch / pool_np / table_np: the scenario's inputs; recs[t][e]: the bounded oracle's record of tick t of env e (plus
    n_pre, id_seq_pre, veh_rec_pre, intention_re); final[e]: its vehicles after the last tick; overflow[e]; stats."""


def _actions(run, t, e, vid, ctl):
    if run.scn.tape == "table":
        tab = run.table_np
        a = tab[t % tab.shape[0], np.minimum(vid, tab.shape[1] - 1)]
    else:
        a = run.pool_np[t % run.scn.n_pool, e, :len(vid)]
    return np.where(ctl != 0, a, 0.0)


def make_oracles(run, capacity="scn"):
    scn = run.scn
    cap = scn.capacity if capacity == "scn" else capacity
    cfg = dict(scn.cfg)
    if scn.lane_num == 12:
        return [OracleEnv(run.arr[e], capacity=cap, **cfg) for e in range(scn.n_envs)]
    return [OracleGeoEnv(run.arr[e], scn.lane_num, choice=None if run.ch is None else run.ch[e], capacity=cap, **cfg)
            for e in range(scn.n_envs)]


def scenario_inputs(scn):
    run = OracleRun()
    run.scn = scn
    rng = np.random.default_rng(scn.seed)
    run.arr = synthetic_arrivals(scn.n_envs, rate=scn.rate, horizon_s=scn.ticks * 0.1 + 30, seed=scn.seed, lane_num=scn.lane_num)
    if scn.min_gap != 1.0:          # the same clipped-exponential shape with a shorter clip
        for e in range(scn.n_envs):
            dt = np.maximum(scn.min_gap, np.random.default_rng(scn.seed + e).exponential(3600.0 / scn.rate, size=(run.arr.shape[1] - 1, scn.lane_num)))
            run.arr[e, :-1, :] = np.cumsum(dt, axis=0)
    run.ch = synthetic_intentions(scn.n_envs, run.arr.shape[1], seed=scn.seed, lane_num=8) if scn.lane_num == 8 else None
    pool = rng.uniform(scn.lo, scn.hi, size=(scn.n_pool, scn.n_envs, scn.capacity)).astype(np.float32).astype(np.float64)
    table = rng.uniform(scn.lo, scn.hi, size=(23, 150)).astype(np.float32).astype(np.float64)
    if scn.quantize:
        pool, table = np.round(pool / scn.quantize) * scn.quantize, np.round(table / scn.quantize) * scn.quantize
    run.pool_np, run.table_np = pool, table
    return run


def _non_vacuity(run):
    """From the bounded oracle's records alone: what makes a scenario able to tell the rule from its near misses."""
    scn = run.scn
    tot = collections.Counter()
    per_env = []
    for e in range(scn.n_envs):
        c = collections.Counter()
        streak = [0] * scn.lane_num
        for t in range(scn.ticks):
            r = run.recs[t][e]
            granted = r["id_seq"] - r["id_seq_pre"]
            c["collisions"] += r["collisions"]
            c["locks"] += r["lock"]
            for l in range(scn.lane_num):
                streak[l] = streak[l] + 1 if (r["deferred_lanes"] >> l) & 1 else 0
                c["longest_starved"] = max(c["longest_starved"], streak[l])
            if r["deferred"] > 0:
                c["deferring_ticks"] += 1
                c["partial_grants"] += 1 if granted > 0 else 0          # 0 < granted < due = granted + deferred
                c["deferred_while_deleting"] += 1 if len(r["deleted"]) > 0 else 0
        c["overflow"] = run.overflow[e]
        assert c["overflow"] > 0 and c["deferring_ticks"] > 0, "%s: env %d never defers a spawn" % (scn, e)
        per_env.append(dict(c))
        for k, v in c.items():
            tot[k] = max(tot[k], v) if k == "longest_starved" else tot[k] + v
    assert tot["partial_grants"] >= 1, "%s: no tick grants some of the due lanes and defers the others" % (scn,)
    assert tot["deferred_while_deleting"] >= 1, "%s: no tick defers a spawn while it deletes a vehicle" % (scn,)
    assert tot["longest_starved"] >= 3, "%s: no lane stays deferred for 3 ticks" % (scn,)
    assert tot["collisions"] >= 1 and tot["locks"] >= 1, "%s: %d collisions, %d dead-locks" % (scn, tot["collisions"], tot["locks"])
    return dict(tot), per_env


_KEEP = ("time", "ids", "nbr", "reward", "obs0", "coll_pv", "collisions", "lock", "jerks", "deleted", "veh_i", "veh_f", "id_seq",
         "passed", "passed_step_total", "veh_num", "veh_rec", "heads", "overflow", "deferred", "deferred_lanes", "intent", "intention_re")


@functools.lru_cache(maxsize=2)
def oracle_run(scn):
    """The bounded oracle's run of a scenario (every env, every tick), with the non-vacuity conditions asserted."""
    run = scenario_inputs(scn)
    oracles = make_oracles(run)
    run.recs = []
    for t in range(scn.ticks):
        row = []
        for e, o in enumerate(oracles):
            vid, ctl, _ = o.alive_view()
            pre = o.snapshot()
            rec = o.tick(_actions(run, t, e, vid, ctl))
            rec = {k: rec[k] for k in _KEEP if k in rec}
            rec.update(tick=t, state=None, act7=None, n_pre=len(vid), id_seq_pre=pre["id_seq"], veh_rec_pre=pre["veh_rec"])
            row.append(rec)
        run.recs.append(row)
    run.final = [o.vehicles() for o in oracles]
    run.overflow = [o.overflow for o in oracles]
    assert all(o.ref_would_raise == 0 for o in oracles)
    run.stats, run.env_stats = _non_vacuity(run)
    return run


def rewritten_arrivals(run, e):
    """The arrival stream of env e as the bounded run served it: every entry that was granted late carries the time of its
    grant tick, every entry still waiting at the end +inf.  The reference reads an arrival time only in
    `current_time >= arrive[veh_rec][lane]` (ref :379), so an UNBOUNDED run on this stream must equal the bounded run."""
    scn = run.scn
    arr = np.array(run.arr[e], copy=True)
    late = set()
    for t in range(scn.ticks):
        r = run.recs[t][e]
        for l in range(scn.lane_num):
            row = int(r["veh_rec_pre"][l])
            if (r["deferred_lanes"] >> l) & 1:
                assert int(r["veh_rec"][l]) == row, "a deferred lane advanced its cursor"
                late.add((row, l))
            elif int(r["veh_rec"][l]) == row + 1 and (row, l) in late:
                arr[row, l] = r["time"]
                late.discard((row, l))
    for row, l in late:
        arr[row, l] = np.inf
    return arr, len(late)


# ---------------------------------------------------------------- one tick of one env against its record
def _expected_new_slot(rec):
    """pre slot -> post slot of a fused tick, from the record (snapshot before delete_vehicle, spawns included)."""
    vi = rec["veh_i"]
    spawn = vi[:, 2] >= rec["id_seq_pre"]
    dele = np.zeros(len(vi), bool)
    if len(rec["deleted"]):
        key = vi[:, 0].astype(np.int64) * 65536 + vi[:, 1]
        dele = np.isin(key, rec["deleted"][:, 0].astype(np.int64) * 65536 + rec["deleted"][:, 1])
    post = np.cumsum(~dele) - 1
    return np.where(dele, -1, post)[~spawn], int((~dele).sum()), dele


def compare_tick(rec, o, what, split=False, rows="pre"):
    """o: this tick's outputs of one env (numpy: flags, lanej, nbr, reward, env_out, new_slot, obs_pre | obs_post)."""
    n = rec["n_pre"]
    eo = o["env_out"]
    f = o["flags"].astype(np.int64)
    assert int(eo[EO["n_pre"]]) == n, "%s: n_pre %d vs %d" % (what, eo[EO["n_pre"]], n)
    assert np.all((f[:n] & _capi.F_ALIVE) != 0) and np.all(f[n:] == 0), what + ": alive flags"
    f = f[:n]
    lj = o["lanej"][:n].astype(np.int64)
    order = np.lexsort((lj & 0xFFFF, (f >> _capi.F_INTENT_SHIFT) & 3, lj >> 16)) if n else np.zeros(0, np.int64)
    ctl = order[((f & _capi.F_CTL) != 0)[order]]
    assert len(ctl) == len(rec["ids"]) == int(eo[EO["n_ctl"]]), what + ": controlled set"
    assert np.array_equal(np.stack([lj[ctl] >> 16, lj[ctl] & 0xFFFF], -1), rec["ids"]), what + ": ids"
    assert int(eo[EO["collisions"]]) == rec["collisions"] and int(eo[EO["lock"]]) == rec["lock"], what + ": counters"
    assert np.array_equal(f[ctl] >> 8, rec["coll_pv"]), what + ": coll_pv"
    nb = o["nbr"][:n][ctl].astype(np.int64)
    nb = np.stack([np.where(nb < 0, -1, nb >> 16), np.where(nb < 0, -1, nb & 0xFFFF)], -1)
    assert np.array_equal(nb, rec["nbr"]), what + ": neighbours"
    assert close(rec["reward"], o["reward"][:n][ctl], 1e-9), what + ": reward"
    dl = order[((f & _capi.F_DELETED) != 0)[order]]
    assert np.array_equal(np.stack([lj[dl] >> 16, lj[dl] & 0xFFFF], -1).reshape(-1, 2), rec["deleted"]), what + ": deleted"
    assert int(eo[EO["n_deleted"]]) == len(rec["deleted"]) and int(eo[EO["n_finished"]]) == len(rec["jerks"]), what + ": n_deleted / n_finished"
    # the capacity bound: who spawned, and where
    granted = rec["id_seq"] - rec["id_seq_pre"]
    assert int(eo[EO["n_spawned"]]) == granted, "%s: N_SPAWNED %d vs %d granted (%d deferred)" % (what, eo[EO["n_spawned"]], granted, rec["deferred"])
    want_slot, n_post, _ = _expected_new_slot(rec)
    assert int(eo[EO["n_post"]]) == (len(rec["veh_i"]) if split else n_post), what + ": N_POST"
    if not split:
        ns = o["new_slot"][:n]
        assert np.array_equal(ns, want_slot), what + ": new_slot"
        if rows == "post":
            kept = ns[ctl] >= 0
            assert close(rec["obs0"][kept], o["obs_post"][ns[ctl][kept]], 1e-9), what + ": obs rows (post)"
    if rows == "pre":
        assert close(rec["obs0"], o["obs_pre"][:n][ctl], 1e-9), what + ": obs rows (pre)"


def compare_header(rec, info, what, lane_num, split=False):
    """read_env after the tick: the spawn cursors, the id counter, the intention counter, the deferral count."""
    assert info.id_seq == rec["id_seq"], "%s: id_seq %d vs %d" % (what, info.id_seq, rec["id_seq"])
    assert list(info.veh_rec)[:lane_num] == rec["veh_rec"].tolist(), what + ": veh_rec"
    assert info.overflow == rec["overflow"], "%s: overflow %d vs %d" % (what, info.overflow, rec["overflow"])
    if lane_num != 12:
        assert info.intention_re == rec["intention_re"], what + ": intention_re"
    _, n_post, dele = _expected_new_slot(rec)
    lanes = rec["veh_i"][:, 0] if split else rec["veh_i"][~dele, 0]
    assert info.n_alive == len(lanes), what + ": n_alive"
    assert list(info.lane_count)[:lane_num] == np.bincount(lanes, minlength=lane_num).tolist(), what + ": lane_count"
    assert info.passed_veh == rec["passed"] and info.passed_veh_step_total == rec["passed_step_total"], what + ": passed"


def compare_final(run, b, what):
    """the persistent state after the last tick, field by field, and the deferral count of the metrics vector"""
    scn = run.scn
    for e in range(scn.n_envs):
        info, vi, vf = state_snapshot(b, e)
        ovi, ovf = run.final[e][0], run.final[e][1]
        assert np.array_equal(vi[:, :13], ovi[:, :13]), "%s: final state ints, env %d" % (what, e)
        assert close(ovf[:, :5], vf[:, :5], 1e-9), "%s: final state floats, env %d" % (what, e)
        compare_header(dict(run.recs[-1][e], veh_i=ovi, deleted=np.zeros((0, 2), np.int32)), info, "%s: final header, env %d" % (what, e),
                       scn.lane_num)
        if scn.lane_num != 12:
            got = np.array([[v.intention, v.route] for v in b.read_vehicles(e)], np.int32).reshape(-1, 2)
            assert np.array_equal(got, run.final[e][3]), "%s: intentions / routes, env %d" % (what, e)
    m = b.metrics()
    assert m["overflow"] == sum(run.overflow) > 0, "%s: metrics overflow %r vs the oracles' %d" % (what, m["overflow"], sum(run.overflow))
    assert m["spawned"] == sum(run.recs[-1][e]["id_seq"] for e in range(scn.n_envs)), what + ": metrics spawned"
    return m


def _batch(run, backend, outputs, **bkw):
    scn = run.scn
    kw = dict(scn.cfg)
    kw.update(bkw)
    if scn.lane_num != 12:
        kw.update(lane_num=scn.lane_num, intentions=run.ch)
    b = make_batch(run.arr, scn.n_envs, scn.capacity, backend, outputs=outputs, **kw)
    b.reset()
    if scn.tape == "table":
        b.set_action_table(torch.as_tensor(run.table_np))
    return b


def _tick_actions(run, b, pool_dev, t):
    return b.actions_from_table() if run.scn.tape == "table" else pool_dev[t % run.scn.n_pool]


# ---------------------------------------------------------------- checkers
def check_fused_bounded(backend, scn, **bkw):
    """pve_step_all, one call per tick: every tick's outputs and header against the bounded oracle's record, through every
    deferred spawn; the full state and metrics()["overflow"] at the end.  bkw: general_path / geo_scan."""
    run = oracle_run(scn)
    outs = ("obs_post", "obs_pre", "reward", "flags", "nbr", "env_out", "new_slot", "lanej")
    b = _batch(run, backend, outs, **bkw)
    pool_dev = torch.as_tensor(run.pool_np).to(b.device)
    for t in range(scn.ticks):
        out = b.step(_tick_actions(run, b, pool_dev, t))
        host = {k: _np(out[k]) for k in outs if k != "obs_post"}
        for e in range(scn.n_envs):
            what = "fused tick %d env %d" % (t, e)
            compare_tick(run.recs[t][e], {k: v[e] for k, v in host.items()}, what)
            compare_header(run.recs[t][e], b.read_env(e), what, scn.lane_num)
    return compare_final(run, b, "fused"), run.stats


def check_split_bounded(backend, scn, **bkw):
    """pve_scene_update + pve_compact (the reference's call sequence): the canonical record of every tick, every field, against
    the bounded oracle's; room is measured at tick start in this mode too (the Done vehicles still hold their slots)."""
    run = oracle_run(scn)
    outs = ("obs_post", "obs_pre", "reward", "flags", "nbr", "env_out", "new_slot", "lanej")
    b = _batch(run, backend, outs, **bkw)
    envs = [SplitEnv(b, e) for e in range(scn.n_envs)]
    pool_dev = torch.as_tensor(run.pool_np).to(b.device)
    for t in range(scn.ticks):
        # (the split protocol applies the caller's action to every vehicle, as the reference's step() does; the caller passes 0 for
        #  the uncontrolled ones, main.py:401 -- pve_step_all / pve_step_many do that themselves)
        ctl = (b.state_field("meta") & 1) != 0
        out = b.scene_update(torch.where(ctl, _tick_actions(run, b, pool_dev, t), torch.zeros((), dtype=torch.float64, device=b.device)).contiguous())
        b.synchronize()
        host = {k: _np(out[k]) for k in outs if k != "obs_post"}
        for e, env in enumerate(envs):
            what = "split tick %d env %d" % (t, e)
            rec = run.recs[t][e]
            got = env.record(out)
            got["tick"] = t
            compare_records(rec, got, tol=1e-9, label="split env %d" % e)
            if scn.lane_num != 12:
                assert np.array_equal(rec["intent"], got["intent"]) and rec["intention_re"] == got["intention_re"], what + ": intentions"
            compare_tick(rec, {k: v[e] for k, v in host.items()}, what, split=True)
            compare_header(rec, b.read_env(e), what, scn.lane_num, split=True)
        b.compact()
    return compare_final(run, b, "split"), run.stats


def check_rollout_bounded(backend, scn, persistent=False, chunk=0, calls=None, rows="pre", want_launch=None, **bkw):
    """pve_step_many trajectory roll-outs: the retained blocks (flags, reward, env_out, new_slot, lanej, nbr and the observation
    rows) of EVERY tick directly against the bounded oracle's records -- no single-tick twin in between -- across call and chunk
    boundaries; header, state and metrics after the last call.  rows="post": without the training outputs (the HOME build of
    the 128-slot queue form runs only then); the rows are read from obs_post through new_slot."""
    run = oracle_run(scn)
    outs = ("obs_post", "reward", "flags", "nbr", "env_out", "new_slot", "lanej") + (("obs_pre",) if rows == "pre" else ())
    b = _batch(run, backend, outs, **bkw)
    source = scn.tape
    if source == "pool":
        b.set_action_pool(torch.as_tensor(run.pool_np))
    if calls is None:
        q = scn.ticks // 4
        calls = (q, q + 3, 1, scn.ticks - 2 * q - 4)
    assert sum(calls) == scn.ticks
    ring = [b.alloc_trajectory(max(calls)) for _ in range(2)]
    keys = [k for k in outs if k != ("obs_post" if rows == "pre" else "")]
    t = 0
    for ci, n in enumerate(calls):
        traj = b.step_many(n, source=source, trajectory=ring[ci & 1], chunk=chunk, persistent=persistent)
        b.synchronize()
        if want_launch is not None:
            want = want_launch if (not persistent or 0 < chunk < n) else "resident"
            assert b.last_launch() == want, (b.last_launch(), want, n, chunk)
        host = {k: _np(traj[k][:n]) for k in keys}
        for k in range(n):
            for e in range(scn.n_envs):
                compare_tick(run.recs[t + k][e], {x: v[k, e] for x, v in host.items()}, "roll-out tick %d env %d" % (t + k, e), rows=rows)
        t += n
        for e in range(scn.n_envs):
            rec = run.recs[t - 1][e]
            compare_header(rec, b.read_env(e), "after the call that ends at tick %d, env %d" % (t, e), scn.lane_num)
    return compare_final(run, b, "roll-out"), run.stats


def check_closed_loop_full(backend, capacity, n_envs=4, ticks=300, rate=None, seed=7, chunk=13):
    """PVE_SRC_ACTOR on a batch that fills every slot: the persistent form, the resident form and the two-launch form
    (step_with_actor) must be BIT-equal to each other through the deferred spawns, overflow > 0 in every env.
    A SELF-comparison by necessity: the float32 actor's actions cannot be held to the FP64 oracle at 1e-9, and an action that
    differs in its last bit moves who is alive when a spawn is due.  The deferral rule itself is held to the bounded oracle by
    every other checker of this module, on the same ph_final."""
    from oracle.actor_np import flat_weights, load_weights
    from tests.scenarios import batches_equal
    rate = rate or {64: 1500.0, 128: 6000.0}[capacity]
    arr = synthetic_arrivals(n_envs, rate=rate, horizon_s=ticks * 0.1 + 30, seed=seed)
    outs = ("obs_post", "reward", "flags", "nbr", "new_slot", "env_out", "lanej")
    two, res, per = (make_batch(arr, n_envs, capacity, backend, outputs=outs) for _ in range(3))
    w = flat_weights(load_weights())
    for b in (two, res, per):
        b.reset()
        b.set_actor(w)
    calls = (ticks // 2, ticks - ticks // 2)
    for n in calls:
        for _ in range(n):
            o1 = two.step_with_actor()
        o2 = res.step_many(n, actor=True)
        o3 = per.step_many(n, actor=True, chunk=chunk, persistent=True)
        for b in (two, res, per):
            b.synchronize()
        if backend != "emu":
            assert res.last_launch() == "resident" and per.last_launch() == "persistent", (res.last_launch(), per.last_launch())
        for b, o, what in ((res, o2, "resident"), (per, o3, "persistent")):
            batches_equal(two, b, "closed loop, %s form vs two launches" % what)
            f = _np(o1["flags"])
            assert np.array_equal(f, _np(o["flags"])) and np.array_equal(_np(o1["env_out"]), _np(o["env_out"])), what
            alive = (f & 1) != 0
            for k in ("reward", "new_slot", "lanej"):
                assert np.array_equal(_np(o1[k])[alive], _np(o[k])[alive]), "%s: %s" % (what, k)
    m = two.metrics()
    for b in (res, per):
        mb = b.metrics()
        for k in m:
            assert m[k] == mb[k], (k, m[k], mb[k])
    assert all(two.read_env(e).overflow > 0 for e in range(n_envs)), [two.read_env(e).overflow for e in range(n_envs)]
    return m

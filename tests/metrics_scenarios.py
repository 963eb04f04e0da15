"""Scenarios that hold BatchedIntersections.metrics() to the reference accumulator (tests/metrics_ref.py), shared by the CPU file
(tests/test_metrics.py: the emulator, and the reach conditions on the oracle side alone) and the `-m gpu` file
(tests/test_gpu_metrics.py: the real kernels, whose block reductions exist on the device only).

An open-loop scenario is a batch of burst arrival streams (every lane spawns every `gap` seconds for `dur` seconds, then the
stream is dry) and a tape that is a function of (tick, vehicle id).  The sequential oracle runs it ONCE (reference(): cached),
feeds one accumulator per intersection and records the slot-indexed actions of every tick; every launch form of the device is
then driven by that record -- step(actions), scene_update + compact, or step_many from the pool (the record itself), the table
(the tape by (tick, id)) or the zero source -- and its metrics() vector is compared at the end of every segment (`calls`).
The closed loop cannot be taped in advance: there the device's own actions are read back tick by tick and drive the oracle."""
import collections

import numpy as np
import torch

from oracle.record import get_policy
from pve_mcc_amd.arrivals import synthetic_arrivals, synthetic_intentions
from tests import metrics_ref
from tests.hip_adapter import _np, make_batch

OUTS = ("obs_post", "reward", "flags", "nbr", "new_slot", "env_out", "lanej")
TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")


def burst_arrivals(lane_num, gap, dur, seed, t0=1.0):
    """[rows, lane_num]: per lane one vehicle every `gap` s (jittered) from t0 for `dur` s, then +inf: a stream that runs dry."""
    n = int(round(dur / gap))
    out = np.full((n + 2, lane_num), np.inf)
    if n:
        rng = np.random.default_rng(seed)
        for l in range(lane_num):
            out[:n, l] = t0 + rng.uniform(0, gap) + gap * np.arange(n) + rng.uniform(0, 0.3 * gap, n)
    return out


# name -> (lane_num, capacity, [(gap, dur, seed) per intersection; dur 0 = empty for the whole run], calls, tape, cfg)
Spec = collections.namedtuple("Spec", "name lane_num capacity envs calls tape cfg")


def _ctor_of(case_name):
    """constructor arguments of a golden fixture"""
    from tests.parity_util import GoldenCase
    return dict(GoldenCase(case_name).ctor)


SPECS = {s.name: s for s in [
    # 12 lanes: one, two and four waves
    Spec("l12_c64", 12, 64, [(1.0, 4.0, 11)], (150, 7, 243), "rand3", {}),
    Spec("l12_c128", 12, 128, [(0.5, 4.5, 12), (1.0, 4.0, 13)], (120, 7, 283), "rand3", {}),
    Spec("l12_c256", 12, 256, [(0.3, 6.0, 14)], (130, 7, 363), "rand3", {}),
    Spec("l12_c128_zero", 12, 128, [(0.5, 4.5, 12), (1.0, 4.0, 13)], (120, 7, 173), "zero", {}),
    # very different populations in one batch: empty for the whole run, dry after a few vehicles, medium, dense, sparse
    Spec("l12_c128_five", 12, 128, [(1.0, 0.0, 0), (1.0, 2.0, 21), (0.5, 4.5, 22), (0.45, 4.5, 23), (3.0, 24.0, 24)], (120, 7, 283),
         "rand3", {}),
    # 4 / 8 lanes
    Spec("l4_c64", 4, 64, [(0.5, 9.0, 31)], (150, 7, 243), "rand3", {}),
    Spec("l4_c128", 4, 128, [(0.4, 12.0, 32), (1.0, 8.0, 33)], (150, 7, 243), "rand3", {}),
    Spec("l8_c64", 8, 64, [(1.0, 6.0, 34)], (150, 7, 243), "rand3", {}),
    Spec("l8_c128", 8, 128, [(0.5, 6.0, 35), (1.0, 6.0, 36)], (150, 7, 243), "rand3", {}),
    Spec("l4_c128_kw", 4, 128, [(0.4, 12.0, 37)], (150, 7, 243), "rand3", "geo_g4_rand_kw"),
    Spec("l8_c64_kw", 8, 64, [(1.0, 6.0, 38)], (150, 7, 243), "rand3", "geo_g8_rand_kw"),
]}


# Full intersections: bursts that want more slots than the capacity has.  The oracles of these run capacity-bound (the deferral
# rule of ph_final, pinned to the reference by tests/test_oracle_bounded.py), the accumulators take every tick's deferral count
# from their records; once the streams are dry the lanes that were kept waiting drain.  One per kernel family.
FULL_SPECS = {s.name: s for s in [
    Spec("l12_c64_full", 12, 64, [(0.5, 9.0, 41), (0.8, 8.0, 42)], (150, 7, 243), "rand3", {}),
    Spec("l12_c128_full", 12, 128, [(0.3, 12.0, 45), (0.4, 12.0, 46)], (150, 7, 243), "rand3", {}),       # (the HOME build's width)
    Spec("l4_c64_full", 4, 64, [(0.2, 9.0, 43)], (150, 7, 243), "rand3", {}),
    Spec("l8_c64_full", 8, 64, [(0.4, 9.0, 44)], (150, 7, 243), "rand3", {}),
]}


def spec_cfg(spec):
    return _ctor_of(spec.cfg) if isinstance(spec.cfg, str) else dict(spec.cfg)


def make_oracle(arr, lane_num, choice=None, **cfg):
    if lane_num == 12:
        from oracle.oracle import OracleEnv
        return OracleEnv(arr, **cfg)
    from oracle.oracle_geo import OracleGeoEnv
    return OracleGeoEnv(arr, lane_num, choice=choice, **cfg)


class TickStats:
    """What a scenario contains, from the oracle's records alone (the reach conditions of tests/test_metrics.py)."""

    def __init__(self, capacity):
        self.nw = capacity // 64
        self.pops = []
        self.collided = self.locks = self.rew_ovr = self.two_fin_waves = self.skip_and_tree = self.no_ctl = self.max_ctl = 0
        self.ctl_two_waves = 0
        self._finished = set()

    def add(self, rec, pre_ids):
        n_pre = len(pre_ids)
        self.pops.append(n_pre)
        coll = np.asarray(rec["coll_pv"]) > 0
        self.collided += int(coll.sum())
        self.locks += int(rec["lock"])
        # -10 on a vehicle that did not collide itself: the reference's reward[-1] of a collided uncontrolled vehicle (ref :346)
        self.rew_ovr += int(((np.asarray(rec["reward"]) == -10.0) & ~coll).sum())
        n_ctl = len(rec["ids"])
        self.no_ctl += int(n_ctl == 0)
        self.max_ctl = max(self.max_ctl, n_ctl)
        vi = rec["veh_i"]
        pre = vi[np.isin(vi[:, 2], pre_ids)]            # (the snapshot also holds this tick's spawns, at the lane ends)
        assert len(pre) == n_pre
        fin_now = [(s, int(r[2])) for s, r in enumerate(pre) if r[6] and int(r[2]) not in self._finished]
        assert len(fin_now) == len(rec["jerks"])
        self._finished.update(i for _, i in fin_now)
        waves = {s // 64 for s, _ in fin_now}
        self.two_fin_waves += int(len(waves) >= 2)
        self.skip_and_tree += int(len(waves) >= 1 and len(waves) < self.nw)

    def summary(self):
        p = np.asarray(self.pops)
        k = int(p.argmax()) if len(p) else 0
        crossed = [x for x in (64, 128, 192) if len(p) and p.max() > x and p[k:].min() < x]
        return dict(collided=self.collided, locks=self.locks, rew_ovr=self.rew_ovr, two_fin_waves=self.two_fin_waves,
                    skip_and_tree=self.skip_and_tree, no_ctl=self.no_ctl, max_ctl=self.max_ctl, peak=int(p.max()) if len(p) else 0,
                    crossed=crossed, emptied=bool(len(p) and p.max() > 0 and p[k:].min() == 0))


Reference = collections.namedtuple("Reference", "spec arr choice actions table snaps env_snaps stats cfg spawned0")
_refs = {}


def reference(name):
    """The oracle's run of an open-loop scenario, once: arrival (and intention) streams, the slot-indexed actions of every tick
    [T, E, capacity], the tape as a (tick, id) table, the accumulators' snapshots at the end of every segment
    (snaps[t] = the batch's vector after t ticks, env_snaps[t] = one per intersection) and the reach statistics."""
    if name in _refs:
        return _refs[name]
    bounded = name in FULL_SPECS
    spec = FULL_SPECS[name] if bounded else SPECS[name]
    cfg = spec_cfg(spec)
    E, K, L, T = len(spec.envs), spec.capacity, spec.lane_num, sum(spec.calls)
    streams = [burst_arrivals(L, g, d, s) for g, d, s in spec.envs]
    rows = max(len(a) for a in streams)
    arr = np.full((E, rows, L), np.inf)
    for e, a in enumerate(streams):
        arr[e, :len(a)] = a
    choice = synthetic_intentions(E, rows, seed=spec.envs[0][2], lane_num=8) if L == 8 else None
    pol = get_policy(spec.tape)
    oracles = [make_oracle(arr[e], L, choice=None if choice is None else choice[e], **(dict(cfg, capacity=K) if bounded else cfg))
               for e in range(E)]
    accs = [metrics_ref.MetricsRef(K) for _ in range(E)]
    stats = [TickStats(K) for _ in range(E)]
    actions = np.zeros((T, E, K))
    cuts = set(np.cumsum(spec.calls).tolist())
    snaps, env_snaps = {}, {}
    for t in range(T):
        for e, o in enumerate(oracles):
            vid, ctl, _ = o.alive_view()
            n = len(vid)
            assert n <= K, "%s: %d vehicles alive in env %d at tick %d: the scenario does not fit %d slots" % (name, n, e, t, K)
            a = pol(t, vid, ctl)
            actions[t, e, :n] = a
            rec = o.tick(a)
            assert len(rec["veh_i"]) <= K, "%s: the spawns of tick %d would be deferred (overflow)" % (name, t)
            accs[e].add(rec, n)
            stats[e].add(rec, vid)
        if t + 1 in cuts:
            env_snaps[t + 1] = [a.snapshot() for a in accs]
            snaps[t + 1] = metrics_ref.total(env_snaps[t + 1])
    if bounded:             # every intersection defers spawns, and still does in the last segment (every snapshot moves)
        cut = sorted(cuts)
        assert all(s[0]["overflow"] > 0 for s in env_snaps[cut[0]]), "%s: an intersection never defers a spawn" % name
        assert snaps[T][0]["overflow"] > snaps[cut[1]][0]["overflow"] > snaps[cut[0]][0]["overflow"], name
    n_ids = max(int(s[0]["spawned"]) for s in env_snaps[T]) + 1
    table = np.stack([pol(t, np.arange(n_ids), np.ones(n_ids, np.int32)) for t in range(T)])
    ref = Reference(spec, arr, choice, actions, table, snaps, env_snaps, [s.summary() for s in stats], cfg,
                    sum(s.pops[0] for s in stats))
    _refs[name] = ref
    return ref


def new_batch(ref, backend, outputs=OUTS, obs_dtype=torch.float64, pipelined=0):
    spec = ref.spec
    kw = dict(ref.cfg)
    if spec.lane_num != 12:
        kw.update(lane_num=spec.lane_num, intentions=ref.choice)
    E = len(spec.envs)
    if pipelined:
        from pve_mcc_amd.batched import PipelinedIntersections
        from tests.hip_adapter import emulator_lib
        dev = dict(device="cpu", _lib=emulator_lib()) if backend == "emu" else dict(device="cuda")
        b = PipelinedIntersections(E, spec.capacity, ref.arr, n_sub=pipelined, outputs=outputs, **dev, **kw)
    else:
        b = make_batch(ref.arr, E, spec.capacity, backend, outputs=outputs, obs_dtype=obs_dtype, **kw)
    b.reset()
    return b


def check_zero(b, what, spawned0):
    """after reset(): every sum is zero; `spawned` is the id counter, which the constructor's warm-up leaves at the vehicles it
    put on the road (ref :214-220; the oracle's count)"""
    m = b.metrics()
    print("metrics after reset() [%s]: spawned %d (the oracle's warm-up: %d)" % (what, m["spawned"], spawned0))
    assert set(m) == set(metrics_ref.NAMES) and m.pop("spawned") == spawned0, "%s: metrics after reset(): %r" % (what, m)
    assert all(v == 0 for v in m.values()), "%s: metrics after reset(): %r" % (what, m)


def drive(b, ref, form, chunk=0, persistent=False, what="", launch=None, waves=None):
    """Runs the scenario's segments on batch `b` in launch form `form` and compares metrics() with the accumulators at the end of
    every segment.  Returns ({entry: worst deviation / bar}, the final metrics() dict)."""
    spec = ref.spec
    dev = b.device
    worst = {}
    if form == "pool":
        b.set_action_pool(torch.as_tensor(ref.actions))
    if form == "table":
        b.set_action_table(torch.as_tensor(ref.table))
    train = "state_pre" in getattr(b, "out", {})
    traj = b.alloc_trajectory(max(spec.calls)) if train else False
    t = 0
    for n in spec.calls:
        if form in ("step", "split"):
            for k in range(t, t + n):
                a = torch.as_tensor(ref.actions[k]).to(dev)
                if form == "step":
                    b.step(a)
                else:
                    b.scene_update(a)
                    b.compact()
        else:
            b.step_many(n, source=form, chunk=chunk, persistent=persistent, trajectory=traj)
            if launch is not None and not hasattr(b, "subs"):
                want = launch if (0 < chunk < n or launch == "resident") else "resident"
                assert b.last_launch() == want, (what, n, b.last_launch(), want)
                if waves is not None:         # (the build a queue launch must be: 5 = HOME, 4 = the register build, as every other launch)
                    v = b.last_variant()
                    assert v["waves_per_simd"] == (waves if want == "persistent" else 4) and v["prof"] == 0, (what, n, v, waves)
        b.synchronize()
        t += n
        m = b.metrics()
        frac = metrics_ref.compare(m, ref.snaps[t], "%s %s [%s] after %d ticks" % (spec.name, form, what, t))
        for k, v in frac.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst, m


def check_open_loop(backend, name, form, outputs=OUTS, obs_dtype=torch.float64, chunk=0, persistent=False, launch=None,
                    pipelined=0, replay=False, waves=None):
    """One scenario in one launch form against the accumulators.  replay=True: reset() then returns every entry to zero and the
    same run gives the same vector again, bit for bit in the float sums."""
    ref = reference(name)
    b = new_batch(ref, backend, outputs=outputs, obs_dtype=obs_dtype, pipelined=pipelined)
    what = "chunk %d%s" % (chunk, ", queue" if persistent else "")
    check_zero(b, what, ref.spawned0)
    worst, m = drive(b, ref, form, chunk, persistent, what, launch, waves)
    if replay:
        b.reset()
        check_zero(b, what + ", second reset", ref.spawned0)
        _, m2 = drive(b, ref, form, chunk, persistent, what + ", replay", launch)
        assert m == m2, "the replay after reset() gave another vector: %r vs %r" % (m, m2)
    return worst


# ---------------------------------------------------------------------------------------------- closed loop
ClosedLoop = collections.namedtuple("ClosedLoop", "arr choice calls snaps cfg lane_num capacity sigma reach")
_loops = {}
NOISE = (0.4, 4242, 7)        # (sigma, seed, env_offset) of the noisy closed loop


def closed_loop_reference(backend, lane_num, capacity, noisy=False, cfg=None, n_envs=2, calls=None, rate=None, seed=91):
    """The closed loop in its two-launch form (act() + fused tick): the device's own actions are read back every tick and drive
    the oracle (the tape discipline of test_gpu_noisy_actions_drive_the_oracle), so the accumulators see exactly the trajectory
    the device ran; the form's own metrics() is compared here, the snapshots serve the resident / queue forms (which existing
    tests hold to this form bit for bit)."""
    key = (backend, lane_num, capacity, noisy, tuple(sorted((cfg or {}).items())))
    if key in _loops:
        return _loops[key]
    cfg = dict(cfg or {})
    rate = rate or {12: {128: 1400.0, 256: 2600.0}, 4: {128: 1500.0}}[lane_num][capacity]
    calls = calls or ((150, 7, 143) if capacity == 256 else (90, 7, 103))   # (256 slots: long enough to hold more than 128 vehicles)
    T = sum(calls)
    arr = synthetic_arrivals(n_envs, rate=rate, horizon_s=T * 0.1 + 30, seed=seed, lane_num=lane_num)
    lp = ClosedLoop(arr, None, calls, {}, cfg, lane_num, capacity, NOISE if noisy else None, dict(peak=0, max_ctl=0))
    b = closed_loop_batch(lp, backend)
    oracles = [make_oracle(arr[e], lane_num, **cfg) for e in range(n_envs)]
    accs = [metrics_ref.MetricsRef(capacity) for _ in range(n_envs)]
    cuts = set(np.cumsum(calls).tolist())
    for t in range(T):
        acts = _np(b.act()).copy()
        b.step_with_actor()
        for e, o in enumerate(oracles):
            n = o.n_alive
            _vid, ctlm, _ = o.alive_view()
            assert np.all(acts[e, :n][ctlm == 0] == 0) and np.all(acts[e, n:] == 0), "uncontrolled slots get 0 (main.py:401)"
            rec = o.tick(acts[e, :n])
            accs[e].add(rec, n)
            lp.reach.update(peak=max(lp.reach["peak"], n), max_ctl=max(lp.reach["max_ctl"], len(rec["ids"])))
        if t + 1 in cuts:
            lp.snaps[t + 1] = metrics_ref.total([a.snapshot() for a in accs])
            b.synchronize()
            metrics_ref.compare(b.metrics(), lp.snaps[t + 1], "closed loop lane_num %d x %d%s, two-launch form, after %d ticks"
                                % (lane_num, capacity, ", noise" if noisy else "", t + 1))
    want, _ = lp.snaps[T]
    print("closed loop lane_num %d x %d: peak population %d, most controlled vehicles in a tick %d, %s"
          % (lane_num, capacity, lp.reach["peak"], lp.reach["max_ctl"], {k: want[k] for k in ("ctl_steps", "passed", "collided", "locks")}))
    assert want["ctl_steps"] > 20 * T and want["passed"] > 0, want
    # the loop uses what its capacity adds: more vehicles than the next smaller capacity holds, and a second wave of controlled ones
    if capacity == 256:
        assert lp.reach["peak"] > 128 and lp.reach["max_ctl"] > 64, lp.reach
    _loops[key] = lp
    return lp


def closed_loop_batch(lp, backend):
    from oracle.actor_np import flat_weights, load_weights
    kw = dict(lp.cfg)
    if lp.lane_num != 12:
        kw.update(lane_num=lp.lane_num)
    b = make_batch(lp.arr, lp.arr.shape[0], lp.capacity, backend, outputs=OUTS, **kw)
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    if lp.sigma:
        b.set_exploration(lp.sigma[0], seed=lp.sigma[1], env_offset=lp.sigma[2])
    return b


def check_closed_loop(backend, lane_num, capacity, chunk=0, persistent=False, noisy=False, cfg=None):
    """step_many(source="actor") -- resident, chunked or through the work queue -- against the accumulators that the two-launch
    form's actions fed."""
    lp = closed_loop_reference(backend, lane_num, capacity, noisy=noisy, cfg=cfg)
    b = closed_loop_batch(lp, backend)
    t, worst = 0, {}
    for n in lp.calls:
        b.step_many(n, source="actor", chunk=chunk, persistent=persistent)
        b.synchronize()
        if backend != "emu":
            want = "persistent" if (persistent and 0 < chunk < n) else "resident"
            assert b.last_launch() == want, (b.last_launch(), want, n)
        t += n
        frac = metrics_ref.compare(b.metrics(), lp.snaps[t], "closed loop lane_num %d x %d%s, step_many chunk %d%s, after %d ticks"
                                   % (lane_num, capacity, ", noise" if noisy else "", chunk, ", queue" if persistent else "", t))
        for k, v in frac.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ---------------------------------------------------------------------------------------------- golden digests
def digest_accumulator(case, capacity, ticks=None):
    """The golden fixture's per-tick digests (written by the unmodified reference) summed.  The population at the start of a
    tick is the previous row's n_alive (taken before delete_vehicle(): the deleted vehicles are still in it) minus its
    n_deleted; in front of the first tick it is what the constructor's warm-up left (the oracle's, pinned by
    test_oracle_constructor_warmup_pins)."""
    from oracle.record import DIGEST_F_COLS, DIGEST_I_COLS
    choice = case.choice if case.lane_num == 8 else None
    n_pre = make_oracle(case.arrive, case.lane_num, choice=choice, **case.ctor).n_alive
    acc = metrics_ref.MetricsRef(capacity)
    ia, idl = DIGEST_I_COLS.index("n_alive"), DIGEST_I_COLS.index("n_deleted")
    for t in range(case.ticks if ticks is None else ticks):
        acc.add_digest(case.dig_i[t], case.dig_f[t], n_pre, DIGEST_I_COLS, DIGEST_F_COLS)
        n_pre = int(case.dig_i[t][ia]) - int(case.dig_i[t][idl])
    return acc


def check_golden_anchor(backend, case_name, capacity=128, ticks=None):
    """A golden case replayed with fused ticks: metrics() equals the fixture's digests summed.  sum_reward, sum_jerk, locks,
    ctl_steps, spawned, passed and passed_steps are the reference's own numbers; alive_steps is derived from the digests'
    n_alive - n_deleted, its first term from the oracle's constructor (digest_accumulator).  The tape is a function of the
    vehicle ids the batch itself holds."""
    from tests.parity_util import GoldenCase
    case = GoldenCase(case_name)
    T = case.ticks if ticks is None else min(ticks, case.ticks)
    kw = dict(case.ctor)
    if case.lane_num != 12:
        kw.update(lane_num=case.lane_num, intentions=case.choice if case.lane_num == 8 else None)
    b = make_batch(case.arrive, 1, capacity, backend, outputs=("obs_post", "reward", "flags", "env_out"), **kw)
    b.reset()
    for t in range(T):
        n = b.read_env(0).n_alive
        ids = _np(b.state_field("id")[0, :n]).astype(np.int64)
        ctl = _np(b.state_field("meta")[0, :n]) & 1
        acts = torch.zeros(1, capacity, dtype=torch.float64)
        acts[0, :n] = torch.as_tensor(case.policy(t, ids, ctl))
        b.step(acts.to(b.device))
    b.synchronize()
    return metrics_ref.compare(b.metrics(), digest_accumulator(case, capacity, T).snapshot(), "golden %s, fused ticks" % case_name)

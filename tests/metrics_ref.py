"""Reference accumulator of the twelve metric sums (pve_get_metrics / BatchedIntersections.metrics()).

Plain Python.  A MetricsRef is fed one tick at a time -- an oracle tick record (oracle/record.py), or a row of a golden
fixture's per-tick digests where only those exist -- together with the population at the START of the tick, and yields the
entries under the names metrics() uses:

  ticks          ticks fed
  slot_steps     ticks x capacity
  alive_steps    sum of the population at the start of the tick (PVE_EO_N_PRE; not the digest's post-tick n_alive)
  ctl_steps      sum of len(ids)
  spawned        the last id_seq
  passed, passed_steps   the last passed / passed_step_total
  collided       sum of count(coll_pv > 0): main.py:410-412 (tests/golden/gen_golden.py), not the 9-tuple's `collisions`
  locks          sum of lock
  overflow       sum of the tick's deferral count (`deferred`) of a capacity-bound oracle's records; 0 for unbounded records and
                 for digest rows (the reference never defers a spawn)
  sum_reward     math.fsum of every reward of every tick
  sum_jerk       math.fsum of every `jerks` entry

Bars (compare()): the ten counters are exact.  The two float sums get 1e-9 x sum(max(1, |term|)) over the reference's own
terms: the project's per-value bar (oracle.record.close at 1e-9, asserted for every reward and every jerk_sum) summed over
the terms.  The rounding of the reduction itself, n x 2^-53 x sum|term|, is orders of magnitude below it; one dropped,
doubled or stale term of ordinary size (rewards O(1), -10 / +5 on events; jerk sums O(100)) is far above it.

Largest deviation seen per kernel family, as a fraction of that bar (sum_reward / sum_jerk; tests/test_gpu_metrics.py
prints every comparison):
  CPU emulator (serial sums), every scenario of tests/metrics_scenarios.py     7.5e-7 / 0
  MI355X: k_tick / k_rollout, 12 lanes (register and HOME builds, queue)       4.4e-7 / 0
  MI355X: k_tick_geo / k_rollout_geo, 4 and 8 lanes                            6.2e-7 / 0
  MI355X: closed loop (two-launch form, resident, queue; noise on and off)     1.1e-7 / 1.7e-7
"""
import math

COUNTERS = ("slot_steps", "alive_steps", "ctl_steps", "spawned", "passed", "collided", "locks", "passed_steps", "overflow",
            "ticks")
FLOAT_SUMS = ("sum_reward", "sum_jerk")
NAMES = ("slot_steps", "alive_steps", "ctl_steps", "spawned", "passed", "collided", "locks", "sum_reward", "sum_jerk",
         "passed_steps", "overflow", "ticks")
REL_BAR = 1e-9


class MetricsRef:
    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.ticks = self.alive_steps = self.ctl_steps = self.collided = self.locks = 0
        self.spawned = self.passed = self.passed_steps = self.overflow = 0
        self.collided_known = True                # (a digest row carries no coll_pv)
        self._rewards, self._jerks = [], []       # every term (records), or one partial sum per tick (digest rows)
        self.reward_scale = self.jerk_scale = 0.0  # sum of max(1, |term|)

    # ---- feeding
    def add(self, rec, n_pre):
        """One oracle tick record; n_pre: vehicles alive when the tick began."""
        self.ticks += 1
        self.alive_steps += int(n_pre)
        self.ctl_steps += len(rec["ids"])
        self.collided += sum(1 for c in rec["coll_pv"] if c > 0)
        self.locks += int(rec["lock"])
        self.overflow += int(rec.get("deferred", 0))     # (a capacity-bound oracle: the lanes it deferred this tick)
        self.spawned, self.passed, self.passed_steps = int(rec["id_seq"]), int(rec["passed"]), int(rec["passed_step_total"])
        for x in rec["reward"]:
            self._rewards.append(float(x)); self.reward_scale += max(1.0, abs(float(x)))
        for x in rec["jerks"]:
            self._jerks.append(float(x)); self.jerk_scale += max(1.0, abs(float(x)))

    def add_digest(self, dig_i, dig_f, n_pre, i_cols, f_cols):
        """One row of a golden fixture's digests (written by the unmodified reference).  The row holds the tick's sums, not
        its terms: the bar's scale takes max(n, |sum|) for n terms, a lower bound of sum(max(1, |term|)).  No coll_pv in a
        digest: `collided` is then unknown (left out of as_dict())."""
        gi = dict(zip(i_cols, (int(x) for x in dig_i)))
        gf = dict(zip(f_cols, (float(x) for x in dig_f)))
        self.ticks += 1
        self.alive_steps += int(n_pre)
        self.ctl_steps += gi["n_ctl"]
        self.collided_known = False
        self.locks += gi["lock"]
        self.spawned, self.passed, self.passed_steps = gi["id_seq"], gi["passed"], gi["passed_step_total"]
        self._rewards.append(gf["sum_reward"]); self.reward_scale += max(float(gi["n_ctl"]), abs(gf["sum_reward"]))
        self._jerks.append(gf["sum_jerks"]); self.jerk_scale += max(float(gi["n_jerks"]), abs(gf["sum_jerks"]))

    # ---- reading
    def as_dict(self):
        d = dict(ticks=self.ticks, slot_steps=self.ticks * self.capacity, alive_steps=self.alive_steps,
                 ctl_steps=self.ctl_steps, spawned=self.spawned, passed=self.passed, passed_steps=self.passed_steps,
                 collided=self.collided, locks=self.locks, overflow=self.overflow,
                 sum_reward=math.fsum(self._rewards), sum_jerk=math.fsum(self._jerks))
        if not self.collided_known:
            del d["collided"]
        return d

    def bars(self):
        return dict(sum_reward=REL_BAR * self.reward_scale, sum_jerk=REL_BAR * self.jerk_scale)

    def snapshot(self):
        """(entries, bars) now: what a mid-run read of metrics() is compared with."""
        return self.as_dict(), self.bars()


def total(snapshots):
    """The vector of a batch: entry-wise sum of several accumulators' snapshots (spawned / passed / passed_steps add up like
    the rest: the handle sums its intersections' headers)."""
    ents, bars = {}, {}
    for d, b in snapshots:
        for k, v in d.items():
            ents.setdefault(k, []).append(v)
        for k, v in b.items():
            bars[k] = bars.get(k, 0.0) + v
    n = len(snapshots)
    out = {}
    for k, vs in ents.items():
        if len(vs) == n:                          # (an entry one of the parts does not know is unknown for the batch)
            out[k] = math.fsum(vs) if k in FLOAT_SUMS else sum(vs)
    return out, bars


def compare(got, ref, what="", names=None, quiet=False):
    """metrics() dict `got` against a snapshot `ref` = (entries, bars): counters exact, float sums at their bars.  Prints
    the measured deviation of each float sum; returns {name: deviation / bar}."""
    want, bars = ref
    names = NAMES if names is None else names
    frac = {}
    for k in names:
        if k not in want:
            continue
        if k in FLOAT_SUMS:
            dev = abs(float(got[k]) - want[k])
            frac[k] = dev / bars[k] if bars[k] > 0 else (0.0 if dev == 0 else math.inf)
            if not quiet:
                print("metrics %s: %s %.17g vs reference %.17g: deviation %.3e, bar %.3e (%.2e of it)"
                      % (what, k, got[k], want[k], dev, bars[k], frac[k]))
            assert dev <= bars[k], "%s: %s = %.17g, reference %.17g: off by %.3e, bar %.3e" % (what, k, got[k], want[k], dev, bars[k])
        else:
            assert float(got[k]) == float(want[k]), "%s: %s = %r, reference %r" % (what, k, got[k], want[k])
    return frac

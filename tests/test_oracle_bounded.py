"""The capacity bound of the oracles (OracleEnv / OracleGeoEnv `capacity=`) pinned to the unbounded oracle and to the reference.

The reference reads an arrival time only in `current_time >= arrive[veh_rec][lane]` (ref :379).  So a run that defers spawns
must equal an UNBOUNDED run on the arrival stream it effectively served: every entry that was granted late rewritten to the
`current_time` of its grant tick, every entry still waiting at the end to +inf (tests/bounded_scenarios.rewritten_arrivals).
Every record field of every tick and the vehicles at the end are compared bit for bit with the unbounded oracle, and -- where
the unmodified reference is present -- at the 1e-12 of test_oracle_vs_reference.py with the reference itself on the rewritten
stream: the deferral semantics are tied to reference behaviour, not to a reading of the kernel.

Oracle-side counts of the scenarios (all envs; deferring ticks / partial grants / deferring ticks that also delete / longest
run of ticks one lane stayed deferred / collisions / dead-locks / deferred spawns):
  S12_64        511 /  73 /  75 / 182 /  72 /  323 / 4565      S4_64    431 /  93 / 105 /  84 / 345 /  991 / 1316
  S12_64_Q      511 /  87 /  88 / 182 /  97 /  333 / 4452      S4_128   433 / 193 / 207 /  64 / 762 / 1947 / 1319
  S12_64_TABLE  491 /  94 /  94 / 172 / 151 /  315 / 3949      S8_64    501 /  97 /  99 / 162 / 216 /  681 / 3043
  S12_128       849 / 313 / 313 / 278 / 531 / 1558 / 6859      S8_128    91 /  36 /  43 /  47 / 381 / 1843 /  251
  S12_128_TABLE 847 / 290 / 291 / 281 / 413 / 1135 / 7156      S12_256  217 /  92 / 101 /  85 / 245 /  899 / 1339
"""
import numpy as np
import pytest

from oracle.oracle import OracleEnv
from oracle.oracle_geo import OracleGeoEnv
from oracle.record import compare_records, get_policy
from tests import bounded_scenarios as bs

SCENARIOS = {"lanes12": bs.S12_64, "lanes4": bs.S4_64, "lanes8": bs.S8_64, "lanes12_256": bs.S12_256}


def _unbounded(run, e, arr):
    scn = run.scn
    if scn.lane_num == 12:
        return OracleEnv(arr, **dict(scn.cfg))
    return OracleGeoEnv(arr, scn.lane_num, choice=None if run.ch is None else run.ch[e], **dict(scn.cfg))


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_bounded_run_equals_unbounded_run_on_the_rewritten_stream(name):
    run = bs.oracle_run(SCENARIOS[name])
    scn = run.scn
    if scn.lane_num == 8:
        assert 0.3 < run.ch.mean() < 0.7 and all(len(np.unique(run.ch[:, :40, l])) == 2 for l in range(8))      # a non-trivial intention stream
    n_rewritten = n_waiting = 0
    for e in range(scn.n_envs):
        arr, waiting = bs.rewritten_arrivals(run, e)
        n_rewritten += int((arr != run.arr[e]).sum()) - waiting
        n_waiting += waiting
        o = _unbounded(run, e, arr)
        for t in range(scn.ticks):
            vid, ctl, _ = o.alive_view()
            rec = o.tick(bs._actions(run, t, e, vid, ctl))
            want = run.recs[t][e]
            compare_records(want, rec, tol=0.0, label="%s env %d" % (name, e))
            assert np.array_equal(want["veh_f"], rec["veh_f"]) and np.array_equal(want["obs0"], rec["obs0"])
            if scn.lane_num != 12:
                assert np.array_equal(want["intent"], rec["intent"]) and want["intention_re"] == rec["intention_re"]
            assert rec["deferred"] == 0
        assert o.overflow == 0 and o.ref_would_raise == 0
        for a, b in zip(run.final[e], o.vehicles()):
            assert np.array_equal(a, b)
    assert n_rewritten > 0, "no late grant"
    if name == "lanes12":                       # (64 slots: the high lanes are still starved when the run ends -> +inf entries)
        assert n_waiting > 0


def test_unbounded_is_the_default_and_reports_no_deferral():
    run = bs.scenario_inputs(bs.S12_64)
    a, b, c = OracleEnv(run.arr[0]), OracleEnv(run.arr[0], capacity=None), OracleEnv(run.arr[0], capacity=64)
    assert a.capacity is None and c.capacity == 64
    pol = get_policy("rand3")
    differs = False
    for t in range(200):
        vid, ctl, _ = a.alive_view()
        ra, rb = a.tick(pol(t, vid, ctl)), b.tick(pol(t, vid, ctl))
        compare_records(ra, rb, tol=0.0)
        assert ra["overflow"] == ra["deferred"] == ra["deferred_lanes"] == 0
        vc, cc, _ = c.alive_view()
        rc = c.tick(pol(t, vc, cc))
        assert len(vc) <= 64 and rc["deferred"] == bin(rc["deferred_lanes"]).count("1")
        differs = differs or rc["id_seq"] != ra["id_seq"]
    assert a.overflow == b.overflow == 0 and c.overflow > 0 and differs and a.n_alive > 64


def test_a_deferred_spawn_touches_nothing():
    """veh_rec, veh_num, id_seq, intention_re and the 8-lane choice cursor of a deferred lane stay where they are; the lowest due
    lanes are granted; room is what was free at tick start."""
    for scn in (bs.S12_64, bs.S4_64, bs.S8_64):
        run = bs.oracle_run(scn)
        for e in range(scn.n_envs):
            for t in range(scn.ticks):
                r = run.recs[t][e]
                granted = (r["veh_rec"] - r["veh_rec_pre"]).astype(int)
                assert set(granted.tolist()) <= {0, 1}
                deferred = np.array([(r["deferred_lanes"] >> l) & 1 for l in range(scn.lane_num)])
                assert not np.any(granted & deferred)
                assert r["id_seq"] - r["id_seq_pre"] == granted.sum()
                if scn.lane_num != 12 and t > 0:
                    assert r["intention_re"] - run.recs[t - 1][e]["intention_re"] == granted.sum()
                if deferred.any():
                    assert granted.sum() == scn.capacity - r["n_pre"], "room is capacity - (alive at tick start)"
                    due = np.flatnonzero(granted | deferred)
                    assert np.array_equal(due[:granted.sum()], np.flatnonzero(granted)), "the lowest due lanes are granted"
                assert len(r["veh_i"]) <= scn.capacity


def test_capacity_below_one_slot_per_lane_is_refused():
    run = bs.scenario_inputs(bs.S12_64)
    with pytest.raises(ValueError):
        OracleEnv(run.arr[0], capacity=8)
    run4 = bs.scenario_inputs(bs.S4_64)
    with pytest.raises(ValueError):
        OracleGeoEnv(run4.arr[0], 4, capacity=3)


# ---------------------------------------------------------------- the live reference on the rewritten stream
@pytest.mark.reference
@pytest.mark.parametrize("name", ["lanes12", "lanes4", "lanes8"])
def test_bounded_oracle_vs_live_reference_on_the_rewritten_stream(name):
    from tests.golden import ref_harness as rh
    run = bs.oracle_run(SCENARIOS[name])
    scn = run.scn
    e = 1
    arr, _ = bs.rewritten_arrivals(run, e)
    if scn.lane_num == 12:
        ref = rh.RefRunner(arr, None, want_state=False, **dict(scn.cfg))
    else:
        ref = rh.GeoRefRunner(arr, scn.lane_num, None, choice=None if run.ch is None else run.ch[e], want_state=False, **dict(scn.cfg))
    try:
        for t in range(scn.ticks):
            vid, ctl, _ = ref.alive_view()
            ra = ref.tick(bs._actions(run, t, e, vid, ctl))
            rb = run.recs[t][e]
            compare_records(ra, rb, tol=1e-12, label="%s vs reference" % name)
            if scn.lane_num != 12:
                assert np.array_equal(ra["intent"], rb["intent"]) and ra["intention_re"] == rb["intention_re"]
        assert run.overflow[e] > 0
    finally:
        if hasattr(ref, "close"):
            ref.close()

"""CPU tests of the metrics vector (pve_get_metrics): the reference accumulator (tests/metrics_ref.py) against the golden
fixtures' own numbers, the reach conditions of the scenarios (tests/metrics_scenarios.py) on the oracle side alone, and the
emulator's metrics() against the accumulator in every launch form.  The emulator adds the float sums serially; the block
reductions of the kernels exist on the device only: the `-m gpu` twin, tests/test_gpu_metrics.py, runs the same scenarios."""
import pytest
import torch

from tests import hip_adapter, metrics_ref
from tests import metrics_scenarios as S
from tests.parity_util import CASE_NAMES, GEO_CASE_NAMES, GoldenCase, replay_case

BACKEND = "emu"


@pytest.fixture
def wide(monkeypatch):
    """the 256-slot scenarios run on the wide emulator (tests/emu_wide)"""
    from tests.test_capacity256 import wide_lib
    lib = wide_lib()
    monkeypatch.setattr(hip_adapter, "emulator_lib", lambda: lib)
    return lib


# ------------------------------------------------------------------ 1. the accumulator against the reference's numbers
class Feeding:
    """An oracle env whose ticks also feed an accumulator (the shape parity_util.replay_case drives)."""

    def __init__(self, env, acc):
        self.env, self.acc, self.n_pre = env, acc, 0

    def alive_view(self):
        v = self.env.alive_view()
        self.n_pre = len(v[0])
        return v

    def tick(self, actions, want_state=False):
        rec = self.env.tick(actions, want_state=want_state)
        self.acc.add(rec, self.n_pre)
        return rec


@pytest.mark.parametrize("name", CASE_NAMES + GEO_CASE_NAMES)
def test_accumulator_matches_golden_digests(name):
    case = GoldenCase(name)
    choice = case.choice if case.lane_num == 8 else None
    acc = metrics_ref.MetricsRef(128)
    replay_case(case, Feeding(S.make_oracle(case.arrive, case.lane_num, choice=choice, **case.ctor), acc))
    got = acc.as_dict()
    dig = S.digest_accumulator(case, 128)
    frac = metrics_ref.compare(got, dig.snapshot(), "accumulator on %s vs its digests summed" % name)
    assert set(frac) == {"sum_reward", "sum_jerk"} and got["ticks"] == case.ticks
    if name == "s1000_actor":
        agg = case.aggregates
        assert (got["spawned"], got["passed"], got["collided"], got["locks"], got["ctl_steps"]) == (323, 281, 0, 548, 37295)
        assert (agg["id_seq"], agg["passed"], agg["collided"], agg["locks"], agg["ctl_steps"]) == (323, 281, 0, 548, 37295)
        assert abs(got["sum_reward"] / got["ctl_steps"] - agg["reward_mean"]) < 1e-9
        assert abs(got["sum_jerk"] / got["passed"] - agg["jerk_per_veh"]) < 1e-9 * 208.799
        assert abs(got["passed_steps"] / (got["passed"] + 1e-4) * 0.1 - agg["pT_m"]) < 1e-12


def test_accumulators_add_up_and_bars():
    a, b = metrics_ref.MetricsRef(64), metrics_ref.MetricsRef(64)
    rec = dict(ids=[(0, 0), (1, 0)], coll_pv=[0, 2], lock=1, id_seq=5, passed=2, passed_step_total=300, reward=[-10.0, 0.25],
               jerks=[150.0])
    a.add(rec, 3)
    b.add(dict(rec, reward=[0.5, 0.5], jerks=[], lock=0, coll_pv=[0, 0]), 4)
    b.add(dict(rec, ids=[], reward=[], jerks=[], lock=0, coll_pv=[], id_seq=6), 2)
    d, bars = metrics_ref.total([a.snapshot(), b.snapshot()])
    assert d == dict(ticks=3, slot_steps=192, alive_steps=9, ctl_steps=4, spawned=11, passed=4, passed_steps=600, collided=1,
                     locks=1, overflow=0, sum_reward=-8.75, sum_jerk=150.0)
    assert bars == dict(sum_reward=1e-9 * 13.0, sum_jerk=1e-9 * 150.0)
    with pytest.raises(AssertionError):
        metrics_ref.compare(dict(d, sum_reward=-8.75 + 1e-7), (d, bars), quiet=True)
    with pytest.raises(AssertionError):
        metrics_ref.compare(dict(d, locks=2), (d, bars), quiet=True)
    metrics_ref.compare(dict(d, sum_reward=-8.75 + 1e-9), (d, bars), quiet=True)


# ------------------------------------------------------------------ 2. what the scenarios contain (oracle side alone)
def test_scenarios_reach_the_paths_they_are_meant_for():
    """Every scenario fits its capacity (reference() asserts it: overflow == 0) and the set covers the conditions under which
    the device's sums can go wrong.  The count of -10s that land on ANOTHER vehicle's reward (rew_ovr, ref :346) is printed, not
    asserted: the reference's own rules leave no stream that produces one.  The override needs an UNCONTROLLED vehicle A with
    collision > 0.  Only controlled vehicles are listed (step() pushes them, ref :1539), so A can only have been hit in the tick
    T in which it finished, by a vehicle B processed after it whose nearest listed vehicle (ref :293, nearest in |vd - vd_B|)
    was A at less than collision_thr.  A vehicle of another lane is listed in B's frame only in front of its conflict point
    (get_virtual_distance: delta > 0), never at p < 0, so B follows A in A's own lane and vd_A = p_A < 0 is the smallest key of
    the list (vehicles further ahead finished earlier and are not listed; other lanes have vd > 0).  At T, A itself is still
    controlled and checks ITS nearest listed vehicle first: unless that is someone other than B, A counts the same hit
    (ref :332-334), is deleted as a controlled vehicle and takes its own -10.  Someone nearer to A than B in |vd| has its key
    between vd_A and vd_B -- and is then nearer to B than A is, so B's nearest is not A.  The one way out is a vehicle that
    finishes in the same tick right in front of A with the chord / arc slack of the left-turn curve (centimetres) between the
    three distances; no arrival stream steers that.  The device path itself (rew_ovr through LDS) stays covered by the per-tick
    reward comparisons of the parity suite wherever the oracle produces it."""
    tot = {}
    for name in S.SPECS:
        ref = S.reference(name)
        want, _ = ref.snaps[sum(ref.spec.calls)]
        print("reach %-14s %s" % (name, "; ".join("env %d: %s" % (e, st) for e, st in enumerate(ref.stats))))
        print("      %-14s totals: %s" % (name, {k: want[k] for k in ("ctl_steps", "alive_steps", "spawned", "passed", "collided", "locks")}))
        assert want["overflow"] == 0
        tot[name] = ref.stats
    st = tot
    every = [s for ss in st.values() for s in ss]
    print("reach totals: collided %d, locks %d, rew_ovr %d" % (sum(s["collided"] for s in every), sum(s["locks"] for s in every),
                                                              sum(s["rew_ovr"] for s in every)))
    for name in ("l12_c64", "l12_c128", "l12_c256", "l4_c64", "l4_c128", "l8_c64", "l8_c128", "l4_c128_kw", "l8_c64_kw"):
        s = st[name]
        assert sum(x["collided"] for x in s) > 0 and sum(x["locks"] for x in s) > 0, name
        assert S.reference(name).snaps[sum(S.SPECS[name].calls)][0]["passed"] > 0, name
        assert sum(x["no_ctl"] for x in s) > 0, name                       # a tick with no controlled vehicle at all
    for name in ("l12_c128", "l12_c256", "l12_c128_five"):                 # 12 lanes, two and four waves
        s = st[name]
        assert sum(x["two_fin_waves"] for x in s) > 0, name                # vehicles of two waves finish in one tick
        assert sum(x["skip_and_tree"] for x in s) > 0, name                # the ballot skip and the tree in one tick
        assert max(x["max_ctl"] for x in s) > 64, name                     # more than 64 controlled vehicles in one tick
    for name in ("l4_c128", "l8_c128", "l4_c128_kw"):                      # 4 / 8 lanes, two waves (few finish per tick)
        s = st[name]
        assert sum(x["skip_and_tree"] for x in s) > 0 and any(64 in x["crossed"] for x in s), name
    assert max(x["max_ctl"] for x in st["l4_c128"]) > 64 and max(x["max_ctl"] for x in st["l8_c128"]) > 64
    # up through 64, back below it and down to an empty intersection; at 256 slots the same for 128 and 192
    assert any(64 in x["crossed"] and x["emptied"] for x in st["l12_c128"])
    assert any(64 in x["crossed"] and x["emptied"] for x in st["l4_c128_kw"])
    assert st["l12_c256"][0]["crossed"] == [64, 128, 192] and st["l12_c256"][0]["emptied"]
    # reset() leaves `spawned` at the warm-up's id counter: the scenarios do have a non-empty warm-up (one vehicle per stream)
    assert S.reference("l12_c128").spawned0 == 2 and S.reference("l12_c128_five").spawned0 == 7
    five = st["l12_c128_five"]
    assert five[0]["peak"] == 0 and five[1]["emptied"] and 0 < five[1]["peak"] < 40 and five[3]["peak"] > 100


# ------------------------------------------------------------------ 3. the emulator's metrics() against the accumulator
FORMS = [("step", {}), ("split", {}), ("pool", dict(launch="resident")), ("pool", dict(chunk=7, persistent=True, launch="persistent")),
         ("table", dict(chunk=1, persistent=True, launch="persistent"))]


@pytest.mark.parametrize("form,kw", FORMS)
@pytest.mark.parametrize("name", ["l12_c64", "l12_c128", "l4_c64", "l4_c128", "l8_c64", "l8_c128"])
def test_emulated_metrics_match_the_accumulator(name, form, kw):
    S.check_open_loop(BACKEND, name, form, **kw)


@pytest.mark.parametrize("form,kw", FORMS)
@pytest.mark.parametrize("name", sorted(S.FULL_SPECS))
def test_emulated_metrics_full_intersections(name, form, kw):
    """overflowing bursts: `overflow` (and every other sum, through the deferred spawns) against capacity-bound oracles"""
    S.check_open_loop(BACKEND, name, form, **kw)


def test_emulated_metrics_full_intersection_home_block(monkeypatch):
    monkeypatch.setenv("PVE_EMU_HOME", "1")
    for source in ("pool", "table"):
        S.check_open_loop(BACKEND, "l12_c128_full", source, chunk=7, persistent=True, launch="persistent")


@pytest.mark.parametrize("form,kw", FORMS)
def test_emulated_metrics_match_the_accumulator_256(wide, form, kw):
    S.check_open_loop(BACKEND, "l12_c256", form, **kw)


@pytest.mark.parametrize("name", ["l4_c128_kw", "l8_c64_kw"])
def test_emulated_metrics_constructor_arguments(name):
    S.check_open_loop(BACKEND, name, "step")
    S.check_open_loop(BACKEND, name, "pool", chunk=7, persistent=True, launch="persistent")


@pytest.mark.parametrize("source", ["pool", "table"])
def test_emulated_metrics_home_block(monkeypatch, source):
    monkeypatch.setenv("PVE_EMU_HOME", "1")
    S.check_open_loop(BACKEND, "l12_c128", source, chunk=7, persistent=True, launch="persistent")


def test_emulated_metrics_home_block_zero_source(monkeypatch):
    monkeypatch.setenv("PVE_EMU_HOME", "1")
    S.check_open_loop(BACKEND, "l12_c128_zero", "zero", chunk=7, persistent=True, launch="persistent")


def test_emulated_metrics_training_outputs_and_float32_rows():
    S.check_open_loop(BACKEND, "l12_c128", "pool", outputs=S.TRAIN_OUTS, chunk=7, persistent=True, launch="persistent")
    S.check_open_loop(BACKEND, "l12_c128", "step", obs_dtype=torch.float32)


def test_emulated_metrics_batch_of_five_and_reset():
    S.check_open_loop(BACKEND, "l12_c128_five", "step", replay=True)
    S.check_open_loop(BACKEND, "l12_c128_five", "pool", chunk=7, persistent=True, launch="persistent", replay=True)
    S.check_open_loop(BACKEND, "l12_c128_five", "pool", chunk=7, pipelined=2)


@pytest.mark.parametrize("lane_num,capacity,kw", [(12, 128, {}), (4, 128, dict(cfg=dict(vm=6.0)))])     # (the emulator has no noisy actor: test_gpu_metrics.py)
def test_emulated_metrics_closed_loop(lane_num, capacity, kw):
    S.check_closed_loop(BACKEND, lane_num, capacity, **kw)
    S.check_closed_loop(BACKEND, lane_num, capacity, chunk=7, persistent=True, **kw)


def test_emulated_metrics_closed_loop_256(wide):
    S.check_closed_loop(BACKEND, 12, 256)
    S.check_closed_loop(BACKEND, 12, 256, chunk=7, persistent=True)


@pytest.mark.parametrize("name", ["s1000_rand_kw", "geo_g8_rand_kw"])
def test_emulated_metrics_equal_golden_digests(name):
    S.check_golden_anchor(BACKEND, name, ticks=300)

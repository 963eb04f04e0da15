"""-m gpu: the HIP kernels against capacity-bound oracles, through every deferred spawn of a full intersection -- k_tick,
k_tick_geo (fused and split), and the retained trajectory blocks of k_rollout / k_rollout_geo in the resident, the persistent
queue and the HOME form compared DIRECTLY with the bounded oracle's records (not with single ticks of the same library).
Scenarios, checkers and the rule: tests/bounded_scenarios.py; the rule's link to the reference: tests/test_oracle_bounded.py;
the CPU twin: tests/test_bounded_emulated.py."""
import pytest

from tests import bounded_scenarios as bs

pytestmark = pytest.mark.gpu
BACKEND = "hip"

FUSED = {"lanes12_cap64": (bs.S12_64, {}), "lanes12_cap128": (bs.S12_128, {}), "lanes12_cap256": (bs.S12_256, {}),
         "lanes12_cap64_quantised": (bs.S12_64_Q, {}), "lanes12_cap64_table": (bs.S12_64_TABLE, {}),
         "lanes12_cap64_general_path": (bs.S12_64, dict(general_path=True)),
         "lanes12_cap128_general_path": (bs.S12_128, dict(general_path=True)),
         "lanes4_cap64": (bs.S4_64, {}), "lanes4_cap128": (bs.S4_128, {}),
         "lanes8_cap64": (bs.S8_64, {}), "lanes8_cap128": (bs.S8_128, {}),
         "lanes8_cap64_geo_scan": (bs.S8_64, dict(geo_scan=True))}
SPLIT = {"lanes12_cap64": (bs.S12_64, {}), "lanes12_cap128": (bs.S12_128, {}), "lanes12_cap256": (bs.S12_256, {}),
         "lanes12_cap64_quantised": (bs.S12_64_Q, {}), "lanes12_cap64_general_path": (bs.S12_64, dict(general_path=True)),
         "lanes4_cap64": (bs.S4_64, {}), "lanes8_cap64": (bs.S8_64, {}), "lanes4_cap128": (bs.S4_128, {}), "lanes8_cap128": (bs.S8_128, {})}


@pytest.mark.parametrize("name", sorted(FUSED))
def test_gpu_fused_ticks_vs_bounded_oracle(name):
    scn, kw = FUSED[name]
    bs.check_fused_bounded(BACKEND, scn, **kw)


@pytest.mark.parametrize("name", sorted(SPLIT))
def test_gpu_split_protocol_vs_bounded_oracle(name):
    scn, kw = SPLIT[name]
    bs.check_split_bounded(BACKEND, scn, **kw)


# (rows="post": without the training outputs -- only then does the 128-slot queue form run its HOME build; the table source
#  gathers a granted spawn's first action behind FIN, where the grant is known)
ROLLOUT = {"resident_cap64_pool": (bs.S12_64, dict(chunk=0)), "resident_cap64_table": (bs.S12_64_TABLE, dict(chunk=0)),
           "resident_cap128_pool": (bs.S12_128, dict(chunk=0)), "resident_cap128_table": (bs.S12_128_TABLE, dict(chunk=0)),
           "resident_cap128_pool_chunked": (bs.S12_128, dict(chunk=13, rows="post")),
           "queue_cap64_pool": (bs.S12_64, dict(persistent=True, chunk=13)), "queue_cap64_table": (bs.S12_64_TABLE, dict(persistent=True, chunk=13)),
           "queue_cap64_pool_post_rows": (bs.S12_64, dict(persistent=True, chunk=13, rows="post")),
           "queue_cap128_pool_training_rows": (bs.S12_128, dict(persistent=True, chunk=13)),
           "home_cap128_pool": (bs.S12_128, dict(persistent=True, chunk=13, rows="post")),
           "home_cap128_table": (bs.S12_128_TABLE, dict(persistent=True, chunk=13, rows="post")),
           "resident_cap256": (bs.S12_256, dict(chunk=0)), "queue_cap256": (bs.S12_256, dict(persistent=True, chunk=13)),
           "resident_lanes4": (bs.S4_64, dict(chunk=0)), "queue_lanes4": (bs.S4_64, dict(persistent=True, chunk=13)),
           "resident_lanes8": (bs.S8_64, dict(chunk=0)), "queue_lanes8": (bs.S8_64, dict(persistent=True, chunk=13))}


@pytest.mark.parametrize("name", sorted(ROLLOUT))
def test_gpu_rollout_blocks_vs_bounded_oracle(name):
    scn, kw = ROLLOUT[name]
    bs.check_rollout_bounded(BACKEND, scn, want_launch="persistent" if kw.get("persistent") else "resident", **kw)


@pytest.mark.parametrize("capacity", [64, 128])
def test_gpu_closed_loop_on_a_full_batch(capacity):
    """PVE_SRC_ACTOR, every slot full: persistent == resident == two launches, bit for bit, overflow > 0 in every env.  A
    self-comparison: the float32 actor cannot be held to the FP64 oracle at 1e-9 (bounded_scenarios.check_closed_loop_full)."""
    m = bs.check_closed_loop_full(BACKEND, capacity)
    assert m["overflow"] > 0


# fresh random actions every tick (no pool); the last column: the deferred spawns of the three envs, counted by the oracles
FUZZ = [(12, 64, 1500.0, 7, 300, 4442), (12, 128, 6000.0, 7, 400, 7267), (4, 64, 5000.0, 9, 300, 104), (8, 64, 3000.0, 9, 300, 3015),
        (8, 128, 6000.0, 9, 350, 325)]


@pytest.mark.parametrize("lane_num,capacity,rate,seed,ticks,deferred", FUZZ)
def test_gpu_fuzz_tapes_vs_bounded_oracle(lane_num, capacity, rate, seed, ticks, deferred):
    """scenarios.check_fuzz_vs_oracle / check_geo_fuzz_vs_oracle in their bounded mode"""
    from tests import scenarios
    if lane_num == 12:
        scenarios.check_fuzz_vs_oracle(BACKEND, 3, capacity, ticks, rate, seed, bounded=True)
        assert scenarios.check_fuzz_vs_oracle.overflow == deferred
    else:
        scenarios.check_geo_fuzz_vs_oracle(BACKEND, lane_num, 3, capacity, ticks, rate, seed, bounded=True)
        assert scenarios.check_geo_fuzz_vs_oracle.overflow == deferred


def test_gpu_full_intersection_split_protocol_at_256():
    from tests import cap256_scenarios as cs
    b = cs.check_full_split(BACKEND)
    assert b.metrics()["overflow"] == 464 and b.metrics()["locks"] == 198

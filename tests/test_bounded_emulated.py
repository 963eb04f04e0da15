"""CPU: the emulated kernels (tests/emu, tests/emu_wide) against capacity-bound oracles, through every deferred spawn of a full
intersection (tests/bounded_scenarios.py; the rule and its link to the reference: tests/test_oracle_bounded.py).
The `-m gpu` twin is test_gpu_bounded.py."""
import pytest

from tests import bounded_scenarios as bs
from tests import hip_adapter
from tests.test_capacity256 import wide_lib

BACKEND = "emu"


@pytest.fixture
def wide(monkeypatch):
    lib = wide_lib()
    monkeypatch.setattr(hip_adapter, "emulator_lib", lambda: lib)
    return lib


FUSED = {"lanes12_cap64": (bs.S12_64, {}), "lanes12_cap128": (bs.S12_128, {}),
         "lanes12_cap64_quantised": (bs.S12_64_Q, {}), "lanes12_cap64_table": (bs.S12_64_TABLE, {}),
         "lanes12_cap64_general_path": (bs.S12_64, dict(general_path=True)),
         "lanes12_cap128_general_path": (bs.S12_128, dict(general_path=True)),
         "lanes4_cap64": (bs.S4_64, {}), "lanes4_cap128": (bs.S4_128, {}),
         "lanes8_cap64": (bs.S8_64, {}), "lanes8_cap128": (bs.S8_128, {}),
         "lanes8_cap64_geo_scan": (bs.S8_64, dict(geo_scan=True))}
SPLIT = {"lanes12_cap64": (bs.S12_64, {}), "lanes12_cap128": (bs.S12_128, {}), "lanes12_cap64_quantised": (bs.S12_64_Q, {}),
         "lanes12_cap64_general_path": (bs.S12_64, dict(general_path=True)),
         "lanes4_cap64": (bs.S4_64, {}), "lanes8_cap64": (bs.S8_64, {}), "lanes4_cap128": (bs.S4_128, {}), "lanes8_cap128": (bs.S8_128, {})}


@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_ticks_vs_bounded_oracle(name):
    scn, kw = FUSED[name]
    bs.check_fused_bounded(BACKEND, scn, **kw)


@pytest.mark.parametrize("name", sorted(SPLIT))
def test_split_protocol_vs_bounded_oracle(name):
    scn, kw = SPLIT[name]
    bs.check_split_bounded(BACKEND, scn, **kw)


def test_fused_ticks_vs_bounded_oracle_at_256(wide):
    bs.check_fused_bounded(BACKEND, bs.S12_256)


def test_split_protocol_vs_bounded_oracle_at_256(wide):
    bs.check_split_bounded(BACKEND, bs.S12_256)


ROLLOUT = {"resident_cap64_pool": (bs.S12_64, dict(chunk=0)), "resident_cap64_table": (bs.S12_64_TABLE, dict(chunk=0)),
           "resident_cap128_pool": (bs.S12_128, dict(chunk=0)), "resident_cap128_table": (bs.S12_128_TABLE, dict(chunk=0)),
           "queue_cap64_pool": (bs.S12_64, dict(persistent=True, chunk=13)), "queue_cap64_table": (bs.S12_64_TABLE, dict(persistent=True, chunk=13)),
           "queue_cap128_pool": (bs.S12_128, dict(persistent=True, chunk=13, rows="post")),
           "queue_cap128_table": (bs.S12_128_TABLE, dict(persistent=True, chunk=13, rows="post")),
           "resident_lanes4": (bs.S4_64, dict(chunk=0)), "queue_lanes4": (bs.S4_64, dict(persistent=True, chunk=13)),
           "resident_lanes8": (bs.S8_64, dict(chunk=0)), "queue_lanes8": (bs.S8_64, dict(persistent=True, chunk=13))}


@pytest.mark.parametrize("name", sorted(ROLLOUT))
def test_rollout_blocks_vs_bounded_oracle(name):
    scn, kw = ROLLOUT[name]
    bs.check_rollout_bounded(BACKEND, scn, want_launch="persistent" if kw.get("persistent") else "resident", **kw)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("scn", [bs.S12_128, bs.S12_128_TABLE], ids=["pool", "table"])
def test_home_block_rollout_blocks_vs_bounded_oracle(monkeypatch, mode, scn):
    """the HOME block (entry pool of 304 / 296 entries worked in passes: reached only with a full intersection) through the
    work queue; the table source gathers a granted spawn's first action behind FIN"""
    import ctypes as C
    monkeypatch.setenv("PVE_EMU_HOME", str(mode))
    lib = hip_adapter.emulator_lib()
    lib.pve_emu_max_passes.restype = C.c_int
    lib.pve_emu_max_passes()
    bs.check_rollout_bounded(BACKEND, scn, persistent=True, chunk=13, rows="post", want_launch="persistent")
    assert int(lib.pve_emu_max_passes()) >= 2, "a full intersection must take several passes of the entry pool"


@pytest.mark.parametrize("persistent", [False, True])
def test_rollout_blocks_vs_bounded_oracle_at_256(wide, persistent):
    bs.check_rollout_bounded(BACKEND, bs.S12_256, persistent=persistent, chunk=13 if persistent else 0,
                             want_launch="persistent" if persistent else "resident")


@pytest.mark.parametrize("capacity", [64, 128])
def test_closed_loop_on_a_full_batch(capacity):
    bs.check_closed_loop_full(BACKEND, capacity)


# fresh random actions every tick (no pool); the last column: the deferred spawns of the three envs, counted by the oracles
FUZZ = [(12, 64, 1500.0, 7, 300, 4442), (12, 128, 6000.0, 7, 400, 7267), (4, 64, 5000.0, 9, 300, 104), (8, 64, 3000.0, 9, 300, 3015),
        (8, 128, 6000.0, 9, 350, 325)]


@pytest.mark.parametrize("lane_num,capacity,rate,seed,ticks,deferred", FUZZ)
def test_fuzz_tapes_vs_bounded_oracle(lane_num, capacity, rate, seed, ticks, deferred):
    """scenarios.check_fuzz_vs_oracle / check_geo_fuzz_vs_oracle in their bounded mode"""
    from tests import scenarios
    if lane_num == 12:
        scenarios.check_fuzz_vs_oracle(BACKEND, 3, capacity, ticks, rate, seed, bounded=True)
        assert scenarios.check_fuzz_vs_oracle.overflow == deferred
    else:
        scenarios.check_geo_fuzz_vs_oracle(BACKEND, lane_num, 3, capacity, ticks, rate, seed, bounded=True)
        assert scenarios.check_geo_fuzz_vs_oracle.overflow == deferred


def test_full_intersection_split_protocol_at_256(wide):
    from tests import cap256_scenarios as cs
    b = cs.check_full_split(BACKEND)
    assert b.metrics()["overflow"] == 464 and b.metrics()["locks"] == 198

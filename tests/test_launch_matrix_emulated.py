"""The launch matrix of pve_step_many (tests/launch_matrix_scenarios.py) on CPU, through the emulator backends and with their
own expected table: the frozen emulator for 64 / 128 slots, the wide emulator for 256.  The `-m gpu` twin is
test_gpu_launch_matrix.py."""
import pytest

from tests import hip_adapter
from tests import launch_matrix_scenarios as lm
from tests.test_capacity256 import wide_lib

CASES = lm.matrix()


@pytest.mark.parametrize("case", CASES, ids=lm.case_id)
def test_launch_matrix_emulated(case, monkeypatch):
    if case.capacity == 256:
        lib = wide_lib()
        monkeypatch.setattr(hip_adapter, "emulator_lib", lambda: lib)
    lm.run_case("emu", case, lm.expected_emulated(case), lm.expected_emulated_variant(case))


def test_variant_table_is_literal_and_home_holds_exactly_where_stated():
    """the GPU table of variants: one row per row of the kind table; HOME (5) exactly for 12 lanes, 128 slots, the queue form,
    zero / pool / table, no training outputs; the flags as requested; prof nowhere"""
    assert set(lm.GPU_VARIANTS) == set(lm.GPU_TABLE)
    home = [c for c in CASES if lm.expected_gpu_variant(c)["waves_per_simd"] == 5]
    assert sorted(lm.case_id(c) for c in home) == ["l12-c128-pool-plain-queue-f32", "l12-c128-table-plain-queue-f64",
                                                   "l12-c128-zero-plain-queue-f64"]
    for c in CASES:
        v = lm.expected_gpu_variant(c)
        assert v["prof"] == 0 and v["kind"] == lm.expected_gpu(c)
        if v["kind"] != "tick":
            assert (v["table"], v["train"], v["actor"]) == (int(c.source == "table"), int(c.train), int(c.source == "actor")), c
            assert v["waves_per_simd"] in (4, 5) and v["grid"] == (15 if v["kind"] == "persistent" else 5)


def test_matrix_covers_every_accepted_combination():
    # 12 lanes: 3 capacities x 4 sources x 2 x 2; 4 and 8 lanes: 2 capacities x (4 sources x 2 - table with training) x 2; + 2
    assert len(CASES) == 48 + 2 * 2 * 7 * 2 + 2 and len(set(CASES)) == len(CASES)
    assert sum(c.obs_f32 for c in CASES[:-2]) * 2 == len(CASES) - 2
    assert {lm.expected_gpu(c) for c in CASES} == {"tick", "resident", "persistent"}


@pytest.mark.parametrize("lane_num", [4, 8])
def test_table_with_training_outputs_refused_emulated(lane_num):
    lm.check_refusal("emu", lane_num)

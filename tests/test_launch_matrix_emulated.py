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
    lm.run_case("emu", case, lm.expected_emulated(case))


def test_matrix_covers_every_accepted_combination():
    # 12 lanes: 3 capacities x 4 sources x 2 x 2; 4 and 8 lanes: 2 capacities x (4 sources x 2 - table with training) x 2; + 2
    assert len(CASES) == 48 + 2 * 2 * 7 * 2 + 2 and len(set(CASES)) == len(CASES)
    assert sum(c.obs_f32 for c in CASES[:-2]) * 2 == len(CASES) - 2
    assert {lm.expected_gpu(c) for c in CASES} == {"tick", "resident", "persistent"}


@pytest.mark.parametrize("lane_num", [4, 8])
def test_table_with_training_outputs_refused_emulated(lane_num):
    lm.check_refusal("emu", lane_num)

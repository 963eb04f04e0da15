"""The launch matrix of pve_step_many (tests/launch_matrix_scenarios.py) on an MI355X: which kernel form every accepted
configuration launches (last_launch() against the literal table) and that it computes what one launch per tick computes.
The CPU twin is test_launch_matrix_emulated.py."""
import pytest

from tests import launch_matrix_scenarios as lm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", lm.matrix(), ids=lm.case_id)
def test_gpu_launch_matrix(case):
    lm.run_case("hip", case, lm.expected_gpu(case), lm.expected_gpu_variant(case))


@pytest.mark.parametrize("lane_num", [4, 8])
def test_gpu_table_with_training_outputs_refused(lane_num):
    lm.check_refusal("hip", lane_num)

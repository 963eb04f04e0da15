"""-m gpu: RANK on pairs of list entries in the HOME build of the 128-slot queue kernel (k_rollout<128, 5, ..>), through
pve_step_many(source="table", persistent=True, chunk=...), against the sequential oracle: every retained tick, every field, then
the header and the persistent state (tests/rank_pairs_scenarios.py; the CPU twin, tests/test_rank_pairs_emulated.py, runs the same
streams through the emulator, reports the list lengths and fix-ups they cause and drives the tie inside one pair)."""
import pytest

from tests import rank_pairs_scenarios as R

pytestmark = pytest.mark.gpu
BACKEND = "hip"


def test_gpu_rank_pairs_traffic_from_empty():
    run = R.check_queue_kernel_vs_oracle(BACKEND, R.TRAFFIC)
    assert run.max_ctl > 8


def test_gpu_rank_pairs_symmetric_lanes_equal_distances():
    run = R.check_queue_kernel_vs_oracle(BACKEND, R.SYMMETRIC)
    assert R.equal_distance_pairs(run, R.SYMMETRIC) > 0


def test_gpu_rank_pairs_quantised_tape_near_ties():
    run = R.check_queue_kernel_vs_oracle(BACKEND, R.QUANTISED)
    assert run.max_ctl > 20


def test_gpu_rank_pairs_full_intersection_multi_pass():
    """more than 80 controlled vehicles: more than 304 list entries (asserted on the emulator with the same stream), i.e. several
    BUILD .. WALK passes with the grouped RANK"""
    run = R.check_queue_kernel_vs_oracle(BACKEND, R.FULL)
    assert run.max_ctl > 80 and sum(run.overflow) > 0

"""-m gpu: the side jobs of the HOME block (csrc/pve_tick_core.h, Shared<128, false, true>::SIDE) on the device,
where the two waves of a workgroup really run side by side: the three shapes of tests/test_side_jobs_emulated.py through the
work queue == single ticks of k_tick bit for bit (scenarios.check_step_many asserts last_launch() == "persistent")."""
import pytest

from tests import side_jobs_scenarios as S

pytestmark = pytest.mark.gpu
BACKEND = "hip"


def test_gpu_side_jobs_dense_vehicles_all_in_the_first_wave():
    st = S.run(BACKEND, S.WAVE0, n_envs=9)
    print(st)
    assert st["locks"] > 0 and st["collided"] > 0, st


def test_gpu_side_jobs_controlled_count_crosses_64():
    st = S.run(BACKEND, S.CROSSING, n_envs=6)
    print(st)
    assert st["locks"] > 0 and st["collided"] > 0, st
    n_ctl = S.controlled_per_tick(BACKEND, S.CROSSING, n_envs=6)
    assert (n_ctl > 64).any() and ((n_ctl > 0) & (n_ctl <= 64)).any(), "the controlled count must lie on both sides of 64"
    assert int(n_ctl.sum()) == int(st["ctl_steps"]), "the trajectory call is not the run the metrics are of"


def test_gpu_side_jobs_more_than_64_controlled_throughout():
    st = S.run(BACKEND, S.FULL, n_envs=6)
    print(st)
    assert st["locks"] > 0, st
    assert st["mean_ctl"] > 64 and st["overflow"] > 0, st

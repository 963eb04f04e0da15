"""The 256-slot capacity of the 12-lane fast path on an MI355X: k_tick<256>, k_compact<256>, k_reset<256> and the
k_rollout<256, ..> variants against the CPU oracle (the CPU twin, test_capacity256.py, runs the same phases in the wide
emulator), plus the BASELINE-size checks at 1100 veh/h/lane -- the rate at which 128 slots defer spawns in the closed loop."""
import pytest

from pve_mcc_amd import _capi
from tests import cap256_scenarios as cs
from tests import scenarios
from tests.hip_adapter import SplitEnv, make_batch
from tests.parity_util import GoldenCase, replay_case

pytestmark = pytest.mark.gpu
BACKEND = "hip"


def test_gpu_library_accepts_256():
    lib = _capi.load_library()
    assert lib.pve_workspace_bytes(4096, 256) > lib.pve_workspace_bytes(4096, 128) > 0
    assert lib.pve_workspace_bytes(4096, 192) == 0


@pytest.mark.parametrize("env", range(cs.DENSE_ENVS))
def test_gpu_dense_split_protocol_vs_oracle(env):
    cs.check_dense_split(BACKEND, env)


def test_gpu_dense_stream_overflows_128_slots():
    cs.check_dense_overflows_128(BACKEND, 1)


def test_gpu_dense_fused_equals_split():
    cs.check_dense_fused(BACKEND, 2)


@pytest.mark.parametrize("source", ["pool", "zero", "table", "actor"])
@pytest.mark.parametrize("persistent", [False, True])
def test_gpu_dense_step_many(source, persistent):
    cs.check_dense_step_many(BACKEND, source, persistent=persistent)


@pytest.mark.parametrize("persistent,source,chunk", [(False, "pool", 0), (False, "pool", 7), (True, "pool", 7), (False, "table", 0)])
def test_gpu_dense_training_rows_vs_oracle(persistent, source, chunk):
    cs.check_dense_training_rows(BACKEND, persistent=persistent, source=source, chunk=chunk)


@pytest.mark.parametrize("name", ["s1000_zero", "s1000_sin1", "s1200_sin1", "s1200_zero", "s1000_actor"])
def test_gpu_golden_at_256(name):
    case = GoldenCase(name)
    b = make_batch(case.arrive, 1, 256, BACKEND, **case.ctor)
    replay_case(case, SplitEnv(b), ftol=1e-9, dtol=1e-9, want_state=False)
    assert b.metrics()["overflow"] == 0


def test_gpu_capacity_equivalence_128_vs_256():
    cs.check_capacity_equivalence(BACKEND, n_envs=16)


def test_gpu_step_many_at_256():
    scenarios.check_step_many(BACKEND, "pool", n_envs=6, capacity=256, chunks=(1, 7, 40, 3, 60), trajectory_chunk=12)
    scenarios.check_step_many_state_rows(BACKEND, n_envs=4, capacity=256, calls=(40, 25, 60, 35), chunk=7)


def test_gpu_full_size_vs_oracle_at_256():
    """4096 x 256 slots at 1100 veh/h/lane, 16 sampled oracles, no deferred spawn anywhere"""
    scenarios.check_full_size_vs_oracle(BACKEND, 4096, 256, 1100.0)
    scenarios.check_full_size_vs_oracle(BACKEND, 4096, 256, 1100.0, many=20)


def test_gpu_driver_shape_vs_oracle_at_256():
    scenarios.check_driver_shape_vs_oracle(BACKEND, capacity=256, rate=1100.0)
    scenarios.check_driver_shape_vs_oracle(BACKEND, capacity=256, rate=1100.0, persistent=True, table=True)


def test_gpu_closed_loop_at_1100_with_256_slots():
    """BASELINE config 5 at its stated 1100 veh/h/lane (128 slots defer spawns there): the actor inside k_rollout<256, .., ACT>
    bit-equal to actor + tick launches, 0 overflow on every env"""
    scenarios.check_closed_loop_rollout_vs_two_launch(BACKEND, capacity=256, rate=1100.0)
    scenarios.check_closed_loop_rollout_vs_two_launch(BACKEND, capacity=256, rate=1100.0, persistent=True)

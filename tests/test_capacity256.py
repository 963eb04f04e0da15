"""CPU tests of the 256-slot capacity of the 12-lane fast path: the C ABI of the cross-compiled HIP library accepts it, the
frozen 64 / 128 emulator (tests/emu) still refuses it, and the phase bodies at 256 slots -- run by the wide emulator
(tests/emu_wide, the 256-slot kernels' phase order) -- follow the oracle on a stream that peaks far above 128 vehicles.
The `-m gpu` twin is test_gpu_capacity256.py."""
import pytest

from pve_mcc_amd import _capi
from pve_mcc_amd._capi import PveError
from pve_mcc_amd.arrivals import synthetic_arrivals
from tests import cap256_scenarios as cs
from tests import hip_adapter, native, scenarios
from tests.hip_adapter import make_batch
from tests.parity_util import GoldenCase, replay_case


def wide_lib():
    return native.load_emulator("emu_wide", "libpveenv_emu_wide.so")


@pytest.fixture
def wide(monkeypatch):
    """backend "emu" of the shared scenario helpers runs on the wide emulator for the duration of a test"""
    lib = wide_lib()
    monkeypatch.setattr(hip_adapter, "emulator_lib", lambda: lib)
    return lib


def test_hip_library_accepts_256():
    lib = _capi.load_library()
    assert lib.pve_workspace_bytes(4096, 256) > lib.pve_workspace_bytes(4096, 128) > 0
    assert lib.pve_workspace_bytes(4096, 192) == 0
    assert lib.pve_workspace_bytes(4096, 512) == 0


def test_frozen_emulator_refuses_256():
    lib = hip_adapter.emulator_lib()
    assert lib.pve_workspace_bytes(4, 128) > 0
    assert lib.pve_workspace_bytes(4, 256) == 0


@pytest.mark.parametrize("kw", [dict(lane_num=4), dict(lane_num=8), dict(general_path=True)])
def test_256_refused_off_the_fast_path(wide, kw):
    arr = synthetic_arrivals(1, 1000.0, 60.0, lane_num=kw.get("lane_num", 12))[0]
    with pytest.raises(PveError, match="capacity 256 needs lane_num 12"):
        make_batch(arr, 1, 256, "emu", **kw)


def test_wide_emulator_refuses_other_capacities(wide):
    assert wide.pve_workspace_bytes(4, 192) == 0 and wide.pve_workspace_bytes(4, 512) == 0
    with pytest.raises(PveError, match="64, 128 or 256"):
        make_batch(cs.dense_arrivals(1)[0], 1, 192, "emu")


def test_dense_scenario_lies_between_128_and_256():
    peaks = [cs.oracle_peak(cs.dense_arrivals()[e]) for e in range(cs.DENSE_ENVS)]
    assert all(160 <= p <= 250 for p in peaks), peaks


@pytest.mark.parametrize("env", range(cs.DENSE_ENVS))
def test_dense_split_protocol_vs_oracle(wide, env):
    cs.check_dense_split("emu", env)


def test_dense_stream_overflows_128_slots(wide):
    cs.check_dense_overflows_128("emu", 1)


def test_dense_fused_equals_split(wide):
    cs.check_dense_fused("emu", 1, ticks=260)


@pytest.mark.parametrize("source", ["pool", "zero", "table", "actor"])
def test_dense_step_many_chunked(wide, source):
    cs.check_dense_step_many("emu", source)


@pytest.mark.parametrize("source", ["pool", "table"])
def test_dense_step_many_queue(wide, source):
    cs.check_dense_step_many("emu", source, persistent=True)


@pytest.mark.parametrize("persistent,source", [(False, "pool"), (True, "pool"), (False, "table")])
def test_dense_training_rows_vs_oracle(wide, persistent, source):
    cs.check_dense_training_rows("emu", persistent=persistent, source=source, chunk=7 if persistent else 0)


@pytest.mark.parametrize("name", ["s1000_zero", "s1000_sin1", "s1200_sin1", "s1200_zero", "s1000_actor"])
def test_golden_at_256(wide, name):
    case = GoldenCase(name)
    b = make_batch(case.arrive, 1, 256, "emu", **case.ctor)
    replay_case(case, hip_adapter.SplitEnv(b), ftol=1e-9, dtol=1e-9, want_state=False)
    assert b.metrics()["overflow"] == 0


def test_capacity_equivalence_128_vs_256(wide):
    cs.check_capacity_equivalence("emu")


def test_wide_emulator_matches_frozen_emulator_at_128(wide):
    """the wide emulator's 128-slot loops are the frozen emulator's (same phase order): same records on a golden case"""
    scenarios.check_split_vs_oracle(GoldenCase("s1000_sin3"), "emu", ticks=200)

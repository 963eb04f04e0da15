"""The generators' and replay helpers' PVE_HD functions in isolation, DEVICE build (hipcc, the product's HIPFLAGS, gfx950):
the scenarios of tests/gen_probe_scenarios.py on the device and the device build against the host build bit for bit (all
but prio_weight, whose powf is libm's on the host and ocml's on the device).  Every call launches one bounds-checked
element-wise kernel over at most 2^22 elements and returns the hipError_t, which the wrapper asserts to be 0.  The
device object travels with the tree (tests/test_math_probe.py builds it); if it can neither be found nor built the tests fail."""
import pytest

from tests import gen_probe_scenarios as S

pytestmark = pytest.mark.gpu
_probes = {}


def probe(kind="hip"):
    if kind not in _probes:
        _probes[kind] = S.Probe(kind, always_make=False)
    return _probes[kind]


def test_gpu_device_build_equals_host_build_bit_for_bit():
    S.check_bit_equal(probe(), probe("host"))


def test_gpu_philox_known_answers_and_numpy():
    S.check_philox(probe())


def test_gpu_noise_gauss_at_the_edge_words():
    S.check_noise_gauss(probe())


def test_gpu_arrival_exp_at_the_edge_words():
    S.check_arrival_exp(probe())


def test_gpu_action_noise_and_the_noisy_action():
    S.check_action_noise(probe())


def test_gpu_arrival_gap_either_side_of_min_gap():
    S.check_arrival_gap(probe())


def test_gpu_arrival_and_intention_words():
    S.check_stream_words(probe())


def test_gpu_replay_half_bits():
    S.check_half_bits(probe())


def test_gpu_replay_perm_is_the_models_permutation():
    S.check_perm(probe())


def test_gpu_replay_append_plan_and_slot():
    S.check_append(probe())


def test_gpu_prio_update_bits_and_key():
    S.check_prio_bits(probe())


def test_gpu_prio_update_slot():
    S.check_prio_slot(probe())


def test_gpu_prio_partition_at_every_threshold():
    S.check_prio_partition(probe())


def test_gpu_prio_draw_rank():
    S.check_prio_draw(probe())


def test_gpu_prio_weight():
    S.check_prio_weight(probe())

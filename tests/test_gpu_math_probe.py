"""The tick's arithmetic helpers in isolation, DEVICE build (hipcc, the product's HIPFLAGS, gfx950): the checks of
tests/math_probe_scenarios.py on the device, the comparison of the device build with the host build bit for bit, and the
device-only helpers (value_div's reciprocal + Newton form, the actor's activation).  Every entry point launches one
bounds-checked element-wise kernel and returns the hipError_t, which the probe wrapper asserts to be 0.

The device object normally travels with the tree (tests/test_math_probe.py builds it); it is rebuilt only if it is missing
or older than its sources.  If it can neither be found nor built the tests fail."""
import pytest

from tests import math_probe_scenarios as S
from tests.test_math_probe import GEO_CASES, PAIR_CASES

pytestmark = pytest.mark.gpu
_probes = {}


def probe(kind="hip"):
    if kind not in _probes:
        _probes[kind] = S.Probe(kind, always_make=False)
    return _probes[kind]


def test_gpu_refused_arguments():
    S.check_refused_arguments(probe())


def test_gpu_device_build_equals_host_build_bit_for_bit():
    S.check_bit_equal(probe(), probe("host"))


# ------------------------------------------------------------------ decisions: zero tolerance
def test_gpu_div_const_is_ieee_division():
    S.check_div_const(probe())


def test_gpu_brake_needed_is_the_true_division_form():
    S.check_brake_needed(probe())


def test_gpu_min_max_are_compare_and_select():
    S.check_min_max(probe())


def test_gpu_clip_a_and_the_speed_clamp_at_their_bounds():
    S.check_clamps(probe())


def test_gpu_key_less_and_24_bit_products():
    S.check_key_less(probe())
    S.check_mul24(probe())


def test_gpu_word_helpers():
    S.check_words(probe())


@pytest.mark.parametrize("NW", [1, 2, 4])
def test_gpu_mask_helpers(NW):
    S.check_masks(probe(), NW)


def test_gpu_collision_distance_sqrt():
    S.check_sqrt(probe())


# ------------------------------------------------------------------ reward values
def test_gpu_exp_m2_0():
    S.check_exp(probe())


def test_gpu_reward_coth_term():
    S.check_coth(probe())


def test_gpu_reward_log_term():
    S.check_log(probe())


def test_gpu_value_div_within_2_ulp():
    S.check_value_div(probe())


# ------------------------------------------------------------------ geometry values
def test_gpu_sincos_q1():
    S.check_sincos(probe())


def test_gpu_xy_vs_the_reference_tables():
    S.check_xy_golden(probe())


@pytest.mark.parametrize("lane_num,gname", GEO_CASES)
def test_gpu_xy_vs_the_oracle_sweep(lane_num, gname):
    S.check_xy_oracle(probe(), lane_num, gname)


# ------------------------------------------------------------------ pre-filter soundness
def test_gpu_frcp():
    S.check_frcp(probe())


@pytest.mark.parametrize("lane_num,gname", GEO_CASES)
def test_gpu_f32_twins(lane_num, gname):
    S.check_f32_twins(probe(), lane_num, gname)


@pytest.mark.parametrize("lane_num,gname,thr", PAIR_CASES)
def test_gpu_prefilter_drops_no_collision(lane_num, gname, thr):
    S.check_prefilter_pairs(probe(), lane_num, gname, thr)


# ------------------------------------------------------------------ the actor's activation
def test_gpu_actor_tanh3():
    S.check_actor_tanh3(probe())

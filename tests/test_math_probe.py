"""The tick's arithmetic helpers in isolation, HOST build (g++, the flags of tests/emu: the branches the CPU emulator runs).
The checks live in tests/math_probe_scenarios.py and take the backend as an argument; tests/test_gpu_math_probe.py runs the
same checks on the device build.  This module builds BOTH flavours with `make`, so that a cross-compile error of the device
object shows here and the object travels with the tree."""
import os

import pytest

from tests import math_probe_scenarios as S

_probe = None


def host():
    global _probe
    if _probe is None:
        _probe = S.Probe("host")
    return _probe


def test_both_flavours_build_and_the_device_flags_are_the_products():
    """The device object is compiled with exactly the product's HIPFLAGS (asked of csrc/Makefile, recorded next to the object)
    == what the product library's build recorded in libpveenv.flags.  Both are shared objects: nothing to subtract."""
    S.build("host")
    S.build("hip")
    with open(os.path.join(S.PROBE_DIR, "libpve_math_probe_hip.flags")) as f:
        mine = f.read().split()
    with open(os.path.join(os.path.dirname(S.CSRC_DIR), "libpveenv.flags")) as f:
        product = f.read().split()
    assert mine == product
    assert "-ffp-contract=off" in mine and "--offload-arch=gfx950" in mine


def test_refused_arguments():
    S.check_refused_arguments(host())


# ------------------------------------------------------------------ decisions: zero tolerance
def test_div_const_is_ieee_division():
    S.check_div_const(host())


def test_brake_needed_is_the_true_division_form():
    S.check_brake_needed(host())


def test_min_max_are_compare_and_select():
    S.check_min_max(host())


def test_clip_a_and_the_speed_clamp_at_their_bounds():
    S.check_clamps(host())


def test_key_less_and_24_bit_products():
    S.check_key_less(host())
    S.check_mul24(host())


def test_word_helpers():
    S.check_words(host())


@pytest.mark.parametrize("NW", [1, 2, 4])
def test_mask_helpers(NW):
    S.check_masks(host(), NW)


def test_collision_distance_sqrt():
    S.check_sqrt(host())


# ------------------------------------------------------------------ reward values
def test_exp_m2_0():
    S.check_exp(host())


def test_reward_coth_term():
    S.check_coth(host())


def test_reward_log_term():
    S.check_log(host())


def test_value_div_is_exact_on_the_host():
    S.check_value_div(host())


# ------------------------------------------------------------------ geometry values
def test_sincos_q1():
    S.check_sincos(host())


def test_xy_vs_the_reference_tables():
    S.check_xy_golden(host())


GEO_CASES = [(ln, g) for g, _ in S.GEOMETRIES for ln in (12, 4, 8)]


@pytest.mark.parametrize("lane_num,gname", GEO_CASES)
def test_xy_vs_the_oracle_sweep(lane_num, gname):
    S.check_xy_oracle(host(), lane_num, gname)


# ------------------------------------------------------------------ pre-filter soundness
def test_frcp():
    S.check_frcp(host())


@pytest.mark.parametrize("lane_num,gname", GEO_CASES)
def test_f32_twins(lane_num, gname):
    S.check_f32_twins(host(), lane_num, gname)


PAIR_CASES = [(12, "default", 2.0), (12, "kw", 3.0), (12, "wide", 2.0), (4, "default", 2.0), (4, "kw", 3.0), (8, "default", 2.0), (8, "kw", 3.0)]


@pytest.mark.parametrize("lane_num,gname,thr", PAIR_CASES)
def test_prefilter_drops_no_collision(lane_num, gname, thr):
    S.check_prefilter_pairs(host(), lane_num, gname, thr)

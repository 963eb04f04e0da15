"""The generators' and replay helpers' PVE_HD functions in isolation, HOST build (g++): every scenario of
tests/gen_probe_scenarios.py, which tests/test_gpu_gen_probe.py runs on the device build.  The edge words of the scenarios --
every binade's fold, the quadrant and octant borders -- also go through the g++ builds of the single headers
(tests/noise_host, tests/arrivals_host) against the NumPy restatements, beside what tests/test_action_noise.py and
tests/test_arrivals_device.py assert with their own lists."""
import numpy as np

from pve_mcc_amd import arrivals, noise
from tests import gen_probe_scenarios as S

_probe = None


def host():
    global _probe
    if _probe is None:
        _probe = S.Probe("host")
    return _probe


def test_philox_known_answers_and_numpy():
    S.check_philox(host())


def test_noise_gauss_at_the_edge_words():
    S.check_noise_gauss(host())


def test_arrival_exp_at_the_edge_words():
    S.check_arrival_exp(host())


def test_action_noise_and_the_noisy_action():
    S.check_action_noise(host())


def test_arrival_gap_either_side_of_min_gap():
    S.check_arrival_gap(host())


def test_arrival_and_intention_words():
    S.check_stream_words(host())


def test_replay_half_bits():
    S.check_half_bits(host())


def test_replay_perm_is_the_models_permutation():
    S.check_perm(host())


def test_replay_append_plan_and_slot():
    S.check_append(host())


def test_prio_update_bits_and_key():
    S.check_prio_bits(host())


def test_prio_update_slot():
    S.check_prio_slot(host())


def test_prio_partition_at_every_threshold():
    S.check_prio_partition(host())


def test_prio_draw_rank():
    S.check_prio_draw(host())


def test_prio_weight():
    S.check_prio_weight(host())


def test_single_header_builds_at_the_edge_words():
    """the g++ shims of pve_noise.h and pve_arrivals.h == NumPy, bit for bit, on the scenarios' edge sets"""
    from tests.test_action_noise import same_bits, shim_gauss
    from tests.test_arrivals_device import host as arrivals_host
    w0, w1 = S.gauss_edge_pairs()
    assert same_bits(shim_gauss(w0, w1), noise.gauss_from_words(w0, w1))
    w = S.radius_words()
    x = np.empty(len(w))
    arrivals_host().arrival_exp_host(w.ctypes.data, len(w), x.ctypes.data)
    assert same_bits(x, arrivals.exp_from_words(w))

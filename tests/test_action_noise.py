"""Exploration noise of the device actor, CPU side: the noise function itself (csrc/pve_noise.h through a g++ host shim and
its NumPy restatement pve_mcc_amd/noise.py) and the C ABI entry point through the CPU test emulator.  The kernels that add
the noise are checked in tests/test_gpu_action_noise.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from pve_mcc_amd import PveError, _capi, noise
from tests import native
from tests.hip_adapter import _np, emulator_lib, make_batch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _signatures(L):
    L.noise_philox.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.noise_gauss_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    L.noise_z_many.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    L.noise_apply.argtypes = [C.c_double, C.c_double, C.c_uint64, C.c_int64, C.c_int32, C.c_uint32]
    L.noise_apply.restype = C.c_double
    return L


def shim():
    """csrc/pve_noise.h compiled by g++ (tests/noise_host), built and loaded by tests/native.py."""
    return native.load("noise_host", "libnoise_host.so", _signatures)


def shim_gauss(w0, w1):
    w0, w1 = np.ascontiguousarray(w0, np.uint32), np.ascontiguousarray(w1, np.uint32)
    out = np.empty(len(w0))
    shim().noise_gauss_many(w0.ctypes.data, w1.ctypes.data, out.ctypes.data, len(w0))
    return out


def shim_z(seed, env, ids, tick):
    env, ids = np.ascontiguousarray(env, np.int64), np.ascontiguousarray(ids, np.int32)
    tick = np.ascontiguousarray(tick, np.uint32)
    out = np.empty(len(env))
    shim().noise_z_many(seed, env.ctypes.data, ids.ctypes.data, tick.ctypes.data, out.ctypes.data, len(env))
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ------------------------------------------------------------------ 1. Philox4x32-10 known answers (Random123's vectors)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    c, k, o = (C.c_uint32 * 4)(*counter), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
    shim().noise_philox(c, k, o)
    assert tuple(o) == want, [hex(x) for x in o]
    got = noise.philox4x32_10([np.array([x]) for x in counter], key)
    assert tuple(int(x[0]) for x in got) == want


# ------------------------------------------------------------------ 2. host shim == NumPy restatement, bit for bit
def libm_gauss(w0, w1):
    u1 = (np.asarray(w0, np.float64) + 0.5) * 2.0 ** -32
    u2 = (np.asarray(w1, np.float64) + 0.5) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def test_shim_and_numpy_are_bit_equal():
    rng = np.random.default_rng(20250213)
    n = 1 << 20
    seeds = [0, 1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0]
    for seed in seeds:
        m = n // len(seeds)
        env = rng.integers(-5, 1 << 40, m)
        env[: m // 2] = rng.integers(0, 4096, m // 2)
        ids = rng.integers(0, 1 << 31, m).astype(np.int32)
        ids[: m // 2] = rng.integers(0, 2000, m // 2)
        tick = rng.integers(0, 1 << 32, m).astype(np.uint32)
        tick[: m // 2] = rng.integers(0, 5000, m // 2)
        z_c, z_np = shim_z(seed, env, ids, tick), noise.action_noise(seed, env, ids, tick)
        assert same_bits(z_c, z_np), "seed %x" % seed
        assert np.all(np.isfinite(z_np))
    # the transform on raw words, the edge words in both positions included
    w0 = rng.integers(0, 1 << 32, n).astype(np.uint32)
    w1 = rng.integers(0, 1 << 32, n).astype(np.uint32)
    edge = [0, 1, 0x3FFFFFFF, 0x40000000, 0x7FFFFFFF, 0x80000000, 0xBFFFFFFF, 0xC0000000, 0xFFFFFFFE, 0xFFFFFFFF]
    k = 0
    for a in edge:
        for b in edge:
            w0[k], w1[k] = a, b
            k += 1
    z_c, z_np = shim_gauss(w0, w1), noise.gauss_from_words(w0, w1)
    assert same_bits(z_c, z_np)
    assert np.all(np.isfinite(z_np)) and np.abs(z_np).max() <= 6.764
    assert abs(z_np[0]) > 6.76                               # word 0 in the radius position: the largest |z|
    # shape accuracy: a condition (1e-6), with a lot of room
    err = np.abs(z_np - libm_gauss(w0, w1)).max()
    print("max |z - z_libm| over 2^20 draws: %.3e" % err)
    assert err <= 1e-6
    # a + sigma z is the float64 expression, product and sum rounded separately
    for a, s, e, i, t in [(0.7312, 0.2, 3, 17, 5), (-2.9999, 0.5, 4095, 1999, 123456)]:
        z = float(noise.action_noise(99, e, i, t))
        assert shim().noise_apply(a, s, 99, e, i, t) == a + s * z


# ------------------------------------------------------------------ 3. distribution, keyed as the kernels key it
def norm_cdf(x):
    return 0.5 * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


def corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_distribution_of_the_keyed_draws():
    E, I, T = 64, 128, 128
    N = E * I * T
    assert N == 1 << 20
    env = np.arange(E)[:, None, None]
    ids = np.arange(I)[None, :, None]
    tick = np.arange(T)[None, None, :]
    z = noise.action_noise(20250213, env, ids, tick)
    z2 = noise.action_noise(20250214, env, ids, tick)
    assert z.shape == (E, I, T)
    mean, var = float(z.mean()), float(z.var())
    zs = np.sort(z.ravel())
    cdf = norm_cdf(zs)
    ks = max(float(np.max(np.arange(1, N + 1) / N - cdf)), float(np.max(cdf - np.arange(0, N) / N)))
    lag = {"tick": corr(z[:, :, 1:], z[:, :, :-1]), "id": corr(z[:, 1:, :], z[:, :-1, :]), "env": corr(z[1:], z[:-1]),
           "seed": corr(z, z2)}
    print("mean %.3e  var - 1 %.3e  KS %.3e  correlations %s" % (mean, var - 1, ks, lag))
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1) <= 5 * math.sqrt(2.0 / N)
    assert ks <= 1.95 / math.sqrt(N)
    for k, v in lag.items():
        assert abs(v) <= 5 / math.sqrt(N), (k, v)


# ------------------------------------------------------------------ 4. the C ABI through the emulator library
def test_abi_version_and_export():
    lib = emulator_lib()
    assert lib.pve_abi_version() == _capi.ABI_VERSION          # (against the header: tests/test_binding_contract.py)
    assert "pve_set_action_noise" in _capi.EXPORTS and hasattr(lib, "pve_set_action_noise")
    header = open(os.path.join(ROOT, "include", "pve_env.h")).read()
    assert "main.py:44, :239" in header


def closed_loop(b, ticks):
    from oracle.actor_np import flat_weights, load_weights
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    rewards = []
    for _ in range(ticks):
        rewards.append(_np(b.step_with_actor()["reward"]).copy())
    b.step_many(8, source="actor")
    fields = {k: _np(b.state_field(k)).copy() for k in ("p", "v", "a", "jerk", "jerk_sum", "vir_dis", "closer_p", "id", "seq",
                                                        "vnum", "step", "count", "meta", "hdr")}
    return rewards, fields, b.metrics()


def test_entry_point_validation_and_noise_off_on_the_emulator():
    from pve_mcc_amd.arrivals import synthetic_arrivals
    lib = emulator_lib()
    arr = synthetic_arrivals(2, rate=1000.0, horizon_s=40.0, seed=5)
    outs = ("obs_post", "reward", "flags", "env_out")
    plain = make_batch(arr, 2, 64, "emu", outputs=outs)
    b = make_batch(arr, 2, 64, "emu", outputs=outs)
    assert lib.pve_set_action_noise(None, 0.0, 0, 0) == -1                 # PVE_ERR_INVALID
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        assert lib.pve_set_action_noise(b._h, bad, 1, 0) == -1, bad
        assert b"sigma" in lib.pve_last_error()
        with pytest.raises(PveError):
            b.set_exploration(bad, seed=1)
    # the emulator has no noisy actor kernels: sigma > 0 is refused, and says why
    assert lib.pve_set_action_noise(b._h, 0.2, 7, 0) == -1
    assert b"backend" in lib.pve_last_error()
    with pytest.raises(PveError, match="backend"):
        b.set_exploration(0.2, seed=7)
    assert b.exploration == (0.0, 0, 0)
    # sigma = 0 is accepted by every backend, whatever the other arguments
    assert lib.pve_set_action_noise(b._h, 0.0, 0xFFFFFFFFFFFFFFFF, -3) == 0
    b.set_exploration(0.0, seed=12345, env_offset=77)
    assert b.exploration == (0.0, 12345, 77)
    r0, f0, m0 = closed_loop(plain, 60)
    r1, f1, m1 = closed_loop(b, 60)
    assert m0 == m1 and m0["ctl_steps"] > 0
    for x, y in zip(r0, r1):
        assert same_bits(x, y)
    for k in f0:
        assert np.array_equal(f0[k], f1[k]), k


def test_pipelined_offsets_are_the_sub_batch_bounds():
    from pve_mcc_amd import PipelinedIntersections
    from pve_mcc_amd.arrivals import synthetic_arrivals
    from pve_mcc_amd.distributed import set_shard_exploration, shard_range
    arr = synthetic_arrivals(5, rate=500.0, horizon_s=20.0, seed=5)
    p = PipelinedIntersections(5, 64, arr, n_sub=2, device="cpu", _lib=emulator_lib())
    p.set_exploration(0.0, seed=9)
    assert [s.exploration for s in p.subs] == [(0.0, 9, 0), (0.0, 9, 3)] and p.bounds == [0, 3, 5]
    set_shard_exploration(p.subs[1], 0.0, 4, 10, 1, 2)
    assert p.subs[1].exploration == (0.0, 4, shard_range(10, 1, 2)[0]) == (0.0, 4, 5)

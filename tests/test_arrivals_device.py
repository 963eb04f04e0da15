"""The device arrival generator on the CPU (csrc/pve_arrivals.h, pve_generate_arrivals): a g++ build of the header against the
NumPy restatement (pve_mcc_amd.arrivals.device_arrivals / device_intentions) bit for bit, the logarithm against libm, the purity
properties the header states, the shape of the distribution, the stream as an environment input (through the CPU emulator
against the sequential oracles) and the C ABI's argument checks through the emulator, which has no such kernels and says so.
The kernels are held to the model in tests/test_gpu_arrivals.py."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle.oracle import OracleEnv
from oracle.record import close
from pve_mcc_amd import _capi, arrivals as AR
from pve_mcc_amd.batched import BatchedIntersections
from tests import native, scenarios
from tests.hip_adapter import emulator_lib, make_batch, state_snapshot

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _declare(lib):
    vp = C.c_void_p
    lib.arrivals_generate_host.restype = None
    lib.arrivals_generate_host.argtypes = [C.c_uint64, C.c_longlong, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_double, vp, C.c_double,
                                           vp, vp, vp]
    lib.arrival_exp_host.restype = None
    lib.arrival_exp_host.argtypes = [vp, C.c_longlong, vp]
    return lib


def host():
    return native.load("arrivals_host", "libarrivals_host.so", _declare)


def host_generate(n_envs, rows, lane_num, rate, seed=0, epoch=0, env_offset=0, min_gap=1.0, intentions=True):
    """(arrivals, intentions, covered) of the g++ build of the header; 0xFF-filled buffers with a guard row behind each"""
    mean = AR.device_mean(rate, n_envs)
    per_env = np.ndim(rate) > 0
    arr = np.full(n_envs * rows * lane_num + 16, np.nan)
    arr.view(np.uint8)[:] = 0xFF
    ch = np.full(n_envs * rows * lane_num + 16, -1, np.int32)
    cov = np.full(n_envs + 4, np.nan)
    cov.view(np.uint8)[:] = 0xFF
    host().arrivals_generate_host(int(seed) & 0xFFFFFFFFFFFFFFFF, env_offset, epoch & 0xFFFFFFFF, rows, n_envs, lane_num,
                                  float(mean[0]), mean.ctypes.data if per_env else None, min_gap, arr.ctypes.data,
                                  ch.ctypes.data if intentions else None, cov.ctypes.data)
    assert np.all(arr.view(np.uint8)[-128:] == 0xFF) and np.all(ch[-16:] == -1) and np.all(cov.view(np.uint8)[-32:] == 0xFF), "guard"
    n = n_envs * rows * lane_num
    return arr[:n].reshape(n_envs, rows, lane_num), ch[:n].reshape(n_envs, rows, lane_num), cov[:n_envs]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------ 1. the g++ build of the header against the NumPy model
@pytest.mark.parametrize("lane_num", [4, 8, 12])
def test_host_build_equals_the_numpy_model_bit_for_bit(lane_num):
    n = 0
    # (five variants against 18 shapes x 2 kinds of mean: every variant meets both kinds and every row count)
    variants = itertools.cycle([dict(min_gap=1.0), dict(min_gap=0.0, env_offset=3, epoch=1),
                                dict(min_gap=0.0, env_offset=(1 << 32) - 2, epoch=(1 << 32) - 1, seed=0xFEDCBA9876543210),
                                dict(min_gap=1.0, rate=3600.0 / 1e-3, epoch=1),
                                dict(min_gap=0.5, rate=3600.0 / 1e6, seed=77, env_offset=(1 << 32) - 2)])
    for n_envs, rows in itertools.product((1, 5, 17), (2, 3, 5, 6, 33, 130)):
        for per_env in (False, True):
            kw = dict(next(variants))
            rate = kw.pop("rate", None)
            if per_env:
                rate = np.linspace(200.0, 1200.0, n_envs) if rate is None else np.full(n_envs, rate)
            elif rate is None:
                rate = 1100.0
            got_a, got_c, got_cov = host_generate(n_envs, rows, lane_num, rate, **kw)
            kw_i = {k: v for k, v in kw.items() if k != "min_gap"}
            want_a = AR.device_arrivals(n_envs, rows, lane_num, rate, **kw)
            want_c = AR.device_intentions(n_envs, rows, lane_num=lane_num, **kw_i)
            assert np.array_equal(bits(got_a), bits(want_a)), (n_envs, rows, lane_num, kw)
            assert np.array_equal(got_c, want_c), (n_envs, rows, lane_num, kw)
            assert np.array_equal(bits(got_cov), bits(AR.device_covered(want_a)))
            assert np.all(np.isposinf(got_a[:, -1, :])) and np.all(np.isfinite(got_a[:, :-1, :]))
            n += 1
    assert n == 36


def test_every_gap_clipped_and_no_gap_clipped():
    a = AR.device_arrivals(3, 40, 12, 3600.0 / 1e-3, seed=5)                 # mean 1 ms: every gap is min_gap
    assert np.array_equal(a[:, :-1, :], np.broadcast_to(np.arange(1.0, 40.0)[None, :, None], (3, 39, 12)))
    b = AR.device_arrivals(3, 40, 12, 3600.0 / 1e6, seed=5)                  # mean 1e6 s: hardly any is
    m = AR.device_mean(3600.0 / 1e6, 3)[0]
    x = AR.exp_from_words(AR.arrival_words(3, 40, 12, seed=5))
    assert np.array_equal(bits(b[:, 0, :]), bits(np.maximum(1.0, m * x[:, 0, :]))) and (m * x > 1.0).mean() > 0.99


def test_cumsum_is_the_sequential_chain():
    """np.cumsum along the rows adds in ascending r, one chain per (env, lane): the header's order."""
    d = np.random.default_rng(3).exponential(3.27, size=(5, 431, 12))
    d = np.maximum(1.0, d)
    want = np.empty_like(d)
    t = np.zeros((5, 12))
    for r in range(d.shape[1]):
        t = d[:, r, :] if r == 0 else t + d[:, r, :]
        want[:, r, :] = t
    assert np.array_equal(bits(np.cumsum(d, axis=1)), bits(want))
    rate = np.linspace(200.0, 1200.0, 5)
    a = AR.device_arrivals(5, 130, 12, rate, seed=9, min_gap=0.25)
    g = AR.device_mean(rate, 5)[:, None, None] * AR.exp_from_words(AR.arrival_words(5, 130, 12, seed=9))
    g = np.where(g < 0.25, 0.25, g)
    t = g[:, 0, :]
    for r in range(129):
        t = g[:, r, :] if r == 0 else t + g[:, r, :]
        assert np.array_equal(bits(a[:, r, :]), bits(t)), r


# ------------------------------------------------------------------ 2. the logarithm
def test_logarithm_against_libm():
    """x = -ln((2 w + 1) 2^-33) in the header's arithmetic against -np.log(u) in float64: bar 1e-12 relative.
    Measured maximum over these 2^20 + 30 words: 1.13e-15 (g++ build and NumPy model, which agree to the bit)."""
    rng = np.random.default_rng(2024)
    edge = [0, 0xFFFFFFFF, 1, 0xFFFFFFFE, 0x7FFFFFFF, 0x80000000]
    for e in (33, 32, 31, 24, 12, 5):                      # the words either side of the sqrt(1/2) fold of binade [2^(e-1), 2^e)
        m0 = int(math.floor(0.70710678118654757 * 2.0 ** e))
        edge += [m0 // 2 - 1, m0 // 2, m0 // 2 + 1, m0 // 2 + 2]
    w = np.concatenate([rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64), np.array(edge, np.uint64)]).astype(np.uint32)
    x_np = AR.exp_from_words(w)
    x_host = np.empty(len(w))
    host().arrival_exp_host(w.ctypes.data, len(w), x_host.ctypes.data)
    assert np.array_equal(bits(x_np), bits(x_host))
    u = (2.0 * w.astype(np.float64) + 1.0) * 2.0 ** -33                      # exact
    ref = -np.log(u)
    rel = np.abs(x_np - ref) / ref
    print("arrival_exp vs -log(u): max relative deviation %.3e over %d words" % (rel.max(), len(w)))
    assert rel.max() <= 1e-12
    assert x_np.min() > 0 and abs(x_np.min() - 1.16e-10) < 1e-12 and x_np.max() < 22.8745 and x_np.max() > 22.873
    assert AR.exp_from_words(np.uint64(0xFFFFFFFF)) == x_np.min() and AR.exp_from_words(np.uint64(0)) == x_np.max()


# ------------------------------------------------------------------ 3. purity
def test_streams_are_pure_functions_of_their_coordinates():
    kw = dict(seed=41, epoch=2, min_gap=1.0)
    rate = np.linspace(300.0, 1200.0, 8)
    full = AR.device_arrivals(8, 70, 12, rate, **kw)
    piece = AR.device_arrivals(2, 70, 12, rate[3:5], env_offset=3, **kw)
    assert np.array_equal(bits(full[3:5]), bits(piece))
    short = AR.device_arrivals(8, 33, 12, rate, **kw)
    assert np.array_equal(bits(short[:, :32]), bits(full[:, :32])) and np.all(np.isposinf(short[:, 32]))
    ch = AR.device_intentions(8, 300, seed=41, epoch=2)
    assert np.array_equal(ch[3:5], AR.device_intentions(2, 300, seed=41, epoch=2, env_offset=3))
    assert np.array_equal(ch[:, :131], AR.device_intentions(8, 131, seed=41, epoch=2))
    got_a, got_c, _ = host_generate(2, 70, 8, rate[3:5], env_offset=3, **kw)
    assert np.array_equal(bits(got_a), bits(AR.device_arrivals(8, 70, 8, rate, **kw)[3:5])) and np.array_equal(got_c, ch[3:5, :70])
    # another seed / epoch / lane / env: another chain
    base = AR.device_arrivals(4, 40, 12, 1100.0, seed=1, epoch=0, min_gap=0.0)
    for other in (AR.device_arrivals(4, 40, 12, 1100.0, seed=2, epoch=0, min_gap=0.0),
                  AR.device_arrivals(4, 40, 12, 1100.0, seed=1 + (1 << 32), epoch=0, min_gap=0.0),
                  AR.device_arrivals(4, 40, 12, 1100.0, seed=1, epoch=1, min_gap=0.0),
                  AR.device_arrivals(4, 40, 12, 1100.0, seed=1, epoch=0, min_gap=0.0, env_offset=1 << 32)):
        assert not np.any(other[:, :-1] == base[:, :-1])
    chains = base[:, :-1].transpose(0, 2, 1).reshape(48, 39)
    assert len({c.tobytes() for c in chains}) == 48 and len(set(chains[:, 0].tolist())) == 48
    # arrivals and intentions of one seed draw from different keys: the words differ, and the bits do not follow the gaps
    w = AR.arrival_words(4, 129, 8, seed=1)
    c = AR.device_intentions(4, 128, seed=1)
    assert AR.ARR_KEY != AR.INT_KEY and abs(np.corrcoef((w & np.uint64(1)).ravel().astype(np.float64), c.ravel())[0, 1]) < 0.05
    assert abs(np.corrcoef((w >> np.uint64(31)).ravel().astype(np.float64), c.ravel())[0, 1]) < 0.05


# ------------------------------------------------------------------ 4. the shape of the distribution
def test_distribution_of_gaps_and_intentions():
    E, R, LN, mean = 64, 432, 12, 3600.0 / 1100.0
    x = AR.exp_from_words(AR.arrival_words(E, R, LN, seed=12345))
    N = x.size
    assert N == 64 * 431 * 12
    z_mean = (x.mean() - 1.0) * math.sqrt(N)
    p = 1.0 - math.exp(-1.0 / mean)
    clipped = (mean * x < 1.0).mean()
    z_clip = (clipped - p) / math.sqrt(p * (1 - p) / N)
    ch = AR.device_intentions(E, R, seed=12345)
    z_int = (ch.mean() - 0.5) / math.sqrt(0.25 / ch.size)
    print("gaps: mean(x) z = %.2f, clipped share %.4f (expected %.4f) z = %.2f; intentions: ones z = %.2f" % (z_mean, clipped, p, z_clip, z_int))
    assert abs(p - 0.2633) < 5e-5
    assert abs(z_mean) <= 4.0 and abs(z_clip) <= 4.0 and abs(z_int) <= 4.0
    a = AR.device_arrivals(E, R, LN, 1100.0, seed=12345)
    assert abs((np.diff(a[:, :-1], axis=1) == 1.0).mean() - clipped) < 2e-3            # (the clip as the stream shows it)


# ------------------------------------------------------------------ 5. validity as an environment input
@pytest.mark.parametrize("lane_num,rate", [(12, 1100.0), (8, np.array([200.0, 700.0, 1200.0])), (4, 2200.0)])
def test_stream_is_a_valid_environment_input(lane_num, rate):
    a = AR.device_arrivals(3, 200, lane_num, rate, seed=8, epoch=4)
    got, _, cov = host_generate(3, 200, lane_num, rate, seed=8, epoch=4)
    assert np.array_equal(bits(a), bits(got))
    assert np.all(np.diff(a[:, :-1], axis=1) > 0) and np.all(a[:, 0] > 0)
    assert np.all(a[:, :-1] >= np.arange(1.0, 200.0)[None, :, None]) and np.all(np.isposinf(a[:, -1]))
    assert np.array_equal(cov, a[:, -2].min(axis=1)) and np.all(cov >= 199.0)
    a0 = AR.device_arrivals(3, 200, lane_num, rate, seed=8, epoch=4, min_gap=0.0)
    assert np.all(np.diff(a0[:, :-1], axis=1) > 0) and np.all(a0[:, 0] > 0)           # (x is never 0)
    assert AR.default_rows(1100.0, 600.0) == 432 and AR.default_rows([200.0, 1100.0], 600.0) == 432


# ------------------------------------------------------------------ 6. the generated stream through the emulator against the oracle
def test_generated_stream_12_lanes_through_the_emulator_against_the_oracle():
    arr = AR.device_arrivals(2, AR.default_rows(1100.0, 50.0), 12, 1100.0, seed=31)
    scenarios.check_fuzz_vs_oracle("emu", 2, 128, 200, 1100.0, 31, arrivals=arr)


def test_generated_stream_8_lanes_with_intentions_through_the_emulator_against_the_oracle():
    """As scenarios.check_geo_fuzz_vs_oracle, with the generated intention stream in the place of synthetic_intentions."""
    from oracle.oracle_geo import OracleGeoEnv
    n_envs, cap, ticks = 2, 128, 200
    rows = AR.default_rows(1500.0, 50.0)
    arr, ch = AR.device_arrivals(n_envs, rows, 8, 1500.0, seed=32), AR.device_intentions(n_envs, rows, seed=32)
    assert 0.3 < ch.mean() < 0.7
    b = make_batch(arr, n_envs, cap, "emu", lane_num=8, intentions=ch,
                   outputs=("obs_post", "obs_pre", "reward", "flags", "nbr", "env_out", "new_slot", "lanej"))
    b.reset()
    oracles = [OracleGeoEnv(arr[e], 8, choice=ch[e]) for e in range(n_envs)]
    rng = np.random.default_rng(32)
    n_ctl = 0
    for t in range(ticks):
        acts = rng.uniform(-3, 3, size=(n_envs, cap)).astype(np.float32).astype(np.float64)
        out = b.step(torch.as_tensor(acts))
        rew, flags, eo = out["reward"].numpy(), out["flags"].numpy().astype(np.int64), out["env_out"].numpy()
        nbr, obs, lanej = out["nbr"].numpy(), out["obs_pre"].numpy(), out["lanej"].numpy().astype(np.int64)
        for e, o in enumerate(oracles):
            n = o.n_alive
            _vid, ctlm, _ = o.alive_view()
            rec = o.tick(np.where(ctlm != 0, acts[e, :n], 0.0))
            f = flags[e, :n]
            order = np.lexsort((lanej[e, :n] & 0xFFFF, (f >> 6) & 3, lanej[e, :n] >> 16))
            ctl = order[((f & 2) != 0)[order]]
            n_ctl += len(ctl)
            assert int(eo[e, 0]) == n and len(ctl) == len(rec["ids"]), "controlled set: tick %d env %d" % (t, e)
            assert np.array_equal(np.stack([lanej[e, ctl] >> 16, lanej[e, ctl] & 0xFFFF], -1), rec["ids"]), "ids: tick %d env %d" % (t, e)
            assert int(eo[e, 2]) == rec["collisions"] and int(eo[e, 3]) == rec["lock"], "counters: tick %d env %d" % (t, e)
            assert close(rec["reward"], rew[e, ctl], 1e-9), "reward: tick %d env %d" % (t, e)
            assert close(rec["obs0"], obs[e, ctl], 1e-9), "obs: tick %d env %d" % (t, e)
    assert n_ctl > 500
    for e, o in enumerate(oracles):
        _info, vi, vf = state_snapshot(b, e)
        ovi, ovf, _, ointent = o.vehicles()
        assert np.array_equal(vi[:, :13], ovi[:, :13]) and close(ovf[:, :5], vf[:, :5], 1e-9), "final state, env %d" % e
        got = np.array([[v.intention, v.route] for v in b.read_vehicles(e)], np.int32).reshape(-1, 2)
        assert np.array_equal(got, ointent), "intentions / routes, env %d" % e
    assert b.metrics()["overflow"] == 0


# ------------------------------------------------------------------ 7. the C ABI on a backend without the kernels
def test_entry_point_on_the_emulator():
    lib = emulator_lib()
    assert _capi.EXPORTS_EXT == ("pve_generate_arrivals",) and hasattr(lib, "pve_generate_arrivals")
    assert lib.pve_abi_version() == _capi.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "pve_env.h")).read()
    for text in ("0x41525256", "0x54494D45", "0x494E5445", "0x4E54494F", "main.py:228-229", ":388-389",
                 "ref :381, :390", "} pve_arrival_gen;", "include/pve_env_arrivals.h"):
        assert text in header, text
    # the extension header's prototype, and the product library exports it (that the header declares exactly EXPORTS_EXT, the
    # version, the signature's classes and the struct's layout: tests/test_binding_contract.py)
    ext = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pve_env_arrivals.h")).read(), flags=re.S)
    assert "int pve_generate_arrivals(pve_handle h, const pve_arrival_gen *g, double *arrivals" in ext
    assert all(hasattr(_capi.load_library(), n) for n in _capi.EXPORTS_EXT) and not set(_capi.EXPORTS) & set(_capi.EXPORTS_EXT)
    b12 = make_batch(np.full((4, 12), np.inf), 3, 64, "emu", outputs=("obs_post", "flags"))
    b8 = make_batch(np.full((4, 8), np.inf), 3, 64, "emu", outputs=("obs_post", "flags"), lane_num=8)
    keep = []

    def P(n, dt, off=0):
        raw = np.zeros(n * np.dtype(dt).itemsize + 32, np.uint8)
        keep.append(raw)
        return raw.ctypes.data + (-raw.ctypes.data) % 16 + off

    rows = 20
    arr, ch, cov, mean_env = P(3 * rows * 12, np.float64), P(3 * rows * 8, np.int32), P(3, np.float64), P(3, np.float64)

    def gen(h=b12._h, g=True, arrivals=arr, intentions=None, covered=cov, **kw):
        d = dict(seed=1, env_offset=0, epoch=0, rows=rows, mean_s=3.0, mean_env=None, min_gap_s=1.0, block_threads=0)
        d.update(kw)
        return lib.pve_generate_arrivals(h, C.byref(_capi.PveArrivalGen(**d)) if g else None, arrivals, intentions, covered)

    bad = [(dict(h=None), b"null"), (dict(g=False), b"null"), (dict(arrivals=None), b"null"), (dict(env_offset=-1), b"env_offset"),
           (dict(rows=1), b"rows"), (dict(rows=0), b"rows"), (dict(rows=-5), b"rows"), (dict(rows=(1 << 28) + 1), b"rows"),
           (dict(mean_s=0.0), b"mean_s"), (dict(mean_s=-1.0), b"mean_s"), (dict(mean_s=float("inf")), b"mean_s"),
           (dict(mean_s=float("nan")), b"mean_s"), (dict(min_gap_s=-0.5), b"min_gap_s"), (dict(min_gap_s=float("inf")), b"min_gap_s"),
           (dict(min_gap_s=float("nan")), b"min_gap_s"), (dict(block_threads=100), b"block_threads"), (dict(block_threads=2048), b"block_threads"),
           (dict(block_threads=-64), b"block_threads"), (dict(intentions=ch), b"lane_num = 8"), (dict(arrivals=arr + 8), b"aligned"),
           (dict(covered=cov + 4), b"aligned"), (dict(mean_env=mean_env + 4), b"aligned"),
           (dict(h=b8._h, intentions=ch + 8), b"aligned"), (dict(h=b8._h, intentions=ch + 4), b"aligned")]
    for kw, word in bad:
        assert gen(**kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    # valid arguments: the emulator has no such kernels and says so
    for kw in (dict(), dict(covered=None), dict(mean_env=mean_env, mean_s=0.0), dict(min_gap_s=0.0), dict(rows=2), dict(block_threads=1024),
               dict(h=b8._h, intentions=ch), dict(env_offset=(1 << 62), epoch=0xFFFFFFFF, seed=0xFFFFFFFFFFFFFFFF)):
        assert gen(**kw) == -1 and b"backend has no arrival generator kernels" in lib.pve_last_error(), (kw, lib.pve_last_error())
    # the Python method asks the backend and passes its refusal on; the batch keeps the stream it had
    before = b12.arrivals
    with pytest.raises(_capi.PveError, match="no arrival generator kernels"):
        b12.generate_arrivals(1100.0, horizon_s=30.0)
    with pytest.raises(_capi.PveError, match="rows or horizon_s"):
        b12.generate_arrivals(1100.0)
    assert b12.arrivals is before
    # a batch built without a stream cannot be reset before it has one
    nb = BatchedIntersections(2, 64, None, device="cpu", outputs=("obs_post",), _lib=lib)
    with pytest.raises(_capi.PveError):
        nb.reset()

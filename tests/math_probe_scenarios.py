"""The tick's hand-written arithmetic helpers, one at a time (tests/math_probe/pve_math_probe.hip), against plain references:
mpmath at 40 digits for values, NumPy float64 / Python integers for everything that must be exact.  Every check takes the
backend (`Probe("host")`: the g++ build, i.e. the branches the CPU emulator compiles; `Probe("hip")`: the hipcc build with the
product's flags on the device) and is called by tests/test_math_probe.py and tests/test_gpu_math_probe.py.

Every sample set is random points from a fixed seed plus the named edge points; <= 50 000 points where mpmath is the
reference, <= 1 000 000 where NumPy is.  Value checks print `MATH_PROBE <backend> <what> <figure>` before they assert
(profiles/math_probe.txt keeps those lines)."""
import ctypes as C
import functools
import math
import os

import mpmath
import numpy as np

from pve_mcc_amd._capi import PveConfig
from tests import native

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PROBE_DIR = os.path.join(ROOT, "tests", "math_probe")
CSRC_DIR = os.path.join(ROOT, "pve-mcc_for_unsignalized_intersection_amd", "csrc")
LIB = {"host": "libpve_math_probe_host.so", "hip": "libpve_math_probe_hip.so"}
E_ARGS, E_LANE, E_DEVICE_ONLY = -1, -2, -3
mpmath.mp.dps = 40

DEFAULT_CFG = dict(deltaT=0.1, vm=5.0, vM=13.0, am=-3.0, aM=3.0, v0=10.0, lane_cw=2.5, dis_ctl=150.0, collision_thr=2.0, lane_num=12, flags=0)
# the constructor arguments of the *_kw fixtures (tests/test_ctor_kwargs.py asserts the generator used these) and of *_vm6
ALL_KW = {"dis_ctl": 120, "lane_cw": 3, "collision_thr": 3, "vM": 15, "v0": 9, "am": -2.5, "aM": 2.5, "deltaT": 0.2, "vm": 6}
VM6 = {"vm": 6}
ACCEL_ASYM = {"am": -3.7, "aM": 1.3}                       # tests/test_ctor_kwargs.py VARIANTS: |am| != aM
LIMIT_CFGS = [("default", {}), ("kw", ALL_KW), ("vm6", VM6), ("accel_asym", ACCEL_ASYM)]
# geometry: the default, the moved-argument fixtures' lane_cw / dis_ctl, and a wider intersection than any fixture (float32
# error grows with both arguments)
GEOMETRIES = [("default", {}), ("kw", {"lane_cw": 3, "dis_ctl": 120}), ("wide", {"lane_cw": 3.5, "dis_ctl": 260})]


class ProbeArgs(C.Structure):
    _fields_ = [("n", C.c_longlong), ("inp", C.c_void_p * 6), ("out", C.c_void_p * 3), ("k", C.c_int * 4)]


def build(kind, always_make=True):
    """`make` the flavour through tests/native.py (a no-op when it is up to date) -> its path.  always_make=False once meant
    "only if the object is missing or older than its sources"; that is `make`'s own question, so both values ask `make` now
    and the argument only keeps the callers' spelling.  A failure to build is an error, never a skip."""
    return native.build("math_probe", LIB[kind])


def make_cfg(**kw):
    d = dict(DEFAULT_CFG)
    d.update(kw)
    return PveConfig(**{k: (int(v) if k in ("lane_num", "flags") else float(v)) for k, v in d.items()})


class Probe:
    """One flavour of the probe library.  call() takes and returns NumPy arrays; the device flavour moves them through torch
    tensors (byte tensors: every element type, uint64 included, travels as is) and hands their data_ptr() to the entry point."""

    def __init__(self, kind, always_make=True):
        self.kind = kind
        self.lib = native.load("math_probe", LIB[kind])             # (always_make: see build)
        assert self.lib.pve_probe_is_device() == (1 if kind == "hip" else 0)

    def raw(self, name, ins, outs, cfg=None, k=(), n=None):
        """-> (return code, outputs).  ins: arrays; outs: [(dtype, elements)]"""
        fn = getattr(self.lib, "pve_probe_" + name)
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(PveConfig), C.POINTER(ProbeArgs)]
        a = ProbeArgs()
        ins = [np.ascontiguousarray(x) for x in ins]
        a.n = len(ins[0]) if n is None else n
        for q, v in enumerate(k):
            a.k[q] = int(v)
        keep = []
        if self.kind == "hip":
            import torch
            for q, x in enumerate(ins):
                t = torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).cuda()
                keep.append(t)
                a.inp[q] = t.data_ptr()
            res = [torch.zeros(max(1, cnt * np.dtype(dt).itemsize), dtype=torch.uint8, device="cuda") for dt, cnt in outs]
            for q, t in enumerate(res):
                a.out[q] = t.data_ptr()
            torch.cuda.synchronize()
            rc = fn(C.byref(cfg if cfg is not None else make_cfg()), C.byref(a))
            got = [t.cpu().numpy()[:cnt * np.dtype(dt).itemsize].view(dt) for t, (dt, cnt) in zip(res, outs)]
        else:
            for q, x in enumerate(ins):
                keep.append(x)
                a.inp[q] = x.ctypes.data
            got = [np.zeros(max(1, cnt), dt) for dt, cnt in outs]
            for q, x in enumerate(got):
                a.out[q] = x.ctypes.data
            rc = fn(C.byref(cfg if cfg is not None else make_cfg()), C.byref(a))
            got = [x[:cnt] for x, (dt, cnt) in zip(got, outs)]
        return rc, got

    def call(self, name, ins, out_dtypes, cfg=None, k=(), n=None):
        n_el = len(ins[0]) if n is None else n
        rc, got = self.raw(name, ins, [(dt, n_el) for dt in out_dtypes], cfg, k, n)
        assert rc == 0, (name, self.kind, rc)
        return got[0] if len(got) == 1 else got


def f64(x):
    return np.ascontiguousarray(x, np.float64)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({8: np.uint64, 4: np.uint32}[x.dtype.itemsize])


def neighbours(x):
    x = f64(np.atleast_1d(x))
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def ordinal(x):
    """float64 -> int64 that counts representable numbers (the distance of two values in ulps is the difference)"""
    b = f64(x).view(np.int64)
    return np.where(b < 0, np.int64(-2 ** 63) - b, b)


def report(P, what, figure, note=""):
    print("MATH_PROBE %-4s %-44s %.3e %s" % (P.kind, what, figure, note))


def mp_map(fn, xs):
    return [fn(mpmath.mpf(float(x))) for x in xs]


def abs_err(got, ref_mp):
    return max(abs(mpmath.mpf(float(g)) - r) for g, r in zip(got, ref_mp))


# ====================================================================================== sample sets (shared by the checks
# and by the device-vs-host bit comparison) and their mpmath references, computed once per process
@functools.lru_cache(None)
def exp_points():
    r = np.random.default_rng(101)
    log2e = 1.4426950408889634074
    brk = np.concatenate([neighbours(np.nextafter(-h / log2e, s)) for h in (0.5, 1.5, 2.5) for s in (-np.inf, np.inf)])
    x = np.concatenate([r.uniform(-2, 0, 40000), [0.0, -0.0, -2.0, np.nextafter(-2.0, 0), -5e-324, -1e-300, -1e-17], brk])
    return x[(x >= -2) & (x <= 0)]


@functools.lru_cache(None)
def exp_ref():
    return mp_map(mpmath.exp, exp_points())


@functools.lru_cache(None)
def coth_points():
    r = np.random.default_rng(102)
    hi = np.concatenate([r.uniform(1 / 16, 4, 30000), 1 / 16 * np.exp(r.uniform(0, math.log(64), 10000)),
                         [1 / 16, np.nextafter(1 / 16, 1), np.nextafter(4.0, 0), 1.0, 2.0, 3.999]])
    hi = hi[(hi >= 1 / 16) & (hi < 4)]
    lo = np.concatenate([np.exp(r.uniform(math.log(1e-17), math.log(1 / 16), 9000)),
                         [1e-17, 5e-17, 1e-16, 1.1e-16, 2.2e-16, 2.3e-16, 4.4e-16, 1e-15, 1e-9, 1e-3, np.nextafter(1 / 16, 0)]])
    lo = lo[(lo > 0) & (lo < 1 / 16)]
    return hi, lo


@functools.lru_cache(None)
def coth_ref():
    return mp_map(lambda t: mpmath.coth(-t / 4), coth_points()[0])


@functools.lru_cache(None)
def log_points():
    r = np.random.default_rng(103)
    fold = 0.70710678118654752
    edges = [1e-5, 1.00001, np.nextafter(1.00001, 0), np.nextafter(1e-5, 1)]
    edges += list(neighbours(1.0)) + [math.ldexp(v, -k) for k in range(0, 17) for v in neighbours(fold)]
    edges += [v for k in range(0, 17) for v in neighbours(math.ldexp(1.0, -k))]
    z = np.concatenate([r.uniform(1e-5, 1.00001, 20000), np.exp(r.uniform(math.log(1e-5), math.log(1.00001), 20000)), edges])
    return z[(z >= 1e-5) & (z <= 1.00001)]


@functools.lru_cache(None)
def log_ref():
    return mp_map(mpmath.log, log_points())


@functools.lru_cache(None)
def log_series_points():
    r = np.random.default_rng(120)
    fold = 0.70710678118654752
    z = np.concatenate([r.uniform(fold, 1, 20000), r.uniform(fold, 0.76, 10000), neighbours(fold), [np.nextafter(1.0, 0), 0.75, 0.999]])
    return z[(z >= fold) & (z < 1)]


@functools.lru_cache(None)
def log_series_ref():
    return mp_map(mpmath.log, log_series_points())


@functools.lru_cache(None)
def sincos_points():
    r = np.random.default_rng(104)
    return np.concatenate([r.uniform(0, math.pi / 2, 40000), [0.0, 5e-324, 1e-300, 1e-9, math.pi / 2, 3.141593 / 2, 3.1415 / 2],
                           neighbours(math.pi / 4), neighbours(0.7853981633974483)])


@functools.lru_cache(None)
def sincos_ref():
    x = sincos_points()
    return mp_map(mpmath.sin, x), mp_map(mpmath.cos, x)


def value_div_points():
    r = np.random.default_rng(105)
    n = 60000
    y = np.concatenate([r.uniform(-0.865, -1e-16, n), -np.exp(r.uniform(math.log(1e-16), math.log(0.865), n)), r.uniform(1.707, 2.414, n),
                        np.ldexp(r.uniform(0.5, 1, 2 * n), r.integers(-63, 65, 2 * n)) * r.choice([-1.0, 1.0], 2 * n),
                        [-0.865, -1e-16, 1.707, 2.414, 2.0 ** -64, 2.0 ** 64, -2.0 ** -64, -2.0 ** 64, 1.0, -1.0, 3.0, -3.0]])
    # the numerators the reward forms: u + 1 in (1.13, 2], f = m - 1 in [-0.293, 0.415); and anything
    x = np.concatenate([r.uniform(1.13, 2, len(y) // 3), r.uniform(-0.293, 0.415, len(y) // 3),
                        np.ldexp(r.uniform(0.5, 1, len(y) - 2 * (len(y) // 3)), r.integers(-40, 40, len(y) - 2 * (len(y) // 3)))])
    return x, y


def div_const_points(b):
    """x for the exact division by the constant b: random over 128 binades, the operand range of brake_needed, and the doubles
    around the rounding midpoints of 100 000 random quotients"""
    r = np.random.default_rng(106)
    n = 250000
    wide = np.ldexp(r.uniform(0.5, 1, n), r.integers(-64, 64, n)) * r.choice([-1.0, 1.0], n)
    v, fv = r.uniform(0, 15, n), r.uniform(0, 15, n)
    fv[: n // 8] = v[: n // 8]
    brake = np.concatenate([v * v - fv * fv, (v - fv) * 5.0, (v - fv) * 6.0])
    q = np.ldexp(r.uniform(0.5, 1, 100000), r.integers(-30, 30, 100000)) * r.choice([-1.0, 1.0], 100000)
    mid = (q.astype(np.longdouble) + np.spacing(q).astype(np.longdouble) / 2) * np.longdouble(b)
    return np.concatenate([wide, brake, neighbours(mid.astype(np.float64)), [0.0, b, -b, 2 * b, 3 * b]])


def brake_points(cfg_kw):
    """(p, v, fp, fv) and the NumPy restatement of the brake test with true divisions (ref :1509-1516)"""
    d = dict(DEFAULT_CFG)
    d.update(cfg_kw)
    r = np.random.default_rng(107)
    n = 200000
    vM, vm, abs_am = float(d["vM"]), float(d["vm"]), abs(float(d["am"]))
    v, fv = r.uniform(0, vM, n), r.uniform(0, vM, n)
    v[:1000], fv[:1000] = vM, r.uniform(0, vM, 1000)
    fv[1000:2000] = v[1000:2000]
    fv[2000:3000] = np.nextafter(v[2000:3000], 0)

    def d_safe(v, fv):
        return v * 0.4 + (v * v - fv * fv) / (2 * abs_am) - (v - fv) * vm / abs_am

    ds = d_safe(v, fv)
    # fp = 0, so that p - fp IS p: d_safe itself and its two neighbours; then random gaps around d_safe
    fp = np.zeros(3 * n)
    p = np.concatenate([np.nextafter(ds, -np.inf), ds, np.nextafter(ds, np.inf)])
    v3, fv3 = np.tile(v, 3), np.tile(fv, 3)
    fp2 = r.uniform(0, 150, n)
    p2 = fp2 + ds * r.uniform(0.5, 1.5, n)
    p, v3, fp, fv3 = np.concatenate([p, p2]), np.concatenate([v3, v]), np.concatenate([fp, fp2]), np.concatenate([fv3, fv])
    want = ((fv3 < v3) & (p - fp < d_safe(v3, fv3))).astype(np.int32)
    return p, v3, fp, fv3, want


def key_less_points():
    r = np.random.default_rng(108)
    n = 200000
    dv = np.array([0.0, 1.0, 1.5, np.nextafter(1.5, 2), 2.0, 1e-300, 100.0])
    return (r.choice(dv, n), r.choice(dv, n), r.integers(0, 4, n).astype(np.int32),
            r.choice(dv, n), r.choice(dv, n), r.integers(0, 4, n).astype(np.int32))


def mul24_points():
    """counts, ranks, slots and slot-derived indices: operands and results < 2^22 (csrc/pve_tick_core.h: env_at, mul24)"""
    r = np.random.default_rng(109)
    n = 200000
    a = r.integers(0, 1 << 11, n)
    b = r.integers(0, 1 << 11, n)
    a2 = r.integers(0, 1 << 22, n)                    # one large factor, the product still < 2^22
    b2 = ((1 << 22) - 1) // np.maximum(a2, 1)
    b2 = (b2 * r.uniform(0, 1, n)).astype(np.int64)
    a = np.concatenate([a, a2, b2, [0, 1, (1 << 22) - 1, 2047, 2048, 256, 255]])
    b = np.concatenate([b, b2, a2, [0, (1 << 22) - 1, 1, 2047, 2047, 16383, 16448]])
    c = r.integers(0, 1 << 22, len(a))
    assert np.all(a * b < (1 << 22)) and np.all(a < (1 << 22)) and np.all(b < (1 << 22))
    return a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)


def mask_set(NW):
    """Python integers of 64 NW bits: empty, full, single bits at word edges, alternating, 1000 random"""
    r = np.random.default_rng(110 + NW)
    nb = 64 * NW
    full = (1 << nb) - 1
    ms = [0, full, full // 3, full - full // 3]
    for w in range(NW):
        ms += [1 << (64 * w), 1 << (64 * w + 63), 1 << (64 * w + 1), 1 << (64 * w + 62), 1 << (64 * w + 31), 1 << (64 * w + 32)]
        ms += [((1 << 64) - 1) << (64 * w)]
    for k in range(1000):
        m = int.from_bytes(r.bytes(nb // 8), "little")
        if k % 3 == 1:
            m &= int.from_bytes(r.bytes(nb // 8), "little")     # sparse
        ms.append(m)
    return ms


def mask_words(ms, NW):
    return np.array([[(m >> (64 * w)) & ((1 << 64) - 1) for w in range(NW)] for m in ms], np.uint64).reshape(-1)


@functools.lru_cache(None)
def mask_reference(NW):
    """(masks, below[mask][t], prev[mask][t]) for t in [0, 64 NW], by Python integer bit operations"""
    ms = mask_set(NW)
    nb = 64 * NW
    below = np.zeros((len(ms), nb + 1), np.int32)
    prev = np.zeros((len(ms), nb + 1), np.int32)
    for q, m in enumerate(ms):
        for t in range(nb + 1):
            lowbits = m & ((1 << t) - 1)
            below[q, t] = bin(lowbits).count("1")
            prev[q, t] = lowbits.bit_length() - 1
    return ms, below, prev


def word_points():
    r = np.random.default_rng(114)
    ws = [0, (1 << 64) - 1, 1, 1 << 63, 1 << 62, 2, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 1 << 31, 1 << 32]
    ws += [int.from_bytes(r.bytes(8), "little") for _ in range(1000)]
    rels = [-1, 0, 1, 63, 64, 65] + list(range(-70, 140)) + [-(1 << 20), 1 << 20]
    w = np.array([x for x in ws for _ in rels], np.uint64)
    rel = np.array([x for _ in ws for x in rels], np.int32)
    return w, rel


def clamp_points(cfg_kw):
    d = dict(DEFAULT_CFG)
    d.update(cfg_kw)
    r = np.random.default_rng(115)
    special = np.concatenate([neighbours([float(d[k]) for k in ("am", "aM", "vm", "vM")] + [20.0, -20.0, 1.0, -1.0]), [1e300, -1e300, 5e-324, -5e-324]])
    a, b = np.meshgrid(special, special)
    n = 200000
    ra = np.ldexp(r.uniform(-1, 1, n), r.integers(-20, 20, n))
    rb = np.where(r.uniform(0, 1, n) < 0.2, ra, np.ldexp(r.uniform(-1, 1, n), r.integers(-20, 20, n)))
    return np.concatenate([a.reshape(-1), ra, r.choice(special, n), ra]), np.concatenate([b.reshape(-1), rb, ra, r.choice(special, n)])


# ====================================================================================== decisions (zero tolerance)
def limit_divisors():
    out = []
    for name, kw in LIMIT_CFGS:
        am = abs(float(dict(DEFAULT_CFG, **kw)["am"]))
        for b in (am, 2 * am):
            if b not in out:
                out.append(b)
    return out


def check_div_const(P):
    """div_const(x, b, RN(1 / b)) == x / b, for b = |am|, 2 |am| of the default configuration and of every moved-argument
    fixture / variant.  Excluded, as the source documents: the sign of a zero result, results in the subnormal range."""
    for b in limit_divisors():
        x = div_const_points(b)
        got = P.call("div_const", [x, np.full_like(x, b), np.full_like(x, 1.0 / b)], [np.float64])
        want = x / b
        normal = np.abs(want) >= 2.2250738585072014e-308
        assert np.array_equal(got[normal], want[normal]), (b, x[normal][got[normal] != want[normal]][:5])
        assert np.array_equal(bits(got[normal]), bits(want[normal]))
        zero = want == 0
        assert np.all(got[zero] == 0)
        assert np.count_nonzero(normal) > 900000


def check_brake_needed(P):
    for name, kw in LIMIT_CFGS:
        p, v, fp, fv, want = brake_points(kw)
        got = P.call("brake_needed", [p, v, fp, fv], [np.int32], cfg=make_cfg(**kw))
        assert 0.1 < want.mean() < 0.9, (name, want.mean())                    # both outcomes are there
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (name, len(bad), p[bad[:3]], v[bad[:3]], fp[bad[:3]], fv[bad[:3]])


def check_min_max(P):
    """dmin / dmax == the compare-and-select forms on finite operands; zeros of different sign: a zero, either sign (documented)"""
    for name, kw in LIMIT_CFGS:
        a, b = clamp_points(kw)
        mn, mx = P.call("dmin", [a, b], [np.float64]), P.call("dmax", [a, b], [np.float64])
        assert np.array_equal(bits(mn), bits(np.where(a < b, a, b))) and np.array_equal(bits(mx), bits(np.where(a > b, a, b))), name
    z = f64([0.0, -0.0, 0.0, -0.0])
    w = f64([-0.0, 0.0, 0.0, -0.0])
    mn, mx = P.call("dmin", [z, w], [np.float64]), P.call("dmax", [z, w], [np.float64])
    assert np.all(mn == 0) and np.all(mx == 0)
    assert np.array_equal(bits(mn[2:]), bits(z[2:])) and np.array_equal(bits(mx[2:]), bits(z[2:]))     # like signs: that zero
    print("MATH_PROBE %-4s min/max(+0,-0),(-0,+0) sign bits: dmin %s dmax %s" % (P.kind, np.signbit(mn[:2]).astype(int), np.signbit(mx[:2]).astype(int)))


def check_clamps(P):
    """clip_a and the speed clamp of outcome(), at, just inside and just outside the bounds (ref :1502, :1521, :1528-1535)"""
    for name, kw in LIMIT_CFGS:
        d = dict(DEFAULT_CFG, **kw)
        am, aM, vm, vM, v0, dt = (float(d[k]) for k in ("am", "aM", "vm", "vM", "v0", "deltaT"))
        cfg = make_cfg(**kw)
        r = np.random.default_rng(116)
        x = np.concatenate([neighbours([am, aM, 0.0, -0.0]), r.uniform(2 * am, 2 * aM, 100000), [1e300, -1e300]])
        got = P.call("clip_a", [x], [np.float64], cfg=cfg)
        t = np.where(x > am, x, am)
        want = np.where(aM < t, aM, t)
        nz = x != 0
        assert np.array_equal(bits(got[nz]), bits(want[nz])) and np.all(got[~nz] == 0), name
        # a = 0: v + a deltaT IS v, so the bounds are hit exactly; then anything
        n = 100000
        v = np.concatenate([neighbours([vm, vM]), r.uniform(vm - 2, vM + 2, n)])
        a = np.concatenate([np.zeros(6), np.where(r.uniform(0, 1, n) < 0.3, 0.0, r.uniform(am, aM, n))])
        p = r.uniform(-20, 170, len(v))
        ctl = (r.uniform(0, 1, len(v)) < 0.8).astype(np.int32)
        ctl[:6] = 1
        pn, vn = P.call("outcome", [p, v, a, ctl], [np.float64, np.float64], cfg=cfg)
        xx = v + a * dt
        t = np.where(vm > xx, vm, xx)
        wv = np.where(ctl != 0, np.where(t < vM, t, vM), v0)
        wp = p - v * dt - 0.5 * a * math.pow(dt, 2)
        assert np.array_equal(bits(vn), bits(wv)) and np.array_equal(bits(pn), bits(wp)), name
        assert np.count_nonzero(vn == vm) > 100 and np.count_nonzero(vn == vM) > 100


def check_key_less(P):
    d1, v1, r1, d2, v2, r2 = key_less_points()
    got = P.call("key_less", [d1, v1, r1, d2, v2, r2], [np.int32])
    want = (d1 < d2) | ((d1 == d2) & ((v1 < v2) | ((v1 == v2) & (r1 < r2))))
    assert np.array_equal(got, want.astype(np.int32)) and 0.3 < want.mean() < 0.7


def check_mul24(P):
    a, b, c = mul24_points()
    assert np.array_equal(P.call("mul24", [a, b], [np.int32]), a * b)
    assert np.array_equal(P.call("mad24", [a, b, c], [np.int32]), a * b + c)


def check_words(P):
    w, rel = word_points()
    got_sel = P.call("below_sel", [rel], [np.uint64])
    got_pop = P.call("popc_below", [w, rel], [np.int32])
    for q in range(len(w)):
        r = min(max(int(rel[q]), 0), 64)
        sel = (1 << r) - 1
        assert int(got_sel[q]) == sel, (int(rel[q]), hex(int(got_sel[q])))
        assert int(got_pop[q]) == bin(int(w[q]) & sel).count("1"), (hex(int(w[q])), int(rel[q]), int(got_pop[q]))


def check_masks(P, NW):
    ms, below, prev = mask_reference(NW)
    words = mask_words(ms, NW)
    T = 64 * NW + 1
    n = len(ms) * T
    assert np.array_equal(P.call("mask_below", [words], [np.int32], k=(NW, T), n=n).reshape(len(ms), T), below)
    assert np.array_equal(P.call("mask_prev", [words], [np.int32], k=(NW, T), n=n).reshape(len(ms), T), prev)
    assert np.array_equal(P.call("mask_count", [words], [np.int32], k=(NW, 1), n=len(ms)), below[:, -1])
    # mask_rank: t is the calling thread (one mask per workgroup of 64 NW threads on the device)
    got = P.call("mask_rank", [words], [np.int32], k=(NW, T - 1), n=len(ms) * (T - 1)).reshape(len(ms), T - 1)
    assert np.array_equal(got, below[:, :-1])


def check_sqrt(P):
    """sqrt(dx * dx + dy * dy) as ph_reward forms the FP64 collision distance == NumPy's (correctly rounded sqrt, no contraction)"""
    r = np.random.default_rng(117)
    n = 1000000
    dx, dy = r.uniform(-200, 200, n), r.uniform(-200, 200, n)
    ang, rad = r.uniform(0, 2 * math.pi, n // 4), r.uniform(1.9, 3.1, n // 4)
    dx[: n // 4], dy[: n // 4] = rad * np.cos(ang), rad * np.sin(ang)
    dx[-4:], dy[-4:] = [0, 2, 0, 1e-200], [0, 0, 3, 1e-200]
    got = P.call("sqrt_xy", [dx, dy], [np.float64])
    assert np.array_equal(bits(got), bits(np.sqrt(dx * dx + dy * dy)))


def check_refused_arguments(P):
    """lane / m select table entries: the entry points refuse what the layout does not have, before anything runs"""
    p = f64([1.0, 2.0])
    o2 = [(np.float64, 2), (np.float64, 2)]
    assert P.raw("get_xy", [p], o2, k=(12, 0))[0] == E_LANE and P.raw("get_xy", [p], o2, k=(-1, 0))[0] == E_LANE
    assert P.raw("get_xy", [p], o2, cfg=make_cfg(lane_num=4), k=(0, 0))[0] == E_LANE
    assert P.raw("geo_xy", [p], o2, cfg=make_cfg(lane_num=4), k=(4, 0))[0] == E_LANE
    assert P.raw("geo_xy", [p], o2, cfg=make_cfg(lane_num=8), k=(0, 2))[0] == E_LANE        # no right turn from an inner lane
    assert P.raw("geo_xy", [p], o2, cfg=make_cfg(lane_num=8), k=(0, 3))[0] == E_LANE
    assert P.raw("geo_xy", [p], o2, cfg=make_cfg(lane_num=5), k=(0, 0))[0] == E_ARGS
    assert P.raw("mask_below", [np.zeros(3, np.uint64)], [(np.int32, 1)], k=(3, 1), n=1)[0] == E_ARGS
    assert P.raw("mask_rank", [np.zeros(2, np.uint64)], [(np.int32, 64)], k=(2, 64), n=64)[0] == E_ARGS
    if P.kind == "host":
        assert P.raw("actor_tanh3", [np.zeros(2, np.float32)], [(np.float32, 2)])[0] == E_DEVICE_ONLY


# ====================================================================================== reward values
REWARD_BAR = 1e-12       # 1 / 1000 of the 1e-9 at which the suite asserts rewards


def check_exp(P):
    x = exp_points()
    got = P.call("exp_m2_0", [x], [np.float64])
    rel = max(abs(mpmath.mpf(float(g)) - r) / r for g, r in zip(got, exp_ref()))
    report(P, "exp_m2_0 [-2,0] max rel (bar 2^-50=8.9e-16)", float(rel), "= %.2f x 2^-52" % float(rel * 2 ** 52))
    assert rel <= 2.0 ** -50
    assert got[np.nonzero(x == 0)[0]].tolist() == [1.0, 1.0]                   # 0 and -0.0


def check_coth(P):
    hi, lo = coth_points()
    got = P.call("reward_coth_term", [hi], [np.float64])
    err = abs_err(got, coth_ref())
    report(P, "reward_coth_term [1/16,4) max abs (bar 1e-12)", float(err))
    assert err <= REWARD_BAR
    g = P.call("reward_coth_term", [lo], [np.float64])
    report(P, "reward_coth_term (0,1/16) max value (<= -64)", float(np.max(g)))
    assert not np.any(np.isnan(g)) and np.all(g <= -64.0)
    tiny = P.call("reward_coth_term", [f64([2.2e-16, 1.1e-16, 1e-17])], [np.float64])
    assert not np.any(np.isnan(tiny)) and np.all(tiny <= -64.0) and tiny[2] == -np.inf, tiny      # den == 0: -inf, never NaN


def check_log(P):
    z = log_points()
    got = P.call("reward_log_term", [z], [np.float64])
    err = abs_err(got, log_ref())
    report(P, "reward_log_term [1e-5,1.00001] max abs (bar 1e-12)", float(err))
    assert err <= REWARD_BAR
    assert got[np.nonzero(z == 1.0)[0][0]] == 0.0
    # The fold at sqrt(1/2) is what keeps |s| <= 0.172, which is what the 10-term series needs for its 1e-16.  Where the result
    # is the series alone (z in [sqrt(1/2), 1): e = 0, nothing is added) the RELATIVE error is bounded by the roundings, each
    # <= u = 2^-53: 2 + f, the quotient (host: 1 u; device: value_div's 2 ulp = 4 u), s * s into q (x 0.03), q's last step,
    # s + s exact, the product, fma(0, ln 2, t) exact: 4 u on the host, 7 u on the device, + 0.2 u of truncation
    # (0.0295^10 / 21).  A fold moved to 0.75 sends [sqrt(1/2), 0.75) through s = 0.2 and a cancelling -ln 2: 8.7 u measured (host).
    zs, ref = log_series_points(), log_series_ref()
    g = P.call("reward_log_term", [zs], [np.float64])
    rel = max(abs(mpmath.mpf(float(a)) - q) / abs(q) for a, q in zip(g, ref))
    bar = (5 if P.kind == "host" else 8) * 2.0 ** -53
    report(P, "reward_log_term [sqrt(1/2),1) max rel (bar %.2e)" % bar, float(rel), "= %.2f x 2^-53" % float(rel * 2 ** 53))
    assert rel <= bar


def check_value_div(P):
    """host: x / y itself.  device: v_rcp_f64 + two Newton steps and one product: within 2 ulp of the correctly rounded quotient"""
    x, y = value_div_points()
    got = P.call("value_div", [x, y], [np.float64])
    want = x / y
    ulps = int(np.max(np.abs(ordinal(got) - ordinal(want))))
    report(P, "value_div max ulp distance to RN(x/y) (bar %d)" % (0 if P.kind == "host" else 2), ulps, "differing %d of %d" % (np.count_nonzero(got != want), len(x)))
    assert ulps <= (0 if P.kind == "host" else 2)


# ====================================================================================== geometry values
def check_sincos(P):
    x = sincos_points()
    sn, cs = P.call("sincos_q1", [x], [np.float64, np.float64])
    rs, rc = sincos_ref()
    err = max(abs_err(sn, rs), abs_err(cs, rc))
    report(P, "sincos_q1 [0,pi/2] max abs (bar 4e-16)", float(err))
    assert err <= 4e-16
    assert sn[np.nonzero(x == 0)[0][0]] == 0.0 and cs[np.nonzero(x == 0)[0][0]] == 1.0


def layout(lane_num, lane_cw, dis_ctl):
    """(Lb of the left / straight / right movement, spawn_p) as the reference's constructor derives them (ref :66-71, :103-105, :148-152)"""
    RL, H = {12: (7, 6), 4: (3, 2), 8: (5, 4)}[lane_num]
    inbox = [3.1415 / 2 * RL * lane_cw, 2 * H * lane_cw, 3.1415 / 2 * lane_cw]
    return inbox, [dis_ctl - H * lane_cw + b for b in inbox]


def routes(lane_num):
    if lane_num == 12:
        return [(lane, lane % 3) for lane in range(12)]
    if lane_num == 4:
        return [(lane, m) for lane in range(4) for m in range(3)]
    return [(lane, m) for lane in range(8) for m in ((0, 1) if lane % 2 == 0 else (1, 2))]


def sweep_points(lane_num, m, lane_cw, dis_ctl):
    """p from -40 m to spawn_p + 60 m; Lb, 0 and both neighbours of each; the doubles whose float32 rounding crosses (float)Lb
    or 0 (the float32 twins change branch there, the FP64 ones at Lb / 0 themselves)"""
    inbox, spawn = layout(lane_num, lane_cw, dis_ctl)
    Lb = inbox[0] if m != 2 else inbox[2]          # (get_xy / geo_xy: sel2(inbox[0], inbox[2], m == 2); the straight path has no branch)
    r = np.random.default_rng(200 + lane_num + m)
    Lf = np.float32(Lb)
    f32_edges = [float(Lf), float(np.nextafter(Lf, np.float32(0))), float(np.nextafter(Lf, np.float32(1e9)))]
    f32_edges += [(f32_edges[0] + f32_edges[1]) / 2, (f32_edges[0] + f32_edges[2]) / 2]
    tiny = [1e-46, -1e-46, 7e-46, 1.4e-45, 1e-38, -1e-38, 1e-30, -1e-30]
    return np.concatenate([np.arange(-40.0, spawn[m] + 60.0, 0.25), r.uniform(-40, spawn[m] + 60, 300), r.uniform(-1, Lb + 1, 300),
                           neighbours([Lb, 0.0, inbox[1], spawn[m]]), neighbours(f32_edges), tiny])


@functools.lru_cache(None)
def oracle_sweep(lane_num, gname):
    """{(lane, m): (p, XY of the C oracle's get_p)}"""
    from oracle.oracle import OracleEnv
    from oracle.oracle_geo import OracleGeoEnv
    kw = dict(GEOMETRIES)[gname]
    d = dict(DEFAULT_CFG, **kw)
    arr = np.cumsum(np.full((4, lane_num), 50.0), axis=0)
    env = OracleEnv(arr, **kw) if lane_num == 12 else OracleGeoEnv(arr, lane_num, **kw)
    out = {}
    for lane, m in routes(lane_num):
        p = sweep_points(lane_num, m, float(d["lane_cw"]), float(d["dis_ctl"]))
        xy = np.array([env.get_p(float(v), lane) if lane_num == 12 else env.get_p(float(v), lane, m) for v in p])
        out[(lane, m)] = (p, xy)
    return out


def probe_xy(P, lane_num, gname, lane, m, p, single=False, general=False):
    cfg = make_cfg(lane_num=lane_num, **dict(GEOMETRIES)[gname])
    dt = np.float32 if single else np.float64
    if lane_num == 12 and not general:
        X, Y = P.call("get_xy_f32" if single else "get_xy", [f64(p)], [dt, dt], cfg=cfg, k=(lane,))
    else:
        X, Y = P.call("geo_xy_f32" if single else "geo_xy", [f64(p)], [dt, dt], cfg=cfg, k=(lane, m))
    return np.stack([X, Y], axis=1)


GEO_BAR = 1e-12          # the bar tests/test_oracle_golden.py / test_oracle_geo.py hold the oracle's get_p to


def check_xy_golden(P):
    """get_xy / geo_xy == the reference's own get_p tables (tests/golden/geometry*.npz)"""
    from tests.parity_util import GOLDEN_DIR
    g = np.load(os.path.join(GOLDEN_DIR, "geometry.npz"))
    worst = 0.0
    for lane in range(12):
        for general in (False, True):
            xy = probe_xy(P, 12, "default", lane, lane % 3, g["ps"], general=general)
            worst = max(worst, float(np.max(np.abs(xy - g["get_p"][lane]))))
    for fname, gname in (("geometry_geo.npz", "default"), ("geometry_geo_kw.npz", "kw")):
        g = np.load(os.path.join(GOLDEN_DIR, fname))
        for lane_num in (4, 8):
            n = 0
            for lane, m in routes(lane_num):
                ref = g["get_p%d" % lane_num][lane, m]
                assert not np.any(np.isnan(ref))
                worst = max(worst, float(np.max(np.abs(probe_xy(P, lane_num, gname, lane, m, g["ps%d" % lane_num]) - ref))))
                n += 1
            assert n == np.count_nonzero(~np.all(np.isnan(g["get_p%d" % lane_num]), axis=(2, 3)))      # every route the reference has
    report(P, "get_xy/geo_xy vs golden tables max abs (bar 1e-12)", worst)
    assert worst <= GEO_BAR


def check_xy_oracle(P, lane_num, gname):
    """get_xy / geo_xy == the C oracle's get_p on the dense sweep"""
    worst = 0.0
    for (lane, m), (p, ref) in oracle_sweep(lane_num, gname).items():
        xy = probe_xy(P, lane_num, gname, lane, m, p)
        worst = max(worst, float(np.max(np.abs(xy - ref))))
        if lane_num == 12:                                          # the general path hands 12 lanes to get_xy: bit for bit
            assert np.array_equal(bits(probe_xy(P, 12, gname, lane, m, p, general=True)), bits(xy))
    report(P, "xy vs oracle sweep lanes=%d %s max abs (bar 1e-12)" % (lane_num, gname), worst)
    assert worst <= GEO_BAR


# ====================================================================================== pre-filter soundness
PREFILTER_BAR = 1e-3     # the bound the source states; soundness needs 0.025 m per vehicle (half of the 5 cm margin)


def check_f32_twins(P, lane_num, gname):
    worst = 0.0
    for (lane, m), (p, _) in oracle_sweep(lane_num, gname).items():
        d = probe_xy(P, lane_num, gname, lane, m, p, single=True).astype(np.float64) - probe_xy(P, lane_num, gname, lane, m, p)
        worst = max(worst, float(np.max(np.hypot(d[:, 0], d[:, 1]))))
    report(P, "f32 twin vs f64 lanes=%d %s max dist m (bar 1e-3)" % (lane_num, gname), worst)
    assert worst <= PREFILTER_BAR


def check_frcp(P):
    """1 / x of the pre-filters (v_rcp_f32 on the device: 1 ulp) on the divisors they form: Lb, rl * cw, cw"""
    r = np.random.default_rng(118)
    x = np.concatenate([r.uniform(1, 100, 100000), [2.5, 3.0, 3.5, 7.5, 17.5, 27.488125, 3.926875]]).astype(np.float32)
    got = P.call("frcp", [x], [np.float32])
    rel = float(np.max(np.abs(got.astype(np.float64) * x.astype(np.float64) - 1.0)))
    report(P, "frcp [1,100] max rel (bar 2^-22=2.4e-7)", rel)
    assert rel <= 2.0 ** -22                                                    # 1 ulp of the result + its own rounding, with room: a pre-filter


def check_prefilter_pairs(P, lane_num, gname, thr):
    """No pair closer than collision_thr in FP64 may fail the float32 pre-filter (it would never reach the FP64 test).  200 000
    pairs whose FP64 distance is within 0.1 m of the threshold, across routes and within a route: a coarse grid per route finds
    the (route, p) x (route, p) cells near the threshold, the pairs are drawn inside those cells."""
    d = dict(DEFAULT_CFG, **dict(GEOMETRIES)[gname])
    inbox, _ = layout(lane_num, float(d["lane_cw"]), float(d["dis_ctl"]))
    r = np.random.default_rng(300 + lane_num)
    rts = routes(lane_num)
    G = 240
    grid = np.linspace(-12.0, max(inbox) + 12.0, G)
    h = grid[1] - grid[0]
    C64 = [probe_xy(P, lane_num, gname, lane, m, grid) for lane, m in rts]
    cells = []
    for i in range(len(rts)):
        for j in range(i, len(rts)):
            dist = np.hypot(C64[i][:, None, 0] - C64[j][None, :, 0], C64[i][:, None, 1] - C64[j][None, :, 1])
            k, l = np.nonzero(np.abs(dist - thr) < 0.1 + 1.5 * h)
            if i == j:
                k, l = k[k != l], l[k != l]
            cells.append(np.stack([np.full(len(k), i), k, np.full(len(k), j), l], axis=1))
    cells = np.concatenate(cells)
    same_cell = cells[:, 0] == cells[:, 2]                          # a quarter of the draws within a route, the rest across routes
    pick = np.concatenate([cells[same_cell][r.integers(0, np.count_nonzero(same_cell), 400000)],
                           cells[~same_cell][r.integers(0, np.count_nonzero(~same_cell), 1400000)]])
    pick = pick[r.permutation(len(pick))]
    ra, rb = pick[:, 0], pick[:, 2]
    pa, pb = grid[pick[:, 1]] + r.uniform(-h / 2, h / 2, len(pick)), grid[pick[:, 3]] + r.uniform(-h / 2, h / 2, len(pick))
    A64, B64 = np.zeros((len(pick), 2)), np.zeros((len(pick), 2))
    A32, B32 = np.zeros((len(pick), 2), np.float32), np.zeros((len(pick), 2), np.float32)
    for q, (lane, m) in enumerate(rts):
        for rr, pp, o64, o32 in ((ra, pa, A64, A32), (rb, pb, B64, B32)):
            idx = np.nonzero(rr == q)[0]
            if len(idx):
                o64[idx] = probe_xy(P, lane_num, gname, lane, m, pp[idx])
                o32[idx] = probe_xy(P, lane_num, gname, lane, m, pp[idx], single=True)
    dx, dy = B64[:, 0] - A64[:, 0], B64[:, 1] - A64[:, 1]
    d64 = np.sqrt(dx * dx + dy * dy)
    band = np.nonzero(np.abs(d64 - thr) < 0.1)[0]
    assert len(band) >= 200000, len(band)
    band = band[:200000]                                            # (the draws are in random order already)
    d64, same_route = d64[band], (ra == rb)[band]
    assert np.count_nonzero(same_route) >= 5000 and np.count_nonzero(~same_route) >= 50000, np.count_nonzero(same_route)
    fx, fy = B32[band, 0] - A32[band, 0], B32[band, 1] - A32[band, 1]
    lim = np.float32(thr) + np.float32(0.05)
    assert fx.dtype == np.float32 and (fx * fx + fy * fy).dtype == np.float32 and (lim * lim).dtype == np.float32
    near = fx * fx + fy * fy < lim * lim
    hit = d64 < thr
    assert np.count_nonzero(hit) >= 10000 and np.count_nonzero(~hit) >= 10000, np.count_nonzero(hit)
    slack = float(np.min(d64[~near]) - thr) if np.any(~near) else float("inf")
    report(P, "pre-filter lanes=%d %s thr=%g: closest rejected pair - thr" % (lane_num, gname, thr), slack,
           "hits %d of %d, dropped %d" % (np.count_nonzero(hit), len(band), np.count_nonzero(hit & ~near)))
    assert not np.any(hit & ~near)


# ====================================================================================== the actor's activation (device only)
# Measured on the device (MI355X) against 3 tanh(z) in mpmath: see profiles/math_probe.txt.  The bar is twice the measurement:
# the instructions are deterministic, the factor covers points not drawn.  5e-6 = 1 / 100 of ACTION_TOL is where a bar
# would stop being a bar and become a finding.
ACTOR_TANH3_MEASURED = 8.103e-7          # (the source's "3.6e-7 on the action" was taken on the actions of one roll-out)
ACTOR_TANH3_BAR = 2 * ACTOR_TANH3_MEASURED


@functools.lru_cache(None)
def tanh3_points():
    r = np.random.default_rng(119)
    z = np.concatenate([r.uniform(-20, 20, 30000), r.uniform(-3, 3, 10000), np.linspace(-44.4, -44.3, 200), np.linspace(44.3, 44.4, 200),
                        [0.0, -0.0, 100.0, -100.0, 1e30, -1e30, 20.0, -20.0, 88.0, -88.0, 1e-30, -1e-30, 1e-45, -1e-45]]).astype(np.float32)
    return np.sort(z, kind="stable")


@functools.lru_cache(None)
def tanh3_ref():
    return mp_map(lambda z: 3 * mpmath.tanh(z), tanh3_points())


def check_actor_tanh3(P):
    z = tanh3_points()
    got = P.call("actor_tanh3", [z], [np.float32])
    err = float(abs_err(got, tanh3_ref()))
    report(P, "actor_tanh3 max abs vs 3 tanh(z) (bar %.3e)" % ACTOR_TANH3_BAR, err)
    assert np.all(np.isfinite(got)) and np.all(got <= 3.0) and np.all(got >= -3.0)
    assert np.all(np.diff(got.astype(np.float64)) >= 0), z[np.nonzero(np.diff(got.astype(np.float64)) < 0)[0][:5]]     # z is sorted
    assert np.all(got[z >= 44.3] == 3.0) and np.all(got[z <= -44.3] == -3.0)
    assert np.all(got[z == 0] == 0.0)
    assert ACTOR_TANH3_BAR is not None and ACTOR_TANH3_BAR <= 5e-6
    assert err <= ACTOR_TANH3_BAR


# ====================================================================================== device build == host build, bit for bit
def check_bit_equal(dev, host):
    """Every helper without a device-only branch: the hipcc build on the device returns, bit for bit, what the g++ build returns
    on the same (NaN-free) inputs.  This is the -ffp-contract=off contract of csrc/Makefile for these functions."""
    def same(name, ins, dts, **kw):
        a, b = dev.call(name, ins, dts, **kw), host.call(name, ins, dts, **kw)
        a, b = (a, b) if isinstance(a, list) else ([a], [b])
        for x, y in zip(a, b):
            assert np.array_equal(bits(x) if x.dtype.kind == "f" else x, bits(y) if y.dtype.kind == "f" else y), (name, kw.get("k"))

    same("exp_m2_0", [exp_points()], [np.float64])
    same("sincos_q1", [sincos_points()], [np.float64, np.float64])
    for b in limit_divisors():
        x = div_const_points(b)
        same("div_const", [x, np.full_like(x, b), np.full_like(x, 1.0 / b)], [np.float64])
    for name, kw in LIMIT_CFGS:
        same("brake_needed", list(brake_points(kw)[:4]), [np.int32], cfg=make_cfg(**kw))
    same("key_less", list(key_less_points()), [np.int32])
    a, b, c = mul24_points()
    same("mul24", [a, b], [np.int32])
    same("mad24", [a, b, c], [np.int32])
    w, rel = word_points()
    same("below_sel", [rel], [np.uint64])
    same("popc_below", [w, rel], [np.int32])
    for NW in (1, 2, 4):
        ms = mask_set(NW)
        words, T = mask_words(ms, NW), 64 * NW + 1
        same("mask_below", [words], [np.int32], k=(NW, T), n=len(ms) * T)
        same("mask_prev", [words], [np.int32], k=(NW, T), n=len(ms) * T)
        same("mask_count", [words], [np.int32], k=(NW, 1), n=len(ms))
    for gname, gkw in GEOMETRIES:
        for lane_num in (12, 4, 8):
            cfg = make_cfg(lane_num=lane_num, **gkw)
            d = dict(DEFAULT_CFG, **gkw)
            for lane, m in routes(lane_num):
                p = sweep_points(lane_num, m, float(d["lane_cw"]), float(d["dis_ctl"]))
                if lane_num == 12:
                    same("get_xy", [p], [np.float64, np.float64], cfg=cfg, k=(lane,))
                same("geo_xy", [p], [np.float64, np.float64], cfg=cfg, k=(lane, m))

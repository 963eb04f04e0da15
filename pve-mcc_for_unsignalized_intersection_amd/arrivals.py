"""Arrival streams: the synthetic generator of BASELINE.md §3 and the loader of the reference's
MATLAB v5 `arvTimeNewVeh` files (main.py:387-389, data/test/*.mat)."""
import numpy as np


def synthetic_arrivals(n_envs, rate, horizon_s, seed=20250213, rows=None, lane_num=12):
    """float64 [n_envs, rows, lane_num]: per env e and lane, cumulative sums of inter-arrival times
    max(1.0, Exponential(3600/rate)) from numpy.random.default_rng(seed + e), padded with +inf
    (the shipped streams have the same clipped-exponential shape)."""
    mean = 3600.0 / float(rate)
    if rows is None:
        rows = 64 + int(np.ceil(horizon_s / mean)) * 2
    out = np.full((n_envs, rows, lane_num), np.inf, dtype=np.float64)
    for e in range(n_envs):
        rng = np.random.default_rng(seed + e)
        dt = np.maximum(1.0, rng.exponential(mean, size=(rows - 1, lane_num)))
        out[e, :rows - 1, :] = np.cumsum(dt, axis=0)
    return out


def synthetic_intentions(n_envs, rows, seed=20250213, lane_num=8):
    """int32 [n_envs, rows, lane_num] of 0/1: the intention draws of the 8-lane layout (the reference's
    random.randint(0, 1) at ref :390, one per arriving vehicle), from numpy.random.default_rng(seed + e)."""
    out = np.zeros((n_envs, rows, lane_num), dtype=np.int32)
    for e in range(n_envs):
        out[e] = np.random.default_rng(seed + 7919 * (e + 1)).integers(0, 2, size=(rows, lane_num))
    return out


# ---------------------------------------------------------------------------------------------
# NumPy restatement of csrc/pve_arrivals.h, operation for operation: the streams pve_generate_arrivals
# (BatchedIntersections.generate_arrivals) writes on the device, bit for bit.
ARR_KEY = (0x41525256, 0x54494D45)
INT_KEY = (0x494E5445, 0x4E54494F)


def exp_from_words(w):
    """x = -ln((2 w + 1) 2^-33) of 32-bit words as float64: pve_arrivals.h's arrival_exp (the logarithm of noise_gauss's radius)."""
    from .noise import _LN2, _LOG_C, _MASK32, _SQRT_HALF
    w = np.asarray(w, np.uint64) & _MASK32
    m = (w * np.uint64(2) + np.uint64(1)).astype(np.float64)            # exact: < 2^33
    f, e = np.frexp(m)                                                  # exact: m = f 2^e, f in [1/2, 1)
    e = e.astype(np.int64)
    low = f < _SQRT_HALF
    f = np.where(low, f * 2.0, f)
    e = np.where(low, e - 1, e)
    s = (f - 1.0) / (f + 1.0)
    s2 = s * s
    L = np.full_like(s, _LOG_C[0])
    for c in _LOG_C[1:]:
        L = L * s2 + c
    return (33 - e).astype(np.float64) * _LN2 - 2.0 * (s * L)


def _env_words(n_envs, env_offset):
    env = (np.arange(n_envs, dtype=np.int64) + int(env_offset)).astype(np.uint64)
    return env & np.uint64(0xFFFFFFFF), env >> np.uint64(32)


def _keys(seed, tweak):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed & 0xFFFFFFFF) ^ tweak[0], (seed >> 32) ^ tweak[1]


def device_mean(rate, n_envs):
    """mean gap in seconds, float64 [n_envs]: 3600 / rate with rate in veh/h/lane, a scalar or one per environment"""
    r = np.asarray(rate, np.float64)
    if r.ndim not in (0, 1) or (r.ndim == 1 and r.shape[0] != n_envs):
        raise ValueError("rate must be a scalar or [n_envs]")
    return np.broadcast_to(3600.0 / r, (n_envs,)).astype(np.float64)


def default_rows(rate, horizon_s):
    """The rows synthetic_arrivals allots to horizon_s seconds -- 64 + 2 ceil(horizon / mean) -- at the largest rate"""
    mean = 3600.0 / float(np.max(np.asarray(rate, np.float64)))
    return 64 + int(np.ceil(horizon_s / mean)) * 2


def arrival_words(n_envs, rows, lane_num, seed=0, epoch=0, env_offset=0):
    """uint64 [n_envs, rows - 1, lane_num]: the 32-bit Philox word behind every gap of device_arrivals"""
    from .noise import philox4x32_10
    lo, hi = _env_words(n_envs, env_offset)
    quads = (rows - 1 + 3) // 4
    c0 = np.arange(quads, dtype=np.uint64)[None, :, None] | (np.arange(lane_num, dtype=np.uint64)[None, None, :] << np.uint64(28))
    words = philox4x32_10((c0, np.uint64(int(epoch) & 0xFFFFFFFF), lo[:, None, None], hi[:, None, None]), _keys(seed, ARR_KEY))
    return np.stack(words, axis=2).reshape(n_envs, quads * 4, lane_num)[:, :rows - 1]    # row 4 q + k = word k of quad q


def device_arrivals(n_envs, rows, lane_num, rate, seed=0, epoch=0, env_offset=0, min_gap=1.0):
    """float64 [n_envs, rows, lane_num]: the stream pve_generate_arrivals writes (csrc/pve_arrivals.h).  Row r < rows - 1 of
    chain (env, lane) is the running float64 sum, in ascending r, of max(min_gap, mean * x) with x the exponential deviate of
    Philox word r & 3 at counter ((r >> 2) | (lane << 28), epoch, env_global low, high); row rows - 1 is +inf.
    np.cumsum along the rows adds sequentially in that order (tests/test_arrivals_device.py asserts it)."""
    if rows < 2:
        raise ValueError("rows must be >= 2")
    mean = device_mean(rate, n_envs)
    d = mean[:, None, None] * exp_from_words(arrival_words(n_envs, rows, lane_num, seed, epoch, env_offset))
    d = np.where(d < float(min_gap), float(min_gap), d)
    out = np.full((n_envs, rows, lane_num), np.inf, dtype=np.float64)
    out[:, :rows - 1] = np.cumsum(d, axis=1)
    return out


def device_intentions(n_envs, rows, seed=0, epoch=0, env_offset=0, lane_num=8):
    """int32 [n_envs, rows, lane_num] of 0/1: the intention draws pve_generate_arrivals writes for the 8-lane layout: entry (e, r, l)
    is bit r & 31 of Philox word (r >> 5) & 3 at counter ((r >> 7) | (l << 28), epoch, env_global low, high)."""
    from .noise import philox4x32_10
    lo, hi = _env_words(n_envs, env_offset)
    chunks = (rows + 127) // 128
    c0 = np.arange(chunks, dtype=np.uint64)[None, :, None] | (np.arange(lane_num, dtype=np.uint64)[None, None, :] << np.uint64(28))
    words = philox4x32_10((c0, np.uint64(int(epoch) & 0xFFFFFFFF), lo[:, None, None], hi[:, None, None]), _keys(seed, INT_KEY))
    w = np.stack(words, axis=2)                                                          # [n_envs, chunks, 4, lane_num]
    bits = (w[:, :, :, None, :] >> np.arange(32, dtype=np.uint64)[None, None, None, :, None]) & np.uint64(1)
    return bits.reshape(n_envs, chunks * 128, lane_num)[:, :rows].astype(np.int32)


def device_covered(arrivals):
    """float64 [n_envs]: min over lanes of the last finite row, what pve_generate_arrivals reports as `covered`"""
    return np.asarray(arrivals)[:, -2, :].min(axis=1)


def pad_stream(arr, extra_rows=1):
    """Replace the zero padding at the tail of a shipped stream by +inf so that an
    exhausted lane simply stops spawning (the reference would spawn every tick, ref :379)."""
    a = np.array(arr, dtype=np.float64, copy=True)
    for l in range(a.shape[1]):
        col = a[:, l]
        nz = np.flatnonzero(col > 0)
        last = nz[-1] if len(nz) else -1
        col[last + 1:] = np.inf
    if extra_rows:
        a = np.concatenate([a, np.full((extra_rows, a.shape[1]), np.inf)], axis=0)
    return a


# ---------------------------------------------------------------------------------------------
# MATLAB v5 reader for the reference's arrival streams (main.py:387-389 uses scipy.io.loadmat;
# this ~60-line reader removes the SciPy dependency for the one variable the path needs).
_MI_SIZES = {1: ("i1", 1), 2: ("u1", 1), 3: ("i2", 2), 4: ("u2", 2), 5: ("i4", 4), 6: ("u4", 4),
             7: ("f4", 4), 9: ("f8", 8), 12: ("i8", 8), 13: ("u8", 8)}


def _read_tag(buf, off):
    """-> (type, nbytes, data_offset, next_offset) of one MAT-v5 data element (handles the small format)."""
    import struct
    t, n = struct.unpack_from("<II", buf, off)
    if t >> 16:                                    # small data element: size in the upper half-word
        return t & 0xFFFF, t >> 16, off + 4, off + 8
    return t, n, off + 8, off + 8 + (n + 7) // 8 * 8


def load_arrival_mat(path, name="arvTimeNewVeh"):
    """float64 [rows, 12] `arvTimeNewVeh` matrix of a MATLAB 5.0 MAT-file (data/test/*.mat of the reference).
    Supports little-endian files, zlib-compressed (miCOMPRESSED) or plain miMATRIX elements, real numeric
    2-D arrays of any integer / float storage type."""
    import struct
    import zlib
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 128 or not raw.startswith(b"MATLAB 5.0 MAT-file"):
        raise ValueError("%s: not a MATLAB 5.0 MAT-file" % path)
    if raw[126:128] != b"IM":
        raise ValueError("%s: big-endian MAT-files are not supported" % path)
    off = 128
    while off + 8 <= len(raw):
        t, n, d0, nxt = _read_tag(raw, off)
        off = nxt if t != 15 else d0 + n           # compressed elements are not padded
        if t == 15:
            elem = zlib.decompress(raw[d0:d0 + n])
            t, n, d0, _ = _read_tag(elem, 0)
        else:
            elem = raw
        if t != 14:
            continue
        p = d0
        ft, fn, fd, p = _read_tag(elem, p)          # array flags
        flags = struct.unpack_from("<I", elem, fd)[0]
        klass, is_complex = flags & 0xFF, bool(flags & 0x0800)
        dt, dn, dd, p = _read_tag(elem, p)          # dimensions
        dims = np.frombuffer(elem, dtype="<i4", count=dn // 4, offset=dd)
        nt, nn, nd, p = _read_tag(elem, p)          # name
        vname = elem[nd:nd + nn].decode("latin1")
        if vname != name:
            continue
        if is_complex or klass not in (6, 7, 8, 9, 10, 11, 12, 13, 14, 15) or len(dims) != 2:
            raise ValueError("%s: variable %s is not a real numeric 2-D array" % (path, name))
        rt, rn, rd, p = _read_tag(elem, p)          # real part, column-major, possibly a narrower storage type
        if rt not in _MI_SIZES:
            raise ValueError("%s: unsupported storage type %d" % (path, rt))
        code, size = _MI_SIZES[rt]
        data = np.frombuffer(elem, dtype="<" + code, count=rn // size, offset=rd).astype(np.float64)
        return np.ascontiguousarray(data.reshape(int(dims[1]), int(dims[0])).T)
    raise KeyError("%s: variable %s not found" % (path, name))

"""The generators' and replay helpers' small PVE_HD functions, one at a time (csrc/pve_noise.h, pve_arrivals.h, pve_replay.h,
pve_prio.h behind the entry points of tests/math_probe/pve_math_probe.hip), at the words a roll-out or a memory draws with
probability 2^-32: the ends of the word range, both sides of the sqrt(1/2) fold in every binade, the quadrant and octant
borders of the angle, subnormal differences, NaNs of either sign, Feistel domains of 1 and of 2^31 - 1.  Every check takes the
backend (`Probe("host")`: the g++ build; `Probe("hip")`: the hipcc build with the product's flags, on the device) and is called
by tests/test_gen_probe.py and tests/test_gpu_gen_probe.py.  Everything is compared bit for bit -- against the NumPy
restatements (pve_mcc_amd/noise.py, arrivals.py, replay.py), NumPy float32 and Python integers -- except where a bar is named:
the accuracy of z and of the exponential deviate against mpmath (the headers' own 1e-6 absolute / 1e-12 relative) and the
importance weight (powf: libm on the host, ocml on the device) against the float64 expression under WEIGHT_BAR.
Figures are printed as `GEN_PROBE <backend> <what> <figure>` before they are asserted (profiles/gen_probe.txt keeps them)."""
import functools
import itertools
import math

import mpmath
import numpy as np

from pve_mcc_amd import arrivals, noise, replay
from tests.math_probe_scenarios import Probe, bits  # noqa: F401  (Probe: re-exported for the test modules)
from tests.prio_scenarios import WEIGHT_BAR

U32, I32, U64, I64, F32, F64 = np.uint32, np.int32, np.uint64, np.int64, np.float32, np.float64
SEEDS = [0, 1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0]
ENVS = [-5, -1, 0, (1 << 32) - 1, 1 << 32, 1 << 40]
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),             # Random123's known answers
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
Z_BAR, EXP_BAR = 1e-6, 1e-12                 # pve_noise.h ("the requirement is 1e-6"), pve_arrivals.h ("the bar is 1e-12")
RADIUS_MAX, EXP_MIN, EXP_MAX = 6.764, 1.16e-10, 22.874


def report(P, what, figure, note=""):
    print("GEN_PROBE %-4s %-58s %.3e %s" % (P.kind, what, figure, note))


def u64(values):
    return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in values], U64)


def i64_as_u64(x):
    return np.asarray(x, I64).astype(U64)


def call(P, name, ins, dtype, width=1, k=(), n=None):
    """one output array of n x width elements"""
    n = len(ins[0]) if n is None else n
    rc, got = P.raw(name, ins, [(dtype, n * width)], k=k, n=n)
    assert rc == 0, (name, P.kind, rc)
    return got[0].reshape(n, width) if width > 1 else got[0]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b)


def first_bad(a, b):
    return np.nonzero(np.asarray(a).reshape(len(a), -1) != np.asarray(b).reshape(len(b), -1))[0][:5]


# ====================================================================================== Philox
@functools.lru_cache(None)
def philox_inputs():
    r = np.random.default_rng(401)
    c = r.integers(0, 1 << 32, (1 << 16, 4), dtype=U64).astype(U32)
    k = r.integers(0, 1 << 32, (1 << 16, 2), dtype=U64).astype(U32)
    for q, (ctr, key, _) in enumerate(KAT):
        c[q], k[q] = ctr, key
    return c, k


def check_philox(P):
    c, k = philox_inputs()
    got = call(P, "philox4x32_10", [c, k], U32, 4, n=len(c))
    for q, (_, _, want) in enumerate(KAT):
        assert tuple(int(x) for x in got[q]) == want, (q, [hex(int(x)) for x in got[q]])
    ref = np.stack(noise.philox4x32_10([c[:, q] for q in range(4)], (k[:, 0], k[:, 1])), axis=1).astype(U32)
    assert same(got, ref), first_bad(got, ref)


# ====================================================================================== the words of noise_gauss / arrival_exp
@functools.lru_cache(None)
def radius_words():
    """0, 1, 2^32 - 2, 2^32 - 1; for every binade e = 1 .. 33 of m = 2 w + 1 in [2^(e-1), 2^e): the four words around the
    fl(sqrt(1/2)) fold (m0 = the largest integer with m0 2^-e <= fl(sqrt(1/2)); 2 (m0 // 2) + 1 is m0 or m0 + 1) and the two
    around the power of two 2^(e-1)"""
    ws = [0, 1, 0xFFFFFFFE, 0xFFFFFFFF]
    for e in range(1, 34):
        m0 = int(math.floor(noise._SQRT_HALF * 2.0 ** e))                  # (exact: a 53-bit number times a power of two)
        ws += [m0 // 2 - 1, m0 // 2, m0 // 2 + 1, m0 // 2 + 2]
        if e >= 2:
            ws += [(1 << (e - 2)) - 1, 1 << (e - 2)]
    w = np.unique(np.array([x for x in ws if 0 <= x < (1 << 32)], U64))
    # both sides of the fold, in the binade itself (e = 1 holds m = 1 alone and e = 2 holds m = 3 alone: one side each)
    f, e = np.frexp((w * U64(2) + U64(1)).astype(F64))
    for q in range(3, 34):
        side = f[e == q] < noise._SQRT_HALF
        assert side.any() and not side.all(), q
    assert set(e.tolist()) == set(range(1, 34))
    return w.astype(U32)


@functools.lru_cache(None)
def angle_words():
    """the four quadrant borders (n = 2 w + 1 passes q 2^31) and the four octant borders (k passes 2^30: sine and cosine change
    places between w = q 2^30 + 2^29 - 1 and q 2^30 + 2^29), two words either side and the word itself"""
    ws = [(q * (1 << 30) + half + d) % (1 << 32) for q in range(4) for half in (0, 1 << 29) for d in (-2, -1, 0, 1, 2)]
    w = np.unique(np.array(ws, U64))
    n = w * U64(2) + U64(1)
    k = n & U64(0x7FFFFFFF)
    assert set((n >> U64(31)).tolist()) == {0, 1, 2, 3} and (k > U64(1 << 30)).any() and (k < U64(1 << 30)).any()
    for q in range(4):                                                      # the two words the swap flips between, per quadrant
        assert q * (1 << 30) + (1 << 29) - 1 in w and q * (1 << 30) + (1 << 29) in w
    return w.astype(U32)


@functools.lru_cache(None)
def gauss_edge_pairs():
    """the full cross product of the radius words and the angle words"""
    a, b = np.meshgrid(radius_words(), angle_words(), indexing="ij")
    return np.ascontiguousarray(a.reshape(-1)), np.ascontiguousarray(b.reshape(-1))


@functools.lru_cache(None)
def gauss_sweep_pairs():
    """[(w0, w1)]: 2^22 pairs in a strided sweep (odd strides: every residue class of the low bits), and 2^20 random pairs"""
    i = np.arange(1 << 22, dtype=U64)
    r = np.random.default_rng(402)
    strided = ((i * U64(1021)) & U64(0xFFFFFFFF), (i * U64(2654435761) + U64(12345)) & U64(0xFFFFFFFF))
    rand = (r.integers(0, 1 << 32, 1 << 20, dtype=U64), r.integers(0, 1 << 32, 1 << 20, dtype=U64))
    return [(a.astype(U32), b.astype(U32)) for a, b in (strided, rand)]


def subset18(x):
    """2^18 elements of a sweep, spread over all of it"""
    return np.ascontiguousarray(x[:: len(x) >> 18][: 1 << 18])


@functools.lru_cache(None)
def gauss_edge_ref():
    """z of the edge pairs in mpmath, 50 digits: sqrt(-2 ln u1) cos(2 pi u2), u = (2 w + 1) 2^-33"""
    with mpmath.workdps(50):
        rad = {int(w): mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(2 * int(w) + 1) / 2 ** 33)) for w in radius_words()}
        ang = {int(w): mpmath.cos(2 * mpmath.pi * mpmath.mpf(2 * int(w) + 1) / 2 ** 33) for w in angle_words()}
        w0, w1 = gauss_edge_pairs()
        return [rad[int(a)] * ang[int(b)] for a, b in zip(w0, w1)]


@functools.lru_cache(None)
def exp_edge_ref():
    with mpmath.workdps(50):
        return [-mpmath.log(mpmath.mpf(2 * int(w) + 1) / 2 ** 33) for w in radius_words()]


def check_noise_gauss(P):
    w0, w1 = gauss_edge_pairs()
    z = call(P, "noise_gauss", [w0, w1], F64)
    assert same(z, noise.gauss_from_words(w0, w1)), first_bad(z, noise.gauss_from_words(w0, w1))
    with mpmath.workdps(50):
        err = float(max(abs(mpmath.mpf(float(g)) - r) for g, r in zip(z, gauss_edge_ref())))
    report(P, "noise_gauss edge pairs max abs vs mpmath (bar 1e-6)", err, "%d pairs" % len(z))
    assert err <= Z_BAR
    # the radius: the angle word 0 gives cos(pi 2^-32) = 1 - 2.7e-19, so |z| is the radius to the last bit or two
    rw = radius_words()
    rad = call(P, "noise_gauss", [rw, np.zeros_like(rw)], F64)
    report(P, "noise_gauss radius min / max (0 < radius <= 6.764)", float(rad.min()), "%.6f" % rad.max())
    assert np.all(rad > 0) and np.all(rad <= RADIUS_MAX) and rad.max() == rad[rw == 0][0] and rad.min() == rad[rw == 0xFFFFFFFF][0]
    assert np.all(np.isfinite(z)) and np.abs(z).max() <= RADIUS_MAX
    # the sweeps: a 2^18 subset against NumPy, all of it inside the range
    for s0, s1 in gauss_sweep_pairs():
        zs = call(P, "noise_gauss", [s0, s1], F64)
        assert np.all(np.isfinite(zs)) and np.abs(zs).max() <= RADIUS_MAX
        assert same(subset18(zs), noise.gauss_from_words(subset18(s0), subset18(s1)))


def check_arrival_exp(P):
    w = radius_words()
    x = call(P, "arrival_exp", [w], F64)
    assert same(x, arrivals.exp_from_words(w)), first_bad(x, arrivals.exp_from_words(w))
    with mpmath.workdps(50):
        rel = float(max(abs(mpmath.mpf(float(g)) - r) / r for g, r in zip(x, exp_edge_ref())))
    report(P, "arrival_exp edge words max rel vs mpmath (bar 1e-12)", rel, "%d words" % len(w))
    assert rel <= EXP_BAR
    s0 = gauss_sweep_pairs()[0][0]
    xs = np.concatenate([x, call(P, "arrival_exp", [s0], F64)])
    report(P, "arrival_exp min / max ([1.16e-10, 22.874], never 0)", float(xs.min()), "%.6f" % xs.max())
    assert np.all(xs > 0) and xs.min() >= EXP_MIN and xs.max() <= EXP_MAX
    assert xs.min() == x[w == 0xFFFFFFFF][0] and xs.max() == x[w == 0][0]
    assert same(subset18(xs[len(x):]), arrivals.exp_from_words(subset18(s0)))


# ====================================================================================== action_noise_z / action_with_noise
@functools.lru_cache(None)
def action_inputs():
    """(seed, env_global, vehicle_id, tick): the cross product of the named values, then 2^16 random coordinates under those
    seeds and four random ones"""
    cross = list(itertools.product(SEEDS, ENVS, [0, 1, (1 << 31) - 1, -1], [0, (1 << 32) - 1]))
    r = np.random.default_rng(403)
    n = 1 << 16
    seed = np.concatenate([u64([c[0] for c in cross]), r.choice(np.concatenate([u64(SEEDS), r.integers(0, 1 << 63, 4, dtype=U64)]), n)])
    env = np.concatenate([np.array([c[1] for c in cross], I64), r.integers(-5, 1 << 40, n)])
    vid = np.concatenate([np.array([c[2] for c in cross], I32), r.integers(-1, 1 << 31, n).astype(I32)])
    tick = np.concatenate([np.array([c[3] for c in cross], U64), r.integers(0, 1 << 32, n, dtype=U64)]).astype(U32)
    a = np.concatenate([np.tile([0.7312, -2.9999, 3.0, -0.0], len(cross) // 4), r.uniform(-3, 3, n).astype(F32).astype(F64)])
    sigma = np.concatenate([np.tile([0.2, 0.5, 0.0, 1.0 / 3.0], len(cross) // 4), r.uniform(0, 1, n)])
    assert len(cross) == 192 and len(a) == len(seed)
    return seed, env, vid, tick, a, sigma


def numpy_action_noise(seed, env, vid, tick):
    """noise.action_noise takes one seed: group the elements by seed"""
    z = np.empty(len(seed))
    for s in np.unique(seed):
        m = seed == s
        z[m] = noise.action_noise(int(s), env[m], vid[m], tick[m].astype(I64))
    return z


def check_action_noise(P):
    seed, env, vid, tick, a, sigma = action_inputs()
    z = call(P, "action_noise_z", [seed, env, vid, tick], F64)
    ref = numpy_action_noise(seed, env, vid, tick)
    assert same(z, ref), first_bad(z, ref)
    got = call(P, "action_with_noise", [a, sigma, seed, env, vid, tick], F64)
    prod = sigma * ref                                                   # (rounded on its own, then the sum)
    assert same(got, a + prod), first_bad(got, a + prod)


# ====================================================================================== arrival_gap
def word_of_exp(x):
    """the word whose deviate is nearest x: u = exp(-x) = (2 w + 1) 2^-33"""
    return int(min(max(round((math.exp(-x) * 2.0 ** 33 - 1) / 2), 0), (1 << 32) - 1))


@functools.lru_cache(None)
def gap_inputs():
    """(w, mean, min_gap).  For every (mean, min_gap): the words around the one where mean * x crosses min_gap (when min_gap /
    mean lies inside the deviate's range; outside it the end words), and the range's end words.  Then, exactly on: min_gap
    := the product mean * x(w) itself and its two neighbours, which is where `d < min_gap` must be false, false, true."""
    r = np.random.default_rng(404)
    ws, means, gaps = [], [], []
    for mean, g in itertools.product([1e-3, 3.27, 1e6], [0.0, 0.5, 1.0]):
        c = word_of_exp(g / mean) if g > 0 else 0
        near = [c + d for d in range(-6, 7)] + [0, 1, 0xFFFFFFFE, 0xFFFFFFFF] + r.integers(0, 1 << 32, 16).tolist()
        near = [x for x in near if 0 <= x < (1 << 32)]
        ws += near
        means += [mean] * len(near)
        gaps += [g] * len(near)
    w, mean, g = np.array(ws, U64).astype(U32), np.array(means), np.array(gaps)
    d = mean * arrivals.exp_from_words(w)
    on = np.concatenate([d, np.nextafter(d, 0), np.nextafter(d, np.inf)])
    return np.concatenate([w, w, w, w]), np.tile(mean, 4), np.concatenate([g, on])


def check_arrival_gap(P):
    w, mean, g = gap_inputs()
    got = call(P, "arrival_gap", [w, mean, g], F64)
    d = mean * arrivals.exp_from_words(w)
    ref = np.where(d < g, g, d)
    assert same(got, ref), first_bad(got, ref)
    n = len(w) // 4
    for m, gg in itertools.product([3.27, 1e6], [0.5, 1.0]):             # the crossing is inside the range: both outcomes, next to each other
        sel = (mean[:n] == m) & (g[:n] == gg)
        assert (d[:n][sel] < gg).any() and (d[:n][sel] > gg).any(), (m, gg)
    assert np.all(d[:n][mean[:n] == 1e-3] < 0.5)                         # mean 1 ms: x <= 22.874 never reaches 0.5 s
    assert np.all(got[n:2 * n] == d[:n]) and np.all(got[2 * n:3 * n] == d[:n]) and np.all(got[3 * n:] > d[:n])     # on, below, above


# ====================================================================================== arrival_words / intention_words / _bit
@functools.lru_cache(None)
def words_inputs():
    cross = list(itertools.product(SEEDS, [0, (1 << 32) - 1], ENVS, [0, 11], [0, 1, (1 << 28) - 1]))
    seed, epoch = u64([c[0] for c in cross]), np.array([c[1] for c in cross], U64).astype(U32)
    env, lane, quad = np.array([c[2] for c in cross], I64), np.array([c[3] for c in cross], I32), np.array([c[4] for c in cross], U32)
    return seed, epoch, env, lane, quad


def check_stream_words(P):
    seed, epoch, env, lane, quad = words_inputs()
    c0 = quad.astype(U64) | (lane.astype(U64) << U64(28))
    # the two fields of counter word 0 never meet: or == sum, and both fields come back out
    assert np.array_equal(c0, quad.astype(U64) + lane.astype(U64) * U64(1 << 28)) and c0.max() < (1 << 32)
    assert np.array_equal(c0 & U64((1 << 28) - 1), quad) and np.array_equal(c0 >> U64(28), lane) and len(set(zip(lane.tolist(), quad.tolist()))) == 6
    e = i64_as_u64(env)
    for name, key in (("arrival_words", arrivals.ARR_KEY), ("intention_words", arrivals.INT_KEY)):
        got = call(P, name, [seed, epoch, env, lane, quad], U32, 4, n=len(seed))
        k0, k1 = (seed & U64(0xFFFFFFFF)) ^ U64(key[0]), (seed >> U64(32)) ^ U64(key[1])
        ref = np.stack(noise.philox4x32_10((c0, epoch, e & U64(0xFFFFFFFF), e >> U64(32)), (k0, k1)), axis=1).astype(U32)
        assert same(got, ref), (name, first_bad(got, ref))
    # against the stream model for an env / lane / row it can address: row 4 quad + k of lane 11 is word k
    got = call(P, "arrival_words", [u64([77]), np.array([3], U32), np.array([5], I64), np.array([11], I32), np.array([1], U32)], U32, 4, n=1)
    assert np.array_equal(got[0], arrivals.arrival_words(6, 9, 12, seed=77, epoch=3)[5, 4:8, 11])
    r = np.random.default_rng(405)
    rs = np.array([0, 31, 32, 127, 128, 255], I32)
    words = r.integers(0, 1 << 32, (64, 4), dtype=U64).astype(U32)
    words[0], words[1], words[2] = 0, 0xFFFFFFFF, [1, 1 << 31, 0x80000001, 0]
    wrep, rrep = np.repeat(words, len(rs), axis=0), np.tile(rs, len(words))
    bit = call(P, "intention_bit", [wrep, rrep], I32, n=len(rrep))
    want = [(int(wrep[q, (int(rr) >> 5) & 3]) >> (int(rr) & 31)) & 1 for q, rr in enumerate(rrep)]
    assert bit.tolist() == want


# ====================================================================================== replay
HALF_BITS_N = sorted(set([1, 2, 3, 4, 5, 499999, (1 << 31) - 1] + [(1 << k) + d for k in range(2, 31) for d in (-1, 0, 1)]))
PERM_ALL_N = sorted(set([n for n in HALF_BITS_N if n <= 4100] + [7, 320, 4100]))
PERM_SAMPLED_N = [n for n in HALF_BITS_N if n > 4100]
PERM_D = [0, 1, 1 << 32, (1 << 64) - 1]


def check_half_bits(P):
    N = np.array(HALF_BITS_N, U32)
    got = call(P, "replay_half_bits", [N], I32)
    assert got.tolist() == [replay.half_bits(n) for n in HALF_BITS_N]
    assert got[0] == 1 and got[-1] == 16 and all(4 ** int(h) >= n for h, n in zip(got, HALF_BITS_N))


@functools.lru_cache(None)
def perm_inputs():
    """(seed, d, N, j) and the NumPy model's answer: every j of the small domains, 2^12 sampled j (0 and N - 1 among them) of
    the large ones; seed and d walk through their named values from domain to domain"""
    r = np.random.default_rng(406)
    seed, d, N, j, ref = [], [], [], [], []
    for q, n in enumerate(PERM_ALL_N + PERM_SAMPLED_N):
        jj = np.arange(n, dtype=I64) if n <= 4100 else np.concatenate([[0, n - 1], r.integers(0, n, (1 << 12) - 2)])
        s, dd = SEEDS[q % 4], PERM_D[(q // 4) % 4]
        seed.append(u64([s] * len(jj))), d.append(u64([dd] * len(jj))), N.append(np.full(len(jj), n, U32)), j.append(jj.astype(U32))
        ref.append(replay.perm(s, dd, n, jj))
    return tuple(np.concatenate(x) for x in (seed, d, N, j, ref))


def check_perm(P):
    seed, d, N, j, ref = perm_inputs()
    got = call(P, "replay_perm", [seed, d, N, j], U32)
    assert np.array_equal(got.astype(I64), ref), first_bad(got.astype(I64), ref)
    for n in PERM_ALL_N:                                                 # a permutation of 0 .. N - 1
        assert np.array_equal(np.sort(got[N == n]), np.arange(n, dtype=U32)), n
    assert np.all(got < N)
    # the walk, step by step through replay_feistel: ends (the cycle through a value below N returns to one) where perm ends
    h = call(P, "replay_half_bits", [N], I32)
    x, steps, todo = j.copy(), np.zeros(len(j), I64), np.arange(len(j))
    while len(todo):
        assert steps.max() < 256
        x[todo] = call(P, "replay_feistel", [seed[todo], d[todo], h[todo], x[todo]], U32)
        steps[todo] += 1
        todo = todo[x[todo] >= N[todo]]
    assert np.array_equal(x, got)
    report(P, "replay_perm longest cycle walk (applications of replay_feistel)", int(steps.max()),
           "at N = %d; mean %.3f over %d (N, j)" % (int(N[np.argmax(steps)]), steps.mean(), len(j)))
    # what the entry point answers instead of a walk that need not end
    bad = call(P, "replay_perm", [u64([0, 0]), u64([0, 0]), np.array([5, 0], U32), np.array([5, 0], U32)], U32)
    assert bad.tolist() == [0xFFFFFFFF, 0xFFFFFFFF]


@functools.lru_cache(None)
def append_inputs():
    rows = []
    for cap in (1, 7, 320, 4100, 499999):
        for n_max in sorted({1, cap + 3, 3 * cap + 1, max(cap - 1, 1), cap}):
            for written in (0, cap - 1, cap, 1 << 40, (1 << 40) + 5):
                rows.append((written, 0, 0, n_max, cap))
                rows += [(written, 1, total, n_max, cap) for total in (-3, 0, n_max, n_max + 1)]
    assert any(r[0] % r[4] != 0 for r in rows) and any(r[3] > r[4] for r in rows)
    return [np.array([r[q] for r in rows], I32 if q == 1 else I64) for q in range(5)]


def check_append(P):
    written, has_total, total, n_max, cap = append_inputs()
    got = call(P, "replay_append_plan", [written, has_total, total, n_max, cap], I64, 3, n=len(cap))
    want, slots = [], []
    for q in range(len(cap)):
        w, c = int(written[q]), int(cap[q])
        n = replay.accepted(int(n_max[q]), int(total[q]) if has_total[q] else None)
        skip = max(n - c, 0)
        want.append((n, skip, (w + skip) % c))
        for qq in sorted({0, (n - skip) // 2, n - skip - 1} - {-1}):     # (no record accepted: no slot)
            slots.append(((w + skip) % c, c, qq, (w + skip + qq) % c))
    assert got.tolist() == [list(x) for x in want]
    s = np.array(slots, I64)
    assert np.all(s[:, 2] < s[:, 1]) and len(s) > 500
    assert np.array_equal(call(P, "replay_append_slot", [s[:, 0].copy(), s[:, 1].copy(), s[:, 2].copy()], I64), s[:, 3])
    skip, sl = replay.append_plan(4105, 4103, 4100)                     # the model's own statement of one wrapped append
    got1 = call(P, "replay_append_plan", [np.array([4105], I64), np.array([0], I32), np.array([0], I64), np.array([4103], I64), np.array([4100], I64)], I64, 3, n=1)[0]
    qs = np.arange(4103 - skip, dtype=I64)
    assert got1[1] == skip and np.array_equal(call(P, "replay_append_slot", [np.full_like(qs, got1[2]), np.full_like(qs, 4100), qs], I64), sl)
    none = call(P, "replay_append_plan", [np.zeros(1, I64), np.zeros(1, I32), np.zeros(1, I64), np.ones(1, I64), np.zeros(1, I64)], I64, 3, n=1)
    assert none.tolist() == [[-1, -1, -1]]                               # capacity 0: refused per element


# ====================================================================================== prio
INF_BITS = 0x7F800000
F32_OPERANDS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x00800001,
                         0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF,
                         0xFFFFFFFF, 0x7FA5A5A5, 0xFFA5A5A5, 0x3F800000, 0xBF800000, 0x3F800001, 0x40490FDB, 0x33800000], U32)


@functools.lru_cache(None)
def update_inputs():
    """(q, has_target, target): every pair of the operands with and without a target, then random pairs from normal(0, 3)
    and pairs one or a few ulps apart in the smallest binades (a subnormal difference)"""
    r = np.random.default_rng(407)
    a, b = np.meshgrid(F32_OPERANDS, F32_OPERANDS, indexing="ij")
    q, t = a.reshape(-1), b.reshape(-1)
    lowq = r.integers(0x00000001, 0x01800000, 2000, dtype=U64).astype(U32)
    lowt = lowq + r.integers(0, 5, 2000).astype(U32)
    rq, rt = r.normal(0, 3, 4000).astype(F32).view(U32), r.normal(0, 3, 4000).astype(F32).view(U32)
    q, t = np.concatenate([q, lowq, rq]), np.concatenate([t, lowt, rt])
    q, t = np.concatenate([q, q]), np.concatenate([t, t])
    has = np.concatenate([np.ones(len(q) // 2, I32), np.zeros(len(q) // 2, I32)])
    return q.view(F32), has, t.view(F32)


def check_prio_bits(P):
    q, has, t = update_inputs()
    got = call(P, "prio_update_bits", [q, has, t], U32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.abs(np.where(has != 0, q - t, q)).astype(F32)
    ref = p.view(U32).copy()
    ref[ref > INF_BITS] = INF_BITS                                      # the rule, by hand: above +inf's pattern is a NaN
    assert same(got, ref), first_bad(got, ref)
    with_t = has != 0
    sub = with_t & (ref > 0) & (ref < 0x00800000)
    assert np.count_nonzero(sub) > 1000 and np.count_nonzero(with_t & (ref == 0)) > 10      # subnormal differences, and exactly 0
    inf = np.float32(np.inf)
    assert np.all(got[with_t & (q == inf) & (t == inf)] == INF_BITS) and np.all(got[with_t & (q == -inf) & (t == -inf)] == INF_BITS)
    assert np.count_nonzero(np.isnan(q) & np.signbit(q)) > 100 and np.all(got[np.isnan(q)] == INF_BITS) and got.max() == INF_BITS
    for tgt in (None, t[: len(t) // 2]):                                # and the model's statement of the same rule
        half = slice(0, len(q) // 2) if tgt is not None else slice(len(q) // 2, None)
        assert np.array_equal(got[half], replay.prio_update_bits(q[half], tgt))
    b = np.concatenate([F32_OPERANDS, ref[:4096]])
    b, valid = np.concatenate([b, b]), np.concatenate([np.ones(len(b), I32), np.zeros(len(b), I32)])
    key = call(P, "prio_key", [valid, b], U32)
    assert np.array_equal(key, ~np.where(valid != 0, b, U32(INF_BITS)).astype(U32))
    assert np.all(key[valid == 0] == U32(0x807FFFFF))


def check_prio_slot(P):
    rows = []
    for written, cap in ((0, 8), (5, 8), (8, 8), (20, 8), (4100, 4100), (4099, 4100), (123457, 4100), ((1 << 40) + 3, 499999)):
        L = min(written, cap)
        rows += [(w, written, cap) for w in (-1, written - L - 1, written - L, written - 1, written, written + 5)]
    w, written, cap = (np.array([r[q] for r in rows], I64) for q in range(3))
    got = call(P, "prio_update_slot", [w, written, cap], I64)
    want = [(ww % c if wr - min(wr, c) <= ww < wr else -1) for ww, wr, c in rows]
    assert got.tolist() == want
    assert np.count_nonzero(got >= 0) >= 12 and np.count_nonzero(got < 0) >= 24


@functools.lru_cache(None)
def prio_models():
    return [replay.PrioritizedReplayModel(buffer_size=size, batch_size=batch, learn_start=batch) for size, batch in ((320, 8), (4096, 128))]


def check_prio_partition(P):
    for m in prio_models():
        pf = np.ascontiguousarray(m.part_from, I64)
        L = np.concatenate([pf, pf - 1, [0, 1, m.capacity, m.capacity + 1, 1 << 40]]).astype(I64)
        got = call(P, "prio_partition", [pf, L], I32, n=len(L))
        want = [int(np.count_nonzero(pf <= x)) for x in L]
        assert got.tolist() == want and sorted(set(want)) == list(range(33))


@functools.lru_cache(None)
def draw_inputs():
    """[(ends table, seed, d, L per element, bsz)]: the hand-made rows (8 strata) under every (seed, d, L), then the models' tables"""
    base = [[0, 10, 20, 30, 40, 50, 60, 70, 80],        # e0 < e1
            [0, 1, 2, 3, 4, 5, 6, 7, 8],                # e0 == e1: strata of one rank
            [0, 5, 5, 5, 9, 9, 9, 9, 9],                # e0 > e1: the swapped pair
            [0, 0, 0, 0, 0, 0, 0, 0, 0],                # lo = 0: the r < 1 clamp
            [0, 1, 1, 40, 41, 41, 80, 80, 81]]          # all three kinds in one row
    rows, seed, d, L = [], [], [], []
    for row, s, dd, ll in itertools.product(base, SEEDS, PERM_D + [7, 12345], [81, 3, 1, 1 << 40]):   # (L = 3, 1: the r > L clamp)
        rows.append(row), seed.append(s), d.append(dd), L.append(ll)
    out = [(np.array(rows, I32), u64(seed), u64(d), np.array(L, I64), 8)]
    for m in prio_models():
        reps = 4
        out.append((np.tile(m.ends, (reps, 1)), u64(np.repeat(SEEDS[:reps], 32)), u64(np.repeat(PERM_D[:reps], 32)),
                    np.full(32 * reps, m.capacity, I64), m.batch_size))
    return out


def draw_call(P, case):
    ends, seed, d, L, bsz = case
    return call(P, "prio_draw_rank", [ends, np.repeat(seed, bsz), np.repeat(d, bsz), np.repeat(L, bsz)], I32, k=(bsz, len(ends)),
                n=len(ends) * bsz).reshape(len(ends), bsz)


def check_prio_draw(P):
    for q, case in enumerate(draw_inputs()):
        ends, seed, d, L, bsz = case
        got = draw_call(P, case)
        for row in range(len(ends)):
            want = replay.prio_draw_ranks(int(seed[row]), [int(d[row])], ends[row], int(L[row]))[0]
            assert np.array_equal(got[row], want), (q, row, got[row], want)
        if q == 0:
            lo, hi = np.minimum(ends[:, :-1] + 1, ends[:, 1:]), np.maximum(ends[:, :-1] + 1, ends[:, 1:])
            free = L[:, None] >= hi                                      # no clamp at work: the rank lies in its stratum
            assert np.all((got >= np.maximum(lo, 1))[free]) and np.all((got <= hi)[free])
            assert np.all(got >= 1) and np.all(got <= L[:, None]) and np.count_nonzero(got == L[:, None]) > 100
            swapped = np.broadcast_to((ends[:, :-1] + 1 > ends[:, 1:]), got.shape) & free
            assert len(set(got[swapped].tolist())) > 2                   # the swapped strata draw both of their ranks
    assert P.raw("prio_draw_rank", [np.zeros(9, I32), u64([0] * 9), u64([0] * 9), np.ones(9, I64)], [(I32, 9)], k=(8, 1), n=9)[0] == -1
    assert P.raw("prio_draw_rank", [np.zeros(9, I32), u64([0] * 8), u64([0] * 8), np.ones(8, I64)], [(I32, 8)], k=(0, 1), n=8)[0] == -1


# alpha * beta as float32: the ends of what _PrioConfig._alpha_beta accepts (0 and the largest finite float32; the smallest
# subnormal beside 0), the values a rank-based memory uses (alpha 0.7 times beta from beta_zero = 0.5 to 1; 0.42 of the
# existing tests; alpha = beta = 1) and 2.  Between 2 and the upper end the float32 quotient rank / rank_max, off by 2^-24
# relative, is raised to a power that multiplies that error by alpha_beta: the stated arithmetic itself leaves the bar there,
# so no such value is listed; at the upper end every weight is 0 or 1.
ALPHA_BETA = np.array([0.0, 1e-45, 0.35, 0.42, 0.7, 1.0, 2.0, 3.4028234663852886e38], F32)


@functools.lru_cache(None)
def weight_inputs():
    rank, rmax, ab = [], [], []
    for m, x in itertools.product([2, 320, 500000], ALPHA_BETA):
        rs = sorted({1, 2, m - 1, m})
        rank += rs
        rmax += [m] * len(rs)
        ab += [x] * len(rs)
    return np.array(rank, I32), np.array(rmax, I32), np.array(ab, F32)


def check_prio_weight(P):
    """Against the float64 expression: |w - w64| <= WEIGHT_BAR w64 + 2^-149.  The second term is one step of the float32
    subnormal grid, which is all a float32 result can resolve where w64 lies below the normal range (alpha_beta = 2 with rank
    1 of 500 000 does not get there: 4e-12; the upper end of alpha_beta does, with w64 = 0)."""
    rank, rmax, ab = weight_inputs()
    got = call(P, "prio_weight", [rank, rmax, ab], F32)
    worst = 0.0
    for x in ALPHA_BETA:
        m = ab == x
        w64 = replay.prio_weights(np.stack([rank[m], rmax[m]], axis=-1), x)[:, 0]
        g = got[m].astype(F64)
        assert np.all(np.abs(g - w64) <= WEIGHT_BAR * w64 + 2.0 ** -149), (float(x), g, w64)
        ok = w64 >= 2.0 ** -126
        worst = max(worst, float(np.max(np.abs(g[ok] / w64[ok] - 1))))
    report(P, "prio_weight max rel vs float64 (bar 1e-5)", worst, "%d (rank, rank_max, alpha_beta)" % len(rank))
    assert worst <= WEIGHT_BAR
    assert np.all(got[rank == rmax] == np.float32(1.0)) and np.all(got[ab == 0] == np.float32(1.0))
    assert np.all((got >= 0) & (got <= 1))


# ====================================================================================== device build == host build, bit for bit
def check_bit_equal(dev, host):
    """Every entry point of this file except prio_weight (powf: libm against ocml): the hipcc build on the device returns, bit
    for bit, what the g++ build returns -- on the inputs of the checks above and on the dense sweeps, which only the two
    builds run in full."""
    def eq(name, ins, dtype, width=1, k=(), n=None):
        a, b = call(dev, name, ins, dtype, width, k, n), call(host, name, ins, dtype, width, k, n)
        assert same(a, b), (name, first_bad(a, b))

    c, k = philox_inputs()
    eq("philox4x32_10", [c, k], U32, 4, n=len(c))
    for w0, w1 in [gauss_edge_pairs()] + gauss_sweep_pairs():
        eq("noise_gauss", [w0, w1], F64)
    for w in (radius_words(),) + gauss_sweep_pairs()[0] + gauss_sweep_pairs()[1]:
        eq("arrival_exp", [w], F64)
    seed, env, vid, tick, a, sigma = action_inputs()
    eq("action_noise_z", [seed, env, vid, tick], F64)
    eq("action_with_noise", [a, sigma, seed, env, vid, tick], F64)
    eq("arrival_gap", list(gap_inputs()), F64)
    s0 = subset18(gauss_sweep_pairs()[0][0])
    eq("arrival_gap", [s0, np.full(len(s0), 3.27), np.full(len(s0), 1.0)], F64)
    eq("arrival_words", list(words_inputs()), U32, 4, n=len(words_inputs()[0]))
    eq("intention_words", list(words_inputs()), U32, 4, n=len(words_inputs()[0]))
    r = np.random.default_rng(408)
    words, rr = r.integers(0, 1 << 32, (4096, 4), dtype=U64).astype(U32), r.integers(0, 256, 4096).astype(I32)
    eq("intention_bit", [words, rr], I32, n=4096)
    eq("replay_half_bits", [np.array(HALF_BITS_N, U32)], I32)
    seed, d, N, j, _ = perm_inputs()
    eq("replay_perm", [seed, d, N, j], U32)
    eq("replay_feistel", [seed, d, np.array([replay.half_bits(int(n)) for n in N], I32), j], U32)
    eq("replay_append_plan", append_inputs(), I64, 3, n=len(append_inputs()[0]))
    written, _, _, n_max, cap = append_inputs()
    eq("replay_append_slot", [written % cap, cap, np.minimum(n_max, cap) - 1], I64)
    q, has, t = update_inputs()
    eq("prio_update_bits", [q, has, t], U32)
    eq("prio_key", [has, q.view(U32)], U32)
    for m in prio_models():
        pf = np.ascontiguousarray(m.part_from, I64)
        L = np.concatenate([pf, pf - 1, np.arange(0, m.capacity + 2)]).astype(I64)
        eq("prio_partition", [pf, L], I32, n=len(L))
    for case in draw_inputs():
        assert np.array_equal(draw_call(dev, case), draw_call(host, case))
    w = r.integers(-2, 5000, 4096)
    eq("prio_update_slot", [w, np.full(4096, 4600, I64), np.full(4096, 4100, I64)], I64)

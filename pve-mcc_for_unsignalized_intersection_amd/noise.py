"""NumPy restatement of csrc/pve_noise.h: the exploration noise the device actor adds to a controlled vehicle's action
(`BatchedIntersections.set_exploration`).  The header specifies the deviate as exact float64 arithmetic in a fixed order, so
this module is bit-equal to the kernels: a roll-out can be replayed, and an oracle driven, with the very numbers the device drew.

    a_cmd(env, vehicle, tick) = float64(actor_f32(row)) + sigma * action_noise(seed, env_global, vehicle_id, tick)

Key layout (include/pve_env.h): Philox4x32-10, counter = (vehicle_id, tick mod 2^32, env_global low, env_global high),
key = (seed low, seed high); the deviate uses output words 0 and 1."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
# 1 / (2j + 1), j = 8 .. 0; 1 / (2j)! and 1 / (2j + 1)! with alternating signs, j = 7 .. 0 (correctly rounded quotients)
_LOG_C = [1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0, 1.0]
_COS_C = [-1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -1.0 / 2.0, 1.0]
_SIN_C = [-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0,
          -1.0 / 6.0, 1.0]
_SQRT_HALF = 0.70710678118654757
_LN2 = 0.69314718055994529
_X_SCALE = 1.5707963267948966 / 2147483648.0


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123).  counter: four broadcastable arrays of 32-bit words, key: two -> four uint64
    arrays holding the 32-bit output words."""
    c = [np.asarray(x, np.uint64) & _MASK32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(x, np.uint64) & _MASK32 for x in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK32]
        k0 = (k0 + np.uint64(W0)) & _MASK32
        k1 = (k1 + np.uint64(W1)) & _MASK32
    return c


def gauss_from_words(w0, w1):
    """The standard normal deviate of two 32-bit words: pve_noise.h's noise_gauss, operation for operation."""
    w0 = np.asarray(w0, np.uint64) & _MASK32
    w1 = np.asarray(w1, np.uint64) & _MASK32
    # radius
    m = (w0 * np.uint64(2) + np.uint64(1)).astype(np.float64)          # exact: < 2^33
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
    radius = np.sqrt((2 * (33 - e)).astype(np.float64) * _LN2 - 4.0 * (s * L))
    # angle
    n = w1 * np.uint64(2) + np.uint64(1)
    q = (n >> np.uint64(31)).astype(np.int64)
    k = (n & np.uint64(0x7FFFFFFF)).astype(np.int64)
    swap = k > (1 << 30)
    k = np.where(swap, (1 << 31) - k, k)
    x = k.astype(np.float64) * _X_SCALE
    x2 = x * x
    use_sin = ((q & 1) != 0) != swap
    P = np.where(use_sin, _SIN_C[0], _COS_C[0])
    for cs_, cc_ in zip(_SIN_C[1:-1], _COS_C[1:-1]):
        P = P * x2 + np.where(use_sin, cs_, cc_)
    P = P * x2 + 1.0
    cs = np.where(use_sin, x * P, P)
    cs = np.where((q == 1) | (q == 2), -cs, cs)
    return radius * cs


def action_noise(seed, env_global, vehicle_ids, tick):
    """z(seed, env_global, vehicle_id, tick) as float64; env_global, vehicle_ids and tick broadcast against each other.
    env_global = env index in the batch + the batch's env_offset; tick = ticks since reset() when the action is applied."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    env = np.asarray(env_global, np.int64).astype(np.uint64)
    ids = np.asarray(vehicle_ids, np.int64).astype(np.uint64)
    tk = np.asarray(tick, np.int64).astype(np.uint64)
    w = philox4x32_10((ids, tk, env & _MASK32, env >> _S32), (seed & 0xFFFFFFFF, seed >> 32))
    return gauss_from_words(w[0], w[1])

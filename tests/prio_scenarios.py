"""Inputs shared by tests/test_prio_replay.py and tests/test_gpu_prio_replay.py: priority patterns as float32 bit patterns,
memories brought to a given number of live records, and the update lists with duplicates, stale ids and -1."""
import numpy as np

from tests.replay_scenarios import bits32, payload  # noqa: F401  (records whose every word is recognisable)

INF_BITS = 0x7F800000
PATTERNS = ("all_new", "all_equal", "distinct", "digits", "half_new")
LIVE_COUNTS = (1, 63, 64, 65, 257, 4097, 70001)              # the last: more than one tile of 2048 keys per digit pass, 35 histogram blocks
WEIGHT_BAR = 1e-5                                            # relative, against the float64 expression (the exponent of a float32
#                                                              exp2(ab * log2(x)) is off by at most 19 * 2^-23 * a few for ranks to 500 000)


def digit_bits():
    """Bit patterns of non-negative float32 with one key per value of each of the four digit positions of the radix sort, and the
    corner values: zeros, denormals, 1e-30 .. 1e30, the largest finite, +inf"""
    v = np.arange(256, dtype=np.uint32)
    parts = [v[:128] << np.uint32(24), np.uint32(0x3F000000) | (v << np.uint32(16)), np.uint32(0x3F800000) | (v << np.uint32(8)),
             np.uint32(0x3F800000) | v, np.array([0, 1, 2, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, INF_BITS], np.uint32),
             np.logspace(-30, 30, 61).astype(np.float32).view(np.uint32)]
    out = np.unique(np.concatenate(parts))
    assert out.max() == INF_BITS and all(len(np.unique((out >> np.uint32(s)) & np.uint32(255))) >= 128 for s in (0, 8, 16, 24))
    return out


def pattern_update(pattern, seq, rng):
    """(ids, q float32) of the update that gives the live records `seq` the pattern (|q| is stored: q's bits are the priority's)"""
    n = len(seq)
    if pattern == "all_new":
        return seq[:0], np.zeros(0, np.float32)
    if pattern == "all_equal":
        return seq, np.full(n, 0.75, np.float32)
    if pattern == "distinct":
        return seq, (np.uint32(0x3A000000) + rng.permutation(np.arange(1, n + 1)).astype(np.uint32)).view(np.float32)
    if pattern == "digits":
        d = digit_bits()                                   # (more records than patterns: drawn with repeats, i.e. with ties)
        pick = rng.integers(0, len(d), n) if n > len(d) else rng.permutation(len(d))[:n]
        return seq, d[pick].view(np.float32)
    if pattern == "half_new":
        pick = np.sort(rng.permutation(n)[:n // 2])
        return seq[pick], rng.permutation(np.arange(1, len(pick) + 1)).astype(np.float32)
    raise KeyError(pattern)


def geometry(L):
    """(capacity, written) that leaves L live records: below 64 an unwrapped memory of 64, from 64 on a full memory whose
    capacity does not divide the adds"""
    return (64, L) if L < 64 else (L, L + L // 3 + 1)


def messy_update(written, L, n, rng):
    """n ids around the live range [written - L, written): live ones (with duplicates), overwritten ones, ids not yet written, -1;
    q and target with NaN, infinities, zeros and equal pairs"""
    seq = rng.integers(written - L - max(L // 8, 3), written + 5, n).astype(np.int64)
    seq[rng.integers(0, n, max(n // 16, 1))] = -1
    dup = rng.integers(0, n, n // 4)
    seq[dup] = seq[rng.integers(0, n, n // 4)]
    q = rng.normal(0, 3, n).astype(np.float32)
    target = rng.normal(0, 3, n).astype(np.float32)
    q[::17] = np.nan
    target[5::29] = np.inf
    q[5::58] = np.inf                                      # (inf - inf: NaN, stored as +inf)
    q[3::31] = target[3::31]                               # (a zero priority)
    return seq, q, target

"""Inputs shared by tests/test_replay.py and tests/test_gpu_replay.py: records whose every 32-bit word is recognisable, and the
chunk lists of the append tests."""
import numpy as np

RECORD = 36
SEEDS = (1, 2, 3)
# 0.999 quantiles of chi-square with 999, 4031 and 9899 degrees of freedom (the bars of the uniformity tests)
CHI2_999, CHI2_4031, CHI2_9899 = 1143.0, 4312.0, 10337.0


def payload_of(numbers):
    """The records with the given record numbers, float32 [n, 36].  The words are a bijection of (record number, column): word =
    (number * 36 + column) * an odd constant mod 2^32, so every 16-byte piece of every record differs from every other and a
    misplaced piece shows.  Sprinkled over them: NaNs with payload bits (column 0 of every 5th record, column 35 of every 11th),
    -0.0 (column 29 of every 7th), denormals (column 3 of every 3rd).  Compare as uint32: a NaN never equals itself as a float."""
    num = np.asarray(numbers, np.int64).ravel()
    idx = num.astype(np.uint64)[:, None] * np.uint64(RECORD) + np.arange(RECORD, dtype=np.uint64)[None, :]
    w = ((idx * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    w[num % 5 == 0, 0] = 0x7FC00000 | (w[num % 5 == 0, 0] & 0x003FFFFF)
    w[num % 11 == 0, 35] = 0xFF800001 | (w[num % 11 == 0, 35] & 0x007FFFFE)
    w[num % 7 == 0, 29] = 0x80000000
    w[num % 3 == 0, 3] = (w[num % 3 == 0, 3] & 0x807FFFFF) | 1
    return w.view(np.float32)


def payload(n, first=0):
    """n consecutive records, numbers first .. first + n - 1"""
    return payload_of(np.arange(first, first + n))


def bits32(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def append_chunks(capacity):
    """chunk lengths of the append tests: 1; capacity - 1; capacity; capacity + 1; 3 * capacity + 5; 0; and a wrap in mid-chunk"""
    return [1, capacity - 1, capacity, capacity + 1, 3 * capacity + 5, 0, capacity // 2 + 1, capacity // 2 + 2]


def pearson(counts):
    counts = np.asarray(counts, np.float64)
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())

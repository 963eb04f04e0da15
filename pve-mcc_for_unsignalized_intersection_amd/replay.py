"""The uniform replay memory (csrc/pve_replay.h; reference replay_buffer.py:45-53 `add`, :20-23 `getBatch` with rand_s = True,
main.py:263 and main.py:50-77): a ring of the 36-float records nstep_transitions() emits and minibatch draws from it without
replacement, kept on the device between nstep_transitions() and critic_q().

`ReplayMemory` is the device memory (pve_replay_reset / pve_replay_append / pve_replay_sample), `ReplayModel` the same thing on
NumPy arrays: the host statement of the specification, bit-equal to the kernels and to a g++ build of the header.  Nothing here
does floating-point arithmetic; records are compared as bit patterns.

Ring: record number w (0-based over all adds) lives in slot w mod capacity; the live records are the last
L = min(written, capacity); age index a in [0, L) names record written - L + a (0 = the oldest, the deque's left end).
Draw: minibatch number d (draws, draws + 1, ..) takes the age indices perm(seed, d, L)(j), j = 0 .. batch_size - 1.  The
reference's Mersenne-Twister draw (random.sample) is not reproduced; like the exploration noise the draw is this library's own."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import PveError, check
from .noise import philox4x32_10

RECORD = 36
ROUNDS = 8
TAG0, TAG1 = 0x5245504C, 0x41594D45          # REPLAY_TAG0 / REPLAY_TAG1: xored into the Philox key (include/pve_env.h)
WRITTEN, DRAWS, STATUS = 0, 1, 2             # words of the state block


def half_bits(N):
    """h: bits of one Feistel half for a domain of N values (bit length of N - 1, at least 2, rounded up to even, halved)"""
    b = max((int(N) - 1).bit_length(), 2)
    return (b + 1) // 2


def _feistel(seed, d, h, x):
    mask = np.uint64((1 << h) - 1)
    hh = np.uint64(h)
    L, R = x >> hh, x & mask
    key = ((seed & 0xFFFFFFFF) ^ TAG0, (seed >> 32) ^ TAG1)
    for r in range(ROUNDS):
        w = philox4x32_10((R, np.uint64(r), d & np.uint64(0xFFFFFFFF), d >> np.uint64(32)), key)
        L, R = R, L ^ (w[0] & mask)
    return (L << hh) | R


def perm(seed, d, N, j=None):
    """perm(seed, d, N)(j): a bijection of [0, N), 1 <= N <= 2^31 - 1.  d and j broadcast against each other (j=None: the whole
    range, one row per d); returns int64."""
    N = int(N)
    if not 1 <= N <= 0x7FFFFFFF:
        raise ValueError("N must be 1 .. 2^31 - 1")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d = np.asarray(d, np.uint64) if not isinstance(d, int) else np.asarray(d & 0xFFFFFFFFFFFFFFFF, np.uint64)
    if j is None:
        d, j = d[..., None], np.arange(N, dtype=np.uint64)
    j = np.asarray(j, np.int64)
    if j.size and (j.min() < 0 or j.max() >= N):
        raise ValueError("j must lie in [0, N)")
    d, x = np.broadcast_arrays(d, j.astype(np.uint64))
    shape = x.shape
    d, x = d.ravel(), x.ravel().copy()
    h = half_bits(N)
    todo = np.arange(x.size)
    while todo.size:                                   # the cycle walk: re-apply where the value is still >= N
        x[todo] = _feistel(seed, d[todo], h, x[todo])
        todo = todo[x[todo] >= np.uint64(N)]
    return x.astype(np.int64).reshape(shape)


def append_plan(written, n, capacity):
    """(skip, slots): an append of n records drops the first skip = max(n - capacity, 0) and stores input record skip + q in
    slots[q] (replay_append_plan / replay_append_slot of the header)"""
    skip = max(n - capacity, 0)
    start = (written + skip) % capacity
    s = start + np.arange(n - skip, dtype=np.int64)
    return skip, np.where(s >= capacity, s - capacity, s)


def accepted(n_max, total=None):
    """records one append takes: n_max, or min(total, n_max) with a device-style count (negative counts as 0)"""
    return int(n_max) if total is None else min(max(int(total), 0), int(n_max))


class ReplayModel:
    """The replay memory on NumPy arrays: same methods and same results as ReplayMemory.  capacity = buffer_size - 1, as the
    reference's deque (replay_buffer.py:47-49 increments num_experiences before the `<` test)."""

    def __init__(self, buffer_size=500000, batch_size=128, seed=0):
        self.capacity, self.batch_size, self.seed = int(buffer_size) - 1, int(batch_size), int(seed) & 0xFFFFFFFFFFFFFFFF
        if not 1 <= self.capacity <= 0x7FFFFFFF or not 1 <= self.batch_size <= self.capacity:
            raise ValueError("need 1 <= batch_size <= buffer_size - 1 <= 2^31 - 1")
        self.store = np.zeros((self.capacity, RECORD), np.float32)
        self.reset()

    def reset(self):
        self.written = self.draws = self.status = 0

    def count(self):
        return self.written

    def live(self):
        return min(self.written, self.capacity)

    def perm(self, d, N, j=None):
        return perm(self.seed, d, N, j)

    def add(self, records, total=None):
        """records float32 [n_max, 36]; total: the count of a device-style cut-off (None: all of them)"""
        rec = np.ascontiguousarray(records, np.float32).reshape(-1, RECORD).view(np.uint32)
        n = accepted(len(rec), total)
        skip, slots = append_plan(self.written, n, self.capacity)
        self.store.view(np.uint32)[slots] = rec[skip:n]
        self.written += n

    def live_seq(self):
        L = self.live()
        return self.written - L + np.arange(L, dtype=np.int64)

    def live_records(self):
        """the live records in age order (oldest first): list(deque) of the reference"""
        return self.store[self.live_seq() % self.capacity]

    def sample(self, n_batches=1, check=True):
        """-> (rows [n_batches, batch, 28], act7 [.., 7], target [..], seq int64 [..])"""
        n_batches = int(n_batches)
        if n_batches < 1:
            raise ValueError("n_batches must be >= 1")
        L, B = self.live(), self.batch_size
        self.status = L
        if L < B:
            if check:
                raise PveError("replay memory: %d live records, fewer than batch_size = %d" % (L, B))
            return (np.zeros((n_batches, B, 28), np.float32), np.zeros((n_batches, B, 7), np.float32),
                    np.zeros((n_batches, B), np.float32), np.full((n_batches, B), -1, np.int64))
        d = self.draws + np.arange(n_batches, dtype=np.uint64)[:, None]
        age = perm(self.seed, d, L, np.arange(B)[None, :]).reshape(n_batches, B)
        seq = self.written - L + age
        rec = self.store[seq % self.capacity]
        self.draws += n_batches
        return rec[..., :28].copy(), rec[..., 28:35].copy(), rec[..., 35].copy(), seq


class ReplayMemory:
    """The replay memory on the device of `batch` (a BatchedIntersections): ring and state are allocated there, every call runs
    on the batch's handle and stream, asynchronously.  capacity = buffer_size - 1: the reference's
    ReplayBuffer(500000, ...) holds 499 999 transitions, because `add` increments num_experiences before its `<` test
    (replay_buffer.py:47-49).  With a PipelinedIntersections, bind the memory to ONE sub-batch (`pipe.subs[k]`): its add() and
    sample() are ordered on that sub-batch's stream, and records of the other sub-batches (device tensors) may be added through
    it once their streams are joined -- no fan-out over the sub-batches is needed.
    Sampled rows are float32: critic_q() of a batch created with obs_dtype=torch.float32 takes them without a copy."""

    def __init__(self, batch, buffer_size=500000, batch_size=128, seed=0, block_threads=0):
        import torch
        self._torch = torch
        self.batch = batch
        self.capacity, self.batch_size, self.seed = int(buffer_size) - 1, int(batch_size), int(seed) & 0xFFFFFFFFFFFFFFFF
        if not 1 <= self.capacity <= 0x7FFFFFFF or not 1 <= self.batch_size <= self.capacity:
            raise PveError("ReplayMemory: need 1 <= batch_size <= buffer_size - 1 <= 2^31 - 1")
        with batch._own_stream():
            self.store = torch.zeros(self.capacity, RECORD, dtype=torch.float32, device=batch.device)
            self.state = torch.zeros(_capi.REPLAY_STATE_WORDS, dtype=torch.int64, device=batch.device)
        self._rp = _capi.PveReplay()
        self._rp.capacity, self._rp.store, self._rp.state = self.capacity, self.store.data_ptr(), self.state.data_ptr()
        self._rp.seed, self._rp.block_threads = self.seed, int(block_threads)

    def _call(self, fn, what, *args):
        b = self.batch
        b._bind_stream()
        check(b.lib, fn(b._h, C.byref(self._rp), *args), what)

    def reset(self):
        with self.batch._own_stream():
            self._call(self.batch.lib.pve_replay_reset, "pve_replay_reset")

    def add(self, records, total=None):
        """Append records (float32 device tensor [n_max, 36], the output of nstep_transitions()) in order.  total: the 0-dim
        int64 device tensor nstep_transitions(max_records=...) returns -- the first min(total, n_max) records are appended, with
        no synchronisation -- or None for all n_max."""
        torch = self._torch
        b = self.batch
        if not torch.is_tensor(records) or records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != RECORD:
            raise PveError("ReplayMemory.add: records must be a float32 device tensor [n, 36]")
        if records.device != self.store.device:              # (the full device: another GPU's pointer must not reach this launch)
            raise PveError("ReplayMemory.add: records are on %s, the memory is on %s" % (records.device, self.store.device))
        with b._own_stream():
            records = records.contiguous()
            if total is not None:
                if not torch.is_tensor(total):
                    total = torch.as_tensor(int(total), dtype=torch.int64)
                total = total.to(device=b.device, dtype=torch.int64).reshape(1)
            self._call(b.lib.pve_replay_append, "pve_replay_append", C.c_void_p(records.data_ptr()),
                       C.c_void_p(total.data_ptr() if total is not None else 0), int(records.shape[0]))

    def sample(self, n_batches=1, check=True):
        """Draw n_batches minibatches of batch_size distinct live records -> (rows float32 [n_batches, batch_size, 28], act7
        float32 [.., 7], target float32 [..], seq int64 [..] = the record numbers), device tensors in the layout
        critic_q(rows, act7) takes.  check=True reads the status word once (one synchronisation) and raises PveError when
        fewer than batch_size records are live (the reference's ValueError); check=False never synchronises: a short memory
        then gives seq = -1 and zeros."""
        torch = self._torch
        b, n, B = self.batch, int(n_batches), self.batch_size
        if n < 1:
            raise PveError("ReplayMemory.sample: n_batches must be >= 1")
        with b._own_stream():
            rows = torch.empty(n, B, 28, dtype=torch.float32, device=b.device)
            act7 = torch.empty(n, B, 7, dtype=torch.float32, device=b.device)
            target = torch.empty(n, B, dtype=torch.float32, device=b.device)
            seq = torch.empty(n, B, dtype=torch.int64, device=b.device)
            self._call(b.lib.pve_replay_sample, "pve_replay_sample", B, n, C.c_void_p(rows.data_ptr()), C.c_void_p(act7.data_ptr()),
                       C.c_void_p(target.data_ptr()), C.c_void_p(seq.data_ptr()))
            if check:
                L = int(self.state[STATUS].item())
                if L < B:
                    raise PveError("replay memory: %d live records, fewer than batch_size = %d" % (L, B))
        return rows, act7, target, seq

    def count(self):
        """adds ever made (the reference's count()); synchronises"""
        with self.batch._own_stream():
            return int(self.state[WRITTEN].item())

    def live(self):
        return min(self.count(), self.capacity)

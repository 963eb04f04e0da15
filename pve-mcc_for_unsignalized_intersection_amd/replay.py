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
import numpy as np

from . import _capi
from ._capi import PveError
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

    def reset(self):
        with self.batch._own_stream():
            self.batch._call("pve_replay_reset", self._rp)

    def add(self, records, total=None):
        """Append records (float32 device tensor [n_max, 36], the output of nstep_transitions()) in order.  total: the 0-dim
        int64 device tensor nstep_transitions(max_records=...) returns -- the first min(total, n_max) records are appended, with
        no synchronisation -- or None for all n_max."""
        from ._args import is_tensor_of
        torch = self._torch
        b = self.batch
        if not is_tensor_of(records, torch.float32) or records.dim() != 2 or records.shape[1] != RECORD:
            raise PveError("ReplayMemory.add: records must be a float32 device tensor [n, 36]")
        if records.device != self.store.device:              # (the full device: another GPU's pointer must not reach this launch)
            raise PveError("ReplayMemory.add: records are on %s, the memory is on %s" % (records.device, self.store.device))
        with b._own_stream():
            records = records.contiguous()
            if total is not None:
                if not torch.is_tensor(total):
                    total = torch.as_tensor(int(total), dtype=torch.int64)
                total = total.to(device=b.device, dtype=torch.int64).reshape(1)
            b._call("pve_replay_append", self._rp, records, total, int(records.shape[0]))

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
            b._call("pve_replay_sample", self._rp, B, n, rows, act7, target, seq)
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


# ---------------------------------------------------------------------------------------------------------------------------
# The rank-based prioritised memory (csrc/pve_prio.h; reference rank_based.py `Experience`, which replay_buffer.py:13-18 builds in
# every run and getBatch draws from with rand_s = False; main.py:76-79 td_error / update_priority).  PrioritizedReplayModel is the
# host statement of the specification, PrioritizedReplayMemory the device memory (pve_prio_reset / _rank / _sample / _update).
# Every integer part is bit-exact; the only floating-point arithmetic is the update's one subtraction and the importance weight.
# Two stated departures from the reference: records of EQUAL priority are ordered by record number, newest first (the reference's
# order among ties follows its heap layout), and an update that names a record overwritten since is ignored (the reference would
# write onto the slot's new occupant).
PRIO_PARTS = 32
PRIO_NEW_BITS = 0x7F800000                   # +inf: a record that was never updated
PRIO_TAG0, PRIO_TAG1 = 0x5052494F, 0x52414E4B      # "PRIO", "RANK": xored into the Philox key of the stratified draw
PDRAWS, PLIVE, PPART, PIGNORED = 0, 1, 2, 3  # words of pstate
_UNUSED_THRESHOLD = 1 << 62


def strata_tables(size, batch_size, alpha=0.7, partition_num=PRIO_PARTS):
    """(part_from int64 [32], ends int32 [32, batch_size + 1]): rank_based.py:40-80 and :159-163 restated with math.pow evaluated
    once for all prefixes.  part_from[k] = the smallest L with floor(1.0 * L / size * partition_num) >= k + 1, by that float
    expression; row k of ends is strata_ends of partition k + 1 (n = (k + 1) * floor(size / partition_num) ranks): math.fsum of the
    prefix, np.cumsum(pdf / sum), the walk `while cdf[index] < step` with ends[0] = 0 and ends[batch_size] = n.  Rows and
    thresholds past partition_num (< 32) are never reached: threshold 2^62, the last row repeated."""
    import math
    size, B, P = int(size), int(batch_size), int(partition_num)
    if not 1 <= P <= PRIO_PARTS or size < P or B < 1:
        raise ValueError("need 1 <= partition_num <= 32 <= ... <= size and batch_size >= 1")
    psize = int(math.floor(1.0 * size / P))
    if B > psize:
        raise ValueError("batch_size %d exceeds the first partition's %d ranks" % (B, psize))
    dist = np.floor(1.0 * np.arange(1, size + 1, dtype=np.float64) / size * P)           # dist_index of L = 1 .. size
    part_from = np.full(PRIO_PARTS, _UNUSED_THRESHOLD, np.int64)
    part_from[:P] = 1 + np.searchsorted(dist, np.arange(1, P + 1, dtype=np.float64), side="left")
    powers = [math.pow(x, -alpha) for x in range(1, P * psize + 1)]
    powers_np = np.array(powers, np.float64)
    ends = np.zeros((PRIO_PARTS, B + 1), np.int32)
    for k in range(P):
        n = (k + 1) * psize
        cdf = np.cumsum(powers_np[:n] / math.fsum(powers[:n]))
        ends[k, B] = n
        step, index = 1.0 / B, 1
        for s in range(1, B):
            index = max(index, int(np.searchsorted(cdf, step, side="left")))       # while cdf[index] < step: index += 1
            if index >= n:
                raise ValueError("strata walk ran past the partition (the reference raises IndexError)")
            ends[k, s] = index
            step += 1.0 / B
        if part_from[k] < n:
            raise ValueError("partition %d is reached with fewer live records than its %d ranks" % (k + 1, n))
    ends[P:] = ends[P - 1]
    return part_from, ends


def prio_draw_ranks(seed, d, ends_row, L):
    """ranks int64 [len(d), batch] of minibatches d from one table row (prio_draw_rank of the header)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d = np.asarray(d, np.uint64).reshape(-1, 1)
    row = np.asarray(ends_row, np.int64)
    j = np.arange(len(row) - 1, dtype=np.uint64)[None, :]
    u = philox4x32_10((j, np.uint64(0), d & np.uint64(0xFFFFFFFF), d >> np.uint64(32)),
                      ((seed & 0xFFFFFFFF) ^ PRIO_TAG0, (seed >> 32) ^ PRIO_TAG1))[0]
    lo, hi = np.minimum(row[:-1] + 1, row[1:]), np.maximum(row[:-1] + 1, row[1:])
    r = lo[None, :] + ((u * (hi - lo + 1).astype(np.uint64)[None, :]) >> np.uint64(32)).astype(np.int64)
    return np.clip(r, 1, int(L))


def prio_weights(rank, alpha_beta):
    """float64 (rank / rank_max)^alpha_beta per minibatch (rows of `rank`): rank_based.py:176-182 with the normaliser and
    partition_max cancelled.  (The memories pass alpha_beta rounded to the float32 the device is given.)"""
    rank = np.asarray(rank, np.float64)
    return (rank / rank.max(axis=-1, keepdims=True)) ** float(alpha_beta)


def prio_update_bits(q, target=None):
    """uint32 bits of |q - target| in float32 (|q| without a target), NaN -> +inf"""
    q = np.asarray(q, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.abs(q - np.asarray(target, np.float32)) if target is not None else np.abs(q)
    return np.minimum(np.ascontiguousarray(p, np.float32).view(np.uint32), np.uint32(PRIO_NEW_BITS))


class _PrioConfig:
    """constructor arguments and tables shared by the model and the device class"""

    def _configure(self, buffer_size, batch_size, seed, alpha, beta_zero, learn_start, steps, partition_num, error):
        self.capacity, self.batch_size, self.seed = int(buffer_size), int(batch_size), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.alpha, self.beta_zero, self.learn_start, self.steps = float(alpha), float(beta_zero), int(learn_start), int(steps)
        if not 1 <= self.capacity <= 0x7FFFFFFF or not 1 <= self.batch_size <= self.capacity:
            raise error("need 1 <= batch_size <= buffer_size <= 2^31 - 1")
        if self.steps == self.learn_start:
            raise error("steps must differ from learn_start (rank_based.py:38 divides by their difference)")
        try:
            self.part_from, self.ends = strata_tables(self.capacity, self.batch_size, self.alpha, partition_num)
        except ValueError as e:
            raise error(str(e))
        self.beta_grad = (1 - self.beta_zero) / (self.steps - self.learn_start)          # rank_based.py:38
        self.min_live = max(self.learn_start, int(self.part_from[0]))

    def beta_at(self, count):
        """rank_based.py:176 with global_step = the adds ever made (replay_buffer.py:24)"""
        return min(self.beta_zero + (int(count) - self.learn_start - 1) * self.beta_grad, 1)

    def _alpha_beta(self, beta, error):
        ab = np.float32(self.alpha * float(beta))
        if not (np.isfinite(ab) and ab >= 0):
            raise error("alpha * beta must be finite and >= 0")
        return ab


class PrioritizedReplayModel(ReplayModel, _PrioConfig):
    """The prioritised memory on NumPy arrays: same methods and same results as PrioritizedReplayMemory.  capacity = buffer_size
    (rank_based.py:82-99 cycles its index over 1 .. size; the uniform class keeps its buffer_size - 1)."""

    def __init__(self, buffer_size=500000, batch_size=128, seed=0, alpha=0.7, beta_zero=0.5, learn_start=2000, steps=100000,
                 partition_num=PRIO_PARTS):
        self._configure(buffer_size, batch_size, seed, alpha, beta_zero, learn_start, steps, partition_num, ValueError)
        self.store = np.zeros((self.capacity, RECORD), np.float32)
        self.prio = np.zeros(self.capacity, np.uint32)
        self.pseq = np.zeros(self.capacity, np.int64)
        self.order = np.zeros(self.capacity, np.int32)
        self.reset()

    def reset(self):
        ReplayModel.reset(self)
        self.pseq[:] = -1
        self.pstate = np.zeros(4, np.int64)

    def keys(self):
        """(keys uint32 [L], ages [L]) of the live records, newest first: the sort's input"""
        L = self.live()
        age = L - 1 - np.arange(L, dtype=np.int64)
        w = self.written - L + age
        s = w % self.capacity
        bits = np.where(self.pseq[s] == w, self.prio[s], np.uint32(PRIO_NEW_BITS)).astype(np.uint32)
        return ~bits, age

    def rank(self):
        """-> order int32 [L] (a view of self.order): the age index of the record of rank r + 1"""
        L = self.live()
        key, age = self.keys()
        self.order[:L] = age[np.argsort(key, kind="stable")]
        self.pstate[PLIVE], self.pstate[PPART] = L, int(np.count_nonzero(self.part_from <= L))
        return self.order[:L]

    def sample(self, n_batches=1, beta=None, check=True):
        """-> (rows [n_batches, batch, 28], act7 [.., 7], target [..], seq int64 [..], rank int32 [..], weight float32 [..])"""
        n, B = int(n_batches), self.batch_size
        if n < 1:
            raise ValueError("n_batches must be >= 1")
        ab = self._alpha_beta(self.beta_at(self.count()) if beta is None else beta, ValueError)
        order = self.rank()
        L, part = self.live(), int(self.pstate[PPART])
        if L < self.min_live or part == 0:
            if check:
                raise PveError("prioritised replay memory: %d live records, fewer than the %d it needs" % (L, self.min_live))
            return (np.zeros((n, B, 28), np.float32), np.zeros((n, B, 7), np.float32), np.zeros((n, B), np.float32),
                    np.full((n, B), -1, np.int64), np.zeros((n, B), np.int32), np.zeros((n, B), np.float32))
        rank = prio_draw_ranks(self.seed, int(self.pstate[PDRAWS]) + np.arange(n, dtype=np.uint64), self.ends[part - 1], L)
        seq = self.written - L + order[rank - 1].astype(np.int64)
        rec = self.store[seq % self.capacity]
        self.pstate[PDRAWS] += n
        return (rec[..., :28].copy(), rec[..., 28:35].copy(), rec[..., 35].copy(), seq, rank.astype(np.int32),
                prio_weights(rank, ab).astype(np.float32))

    def update_priority(self, seq, q, target=None):
        seq = np.asarray(seq, np.int64).ravel()
        bits = prio_update_bits(np.asarray(q, np.float32).ravel(), None if target is None else np.asarray(target, np.float32).ravel())
        if bits.shape != seq.shape:
            raise ValueError("seq, q and target must have the same number of elements")
        L = self.live()
        ok = (seq >= self.written - L) & (seq < self.written)
        self.pstate[PIGNORED] = int(np.count_nonzero(~ok))
        s = seq[ok] % self.capacity
        self.pseq[s], self.prio[s] = seq[ok], 0
        np.maximum.at(self.prio, s, bits[ok])


class PrioritizedReplayMemory(ReplayMemory, _PrioConfig):
    """The prioritised memory on the device of `batch`: ReplayMemory's ring, add(), count() and live() with capacity =
    buffer_size, plus the priority store, rank(), the stratified sample() and update_priority().  Nothing here synchronises but
    sample(check=True), count() and live().  Priorities only matter for records that survive more than one sample / update round:
    a trainer that uses this memory cuts its adds with nstep_transitions(max_records=...)."""

    def __init__(self, batch, buffer_size=500000, batch_size=128, seed=0, alpha=0.7, beta_zero=0.5, learn_start=2000, steps=100000,
                 partition_num=PRIO_PARTS, block_threads=0):
        import torch
        self._torch = torch
        self.batch = batch
        self._configure(buffer_size, batch_size, seed, alpha, beta_zero, learn_start, steps, partition_num, PveError)
        scratch_bytes = int(batch.lib.pve_prio_scratch_bytes(self.capacity))          # (a size query: no handle, no status)
        self._ends_host = np.ascontiguousarray(self.ends, np.int32)
        self._part_from = np.ascontiguousarray(self.part_from, np.int64)
        with batch._own_stream():
            dev = batch.device
            self.store = torch.zeros(self.capacity, RECORD, dtype=torch.float32, device=dev)
            self.state = torch.zeros(_capi.REPLAY_STATE_WORDS, dtype=torch.int64, device=dev)
            self.prio = torch.zeros(self.capacity, dtype=torch.int32, device=dev)          # (uint32 bit patterns)
            self.pseq = torch.full((self.capacity,), -1, dtype=torch.int64, device=dev)
            self.order = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
            self.pstate = torch.zeros(_capi.PRIO_STATE_WORDS, dtype=torch.int64, device=dev)
            self.scratch = torch.empty(scratch_bytes // 4, dtype=torch.int32, device=dev)
            self.ends_dev = torch.as_tensor(self._ends_host).to(dev)
        self._pp = _capi.PvePrio()
        self._rp = self._pp.replay                           # (ReplayMemory's calls go through the embedded struct)
        self._rp.capacity, self._rp.store, self._rp.state = self.capacity, self.store.data_ptr(), self.state.data_ptr()
        self._rp.seed, self._rp.block_threads = self.seed, int(block_threads)
        p = self._pp
        p.prio, p.pseq, p.order, p.pstate = self.prio.data_ptr(), self.pseq.data_ptr(), self.order.data_ptr(), self.pstate.data_ptr()
        p.scratch, p.scratch_bytes, p.ends, p.batch = self.scratch.data_ptr(), scratch_bytes, self.ends_dev.data_ptr(), self.batch_size
        p.ends_host, p.part_from = self._ends_host.ctypes.data, self._part_from.ctypes.data

    def reset(self):
        with self.batch._own_stream():
            self.batch._call("pve_replay_reset", self._rp)
            self.batch._call("pve_prio_reset", self._pp)

    def rank(self):
        """Rank the live records -> order (int32 device tensor [capacity]; its first live() entries are the age indices by rank)"""
        with self.batch._own_stream():
            self.batch._call("pve_prio_rank", self._pp)
        return self.order

    def sample(self, n_batches=1, beta=None, check=True):
        """Rank, then draw n_batches stratified minibatches -> (rows, act7, target, seq, rank int32 [n_batches, batch_size],
        weight float32 [..]).  beta=None: beta_at(count()), which synchronises; pass beta to stay asynchronous.  check as in
        ReplayMemory.sample: True reads one status word and raises PveError when the memory is short (fewer live records than
        max(learn_start, part_from[0])), False never synchronises and a short memory gives seq = -1 and zeros."""
        torch = self._torch
        b, n, B = self.batch, int(n_batches), self.batch_size
        if n < 1:
            raise PveError("PrioritizedReplayMemory.sample: n_batches must be >= 1")
        ab = self._alpha_beta(self.beta_at(self.count()) if beta is None else beta, PveError)
        with b._own_stream():
            rows = torch.empty(n, B, 28, dtype=torch.float32, device=b.device)
            act7 = torch.empty(n, B, 7, dtype=torch.float32, device=b.device)
            target = torch.empty(n, B, dtype=torch.float32, device=b.device)
            seq = torch.empty(n, B, dtype=torch.int64, device=b.device)
            rank = torch.empty(n, B, dtype=torch.int32, device=b.device)
            weight = torch.empty(n, B, dtype=torch.float32, device=b.device)
            b._call("pve_prio_sample", self._pp, n, self.min_live, float(ab), rows, act7, target, seq, rank, weight)
            if check:
                L = int(self.pstate[PLIVE].item())
                if L < self.min_live:
                    raise PveError("prioritised replay memory: %d live records, fewer than the %d it needs" % (L, self.min_live))
        return rows, act7, target, seq, rank, weight

    def update_priority(self, seq, q, target=None):
        """Store |q - target| (|q| without a target) as the priority of the records `seq` names: int64 / float32 device tensors
        of equal element counts, e.g. sample()'s seq and target and critic_q(rows, act7)."""
        from ._args import is_tensor_of
        torch = self._torch
        b = self.batch
        want = (("seq", seq, torch.int64), ("q", q, torch.float32)) + ((("target", target, torch.float32),) if target is not None else ())
        for name, t, dt in want:                             # (seq first: the others are counted against it)
            if not is_tensor_of(t, dt, self.store.device, same_device=True) or t.numel() != seq.numel():
                raise PveError("PrioritizedReplayMemory.update_priority: %s must be a %s tensor on %s with seq's element count"
                               % (name, dt, self.store.device))
        with b._own_stream():
            seq, q = seq.contiguous(), q.contiguous()
            target = target.contiguous() if target is not None else None
            b._call("pve_prio_update", self._pp, seq, q, target, int(seq.numel()))

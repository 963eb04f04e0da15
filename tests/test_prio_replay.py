"""The rank-based prioritised memory without a GPU: pve_mcc_amd/replay.py (strata_tables, PrioritizedReplayModel) against the
recorded reference (tests/golden/prio_ref.npz, written by tests/golden/gen_prio_golden.py from the unmodified rank_based.py), against
the LIVE reference where it is present, against its own rules, and against a g++ build of csrc/pve_prio.h (tests/prio_host), bit
for bit; plus the C ABI's argument checks through the CPU emulator, which has no such kernels and says so.  The kernels are held
to the model in tests/test_gpu_prio_replay.py.  Only the importance weight is floating point."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from pve_mcc_amd import PrioritizedReplayMemory, PrioritizedReplayModel, PveError, ReplayModel, _capi, replay
from tests import native
from tests import prio_scenarios as S
from tests.hip_adapter import emulator_lib, make_batch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF_DIR = "/root/reference"
CASES = ((320, 8), (333, 8), (1000, 16), (4096, 128))
_cache = {}


def fixture():
    if "z" not in _cache:
        _cache["z"] = np.load(os.path.join(ROOT, "tests", "golden", "prio_ref.npz"))
    return _cache["z"]


def tables(size, batch):
    if (size, batch) not in _cache:
        _cache[(size, batch)] = replay.strata_tables(size, batch)
    return _cache[(size, batch)]


def _signatures(L):
    vp, ll = C.c_void_p, C.c_longlong
    L.prio_scratch_bytes_host.restype = C.c_ulonglong
    L.prio_scratch_bytes_host.argtypes = [ll]
    L.prio_partition_host.argtypes = [vp, ll]
    L.prio_rank_host.restype = ll
    L.prio_rank_host.argtypes = [ll, ll, vp, vp, vp]
    L.prio_draw_host.restype = None
    L.prio_draw_host.argtypes = [vp, ll, C.c_uint64, C.c_uint64, ll, ll, C.c_float, vp, vp]
    L.prio_update_host.restype = ll
    L.prio_update_host.argtypes = [ll, ll, vp, vp, vp, vp, vp, ll]
    return L


def shim():
    """csrc/pve_prio.h compiled by g++ (tests/prio_host), built and loaded by tests/native.py."""
    return native.load("prio_host", "libprio_host.so", _signatures)


def model(capacity=320, batch=8, **kw):
    kw.setdefault("learn_start", 0)
    kw.setdefault("steps", 1000)
    return PrioritizedReplayModel(buffer_size=capacity, batch_size=batch, **kw)


def partition_of(part_from, L):
    return np.count_nonzero(np.asarray(part_from)[None, :] <= np.asarray(L)[:, None], axis=1)


# ------------------------------------------------------------------ 1. tables and partition index
@pytest.mark.parametrize("size,batch", CASES)
def test_tables_vs_fixture(size, batch):
    z = fixture()
    part_from, ends = tables(size, batch)
    assert ends.dtype == np.int32 and ends.shape == (32, batch + 1) and part_from.dtype == np.int64 and part_from.shape == (32,)
    assert np.array_equal(ends, z["ends_%d_%d" % (size, batch)])
    assert np.array_equal(partition_of(part_from, np.arange(1, size + 1)), z["dist_%d_%d" % (size, batch)])
    assert (ends[:, 0] == 0).all() and (np.diff(ends, axis=1) >= 0).all() and np.array_equal(ends[:, -1], (size // 32) * np.arange(1, 33))
    assert (part_from >= ends[:, -1]).all()                 # a partition is reached only with at least its n_k records live
    if (size, batch) == (4096, 128):
        assert int((np.diff(ends, axis=1) == 0).sum()) == 334            # the degenerate strata exist


@pytest.mark.reference
@pytest.mark.parametrize("size,batch", CASES[:3] + ((640, 16),))
def test_tables_vs_live_reference(size, batch):
    if REF_DIR not in sys.path:
        sys.path.insert(0, REF_DIR)
    import rank_based
    exp = rank_based.Experience({"size": size, "batch_size": batch, "partition_num": 32, "learn_start": 0, "steps": 1000})
    part_from, ends = tables(size, batch)
    want = np.array([[exp.distributions[p]["strata_ends"][s] for s in range(1, batch + 2)] for p in range(1, 33)], np.int32)
    assert np.array_equal(ends, want)
    dist = np.array([int(math.floor(1.0 * L / size * 32)) for L in range(1, size + 1)])
    assert np.array_equal(partition_of(part_from, np.arange(1, size + 1)), dist)


def test_tables_argument_errors():
    for kw in (dict(size=31, batch_size=1), dict(size=320, batch_size=11), dict(size=320, batch_size=0), dict(size=320, batch_size=8, partition_num=33),
               dict(size=320, batch_size=8, partition_num=0)):
        with pytest.raises(ValueError):
            replay.strata_tables(**kw)
    part_from, ends = replay.strata_tables(320, 8, partition_num=4)      # fewer partitions: the rest is never reached
    assert (part_from[4:] == 1 << 62).all() and list(part_from[:4]) == [80, 160, 240, 320] and (ends[4:] == ends[3]).all()
    for kw in (dict(buffer_size=0), dict(buffer_size=320, batch_size=0), dict(buffer_size=320, learn_start=7, steps=7)):
        with pytest.raises(ValueError):
            PrioritizedReplayModel(**dict(dict(buffer_size=320, batch_size=8), **kw))


# ------------------------------------------------------------------ 2. the recorded trace of the reference
@pytest.mark.parametrize("stage", ["A", "B"])
def test_model_vs_recorded_trace(stage):
    z = fixture()
    m = model(learn_start=int(z["learn_start"]), steps=int(z["steps"]), alpha=float(z["alpha"]), beta_zero=float(z["beta_zero"]))
    assert m.capacity == 320
    written = int(z[stage + "_written"])
    rec = S.payload(written)
    m.add(rec)
    m.update_priority(z[stage + "_upd_seq"], z[stage + "_upd_p"])
    assert len(np.unique(z[stage + "_upd_p"])) == m.live() == len(z[stage + "_p2e"]) and m.pstate[replay.PIGNORED] == 0
    order = m.rank()
    assert np.array_equal(m.written - m.live() + order.astype(np.int64), z[stage + "_p2e"])          # priority_to_experience(1 .. L)
    part = int(m.pstate[replay.PPART])
    assert part == int(math.floor(1.0 * m.live() / 320 * 32))
    row = m.ends[part - 1]
    lo, hi = np.minimum(row[:-1] + 1, row[1:]), np.maximum(row[:-1] + 1, row[1:])
    for i, step in enumerate(z[stage + "_steps"]):
        ranks = z[stage + "_ranks"][i]
        assert ((ranks >= lo) & (ranks <= hi)).all()        # the reference's draws fall into the strata the model draws from
        assert np.array_equal(m.written - m.live() + order[ranks - 1], z[stage + "_exp"][i])
        w = replay.prio_weights(ranks, m.alpha * m.beta_at(step))
        assert np.abs(w - z[stage + "_w"][i]).max() <= 1e-12
    assert m.beta_at(2000) == 1 and m.beta_at(101) == 0.5


# ------------------------------------------------------------------ 3. the model's own rules
def test_new_records_first_newest_first_and_wrap():
    m = model()
    m.add(S.payload(100))
    assert np.array_equal(m.rank(), np.arange(100)[::-1]) and m.pstate[replay.PLIVE] == 100      # all NEW: newest first
    m.update_priority(np.array([10, 20, 30]), np.array([3.0, -5.0, 4.0], np.float32))
    new = [a for a in range(99, -1, -1) if a not in (10, 20, 30)]
    assert list(m.rank()) == new + [20, 30, 10]
    m.update_priority(np.array([40, 41]), np.array([np.inf, -np.inf], np.float32))                  # +inf ties with NEW: by record number
    assert list(m.rank()) == [a for a in range(99, -1, -1) if a not in (10, 20, 30)] + [20, 30, 10]
    m.update_priority(np.array([5, 6, 7]), np.array([2.0, 2.0, 2.0], np.float32))                  # equal priorities: newest first
    assert list(m.rank())[-6:] == [20, 30, 10, 7, 6, 5]
    # wrap-around, capacity not dividing written: record w lives in slot w mod 320, an overwritten slot is NEW again
    m.add(S.payload(333, 100))
    assert m.written == 433 and m.live() == 320 and m.written % 320 != 0
    order = m.rank()
    seq = m.written - 320 + order.astype(np.int64)
    assert np.array_equal(np.sort(seq), np.arange(113, 433))
    assert list(seq) == list(range(432, 112, -1))                                        # every survivor's priority was overwritten
    m2 = model()
    m2.add(S.payload(320))
    m2.update_priority(np.arange(320), np.arange(320, dtype=np.float32) + 1)
    m2.add(S.payload(10, 320))                                                                     # slots 0 .. 9 overwritten: NEW again
    seq2 = m2.written - 320 + m2.rank().astype(np.int64)
    assert list(seq2[:10]) == list(range(329, 319, -1)) and list(seq2[10:]) == list(range(319, 9, -1))


def test_update_rules():
    m = model()
    m.add(S.payload(400))                                   # live: 80 .. 399
    m.update_priority(np.array([-1, 79, 80, 399, 400, 5, 1 << 40]), np.ones(7, np.float32))
    assert m.pstate[replay.PIGNORED] == 5 and int((m.pseq >= 0).sum()) == 2                        # stale, unwritten and -1: ignored, counted
    m.update_priority(np.array([100, 100, 100, 101]), np.array([1.0, -7.0, 3.0, 2.0], np.float32))
    assert m.prio[100] == np.float32(7.0).view(np.uint32) and m.prio[101] == np.float32(2.0).view(np.uint32)     # the largest wins
    m.update_priority(np.array([100]), np.array([0.5], np.float32))
    assert m.prio[100] == np.float32(0.5).view(np.uint32) and m.pstate[replay.PIGNORED] == 0       # replaced, not maxed
    m.update_priority(np.array([102, 103, 104, 105]), np.array([np.nan, 1.0, np.inf, 2.0], np.float32),
                      np.array([0.0, np.nan, np.inf, 2.0], np.float32))
    assert list(m.prio[102:106]) == [S.INF_BITS, S.INF_BITS, S.INF_BITS, 0]                        # NaN -> +inf; 2 - 2 = +0
    m.update_priority(np.array([110]), np.array([3.0], np.float32), np.array([1.5], np.float32))
    assert m.prio[110] == np.float32(1.5).view(np.uint32)                                           # |q - target|
    with pytest.raises(ValueError):
        m.update_priority(np.arange(3), np.ones(2, np.float32))


def test_draw_degenerate_strata_and_short_memory():
    m = model(4096, 128, learn_start=200, seed=(1 << 33) + 9)
    assert m.min_live == 200 and model(4096, 128).min_live == 128 == tables(4096, 128)[0][0]
    with pytest.raises(PveError, match="fewer"):
        m.sample()
    m.add(S.payload(199))
    out = m.sample(2, check=False)                          # short: seq = -1, zeros, pdraws unchanged, but ranked
    assert (out[3] == -1).all() and not any(x.any() for x in out[:3] + out[4:]) and m.pstate[replay.PDRAWS] == 0
    assert m.pstate[replay.PLIVE] == 199 and out[4].dtype == np.int32 and out[5].dtype == np.float32 and out[0].shape == (2, 128, 28)
    m.add(S.payload(4096 - 199, 199))
    rows, act7, target, seq, rank, weight = m.sample(50, beta=0.6)
    row = m.ends[31]
    degenerate = np.flatnonzero(np.diff(row) == 0)
    assert len(degenerate) > 0 and m.pstate[replay.PDRAWS] == 50
    lo, hi = np.minimum(row[:-1] + 1, row[1:]), np.maximum(row[:-1] + 1, row[1:])
    assert ((rank >= lo) & (rank <= hi)).all() and rank.min() >= 1 and rank.max() <= 4096
    assert set(np.unique(rank[:, degenerate] - row[degenerate])) == {0, 1}                         # the swapped randint: ends[j] or ends[j] + 1
    assert any(len(set(r.tolist())) < 128 for r in rank)                                            # so ranks repeat within a minibatch
    assert np.array_equal(seq, m.written - 4096 + m.order[rank - 1]) and (weight.max(axis=1) == 1).all()
    rec = np.concatenate([rows, act7, target[..., None]], axis=-1).reshape(-1, 36)
    assert np.array_equal(S.bits32(rec), S.bits32(S.payload(4096)[seq.ravel()]))
    # minibatch d is a function of (seed, d): 50 at once = one at a time; another seed draws differently
    twin = model(4096, 128, learn_start=200, seed=(1 << 33) + 9)
    twin.add(S.payload(4096))
    one = np.concatenate([twin.sample(1, beta=0.6)[4] for _ in range(50)])
    assert np.array_equal(one, rank)
    other = model(4096, 128, learn_start=200, seed=5)
    other.add(S.payload(4096))
    assert not np.array_equal(other.sample(50, beta=0.6)[4], rank)
    # every stratum's draw covers its range and nothing else (4000 minibatches of the narrow first partition)
    small = model(320, 8)
    small.add(S.payload(10))
    r = small.sample(4000, beta=1.0)[4]
    row = small.ends[0]
    for j in range(8):
        want = set(range(min(row[j] + 1, row[j + 1]), max(row[j] + 1, row[j + 1]) + 1))
        assert set(np.unique(r[:, j])) == want, (j, want)
    assert isinstance(small, ReplayModel) and small.count() == 10


# ------------------------------------------------------------------ 4. the header's g++ build equals the model bit for bit
@pytest.mark.parametrize("pattern", S.PATTERNS)
def test_host_build_rank_and_update(pattern):
    L = shim()
    rng = np.random.default_rng(11)
    for live in (1, 63, 64, 65, 257, 4097):
        capacity, written = S.geometry(live)
        m = model(capacity, 2)
        m.add(np.zeros((written, 36), np.float32))
        ids, q = S.pattern_update(pattern, m.live_seq(), rng)
        prio, pseq = m.prio.copy(), m.pseq.copy()
        m.update_priority(ids, q)
        ign = L.prio_update_host(written, capacity, prio.ctypes.data, pseq.ctypes.data, np.ascontiguousarray(ids).ctypes.data,
                                 np.ascontiguousarray(q).ctypes.data, None, len(ids))
        assert ign == 0 and np.array_equal(prio, m.prio) and np.array_equal(pseq, m.pseq)
        seq, q, target = S.messy_update(written, m.live(), 300, rng)
        for tgt in (target, None):
            m.update_priority(seq, q, tgt)
            ign = L.prio_update_host(written, capacity, prio.ctypes.data, pseq.ctypes.data, seq.ctypes.data, q.ctypes.data,
                                     tgt.ctypes.data if tgt is not None else None, len(seq))
            assert ign == m.pstate[replay.PIGNORED] > 0 and np.array_equal(prio, m.prio) and np.array_equal(pseq, m.pseq)
        order = np.full(capacity, -7, np.int32)
        assert L.prio_rank_host(written, capacity, prio.ctypes.data, pseq.ctypes.data, order.ctypes.data) == live
        assert np.array_equal(order[:live], m.rank()) and (order[live:] == -7).all()
        assert np.array_equal(np.sort(order[:live]), np.arange(live))
        assert L.prio_scratch_bytes_host(capacity) == 16 * ((capacity + 3) // 4 * 4) + 1024 * ((capacity + 2047) // 2048 + 4)


@pytest.mark.parametrize("size,batch", CASES)
def test_host_build_draw_is_bit_equal(size, batch):
    L = shim()
    part_from, ends = tables(size, batch)
    lives = np.unique(np.concatenate([part_from, part_from - 1, [1, size]]))
    pf = np.ascontiguousarray(part_from)
    for live in lives:
        assert L.prio_partition_host(pf.ctypes.data, int(live)) == int(np.count_nonzero(part_from <= live))
    worst = 0.0
    for part in (1, 2, 17, 32):
        live = int(part_from[part - 1])
        row = np.ascontiguousarray(ends[part - 1])
        for seed, d0 in ((0, 0), (3, (1 << 32) - 2), ((1 << 64) - 1, (1 << 40) + 3)):
            n = 5
            rank, weight = np.zeros((n, batch), np.int32), np.zeros((n, batch), np.float32)
            L.prio_draw_host(row.ctypes.data, batch, seed, d0, n, live, np.float32(0.42), rank.ctypes.data, weight.ctypes.data)
            want = replay.prio_draw_ranks(seed, (d0 + np.arange(n)).astype(np.uint64), row, live)
            assert np.array_equal(rank, want)
            w64 = replay.prio_weights(want, np.float32(0.42))
            worst = max(worst, float(np.abs(weight / w64 - 1).max()))
    print("host float32 weight vs float64: %.2e relative" % worst)
    assert worst <= S.WEIGHT_BAR


# ------------------------------------------------------------------ 5. the C ABI on a backend without the kernels
def test_entry_points_on_the_emulator():
    from pve_mcc_amd.arrivals import synthetic_arrivals
    lib = emulator_lib()
    names = ("pve_prio_scratch_bytes", "pve_prio_reset", "pve_prio_rank", "pve_prio_sample", "pve_prio_update")
    for name in names:
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert lib.pve_abi_version() == _capi.ABI_VERSION          # (version, constants, layout against the header: tests/test_binding_contract.py)
    header = open(os.path.join(ROOT, "include", "pve_env.h")).read()
    for text in ("0x5052494F", "0x52414E4B", "rank_based.py:148-188",
                 "main.py:76-79", "binary_heap.py:194-221", "rank_based.py:40-80", "replay_buffer.py:13-18"):
        assert text in header, text
    assert (replay.PRIO_TAG0, replay.PRIO_TAG1) == (0x5052494F, 0x52414E4B)
    assert lib.pve_prio_scratch_bytes(0) == 0 and lib.pve_prio_scratch_bytes(1 << 31) == 0 and lib.pve_prio_scratch_bytes(-3) == 0
    assert lib.pve_prio_scratch_bytes(500000) == 16 * 500000 + 1024 * (245 + 4) and lib.pve_prio_scratch_bytes(321) == 16 * 324 + 1024 * 5
    b = make_batch(synthetic_arrivals(2, rate=500.0, horizon_s=20.0, seed=1), 2, 64, "emu", outputs=("obs_post", "flags"))
    keep = []

    def P(shape, dt, off=0):
        raw = np.zeros(int(np.prod(shape)) * np.dtype(dt).itemsize + 32, np.uint8)
        keep.append(raw)
        return raw.ctypes.data + (-raw.ctypes.data) % 16 + off

    cap, batch, nb = 320, 8, 3
    part_from, ends = tables(cap, batch)
    ends, part_from = np.ascontiguousarray(ends), np.ascontiguousarray(part_from)
    need = lib.pve_prio_scratch_bytes(cap)
    store, state = P((cap, 36), np.float32), P((4,), np.int64)
    prio, pseq, order, pstate, scratch = P((cap,), np.uint32), P((cap,), np.int64), P((cap,), np.int32), P((4,), np.int64), P((need,), np.uint8)
    rows, act7, target, seq = P((nb, batch, 28), np.float32), P((nb, batch, 7), np.float32), P((nb, batch), np.float32), P((nb, batch), np.int64)
    rank, weight, q = P((nb, batch), np.int32), P((nb, batch), np.float32), P((nb, batch), np.float32)

    def pp(**kw):
        p = _capi.PvePrio()
        p.replay.capacity, p.replay.store, p.replay.state, p.replay.seed, p.replay.block_threads = cap, store, state, 1, 0
        p.prio, p.pseq, p.order, p.pstate, p.scratch, p.scratch_bytes = prio, pseq, order, pstate, scratch, need
        p.ends, p.ends_host, p.part_from, p.batch = ends.ctypes.data, ends.ctypes.data, part_from.ctypes.data, batch
        for k, v in kw.items():
            if k in ("capacity", "store", "state", "block_threads"):
                setattr(p.replay, k, v)
            else:
                setattr(p, k, v)
        return p

    def ref(p):
        return C.byref(p) if p is not None else None

    def sample(p, h=b._h, nb=nb, min_live=8, ab=0.35, out=(rows, act7, target, seq, rank, weight)):
        return lib.pve_prio_sample(h, ref(p), nb, min_live, C.c_float(ab), *out)

    def update(p, h=b._h, seq=seq, q=q, target=target, n=nb * batch):
        return lib.pve_prio_update(h, ref(p), seq, q, target, n)

    calls = (lambda p, h=b._h: lib.pve_prio_reset(h, ref(p)), lambda p, h=b._h: lib.pve_prio_rank(h, ref(p)), sample, update)

    def bad_ends(j, value, row=5):
        e = ends.copy()
        e[row, j] = value
        keep.append(e)
        return e.ctypes.data

    def bad_parts(k, value):
        f = part_from.copy()
        f[k] = value
        keep.append(f)
        return f.ctypes.data

    shared = [(dict(store=None), b"null"), (dict(state=None), b"null"), (dict(capacity=0), b"capacity"), (dict(capacity=1 << 31), b"capacity"),
              (dict(block_threads=100), b"block_threads"), (dict(block_threads=2048), b"block_threads"), (dict(store=store + 8), b"aligned"),
              (dict(state=state + 4), b"aligned")]
    shared += [(dict([(k, None)]), b"null") for k in ("prio", "pseq", "order", "pstate", "scratch", "ends", "ends_host", "part_from")]
    shared += [(dict(prio=prio + 2), b"aligned"), (dict(order=order + 1), b"aligned"), (dict(ends=ends.ctypes.data + 2), b"aligned"),
               (dict(pseq=pseq + 4), b"aligned"), (dict(pstate=pstate + 4), b"aligned"), (dict(scratch=scratch + 8), b"aligned"),
               (dict(scratch_bytes=need - 1), b"scratch_bytes"), (dict(scratch_bytes=-1), b"scratch_bytes"), (dict(batch=0), b"batch"),
               (dict(batch=cap + 1), b"batch"), (dict(part_from=bad_parts(0, 0)), b"part_from"), (dict(part_from=bad_parts(7, 3)), b"part_from"),
               (dict(ends_host=bad_ends(0, 1)), b"start at 0"), (dict(ends_host=bad_ends(4, 1)), b"non-decreasing"),
               (dict(ends_host=bad_ends(batch, cap + 1)), b"non-decreasing"), (dict(ends_host=bad_ends(3, -2, row=31)), b"non-decreasing")]
    for kw, word in shared:
        for fn in calls:
            assert fn(pp(**kw)) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    for fn in calls:
        assert fn(None) == -1 and b"null" in lib.pve_last_error()
        assert fn(pp(), h=None) == -1 and b"null" in lib.pve_last_error()
    outs = (rows, act7, target, seq, rank, weight)
    bad_sample = [(dict(nb=0), b"n_batches"), (dict(nb=-2), b"n_batches"), (dict(nb=1 << 29), b"n_batches"), (dict(min_live=-1), b"min_live"),
                  (dict(ab=-0.1), b"alpha_beta"), (dict(ab=float("nan")), b"alpha_beta"), (dict(ab=float("inf")), b"alpha_beta")]
    bad_sample += [(dict(out=outs[:k] + (None,) + outs[k + 1:]), b"null output") for k in range(6)]
    bad_sample += [(dict(out=outs[:k] + (outs[k] + off,) + outs[k + 1:]), b"aligned") for k, off in enumerate((4, 8, 2, 4, 2, 2))]
    for kw, word in bad_sample:
        assert sample(pp(), **kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    for kw, word in ((dict(n=-1), b"n must"), (dict(seq=None), b"null seq or q"), (dict(q=None), b"null seq or q"), (dict(seq=seq + 4), b"aligned"),
                     (dict(q=q + 2), b"aligned"), (dict(target=target + 2), b"aligned")):
        assert update(pp(), **kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    # valid arguments: the emulator has no such kernels and says so (a NULL target, n = 0 and min_live = 0 are valid too)
    for fn in (lambda: calls[0](pp()), lambda: calls[1](pp()), lambda: sample(pp()), lambda: sample(pp(block_threads=1024), nb=1, min_live=0, ab=0.0),
               lambda: update(pp()), lambda: update(pp(), target=None), lambda: update(pp(), seq=None, q=None, n=0)):
        assert fn() == -1 and b"backend has no prioritised replay kernels" in lib.pve_last_error(), lib.pve_last_error()
    # the Python class asks the backend
    import torch
    m = PrioritizedReplayMemory(b, buffer_size=cap, batch_size=batch, learn_start=0, steps=1000)
    assert m.capacity == cap and m.store.shape == (cap, 36) and m.pseq.dtype == torch.int64 and m.min_live == 10 and m.batch_size == batch
    assert np.array_equal(m.ends, ends) and m.scratch.numel() * 4 == need
    for call in (lambda: m.rank(), lambda: m.sample(beta=0.5, check=False), lambda: m.add(torch.zeros(5, 36)),
                 lambda: m.update_priority(torch.zeros(4, dtype=torch.int64), torch.zeros(4))):
        with pytest.raises(PveError, match="backend"):
            call()
    with pytest.raises(PveError, match="n_batches"):
        m.sample(0)
    with pytest.raises(PveError, match="float32"):
        m.update_priority(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(PveError, match="element count"):
        m.update_priority(torch.zeros(4, dtype=torch.int64), torch.zeros(5))
    for kw in (dict(buffer_size=16), dict(batch_size=11), dict(learn_start=5, steps=5)):
        with pytest.raises(PveError):
            PrioritizedReplayMemory(b, **dict(dict(buffer_size=cap, batch_size=batch), **kw))


# ------------------------------------------------------------------ 6. the host build is stale after an edit of what it reads
def test_host_build_is_stale_after_any_file_it_reads():
    import subprocess
    native.build("prio_host", "libprio_host.so")
    here = os.path.join(native.TESTS_DIR, "prio_host")
    csrc = "../../pve-mcc_for_unsignalized_intersection_amd/csrc/"
    assert subprocess.run(["make", "-s", "-q", "libprio_host.so"], cwd=here).returncode == 0
    for f in ("prio_host.cpp", "Makefile", "../native.mk", csrc + "pve_prio.h", csrc + "pve_replay.h", csrc + "pve_noise.h", csrc + "pve_types.h"):
        assert subprocess.run(["make", "-s", "-q", "-W", f, "libprio_host.so"], cwd=here).returncode == 1, f

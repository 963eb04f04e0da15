"""The replay memory without a GPU: pve_mcc_amd/replay.py (ReplayModel, perm) against the LIVE reference's ReplayBuffer, against
its own specification (bijection, independence of how the j range is cut, uniformity) and against a g++ build of csrc/pve_replay.h
(tests/replay_host), plus the C ABI's argument checks through the CPU emulator, which has no replay kernels and says so.  The
kernels are held to ReplayModel in tests/test_gpu_replay.py.  Everything is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from pve_mcc_amd import PveError, ReplayMemory, ReplayModel, _capi, replay
from tests import native
from tests import replay_scenarios as S
from tests.hip_adapter import emulator_lib, make_batch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF_DIR = "/root/reference"


def _signatures(L):
    L.replay_half_bits_host.argtypes = [C.c_uint32]
    L.replay_perm_host.restype = None
    L.replay_perm_host.argtypes = [C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_longlong, C.c_void_p]
    L.replay_append_host.restype = C.c_longlong
    L.replay_append_host.argtypes = [C.c_longlong, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_void_p]
    return L


def shim():
    """csrc/pve_replay.h compiled by g++ (tests/replay_host), built and loaded by tests/native.py."""
    return native.load("replay_host", "libreplay_host.so", _signatures)


# ------------------------------------------------------------------ 1. the store against the live reference
@pytest.mark.reference
def test_store_vs_live_reference():
    """ReplayBuffer(320, 8, 0, 100, rand_s=True) fed one record at a time against ReplayModel(buffer_size=320) fed in chunks of
    1, 7, 318, 319, 320, 321, 0 and 700 records, every chunk at its full length (1986 records in all; the 960 the issue speaks
    of would cut the chunks longer than the ring short, and those are the ones that take the skip path against the real
    deque): after every chunk list(buffer) is the model's live records in age order, count() agrees and the deque never holds
    more than 319 entries."""
    if REF_DIR not in sys.path:
        sys.path.insert(0, REF_DIR)
    from replay_buffer import ReplayBuffer
    ref = ReplayBuffer(320, 8, 0, 100, rand_s=True)
    model = ReplayModel(buffer_size=320, batch_size=8)
    assert model.capacity == 319
    chunks = (1, 7, 318, 319, 320, 321, 0, 700)
    rec = S.payload(sum(chunks))
    assert len(rec) == 1986 >= 960
    fed = 0
    for n in chunks:
        chunk = rec[fed:fed + n]
        assert len(chunk) == n                               # no chunk is shortened
        for r in chunk:
            ref.add(r[:28].copy(), r[28:35].copy(), r[35], None, False)
        model.add(chunk)
        fed += n
        have = list(ref.buffer)
        got = np.array([np.concatenate([s, a, [t]]) for s, a, t, _, _ in have], np.float32).reshape(len(have), 36)
        assert all(x[3] is None and x[4] is False for x in have)
        assert ref.count() == model.count() == fed
        assert len(have) == model.live() == min(fed, 319)
        assert np.array_equal(S.bits32(got), S.bits32(model.live_records()))
        if n > 319:                                          # longer than the ring: only its last 319 records are live
            assert np.array_equal(S.bits32(got), S.bits32(chunk[-319:]))
    assert fed == len(rec) and model.live() == 319


# ------------------------------------------------------------------ 2. perm: a bijection, whatever way the j range is cut
@pytest.mark.parametrize("N", [1, 2, 3, 5, 16, 64, 65, 1000, 4097])
def test_perm_is_a_bijection(N):
    for seed, d in ((0, 0), (1, 5), (3, 1 << 32), ((1 << 32) + 5, (1 << 32) + 7), ((1 << 64) - 1, (1 << 40) + 3)):
        p = replay.perm(seed, d, N)
        assert p.shape == (N,) and np.array_equal(np.sort(p), np.arange(N)), (N, seed, d)
        # the value at j does not depend on which other j are evaluated with it: one at a time, in two ragged pieces, reversed
        cut = N // 3
        pieces = np.concatenate([replay.perm(seed, d, N, np.arange(0, cut)), replay.perm(seed, d, N, np.arange(cut, N))])
        assert np.array_equal(pieces, p)
        assert np.array_equal(replay.perm(seed, d, N, np.arange(N)[::-1])[::-1], p)
        for j in (0, N // 2, N - 1):
            assert int(replay.perm(seed, d, N, j)) == p[j]
    # several draw numbers in one call = one call each; different draws and seeds give different permutations
    if N >= 64:
        many = replay.perm(7, np.arange(4, dtype=np.uint64)[:, None], N, np.arange(N)[None, :])
        for d in range(4):
            assert np.array_equal(many[d], replay.perm(7, d, N))
        assert not np.array_equal(many[0], many[1]) and not np.array_equal(many[0], replay.perm(8, 0, N))
        assert not np.array_equal(replay.perm(7, 1 << 32, N), many[0]) and not np.array_equal(replay.perm(7 + (1 << 32), 0, N), many[0])


def test_perm_argument_errors():
    for bad in (0, -1, 1 << 31):
        with pytest.raises(ValueError):
            replay.perm(0, 0, bad)
    with pytest.raises(ValueError):
        replay.perm(0, 0, 10, 10)
    assert [replay.half_bits(n) for n in (1, 2, 4, 5, 16, 17, 64, 65, 1000, 4097, (1 << 31) - 1)] == [1, 1, 1, 2, 2, 3, 3, 4, 5, 7, 16]


# ------------------------------------------------------------------ 3. perm draws uniformly
def test_perm_marginals_are_uniform():
    """N = 1000, batch 128, 2000 consecutive draws: Pearson's statistic of the per-record counts against the 0.999 quantile of
    chi-square with 999 degrees of freedom.  Measured with the tagged key: 862 / 825 / 897 for seeds 1 / 2 / 3."""
    for seed in S.SEEDS:
        v = replay.perm(seed, np.arange(2000, dtype=np.uint64)[:, None], 1000, np.arange(128)[None, :])
        stat = S.pearson(np.bincount(v.ravel(), minlength=1000))
        print("seed %d: marginals %.1f (bar %.0f)" % (seed, stat, S.CHI2_999))
        assert stat < S.CHI2_999


@pytest.mark.parametrize("N,draws,bar", [(64, 403200, S.CHI2_4031), (100, 990000, S.CHI2_9899)])
def test_perm_ordered_pairs_are_uniform(N, draws, bar):
    """(perm(0), perm(1)) over consecutive draws: the diagonal is empty (a bijection), Pearson's statistic over the N (N - 1)
    off-diagonal cells against the 0.999 quantile of chi-square with N (N - 1) - 1 degrees of freedom.  Measured with the
    tagged key: N = 64: 4114 / 3927 / 4098, N = 100: 9896 / 9826 / 9920 for seeds 1 / 2 / 3 (four rounds instead of eight gave
    9299 and 10 419 untagged: too few)."""
    for seed in S.SEEDS:
        v = replay.perm(seed, np.arange(draws, dtype=np.uint64)[:, None], N, np.arange(2)[None, :])
        cells = np.bincount(v[:, 0] * N + v[:, 1], minlength=N * N).reshape(N, N)
        assert np.trace(cells) == 0
        stat = S.pearson(cells[~np.eye(N, dtype=bool)])
        print("seed %d, N %d: ordered pairs %.1f (bar %.0f)" % (seed, N, stat, bar))
        assert stat < bar


# ------------------------------------------------------------------ 4. the header's g++ build equals replay.py bit for bit
def test_host_build_perm_is_bit_equal():
    L = shim()
    rng = np.random.default_rng(5)
    n_checked = 0
    for N in (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 257, 1000, 4097, 65536, 65537, 499999, (1 << 31) - 1):
        assert L.replay_half_bits_host(N) == replay.half_bits(N)
        for seed in (0, 1, 3, (1 << 32) + 5, (1 << 64) - 1):
            d = np.concatenate([np.arange(3), [(1 << 32) - 1, 1 << 32, (1 << 63) + 11]]).astype(np.uint64)
            j = np.unique(np.concatenate([[0, N - 1, N // 2], rng.integers(0, N, 24)])).astype(np.uint32)
            dd, jj = (np.ascontiguousarray(x.ravel()) for x in np.meshgrid(d, j, indexing="ij"))
            out = np.zeros(dd.size, np.uint32)
            L.replay_perm_host(seed, dd.ctypes.data, N, jj.ctypes.data, dd.size, out.ctypes.data)
            want = replay.perm(seed, dd, N, jj)
            assert np.array_equal(out.astype(np.int64), want), (N, seed)
            n_checked += dd.size
    assert n_checked > 5000


def test_host_build_append_plan_is_bit_equal():
    L = shim()
    for capacity in (1, 7, 64, 319, 4099):
        written = 0
        for n_max, total in [(c, None) for c in S.append_chunks(capacity)] + [(50, 20), (50, 50), (50, 70), (50, 0), (50, -3), (3 * capacity, 2 * capacity + 1)]:
            slot = np.full(max(n_max, 1), -1, np.int64)          # (one spare element so that n_max = 0 has an address)
            n = L.replay_append_host(written, total is not None, total if total is not None else 0, n_max, capacity, slot.ctypes.data)
            assert n == replay.accepted(n_max, total)
            skip, slots = replay.append_plan(written, n, capacity)
            want = np.full(max(n_max, 1), -1, np.int64)
            want[skip:n] = slots
            assert np.array_equal(slot, want), (capacity, written, n_max, total)
            assert len(set(slots.tolist())) == len(slots) and np.array_equal(slots, (written + np.arange(skip, n)) % capacity)
            written += n
    # far along: `written` beyond 2^32
    slot = np.zeros(10, np.int64)
    assert L.replay_append_host((1 << 40) + 3, 0, 0, 10, 7, slot.ctypes.data) == 10
    assert np.array_equal(slot[3:], ((1 << 40) + 3 + np.arange(3, 10)) % 7) and (slot[:3] == -1).all()


# ------------------------------------------------------------------ 5. model edge cases
def naive_ring(chunks, capacity):
    """every record appended one by one to a Python list cut to the last `capacity`: the reference's deque"""
    live, first = [], 0
    for n in chunks:
        live = (live + list(range(first, first + n)))[-capacity:]
        first += n
        yield first, live


@pytest.mark.parametrize("capacity", [7, 64, 319])
def test_model_append_edges(capacity):
    chunks = S.append_chunks(capacity)
    m = ReplayModel(buffer_size=capacity + 1, batch_size=1)
    fed = 0
    for n, (count, live) in zip(chunks, naive_ring(chunks, capacity)):
        m.add(S.payload(n, fed))
        fed += n
        assert m.count() == count == fed and m.live() == len(live)
        assert np.array_equal(m.live_seq(), np.array(live, np.int64))
        want = S.payload_of(live)
        assert np.array_equal(S.bits32(m.live_records()), S.bits32(want))
    assert any(n == 0 for n in chunks) and any(n == 3 * capacity + 5 for n in chunks)


def test_model_device_style_total():
    m = ReplayModel(buffer_size=65, batch_size=4)
    rec = S.payload(50)
    for total, took in ((20, 20), (50, 50), (70, 50), (0, 0), (-3, 0), (np.int64(7), 7)):
        before = m.count()
        m.add(rec, total=total)
        assert m.count() == before + took
        if took:
            assert np.array_equal(S.bits32(m.live_records()[-took:]), S.bits32(rec[:took]))


def test_model_sample():
    m = ReplayModel(buffer_size=101, batch_size=32, seed=9)
    with pytest.raises(PveError, match="fewer"):
        m.sample()
    m.add(S.payload(31))
    rows, act7, target, seq = m.sample(2, check=False)
    assert (seq == -1).all() and not rows.any() and not act7.any() and not target.any() and m.draws == 0 and m.status == 31
    assert rows.shape == (2, 32, 28) and act7.shape == (2, 32, 7) and target.shape == (2, 32) and seq.dtype == np.int64
    m.add(S.payload(1, 31))
    rows, act7, target, seq = m.sample()                      # L == batch: every live record exactly once
    assert np.array_equal(np.sort(seq[0]), np.arange(32)) and m.draws == 1 and m.status == 32
    m.add(S.payload(300, 32))                                 # wrapped
    twin = ReplayModel(buffer_size=101, batch_size=32, seed=9)
    twin.store, twin.written, twin.draws = m.store.copy(), m.written, m.draws
    rows, act7, target, seq = m.sample(3)
    assert m.draws == 4 and seq.min() >= 332 - 100 and seq.max() < 332
    for k in range(3):
        assert len(set(seq[k].tolist())) == 32
        one = twin.sample(1)
        for a, b in zip((rows, act7, target), one):
            assert np.array_equal(S.bits32(a[k]), S.bits32(b[0]))
        assert np.array_equal(seq[k], one[3][0])
        want = S.payload_of(seq[k])
        assert np.array_equal(S.bits32(np.concatenate([rows[k], act7[k], target[k][:, None]], axis=1)), S.bits32(want))
        assert np.array_equal(seq[k] - (332 - 100), replay.perm(9, 1 + k, 100, np.arange(32)))
    m.reset()
    assert m.count() == 0 and m.live() == 0 and m.draws == 0
    for kw in (dict(buffer_size=1), dict(buffer_size=10, batch_size=10), dict(buffer_size=10, batch_size=0)):
        with pytest.raises(ValueError):
            ReplayModel(**kw)


# ------------------------------------------------------------------ 6. the C ABI on a backend without the kernels
def test_entry_points_on_the_emulator():
    from pve_mcc_amd.arrivals import synthetic_arrivals
    lib = emulator_lib()
    for name in ("pve_replay_reset", "pve_replay_append", "pve_replay_sample"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert lib.pve_abi_version() == _capi.ABI_VERSION          # (version, constants, layout against the header: tests/test_binding_contract.py)
    header = open(os.path.join(ROOT, "include", "pve_env.h")).read()
    assert "replay_buffer.py:45-53" in header and "replay_buffer.py:20-23" in header
    assert "0x5245504C" in header and "0x41594D45" in header and (replay.TAG0, replay.TAG1) == (0x5245504C, 0x41594D45)
    b = make_batch(synthetic_arrivals(2, rate=500.0, horizon_s=20.0, seed=1), 2, 64, "emu", outputs=("obs_post", "flags"))
    keep = []

    def P(shape, dt, off=0):
        raw = np.zeros(int(np.prod(shape)) * np.dtype(dt).itemsize + 32, np.uint8)
        keep.append(raw)
        return raw.ctypes.data + (-raw.ctypes.data) % 16 + off

    cap, batch, nb = 100, 8, 3
    store, state, records, total = P((cap, 36), np.float32), P((4,), np.int64), P((50, 36), np.float32), P((1,), np.int64)
    rows, act7, target, seq = P((nb, batch, 28), np.float32), P((nb, batch, 7), np.float32), P((nb, batch), np.float32), P((nb, batch), np.int64)

    def rp(**kw):
        r = _capi.PveReplay()
        r.capacity, r.store, r.state, r.seed, r.block_threads = cap, store, state, 1, 0
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def append(r=None, h=b._h, rec=records, tot=total, n_max=50):
        return lib.pve_replay_append(h, C.byref(r) if r is not None else None, rec, tot, n_max)

    def sample(r=None, h=b._h, batch=batch, nb=nb, out=(rows, act7, target, seq)):
        return lib.pve_replay_sample(h, C.byref(r) if r is not None else None, batch, nb, *out)

    shared = [(dict(store=None), b"null"), (dict(state=None), b"null"), (dict(capacity=0), b"capacity"), (dict(capacity=1 << 31), b"capacity"),
              (dict(capacity=-5), b"capacity"), (dict(block_threads=100), b"block_threads"), (dict(block_threads=2048), b"block_threads"),
              (dict(block_threads=-64), b"block_threads"), (dict(store=store + 8), b"aligned"), (dict(state=state + 4), b"aligned")]
    for kw, word in shared:
        for fn in (lambda r: lib.pve_replay_reset(b._h, C.byref(r)), append, sample):
            assert fn(rp(**kw)) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    for fn in (lambda: lib.pve_replay_reset(None, C.byref(rp())), lambda: lib.pve_replay_reset(b._h, None), lambda: append(rp(), h=None),
               lambda: append(None), lambda: sample(rp(), h=None), lambda: sample(None)):
        assert fn() == -1 and b"null" in lib.pve_last_error()
    for kw, word in ((dict(n_max=-1), b"n_max"), (dict(rec=None), b"null records"), (dict(rec=records + 4), b"aligned"), (dict(tot=total + 4), b"aligned")):
        assert append(rp(), **kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    for kw, word in ((dict(batch=0), b"batch"), (dict(batch=cap + 1), b"batch"), (dict(nb=0), b"n_batches"), (dict(nb=-2), b"n_batches"),
                     (dict(batch=100, nb=1 << 25), b"n_batches"), (dict(out=(None, act7, target, seq)), b"null output"),
                     (dict(out=(rows, None, target, seq)), b"null output"), (dict(out=(rows, act7, None, seq)), b"null output"),
                     (dict(out=(rows, act7, target, None)), b"null output"), (dict(out=(rows + 4, act7, target, seq)), b"aligned"),
                     (dict(out=(rows, act7 + 8, target, seq)), b"aligned"), (dict(out=(rows, act7, target + 2, seq)), b"aligned"),
                     (dict(out=(rows, act7, target, seq + 4)), b"aligned")):
        assert sample(rp(), **kw) == -1 and word in lib.pve_last_error(), (kw, lib.pve_last_error())
    # valid arguments: the emulator has no replay kernels and says so (NULL total_dev and n_max = 0 are valid too)
    for fn in (lambda: lib.pve_replay_reset(b._h, C.byref(rp())), lambda: append(rp()), lambda: append(rp(), tot=None),
               lambda: append(rp(), rec=None, n_max=0), lambda: sample(rp()), lambda: sample(rp(block_threads=1024), batch=cap, nb=1)):
        assert fn() == -1 and b"backend has no replay kernels" in lib.pve_last_error()
    # the Python class asks the backend
    import torch
    m = ReplayMemory(b, buffer_size=cap + 1, batch_size=batch)
    assert m.capacity == cap and m.store.shape == (cap, 36) and m.state.dtype == torch.int64
    with pytest.raises(PveError, match="backend"):
        m.add(torch.zeros(5, 36))
    with pytest.raises(PveError, match="backend"):
        m.sample(check=False)
    with pytest.raises(PveError, match="float32"):
        m.add(torch.zeros(5, 35))
    with pytest.raises(PveError, match="n_batches"):
        m.sample(0)
    with pytest.raises(PveError, match="are on meta"):       # the full device is compared, not its type alone
        m.add(torch.zeros(5, 36, device="meta"))
    for kw in (dict(buffer_size=1), dict(buffer_size=10, batch_size=10)):
        with pytest.raises(PveError):
            ReplayMemory(b, **kw)

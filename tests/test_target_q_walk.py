"""The host model of k_target_q's row walk (tests/target_q_walk.py): consistent with itself on small inputs with many chunks per
wave, and the inputs of tests/test_gpu_streaming.py do reach the paths of the walk that only exist from a wave's second chunk on
(facts about the inputs, established here on the CPU; the GPU tests print the same counters next to their results)."""
import numpy as np
import pytest

from pve_mcc_amd import _capi
from tests import target_q_walk as W


def check_cover(w, ev):
    """every evaluated row in exactly one tile; per wave ascending; tiles full except a wave's last one"""
    want = np.flatnonzero(ev) if ev is not None else np.arange(w.n)
    got = []
    for gw, tiles in enumerate(w.tiles):
        rows = np.concatenate(tiles) if tiles else np.zeros(0, np.int64)
        assert np.all(np.diff(rows) > 0), "wave %d: rows out of order" % gw
        assert np.all((rows // W.CHUNK) % (w.grid * W.WAVES) == gw), "wave %d ran another wave's rows" % gw
        assert all(len(t) == W.TILE for t in tiles[:-1]) and all(1 <= len(t) <= W.TILE for t in tiles)
        got.append(rows)
    got = np.sort(np.concatenate(got))
    assert np.array_equal(got, want), "the tiles do not cover the evaluated rows exactly once"


def test_flag_constants_are_the_abi_s():
    assert (W.F_ALIVE, W.F_CTL, W.F_DONE, W.F_DELETED, W.F_LOCK) == (_capi.F_ALIVE, _capi.F_CTL, _capi.F_DONE, _capi.F_DELETED, _capi.F_LOCK)


def test_grid_mirror():
    # (n + 255) / 256 workgroups up to 256 CUs x per_cu: the sizes at which a wave gets a second chunk
    assert W.target_q_grid(1, 2) == 1 and W.target_q_grid(256, 2) == 1 and W.target_q_grid(257, 2) == 2
    assert W.target_q_grid(W.BOOT_PASS, 2) == 512 and W.target_q_grid(W.BOOT_PASS + 1, 2) == 512
    assert W.target_q_grid(W.CRITIC_PASS, 4) == 1024 and W.target_q_grid(10 ** 7, 4) == 1024
    assert W.BOOT_PASS == 131072 and W.CRITIC_PASS == 262144
    assert (W.N_BOOT_F32, W.N_BOOT_F64, W.N_CRITIC) == (393179, 278557, 524497)
    # up to one pass every wave has at most one chunk: the path the older tests pin
    w = W.walk(W.BOOT_PASS, None, 2)
    assert w.carry == 0 and w.straddle == 0 and w.wrapped_waves == 0 and w.max_pending == 64 and w.third_chunk_waves == 0


def test_model_is_self_consistent():
    rng = np.random.default_rng(1)
    seen = dict(carry=0, straddle=0, wrapped_waves=0, partial_tiles=0, flush_after_empty=0, idle_last=0)
    worst = 0
    for case in range(300):
        n = int(rng.integers(1, 2001))
        grid = int(rng.integers(1, 4))                          # 4 .. 12 waves: up to 8 chunks per wave
        kind = case % 4
        if kind == 0:
            ev = None
        else:
            density = rng.choice([0.0, 0.1, 0.5, 0.9, 1.0], (n + 63) // 64) if kind == 1 else np.full((n + 63) // 64, rng.random())
            ev = rng.random(n) < np.repeat(density, 64)[:n]
        w = W.walk(n, ev, grid=grid)                            # (raises on a ring overrun)
        check_cover(w, ev)
        assert len(w.tiles) == 4 * grid and w.max_pending <= W.TILE - 1 + W.CHUNK < W.TQ_RING
        worst = max(worst, w.max_pending)
        for k in seen:
            seen[k] += getattr(w, k)
    assert worst == 95 and all(v > 0 for v in seen.values()), (worst, seen)


def test_model_counts_what_it_says():
    # one wave's worth of hand-made chunks on a grid of one workgroup (chunks 0, 4, 8, ... belong to wave 0)
    n = 64 * 12
    ev = np.zeros(n, bool)
    ev[0:31] = True                       # chunk 0: 31 rows, no tile
    ev[4 * 64:4 * 64 + 64] = True         # chunk 4: entered with 31 pending (carry), 95 pending (max), two tiles, 31 left
    ev[8 * 64 + 5:8 * 64 + 64] = True     # chunk 8: carry again; writes 95 .. 153 straddle 127 -> 0; two tiles, 26 left
    w = W.walk(n, ev, grid=1)
    assert w.carry == 2 and w.straddle == 1 and w.max_pending == 95 and w.wrapped_waves == 1
    assert [len(t) for t in w.tiles[0]] == [32, 32, 32, 32, 26] and w.partial_tiles == 1
    assert w.flush_after_empty == 0 and w.idle_last == 3 and w.third_chunk_waves == 4
    ev[8 * 64:] = False                   # the final chunk of wave 0 accepts nothing: its 31 rows wait for the `last` pass
    w = W.walk(n, ev, grid=1)
    assert [len(t) for t in w.tiles[0]] == [32, 32, 31] and w.flush_after_empty == 1 and w.carry == 2
    assert np.array_equal(w.tiles[0][2], np.arange(4 * 64 + 33, 4 * 64 + 64))
    with pytest.raises(RuntimeError):     # (the overrun check is live: a ring that small would be overwritten)
        old, W.TQ_RING = W.TQ_RING, 64
        try:
            W.walk(n, ev, grid=1)
        finally:
            W.TQ_RING = old


@pytest.mark.parametrize("n", [W.N_BOOT_F32, W.N_BOOT_F64])
def test_bootstrap_inputs_reach_the_paths(n):
    flags = W.bootstrap_flags(n)
    ev = W.evaluated(flags)
    assert flags.shape == (n,) and flags.dtype == np.int32
    assert np.array_equal(ev, (flags & (_capi.F_CTL | _capi.F_DONE)) == _capi.F_CTL)
    assert set(np.unique(flags[~ev])) == set(W.MASKED) and set(np.unique(flags[ev])) == set(W.ACCEPTED)
    w = W.bootstrap_walk(n)
    check_cover(w, ev)
    c = W.counters(w)
    print("bootstrap walk, n = %d, grid %d: accepted share %.3f, %s" % (n, w.grid, ev.mean(), c))
    assert w.grid == 512 and W.target_q_grid(n, W.BOOT_PER_CU) == 512
    assert c["carry"] >= 1000
    assert c["straddle"] >= 100
    assert c["flush_after_empty"] >= 4
    assert c["partial_tiles"] >= 500
    assert c["max_pending"] >= 90
    assert 0.5 <= ev.mean() <= 0.8
    assert c["wrapped_waves"] >= 100 and n % 64 != 0
    # the waves of the cleared chunks end on them
    assert all(ch < w.n_chunks <= ch + 4 * w.grid for ch in W.CLEARED_CHUNKS)


def test_critic_input_reaches_the_paths():
    n = W.N_CRITIC
    w = W.critic_walk(n)
    check_cover(w, None)
    c = W.counters(w)
    print("critic walk, n = %d, grid %d: %s" % (n, w.grid, c))
    assert w.grid == 1024
    assert c["third_chunk_waves"] >= 4 and n % 64 != 0 and len(w.tiles[3][-1]) == n % 64
    assert c["wrapped_waves"] == c["third_chunk_waves"]          # flags = NULL: only whole chunks, the ring wraps with the third
    assert c["carry"] == 0 and c["max_pending"] == 64


def test_row_map_covers_the_fixture():
    idx = W.row_map(W.N_BOOT_F64, 301)
    assert idx.shape == (W.N_BOOT_F64,) and idx.min() == 0 and idx.max() == 300
    assert np.array_equal(idx[:301], np.arange(301)) and np.array_equal(idx[-301:], np.arange(301))
    assert len(np.unique(idx[301:-301])) == 301

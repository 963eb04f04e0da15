"""A host model of the row walk of k_target_q (csrc/pve_critic.h), in plain Python / NumPy, and the inputs the GPU tests of that
walk use (tests/test_gpu_streaming.py).  The kernel states the walk under `#if defined(__HIPCC__)` only; this file is its CPU
statement, held to itself by tests/test_target_q_walk.py.

The walk: `grid` workgroups of 4 waves; wave gw = 4 * block + wave takes the 64-row chunks gw, gw + 4 * grid, ... and, one step
behind its last chunk, ONE `last` pass.  The accepted rows of a chunk are appended to the wave's ring of 128 entries at
(head + npend + rank) & 127, rank = the row's position among the accepted rows of the chunk.  After every chunk a tile of
min(npend, 32) rows, read from head on, runs while npend >= 32; in the `last` pass while npend > 0."""
import functools

import numpy as np

from pve_mcc_amd._capi import F_ALIVE, F_CTL, F_DELETED, F_DONE, F_LOCK     # noqa: F401  (PVE_F_* of include/pve_env.h)

TQ_RING = 128                     # TQ_RING of csrc/pve_critic.h
CHUNK, TILE, WAVES = 64, 32, 4

BOOT_PER_CU, CRITIC_PER_CU = 2, 4                 # launch_bootstrap_q / launch_critic of csrc/pve_hip.hip
BOOT_PASS = 256 * BOOT_PER_CU * WAVES * CHUNK     # rows one pass of the full bootstrap grid covers: 131 072
CRITIC_PASS = 256 * CRITIC_PER_CU * WAVES * CHUNK     # 262 144
N_BOOT_F32 = 3 * BOOT_PASS - 37                   # 393 179: every wave three chunks, the last chunk partial
N_BOOT_F64 = 2 * BOOT_PASS + 64 * 256 + 29        # 278 557: 256 waves take a third chunk, the last chunk holds 29 rows
N_CRITIC = 2 * CRITIC_PASS + 3 * 64 + 17          # 524 497: 4 waves take a third chunk, the last chunk holds 17 rows
CLEARED_CHUNKS = tuple(range(4096 + 40, 4096 + 48))   # the final real chunks of waves 40 .. 47 at both bootstrap sizes


def target_q_grid(n, per_cu):
    """Workgroups of a k_target_q launch: `target_q_grid` of csrc/pve_hip.hip -- as many as stay resident (256 CUs x per_cu),
    never more than there are pieces of 256 rows."""
    want, cap = (n + 255) // 256, 256 * per_cu
    return int(want if want < cap else cap)


def evaluated(flags):
    """the rows k_target_q evaluates: PVE_F_CTL set and PVE_F_DONE clear"""
    return (np.asarray(flags) & (F_CTL | F_DONE)) == F_CTL


class Walk:
    """tiles[gw] = the ordered list of row-index arrays wave gw evaluates; counters: see walk()"""


def walk(n, ev=None, per_cu=BOOT_PER_CU, grid=None):
    """Replay the walk of k_target_q over n rows.  ev: bool [n], the rows to evaluate (None: every row -- flags = NULL);
    grid: workgroups (None: target_q_grid(n, per_cu)).  Returns a Walk with
      tiles              per wave, the tiles in the order the wave runs them
      carry              chunks entered with 1 .. 31 rows pending
      straddle           chunks whose ring writes cross index 127 -> 0
      wrapped_waves      waves whose ring wrapped (more than 128 entries written: an index is used a second time)
      max_pending        the largest npend
      partial_tiles      tiles with fewer than 32 rows
      flush_after_empty  `last`-pass tiles of waves whose final real chunk accepted nothing while rows were pending
      idle_last          waves with nothing pending at `last`
      third_chunk_waves  waves that take three or more chunks
    A ring entry overwritten before its tile ran raises RuntimeError."""
    n = int(n)
    grid = target_q_grid(n, per_cu) if grid is None else int(grid)
    n_chunks, stride = (n + CHUNK - 1) // CHUNK, grid * WAVES
    w = Walk()
    w.n, w.grid, w.n_chunks, w.tiles = n, grid, n_chunks, []
    w.carry = w.straddle = w.wrapped_waves = w.max_pending = w.partial_tiles = w.flush_after_empty = w.idle_last = 0
    w.third_chunk_waves = 0
    lane = np.arange(CHUNK)
    for gw in range(stride):
        ring = np.full(TQ_RING, -1, np.int64)
        head = npend = taken = written = 0
        empty_final = False
        mine = []
        c = gw
        while c < n_chunks + stride:
            last = c >= n_chunks
            if not last:
                taken += 1
                i = c * CHUNK + lane
                inside = i < n
                keep = inside if ev is None else inside & ev[np.minimum(i, n - 1)]
                acc = i[keep]
                if 1 <= npend < TILE:
                    w.carry += 1
                empty_final = len(acc) == 0 and npend > 0        # (overwritten by every later real chunk of the wave)
                if npend + len(acc) > TQ_RING:
                    raise RuntimeError("wave %d: ring overrun, %d pending + %d new" % (gw, npend, len(acc)))
                pos = (head + npend + np.arange(len(acc))) & (TQ_RING - 1)
                if len(acc) and pos[-1] < pos[0]:
                    w.straddle += 1
                ring[pos] = acc
                npend += len(acc)
                written += len(acc)
                w.max_pending = max(w.max_pending, npend)
            elif npend == 0:
                w.idle_last += 1
            while npend >= TILE or (last and npend > 0):
                cnt = min(npend, TILE)
                mine.append(ring[(head + np.arange(cnt)) & (TQ_RING - 1)].copy())
                w.partial_tiles += cnt < TILE
                w.flush_after_empty += bool(last and empty_final)
                head = (head + cnt) & (TQ_RING - 1)
                npend -= cnt
            c += stride
        w.wrapped_waves += written > TQ_RING
        w.third_chunk_waves += taken >= 3
        w.tiles.append(mine)
    return w


def counters(w):
    return {k: int(getattr(w, k)) for k in ("carry", "straddle", "wrapped_waves", "max_pending", "partial_tiles", "flush_after_empty",
                                            "idle_last", "third_chunk_waves")}


# ------------------------------------------------------------------ the inputs of the GPU tests (one definition for both sides)
MASKED = (0, F_ALIVE, F_ALIVE | F_CTL | F_DONE, F_ALIVE | F_DONE | F_DELETED)     # as test_gpu_bootstrap_masking_and_bounds
ACCEPTED = (F_ALIVE | F_CTL, F_ALIVE | F_CTL | F_LOCK | (3 << 8))


@functools.lru_cache(maxsize=None)
def bootstrap_flags(n, seed=7):
    """int32 [n] flags of the big bootstrap call: an acceptance density per 64-row chunk from {0.25, 0.5, 0.85, 1.0}, accepted
    rows ALIVE|CTL (some with LOCK and a collision count), rejected rows one of the masked values, chunks CLEARED_CHUNKS
    without an accepted row."""
    rng = np.random.default_rng(seed)
    n_chunks = (n + CHUNK - 1) // CHUNK
    density = rng.choice(np.array([0.25, 0.5, 0.85, 1.0]), n_chunks)
    accept = rng.random(n_chunks * CHUNK) < np.repeat(density, CHUNK)
    for c in CLEARED_CHUNKS:
        accept[c * CHUNK:(c + 1) * CHUNK] = False
    yes = rng.choice(np.array(ACCEPTED, np.int32), n_chunks * CHUNK)
    no = rng.choice(np.array(MASKED, np.int32), n_chunks * CHUNK)
    flags = np.where(accept, yes, no)[:n].astype(np.int32)
    flags.setflags(write=False)
    return flags


@functools.lru_cache(maxsize=None)
def row_map(n, n_fixture, seed=11):
    """int64 [n] indices into a fixture of n_fixture rows: a fixed-seed map whose first and last n_fixture entries walk the
    fixture in order (so every fixture row, the degenerate states at its end included, occurs)."""
    idx = np.random.default_rng(seed).integers(0, n_fixture, n, dtype=np.int64)
    idx[:n_fixture] = np.arange(n_fixture)
    idx[n - n_fixture:] = np.arange(n_fixture)
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def bootstrap_walk(n):
    """the walk of the big bootstrap call over n rows"""
    return walk(n, evaluated(bootstrap_flags(n)), BOOT_PER_CU)


@functools.lru_cache(maxsize=None)
def critic_walk(n):
    return walk(n, None, CRITIC_PER_CU)

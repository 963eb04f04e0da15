"""CPU: RANK on pairs of list entries (csrc/pve_tick_core.h, ph_rank_pairs) through the emulator's HOME block -- the pool of the
kernel (PVE_EMU_HOME=1) and the smaller one that sends ordinary traffic through the multi-pass form (=2) -- against the sequential
oracle, every tick, every field (tests/rank_pairs_scenarios.py).  The emulator reports what the streams made RANK do: the list
lengths it ranked, the fix-ups that the second entry of a pair ran because its partner shares its distance, the other fix-ups,
the passes -- in a build of its own (tests/emu_diag: the sources of tests/emu with the counters of PVE_EMU_DIAG and a probe of RANK
alone)."""
import ctypes as C

import pytest

from tests import rank_pairs_scenarios as R
from tests.rank_pairs_scenarios import diag_emulator_lib as emulator_lib

BACKEND = "emu"
MODES = [1, 2]


def _diagnostics():
    """(list-length histogram, fix-ups [inside a pair, others], most passes, most entries) since the last call"""
    lib = emulator_lib()
    hist, ties = (C.c_int * 64)(), (C.c_int * 2)()
    lib.pve_emu_list_lengths(hist)
    lib.pve_emu_rank_ties(ties)
    lib.pve_emu_max_passes.restype = lib.pve_emu_max_entries.restype = C.c_int
    return list(hist), list(ties), int(lib.pve_emu_max_passes()), int(lib.pve_emu_max_entries())


def _run(monkeypatch, mode, case):
    monkeypatch.setenv("PVE_EMU_HOME", str(mode))
    with R.diag_emulator():
        _diagnostics()
        run = R.check_queue_kernel_vs_oracle(BACKEND, case)
        hist, ties, passes, entries = _diagnostics()
    assert passes >= 1, "the HOME block did not run"
    return run, hist, ties, passes, entries


@pytest.mark.parametrize("mode", MODES)
def test_rank_pairs_traffic_from_empty_lists_of_every_small_length(monkeypatch, mode):
    _run_, hist, _ties, _passes, _entries = _run(monkeypatch, mode, R.TRAFFIC)
    # an odd list ends in a pair of one entry; 0, 1 and 2 are the lists without a pair, of one half pair and of one whole pair
    assert hist[0] > 0 and hist[1] > 0 and hist[2] > 0, hist
    assert sum(hist[3::2]) > 0 and sum(hist[4::2]) > 0, hist
    assert any(hist[n] > 0 for n in range(9, 64, 2)), "no odd list long enough for a full round of 8 reads: %s" % hist


@pytest.mark.parametrize("mode", MODES)
def test_rank_pairs_symmetric_lanes_equal_distances_across_pairs(monkeypatch, mode):
    """(equal distances INSIDE a pair never come out of traffic: test_rank_pairs_probe_equal_distances_inside_a_pair)"""
    run, _hist, ties, _passes, _entries = _run(monkeypatch, mode, R.SYMMETRIC)
    assert R.equal_distance_pairs(run, R.SYMMETRIC) > 0
    assert ties[1] > 0, "no run of equal distances: %s" % ties


@pytest.mark.parametrize("mode", MODES)
def test_rank_pairs_quantised_tape_near_ties(monkeypatch, mode):
    run, hist, _ties, _passes, _entries = _run(monkeypatch, mode, R.QUANTISED)
    assert run.max_ctl > 20 and sum(hist[1::2]) > 0, (run.max_ctl, hist)


@pytest.mark.parametrize("mode", MODES)
def test_rank_pairs_full_intersection_multi_pass(monkeypatch, mode):
    run, _hist, _ties, passes, entries = _run(monkeypatch, mode, R.FULL)
    assert run.max_ctl > 80 and sum(run.overflow) > 0, (run.max_ctl, run.overflow)
    assert passes >= 2 and entries > 304, "a full intersection must overflow the kernel's pool of 304 entries: %d passes, %d entries" % (passes, entries)


def test_rank_pairs_one_ulp_apart_stream_of_the_parity_suite():
    """the 8-lane stream behind test_gpu_left_neighbours_one_ulp_apart_share_a_distance (general-geometry kernel: per-route
    lists, a RANK of its own), on the emulator"""
    from tests import scenarios
    scenarios.check_geo_fuzz_vs_oracle(BACKEND, 8, n_envs=24, capacity=128, ticks=160, rate=1600.0, seed=3110, quantize=1.0)


def _probe(home, lens, nown, vd, slot, ticks=77, stale=0):
    import numpy as np
    lib = emulator_lib()
    n = int(sum(lens))
    order, mypos = np.full(max(n, 1), -7, np.int32), np.full(128, -7, np.int32)
    ip, dp, bp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    lib.pve_emu_rank_probe.restype = C.c_int
    lib.pve_emu_rank_probe.argtypes = [C.c_int, ip, ip, dp, bp, C.c_int, C.c_int, ip, ip]
    lens, nown = np.asarray(lens, np.int32), np.asarray(nown, np.int32)
    vd, slot = np.ascontiguousarray(vd, np.float64), np.ascontiguousarray(slot, np.uint8)
    got = lib.pve_emu_rank_probe(home, lens.ctypes.data_as(ip), nown.ctypes.data_as(ip), vd.ctypes.data_as(dp), slot.ctypes.data_as(bp),
                                 ticks, stale, order.ctypes.data_as(ip), mypos.ctypes.data_as(ip))
    assert got == n, (got, n)
    return order[:n], mypos


def _expected(lens, nown, vd, slot):
    """the reference's stable sort of every list by distance (ref :271) = by (vd, slot); unchosen entries (+inf) are not listed"""
    import numpy as np
    order, mypos, lo = np.full(int(sum(lens)), -1, np.int32), np.full(128, -1, np.int32), 0
    for d, n in enumerate(lens):
        fin = [q for q in range(n) if np.isfinite(vd[lo + q])]
        fin.sort(key=lambda q: (vd[lo + q], slot[lo + q]))
        order[lo:lo + len(fin)] = fin
        for pos, q in enumerate(fin):
            if q < nown[d]:
                mypos[slot[lo + q]] = pos
        lo += n
    return order, mypos


def _random_lists(rng, pool, values, p_inf):
    """twelve lists of 0 .. 40 entries (every small and some odd lengths), distances drawn from a handful of values -- runs of
    equal distances everywhere, neighbours included --, unchosen entries behind the own-lane segment"""
    import numpy as np
    while True:
        lens = rng.choice([0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 23, 24, 31, 40], size=12)
        nown = np.array([rng.integers(0, min(n, 10) + 1) for n in lens])
        if lens.sum() <= pool and nown.sum() <= 128:
            break
    own_slots = rng.permutation(128)[:nown.sum()]
    vd, slot, k = [], [], 0
    for n, m in zip(lens, nown):
        mine = own_slots[k:k + m]
        k += m
        others = rng.permutation(np.setdiff1d(np.arange(128), mine))[:n - m]
        slot += list(mine) + list(others)
        v = rng.choice(values, size=n)
        v[m:][rng.random(n - m) < p_inf] = np.inf
        vd += list(v)
    return lens, nown, np.array(vd, np.float64), np.array(slot, np.uint8)


@pytest.mark.parametrize("home", [0, 1])
def test_rank_pairs_probe_equal_distances_inside_a_pair(home):
    """RANK alone on hand-made lists.  Traffic never files two vehicles with the same distance NEXT to each other (neighbours in a
    list are followers of one lane), so the case of a lane whose own two entries tie -- the second claim meets the first one's tag
    -- is driven here: against the stable sort by (distance, slot), positions of every entry and mypos of every own entry."""
    import numpy as np
    rng = np.random.default_rng(20 + home)
    _diagnostics()
    # the smallest cases by hand: a pair that ties, an odd list whose last entry ties with the pair before it, ties with +inf between
    inf = np.inf
    for lens0, vd in (([2], [5.0, 5.0]), ([3], [5.0, 5.0, 5.0]), ([3], [7.0, 5.0, 5.0]), ([4], [5.0, inf, 5.0, 5.0]), ([1], [5.0]),
                      ([5], [3.0, 3.0, inf, inf, 3.0]), ([9], [1.0] * 9), ([17], [2.0, 1.0] * 8 + [1.0])):
        for nown0 in (0, 1, lens0[0]):
            if any(np.isinf(vd[:nown0])):
                continue
            lens, nown = np.array(lens0 + [0] * 11), np.array([nown0] + [0] * 11)
            for slot in (np.arange(lens0[0]), np.arange(lens0[0])[::-1] + 60):
                for stale in (0, 1):
                    order, mypos = _probe(home, lens, nown, vd, slot.astype(np.uint8), stale=stale)
                    want_o, want_m = _expected(lens, nown, np.array(vd), slot)
                    assert np.array_equal(order, want_o) and np.array_equal(mypos, want_m), (lens0, vd, nown0, slot, stale, order, want_o, mypos, want_m)
    _hist, ties, _p, _e = _diagnostics()
    assert ties[0] > 0 and ties[1] > 0, ties
    seen = set()
    for trial in range(300):
        values = rng.choice([1.5, 2.5, 2.5000000000000004, 3.0, 8.0, 1e-300, 0.0, 77.25], size=rng.integers(1, 8))
        lens, nown, vd, slot = _random_lists(rng, 304 if home else 640, values, rng.choice([0.0, 0.3, 0.9]))
        order, mypos = _probe(home, lens, nown, vd, slot, ticks=int(rng.integers(0, 1 << 20)), stale=trial & 1)
        want_o, want_m = _expected(lens, nown, vd, slot)
        assert np.array_equal(order, want_o), (trial, lens, nown)
        assert np.array_equal(mypos, want_m), (trial, lens, nown)
        seen.update(int(n) for n in lens)
    _hist, ties, _p, _e = _diagnostics()
    assert ties[0] > 100 and ties[1] > 100, ties
    assert {0, 1, 2, 3, 9, 17}.issubset(seen), seen

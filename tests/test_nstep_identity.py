"""The n-step pass by vehicle identity, CPU side.

1. tests/nstep_by_vehicle.py (the reference's per-vehicle buffers, no slots) against tests/golden/nstep_ref.npz, the
   transitions the unmodified reference emitted under main.py:243-266: bit for bit, both gammas.  Without this pin the model is
   not a reference.
2. tests/nstep_identity_scenarios.py on the CPU emulator, every scenario and both launch forms: the roll-out's blocks through
   nstep.py against that model fed from the oracle (B), and the same roll-out into a ring filled with 0xFF (C).  The emulator runs
   the product's own ph_final, so the block contract the pass relies on -- and the scenarios' vacuity conditions -- are proven
   here without a GPU; tests/test_gpu_nstep_layouts.py runs the same bodies on the kernels."""
import numpy as np
import pytest

from pve_mcc_amd import nstep
from tests import nstep_identity_scenarios as N
from tests import nstep_scenarios as S
from tests.nstep_by_vehicle import VehicleBuffers


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def fed_from_the_fixture(gamma, tail=False):
    """the model fed with the fixture's controlled vehicles, tick by tick, keyed by ids[t, 0, slot]"""
    z, cur = S.load_reference_fixture()
    T, K, window = int(z["T"]), int(z["K"]), int(z["window"])
    model = VehicleBuffers(gamma, window, tail=tail)
    ids, flags, reward, q = z["ids"], z["flags"], z["reward"], z["q"]         # (an .npz member is decompressed on every access)
    obs_first, act7 = z["obs_first"][0], cur["state_pre"][:, 0, :, :, 2]
    for t in range(T):
        rows = obs_first if t == 0 else cur["obs_post"][t - 1, 0]
        for s in range(K):                                   # 12 lanes: slot order is the reference's `ids` order
            f = int(flags[t, 0, s])
            if f & S.F_CTL:
                model.feed(t, ids[t, 0, s], rows[s], act7[t, s], reward[t, 0, s], q[t, 0, s], f & S.F_DONE)
    return z, cur, model, window


@pytest.mark.parametrize("gi", [0, 1])
def test_model_reproduces_the_reference_fixture(gi):
    z, cur, model, window = fed_from_the_fixture(S.load_reference_fixture()[0]["gammas"][gi])
    em_tick, em_id, em_row, em_act, em_target = z["em_tick"], z["em_id"], z["em_row"], z["em_act"], z["em_target"]
    M = len(em_tick)
    assert M > 0 and len(model.out) == M
    # the same emissions in the same order (so the same multiset of keys), every value bit for bit
    n_done = n_boot = 0
    for i, em in enumerate(model.out):
        assert (em.tick, em.vid) == (int(em_tick[i]), int(em_id[i])), i
        assert np.array_equal(bits(em.row), bits(em_row[i])) and np.array_equal(bits(em.act7), bits(em_act[i])), i
        assert bits(em.target) == bits(em_target[gi, i]), (i, em.target, em_target[gi, i])
        assert em.boot != em.done and em.entries <= window
        n_done += em.done
        n_boot += em.boot
    assert len(model.emitted()) == M and n_done > 0 and n_boot > 0


def test_model_tail_is_the_tail_of_the_pass_on_the_fixture():
    """the reference drops the younger entries of a vehicle that is Done, so its fixture cannot pin tail=True: here the model's
    tail emissions against NSTEP_TAIL of nstep.py (== the header, tests/test_nstep.py) on the fixture's blocks, by vehicle id"""
    gamma = S.load_reference_fixture()[0]["gammas"][0]
    z, cur, model, window = fed_from_the_fixture(gamma, tail=True)
    want = model.emitted()                                    # (closing tick, vehicle id, entries used)
    ids, obs_first, q = z["ids"], z["obs_first"], z["q"]
    tgt, code, _ = nstep.scan(cur, gamma, window, obs_first=obs_first, q=q, tail=True)
    c, e, s = nstep.order(code)
    got = {}
    for t, sl in zip(c.tolist(), s.tolist()):
        n = int(code[t, 0, sl]) & 0xFF
        key = (t + n - 1, int(ids[t, 0, sl]), n)
        assert key not in got
        got[key] = (tgt[t, 0, sl], int(code[t, 0, sl]))
    assert set(got) == set(want) and len(want) > len(z["em_tick"])
    for key, em in want.items():
        target, cw = got[key]
        assert bits(target) == bits(em.target) and (bool(cw & nstep.BOOT), bool(cw & nstep.DONE)) == (em.boot, em.done), key
    assert sum(1 for em in want.values() if em.done and em.entries < window) > 0


def test_model_tail_and_slide():
    """one vehicle by hand: a full window slides, Done drops the younger entries, tail emits them"""
    for tail in (False, True):
        m = VehicleBuffers(0.5, window=3, tail=tail)
        for t in range(5):                                   # vehicle 7: rewards 1, 2, 4, 8, 16, Done at tick 4
            m.feed(t, 7, np.full(28, float(t)), np.full(7, 10.0 + t), float(1 << t), np.float32(100.0), t == 4)
        got = [(e.tick, e.entries, e.boot, e.done, float(e.target), float(e.row[0]), float(e.act7[0])) for e in m.out]
        want = [(2, 3, True, False, 1 + 0.5 * (2 + 0.5 * (4 + 0.5 * 100.0)), 0.0, 10.0),
                (3, 3, True, False, 2 + 0.5 * (4 + 0.5 * (8 + 0.5 * 100.0)), 1.0, 11.0),
                (4, 3, False, True, 4 + 0.5 * (8 + 0.5 * 16.0), 2.0, 12.0)]
        if tail:
            want += [(4, 2, False, True, 8 + 0.5 * 16.0, 3.0, 13.0), (4, 1, False, True, 16.0, 4.0, 14.0)]
        assert got == want and not m.buf


@pytest.mark.parametrize("form", sorted(N.LAUNCH_FORMS))
@pytest.mark.parametrize("name", sorted(N.SCENARIOS))
def test_emulated_identity_and_dirty_ring(name, form, monkeypatch):
    if N.SCENARIOS[name]["capacity"] == 256:                 # (the 256-slot kernels' emulator: tests/emu_wide)
        from tests import hip_adapter
        from tests.test_capacity256 import wide_lib
        lib = wide_lib()
        monkeypatch.setattr(hip_adapter, "emulator_lib", lambda: lib)
    clean = N.rollout(name, "emu", **N.LAUNCH_FORMS[form])
    N.check_identity(name, "emu", clean)
    dirty = N.rollout(name, "emu", dirty=True, **N.LAUNCH_FORMS[form])
    left = N.check_dirty(name, clean, dirty)
    print("%s %s: elements still holding the fill: %s" % (name, form, left))

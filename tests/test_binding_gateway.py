"""The Python binding's one gateway to the library (BatchedIntersections._call), its stream rule and the shared argument
checks (pve_mcc_amd/_args.py), without a GPU: on the CPU emulator, which checks every entry point's arguments like the product
and says "backend" where it has no kernels -- so a call whose arguments arrived intact is told from one whose did not.
The orderings the stream rule protects are checked on the device in tests/test_gpu_binding_gateway.py."""
import collections
import ctypes as C
import glob
import os
import re
import types

import numpy as np
import pytest
import torch

from pve_mcc_amd import Learner, PrioritizedReplayMemory, PveError, ReplayMemory, _capi
from pve_mcc_amd._capi import check
from pve_mcc_amd.arrivals import synthetic_arrivals
from pve_mcc_amd.batched import BatchedIntersections
from tests.hip_adapter import emulator_lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(ROOT, "pve-mcc_for_unsignalized_intersection_amd")
OUTS = ("obs_post", "obs_pre", "reward", "flags", "new_slot", "env_out")


class CountingLib:
    """The emulator library with every attribute look-up and every pve_set_stream call counted"""

    def __init__(self, lib):
        self._lib, self.lookups, self.binds = lib, collections.Counter(), 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        self.lookups[name] += 1
        if name != "pve_set_stream":
            return fn

        def counted(*args):
            self.binds += 1
            return fn(*args)
        return counted


def batch(own_stream, lib=None, outputs=OUTS):
    """2 environments x 64 slots on the emulator: with a stream of its own (a stand-in object, the CPU has none) or, created
    with stream=None, following the current one"""
    arr = synthetic_arrivals(2, rate=1000.0, horizon_s=40.0, seed=5)
    stream = types.SimpleNamespace(cuda_stream=0) if own_stream else None
    return BatchedIntersections(2, 64, arr, device="cpu", outputs=outputs, stream=stream, _lib=lib or emulator_lib())


def replay_struct(b, cap=16, **kw):
    store, state = torch.zeros(cap, 36), torch.zeros(_capi.REPLAY_STATE_WORDS, dtype=torch.int64)
    rp = _capi.PveReplay(capacity=cap, store=store.data_ptr(), state=state.data_ptr(), seed=1, block_threads=0)
    for k, v in kw.items():
        setattr(rp, k, v)
    return rp, (store, state)


def last_error(lib):
    return lib.pve_last_error().decode()


# ------------------------------------------------------------------ 1. the gateway
@pytest.mark.parametrize("own_stream", [True, False], ids=["own_stream", "current_stream"])
def test_gateway_converts_tensor_none_and_structure(own_stream):
    from oracle.actor_np import flat_weights, load_weights
    lib = emulator_lib()
    b, twin = batch(own_stream), batch(own_stream)
    # scalars pass as they are (pve_set_action_noise): accepted where today's spelling is, refused with its words where not
    assert b._call("pve_set_action_noise", 0.0, 12345, 77, bind=False) is None
    assert lib.pve_set_action_noise(twin._h, 0.0, 12345, 77) == 0
    assert lib.pve_set_action_noise(twin._h, 0.2, 7, 0) == -1
    want = last_error(lib)
    with pytest.raises(PveError) as e:
        b._call("pve_set_action_noise", 0.2, 7, 0, bind=False)
    assert str(e.value) == "pve_set_action_noise failed (-1): " + want and "backend" in want
    # tensors as data_ptr(), None as a null pointer (pve_actor_forward's optional weights): the same actions as today's spelling
    w = flat_weights(load_weights())
    for x in (b, twin):
        x.reset()
        x.set_actor(w)
        for _ in range(40):
            x.step_with_actor()
    got = torch.full((2, 64), 7.0, dtype=torch.float64)
    b._call("pve_actor_forward", None, b.obs, got)
    ref = torch.full((2, 64), 7.0, dtype=torch.float64)
    check(lib, lib.pve_actor_forward(twin._h, None, C.c_void_p(twin.obs.data_ptr()), C.c_void_p(ref.data_ptr())), "pve_actor_forward")
    assert torch.equal(b.obs, twin.obs) and np.array_equal(got.numpy().view(np.uint64), ref.numpy().view(np.uint64))
    assert int((got != 0).sum()) > 0 and not bool((got == 7.0).any())
    assert torch.equal(b.act(), got)                         # (and the method that goes through it)
    # a structure by reference (pve_replay_reset with a PveReplay): a valid one passes the argument checks and reaches the
    # backend, which has no replay kernels; a field the library refuses is refused by name -- both as today's spelling reports
    for kw, word in ((dict(), "backend has no replay kernels"), (dict(capacity=-5), "capacity")):
        rp, keep = replay_struct(b, **kw)
        assert lib.pve_replay_reset(twin._h, C.byref(rp)) == -1
        want = last_error(lib)
        with pytest.raises(PveError) as e:
            b._call("pve_replay_reset", rp)
        assert str(e.value) == "pve_replay_reset failed (-1): " + want and word in want
    # an optional pointer passed as None (pve_replay_append's total) is valid; None for the records is "null records"
    rp, keep = replay_struct(b)
    records = torch.zeros(5, 36)
    for args, spelled, word in (((records, None, 5), (C.c_void_p(records.data_ptr()), C.c_void_p(0), 5), "backend has no replay kernels"),
                                ((None, None, 5), (C.c_void_p(0), C.c_void_p(0), 5), "null records")):
        assert lib.pve_replay_append(twin._h, C.byref(rp), *spelled) == -1
        want = last_error(lib)
        with pytest.raises(PveError) as e:
            b._call("pve_replay_append", rp, *args)
        assert str(e.value) == "pve_replay_append failed (-1): " + want and word in want


@pytest.mark.parametrize("own_stream", [True, False], ids=["own_stream", "current_stream"])
def test_gateway_failure_unknown_name_stream_rule_and_cache(own_stream):
    lib = CountingLib(emulator_lib())
    b = batch(own_stream, lib)
    # a failing call: PveError that starts with the entry point's name and carries pve_last_error(), as check() words it
    with pytest.raises(PveError) as e:
        b._call("pve_read_env", 99, _capi.PveEnvInfo(), bind=False)
    assert str(e.value).startswith("pve_read_env failed (-1): ") and str(e.value).endswith(last_error(lib)) and last_error(lib)
    # an unknown name is an error at the call
    with pytest.raises(AttributeError):
        b._call("pve_no_such_entry_point")
    # the stream rule: a batch that follows the current stream re-binds it before every call that may launch, a batch with a
    # stream of its own never does (pve_create bound it); bind=False calls leave the handle's stream alone either way
    lib.binds = 0
    b._call("pve_reset")
    b._call("pve_synchronize", bind=False)
    b._call("pve_reset")
    assert lib.binds == (0 if own_stream else 2)
    b.reset(), b.step(), b.scene_update(), b.compact(), b.set_actor(np.zeros(_capi.PVE_ACTOR_N_WEIGHTS, np.float32)), b.act(), b.step_with_actor()
    assert lib.binds == (0 if own_stream else 9)
    b.synchronize(), b.metrics(), b.read_env(0), b.read_vehicles(0), b.state_field("id"), b.set_exploration(0.0, 3), b.last_variant()
    assert lib.binds == (0 if own_stream else 9)
    # every entry point is looked up in the library once per handle: the bound function is kept
    n = lib.lookups["pve_reset"]
    for _ in range(3):
        b._call("pve_reset")
    assert n == 1 and lib.lookups["pve_reset"] == 1 and lib.lookups["pve_synchronize"] == 1 and set(b._fns) >= {"pve_reset", "pve_synchronize"}


# ------------------------------------------------------------------ 2. the package's sources: who calls the library directly
# (file, entry point) -> number of sites, with the reason each states where it stands
DIRECT = {
    ("batched.py", "pve_default_config"): 1,            # no handle, no status
    ("batched.py", "pve_workspace_bytes"): 1,           # a size query: no handle, no status
    ("batched.py", "pve_create"): 1,                    # makes the handle
    ("batched.py", "pve_destroy"): 1,                   # ends it
    ("batched.py", "pve_set_stream"): 1,                # the gateway's own stream rule (_bind_stream)
    ("batched.py", "pve_step_all"): 1,                  # the stepping calls, which bench.py times: step()
    ("batched.py", "pve_step_all_actor"): 1,            # ... step_with_actor()
    ("batched.py", "pve_step_many"): 3,                 # ... step_many() (with and without a trajectory), prepare_step_many()'s callable
    ("batched.py", "pve_debug_last_launch"): 1,         # returns the kind, not a status
    ("replay.py", "pve_prio_scratch_bytes"): 1,         # a size query: no handle, no status
}


def test_direct_library_calls_are_the_listed_exceptions():
    found = collections.Counter()
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) >= 13
    for path in files:
        for m in re.finditer(r"(?:\.lib\.pve_|lib\.pve_)(\w+)", open(path).read()):
            found[(os.path.basename(path), "pve_" + m.group(1))] += 1
    assert dict(found) == DIRECT
    # (_capi.py's own two, on the library it is loading: the ABI version and the error text check() reads)
    capi = open(os.path.join(PKG, "_capi.py")).read()
    assert sorted(set(re.findall(r"\bL\.(pve_\w+)\(", capi))) == ["pve_abi_version", "pve_last_error"]
    # the size query nobody needs yet stays uncalled rather than called around the gateway
    assert not any("pve_stats_scratch_bytes(" in open(p).read() for p in files)
    # and the wrappers the gateway replaced are gone
    for name, words in (("replay.py", ("_pcall", "def _call", "c_void_p")), ("learner.py", ("def _call", "c_void_p"))):
        text = open(os.path.join(PKG, name)).read()
        assert not any(w in text for w in words), name


# ------------------------------------------------------------------ 3. the argument checks: every refusal, in the words of before
def refused(message, fn, *args, **kw):
    with pytest.raises(PveError) as e:
        fn(*args, **kw)
    assert str(e.value) == message, str(e.value)


def other_device_tensor(*shape, dtype=torch.float32):
    """a tensor on another device TYPE than the CPU batch's, where one exists without a GPU (torch's meta device)"""
    try:
        return torch.empty(*shape, dtype=dtype, device="meta")
    except Exception:
        return None


def test_argument_refusals_of_the_batch():
    b = batch(False, outputs=OUTS + ("state_pre",))
    f64, f32, i32 = torch.float64, torch.float32, torch.int32
    rows, act7 = torch.zeros(3, 28, dtype=f64), torch.zeros(3, 7)
    # --- inputs: trailing shape, emptiness, full shape (the dtype is converted, as before)
    refused("rows must be [..., 28] and not empty", b.critic_q, torch.zeros(3, 27, dtype=f64), act7)
    refused("rows must be [..., 28] and not empty", b.critic_q, torch.zeros(0, 28, dtype=f64), torch.zeros(0, 7))
    refused("rows must be [..., 28] and not empty", b.critic_q, torch.zeros((), dtype=f64), act7)
    refused("act7 must be [..., 7] with the leading shape of rows", b.critic_q, rows, torch.zeros(3, 6))
    refused("act7 must be [..., 7] with the leading shape of rows", b.critic_q, rows, torch.zeros(4, 7))
    refused("state must be [..., 7, 28] and not empty", b.bootstrap_q, torch.zeros(3, 28, dtype=f64))
    refused("state must be [..., 7, 28] and not empty", b.bootstrap_q, torch.zeros(0, 7, 28, dtype=f64))
    refused("flags must have the leading shape of state", b.bootstrap_q, torch.zeros(3, 7, 28, dtype=f64), torch.zeros(4, dtype=i32))
    # --- outputs: dtype, contiguity, element count (the float32 ones take any shape of the right count, as before)
    refused("out must be a contiguous float32 device tensor of 3 elements", b.critic_q, rows, act7, out=torch.zeros(3, dtype=f64))
    refused("out must be a contiguous float32 device tensor of 3 elements", b.critic_q, rows, act7, out=torch.zeros(4))
    refused("out must be a contiguous float32 device tensor of 3 elements", b.critic_q, rows, act7, out=torch.zeros(6)[::2])
    refused("out must be a contiguous float32 device tensor of 3 elements", b.critic_q, rows, act7, out=torch.zeros(0))
    refused("actions_out must be a contiguous float32 device tensor of 21 elements", b.bootstrap_q, torch.zeros(3, 7, 28, dtype=f64),
            actions_out=torch.zeros(7, 3).t())
    # accepted, as before: another dtype or a list for an input, an output of another shape with the right count -- these reach the
    # backend, which has no critic
    for call in (lambda: b.critic_q(rows.float().tolist(), act7.double(), out=torch.zeros(1, 3)),
                 lambda: b.bootstrap_q(torch.zeros(3, 7, 28), [0, 0, 0], out=torch.zeros(3, 1), actions_out=torch.zeros(21))):
        with pytest.raises(PveError, match="backend"):
            call()
    # --- n-step blocks: strict tensors (nothing converted), and the two converted inputs
    b.reset()
    cur = b.step_many(3, trajectory=True)
    blk = lambda **kw: dict(cur, **kw)                                        # noqa: E731
    q = torch.zeros(3, 2, 64)
    refused("nstep_transitions: cur['flags'] must be a torch.int32 device tensor of shape (3, 2, 64)", b.nstep_transitions, 0.9,
            cur=blk(flags=cur["flags"].long()), q=q)
    refused("nstep_transitions: cur['reward'] must be a torch.float64 device tensor of shape (3, 2, 64)", b.nstep_transitions, 0.9,
            cur=blk(reward=cur["reward"][:, :, :63]), q=q)
    refused("nstep_transitions: cur['obs_post'] must be a torch.float64 device tensor of shape (3, 2, 64, 28)", b.nstep_transitions, 0.9,
            cur=blk(obs_post=cur["obs_post"].numpy()), q=q)
    refused("obs_first must be [..., 2, 64, 28] and not empty", b.nstep_transitions, 0.9, cur=cur, q=q, obs_first=torch.zeros(2, 64, 27))
    first = torch.zeros(2, 64, 28, dtype=f64)
    refused("nstep_transitions: q must be [n_ticks, n_envs, capacity]", b.nstep_transitions, 0.9, cur=cur, q=torch.zeros(2, 2, 64), obs_first=first)
    with pytest.raises(AttributeError):                                       # (q is not converted: a tensor or nothing, as before)
        b.nstep_transitions(0.9, cur=cur, q=q.numpy(), obs_first=first)
    with pytest.raises(PveError, match="pve_nstep_scan failed .*backend"):    # (a float64 q is converted and taken, as before)
        b.nstep_transitions(0.9, cur=cur, q=q.double(), obs_first=first.tolist())
    # --- statistics: strict blocks, the group map, the float64 outputs of an exact shape
    refused("rollout_stats: flags must be a torch.int32 device tensor of shape (3, 2, 64)", b.rollout_stats, blk(flags=cur["flags"].long()))
    refused("rollout_stats: reward must be a torch.float64 device tensor of shape (3, 2, 64)", b.rollout_stats, blk(reward=cur["reward"][:2]))
    refused("rollout_stats: env_out must be a torch.int32 device tensor of shape (3, 2, 8)", b.rollout_stats, blk(env_out=cur["env_out"].tolist()))
    refused("rollout_stats: groups must be [n_envs]", b.rollout_stats, cur, groups=[0, 1, 0])
    refused("metrics_by_group: groups must be [n_envs]", b.metrics_by_group, [[0, 1]], 2)
    refused("out must be a contiguous float64 device tensor of shape (3, 2, 14)", b.rollout_stats, cur, groups=[0, 1], out=torch.zeros(3, 2, 14))
    refused("out must be a contiguous float64 device tensor of shape (3, 2, 14)", b.rollout_stats, cur, groups=[0, 1],
            out=torch.zeros(84, dtype=f64))                                   # (the right count in another shape: refused here)
    refused("out must be a contiguous float64 device tensor of shape (3, 2, 14)", b.rollout_stats, cur, groups=[0, 1],
            out=torch.zeros(3, 2, 28, dtype=f64)[:, :, ::2])
    refused("out must be a contiguous float64 device tensor of shape (3, 2, 14)", b.rollout_stats, cur, groups=[0, 1], out=np.zeros((3, 2, 14)))
    refused("totals must be a contiguous float64 device tensor of shape (2, 14)", b.rollout_stats, cur, groups=[0, 1], totals=torch.zeros(14, 2, dtype=f64))
    refused("out must be a contiguous float64 device tensor of shape (2, 12)", b.metrics_by_group, [0, 1], 2, out=torch.zeros(2, 12))
    # --- another device type
    m = other_device_tensor(3, dtype=f32)
    if m is None:
        pytest.skip("no second device type without a GPU: the wrong-device refusals run in tests/test_gpu_binding_gateway.py")
    refused("out must be a contiguous float32 device tensor of 3 elements", b.critic_q, rows, act7, out=m)
    refused("out must be a contiguous float64 device tensor of shape (2, 12)", b.metrics_by_group, [0, 1], 2, out=other_device_tensor(2, 12, dtype=f64))
    refused("rollout_stats: flags must be a torch.int32 device tensor of shape (3, 2, 64)", b.rollout_stats,
            blk(flags=other_device_tensor(3, 2, 64, dtype=i32)))
    refused("nstep_transitions: cur['flags'] must be a torch.int32 device tensor of shape (3, 2, 64)", b.nstep_transitions, 0.9,
            cur=blk(flags=other_device_tensor(3, 2, 64, dtype=i32)), q=q)


def test_argument_refusals_of_the_replay_memories():
    b = batch(False)
    mem = ReplayMemory(b, buffer_size=17, batch_size=4)
    bad = "ReplayMemory.add: records must be a float32 device tensor [n, 36]"
    refused(bad, mem.add, torch.zeros(5, 36, dtype=torch.float64))
    refused(bad, mem.add, torch.zeros(5, 35))
    refused(bad, mem.add, torch.zeros(180))
    refused(bad, mem.add, np.zeros((5, 36), np.float32))
    with pytest.raises(PveError, match="backend"):           # (an empty or non-contiguous block of records is taken, as before)
        mem.add(torch.zeros(5, 72)[:, ::2])
    pm = PrioritizedReplayMemory(b, buffer_size=320, batch_size=8, learn_start=0, steps=1000)
    seq, q = torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    word = "PrioritizedReplayMemory.update_priority: %s must be a %s tensor on cpu with seq's element count"
    refused(word % ("seq", "torch.int64"), pm.update_priority, seq.int(), q)
    refused(word % ("seq", "torch.int64"), pm.update_priority, seq.tolist(), q)
    refused(word % ("q", "torch.float32"), pm.update_priority, seq, q.double())
    refused(word % ("q", "torch.float32"), pm.update_priority, seq, torch.zeros(5))
    refused(word % ("target", "torch.float32"), pm.update_priority, seq, q, torch.zeros(2, 4))
    with pytest.raises(PveError, match="backend"):           # (shapes are free, counts are not; non-contiguous is taken)
        pm.update_priority(seq.reshape(2, 2), torch.zeros(8)[::2], q.reshape(4, 1))
    m = other_device_tensor(4)
    if m is None:
        pytest.skip("no second device type without a GPU: the wrong-device refusals run in tests/test_gpu_binding_gateway.py")
    refused("ReplayMemory.add: records are on meta, the memory is on cpu", mem.add, other_device_tensor(5, 36))
    refused(word % ("q", "torch.float32"), pm.update_priority, seq, m)


@pytest.mark.parametrize("method", ["step", "step_wide"])
def test_argument_refusals_of_the_learner(method):
    # (the emulator has no learner kernels and pve_learner_init says so: the checks run on an object with the constructor's
    #  attributes, and refuse before any call)
    lrn = object.__new__(Learner)
    lrn._torch, lrn.batch, lrn.params = torch, batch(False), torch.zeros(_capi.LEARNER_N_FLOATS)
    lrn._lr = _capi.PveLearner(params=lrn.params.data_ptr(), actor_lr=1e-4, critic_lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, tau=0.998,
                               flags=0, block_threads=0)
    fn = getattr(lrn, method)
    rows, act7, target = torch.zeros(2, 5, 28), torch.zeros(2, 5, 7), torch.zeros(2, 5)
    refused("Learner.%s: rows must be a float32 tensor on cpu" % method, fn, rows.double(), act7, target)
    refused("Learner.%s: act7 must be a float32 tensor on cpu" % method, fn, rows, act7.numpy(), target)
    refused("Learner.%s: target must be a float32 tensor on cpu" % method, fn, rows, act7, target.half())
    shape = "Learner.%s: rows [n_batches, batch, 28], act7 [.., 7] and target [..] are needed" % method
    refused(shape, fn, torch.zeros(2, 5, 27), act7, target)
    refused(shape, fn, rows, torch.zeros(2, 5, 6), target)
    refused(shape, fn, rows, act7, torch.zeros(2, 4))
    refused(shape, fn, torch.zeros(2, 0, 28), torch.zeros(2, 0, 7), torch.zeros(2, 0))
    refused(shape, fn, torch.zeros(0, 5, 28), torch.zeros(0, 5, 7), torch.zeros(0, 5))
    refused(shape, fn, torch.zeros(28), torch.zeros(7), torch.zeros(()))
    refused(shape, fn, rows[0], act7, target)                # ([batch, 28] means one minibatch: the others must agree)
    refused("Learner.%s: losses must be a contiguous float32 device tensor [2, 2]" % method, fn, rows, act7, target, losses=torch.zeros(2, 2, dtype=torch.float64))
    refused("Learner.%s: losses must be a contiguous float32 device tensor [2, 2]" % method, fn, rows, act7, target, losses=torch.zeros(2, 4)[:, ::2])
    refused("Learner.%s: losses must be a contiguous float32 device tensor [1, 2]" % method, fn, rows[0], act7[0], target[0], losses=torch.zeros(3))
    refused("Learner.%s: grads must be a contiguous float32 device tensor [2, 13234]" % method, fn, rows, act7, target, grads=torch.zeros(2, 13233))
    refused("Learner.%s: grads must be a contiguous float32 device tensor [2, 13234]" % method, fn, rows, act7, target, grads=[0.0])
    # accepted, as before: True / False / None, a tensor of another shape with the right count -- then the backend has no learner
    for kw in (dict(), dict(losses=True, grads=True), dict(losses=False, grads=None), dict(losses=torch.zeros(4), grads=torch.zeros(13234, 2))):
        with pytest.raises(PveError, match="pve_learner_%s failed .*backend" % method):
            fn(rows, act7, target, **kw)
    m = other_device_tensor(2, 2)
    if m is None:
        pytest.skip("no second device type without a GPU: the wrong-device refusals run in tests/test_gpu_binding_gateway.py")
    refused("Learner.%s: rows must be a float32 tensor on cpu" % method, fn, other_device_tensor(2, 5, 28), act7, target)
    refused("Learner.%s: losses must be a contiguous float32 device tensor [2, 2]" % method, fn, rows, act7, target, losses=m)

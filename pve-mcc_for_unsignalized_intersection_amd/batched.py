"""BatchedIntersections: thousands of independent intersections per GPU (12-lane fast path; 4- / 8-lane layouts
through the general-geometry kernel).

Python host code over the C ABI (include/pve_env.h); torch is used only for device memory and
the stream.  One fused HIP kernel launch per tick = the reference's
`for lane, ind: env.step(lane, ind, a)` + `env.scene_update()` + `env.delete_vehicle()`
(reference traffic_interaction_scene.py:1501, :222, :435; caller protocol main.py:398-441).
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._args import is_tensor_of, tensor_in, tensor_out
from ._capi import PveConfig, PveEnvInfo, PveOutputs, PveRollout, PveVehicle, PveError, check

ALL_OUTPUTS = ("obs_post", "obs_pre", "reward", "flags", "lanej", "nbr", "new_slot", "env_out", "state_pre")
DEFAULT_OUTPUTS = ("obs_post", "reward", "flags", "nbr", "new_slot", "env_out")


def make_config(lib, **kw):
    cfg = PveConfig()
    lib.pve_default_config(C.byref(cfg))         # (no handle, no status: not a gateway call)
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError("unknown config field %r" % k)
        setattr(cfg, k, type(getattr(cfg, k))(v))
    return cfg


class BatchedIntersections:
    """n_envs environments x `capacity` vehicle slots, state resident in HBM (struct of arrays).

    capacity: 64, 128 or 256 slots per intersection.  256 needs lane_num = 12 on the fast path (not the 4- / 8-lane
              layouts, not general_path); a full intersection defers its spawns (metrics()["overflow"]), so a dense
              arrival stream or a slow policy wants 256.

    arrivals: float64 array/tensor [rows, lane_num] (shared by all envs) or [n_envs, rows, lane_num]; the
              reference's `arrive_time` matrix (main.py:388-389). Pad with +inf.  None: no stream yet --
              generate_arrivals() produces it on the device (or set_arrivals() installs one) before reset().
    outputs:  names of per-tick output buffers to allocate (see include/pve_env.h `pve_outputs`).
    intentions: lane_num = 8 only -- int array [rows, 8] / [n_envs, rows, 8] of 0/1: the reference's
              random.randint(0, 1) draws (ref :390) as an input stream (None = zeros).
    config:   reference constructor arguments (lane_num = 12 | 8 | 4, vm, ...); general_path=True runs the
              general-geometry kernel for lane_num = 12 too (cross-checks).
    obs_dtype: torch.float64 (reference parity layout) or torch.float32 (the actor's input type: the largest output
              shrinks by half; fused ticks only, no obs_pre / state_pre).
    """

    def __init__(self, n_envs, capacity, arrivals, device=None, outputs=DEFAULT_OUTPUTS, stream=None,
                 intentions=None, obs_dtype=torch.float64, _lib=None, **config):
        if device is None:
            device = "cuda"
        self.device = torch.device(device)
        if _lib is None:
            if self.device.type != "cuda":
                raise PveError("BatchedIntersections runs on an AMD GPU only (device=%s); there is no CPU path"
                               % self.device)
            _lib = _capi.load_library()
        self.lib = _lib
        self.n_envs, self.capacity = int(n_envs), int(capacity)
        if config.pop("general_path", False):
            config["flags"] = int(config.get("flags", 0)) | _capi.CFG_GENERAL_PATH
        if config.pop("geo_scan", False):
            config["flags"] = int(config.get("flags", 0)) | _capi.CFG_GEO_SCAN
        if config.pop("actor_f32", False):
            config["flags"] = int(config.get("flags", 0)) | _capi.CFG_ACTOR_F32
        if obs_dtype not in (torch.float64, torch.float32):
            raise TypeError("obs_dtype must be torch.float64 or torch.float32")
        self.obs_dtype = obs_dtype
        if obs_dtype == torch.float32:
            config["flags"] = int(config.get("flags", 0)) | _capi.CFG_OBS_F32
        self.cfg = make_config(self.lib, **config)
        self.lane_num = int(self.cfg.lane_num)
        self.dir_num = _capi.DIR_NUM.get(self.lane_num, 12)
        nbytes = self.lib.pve_workspace_bytes(self.n_envs, self.capacity)      # (a size query: no handle, no status)
        if nbytes == 0:
            raise PveError("invalid n_envs/capacity (capacity must be 64, 128 or 256; 256 needs lane_num 12)")
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        dev_index = self.device.index if self.device.index is not None else (
            torch.cuda.current_device() if self.device.type == "cuda" else 0)
        self._stream_obj = stream
        sptr = self._stream_ptr()
        h = C.c_void_p()
        # (pve_create makes the handle the gateway passes, pve_destroy ends it: the two are called directly)
        check(self.lib, self.lib.pve_create(C.byref(self.cfg), self.n_envs, self.capacity, dev_index,
                                            self.workspace.data_ptr(), sptr, C.byref(h)), "pve_create")
        self._h = h
        self._fns = {}                       # the gateway's bound entry points, by name
        self.arrivals = None
        if arrivals is not None:              # (None: generate_arrivals() will produce the stream on the device)
            self.set_arrivals(arrivals)
        self.intentions = None
        if intentions is not None:
            self.set_intentions(intentions)
        E, K = self.n_envs, self.capacity
        dev = self.device
        self.out = {}
        names = set(outputs)
        if "state_pre" in names:
            names.update(("obs_pre", "obs_post"))
        self._obs = None
        self._obs_cur = 0
        if "obs_post" in names:
            # state_pre reads the rows the previous tick stored (stale neighbour rows, ref :1332): ping-pong pair.
            # Otherwise ONE buffer: the tick never reads observations, and 117 MB less working set per 4096 envs
            # keeps more of the tick's traffic in the 256 MB Infinity Cache (57.2 vs 59.1 us per tick).
            self._obs = [torch.zeros(E, K, 28, dtype=obs_dtype, device=dev)
                         for _ in range(2 if "state_pre" in names else 1)]
            self._obs_cur = 0
        shapes = dict(obs_pre=((E, K, 28), obs_dtype), state_pre=((E, K, 7, 28), obs_dtype),
                      reward=((E, K), torch.float64), flags=((E, K), torch.int32), lanej=((E, K), torch.int32),
                      nbr=((E, K, 6), torch.int32), new_slot=((E, K), torch.int32), env_out=((E, 8), torch.int32))
        for n in names:
            if n == "obs_post":
                continue
            if n not in shapes:
                raise TypeError("unknown output %r" % n)
            shp, dt = shapes[n]
            self.out[n] = torch.zeros(shp, dtype=dt, device=dev)
        self._zero_actions = torch.zeros(E, K, dtype=torch.float64, device=dev)
        self.ticks = 0
        self._is_reset = False
        self.exploration = (0.0, 0, 0)       # (sigma, seed, env_offset): set_exploration

    # ------------------------------------------------------------------ plumbing
    def _stream_ptr(self):
        if self._stream_obj is not None:
            return C.c_void_p(self._stream_obj.cuda_stream)
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return C.c_void_p(0)

    def _bind_stream(self):
        """THE stream rule: kernels follow torch's current stream unless the batch was created with its own `stream`, which
        pve_create bound for good (nothing but pve_set_stream re-binds a handle, and nothing but this method calls it)."""
        if self._stream_obj is None:
            self.lib.pve_set_stream(self._h, self._stream_ptr())

    def _call(self, name, *args, bind=True):
        """THE gateway to the library: every entry point that takes the handle and returns a status is called here, by name.
        Binds the stream by _bind_stream's rule, passes the handle first, a tensor as its data_ptr(), a ctypes structure by
        reference and everything else (None = a null pointer) as it is, and raises PveError(name ...) on a status other than 0.
        `args` keeps the tensors alive across the call.  bind=False: calls that launch nothing -- they wait for, read back or
        describe what earlier calls enqueued, or set host state -- and so leave the handle on the stream that work went to.
        Not through here, each with its reason where it stands: pve_create / pve_destroy, the queries that take no handle or
        return no status, and the stepping calls (step, step_with_actor, step_many and prepare_step_many's callable), whose
        host cost per tick is what bench.py times: the gateway costs more per call than those vary from run to run
        (profiles/binding_gateway.txt), so they call their entry points directly, after the same _bind_stream()."""
        fn = self._fns.get(name)
        if fn is None:
            fn = self._fns[name] = getattr(self.lib, name)      # (an unknown name: AttributeError, here)
        if bind:
            self._bind_stream()
        rc = fn(self._h, *[a.data_ptr() if isinstance(a, torch.Tensor) else C.byref(a) if isinstance(a, C.Structure) else a
                           for a in args])
        if rc != 0:
            check(self.lib, rc, name)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.pve_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_arrivals(self, arrivals):
        a = torch.as_tensor(np.asarray(arrivals) if not torch.is_tensor(arrivals) else arrivals,
                            dtype=torch.float64)
        rows, stride_rows = self._stream_shape(a, "arrivals")
        self.arrivals = a.contiguous().to(self.device)
        self._call("pve_set_arrivals", self.arrivals, rows, stride_rows, bind=False)
        self._is_reset = False

    def _stream_shape(self, a, what):
        ln = self.lane_num
        if a.dim() == 2:
            assert a.shape[1] == ln, "%s must be [rows, %d]" % (what, ln)
            return a.shape[0], 0
        assert a.dim() == 3 and a.shape[0] == self.n_envs and a.shape[2] == ln, \
            "%s must be [rows,%d] or [n_envs,rows,%d]" % (what, ln, ln)
        return a.shape[1], a.shape[1]

    def set_intentions(self, choice):
        """lane_num = 8: the 0/1 intention draws (ref :390), same shape as the arrival stream."""
        c = torch.as_tensor(np.asarray(choice) if not torch.is_tensor(choice) else choice, dtype=torch.int32)
        rows, stride_rows = self._stream_shape(c, "intentions")
        self.intentions = c.contiguous().to(self.device)
        self._call("pve_set_intentions", self.intentions, rows, stride_rows, bind=False)
        self._is_reset = False

    def generate_arrivals(self, rate, horizon_s=None, rows=None, seed=0, epoch=0, env_offset=0, min_gap=1.0, covered=False):
        """The next episode's arrival stream, generated on the device and installed (pve_generate_arrivals; replaces the
        loadmat of main.py:228-229 / :388-389 and, for lane_num = 8, the intention draws of ref :381, :390): self.arrivals
        [n_envs, rows, lane_num] = arrivals.device_arrivals(...) bit for bit, for lane_num = 8 also self.intentions
        [n_envs, rows, 8] = arrivals.device_intentions(...).  No host work and no synchronisation: generate -> reset ->
        step_many can be enqueued back to back, and regenerating into the same buffers is ordered by the stream.
        rate: veh/h/lane, a scalar or one value per environment (array, or a float64 device tensor).  rows: given, or
        arrivals.default_rows(rate, horizon_s) (a per-environment rate on the device needs `rows`).  epoch: a new stream per episode
        under one seed.  env_offset: global index of this batch's first environment when the batch is a piece of a larger one.
        The buffers are allocated on the batch's stream and reused while the shape stays (a stream passed to the constructor or
        to set_arrivals is never written to).  covered=True returns the float64 [n_envs] tensor of times every lane of an
        environment is sure to reach (else None); read it when convenient.  Needs reset() afterwards."""
        from .arrivals import default_rows, device_mean
        E, ln = self.n_envs, self.lane_num
        on_device = torch.is_tensor(rate) and rate.device.type == self.device.type == "cuda"
        if rows is None:
            if horizon_s is None or on_device:
                raise PveError("generate_arrivals: pass rows or horizon_s (a rate tensor on the device needs rows)")
            rows = default_rows(rate.cpu().numpy() if torch.is_tensor(rate) else rate, horizon_s)
        rows = int(rows)
        per_env = on_device or np.ndim(rate.cpu().numpy() if torch.is_tensor(rate) else rate) > 0
        g = _capi.PveArrivalGen(seed=int(seed) & 0xFFFFFFFFFFFFFFFF, env_offset=int(env_offset), epoch=int(epoch) & 0xFFFFFFFF, rows=rows,
                                mean_s=1.0, mean_env=None, min_gap_s=float(min_gap), block_threads=0)
        with self._own_stream():
            mean = None
            if on_device:
                if rate.dtype != torch.float64 or tuple(rate.shape) != (E,):
                    raise PveError("generate_arrivals: a rate tensor must be float64 [n_envs]")
                mean = 3600.0 / rate
            elif per_env:
                mean = torch.as_tensor(device_mean(rate.cpu().numpy() if torch.is_tensor(rate) else rate, E)).to(self.device)
            else:
                g.mean_s = 3600.0 / float(rate)
            if mean is not None:
                g.mean_env = mean.data_ptr()
            buf = self.__dict__.setdefault("_gen_buffers", {})
            if buf.get("arrivals") is None or tuple(buf["arrivals"].shape) != (E, rows, ln):
                buf["arrivals"] = torch.empty(E, rows, ln, dtype=torch.float64, device=self.device)
                buf["intentions"] = torch.empty(E, rows, ln, dtype=torch.int32, device=self.device) if ln == 8 else None
            arr, ch = buf["arrivals"], buf["intentions"]
            cov = torch.empty(E, dtype=torch.float64, device=self.device) if covered else None
            self._call("pve_generate_arrivals", g, arr, ch, cov)
            if mean is not None and self._stream_obj is not None and mean.is_cuda:
                mean.record_stream(self._stream_obj)
        self.arrivals = arr
        self._call("pve_set_arrivals", arr, rows, rows, bind=False)
        if ch is not None:
            self.intentions = ch
            self._call("pve_set_intentions", ch, rows, rows, bind=False)
        self._is_reset = False
        return cov

    def state_field(self, name):
        """Zero-copy [n_envs, capacity] view of a persistent per-slot field (see pve_state_field)."""
        p = C.c_void_p()
        eb = C.c_int()
        self._call("pve_state_field", name.encode(), C.byref(p), C.byref(eb), bind=False)
        off = p.value - self.workspace.data_ptr()
        n = self.n_envs * self.capacity * eb.value
        dt = torch.float64 if eb.value == 8 else torch.int32
        return self.workspace[off:off + n].view(dt).view(self.n_envs, self.capacity)

    @property
    def obs(self):
        """[n_envs, capacity, 28] observation (state row 0) of the vehicle now in each slot."""
        return self._obs[self._obs_cur]

    def control_mask(self):
        return (self.state_field("meta") & _capi.META_CONTROL) != 0

    # ------------------------------------------------------------------ reference-shaped calls
    def reset(self):
        """New episode: the reference builds a new TrafficInteraction (main.py:394) whose constructor
        warms up until the first vehicle exists (ref :214-220)."""
        self._call("pve_reset")
        if self._obs is not None:
            for o in self._obs:
                o.zero_()
        for o in self.out.values():       # per-slot outputs of empty slots are not rewritten by the ticks
            o.zero_()
        self.ticks = 0
        self._is_reset = True

    def _outputs_struct(self, flip_obs):
        """pve_outputs for this call (cached per observation buffer: the host side of a tick is ~10 us of Python,
        which matters once sub-batches are pipelined on several streams)."""
        if self._obs is not None and len(self._obs) == 2 and flip_obs:
            self._obs_cur ^= 1
        cache = self.__dict__.setdefault("_out_structs", {})
        o = cache.get(self._obs_cur)
        if o is None:
            o = PveOutputs()
            if self._obs is not None:
                if len(self._obs) == 2:
                    o.obs_prev_post = self._obs[self._obs_cur ^ 1].data_ptr()
                o.obs_post = self._obs[self._obs_cur].data_ptr()
            for n, tns in self.out.items():
                setattr(o, n, tns.data_ptr())
            d = dict(self.out)
            if self._obs is not None:
                d["obs_post"] = self._obs[self._obs_cur]
            cache[self._obs_cur] = o
            self.__dict__.setdefault("_out_dicts", {})[self._obs_cur] = d
        return o

    def _own_stream(self):
        """Context in which torch's allocations / fills / copies are ordered with this handle's kernels: the handle's own
        stream when it has one (a torch side stream is non-blocking: nothing else orders a `torch.zeros` or `copy_` on
        the current stream against kernels launched on it), else a no-op (the kernels follow the current stream)."""
        import contextlib
        if self._stream_obj is not None and self.device.type == "cuda":
            return torch.cuda.stream(self._stream_obj)
        return contextlib.nullcontext()

    def step(self, actions=None):
        """One fused tick for every env. actions: float64 [n_envs, capacity] indexed by current slot
        (None = zeros). Returns the dict of output tensors (views, overwritten by the next call)."""
        a = self._zero_actions if actions is None else actions
        assert a.dtype == torch.float64 and a.is_contiguous() and a.shape == (self.n_envs, self.capacity)
        self._bind_stream()
        o = self._outputs_struct(flip_obs=True)
        rc = self.lib.pve_step_all(self._h, a.data_ptr(), C.byref(o))      # (a stepping call: direct, see _call)
        if rc != 0:
            check(self.lib, rc, "pve_step_all")
        self.ticks += 1
        return self._out_dicts[self._obs_cur]

    # ------------------------------------------------------------------ on-device MADDPG actor
    ACTOR_KEYS = ("ln0_gamma", "ln0_beta", "w1", "b1", "ln1_gamma", "ln1_beta", "w2", "b2", "ln2_gamma",
                  "ln2_beta", "w3", "b3")

    def set_actor(self, weights):
        """Pin the actor weights on the device. weights: flat float32[6393] tensor/array, or a dict with the
        TF variables LayerNorm{,_1,_2}/{gamma,beta} as ln{0,1,2}_{gamma,beta} and dense{,_1,_2}/{kernel,bias}
        as w{1,2,3}/b{1,2,3} (kernels in TF layout [in][out])."""
        if isinstance(weights, dict):
            weights = np.concatenate([np.asarray(weights[k], np.float32).ravel() for k in self.ACTOR_KEYS])
        w = torch.as_tensor(weights, dtype=torch.float32).contiguous()
        if w.numel() != _capi.PVE_ACTOR_N_WEIGHTS:
            raise PveError("actor needs %d float32 weights, got %d" % (_capi.PVE_ACTOR_N_WEIGHTS, w.numel()))
        with self._own_stream():
            self._actor_w = w.to(self.device)
            self._actor_actions = torch.zeros(self.n_envs, self.capacity, dtype=torch.float64, device=self.device)
            # copied into the handle's workspace (flat + packed for the matrix cores) on the handle's stream
            self._call("pve_set_actor", self._actor_w)

    def set_exploration(self, sigma, seed=0, env_offset=0):
        """Exploration noise of the device actor (main.py:44, :239): from the next call on, every controlled vehicle's action
        in act(), step_with_actor() and step_many(source="actor") is float64(actor(row)) + sigma * z, with
        z = noise.action_noise(seed, env + env_offset, vehicle id, ticks since reset()) -- reproducible, and the same in
        every launch form.  sigma = 0 (the default state) switches it off.  env_offset: global index of this batch's first
        environment when the batch is a piece of a larger one.  Actions passed to step() are never touched."""
        self._call("pve_set_action_noise", float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_offset), bind=False)
        self.exploration = (float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_offset))

    # ------------------------------------------------------------------ target networks: critic and bootstrap Q
    def set_target_networks(self, actor=None, critic=None):
        """Install the TARGET actor and / or a critic on the device (pve_set_target_networks); None keeps what is installed.
        actor: flat float32[6393] or a dict as for set_actor; critic: flat float32[6841] or a dict with the same keys (w2 is
        dense_1/kernel [71][64]: 64 hidden rows, own action, six other actions -- critic.flat_critic_weights).  Independent of
        set_actor: the acting policy is untouched."""
        from .critic import flat_critic_weights
        if actor is None and critic is None:
            raise PveError("set_target_networks: pass a target actor, a critic or both")
        ptr = []
        with self._own_stream():
            for w, n, what in ((actor, _capi.PVE_ACTOR_N_WEIGHTS, "target actor"), (critic, _capi.PVE_CRITIC_N_WEIGHTS, "critic")):
                if w is None:
                    ptr.append(None)
                    continue
                if isinstance(w, dict):
                    w = flat_critic_weights(w) if what == "critic" else \
                        np.concatenate([np.asarray(w[k], np.float32).ravel() for k in self.ACTOR_KEYS])
                t = torch.as_tensor(w, dtype=torch.float32).contiguous()
                if t.numel() != n:
                    raise PveError("%s needs %d float32 weights, got %d" % (what, n, t.numel()))
                ptr.append(t.to(self.device))
            self._call("pve_set_target_networks", *ptr)
            self._target_w = [t if t is not None else old for t, old in zip(ptr, getattr(self, "_target_w", [None, None]))]

    def _rows_arg(self, x, tail, what):
        """A contiguous device tensor of the handle's observation type whose trailing dimensions are `tail` -> (tensor, rows)"""
        x = tensor_in(x, self.device, self.obs_dtype, tail, "%s must be [..., %s] and not empty" % (what, ", ".join(str(t) for t in tail)),
                      tail=True)
        return x, x.numel() // int(np.prod(tail))

    def _f32_out(self, out, shape, what):
        return tensor_out(out, self.device, torch.float32, shape,
                          "%s must be a contiguous float32 device tensor of %d elements" % (what, int(np.prod(shape))))

    def critic_q(self, rows, act7, out=None):
        """Q of the installed critic (main.py:76 `agent.Q(state, action, other_action)`): rows [..., 28] (the handle's
        observation type), act7 [..., 7] float32 (own action, then the six other actions) -> float32 [...] (device tensor)."""
        with self._own_stream():
            rows, n = self._rows_arg(rows, (28,), "rows")
            a = tensor_in(act7, self.device, torch.float32, tuple(rows.shape[:-1]) + (7,), "act7 must be [..., 7] with the leading shape of rows")
            q = self._f32_out(out, tuple(rows.shape[:-1]), "out")
            self._call("pve_critic_forward", rows, a, q, n)
        return q

    def bootstrap_q(self, state=None, flags=None, out=None, actions_out=None):
        """The bootstrap term of the n-step target (main.py:253-260) with the installed target networks: every one of the 7
        rows of `state` [..., 7, 28] through the target actor, then the target critic on row 0 with those 7 actions.
        flags [...] int32 (the tick's `flags` output): only rows with F_CTL set and F_DONE clear are evaluated, the others
        get 0.  state=None: the batch's own state_pre / flags -- the trajectory blocks of the last
        step_many(trajectory=True) when there was one, else the single-tick views.  Returns (q float32 [...], act7 float32
        [..., 7]) device tensors (`out` / `actions_out` when given)."""
        with self._own_stream():
            if state is None:
                last = getattr(self, "_last_traj", None)
                src = last[1] if last is not None and last[0] == self.ticks else self.out     # (stale once the batch stepped on)
                if "state_pre" not in src or "flags" not in src:
                    raise PveError("bootstrap_q(): the batch was created without the state_pre / flags outputs; pass state")
                state, flags = src["state_pre"], (src["flags"] if flags is None else flags)
            state, n = self._rows_arg(state, (7, 28), "state")
            lead = tuple(state.shape[:-2])
            if flags is not None:
                flags = tensor_in(flags, self.device, torch.int32, lead, "flags must have the leading shape of state")
            q = self._f32_out(out, lead, "out")
            a7 = self._f32_out(actions_out, lead + (7,), "actions_out")
            self._call("pve_bootstrap_q", state, flags, q, a7, n)
        return q, a7

    # ------------------------------------------------------------------ n-step transitions (pve_nstep_scan / pve_nstep_gather)
    _NSTEP_KEYS = ("obs_post", "state_pre", "reward", "flags", "new_slot")

    def _nstep_segment(self, seg, blocks, what):
        for k in self._NSTEP_KEYS:
            if k not in blocks:
                raise PveError("nstep_transitions: %s lacks the %s output (create the batch with state_pre, reward, flags, new_slot)" % (what, k))
        n = int(blocks["flags"].shape[0])
        want = dict(obs_post=((n, self.n_envs, self.capacity, 28), self.obs_dtype), state_pre=((n, self.n_envs, self.capacity, 7, 28), self.obs_dtype),
                    reward=((n, self.n_envs, self.capacity), torch.float64), flags=((n, self.n_envs, self.capacity), torch.int32),
                    new_slot=((n, self.n_envs, self.capacity), torch.int32))
        keep = []
        for k in self._NSTEP_KEYS:
            tns = blocks[k]
            if not is_tensor_of(tns, want[k][1], self.device, shapes=(want[k][0],)):
                raise PveError("nstep_transitions: %s[%r] must be a %s device tensor of shape %s" % (what, k, want[k][1], want[k][0]))
            tns = tns.contiguous()
            keep.append(tns)
            setattr(seg, k, tns.data_ptr())
        seg.n_ticks = n
        return n, keep

    def nstep_transitions(self, gamma, window=13, prev=None, q=None, tail=False, max_records=None, cur=None, obs_first=None,
                          block_threads=0):
        """The n-step training transitions of a trajectory roll-out, assembled on the device (reference main.py:243-266):
        for every controlled vehicle and tick the reference's sliding buffer of `window` = seq_max_step + 1 ticks, folded into
        target = sum_k gamma^k r_k (+ gamma^window Q' behind the last entry unless the vehicle is Done), in float64 and in the
        reference's backward order (bit-equal to nstep.py).  Returns (records, index, total):
          records float32 [M, 36]: row 0 of s0 [28] (the row the actor consumed), the 7 actions, the target;
          index   int32 [M, 4]: start tick relative to cur (negative: in prev), env, slot, code (entries used | 0x100
                  bootstrapped | 0x200 closed by Done); record order is (tick, env, slot) ascending;
          total   the number of transitions.
        cur: the blocks of the trajectory (default: those of the last step_many(trajectory=...), which must be this batch's
        latest stepping call).  prev: the blocks of the step_many call right before it (the dict it returned), so that windows
        that cross the two calls emit: a transition is emitted by the call in which its window CLOSES, windows still open at
        the end of cur emit when cur is passed as prev next time (alternate two alloc_trajectory() buffer sets).  prev=None:
        the windows that were open before cur are LOST (harmless right after reset()).  prev must hold at least `window`
        ticks; that the two calls are consecutive is checked against the recorded tick stamps.
        q: float32 [n_ticks, n_envs, cap] bootstrap Q of cur (default: bootstrap_q() on cur).  tail=True also emits the
        windows a Done truncates (the reference drops all but the oldest).  max_records=None reads `total` once (one
        synchronisation) and allocates exactly, M = total; a given max_records allocates that many rows without synchronising,
        fills the first min(total, max_records) in order and returns `total` as a 0-dim device tensor.
        lane_num 4 / 8: the pass is slot-indexed; that `ids` order differs from slot order there does not matter
        (tests/nstep_identity_scenarios.py holds it to the reference's per-vehicle buffers, keyed by vehicle id, on those layouts)."""
        window = int(window)
        with self._own_stream():
            stamped = cur is None
            if stamped:
                last = getattr(self, "_last_traj", None)
                if last is None or last[0] != self.ticks:
                    raise PveError("nstep_transitions: no trajectory of the latest stepping call (step_many(trajectory=...)); pass cur")
                cur = last[1]
                if prev is None and obs_first is None:
                    obs_first = last[3]
                if prev is not None:
                    before = getattr(self, "_prev_traj", None)
                    if before is None or "flags" not in prev or before[1]["flags"].data_ptr() != prev["flags"].data_ptr() or before[0] != last[2]:
                        raise PveError("nstep_transitions: prev is not the trajectory of the step_many call right before cur")
                    prev = before[1]
            ns = _capi.PveNstep()
            n_cur, keep = self._nstep_segment(ns.cur, cur, "cur")
            n_prev = 0
            if prev is not None:
                n_prev, keep_prev = self._nstep_segment(ns.prev, prev, "prev")
                keep += keep_prev
                if n_prev < window:
                    raise PveError("nstep_transitions: prev holds %d ticks, fewer than window = %d (pass prev=None and accept the loss)" % (n_prev, window))
            else:
                if obs_first is None:
                    raise PveError("nstep_transitions: without prev, obs_first (the rows stored before cur's first tick) is needed")
                obs_first, _ = self._rows_arg(obs_first, (self.n_envs, self.capacity, 28), "obs_first")
                ns.obs_first = obs_first.data_ptr()
            if q is None:
                q, _ = self.bootstrap_q(cur["state_pre"], cur["flags"])
            q = tensor_in(q, self.device, torch.float32, (n_cur, self.n_envs, self.capacity),
                          "nstep_transitions: q must be [n_ticks, n_envs, capacity]", convert=False)
            n_cand = min(n_prev, window - 1) + n_cur
            dev = self.device
            target = torch.empty(n_cand, self.n_envs, self.capacity, dtype=torch.float64, device=dev)
            code = torch.empty(n_cand, self.n_envs, self.capacity, dtype=torch.int32, device=dev)
            offsets = torch.empty(n_cand * self.n_envs * self.capacity // 64 + 1, dtype=torch.int32, device=dev)
            total = torch.zeros((), dtype=torch.int64, device=dev)
            ns.gamma, ns.window, ns.mode = float(gamma), window, (_capi.NSTEP_TAIL if tail else 0)
            ns.q_boot, ns.target, ns.code, ns.offsets, ns.total = q.data_ptr(), target.data_ptr(), code.data_ptr(), offsets.data_ptr(), total.data_ptr()
            ns.block_threads = int(block_threads)
            self._call("pve_nstep_scan", ns)
            if max_records is None:
                n_out = total_out = int(total.item())
            else:
                n_out, total_out = int(max_records), total
            records = torch.empty(n_out, _capi.NSTEP_RECORD, dtype=torch.float32, device=dev)
            index = torch.empty(n_out, 4, dtype=torch.int32, device=dev)
            ns.max_records, ns.records, ns.index = n_out, records.data_ptr(), index.data_ptr()
            self._call("pve_nstep_gather", ns)
            self._nstep_last = (target, code, offsets)      # (diagnostics: the dense scan outputs of the last call)
        return records, index, total_out

    def act(self):
        """actions [n_envs, capacity] = actor(obs) for the controlled slots (+ the exploration noise, set_exploration),
        0 elsewhere (device tensor)."""
        self._call("pve_actor_forward", None, self.obs, self._actor_actions)
        return self._actor_actions

    def step_with_actor(self):
        """One closed-loop tick entirely on the device: actor(obs) -> fused tick (two launches, no host
        round trip; main.py:398-441 with the actor of model_agent_maddpg.py)."""
        self._bind_stream()
        obs_in = self._obs[self._obs_cur]
        o = self._outputs_struct(flip_obs=True)
        check(self.lib, self.lib.pve_step_all_actor(self._h, None, obs_in.data_ptr(), self._actor_actions.data_ptr(), C.byref(o)),
              "pve_step_all_actor")                                          # (a stepping call: direct, see _call)
        self.ticks += 1
        return self.outputs()

    # ------------------------------------------------------------------ many ticks per call (pve_step_many)
    def set_action_pool(self, pool):
        """Action tape resident on the device: float64 [n_pool, n_envs, capacity]; tick number k since reset() uses
        pool[k % n_pool] (what `step(pool[k % n_pool])` would pass)."""
        p = torch.as_tensor(pool, dtype=torch.float64).contiguous().to(self.device)
        if p.dim() != 3 or tuple(p.shape[1:]) != (self.n_envs, self.capacity):
            raise PveError("action pool must be [n_pool, %d, %d]" % (self.n_envs, self.capacity))
        self._pool = p

    def set_action_table(self, table):
        """A policy that is a function of (tick, vehicle id), resident on the device: float64 [n_rows, n_ids]; at tick
        number k since reset() the vehicle with id v gets table[k % n_rows, min(v, n_ids - 1)] (controlled vehicles; the
        others 0, main.py:401) -- e.g. the sin tape of BASELINE.md 3, float32(sin(0.37 id + 0.05 tick)).
        step_many(source="table") gathers it inside the resident kernel; actions_from_table() gives the same per tick."""
        t = torch.as_tensor(table, dtype=torch.float64).contiguous().to(self.device)
        if t.dim() != 2:
            raise PveError("action table must be [n_rows, n_ids]")
        self._table = t

    def actions_from_table(self):
        """[n_envs, capacity] actions of the CURRENT tick from the table (what step_many(source="table") applies next)."""
        tab = self._table
        ids = self.state_field("id").long().clamp(0, tab.shape[1] - 1)
        return tab[self.ticks % tab.shape[0]][ids].contiguous()

    _TRAJ_SHAPES = dict(reward=(), flags=(), lanej=(), new_slot=(), nbr=(6,))

    def alloc_trajectory(self, n_ticks):
        """Reusable [n_ticks, ...] output buffers for step_many(trajectory=<this dict>): a trainer that collects
        roll-outs chunk by chunk hands the same buffers (or a ring of them) to every call instead of paying an allocation
        and a zero-fill of several GB per chunk.  Slots that hold no vehicle are marked by flags == 0; their other
        per-slot outputs keep whatever an earlier tick left there."""
        E, K, dev = self.n_envs, self.capacity, self.device
        traj = {}
        with self._own_stream():
            if self._obs is not None:
                traj["obs_post"] = torch.zeros(n_ticks, E, K, 28, dtype=self.obs_dtype, device=dev)
            for n, tns in self.out.items():
                traj[n] = torch.zeros((n_ticks,) + tuple(tns.shape), dtype=tns.dtype, device=dev)
        return traj

    def step_many(self, n_ticks, actor=False, source=None, trajectory=False, chunk=0, update_views=True, persistent=False):
        """n_ticks fused ticks in ONE call, the action source on the device (the reference's episode loop
        main.py:397-441 without the host in it): source = "pool" (set_action_pool), "actor" (set_actor; closed loop)
        or "zero".  Bit-identical to n_ticks step() / step_with_actor() calls.
        trajectory=False: returns the usual output dict holding the LAST tick's outputs.
        trajectory=True: returns a dict of freshly allocated [n_ticks, ...] tensors with every tick's outputs (a roll-out).
        trajectory=<dict from alloc_trajectory(m), m >= n_ticks>: the same into the caller's buffers (blocks 0 .. n_ticks-1).
        update_views=False (trajectory roll-outs only): skip the copy of the last tick into the handle's single-tick views
        (`obs`, `out`) -- not with source="actor", whose next call reads `obs`.
        persistent=True (with 0 < chunk < n_ticks): the call is ONE launch whose workgroups pull (intersection, chunk) items
        from a queue -- for a batch of at least twice as many intersections as the chip holds workgroups (4096 x 128 slots on
        one MI355X); same results.  Eligible: lane_num 12 with every source (not the exact-float32 actor), trajectory
        roll-outs and the training outputs included; lane_num 4 / 8 with every source, the training outputs with "pool" / "zero"
        (with "actor" they run in the resident kernel as chunked launches); anything else runs as chunked launches (last_launch() tells which).  With source="actor" the handle's
        `_actor_actions` scratch is the hand-off buffer between the items of an intersection."""
        n_ticks = int(n_ticks)
        if source is None:
            source = "actor" if actor else ("pool" if getattr(self, "_pool", None) is not None else "zero")
        self._bind_stream()
        ro = PveRollout()
        ro.n_ticks = n_ticks
        ro.trajectory = 1 if trajectory else 0
        ro.chunk_ticks = int(chunk)
        ro.persistent = 1 if persistent else 0
        if source == "pool":
            if getattr(self, "_pool", None) is None:
                raise PveError("step_many(source='pool'): call set_action_pool first")
            ro.source, ro.pool, ro.n_pool = _capi.SRC_POOL, self._pool.data_ptr(), self._pool.shape[0]
            ro.pool_tick0 = self.ticks % self._pool.shape[0]
        elif source == "actor":
            if getattr(self, "_actor_w", None) is None:
                raise PveError("step_many(source='actor'): call set_actor first")
            ro.source, ro.actor_weights = _capi.SRC_ACTOR, None          # (installed by set_actor)
            ro.actor_obs, ro.actor_actions = self._obs[self._obs_cur].data_ptr(), self._actor_actions.data_ptr()
            if not update_views:
                raise PveError("step_many(source='actor') reads the handle's observation view: update_views must stay True")
        elif source == "zero":
            ro.source = _capi.SRC_ZERO
        elif source == "table":
            if getattr(self, "_table", None) is None:
                raise PveError("step_many(source='table'): call set_action_table first")
            ro.source, ro.pool, ro.n_pool = _capi.SRC_TABLE, self._table.data_ptr(), self._table.shape[0]
            ro.table_ids, ro.pool_tick0 = self._table.shape[1], self.ticks % self._table.shape[0]
        else:
            raise PveError("unknown action source %r" % (source,))
        if "state_pre" in self.out and not trajectory:
            raise PveError("step_many: state_pre needs a trajectory roll-out (every tick reads the rows the previous one stored)")
        if not trajectory:
            o = self._outputs_struct(flip_obs=False)
            check(self.lib, self.lib.pve_step_many(self._h, C.byref(ro), C.byref(o)), "pve_step_many")     # (a stepping call: direct, see _call)
            self.ticks += n_ticks
            return self._out_dicts[self._obs_cur]
        o = PveOutputs()
        # the zero-fill of fresh trajectory buffers, the roll-out and the copy-back of the last tick are one ordered
        # sequence on the stream the kernels run on (the returned tensors belong to that stream: consume them there or
        # after synchronize())
        with self._own_stream():
            if isinstance(trajectory, dict):
                traj = trajectory
                want = set(self.out) | ({"obs_post"} if self._obs is not None else set())
                if set(traj) != want or any(t.shape[0] < n_ticks for t in traj.values()):
                    raise PveError("step_many: trajectory buffers must come from alloc_trajectory(m) of this batch, m >= n_ticks")
            else:
                traj = self.alloc_trajectory(n_ticks)
            for n, tns in traj.items():
                setattr(o, n, tns.data_ptr())
            if "state_pre" in self.out:      # the stale neighbour rows of the first tick: what the previous tick stored
                o.obs_prev_post = self._obs[self._obs_cur].data_ptr()
                if not update_views:
                    raise PveError("step_many with state_pre reads the handle's observation view: update_views must stay True")
            check(self.lib, self.lib.pve_step_many(self._h, C.byref(ro), C.byref(o)), "pve_step_many")     # (as above)
            self.ticks += n_ticks
            obs_first = self._obs[self._obs_cur] if self._obs is not None else None   # the rows stored before this call
            if n_ticks > 0 and update_views:     # the handle's single-tick views keep showing the latest tick
                if self._obs is not None:
                    if len(self._obs) == 2:      # (into the other buffer of the pair: the rows in front of the call stay readable
                        self._obs_cur ^= 1       #  for nstep_transitions until the batch steps on, at no cost)
                    self._obs[self._obs_cur].copy_(traj["obs_post"][n_ticks - 1])
                for n, tns in self.out.items():
                    tns.copy_(traj[n][n_ticks - 1])
        # (what bootstrap_q() / nstep_transitions() read by default: the blocks this call filled, the tick stamps of its end and
        #  start, the rows stored before it; the call before it is remembered to check that `prev` and `cur` are consecutive)
        if n_ticks > 0:
            self._prev_traj = getattr(self, "_last_traj", None)
            self._last_traj = (self.ticks, {n: tns[:n_ticks] for n, tns in traj.items()}, self.ticks - n_ticks, obs_first)
        else:
            self._last_traj = None
        return traj

    def prepare_step_many(self, n_ticks, source=None, chunk=0, persistent=False):
        """A prepared pve_step_many call (trajectory=False): everything the call needs is built once; the returned callable
        re-issues it (only the position in the action pool advances) at the cost of one ctypes call -- for loops whose host
        side is measured in microseconds (RL inner loops, bench.py's timed region).  The prepared call keeps the pool / table
        tensor it was built on alive and refuses to run (PveError) once set_action_pool / set_action_table has replaced
        the source of ITS kind; a batch without a stream of its own re-binds torch's current stream on every call."""
        n_ticks = int(n_ticks)
        if source is None:
            source = "pool" if getattr(self, "_pool", None) is not None else "zero"
        if source == "actor" or "state_pre" in self.out:
            raise PveError("prepare_step_many: pool / zero sources without state_pre (use step_many)")
        ro = PveRollout()
        ro.n_ticks, ro.trajectory, ro.chunk_ticks, ro.persistent = n_ticks, 0, int(chunk), (1 if persistent else 0)
        if source == "pool":
            if getattr(self, "_pool", None) is None:
                raise PveError("prepare_step_many(source='pool'): call set_action_pool first")
            ro.source, ro.pool, ro.n_pool = _capi.SRC_POOL, self._pool.data_ptr(), self._pool.shape[0]
        elif source == "zero":
            ro.source = _capi.SRC_ZERO
        elif source == "table":
            if getattr(self, "_table", None) is None:
                raise PveError("prepare_step_many(source='table'): call set_action_table first")
            ro.source, ro.pool, ro.n_pool = _capi.SRC_TABLE, self._table.data_ptr(), self._table.shape[0]
            ro.table_ids = self._table.shape[1]
        else:
            raise PveError("unknown action source %r" % (source,))
        self._bind_stream()
        o = self._outputs_struct(flip_obs=False)
        # (the prepared call runs no gateway code: the entry point and its arguments are bound here, once)
        fn, h, pro, po, n_pool = self.lib.pve_step_many, self._h, C.byref(ro), C.byref(o), max(1, int(ro.n_pool))
        src_attr = {"pool": "_pool", "table": "_table"}.get(source)
        src_tensor = getattr(self, src_attr) if src_attr else None
        follow_stream = self._stream_obj is None

        def call():
            if src_attr is not None and getattr(self, src_attr) is not src_tensor:
                raise PveError("prepared step_many call is stale: the action %s was replaced after prepare_step_many"
                               % source)
            if follow_stream:
                self._bind_stream()
            ro.pool_tick0 = self.ticks % n_pool
            rc = fn(h, pro, po)
            if rc != 0:
                check(self.lib, rc, "pve_step_many")
            self.ticks += n_ticks
        call._keep = (ro, o, src_tensor)
        return call

    def scene_update(self, actions=None):
        """Split protocol, part 1: all step() calls + scene_update(); Done vehicles stay in place."""
        a = self._zero_actions if actions is None else actions
        assert a.dtype == torch.float64 and a.is_contiguous() and a.shape == (self.n_envs, self.capacity)
        self._call("pve_scene_update", a, self._outputs_struct(flip_obs=True))
        self.ticks += 1
        return self.outputs()

    def compact(self):
        """Split protocol, part 2: delete_vehicle() (ref :435)."""
        self._call("pve_compact", self._obs[self._obs_cur] if self._obs is not None else None)

    def outputs(self):
        self._outputs_struct(flip_obs=False)
        return self._out_dicts[self._obs_cur]

    def synchronize(self):
        self._call("pve_synchronize", bind=False)

    def last_launch(self):
        """What the last stepping call launched: "tick" (one launch per tick), "resident" (one k_rollout launch per chunk),
        "persistent" (one launch for the call, items pulled from the work queue) or "none" (pve_debug_last_launch)."""
        k = self.lib.pve_debug_last_launch(self._h)        # (returns the kind, not a status: not a gateway call)
        if k < 0 or k > 3:                              # (a negative PVE_ERR_* must not index the tuple from its end)
            check(self.lib, k if k < 0 else -1, "pve_debug_last_launch")
        return _capi.LAUNCH_NAMES[k]

    def last_variant(self):
        """Which kernel variant the last stepping call launched, as a dict (pve_debug_last_variant, include/pve_env_debug.h):
        kind (as last_launch()), family (12, or 4 / 8), capacity, waves_per_simd (4 = the register build, 5 = the HOME build
        of the 128-slot queue kernel, 0 = per-tick launches), the flags prof / actor / train / table / persistent / geo of the
        kernel that ran, grid (workgroups of the last launch) and launches (kernel launches the call enqueued).  Host only:
        waits for nothing.  A call of zero ticks: kind "none" and zeros."""
        v = _capi.PveLaunchVariant()
        if not hasattr(self.lib, "pve_debug_last_variant"):
            raise PveError("this library is an older build: it lacks pve_debug_last_variant (rebuild it)")
        self._call("pve_debug_last_variant", v, bind=False)
        d = {n: int(getattr(v, n)) for n, _t in _capi.PveLaunchVariant._fields_ if n != "reserved"}
        d["kind"] = _capi.LAUNCH_NAMES[d["kind"]]
        return d

    # ------------------------------------------------------------------ host read-back
    def read_env(self, env=0):
        info = PveEnvInfo()
        self._call("pve_read_env", env, info, bind=False)
        return info

    def read_vehicles(self, env=0):
        buf = (PveVehicle * self.capacity)()
        n = C.c_int()
        self._call("pve_read_vehicles", env, buf, self.capacity, C.byref(n), bind=False)
        return [buf[i] for i in range(min(n.value, self.capacity))]

    def metrics(self):
        """dict of the 12 metric sums over this handle's envs since reset (SURVEY §8e vector)."""
        out = (C.c_double * _capi.PVE_N_METRICS)()
        self._call("pve_get_metrics", out, bind=False)
        return dict(zip(_capi.METRIC_NAMES, [float(x) for x in out]))

    # ------------------------------------------------------------------ statistics by group (pve_rollout_stats / pve_metrics_groups)
    def _groups_arg(self, groups, n_groups, what):
        """(int32 device tensor [n_envs] or None, G).  The map's maximum is read only from a host array: a device tensor needs
        n_groups (reading it would wait for the device)."""
        if groups is None:
            if n_groups not in (None, 1):
                raise PveError("%s: n_groups must be 1 without a group map" % what)
            return None, 1
        if n_groups is None:
            if torch.is_tensor(groups) and groups.device.type == "cuda":
                raise PveError("%s: pass n_groups with a group map on the device" % what)
            n_groups = int(np.max(groups.numpy() if torch.is_tensor(groups) else np.asarray(groups))) + 1
        return tensor_in(groups, self.device, torch.int32, (self.n_envs,), "%s: groups must be [n_envs]" % what), int(n_groups)

    def _f64_arg(self, x, shape, what):
        return tensor_out(x, self.device, torch.float64, shape,
                          "%s must be a contiguous float64 device tensor of shape %s" % (what, tuple(shape)), same_shape=True)

    def rollout_stats(self, traj=None, groups=None, n_groups=None, out=None, totals=None, block_threads=0):
        """The roll-out's statistics by tick and by group of environments (pve_rollout_stats; what main.py:286-304 writes per
        tick and main.py:315-328 / :413-415 / :576-581 derive): the float64 device tensor series [T, G, 14], columns
        stats.STAT_NAMES, bit-equal to stats.rollout_stats (csrc/pve_stats.h states the order of every sum).
        traj: a dict of retained blocks (what step_many(trajectory=...) returned; [n_envs, ...] blocks count as T = 1) holding
        flags, reward and env_out, and obs_pre when sum_v / sum_a are wanted (they are 0 without).  None: the blocks of the
        last step_many(trajectory=...) when there was one, else the single-tick views.  groups: int [n_envs] with values in
        [0, n_groups) (an environment outside the range is counted in no group), None = one group.  totals: a float64
        device tensor [G, 14] to which series[t], t ascending, is added on the device: an epoch's totals across calls.
        Runs on the batch's stream and reads nothing back; stats.summaries() turns series or totals into the reference's
        quantities.  (The kernels' scratch, the per-(tick, env) rows [T, n_envs, 14], is kept in the batch and reused by the
        next call of the same shape.)"""
        with self._own_stream():
            if traj is None:
                last = getattr(self, "_last_traj", None)
                traj = last[1] if last is not None and last[0] == self.ticks else self.out
            for k in ("flags", "reward", "env_out"):
                if k not in traj:
                    raise PveError("rollout_stats: the blocks lack the %s output (create the batch with flags, reward, env_out)" % k)
            E, K = self.n_envs, self.capacity
            flags = traj["flags"]
            T = 1 if flags.dim() == 2 else int(flags.shape[0])
            want = dict(flags=((T, E, K), torch.int32), reward=((T, E, K), torch.float64), env_out=((T, E, 8), torch.int32),
                        obs_pre=((T, E, K, 28), self.obs_dtype))
            keep = {}
            for k, (shp, dt) in want.items():
                tns = traj.get(k)
                if tns is None:
                    continue
                if not is_tensor_of(tns, dt, self.device, shapes=(shp, shp[1:] if T == 1 else shp)) or T < 1:
                    raise PveError("rollout_stats: %s must be a %s device tensor of shape %s" % (k, dt, shp))
                keep[k] = tns.contiguous()
            g, G = self._groups_arg(groups, n_groups, "rollout_stats")
            series = self._f64_arg(out, (T, G, _capi.PVE_STAT_N), "out")
            if totals is not None:
                totals = self._f64_arg(totals, (G, _capi.PVE_STAT_N), "totals")
            rows = self.__dict__.get("_stats_rows")
            if rows is None or tuple(rows.shape) != (T, E, _capi.PVE_STAT_N):
                rows = torch.empty(T, E, _capi.PVE_STAT_N, dtype=torch.float64, device=self.device)
            st = _capi.PveStats(n_ticks=T, n_groups=G, block_threads=int(block_threads), reserved=0,
                                group=g.data_ptr() if g is not None else None, flags=keep["flags"].data_ptr(),
                                reward=keep["reward"].data_ptr(), obs_pre=keep["obs_pre"].data_ptr() if "obs_pre" in keep else None,
                                env_out=keep["env_out"].data_ptr(), series=series.data_ptr(),
                                totals=totals.data_ptr() if totals is not None else None, scratch=rows.data_ptr())
            self._call("pve_rollout_stats", st)
            if self._stream_obj is not None and self.device.type == "cuda":
                for tns in list(keep.values()) + ([g] if g is not None else []):
                    tns.record_stream(self._stream_obj)
            self._stats_rows = rows
        return series

    def metrics_by_group(self, groups=None, n_groups=None, out=None):
        """The twelve sums of metrics() per group of environments, read from the per-environment headers on the device
        (pve_metrics_groups): the float64 device tensor [G, 12] in the order of _capi.METRIC_NAMES, on the batch's stream, with
        no host copy and no wait.  With one group it equals metrics() bit for bit.  groups / n_groups as rollout_stats."""
        with self._own_stream():
            g, G = self._groups_arg(groups, n_groups, "metrics_by_group")
            res = self._f64_arg(out, (G, _capi.PVE_N_METRICS), "out")
            self._call("pve_metrics_groups", g, G, res)
            if g is not None and self._stream_obj is not None and self.device.type == "cuda":
                g.record_stream(self._stream_obj)
        return res



class PipelinedIntersections:
    """`n_envs` environments as `n_sub` sub-batches, each a BatchedIntersections on its own HIP stream.
    (capacity: 64, 128 or 256 slots, as BatchedIntersections; 256 with lane_num = 12 only.)

    The environments are independent, so the sub-batches never synchronise with each other: tick t+1 of one is in
    flight while tick t of another still runs.  One launch over all envs runs its workgroups in lock-step (every
    workgroup loads, computes and stores at the same time, and 4096 envs are exactly two rounds of the 2048 resident
    workgroups); two free-running populations interleave instead, the chip-wide LOAD / FIN bursts of one overlap the
    compute phases of the other: 4096 x 128 slots take 39 us per tick of ALL envs instead of 54 us (MI355X).

    Ordering is per sub-batch: `step()` enqueues on `streams[k]`; produce the actions of sub-batch k on that stream (or
    call `wait_stream()` after producing them elsewhere) and consume its outputs on that stream or after
    `synchronize()`.  This is the usual two-batch pipelining of an RL loop: policy inference for one half while the
    environment steps the other.  A replay memory (replay.ReplayMemory) binds to ONE sub-batch's handle and stream
    (`ReplayMemory(pipe.subs[k], ...)`); it is not fanned out over the sub-batches.
    """

    def __init__(self, n_envs, capacity, arrivals, n_sub=2, device=None, outputs=DEFAULT_OUTPUTS, intentions=None,
                 _lib=None, **config):
        if n_sub < 1 or n_sub > n_envs:
            raise PveError("n_sub must be in 1 .. n_envs")
        self.device = torch.device("cuda" if device is None else device)
        self.n_envs, self.capacity, self.n_sub = int(n_envs), int(capacity), int(n_sub)
        base, rem = divmod(self.n_envs, self.n_sub)
        sizes = [base + (1 if k < rem else 0) for k in range(self.n_sub)]
        self.bounds = [0]
        for z in sizes:
            self.bounds.append(self.bounds[-1] + z)
        on_gpu = self.device.type == "cuda"
        self.streams = [torch.cuda.Stream(self.device) if on_gpu else None for _ in range(self.n_sub)]

        def part(x, k):
            if x is None:
                return None
            x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
            return x if x.dim() == 2 else x[self.bounds[k]:self.bounds[k + 1]]
        self.subs = []
        for k in range(self.n_sub):
            with self._on(k):
                self.subs.append(BatchedIntersections(sizes[k], capacity, part(arrivals, k), device=self.device,
                                                      outputs=outputs, stream=self.streams[k],
                                                      intentions=part(intentions, k), _lib=_lib, **config))
        self.synchronize()

    def _on(self, k):
        import contextlib
        return torch.cuda.stream(self.streams[k]) if self.streams[k] is not None else contextlib.nullcontext()

    def _parts(self, x):
        if x is None:
            return [None] * self.n_sub
        if isinstance(x, (list, tuple)):
            return list(x)
        return [x[self.bounds[k]:self.bounds[k + 1]] for k in range(self.n_sub)]     # contiguous row ranges

    def reset(self):
        for k, sub in enumerate(self.subs):
            with self._on(k):
                sub.reset()

    def wait_stream(self, stream=None):
        """Every sub-batch stream waits for what has been enqueued on `stream` (default: torch's current stream)."""
        if self.device.type != "cuda":
            return
        stream = torch.cuda.current_stream(self.device) if stream is None else stream
        for s in self.streams:
            s.wait_stream(stream)

    def step(self, actions=None, wait=True):
        """One fused tick of every sub-batch, each on its own stream.  actions: [n_envs, capacity] float64 (or a list of
        per-sub-batch tensors, or None).  Returns the list of per-sub-batch output dicts.
        wait=True orders every sub-batch stream after torch's current stream (where `actions` are normally produced);
        pass wait=False when the actions are known to be complete (e.g. a tape uploaded and synchronised earlier)."""
        outs = []
        for k, (sub, a) in enumerate(zip(self.subs, self._parts(actions))):
            if a is not None and self.streams[k] is not None:
                # device-produced actions (a policy forward on torch's current stream) must be complete before the
                # tick of sub-batch k reads them: an event wait, no host synchronisation
                if wait:
                    self.streams[k].wait_stream(torch.cuda.current_stream(self.device))
                a.record_stream(self.streams[k])       # the caching allocator must not recycle it under the kernel
            outs.append(sub.step(a))
        return outs

    def set_actor(self, weights):
        for k, sub in enumerate(self.subs):
            with self._on(k):
                sub.set_actor(weights)

    def set_target_networks(self, actor=None, critic=None):
        for k, sub in enumerate(self.subs):
            with self._on(k):
                sub.set_target_networks(actor, critic)

    def critic_q(self, rows, act7, out=None):
        """BatchedIntersections.critic_q per sub-batch: rows / act7 (/ out) as lists of per-sub-batch tensors, or tensors
        whose first dimension is the environment (cut at `bounds`).  Returns the list of per-sub-batch results."""
        return [sub.critic_q(r, a, out=o) for sub, r, a, o in zip(self.subs, self._parts(rows), self._parts(act7), self._parts(out))]

    def bootstrap_q(self, state=None, flags=None, out=None, actions_out=None):
        """BatchedIntersections.bootstrap_q per sub-batch (each on its own stream; state=None: every sub-batch's own
        state_pre / flags).  Explicit arguments: lists of per-sub-batch tensors, or tensors whose first dimension is the
        environment.  Returns the list of per-sub-batch (q, act7) pairs."""
        return [sub.bootstrap_q(s, f, out=o, actions_out=a)
                for sub, s, f, o, a in zip(self.subs, self._parts(state), self._parts(flags), self._parts(out), self._parts(actions_out))]

    def nstep_transitions(self, gamma, window=13, prev=None, q=None, tail=False, max_records=None):
        """BatchedIntersections.nstep_transitions per sub-batch (each on its own stream), the pieces concatenated in env order
        (within a piece: tick, env, slot ascending); the index carries GLOBAL env numbers.  prev / q: None, or lists with one
        entry per sub-batch (what step_many / bootstrap_q returned).  max_records bounds every piece.  Reads every piece's
        total (one synchronisation per sub-batch).  Returns (records, index, total)."""
        recs, idxs, tot = [], [], 0
        qs = [None] * self.n_sub if q is None else [x[0] if isinstance(x, tuple) else x for x in q]
        for k, (sub, p, qk) in enumerate(zip(self.subs, self._parts(prev), qs)):
            r, ix, n = sub.nstep_transitions(gamma, window=window, prev=p, q=qk, tail=tail, max_records=max_records)
            n = int(n)
            m = min(n, r.shape[0])
            with self._on(k):
                ix = ix[:m].clone()
                ix[:, 1] += self.bounds[k]
            recs.append(r[:m]); idxs.append(ix); tot += n
        self.synchronize()
        return torch.cat(recs), torch.cat(idxs), tot

    def set_exploration(self, sigma, seed=0):
        """BatchedIntersections.set_exploration for every sub-batch, each with the global index of its first environment:
        the pieces draw the noise one batch of n_envs environments draws."""
        for k, sub in enumerate(self.subs):
            sub.set_exploration(sigma, seed, env_offset=self.bounds[k])

    def generate_arrivals(self, rate, horizon_s=None, rows=None, seed=0, epoch=0, env_offset=0, min_gap=1.0, covered=False):
        """BatchedIntersections.generate_arrivals for every sub-batch on its own stream, each with the global index of its
        first environment (+ env_offset): the pieces generate the streams one batch of n_envs environments generates.
        rate: a scalar or [n_envs], cut at `bounds`.  Returns the list of per-sub-batch `covered` tensors, or None."""
        from .arrivals import default_rows
        host_rate = rate.cpu().numpy() if torch.is_tensor(rate) and rate.device.type != "cuda" else rate
        if rows is None and horizon_s is not None and not torch.is_tensor(host_rate):
            rows = default_rows(host_rate, horizon_s)             # (one row count for all pieces: the largest rate of the batch)
        per_env = torch.is_tensor(host_rate) or np.ndim(host_rate) > 0
        cov = []
        for k, sub in enumerate(self.subs):
            with self._on(k):
                cov.append(sub.generate_arrivals(host_rate[self.bounds[k]:self.bounds[k + 1]] if per_env else host_rate, horizon_s=horizon_s,
                                                 rows=rows, seed=seed, epoch=epoch, env_offset=int(env_offset) + self.bounds[k],
                                                 min_gap=min_gap, covered=covered))
        return cov if covered else None

    def step_with_actor(self):
        return [sub.step_with_actor() for sub in self.subs]

    def set_action_table(self, table):
        for k, sub in enumerate(self.subs):
            with self._on(k):
                sub.set_action_table(table)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def set_action_pool(self, pool):
        pool = torch.as_tensor(pool, dtype=torch.float64)
        for k, sub in enumerate(self.subs):
            with self._on(k):
                sub.set_action_pool(pool[:, self.bounds[k]:self.bounds[k + 1]].contiguous())
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def alloc_trajectory(self, n_ticks):
        return [sub.alloc_trajectory(n_ticks) for sub in self.subs]

    def step_many(self, n_ticks, actor=False, source=None, trajectory=False, chunk=0, update_views=True, persistent=False):
        """n_ticks of every sub-batch, one pve_step_many call each (on its own stream).  chunk > 0 splits every call into
        launches of `chunk` ticks: a launch lasts as long as its slowest intersection, and the other sub-batches'
        workgroups fill the slots its fast ones free, so short launches keep the chip full.
        trajectory: False / True / the list alloc_trajectory() returned (one dict per sub-batch)."""
        tr = trajectory if isinstance(trajectory, (list, tuple)) else [trajectory] * self.n_sub
        return [sub.step_many(n_ticks, actor=actor, source=source, trajectory=tr[k], chunk=chunk, update_views=update_views,
                              persistent=persistent)
                for k, sub in enumerate(self.subs)]

    def prepare_step_many(self, n_ticks, source=None, chunk=0, persistent=False):
        """One prepared call per sub-batch (BatchedIntersections.prepare_step_many); the returned callable issues them all."""
        calls = [sub.prepare_step_many(n_ticks, source=source, chunk=chunk, persistent=persistent) for sub in self.subs]

        def call():
            for c in calls:
                c()
        return call

    def synchronize(self):
        for sub in self.subs:
            sub.synchronize()

    def last_launch(self):
        """last_launch() of every sub-batch, in order"""
        return [sub.last_launch() for sub in self.subs]

    def last_variant(self):
        """last_variant() of every sub-batch, in order (each sub-batch is a handle of its own and launches for itself)"""
        return [sub.last_variant() for sub in self.subs]

    def metrics(self):
        tot = None
        for sub in self.subs:
            m = sub.metrics()
            tot = m if tot is None else {k: tot[k] + m[k] for k in m}
        return tot

    def _sum_of_subs(self, parts):
        """parts[0] + parts[1] + ... in ascending sub-batch order on torch's current stream, which waits for every
        sub-batch's stream first (event waits, no host synchronisation)."""
        cur = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        res = None
        for k, p in enumerate(parts):
            if cur is not None and self.streams[k] is not None:
                cur.wait_stream(self.streams[k])
                p.record_stream(cur)
            res = p.clone() if res is None else res + p
        return res

    def _groups_of_subs(self, groups, n_groups, what):
        """(per-sub-batch maps, G).  A map on the device was produced on torch's current stream: every sub-batch's stream
        waits for that stream (an event wait) before its kernels read their slice."""
        if groups is None:
            return [None] * self.n_sub, n_groups
        on_device = torch.is_tensor(groups) and groups.device.type == "cuda"
        if n_groups is None:
            if on_device:
                raise PveError("%s: pass n_groups with a group map on the device" % what)
            n_groups = int(np.max(groups.numpy() if torch.is_tensor(groups) else np.asarray(groups))) + 1
        if not torch.is_tensor(groups):
            groups = np.asarray(groups)
        if on_device:
            self.wait_stream()
            for s in self.streams:
                groups.record_stream(s)
        return self._parts(groups), n_groups

    def _out_of_subs(self, out, parts):
        res = self._sum_of_subs(parts)
        if out is None:
            return res
        if not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != tuple(res.shape) or out.device != res.device:
            raise PveError("out must be a float64 device tensor of shape %s" % (tuple(res.shape),))
        return out.copy_(res)

    def rollout_stats(self, traj=None, groups=None, n_groups=None, out=None, totals=None, block_threads=0):
        """BatchedIntersections.rollout_stats of every sub-batch on its own stream (traj: None, or the list step_many
        returned; groups: [n_envs], cut at `bounds`; a map on the device is taken as produced on torch's current stream, which
        the sub-batches' streams then wait for), the per-sub-batch series added in ascending sub-batch order:
        series = (s_0 + s_1) + s_2 ... on torch's current stream, which waits for the sub-batches' streams.  The integer
        columns are those of one batch of n_envs environments; the four float columns are another fixed order than that
        batch's (one addition per sub-batch instead of one chain over all chunks), fixed by (n_envs, n_sub, the group map).
        totals [G, 14]: series[t] is added to it for t ascending, on the same stream (one small addition per tick: the order
        is the documented one, which a library reduction over t would not promise).  Returns the device tensor [T, G, 14]
        (`out` when given)."""
        gs, n_groups = self._groups_of_subs(groups, n_groups, "rollout_stats")
        tr = traj if isinstance(traj, (list, tuple)) else [traj] * self.n_sub
        parts = [sub.rollout_stats(tr[k], groups=gk, n_groups=n_groups, block_threads=block_threads)
                 for k, (sub, gk) in enumerate(zip(self.subs, gs))]
        series = self._out_of_subs(out, parts)
        if totals is not None:
            if totals.dtype != torch.float64 or tuple(totals.shape) != tuple(series.shape[1:]):
                raise PveError("rollout_stats: totals must be a float64 device tensor [n_groups, 14]")
            for t in range(series.shape[0]):
                totals.add_(series[t])
        return series

    def metrics_by_group(self, groups=None, n_groups=None, out=None):
        """BatchedIntersections.metrics_by_group of every sub-batch on its own stream, added in ascending sub-batch order on
        torch's current stream (the counters exact; sum_reward / sum_jerk one addition per sub-batch).  groups as
        rollout_stats.  Device tensor [G, 12] (`out` when given)."""
        gs, n_groups = self._groups_of_subs(groups, n_groups, "metrics_by_group")
        return self._out_of_subs(out, [sub.metrics_by_group(gk, n_groups) for sub, gk in zip(self.subs, gs)])

    def sub_of(self, env):
        """(sub-batch index, local env index) of a global env index."""
        for k in range(self.n_sub):
            if env < self.bounds[k + 1]:
                return k, env - self.bounds[k]
        raise IndexError(env)

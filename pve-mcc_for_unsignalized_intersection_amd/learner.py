"""The MADDPG learner step (csrc/pve_learn.h; reference main.py:48-84 `train_agent_seq`: model_agent_maddpg.py:85-118
`train_critic`, `train_actor`, then main.py:19-33 the soft updates of both target networks) on the minibatches
`ReplayMemory.sample` writes.

`Learner` is the device side (pve_learner_init / pve_learner_step): one parameter block on the batch's device holds the four
networks, Adam's moments, the beta powers and a step count, and one launch runs any number of steps in sequence.
`LearnerModel` is the same step on NumPy arrays with a hand-written backward pass: the SEMANTIC statement, in float32 or float64.
The bit-level statement is the header (NumPy's matmul sums in an order of its own): the kernel is held bit for bit to a host
build of the header, the header to this model within float32 rounding, this model to an independent autograd derivation.

Per step, in the reference's order:
  1. critic_loss = mean((target - Q(s, a7))^2), Adam on the critic;
  2. actor_loss = -mean(Q(s, [actor(s), a7[1:]])) with the UPDATED critic, gradients with respect to the actor only, Adam on it;
  3. target = c1 * online + c2 * target for both networks, c1 = float32(1 - tau), c2 = float32(tau) (main.py:30).
Adam is tf.train.AdamOptimizer's update (TF 1.x ApplyAdam) as the header writes it down; it is this library's definition.
Not part of the step: td_error / update_priority (main.py:76-79, dead with rand_s=True) are critic_q() on the sampled rows and
PrioritizedReplayMemory.update_priority (replay.py).  The summaries main.py:286-304 writes per tick, and the collision rate that
keeps best.cptk (main.py:315-328), come from the roll-out's own outputs: BatchedIntersections.rollout_stats and stats.summaries
(stats.py)."""
import numpy as np

from . import _capi
from ._capi import PveError
from .critic import KEYS, flat_critic_weights

N_ACTOR, N_CRITIC = _capi.PVE_ACTOR_N_WEIGHTS, _capi.PVE_CRITIC_N_WEIGHTS
N_GRADS = N_CRITIC + N_ACTOR
# float offsets of the block's segments (include/pve_env.h PVE_LEARNER_*)
ACTOR, CRITIC, TARGET_ACTOR = _capi.LEARNER_ACTOR, _capi.LEARNER_CRITIC, _capi.LEARNER_TARGET_ACTOR
TARGET_CRITIC, M_ACTOR, V_ACTOR = _capi.LEARNER_TARGET_CRITIC, _capi.LEARNER_M_ACTOR, _capi.LEARNER_V_ACTOR
M_CRITIC, V_CRITIC, POWERS = _capi.LEARNER_M_CRITIC, _capi.LEARNER_V_CRITIC, _capi.LEARNER_POWERS
STEPS, GRAD, N_FLOATS = _capi.LEARNER_STEPS, _capi.LEARNER_GRAD, _capi.LEARNER_N_FLOATS
GRAD_ACTOR = GRAD + 6844
CRITIC_ONLY = _capi.LEARN_CRITIC_ONLY
SLICE, WIDE_ROW = _capi.LEARN_SLICE, _capi.LEARNER_WIDE_ROW         # step_wide: rows per slice, workspace floats per slice


def wide_floats(batch):
    """PVE_LEARNER_WIDE_FLOATS(batch): the float32 workspace pve_learner_step_wide needs for a batch"""
    return (int(batch) + SLICE - 1) // SLICE * WIDE_ROW


def _shapes(critic):
    k2 = 71 if critic else 64
    return (("ln0_gamma", (28,)), ("ln0_beta", (28,)), ("w1", (28, 64)), ("b1", (64,)), ("ln1_gamma", (64,)), ("ln1_beta", (64,)),
            ("w2", (k2, 64)), ("b2", (64,)), ("ln2_gamma", (64,)), ("ln2_beta", (64,)), ("w3", (64, 1)), ("b3", (1,)))


def flat_weights(w, critic):
    """dict (critic.KEYS) or flat array -> flat float32 [6393 | 6841] in the order pve_set_actor / pve_set_target_networks take"""
    if isinstance(w, dict):
        w = np.concatenate([np.asarray(w[k], np.float32).ravel() for k in KEYS])
    w = np.ascontiguousarray(np.asarray(w, np.float32).ravel())
    n = N_CRITIC if critic else N_ACTOR
    if w.size != n:
        raise ValueError("%s needs %d weights, got %d" % ("critic" if critic else "actor", n, w.size))
    return w


def unflat_weights(flat, critic):
    """flat [6393 | 6841] -> dict of views (critic.KEYS)"""
    flat = np.asarray(flat)
    out, o = {}, 0
    for k, s in _shapes(critic):
        n = int(np.prod(s))
        out[k] = flat[o:o + n].reshape(s)
        o += n
    assert o == flat.size
    return out


def _flat_grads(g):
    return np.concatenate([g[k].ravel() for k in KEYS])


def _ln_forward(x, gamma, beta, F):
    mean = x.mean(axis=-1, keepdims=True, dtype=F)
    d = x - mean
    var = np.mean(d * d, axis=-1, keepdims=True, dtype=F)
    rstd = F(1.0) / np.sqrt(var + F(np.float32(1e-12)))
    xh = d * rstd
    return xh * gamma + beta, xh, rstd


def _ln_backward(dy, xh, rstd, gamma, F):
    dxh = dy * gamma
    m1 = dxh.mean(axis=-1, keepdims=True, dtype=F)
    m2 = (dxh * xh).mean(axis=-1, keepdims=True, dtype=F)
    return rstd * (dxh - m1 - xh * m2), (dy * xh).sum(axis=0, dtype=F), dy.sum(axis=0, dtype=F)


def net_forward(w, rows, act7=None, dtype=np.float32):
    """Forward with a tape.  act7 given: the critic ([h, own action, six others] into dense_1), output Q; else the actor,
    output 3 tanh."""
    F = dtype
    t = {"x": np.asarray(rows, np.float32).astype(F)}
    t["a0"], t["xh0"], t["r0"] = _ln_forward(t["x"], w["ln0_gamma"], w["ln0_beta"], F)
    y1, t["xh1"], t["r1"] = _ln_forward(t["a0"] @ w["w1"] + w["b1"], w["ln1_gamma"], w["ln1_beta"], F)
    t["y1"] = np.maximum(y1, F(0))
    t["in2"] = t["y1"] if act7 is None else np.concatenate([t["y1"], np.asarray(act7).astype(F)], axis=-1)
    y2, t["xh2"], t["r2"] = _ln_forward(t["in2"] @ w["w2"] + w["b2"], w["ln2_gamma"], w["ln2_beta"], F)
    t["y2"] = np.maximum(y2, F(0))
    z = (t["y2"] @ w["w3"] + w["b3"])[..., 0]
    t["out"] = z if act7 is not None else F(3.0) * np.tanh(z)
    return t


def net_backward(w, t, dout, dtype=np.float32):
    """dout = d loss / d (dense_2 output) [batch] -> (gradient dict, d loss / d in2 [batch, 64 | 71])"""
    F = dtype
    g = {}
    dz = dout[:, None]
    g["w3"], g["b3"] = t["y2"].T @ dz, dz.sum(axis=0, dtype=F)
    dy2 = (dz @ w["w3"].T) * (t["y2"] > 0)
    dh2, g["ln2_gamma"], g["ln2_beta"] = _ln_backward(dy2, t["xh2"], t["r2"], w["ln2_gamma"], F)
    g["w2"], g["b2"] = t["in2"].T @ dh2, dh2.sum(axis=0, dtype=F)
    din2 = dh2 @ w["w2"].T
    dy1 = din2[:, :64] * (t["y1"] > 0)
    dh1, g["ln1_gamma"], g["ln1_beta"] = _ln_backward(dy1, t["xh1"], t["r1"], w["ln1_gamma"], F)
    g["w1"], g["b1"] = t["a0"].T @ dh1, dh1.sum(axis=0, dtype=F)
    da0 = dh1 @ w["w1"].T
    g["ln0_gamma"], g["ln0_beta"] = (da0 * t["xh0"]).sum(axis=0, dtype=F), da0.sum(axis=0, dtype=F)
    return g, din2


def adam_update(w, m, v, g, lr, b1p, b2p, beta1, beta2, epsilon, F=np.float32):
    """One ApplyAdam in the arithmetic F, every operation rounded on its own -> (w, m, v, b1p, b2p)"""
    lr, b1p, b2p, beta1, beta2, epsilon = (F(np.float32(x)) if F is np.float32 else F(x) for x in (lr, b1p, b2p, beta1, beta2, epsilon))
    alpha = lr * np.sqrt(F(1.0) - b2p) / (F(1.0) - b1p)
    m = m + (g - m) * (F(1.0) - beta1)
    v = v + (g * g - v) * (F(1.0) - beta2)
    w = w - (m * alpha) / (np.sqrt(v) + epsilon)
    return w, m, v, b1p * beta1, b2p * beta2


def soft_update(online, target, tau, F=np.float32):
    """target <- c1 * online + c2 * target, c1 = float32(1.0 - (double)tau), c2 = float32(tau), products rounded separately"""
    c1, c2 = F(np.float32(1.0 - float(np.float32(tau)))), F(np.float32(tau))
    p1, p2 = c1 * online, c2 * target
    return p1 + p2


class LearnerModel:
    """The learner step on NumPy arrays.  Networks: dicts (critic.KEYS) or flat float32 arrays.  dtype = the arithmetic; the
    hyper-parameters and the networks are float32 values either way."""

    def __init__(self, actor, critic, target_actor=None, target_critic=None, actor_lr=1e-4, critic_lr=1e-3, tau=0.998,
                 beta1=0.9, beta2=0.999, epsilon=1e-8, dtype=np.float32):
        F = self.F = dtype
        f32 = lambda x: F(np.float32(x))                                     # noqa: E731
        self.actor_lr, self.critic_lr, self.tau = f32(actor_lr), f32(critic_lr), np.float32(tau)
        self.beta1, self.beta2, self.epsilon = f32(beta1), f32(beta2), f32(epsilon)
        a, c = flat_weights(actor, False), flat_weights(critic, True)
        self.net = {"actor": a.astype(F), "critic": c.astype(F),
                    "target_actor": (a if target_actor is None else flat_weights(target_actor, False)).astype(F),
                    "target_critic": (c if target_critic is None else flat_weights(target_critic, True)).astype(F)}
        self.m = {k: np.zeros_like(self.net[k]) for k in ("actor", "critic")}
        self.v = {k: np.zeros_like(self.net[k]) for k in ("actor", "critic")}
        self.powers = {k: [self.beta1, self.beta2] for k in ("actor", "critic")}
        self.steps = 0

    # ---- the block of the device side / the host build
    def load_block(self, block):
        """take the whole state from a float32 block [N_FLOATS] (Learner.state_dict()["params"], or the host build's)"""
        F, b = self.F, np.asarray(block, np.float32)
        for k, o, n in (("actor", ACTOR, N_ACTOR), ("critic", CRITIC, N_CRITIC), ("target_actor", TARGET_ACTOR, N_ACTOR),
                        ("target_critic", TARGET_CRITIC, N_CRITIC)):
            self.net[k] = b[o:o + n].astype(F)
        self.m = {"actor": b[M_ACTOR:M_ACTOR + N_ACTOR].astype(F), "critic": b[M_CRITIC:M_CRITIC + N_CRITIC].astype(F)}
        self.v = {"actor": b[V_ACTOR:V_ACTOR + N_ACTOR].astype(F), "critic": b[V_CRITIC:V_CRITIC + N_CRITIC].astype(F)}
        self.powers = {"actor": [F(b[POWERS]), F(b[POWERS + 1])], "critic": [F(b[POWERS + 2]), F(b[POWERS + 3])]}
        self.steps = int(b[STEPS:STEPS + 1].view(np.int32)[0])

    # ---- the two losses and their gradients (flat, in the networks' own order)
    def critic_gradients(self, rows, act7, target):
        F = self.F
        w = unflat_weights(self.net["critic"], True)
        t = net_forward(w, rows, np.asarray(act7, np.float32), F)
        tgt = np.asarray(target, np.float32).astype(F)
        B = F(len(tgt))
        d = tgt - t["out"]
        g, _ = net_backward(w, t, F(2.0) * (t["out"] - tgt) / B, F)
        return (d * d).sum(dtype=F) / B, _flat_grads(g)

    def actor_gradients(self, rows, act7):
        F = self.F
        wa, wc = unflat_weights(self.net["actor"], False), unflat_weights(self.net["critic"], True)
        ta = net_forward(wa, rows, None, F)
        a7 = np.asarray(act7, np.float32).astype(F).copy()
        a7[:, 0] = ta["out"]
        tc = net_forward(wc, rows, a7, F)
        B = F(len(a7))
        _, din2 = net_backward(wc, tc, np.full(len(a7), F(-1.0) / B, F), F)
        th = ta["out"] / F(3.0)
        g, _ = net_backward(wa, ta, din2[:, 64] * (F(3.0) * (F(1.0) - th * th)), F)
        return -(tc["out"].sum(dtype=F) / B), _flat_grads(g)

    def _apply(self, k, g, lr):
        F = self.F
        self.net[k], self.m[k], self.v[k], b1p, b2p = adam_update(self.net[k], self.m[k], self.v[k], g, lr, self.powers[k][0],
                                                                   self.powers[k][1], self.beta1, self.beta2, self.epsilon, F)
        self.powers[k] = [b1p, b2p]
        self.net["target_" + k] = soft_update(self.net[k], self.net["target_" + k], self.tau, F)

    def step(self, rows, act7, target, critic_only=False):
        """One step on one minibatch -> (losses [2], grads [6841 + 6393]: what the step applied, critic then actor)"""
        lc, gc = self.critic_gradients(rows, act7, target)
        self._apply("critic", gc, self.critic_lr)
        la, ga = self.F(0), np.zeros(N_ACTOR, self.F)
        if not critic_only:
            la, ga = self.actor_gradients(rows, act7)
            self._apply("actor", ga, self.actor_lr)
        self.steps += 1
        return np.array([lc, la], self.F), np.concatenate([gc, ga])


class Learner:
    """The learner on the device of `batch` (a BatchedIntersections): the parameter block is allocated there, every call runs
    on the batch's handle and stream, asynchronously.  actor / critic / targets: dicts (critic.KEYS) or flat float32 arrays or
    tensors; a target left None starts as a copy of its online network (main.py:203-204)."""

    def __init__(self, batch, actor, critic, target_actor=None, target_critic=None, actor_lr=1e-4, critic_lr=1e-3, tau=0.998,
                 beta1=0.9, beta2=0.999, epsilon=1e-8, block_threads=0):
        import torch
        self._torch = torch
        self.batch = batch
        self._lr = _capi.PveLearner()
        self._lr.actor_lr, self._lr.critic_lr, self._lr.tau = actor_lr, critic_lr, tau
        self._lr.beta1, self._lr.beta2, self._lr.epsilon = beta1, beta2, epsilon
        self._lr.flags, self._lr.block_threads = 0, int(block_threads)
        with batch._own_stream():
            self.params = torch.zeros(N_FLOATS, dtype=torch.float32, device=batch.device)
            self._lr.params = self.params.data_ptr()
            nets = []
            for w, crit in ((actor, False), (critic, True), (target_actor, False), (target_critic, True)):
                if w is None:
                    nets.append(None)
                    continue
                if torch.is_tensor(w):
                    w = w.detach().cpu().numpy()
                nets.append(torch.from_numpy(flat_weights(w, crit)).to(batch.device))
            batch._call("pve_learner_init", self._lr, *nets)
            self._init_sources = nets                                         # (alive until the copy has run)

    def _minibatches(self, method, rows, act7, target, losses, grads, critic_only):
        """The arguments `step` and `step_wide` share, checked and made contiguous -> (rows, act7, target, batch, n_batches,
        [losses, grads]); sets the descriptor's flags.  Runs inside the batch's stream context."""
        from ._args import is_tensor_of, tensor_out
        torch, dev = self._torch, self.params.device
        for x, what in ((rows, "rows"), (act7, "act7"), (target, "target")):
            if not is_tensor_of(x, torch.float32, dev, same_device=True):
                raise PveError("Learner.%s: %s must be a float32 tensor on %s" % (method, what, dev))
        if rows.dim() == 2:
            rows, act7, target = rows[None], act7[None], target[None]
        if rows.dim() != 3 or rows.shape[2] != 28 or rows.shape[1] < 1 or rows.shape[0] < 1 or \
                tuple(act7.shape) != tuple(rows.shape[:2]) + (7,) or tuple(target.shape) != tuple(rows.shape[:2]):
            raise PveError("Learner.%s: rows [n_batches, batch, 28], act7 [.., 7] and target [..] are needed" % method)
        n, B = int(rows.shape[0]), int(rows.shape[1])
        outs = [None if o is None or o is False else
                tensor_out(None if o is True else o, dev, torch.float32, (n, width),
                           "Learner.%s: %s must be a contiguous float32 device tensor [%d, %d]" % (method, what, n, width), same_device=True)
                for o, width, what in ((losses, 2, "losses"), (grads, N_GRADS, "grads"))]
        self._lr.flags = CRITIC_ONLY if critic_only else 0
        return rows.contiguous(), act7.contiguous(), target.contiguous(), B, n, outs

    def step(self, rows, act7, target, losses=None, grads=None, critic_only=False):
        """Run one learner step per minibatch, in order.  rows float32 [batch, 28] or [n_batches, batch, 28], act7 [.., 7],
        target [..]: device tensors as ReplayMemory.sample returns them.  losses: True or a float32 device tensor
        [n_batches, 2] to receive (critic loss, actor loss) per step; grads: True or a tensor [n_batches, 6841 + 6393] to
        receive the gradients each step applied.  Returns (losses, grads), None where not asked for.  Never synchronises."""
        with self.batch._own_stream():
            rows, act7, target, B, n, outs = self._minibatches("step", rows, act7, target, losses, grads, critic_only)
            self.batch._call("pve_learner_step", self._lr, rows, act7, target, B, n, *outs)
        return outs[0], outs[1]

    def step_wide(self, rows, act7, target, losses=None, grads=None, critic_only=False, groups=0):
        """`step` for large batches (pve_learner_step_wide): the batch is cut into slices of 128 rows, the slices are worked by
        one workgroup each across the chip and their gradients added in ascending slice order (csrc/pve_learn.h,
        learn_steps_wide).  Same arguments and return value as `step`; up to 128 rows the same bits as `step`, beyond that a
        different, equally fixed order of summation that depends on the batch size alone.  groups: workgroups of the slice
        passes, 0 = one per slice up to the device's compute units (no result depends on it).  The workspace is allocated on the
        batch's stream, kept, and grown with the batch.  Never synchronises."""
        with self.batch._own_stream():
            rows, act7, target, B, n, outs = self._minibatches("step_wide", rows, act7, target, losses, grads, critic_only)
            need = wide_floats(B)
            work = getattr(self, "_wide_work", None)
            if work is None or work.numel() < need:
                # (never zeroed: every float a launch reads was written by an earlier launch of the same call)
                work = self._wide_work = self._torch.empty(need, dtype=self._torch.float32, device=self.params.device)
            self.batch._call("pve_learner_step_wide", self._lr, rows, act7, target, B, n, work, work.numel(), int(groups), *outs)
        return outs[0], outs[1]

    # ---- views of the block, in the layouts set_actor / set_target_networks take
    @property
    def actor_weights(self):
        return self.params[ACTOR:ACTOR + N_ACTOR]

    @property
    def critic_weights(self):
        return self.params[CRITIC:CRITIC + N_CRITIC]

    @property
    def target_actor_weights(self):
        return self.params[TARGET_ACTOR:TARGET_ACTOR + N_ACTOR]

    @property
    def target_critic_weights(self):
        return self.params[TARGET_CRITIC:TARGET_CRITIC + N_CRITIC]

    def install(self):
        """Make the batch act with the online actor and bootstrap with the target networks as they are now: set_actor and
        set_target_networks on the block's own segments, device to device on the batch's stream."""
        self.batch.set_actor(self.actor_weights)
        self.batch.set_target_networks(self.target_actor_weights, self.target_critic_weights)

    def steps(self):
        """steps taken; synchronises"""
        with self.batch._own_stream():
            return int(self.params[STEPS:STEPS + 1].view(self._torch.int32)[0].item())

    def state_dict(self):
        with self.batch._own_stream():
            return {"params": self.params.clone()}

    def load_state_dict(self, state):
        p = state["params"]
        if tuple(p.shape) != (N_FLOATS,):
            raise PveError("Learner.load_state_dict: params must be float32 [%d]" % N_FLOATS)
        with self.batch._own_stream():
            self.params.copy_(self._torch.as_tensor(p, dtype=self._torch.float32))

#!/usr/bin/env python3
"""Time of the learner step (pve_learner_step: critic step, actor step, both soft updates per minibatch, any number of minibatches
in one launch of one workgroup) against what a trainer has without it: the same step written in eager torch on the device
(F.layer_norm / F.linear networks, autograd, torch.optim.Adam, in-place soft updates), in one process, alternating.

    python tools/bench_learner.py [--reps 9] [--torch-reps 3] [--out profiles/learner_bench.txt]

Batch 128; 1, 32 and 1024 minibatches per call; rows, actions and targets from tests/golden/critic_graph.npz, networks from the
same fixture and tests/golden/actor_66.npz.  Times are wall clock around the call with a device synchronisation (medians)."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import pve_mcc_amd  # noqa: E402
from pve_mcc_amd import learner as LN  # noqa: E402
from pve_mcc_amd.arrivals import synthetic_arrivals  # noqa: E402
from pve_mcc_amd.critic import KEYS  # noqa: E402

HYPER = dict(actor_lr=1e-4, critic_lr=1e-3, tau=0.998)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


class TorchLearner:
    """The same step from torch ops: what a trainer writes on the parent commit (a second copy of the weights, kept in step by hand)."""

    def __init__(self, nets, dev):
        def net(flat, critic):
            return {k: torch.tensor(v.copy(), device=dev, requires_grad=True) for k, v in LN.unflat_weights(flat, critic).items()}
        self.actor, self.critic, self.t_actor, self.t_critic = (net(w, c) for w, c in zip(nets, (False, True, False, True)))
        self.opt_a = torch.optim.Adam(list(self.actor.values()), lr=HYPER["actor_lr"], eps=1e-8)
        self.opt_c = torch.optim.Adam(list(self.critic.values()), lr=HYPER["critic_lr"], eps=1e-8)

    @staticmethod
    def forward(w, x, act7=None):
        x = F.layer_norm(x, (28,), w["ln0_gamma"], w["ln0_beta"], 1e-12)
        x = F.relu(F.layer_norm(x @ w["w1"] + w["b1"], (64,), w["ln1_gamma"], w["ln1_beta"], 1e-12))
        if act7 is not None:
            x = torch.cat([x, act7], dim=-1)
        x = F.relu(F.layer_norm(x @ w["w2"] + w["b2"], (64,), w["ln2_gamma"], w["ln2_beta"], 1e-12))
        z = (x @ w["w3"] + w["b3"])[..., 0]
        return z if act7 is not None else 3.0 * torch.tanh(z)

    def step(self, rows, act7, target):
        for k in range(rows.shape[0]):
            r, a, t = rows[k], act7[k], target[k]
            self.opt_c.zero_grad(set_to_none=True)
            ((t - self.forward(self.critic, r, a)) ** 2).mean().backward()
            self.opt_c.step()
            self.opt_a.zero_grad(set_to_none=True)
            act = torch.cat([self.forward(self.actor, r)[:, None], a[:, 1:]], dim=-1)
            (-self.forward(self.critic, r, act).mean()).backward()
            self.opt_a.step()
            with torch.no_grad():
                for online, tgt in ((self.actor, self.t_actor), (self.critic, self.t_critic)):
                    torch._foreach_mul_(list(tgt.values()), HYPER["tau"])
                    torch._foreach_add_(list(tgt.values()), list(online.values()), alpha=1.0 - HYPER["tau"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--torch-reps", type=int, default=3, help="repetitions of the eager-torch step at 1024 minibatches")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", 128
    z = np.load(os.path.join(ROOT, "tests", "golden", "critic_graph.npz"))
    za = np.load(os.path.join(ROOT, "tests", "golden", "actor_66.npz"))
    nets = [LN.flat_weights({k: za[k] for k in KEYS}, False), LN.flat_weights({k: z["critic__" + k] for k in KEYS}, True),
            LN.flat_weights({k: z["target_actor__" + k] for k in KEYS}, False), LN.flat_weights({k: z["target_critic__" + k] for k in KEYS}, True)]
    n_rows = len(z["states"])
    idx = np.random.default_rng(1).integers(0, n_rows, (1024, B))
    rows = torch.tensor(z["states"][:, 0].astype(np.float32)[idx], device=dev)
    act7 = torch.tensor(z["given_act7"][:n_rows].astype(np.float32)[idx], device=dev)
    target = torch.tensor(z["target_q_f32"].astype(np.float32)[idx], device=dev)
    env = pve_mcc_amd.BatchedIntersections(2, 64, synthetic_arrivals(2, rate=500.0, horizon_s=20.0, seed=1), device=dev,
                                           obs_dtype=torch.float32, outputs=("obs_post", "flags"))
    counts = (1, 32, 1024)
    lines = ["learner step, batch %d, wall clock around the call + device synchronisation (us, medians over %d alternating repetitions; "
             "eager torch at 1024 minibatches: %d)" % (B, args.reps, args.torch_reps),
             "device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]
    for threads in (1024, 256):
        lrn = pve_mcc_amd.Learner(env, *nets, block_threads=threads, **HYPER)
        ref = TorchLearner(nets, dev)
        lrn.step(rows[:2], act7[:2], target[:2])                    # warm-up: the function attribute, torch's first autograd pass
        ref.step(rows[:2], act7[:2], target[:2])
        for c in counts:
            reps_t = args.torch_reps if c == 1024 else args.reps
            T, Tt = [], []
            for rep in range(args.reps):
                T.append(timed(lambda: lrn.step(rows[:c], act7[:c], target[:c])))
                if rep < reps_t:
                    Tt.append(timed(lambda: ref.step(rows[:c], act7[:c], target[:c])))
            m, mt = float(np.median(T)), float(np.median(Tt))
            lines.append("block_threads %4d, step(%4d minibatches): library %10.1f (min %10.1f) = %7.1f per step | eager torch %11.1f "
                         "(min %11.1f) = %7.1f per step | ratio torch / library %.1f"
                         % (threads, c, m, min(T), m / c, mt, min(Tt), mt / c, mt / m))
        lines.append("  after %d steps every value of the library's block is finite: %s" % (lrn.steps(), bool(torch.isfinite(lrn.params).all())))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

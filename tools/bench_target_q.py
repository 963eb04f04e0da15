#!/usr/bin/env python3
"""Time of the bootstrap Q (pve_bootstrap_q: 7 target-actor tiles + 1 critic tile per 32 vehicles) on one tick's state_pre block,
against the only device evaluation of the same vehicles the library offered before: one pve_actor_forward pass over the batch.

    python tools/bench_target_q.py [--envs 4096] [--capacity 128] [--reps 30] [--out profiles/target_q_bench.txt]

4096 x 128 intersections, rate 1000, float32 rows; rolled to steady state with the pretrained actor, then the two calls
alternate in one process (warm-up, >= 20 synchronised repetitions each, medians).  Also reported: the controlled-vehicle count,
the bytes the call has to read (784 B of state + 4 B of flags per evaluated row, 4 B of flags per other row) over its time,
against bench.py's measured device copy peak, and critic_q alone on the same rows."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import pve_mcc_amd  # noqa: E402
from pve_mcc_amd import _capi  # noqa: E402
from pve_mcc_amd.arrivals import synthetic_arrivals  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm-ticks", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, cap, K = args.envs, args.capacity, 20
    dev = "cuda:0"
    z = np.load(os.path.join(ROOT, "tests", "golden", "critic_graph.npz"))
    keys = ("ln0_gamma", "ln0_beta", "w1", "b1", "ln1_gamma", "ln1_beta", "w2", "b2", "ln2_gamma", "ln2_beta", "w3", "b3")
    tactor = {k: z["target_actor__" + k] for k in keys}
    tcritic = {k: z["target_critic__" + k] for k in keys}
    arr = synthetic_arrivals(n, rate=1000.0, horizon_s=args.warm_ticks * 0.1 + 40.0, seed=20250213)
    env = pve_mcc_amd.BatchedIntersections(n, cap, arr, device=dev, obs_dtype=torch.float32,
                                           outputs=("obs_post", "obs_pre", "state_pre", "reward", "flags", "env_out"))
    env.set_actor(bench.actor_weights())
    env.set_target_networks(actor=tactor, critic=tcritic)
    env.reset()
    ring = env.alloc_trajectory(K)
    for _ in range(args.warm_ticks // K):
        env.step_many(K, source="actor", trajectory=ring, chunk=10)
    state, flags = ring["state_pre"][K - 1], ring["flags"][K - 1]
    f = flags.cpu().numpy()
    n_ev = int(((f & (_capi.F_CTL | _capi.F_DONE)) == _capi.F_CTL).sum())
    n_ctl_now = int(env.control_mask().sum().item())
    q = torch.empty(n, cap, dtype=torch.float32, device=dev)
    a7 = torch.empty(n, cap, 7, dtype=torch.float32, device=dev)

    def boot():
        env.bootstrap_q(state, flags, out=q, actions_out=a7)

    def actor():
        env.act()

    for _ in range(5):
        boot()
        actor()
    t_boot, t_act = [], []
    for _ in range(args.reps):                       # alternate in the same process
        t_boot += timed(boot, 1)
        t_act += timed(actor, 1)
    # the critic alone on every row of the block (it takes no flags), rows gathered once outside the timing
    rows0 = state[:, :, 0].contiguous()
    q2 = torch.empty(n, cap, dtype=torch.float32, device=dev)

    def crit():
        env.critic_q(rows0, a7, out=q2)
    for _ in range(3):
        crit()
    t_crit = timed(crit, args.reps)
    peak = bench.measured_copy_peak(torch, dev)
    mb, ma, mc = float(np.median(t_boot)), float(np.median(t_act)), float(np.median(t_crit))
    rd = n_ev * (7 * 28 * 4 + 4) + (n * cap - n_ev) * 4
    lines = [
        "bootstrap Q vs one actor pass, %d x %d, rate 1000, float32 rows, %d warm ticks, %d alternating repetitions (medians)"
        % (n, cap, args.warm_ticks // K * K, args.reps),
        "device: %s" % torch.cuda.get_device_name(0),
        "evaluated rows of the tick's block (controlled, not Done): %d of %d slots; controlled vehicles now: %d" % (n_ev, n * cap, n_ctl_now),
        "pve_bootstrap_q   : %8.1f us  (min %.1f)   %.2f ns per evaluated row" % (mb, min(t_boot), mb * 1e3 / max(n_ev, 1)),
        "pve_actor_forward : %8.1f us  (min %.1f)   %.2f ns per controlled vehicle" % (ma, min(t_act), ma * 1e3 / max(n_ctl_now, 1)),
        "ratio bootstrap / actor pass: %.2f   (per vehicle: %.2f; expectation <= 9: 7 actor tiles + a critic tile of 14/12 the blocks, 7 rows read instead of 1)"
        % (mb / ma, (mb / max(n_ev, 1)) / (ma / max(n_ctl_now, 1))),
        "pve_critic_forward on all %d rows: %8.1f us  (%.2f ns per row)" % (n * cap, mc, mc * 1e3 / (n * cap)),
        "bytes the bootstrap must read: %.1f MB -> %.0f GB/s, %.1f %% of the measured copy peak (%.0f GB/s read + write)"
        % (rd / 1e6, rd / (mb * 1e-6) / 1e9, 100.0 * rd / (mb * 1e-6) / 1e9 / peak, peak),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of the replay memory (pve_replay_append / pve_replay_sample) fed by 20-tick closed-loop calls, against what a trainer could
do before it existed: the same ring and selection built from torch ops on the device (`total.item()`, ring `index_copy_`, `randperm`
or `randint`, `index_select`, the three splits), in alternation in one process, and both outputs fed to critic_q.

    python tools/bench_replay.py [--envs 4096] [--capacity 128] [--reps 15] [--out profiles/replay_bench.txt]

4096 x 128 intersections, rate 1000, float32 rows, sigma 0.2; rolled to steady state with the pretrained actor, then every
repetition rolls 20 ticks, assembles the n-step records (about 2.95 M per call against a ring of 499 999, so only the last
`capacity` records of a call are written) and times the calls (synchronised, medians)."""
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
from pve_mcc_amd.arrivals import synthetic_arrivals  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


class TorchRing:
    """The ring and the draw from torch ops: what the parent commit's interface allows."""

    def __init__(self, capacity, batch, dev):
        self.capacity, self.batch, self.written = capacity, batch, 0
        self.store = torch.zeros(capacity, 36, dtype=torch.float32, device=dev)

    def add(self, records, total):
        n = min(int(total.item()), records.shape[0])               # the synchronisation: `total` is a device scalar
        skip = max(n - self.capacity, 0)
        slots = (self.written + torch.arange(skip, n, device=records.device)) % self.capacity
        self.store.index_copy_(0, slots, records[skip:n])
        self.written += n

    def split(self, age):
        L = min(self.written, self.capacity)
        slots = (self.written - L + age.reshape(-1)) % self.capacity
        rec = self.store.index_select(0, slots).view(age.shape[0], self.batch, 36)
        return rec[..., :28].contiguous(), rec[..., 28:35].contiguous(), rec[..., 35].contiguous()

    def sample_randint(self, n_batches):                           # with replacement: the cheap draw
        L = min(self.written, self.capacity)
        return self.split(torch.randint(L, (n_batches, self.batch), device=self.store.device))

    def sample_randperm(self, n_batches):                          # without replacement, as the reference draws
        L = min(self.written, self.capacity)
        return self.split(torch.stack([torch.randperm(L, device=self.store.device)[:self.batch] for _ in range(n_batches)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=128)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm-ticks", type=int, default=300)
    ap.add_argument("--buffer-size", type=int, default=500000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, cap, K, window, B = args.envs, args.capacity, 20, 13, 128
    gamma = float(np.tanh(6.0 / 12.0) * 0.9)
    dev = "cuda:0"
    z = np.load(os.path.join(ROOT, "tests", "golden", "critic_graph.npz"))
    keys = ("ln0_gamma", "ln0_beta", "w1", "b1", "ln1_gamma", "ln1_beta", "w2", "b2", "ln2_gamma", "ln2_beta", "w3", "b3")
    arr = synthetic_arrivals(n, rate=1000.0, horizon_s=(args.warm_ticks + 20 * (args.reps + 10)) * 0.1 + 40.0, seed=20250213)
    env = pve_mcc_amd.BatchedIntersections(n, cap, arr, device=dev, obs_dtype=torch.float32,
                                           outputs=("obs_post", "obs_pre", "state_pre", "reward", "flags", "new_slot", "env_out"))
    env.set_actor(bench.actor_weights())
    env.set_target_networks(actor={k: z["target_actor__" + k] for k in keys}, critic={k: z["target_critic__" + k] for k in keys})
    env.set_exploration(0.2, seed=1)
    env.reset()
    sets = [env.alloc_trajectory(K), env.alloc_trajectory(K)]
    calls = 0
    for _ in range(args.warm_ticks // K):
        env.step_many(K, source="actor", trajectory=sets[calls & 1], chunk=10)
        calls += 1
    mem = pve_mcc_amd.ReplayMemory(env, buffer_size=args.buffer_size, batch_size=B, seed=1)
    ring = TorchRing(mem.capacity, B, dev)
    max_rec = K * n * cap // 2
    counts = (1, 32, 1024)
    T = {k: [] for k in ["add", "t_add"] + ["s%d" % c for c in counts] + ["ri%d" % c for c in counts] + ["rp1", "rp32", "q", "t_q"]}
    totals, same = [], []
    for rep in range(args.reps + 3):
        prev, cur = sets[(calls + 1) & 1], sets[calls & 1]
        env.step_many(K, source="actor", trajectory=cur, chunk=10)
        calls += 1
        rec, _, total = env.nstep_transitions(gamma, window=window, prev=prev, max_records=max_rec)
        t = {}
        t["add"], _ = timed(lambda: mem.add(rec, total))
        t["t_add"], _ = timed(lambda: ring.add(rec, total))
        for c in counts:
            t["s%d" % c], out = timed(lambda: mem.sample(c, check=False))
            t["ri%d" % c], ref = timed(lambda: ring.sample_randint(c))
        for c in (1, 32):
            t["rp%d" % c], _ = timed(lambda: ring.sample_randperm(c))
        for k, x in ((("q", out), ("t_q", ref)) if rep & 1 else (("t_q", ref), ("q", out))):      # (alternating which goes first)
            t[k], _ = timed(lambda: env.critic_q(x[0], x[1]))
        if rep < 3:                                   # warm-up
            continue
        for k, v in t.items():
            T[k].append(v)
        totals.append(int(total))
        same.append(torch.equal(mem.store.view(torch.int32), ring.store.view(torch.int32)) and int(mem.state[0]) == ring.written)
    peak = bench.measured_copy_peak(torch, dev)
    med = lambda k: float(np.median(T[k]))                                 # noqa: E731
    written = min(float(np.median(totals)), mem.capacity)

    def rate(nbytes, us):
        return "%.1f MB -> %.0f GB/s, %.1f %% of the copy peak" % (nbytes / 1e6, nbytes / us / 1e3, 100.0 * nbytes / us / 1e3 / peak)
    lines = [
        "replay memory, %d x %d, rate 1000, float32 rows, %d-tick closed-loop calls (sigma 0.2), %d warm ticks, ring of %d records, "
        "batch_size %d, %d alternating repetitions (medians, us, host call + synchronisation included)"
        % (n, cap, K, args.warm_ticks // K * K, mem.capacity, B, args.reps),
        "device: %s; measured copy peak %.0f GB/s (read + write)" % (torch.cuda.get_device_name(0), peak),
        "records per call: %.0f (the last %d are written)" % (float(np.median(totals)), written),
        "add(records, total)                        : %9.1f  (min %.1f)   %s" % (med("add"), min(T["add"]), rate(written * 288, med("add"))),
        "  torch: total.item() + ring index_copy_   : %9.1f  (min %.1f)   ratio torch / library %.2f" % (med("t_add"), min(T["t_add"]), med("t_add") / med("add")),
    ]
    for c in counts:
        k = "s%d" % c
        lines.append("sample(%4d) x %d                           : %9.1f  (min %.1f)   %s" % (c, B, med(k), min(T[k]), rate(c * B * (288 + 8), med(k))))
        lines.append("  torch: randint, index_select, 3 splits   : %9.1f  (min %.1f)   ratio torch / library %.2f"
                     % (med("ri%d" % c), min(T["ri%d" % c]), med("ri%d" % c) / med(k)))
        if c <= 32:
            lines.append("  torch: randperm per minibatch instead    : %9.1f  (min %.1f)   ratio torch / library %.2f"
                         % (med("rp%d" % c), min(T["rp%d" % c]), med("rp%d" % c) / med(k)))
    lines += [
        "critic_q on sample(1024)'s rows, act7       : %9.1f  (min %.1f)" % (med("q"), min(T["q"])),
        "critic_q on the torch selection's tensors   : %9.1f  (min %.1f)" % (med("t_q"), min(T["t_q"])),
        "ring and count equal to the torch ring bit for bit after every call: %s" % ("every repetition" if all(same) else "NO (%d of %d)" % (sum(same), len(same))),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

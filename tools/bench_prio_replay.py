#!/usr/bin/env python3
"""Time of the prioritised replay memory (pve_prio_rank / pve_prio_sample / pve_prio_update) on a full memory of 500 000 records,
against (a) the uniform ReplayMemory.sample and (b) what a user could do before it existed: priorities and stamps kept in torch
tensors, the `written` synchronisation, keys built on the device, torch.sort(descending=True, stable=True), the stratified draw
with torch.rand, gathers, the three splits and the weights -- in alternation in one process.

    python tools/bench_prio_replay.py [--reps 15] [--out profiles/prio_replay_bench.txt]

Every live record holds a priority of its own (one update_priority over the whole memory); calls are timed synchronised, medians."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import pve_mcc_amd  # noqa: E402
from pve_mcc_amd.arrivals import synthetic_arrivals  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


class TorchPrio:
    """The same memory from torch ops on the ring and state block of a ReplayMemory: what the parent commit's interface allows."""

    def __init__(self, mem, ends, part_from, alpha_beta):
        dev = mem.store.device
        self.mem, self.capacity, self.batch = mem, mem.capacity, mem.batch_size
        self.prio = torch.zeros(self.capacity, dtype=torch.float32, device=dev)
        self.pseq = torch.full((self.capacity,), -1, dtype=torch.int64, device=dev)
        self.ends = torch.as_tensor(ends, device=dev).long()
        self.part_from, self.ab = part_from, alpha_beta

    def live(self):
        written = int(self.mem.state[0].item())                    # the synchronisation: `written` is a device scalar
        return written, min(written, self.capacity)

    def rank(self):
        written, L = self.live()
        w = written - 1 - torch.arange(L, device=self.prio.device)          # newest first
        slots = w % self.capacity
        p = torch.where(self.pseq[slots] == w, self.prio[slots], torch.full_like(self.prio[slots], float("inf")))
        _, at = torch.sort(p, descending=True, stable=True)
        return written, L, w[at]                                   # record numbers by rank

    def sample(self, n_batches):
        written, L, by_rank = self.rank()
        row = self.ends[int(np.count_nonzero(self.part_from <= L)) - 1]
        lo, hi = torch.minimum(row[:-1] + 1, row[1:]), torch.maximum(row[:-1] + 1, row[1:])
        u = torch.rand(n_batches, self.batch, device=row.device)
        rank = (lo + (u * (hi - lo + 1)).long()).clamp(1, L)
        seq = by_rank[rank - 1]
        rec = self.mem.store.index_select(0, (seq % self.capacity).reshape(-1)).view(n_batches, self.batch, 36)
        weight = (rank.float() / rank.max(dim=1, keepdim=True).values.float()) ** self.ab
        return rec[..., :28].contiguous(), rec[..., 28:35].contiguous(), rec[..., 35].contiguous(), seq, rank.int(), weight

    def update(self, seq, q, target):
        written, L = self.live()
        seq, p = seq.reshape(-1), (q - target).abs().reshape(-1)
        ok = (seq >= written - L) & (seq < written)
        slots = seq[ok] % self.capacity
        self.pseq[slots] = seq[ok]
        self.prio[slots] = 0
        self.prio.scatter_reduce_(0, slots, torch.nan_to_num(p[ok], nan=float("inf")), reduce="amax")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--buffer-size", type=int, default=500000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, B, size = "cuda:0", 128, args.buffer_size
    env = pve_mcc_amd.BatchedIntersections(2, 64, synthetic_arrivals(2, rate=500.0, horizon_s=20.0, seed=1), device=dev,
                                           obs_dtype=torch.float32, outputs=("obs_post", "flags"))
    mem = pve_mcc_amd.PrioritizedReplayMemory(env, buffer_size=size, batch_size=B, seed=1, learn_start=0, steps=100000)
    uni = pve_mcc_amd.ReplayMemory(env, buffer_size=size + 1, batch_size=B, seed=1)
    gen = torch.Generator(device=dev).manual_seed(5)
    rec = torch.randn(size + 1234, 36, device=dev, generator=gen)
    mem.add(rec)
    uni.add(rec)
    written = mem.count()
    live = torch.arange(written - size, written, device=dev)
    q = torch.rand(size, device=dev, generator=gen) * 10
    beta = 0.75
    ab = float(np.float32(mem.alpha * beta))
    ref = TorchPrio(mem, mem.ends, mem.part_from, ab)
    mem.update_priority(live, q)
    ref.update(live, q, torch.zeros_like(q))
    # same ranking from both (float priorities are pairwise distinct with overwhelming probability; ties would be ordered alike)
    order = mem.rank()[:size].long()
    same_rank = bool(torch.equal(written - size + order, ref.rank()[2]))
    counts = (1, 32, 1024)
    T = {k: [] for k in ["rank", "t_rank"] + [p + str(c) for c in counts for p in ("s", "t_s", "u", "upd", "t_upd")]}
    for rep in range(args.reps + 3):
        t = {}
        pairs = [("rank", mem.rank), ("t_rank", ref.rank)]
        for c in counts:
            pairs += [("s%d" % c, lambda c=c: mem.sample(c, beta=beta, check=False)), ("t_s%d" % c, lambda c=c: ref.sample(c)),
                      ("u%d" % c, lambda c=c: uni.sample(c, check=False))]
        for k, fn in (pairs if rep & 1 else pairs[::-1]):            # (alternating which goes first)
            t[k], out = timed(fn)
            if k[0] == "s":
                c = int(k[1:])
                qq = torch.rand(c, B, device=dev, generator=gen)
                t["upd%d" % c], _ = timed(lambda: mem.update_priority(out[3], qq, out[2]))
                t["t_upd%d" % c], _ = timed(lambda: ref.update(out[3], qq, out[2]))
        if rep >= 3:                                                 # (the first three: warm-up)
            for k, v in t.items():
                T[k].append(v)
    med = lambda k: float(np.median(T[k]))                           # noqa: E731
    lines = [
        "prioritised replay memory, %d records live (capacity %d, %d adds), batch_size %d, every record with a priority of its own, "
        "%d alternating repetitions (medians, us, host call + synchronisation included)" % (size, size, written, B, args.reps),
        "device: %s" % torch.cuda.get_device_name(0),
        "rank()                                           : %9.1f  (min %.1f)" % (med("rank"), min(T["rank"])),
        "  torch: written.item(), keys, stable sort       : %9.1f  (min %.1f)   ratio torch / library %.2f"
        % (med("t_rank"), min(T["t_rank"]), med("t_rank") / med("rank")),
        "  the two rankings agree: %s" % same_rank,
    ]
    for c in counts:
        lines += [
            "sample(%4d) x %d, ranking included              : %9.1f  (min %.1f)" % (c, B, med("s%d" % c), min(T["s%d" % c])),
            "  torch: sort + rand draw, gathers, splits, pow  : %9.1f  (min %.1f)   ratio torch / library %.2f"
            % (med("t_s%d" % c), min(T["t_s%d" % c]), med("t_s%d" % c) / med("s%d" % c)),
            "  uniform ReplayMemory.sample(%4d)              : %9.1f  (min %.1f)" % (c, med("u%d" % c), min(T["u%d" % c])),
            "update_priority of those %6d ids              : %9.1f  (min %.1f)" % (c * B, med("upd%d" % c), min(T["upd%d" % c])),
            "  torch: written.item(), masks, scatter amax     : %9.1f  (min %.1f)   ratio torch / library %.2f"
            % (med("t_upd%d" % c), min(T["t_upd%d" % c]), med("t_upd%d" % c) / med("upd%d" % c)),
        ]
    verdict = med("s32") <= med("t_s32")
    lines.append("requirement, sample(32) end to end no slower than the torch path: %s (%.1f against %.1f us)"
                 % ("met" if verdict else "NOT met", med("s32"), med("t_s32")))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

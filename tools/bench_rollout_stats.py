#!/usr/bin/env python3
"""Time of a roll-out's statistics at the headline shape (4096 envs x 128 slots, 20 ticks, float32 rows, training outputs on, closed
loop): (a) BatchedIntersections.rollout_stats (pve_rollout_stats) with one group and with seven, (b) the same fourteen columns
from torch ops on the same tensors (masked sums per (tick, env), then `sum` over the environments for one group, `index_add_`
by group for seven): what a user writes without the pass,
(c) the step_many roll-out that produced the blocks; the pass once more without obs_pre (no observation row is read) to show
what the row reads cost.  One process, alternating, one synchronisation around each call, medians.
Also metrics_by_group with seven groups against metrics(), which copies every header to the host and waits.

Bytes the pass must read: 12 B per slot (flags + reward), 32 B of env_out per (tick, env), one 64-B sector per controlled row
(its two values lie in one sector of the 112-byte row); achieved bytes / s against a device-to-device copy of 1 GiB (read +
write counted), the copy peak bench.py --full measures.

    python tools/bench_rollout_stats.py [--reps 15] [--envs 4096] [--ticks 20] [--out profiles/rollout_stats_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import pve_mcc_amd  # noqa: E402
from oracle.actor_np import flat_weights, load_weights  # noqa: E402
from pve_mcc_amd import stats as ST  # noqa: E402

TRAIN_OUTS = ("obs_post", "obs_pre", "state_pre", "reward", "flags", "nbr", "new_slot", "env_out")
EO_OF_COLUMN = (0, 6, 5, 4, 2, 3)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def med(xs):
    return float(np.median(xs))


def torch_stats(tr, groups, G):
    """The fourteen columns from torch ops: float64 [T, G, 14] (its own summation order: equal to the pass in the integer columns)"""
    f = tr["flags"]
    ctl = (f & 2) != 0
    zero = torch.zeros((), dtype=torch.float64, device=f.device)
    r = torch.where(ctl, tr["reward"], zero)
    v = torch.where(ctl, tr["obs_pre"][..., 1].double(), zero)
    a = torch.where(ctl, tr["obs_pre"][..., 2].double(), zero)
    eo = tr["env_out"].double()
    cols = [torch.ones(f.shape[:2], dtype=torch.float64, device=f.device)] + [eo[..., k] for k in EO_OF_COLUMN]
    cols += [ctl.sum(-1).double(), (ctl & ((f >> 8) > 0)).sum(-1).double(), (ctl & ((f & 4) != 0)).sum(-1).double(),
             r.sum(-1), (r * r).sum(-1), v.sum(-1), a.sum(-1)]
    rows = torch.stack(cols, -1)
    if G == 1:                                         # (one group: a plain sum over the environments)
        return rows.sum(1, keepdim=True)
    out = torch.zeros(f.shape[0], G, 14, dtype=torch.float64, device=f.device)
    return out.index_add_(1, groups, rows)


def copy_peak():
    n = 1 << 30
    a, b = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    best = min(timed(lambda: b.copy_(a))[0] for _ in range(6))
    return 2.0 * n / best * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--prefill", type=int, default=300)
    ap.add_argument("--rate", type=float, default=1000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    E, K, T = a.envs, 128, a.ticks
    b = pve_mcc_amd.BatchedIntersections(E, K, None, device="cuda", outputs=TRAIN_OUTS, obs_dtype=torch.float32)
    b.generate_arrivals(a.rate, horizon_s=(a.prefill + (2 * a.reps + 8) * T) * 0.1 + 60.0, seed=3)
    b.reset()
    b.set_actor(flat_weights(load_weights()))
    b.set_exploration(0.2, seed=11)
    ring = b.alloc_trajectory(T)
    for _ in range(a.prefill // T):
        b.step_many(T, source="actor", trajectory=ring)
    g7 = (torch.arange(E, device="cuda") % 7).int()
    g7_long, g1_long = g7.long(), torch.zeros(E, dtype=torch.long, device="cuda")
    tr = b.step_many(T, source="actor", trajectory=ring)
    s1, s7 = b.rollout_stats(), b.rollout_stats(groups=g7, n_groups=7)
    t1, t7 = torch_stats(tr, g1_long, 1), torch_stats(tr, g7_long, 7)
    want = ST.rollout_stats({k: tr[k][:, :256].cpu().numpy() for k in ("flags", "reward", "env_out", "obs_pre")})
    part = pve_mcc_amd.BatchedIntersections(256, K, None, device="cuda", outputs=("obs_post",), obs_dtype=torch.float32)
    got = part.rollout_stats({k: tr[k][:, :256].contiguous() for k in ("flags", "reward", "env_out", "obs_pre")})
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64)), "the kernel differs from the model"
    assert torch.equal(s1[..., :10], t1[..., :10]) and torch.equal(s7[..., :10], t7[..., :10]), "integer columns differ from the torch ops"
    assert torch.allclose(s7[..., 10:], t7[..., 10:], rtol=1e-9, atol=1e-6) and torch.allclose(s1[..., 10:], t1[..., 10:], rtol=1e-9, atol=1e-6)
    n_ctl = float(s1[:, 0, ST.COL["ctl"]].sum())
    need = 12.0 * T * E * K + 32.0 * T * E + 64.0 * n_ctl
    t_roll, t_s1, t_s7, t_t1, t_t7, t_mg, t_m, t_s1n = [], [], [], [], [], [], [], []
    no_rows = {k: tr[k] for k in ("flags", "reward", "env_out")}
    for _ in range(a.reps):
        t_roll.append(timed(lambda: b.step_many(T, source="actor", trajectory=ring))[0])
        t_s1.append(timed(lambda: b.rollout_stats())[0])
        t_t1.append(timed(lambda: torch_stats(tr, g1_long, 1))[0])
        t_s1n.append(timed(lambda: b.rollout_stats(no_rows))[0])
        t_s7.append(timed(lambda: b.rollout_stats(groups=g7, n_groups=7))[0])
        t_t7.append(timed(lambda: torch_stats(tr, g7_long, 7))[0])
        t_mg.append(timed(lambda: b.metrics_by_group(g7, 7))[0])
        t_m.append(timed(lambda: b.metrics())[0])
    peak = copy_peak()
    ok = med(t_s1) < med(t_t1) and med(t_s7) < med(t_t7)
    lines = ["roll-out statistics, %d envs x %d slots x %d ticks, float32 rows, training outputs on, closed loop at %.0f veh/h/lane "
             "(%s, torch %s), medians of %d, us" % (E, K, T, a.rate, torch.cuda.get_device_name(0), torch.__version__, a.reps),
             "controlled rows in the call: %.0f of %d slots; bytes the pass must read = 12 x slots + 32 x ticks x envs + 64 x controlled rows "
             "= %.1f MB; copy peak (1 GiB device to device, read + write) %.0f GB/s" % (n_ctl, T * E * K, need / 1e6, peak / 1e9),
             "(a) rollout_stats G = 1: %.1f (min %.1f; %.0f GB/s = %.2f of the copy peak)   G = 7: %.1f (min %.1f)"
             % (med(t_s1), min(t_s1), need / med(t_s1) / 1e3, need / med(t_s1) * 1e6 / peak, med(t_s7), min(t_s7)),
             "    without obs_pre (sum_v / sum_a 0: no row is read, %.1f MB) G = 1: %.1f (%.0f GB/s)"
             % ((need - 64.0 * n_ctl) / 1e6, med(t_s1n), (need - 64.0 * n_ctl) / med(t_s1n) / 1e3),
             "(b) the same columns from torch ops G = 1: %.1f   G = 7: %.1f   (b) / (a) = %.1f x / %.1f x"
             % (med(t_t1), med(t_t7), med(t_t1) / med(t_s1), med(t_t7) / med(t_s7)),
             "(c) the step_many roll-out of the %d ticks: %.1f (%.2f per tick)   (a) / (c) = %.3f (G = 1), %.3f (G = 7)"
             % (T, med(t_roll), med(t_roll) / T, med(t_s1) / med(t_roll), med(t_s7) / med(t_roll)),
             "metrics_by_group G = 7: %.1f (min %.1f)   metrics() (copies %d headers to the host and waits): %.1f   ratio %.1f x"
             % (med(t_mg), min(t_mg), E, med(t_m), med(t_m) / med(t_mg)),
             "requirement rollout_stats faster than the torch formulation, G = 1 and G = 7: %s" % ("met" if ok else "NOT met")]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

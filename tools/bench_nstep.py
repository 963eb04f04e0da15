#!/usr/bin/env python3
"""Time of the n-step transition pass (pve_nstep_scan + pve_nstep_gather) on a 20-tick closed-loop trajectory, next to the
roll-out that produced it and the bootstrap Q it consumes, against what a trainer could do before the pass existed:
  (a) the same selection written with torch gathers on the device (walk through new_slot, Horner fold, nonzero, row gathers);
  (b) the host path: a D2H copy of reward / flags / new_slot (+ q) and pve_mcc_amd/nstep.py's scan.

    python tools/bench_nstep.py [--envs 4096] [--capacity 128] [--reps 20] [--out profiles/nstep_bench.txt]

4096 x 128 intersections, rate 1000, float32 rows; rolled to steady state with the pretrained actor into two alternating
trajectory buffer sets, then the calls alternate in one process (warm-up, synchronised repetitions, medians)."""
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
from pve_mcc_amd import _capi, nstep  # noqa: E402
from pve_mcc_amd.arrivals import synthetic_arrivals  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def torch_nstep(cur, prev, q, gamma, window):
    """The pass with torch gathers (full windows and fresh vehicles that die early; the reference's default mode)."""
    cat = lambda k: torch.cat([prev[k][-window:], cur[k]])                 # noqa: E731
    flags, reward, new_slot, rows = cat("flags"), cat("reward"), cat("new_slot").long(), cat("obs_post")
    T, E, K = flags.shape
    n_cur, off = cur["flags"].shape[0], window
    n_back = window - 1
    n_cand = n_back + n_cur
    dev = flags.device
    t = torch.arange(-n_back, n_cur, device=dev).view(-1, 1, 1).expand(n_cand, E, K)
    base = (torch.arange(E, device=dev) * K).view(1, -1, 1).expand(n_cand, E, K)
    s = torch.arange(K, device=dev).view(1, 1, -1).expand(n_cand, E, K).clone()
    slot0, s_last = s.clone(), s.clone()
    walking = torch.ones(n_cand, E, K, dtype=torch.bool, device=dev)
    bad, done = torch.zeros_like(walking), torch.zeros_like(walking)
    n = torch.zeros(n_cand, E, K, dtype=torch.int32, device=dev)
    fl, rw, nx = flags.view(-1), reward.view(-1), new_slot.view(-1)
    r = []
    for k in range(window):
        tk = t + k
        pend = walking & (tk >= n_cur)
        bad |= pend
        walking = walking & ~pend
        i = torch.where(walking, (tk + off) * (E * K) + base + s, torch.zeros_like(s))
        f = fl[i]
        lost = walking & ((f & 2) == 0)
        bad |= lost
        walking = walking & ~lost
        r.append(torch.where(walking, rw[i], torch.zeros((), dtype=torch.float64, device=dev)))
        n = torch.where(walking, torch.full_like(n, k + 1), n)
        s_last = torch.where(walking, s, s_last)
        d = walking & ((f & 4) != 0)
        done |= d
        walking = walking & ~d
        if k + 1 < window:
            nxt = nx[i]
            broken = walking & ((nxt < 0) | (nxt >= K))
            bad |= broken
            walking = walking & ~broken
            s = torch.where(walking, nxt, s)
    t_close = t + n - 1
    ok = ~bad & (n > 0) & (t_close >= 0)
    row_i = torch.where(ok, (t + off - 1) * (E * K) + base + slot0, torch.zeros_like(s))
    fresh = ~(rows.view(-1, 28)[row_i] != 0).any(dim=-1)
    ok &= (n == window) | fresh
    boot = ok & ~done
    qi = torch.where(boot, t_close * (E * K) + base + s_last, torch.zeros_like(s))
    qq = torch.where(boot, q.view(-1)[qi].double(), torch.zeros((), dtype=torch.float64, device=dev))
    acc = torch.zeros(n_cand, E, K, dtype=torch.float64, device=dev)
    for k in range(window - 1, -1, -1):
        last = torch.where(boot, r[k] + gamma * qq, r[k])
        acc = torch.where(n - 1 == k, last, torch.where(n - 1 > k, r[k] + gamma * acc, acc))
    c, e, sl = torch.nonzero(ok, as_tuple=True)
    tt = c - n_back
    state = torch.cat([prev["state_pre"][-window:], cur["state_pre"]])
    rec = torch.cat([rows[tt + off - 1, e, sl].float(), state[tt + off, e, sl, :, 2].float(), acc[c, e, sl].float().unsqueeze(1)], dim=1)
    return rec, torch.stack([tt, e, sl], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--capacity", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm-ticks", type=int, default=300)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, cap, K, window = args.envs, args.capacity, 20, 13
    gamma = float(np.tanh(6.0 / 12.0) * 0.9)
    dev = "cuda:0"
    z = np.load(os.path.join(ROOT, "tests", "golden", "critic_graph.npz"))
    keys = ("ln0_gamma", "ln0_beta", "w1", "b1", "ln1_gamma", "ln1_beta", "w2", "b2", "ln2_gamma", "ln2_beta", "w3", "b3")
    arr = synthetic_arrivals(n, rate=1000.0, horizon_s=(args.warm_ticks + 40 * (args.reps + 10)) * 0.1 + 40.0, seed=20250213)
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
    q = torch.empty(K, n, cap, dtype=torch.float32, device=dev)
    a7 = torch.empty(K, n, cap, 7, dtype=torch.float32, device=dev)
    t_roll, t_boot, t_pass, t_torch, t_host, totals, agree = [], [], [], [], [], [], []
    max_rec = K * n * cap // 2
    for rep in range(args.reps + 3):
        prev, cur = sets[(calls + 1) & 1], sets[calls & 1]
        tr, _ = timed(lambda: env.step_many(K, source="actor", trajectory=cur, chunk=10))
        calls += 1
        tb, _ = timed(lambda: env.bootstrap_q(cur["state_pre"], cur["flags"], out=q, actions_out=a7))
        tp, out = timed(lambda: env.nstep_transitions(gamma, window=window, prev=prev, q=q, max_records=max_rec))
        tt, ref = timed(lambda: torch_nstep(cur, prev, q, gamma, window))
        if rep < 3:                                   # warm-up
            continue
        t_roll.append(tr); t_boot.append(tb); t_pass.append(tp); t_torch.append(tt)
        total = int(out[2])
        totals.append(total)
        agree.append(total == ref[0].shape[0] and torch.equal(out[0][:total], ref[0]))
        if len(t_host) < args.host_reps:
            def host():
                c = {k: cur[k].cpu().numpy() for k in ("reward", "flags", "new_slot")}
                p = {k: prev[k][-window:].cpu().numpy() for k in ("reward", "flags", "new_slot")}
                c["obs_post"], p["obs_post"] = cur["obs_post"].cpu().numpy(), prev["obs_post"][-window:].cpu().numpy()   # (the fresh test)
                return nstep.scan(c, gamma, window, prev=p, q=q.cpu().numpy())
            th, hs = timed(host)
            t_host.append(th)
            agree.append(int(np.count_nonzero(hs[1])) == total)
    peak = bench.measured_copy_peak(torch, dev)
    med = lambda x: float(np.median(x))                                    # noqa: E731
    total = med(totals)
    slots = (K + window - 1) * n * cap
    # bytes the pass must move: flags + new_slot + reward of every candidate start (16 B), target + code written and read (24 B),
    # per record 112 B row + 7 x 64 B sectors of state_pre + 4 B q read, 144 + 16 B written
    moved = slots * (16 + 24) + total * (112 + 7 * 64 + 4 + 160)
    lines = [
        "n-step transitions, %d x %d, rate 1000, float32 rows, window %d, %d-tick closed-loop trajectories (sigma 0.2), %d warm ticks, "
        "%d alternating repetitions (medians, us)" % (n, cap, window, K, args.warm_ticks // K * K, args.reps),
        "device: %s" % torch.cuda.get_device_name(0),
        "transitions per call: %.0f of %d candidate starts" % (total, slots),
        "roll-out (step_many, trajectory, training outputs) : %9.1f  (min %.1f)  %.1f us per tick" % (med(t_roll), min(t_roll), med(t_roll) / K),
        "bootstrap_q on the %d ticks                         : %9.1f  (min %.1f)" % (K, med(t_boot), min(t_boot)),
        "pve_nstep_scan + pve_nstep_gather                  : %9.1f  (min %.1f)  %.2f M records/s" % (med(t_pass), min(t_pass), total / med(t_pass)),
        "  bytes moved (lower bound) %.1f MB -> %.0f GB/s, %.1f %% of the measured copy peak (%.0f GB/s read + write)"
        % (moved / 1e6, moved / med(t_pass) / 1e3, 100.0 * moved / med(t_pass) / 1e3 / peak, peak),
        "same selection with torch gathers on the device    : %9.1f  (min %.1f)  ratio torch / pass %.2f" % (med(t_torch), min(t_torch), med(t_torch) / med(t_pass)),
        "host path (D2H of the small blocks + rows, nstep.py): %9.1f  (%d runs)     ratio host / pass %.1f" % (med(t_host), len(t_host), med(t_host) / med(t_pass)),
        "records equal to the torch formulation bit for bit, counts equal to the host path: %s" % ("every repetition" if all(agree) else "NO (%d of %d)" % (sum(agree), len(agree))),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

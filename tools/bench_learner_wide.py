#!/usr/bin/env python3
"""Time of the wide learner step (Learner.step_wide / pve_learner_step_wide: slices of 128 rows on a grid of workgroups, combined in
ascending slice order) against the one-workgroup step (Learner.step / pve_learner_step) on the same tensors and against the eager-torch
step of tools/bench_learner.py at the same batch.

    python tools/bench_learner_wide.py [--reps 7] [--out profiles/learner_wide_bench.txt]

Batches 128, 512, 2 048, 8 192 and 32 768; each as one call of 1 minibatch and one call of 32 minibatches.  The three run in one
process per (batch, minibatches) pair, alternating; times are wall clock around the call with a device synchronisation (medians),
reported per step and as samples / s.  Every pair runs in a child process under a time limit of its own; after a child that
fails or runs out of time nothing more is started.  The floor: at batch 8 192 step_wide at least 8 x faster per
step than pve_learner_step in the same run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BATCHES = (128, 512, 2048, 8192, 32768)
COUNTS = (1, 32)
FLOOR_BATCH, FLOOR = 8192, 8.0


def child(batch, count, reps):
    import torch
    import pve_mcc_amd
    from pve_mcc_amd import learner as LN
    from pve_mcc_amd.arrivals import synthetic_arrivals
    from pve_mcc_amd.critic import KEYS
    from bench_learner import HYPER, TorchLearner, timed

    dev = "cuda:0"
    z = np.load(os.path.join(ROOT, "tests", "golden", "critic_graph.npz"))
    za = np.load(os.path.join(ROOT, "tests", "golden", "actor_66.npz"))
    nets = [LN.flat_weights({k: za[k] for k in KEYS}, False), LN.flat_weights({k: z["critic__" + k] for k in KEYS}, True),
            LN.flat_weights({k: z["target_actor__" + k] for k in KEYS}, False), LN.flat_weights({k: z["target_critic__" + k] for k in KEYS}, True)]
    n_rows = len(z["states"])
    idx = np.random.default_rng(1).integers(0, n_rows, (count, batch))
    rows = torch.tensor(z["states"][:, 0].astype(np.float32)[idx], device=dev)
    act7 = torch.tensor(z["given_act7"][:n_rows].astype(np.float32)[idx], device=dev)
    target = torch.tensor(z["target_q_f32"].astype(np.float32)[idx], device=dev)
    env = pve_mcc_amd.BatchedIntersections(2, 64, synthetic_arrivals(2, rate=500.0, horizon_s=20.0, seed=1), device=dev,
                                           obs_dtype=torch.float32, outputs=("obs_post", "flags"))
    wide, narrow = pve_mcc_amd.Learner(env, *nets, **HYPER), pve_mcc_amd.Learner(env, *nets, **HYPER)
    ref = TorchLearner(nets, dev)
    # warm-up: the function attributes, the workspace, torch's first autograd pass at this shape
    wide.step_wide(rows[:1], act7[:1], target[:1])
    narrow.step(rows[:1, :128], act7[:1, :128], target[:1, :128])
    ref.step(rows[:1], act7[:1], target[:1])
    Tw, Tn, Tt = [], [], []
    for _ in range(reps):
        Tw.append(timed(lambda: wide.step_wide(rows, act7, target)))
        Tn.append(timed(lambda: narrow.step(rows, act7, target)))
        Tt.append(timed(lambda: ref.step(rows, act7, target)))
    finite = bool(torch.isfinite(wide.params).all()) and bool(torch.isfinite(narrow.params).all())
    print(json.dumps({"batch": batch, "count": count, "wide": float(np.median(Tw)), "wide_min": min(Tw), "narrow": float(np.median(Tn)),
                      "narrow_min": min(Tn), "torch": float(np.median(Tt)), "torch_min": min(Tt), "finite": finite,
                      "device": torch.cuda.get_device_name(0), "torch_version": torch.__version__,
                      "cus": torch.cuda.get_device_properties(0).multi_processor_count}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=float, default=150.0, help="seconds one (batch, minibatches) pair may take")
    ap.add_argument("--child", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return
    lines, floor_ratio, stopped = [], None, None
    for batch in BATCHES:
        for count in COUNTS:
            t0 = time.time()
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--child", str(batch), str(count)],
                                   stdout=subprocess.PIPE, universal_newlines=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                stopped = "batch %d x %d minibatches ran past its limit of %.0f s: nothing more was started" % (batch, count, args.limit)
                break
            if p.returncode != 0:
                stopped = "batch %d x %d minibatches ended with status %d: nothing more was started" % (batch, count, p.returncode)
                break
            r = json.loads(p.stdout.strip().splitlines()[-1])
            if not lines:
                lines += ["wide learner step: wall clock around the call + device synchronisation (us, medians over %d alternating "
                          "repetitions; one process per line)" % args.reps,
                          "device: %s, %d compute units; torch %s" % (r["device"], r["cus"], r["torch_version"]),
                          "per step = call / minibatches; samples / s = batch / per step"]
            per = {k: r[k] / count for k in ("wide", "narrow", "torch")}
            lines.append("batch %6d, %2d minibatches: step_wide %10.1f per step (%12.0f samples/s) | pve_learner_step %11.1f per step "
                         "(%11.0f samples/s) | eager torch %9.1f per step (%11.0f samples/s) | narrow / wide %6.2f, torch / wide %6.2f%s"
                         % (batch, count, per["wide"], batch / per["wide"] * 1e6, per["narrow"], batch / per["narrow"] * 1e6, per["torch"],
                            batch / per["torch"] * 1e6, per["narrow"] / per["wide"], per["torch"] / per["wide"],
                            "" if r["finite"] else "  [non-finite values in a block]"))
            if batch == FLOOR_BATCH:
                ratio = per["narrow"] / per["wide"]
                floor_ratio = ratio if floor_ratio is None else min(floor_ratio, ratio)
            print(lines[-1], "(%.0f s)" % (time.time() - t0), flush=True)
        if stopped:
            break
    if stopped:
        lines.append("STOPPED: " + stopped)
    if floor_ratio is not None:
        lines.append("floor at batch %d: step_wide is %.2f x faster per step than pve_learner_step (the smaller of the two lines; floor %.0f x): %s"
                     % (FLOOR_BATCH, floor_ratio, FLOOR, "MET" if floor_ratio >= FLOOR else "MISSED"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Time of a fresh episode's arrival stream at the headline shape (4096 envs x 432 rows, the 600 s episode at 1100 veh/h/lane):
(a) the host path, arrivals.synthetic_arrivals + set_arrivals (12 lanes; 8 lanes with synthetic_intentions + set_intentions),
(b) BatchedIntersections.generate_arrivals (pve_generate_arrivals), (c) a device-to-device copy_ of tensors of the same size, the
memory floor: the generator writes what the copy writes and reads nothing.  One process, alternating, one synchronisation around
each call, medians.  States whether (b) is at least 20 x faster than (a).

    python tools/bench_arrivals.py [--reps 15] [--host-reps 3] [--envs 4096] [--variants build/libpveenv_arr_g*.so]
                                   [--cutouts build/libpveenv_arr_cut*.so]
                                   [--out profiles/arrivals_bench.txt]

--variants: other builds of the library (-DPVE_ARR_GROUP / -DPVE_ARR_TILE, csrc/pve_arrivals.h) timed on path (b) in the same
alternation; each is checked bit for bit against the product library's stream first.  --cutouts: builds with a part of the kernel
taken out (profiles/experiments/arrivals_cutouts.patch), timed the same way; their streams are not the product's."""
import argparse
import ctypes as C
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import pve_mcc_amd  # noqa: E402
from pve_mcc_amd import _capi  # noqa: E402
from pve_mcc_amd.arrivals import default_rows, device_arrivals, synthetic_arrivals, synthetic_intentions  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rate", type=float, default=1100.0)
    ap.add_argument("--horizon", type=float, default=600.0)
    ap.add_argument("--variants", nargs="*", default=[])
    ap.add_argument("--cutouts", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    E, rows = a.envs, default_rows(a.rate, a.horizon)
    lines = ["arrival streams, %d envs x %d rows at %.0f veh/h/lane (%s, torch %s), medians of %d (host path: %d), us"
             % (E, rows, a.rate, torch.cuda.get_device_name(0), torch.__version__, a.reps, a.host_reps)]
    variants = [p for pat in a.variants for p in sorted(glob.glob(pat))]
    cutouts = [p for pat in a.cutouts for p in sorted(glob.glob(pat))]
    ok = True
    for ln in (12, 8):
        b = pve_mcc_amd.BatchedIntersections(E, 128, None, device="cuda", lane_num=ln, outputs=("obs_post",))
        others = [(os.path.basename(p), pve_mcc_amd.BatchedIntersections(E, 128, None, device="cuda", lane_num=ln, outputs=("obs_post",),
                                                                           _lib=_capi._declare(C.CDLL(os.path.abspath(p))))) for p in variants + cutouts]
        b.generate_arrivals(a.rate, rows=rows, seed=1)
        for name, o in others:                                        # a variant is another launch shape, never another stream
            o.generate_arrivals(a.rate, rows=rows, seed=1)
            if name.startswith("libpveenv_arr_cut"):
                continue
            assert torch.equal(o.arrivals.view(torch.int64), b.arrivals.view(torch.int64)), name
            assert ln != 8 or torch.equal(o.intentions, b.intentions), name
        few = device_arrivals(8, rows, ln, a.rate, seed=1)
        assert np.array_equal(b.arrivals[:8].cpu().numpy().view(np.uint64), few.view(np.uint64)), "the kernel differs from the model"
        src_a, dst_a = torch.empty_like(b.arrivals).normal_(), torch.empty_like(b.arrivals)
        src_c = dst_c = None
        if ln == 8:
            src_c, dst_c = torch.ones_like(b.intentions), torch.empty_like(b.intentions)
        hb = pve_mcc_amd.BatchedIntersections(E, 128, None, device="cuda", lane_num=ln, outputs=("obs_post",))

        def host_path(seed):
            t0 = time.perf_counter()
            arr = synthetic_arrivals(E, a.rate, a.horizon, seed=seed, lane_num=ln)
            ch = synthetic_intentions(E, arr.shape[1], seed=seed) if ln == 8 else None
            t1 = time.perf_counter()
            hb.set_arrivals(arr)
            if ch is not None:
                hb.set_intentions(ch)
            return (t1 - t0) * 1e6

        def copy_path():
            dst_a.copy_(src_a)
            if dst_c is not None:
                dst_c.copy_(src_c)

        t_host, t_gen_only, t_dev, t_copy, t_var = [], [], [], [], {n: [] for n, _ in others}
        for rep in range(a.reps):
            if rep < a.host_reps:
                t, g = timed(lambda: host_path(100 + rep))
                t_host.append(t); t_gen_only.append(g)
            t_dev.append(timed(lambda: b.generate_arrivals(a.rate, rows=rows, seed=1, epoch=rep))[0])
            for name, o in others:
                t_var[name].append(timed(lambda: o.generate_arrivals(a.rate, rows=rows, seed=1, epoch=rep))[0])
            t_copy.append(timed(copy_path)[0])
        mb = b.arrivals.numel() * 8 / 1e6 + (b.intentions.numel() * 4 / 1e6 if ln == 8 else 0.0)
        what = "%d lanes%s, %.1f MB" % (ln, " + intentions" if ln == 8 else "", mb)
        factor = med(t_host) / med(t_dev)
        ok = ok and factor >= 20.0
        lines.append("%s: (a) synthetic_arrivals + set_arrivals %.0f (generation alone %.0f)   (b) generate_arrivals %.1f (min %.1f, %.0f GB/s)"
                     "   (c) copy_ %.1f (%.0f GB/s written)   (a) / (b) = %.0f x   (b) / (c) = %.2f"
                     % (what, med(t_host), med(t_gen_only), med(t_dev), min(t_dev), mb / med(t_dev) * 1e3, med(t_copy), mb / med(t_copy) * 1e3,
                        factor, med(t_dev) / med(t_copy)))
        for name, _ in others:
            lines.append("    %s %-32s (b) %.1f (min %.1f)" % ("cut-out" if name.startswith("libpveenv_arr_cut") else "variant", name,
                                                             med(t_var[name]), min(t_var[name])))
    lines.append("requirement (b) at least 20 x faster than (a), both shapes: %s" % ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

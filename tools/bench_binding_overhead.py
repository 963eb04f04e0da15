"""Host cost per call of the Python binding, without a GPU: this tree against a checkout of another commit (the parent), on the
CPU emulator of the kernels (tests/emu), a 1-environment, 64-slot batch.

Three calls, N = 200 000 of each per repeat:
  set_exploration(0.0, 1)   a handle call with no kernel and no allocation: goes through BatchedIntersections._call, so the
                            difference between the trees is the gateway's own cost per call (sigma = 0: the emulator has no
                            noisy actor kernels and refuses any other; the Python path does not depend on the value);
  prepare_step_many(1)()    the prepared call bench.py times: must execute no gateway code (the worker replaces the batch's
                            gateway by a function that raises while it runs);
  step()                    one per-tick stepping method, which calls its pre-bound entry point directly.
Five repeats, every repeat one fresh process per tree, the trees in alternation; medians, the parent's own repeat-to-repeat
spread (max - min) and the difference of the medians next to it -- and the minima with their difference, which a busy host
disturbs least.

    python tools/bench_binding_overhead.py --parent <checkout of the parent commit> [--out profiles/binding_gateway.txt]

(the checkout builds its own emulator on first use: `make` in its tests/emu)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CALLS = ("set_exploration", "prepared step_many(1)", "step()")


def worker(root, n):
    sys.path.insert(0, root)
    import pve_mcc_amd
    from pve_mcc_amd.arrivals import synthetic_arrivals
    from tests.hip_adapter import emulator_lib
    assert os.path.dirname(os.path.abspath(pve_mcc_amd.__file__)) == root
    arr = synthetic_arrivals(1, rate=200.0, horizon_s=20.0, seed=1)
    b = pve_mcc_amd.BatchedIntersections(1, 64, arr, device="cpu", outputs=("obs_post", "reward", "flags", "env_out"), _lib=emulator_lib())
    b.reset()
    prepared = b.prepare_step_many(1)

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) / n * 1e9

    res = {}
    for _ in range(2000):                     # (warm: the streams' vehicles have passed, every tick costs the same)
        prepared()
    res[CALLS[0]] = timed(lambda: b.set_exploration(0.0, 1))

    def forbidden(*a, **k):
        raise AssertionError("the prepared call went through the gateway")
    has_gateway = hasattr(b, "_call")         # (the parent has none)
    if has_gateway:
        b._call = forbidden                   # (an instance attribute in front of the method, for the prepared call only)
    res[CALLS[1]] = timed(prepared)
    if has_gateway:
        del b._call
    res[CALLS[2]] = timed(b.step)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the commit to compare with")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.worker), a.calls)
    trees = (("parent", os.path.abspath(a.parent)), ("tree", ROOT))
    runs = {name: [] for name, _ in trees}
    for _ in range(a.repeats):
        for name, root in trees:
            out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--worker", root, "--calls", str(a.calls)], cwd=root)
            runs[name].append(json.loads(out.decode().strip().splitlines()[-1]))
    lines = ["# ns per call on the CPU emulator, 1 env x 64 slots, %d calls per repeat, %d repeats (one process per tree and repeat,"
             % (a.calls, a.repeats), "# parent and this tree in alternation)",
             "# %-22s %-8s %s    median      min" % ("call", "tree", " ".join("%8s" % ("rep%d" % (k + 1)) for k in range(a.repeats)))]
    for c in CALLS:
        med, low = {}, {}
        for name, _ in trees:
            v = [r[c] for r in runs[name]]
            med[name], low[name] = statistics.median(v), min(v)
            lines.append("%-24s %-8s %s  %8.1f %8.1f" % (c, name, " ".join("%8.1f" % x for x in v), med[name], low[name]))
        vp = [r[c] for r in runs["parent"]]
        lines.append("%-24s this tree - parent: %+.1f ns per call by the medians, %+.1f ns by the minima; the parent's own "
                     "repeat-to-repeat spread: %.1f ns" % (c, med["tree"] - med["parent"], low["tree"] - low["parent"], max(vp) - min(vp)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()

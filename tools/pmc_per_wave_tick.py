#!/usr/bin/env python3
"""Two counter files of tools/pmc_sq.sh (parent, new) side by side, per wave and tick of the run's LAST k_rollout launch
(the timed --steps ticks of the persistent launch).  SQ_*_CYCLES / SQ_WAIT_* / SQ_ACTIVE_INST_* count in units of four cycles.
Usage: python tools/pmc_per_wave_tick.py <parent.txt> <new.txt> [envs=4096] [waves per env=2] [ticks=100]"""
import re
import sys


def read(path):
    out, on = {}, False
    for line in open(path):
        if not line.startswith(" "):
            on = "k_rollout<128, 5" in line
            continue
        m = re.match(r"\s+(\S+)\s+mean/launch\s+\S+\s+last\s+(\S+)", line)
        if m and on:
            out[m.group(1)] = float(m.group(2))
    return out


if __name__ == "__main__":
    a, b = read(sys.argv[1]), read(sys.argv[2])
    envs, waves, ticks = (int(x) for x in (sys.argv[3:6] + ["4096", "2", "100"][len(sys.argv[3:6]):]))
    n = float(envs * waves * ticks)
    print("per wave and tick (%d envs x %d waves x %d ticks)" % (envs, waves, ticks))
    print("%-26s %12s %12s %8s" % ("counter", "parent", "new", "new/par"))
    for c in sorted(set(a) | set(b)):
        x, y = a.get(c), b.get(c)
        print("%-26s %12s %12s %8s" % (c, "-" if x is None else "%.1f" % (x / n), "-" if y is None else "%.1f" % (y / n),
                                        "-" if not x or y is None else "%.3f" % (y / x)))

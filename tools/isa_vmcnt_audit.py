"""Where a kernel's tick loop waits on the vector-memory counter, read from the assembly text.

usage: python tools/isa_vmcnt_audit.py pve.s '_Z9k_rolloutILi128ELi5ELb0ELb0ELb0ELb1ELb1EE' [--loop .LBB12_7]

gfx950 has ONE `vmcnt` for loads and stores, counted in issue order: an `s_waitcnt vmcnt(N)` that the compiler places for a
load also waits for every store issued before that load's successors -- the L2's acknowledgement of a scattered store, which no
result needs.  This tool lists every `s_waitcnt` with a vmcnt field inside the tick loop of the kernel whose mangled name starts
with the given key, with what the text around it says:

  pos       instruction number within the loop (text order = the compiler's layout of the source order)
  line      line of the assembly file
  block     the basic block (.LBBn_m) the wait sits in
  vmcnt     the count waited for
  loads     vector-memory loads issued since the previous listed wait      } text order, the loop walked as a ring: the first
  stores    vector-memory stores issued since the previous listed wait     } wait of the loop sees the tail of the previous tick
  barrier   number of s_barrier passed since the loop's top (which phase the wait belongs to)
  window    `yes` = the wait lies between the loop's first output store and the first load behind the loop's top, i.e. between
            FIN's first store and the FX gather of the following tick: it drains output stores

It reads the text only and knows nothing but loads, stores, barriers, branches (to find the loop) and vmcnt.  Text order is not
control flow: a block the compiler laid out of line (rare paths) is listed where it stands, with its label to tell.
The tick loop = the smallest backward-branch span that holds more than half of the kernel's barriers (the persistent kernels wrap
it in the item loop, and the pool passes loop inside it) -- of its stores where a one-wave kernel has no barrier instruction;
--loop names the header label instead.
"""
import re
import sys

LOAD = re.compile(r"^(global|flat|buffer|scratch)_(load|atomic)")
STORE = re.compile(r"^(global|flat|buffer|scratch)_store")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^s_c?branch\S*\s+(\.LBB\d+_\d+)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


def kernel_body(lines, key):
    """-> (first line index behind the kernel's label, index of its .Lfunc_end)"""
    starts = [i for i, l in enumerate(lines) if l.startswith(key) and l.split()[0].endswith(":")]
    if len(starts) != 1:
        raise SystemExit("%d kernels start with %r: %s" % (len(starts), key, ", ".join(lines[i].split(":")[0] for i in starts[:8])))
    end = next((i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end")), len(lines))
    return starts[0] + 1, end


def instructions(lines, lo, hi):
    """-> [(line number, block label, opcode, text)] of the instructions in lines[lo:hi], labels = {label: instruction index}"""
    ins, labels, block = [], {}, "entry"
    for n in range(lo, hi):
        s = lines[n].split(";")[0].strip()
        m = LABEL.match(s)
        if m:
            block = m.group(1)
            labels[block] = len(ins)
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        ins.append((n + 1, block, s.split()[0], s))
    return ins, labels


def find_loop(ins, labels, header=None):
    """-> (first, last) instruction index of the tick loop"""
    spans = []
    for i, (_, _, _, s) in enumerate(ins):
        m = BRANCH.match(s)
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            spans.append((labels[m.group(1)], i, m.group(1)))
    if header is not None:
        own = [sp for sp in spans if sp[2] == header]
        if not own:
            raise SystemExit("no backward branch to %s" % header)
        return own[0][0], max(sp[1] for sp in own)
    bars = [i for i, x in enumerate(ins) if x[2] == "s_barrier"]
    if not bars:                               # (one wave per workgroup: the barriers compile to nothing)
        bars = [i for i, x in enumerate(ins) if STORE.match(x[2])]
    best = None
    for a, b, _ in spans:
        inside = sum(1 for i in bars if a <= i <= b)
        if 2 * inside > len(bars) and (best is None or b - a < best[1] - best[0]):
            best = (a, b)
    if best is None:
        raise SystemExit("no loop holds more than half of the kernel's %d barriers / stores" % len(bars))
    return best


def audit(lines, key, header=None):
    """-> dict(kernel, loop_block, n_ins, first_store, first_load, waits=[dict(pos, line, block, vmcnt, loads, stores, barrier, window)])"""
    lo, hi = kernel_body(lines, key)
    ins, labels = instructions(lines, lo, hi)
    a, b = find_loop(ins, labels, header)
    loop = ins[a:b + 1]
    first_store = next((i for i, x in enumerate(loop) if STORE.match(x[2])), None)
    first_load = next((i for i, x in enumerate(loop) if LOAD.match(x[2])), None)
    waits = []
    loads = stores = 0
    for rnd in range(2):                       # the ring: the second round starts with what the loop's tail left
        bar = 0
        for i, (line, block, op, s) in enumerate(loop):
            if LOAD.match(op):
                loads += 1
            elif STORE.match(op):
                stores += 1
            elif op == "s_barrier":
                bar += 1
            elif op == "s_waitcnt":
                m = VMCNT.search(s)
                if not m:
                    continue
                if rnd == 1:
                    window = first_store is not None and (i > first_store or (first_load is not None and i < first_load))
                    waits.append(dict(pos=i, line=line, block=block, vmcnt=int(m.group(1)), loads=loads, stores=stores,
                                      barrier=bar, window=window))
                loads = stores = 0
    return dict(kernel=lines[lo - 1].split(":")[0], loop_block=loop[0][1], n_ins=len(loop), first_store=first_store,
                first_load=first_load, waits=waits)


def report(res):
    out = ["kernel %s" % res["kernel"],
           "tick loop: header %s, %d instructions; first load at pos %s, first store at pos %s" %
           (res["loop_block"], res["n_ins"], res["first_load"], res["first_store"]),
           "%6s %8s %-12s %5s %5s %6s %7s %6s" % ("pos", "line", "block", "vmcnt", "loads", "stores", "barrier", "window")]
    for w in res["waits"]:
        out.append("%6d %8d %-12s %5d %5d %6d %7d %6s" % (w["pos"], w["line"], w["block"], w["vmcnt"], w["loads"], w["stores"],
                                                       w["barrier"], "yes" if w["window"] else "no"))
    out.append("vmcnt waits in the loop: %d, of them inside the store window: %d" %
               (len(res["waits"]), sum(1 for w in res["waits"] if w["window"])))
    return "\n".join(out)


def main(argv):
    args = [x for x in argv[1:]]
    header = None
    if "--loop" in args:
        k = args.index("--loop")
        header = args[k + 1]
        del args[k:k + 2]
    if len(args) != 2:
        raise SystemExit(__doc__)
    with open(args[0]) as f:
        lines = f.read().split("\n")
    print(report(audit(lines, args[1], header)))


if __name__ == "__main__":
    main(sys.argv)

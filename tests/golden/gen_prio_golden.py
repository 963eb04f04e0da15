"""Generate tests/golden/prio_ref.npz: what the UNMODIFIED reference's prioritised memory (rank_based.py `Experience`,
binary_heap.py) computes, for tests/test_prio_replay.py.

Run in the build container only:   python tests/golden/gen_prio_golden.py [reference directory]

Stored:
  tables, for (size, batch) in CASES, built as replay_buffer.py:13-18 does (partition_num = 32):
    ends_<size>_<batch>  int32 [32][batch + 1]   distributions[p]['strata_ends'][1 .. batch + 1], p = 1 .. 32
    dist_<size>_<batch>  int32 [size]            int(math.floor(1.0 * L / size * 32)) for L = 1 .. size: rank_based.py:159, the
                                                 expression evaluated as Python evaluates it there
  a trace on Experience(size = 320, batch_size = 8, learn_start = 100, steps = 1000), whose experiences are their record
  numbers 0, 1, ..; two stages, A after 200 stores (not yet full) and B after 500 (wrapped):
    <stage>_written, <stage>_upd_seq int64 [L], <stage>_upd_p float32 [L]: every live record updated with a priority of its
        own (pairwise distinct float32 values, handed to update_priority as e_id = slot + 1 and the float64 of the value)
    <stage>_p2e int64 [L]: priority_to_experience(1 .. L) after rebalance(), as RECORD NUMBERS (the experiences retrieved)
    <stage>_steps int64 [S], <stage>_ranks int64 [S][8], <stage>_w float64 [S][8], <stage>_exp int64 [S][8]: sample(global_step)
        under random.seed(RANDOM_SEED): the rank_list (read back through e2p), the weights and the experiences returned
  alpha, beta_zero, learn_start, steps: the trace's configuration."""
import math
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ((320, 8), (333, 8), (1000, 16), (4096, 128))
RANDOM_SEED = 20240607
TRACE = dict(size=320, batch_size=8, learn_start=100, steps=1000, partition_num=32)
STEPS = (101, 150, 300, 550, 999, 1000, 2000)


def main(ref_dir="/root/reference"):
    sys.path.insert(0, ref_dir)
    import rank_based
    out = {}
    for size, batch in CASES:
        exp = rank_based.Experience({"size": size, "batch_size": batch, "partition_num": 32, "learn_start": 0, "steps": 1000})
        out["ends_%d_%d" % (size, batch)] = np.array([[exp.distributions[p]["strata_ends"][s] for s in range(1, batch + 2)]
                                                      for p in range(1, 33)], np.int32)
        out["dist_%d_%d" % (size, batch)] = np.array([int(math.floor(1.0 * L / size * 32)) for L in range(1, size + 1)], np.int32)
    exp = rank_based.Experience(dict(TRACE))
    rng = np.random.default_rng(7)
    random.seed(RANDOM_SEED)
    written = 0
    for stage, n_store in (("A", 200), ("B", 300)):
        for _ in range(n_store):
            assert exp.store(written)
            written += 1
        L = min(written, TRACE["size"])
        live = np.arange(written - L, written, dtype=np.int64)
        p = np.unique(rng.lognormal(0.0, 3.0, 4 * L).astype(np.float32))
        p = rng.permutation(p[p > 0])[:L]
        assert len(np.unique(p)) == L
        exp.update_priority([int(w % TRACE["size"]) + 1 for w in live], [float(x) for x in p])
        exp.rebalance()
        e_ids = exp.priority_queue.priority_to_experience(list(range(1, L + 1)))
        out[stage + "_written"] = np.int64(written)
        out[stage + "_upd_seq"], out[stage + "_upd_p"] = live, p
        out[stage + "_p2e"] = np.array(exp.retrieve(e_ids), np.int64)
        ranks, ws, exps = [], [], []
        for step in STEPS:
            experience, w, rank_e_id = exp.sample(step)
            ranks.append([exp.priority_queue.e2p[e] for e in rank_e_id])
            ws.append(np.asarray(w, np.float64))
            exps.append(experience)
        out[stage + "_steps"] = np.array(STEPS, np.int64)
        out[stage + "_ranks"], out[stage + "_w"], out[stage + "_exp"] = np.array(ranks, np.int64), np.array(ws), np.array(exps, np.int64)
    out.update(alpha=np.float64(exp.alpha), beta_zero=np.float64(exp.beta_zero), learn_start=np.int64(exp.learn_start),
               steps=np.int64(exp.total_steps))
    path = os.path.join(HERE, "prio_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(*sys.argv[1:2])

"""The critic / bootstrap fixture (tests/golden/critic_graph.npz, written by tests/golden/gen_critic_golden.py from the
reference's own graph), loaded once and shared by tests/test_critic.py and tests/test_gpu_critic.py."""
import functools
import json
import os

import numpy as np

from pve_mcc_amd.critic import KEYS
from tests.parity_util import GOLDEN_DIR


class Golden:
    pass


@functools.lru_cache(maxsize=None)
def load_critic_golden():
    z = np.load(os.path.join(GOLDEN_DIR, "critic_graph.npz"))
    g = Golden()
    for k in ("states", "kinds", "given_act7", "boot_act7_f32", "boot_act7_f64", "boot_q_f32", "boot_q_f64", "target_q_f32",
              "target_q_f64", "critic_q_f32", "critic_q_f64"):
        v = z[k]
        v.setflags(write=False)
        setattr(g, k, v)
    g.spread_critic, g.spread_bootstrap, g.sens = float(z["spread_critic"]), float(z["spread_bootstrap"]), float(z["sens"])
    g.meta = json.loads(str(z["meta"]))
    g.weights = {net: {k: z["%s__%s" % (net, k)] for k in KEYS} for net in ("critic", "target_critic", "target_actor")}
    g.n = len(g.states)
    # the rows / actions the online critic was evaluated on: row 0 of every state, twice (two action sets)
    g.given_rows = np.concatenate([g.states[:, 0], g.states[:, 0]])
    g.given_rows.setflags(write=False)
    return g

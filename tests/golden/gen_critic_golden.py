"""Pin the MADDPG critic and the bootstrap term of the n-step target against the reference's OWN shipped graph -- without
TensorFlow.

Run in the build container only:   python tests/golden/gen_critic_golden.py
Output (committed):                tests/golden/critic_graph.npz

The MetaGraphDef next to the shipped checkpoint (model_data/baseline/66.cptk.meta, decoded by gen_actor_golden.py) holds the
critic sub-graphs of model_agent_maddpg.py:52-74 (`agent1_critic/dense_2/BiasAdd`, `agent1_target_critic/dense_2/BiasAdd`) and
the target actor (`agent1_targetactor/Mul`); the checkpoint holds their variables.  This script walks each sub-graph back to
its placeholders along the graph's own edges, asserts from the file the three placeholder shapes ([-1,28], [-1,1], [-1,6]) and
the order of the two concatenations (own action then other actions; hidden units then actions), and evaluates them with the
interpreter of gen_actor_golden.py plus one more primitive, ConcatV2 -- in float32 (the graph's type) and in float64 (the
real-valued semantics of the same graph on the same float32 weights).

States (seven rows of 28 each, `re_state` of traffic_interaction_scene.py:1325-1337):
  * the CPU oracle's `re_state` on the reference's 1000 stream, driven by the decoded acting actor (sampled every 37th
    controlled vehicle-tick, like closed_loop_rows),
  * observation-shaped random states with 0 .. 6 absent (all-zero) neighbour rows,
  * a state whose row 0 is all zero (a freshly spawned vehicle), and the all-zero state.
Recorded for them: the target actor's actions and the target critic's Q in both precisions (the bootstrap of main.py:253-260),
the online critic's Q on given actions, the measured spreads max |f32 - f64|, and sens = max over states of sum_k |dQ/da_k|
of the target critic (float64 central differences on the graph).  Numbers and a JSON description only -- no reference source.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, HERE)
from extract_actor import load_bundle  # noqa: E402
from gen_actor_golden import CKPT, DT_FLOAT, META, GraphActor, decode_attr, load_graph, subgraph  # noqa: E402

OUT = os.path.join(HERE, "critic_graph.npz")
CRITIC_OUT = "agent1_critic/dense_2/BiasAdd"
TARGET_CRITIC_OUT = "agent1_target_critic/dense_2/BiasAdd"
TARGET_ACTOR_OUT = "agent1_targetactor/Mul"
PRIMITIVES = GraphActor.PRIMITIVES + ("ConcatV2",)
KEYS = {"ln0_gamma": "LayerNorm/gamma", "ln0_beta": "LayerNorm/beta", "w1": "dense/kernel", "b1": "dense/bias",
        "ln1_gamma": "LayerNorm_1/gamma", "ln1_beta": "LayerNorm_1/beta", "w2": "dense_1/kernel", "b2": "dense_1/bias",
        "ln2_gamma": "LayerNorm_2/gamma", "ln2_beta": "LayerNorm_2/beta", "w3": "dense_2/kernel", "b3": "dense_2/bias"}


class SubGraph:
    """The sub-graph that ends in `output`, evaluated op by op (gen_actor_golden.GraphActor's interpreter + ConcatV2, any
    number of placeholders)."""

    def __init__(self, nodes, variables, output):
        self.nodes, self.variables, self.output = nodes, variables, output
        self.order = subgraph(nodes, output)
        ops = set(nodes[n]["op"] for n in self.order)
        assert ops <= set(PRIMITIVES), "unexpected ops %s" % (ops - set(PRIMITIVES))
        self.placeholders = {}
        for n in self.order:
            if nodes[n]["op"] == "Placeholder":
                assert decode_attr(nodes[n]["attrs"]["dtype"]) == ("type", DT_FLOAT)
                self.placeholders[n] = decode_attr(nodes[n]["attrs"]["shape"])[1]

    def attr(self, node, key, default=None):
        a = self.nodes[node]["attrs"]
        return decode_attr(a[key]) if key in a else default

    def by_width(self, width):
        hit = [n for n, shp in self.placeholders.items() if shp == [-1, width]]
        assert len(hit) == 1, (width, self.placeholders)
        return hit[0]

    def run(self, feeds, dtype=np.float32):
        F = dtype
        val = {}
        for name in self.order:
            nd = self.nodes[name]
            op = nd["op"]
            x = [val[i.split(":")[0]] for i in nd["inputs"]]
            if op == "Placeholder":
                v = np.asarray(feeds[name], np.float32).astype(F)
            elif op == "Const":
                c = self.attr(name, "value")
                v = c.astype(F) if c.dtype == np.float32 else c
            elif op == "VariableV2":
                v = self.variables[name].astype(F)
            elif op in ("Identity", "StopGradient"):
                v = x[0]
            elif op == "Mean":
                axes = tuple(int(a) for a in np.atleast_1d(x[1]))
                v = np.mean(x[0], axis=axes, keepdims=bool(self.attr(name, "keep_dims", False)), dtype=F)
            elif op == "SquaredDifference":
                d = (x[0] - x[1]).astype(F)
                v = (d * d).astype(F)
            elif op == "Add":
                v = (x[0] + x[1]).astype(F)
            elif op == "Sub":
                v = (x[0] - x[1]).astype(F)
            elif op == "Mul":
                v = (x[0] * x[1]).astype(F)
            elif op == "Rsqrt":
                v = (F(1.0) / np.sqrt(x[0], dtype=F)).astype(F)
            elif op == "MatMul":
                a = x[0].T if self.attr(name, "transpose_a", False) else x[0]
                b = x[1].T if self.attr(name, "transpose_b", False) else x[1]
                v = (a @ b).astype(F)
            elif op == "BiasAdd":
                assert self.attr(name, "data_format", "NHWC") == "NHWC"
                v = (x[0] + x[1]).astype(F)
            elif op == "Relu":
                v = np.maximum(x[0], F(0))
            elif op == "Tanh":
                v = np.tanh(x[0], dtype=F)
            elif op == "ConcatV2":
                axis = int(np.asarray(x[-1]).reshape(()))
                v = np.concatenate(x[:-1], axis=axis)
            else:
                raise AssertionError(op)
            val[name] = v
        out = val[self.output]
        assert out.ndim == 2 and out.shape[1] == 1
        return out[:, 0]

    def concat_description(self):
        """Every ConcatV2 of the sub-graph: its data inputs in order, and its axis"""
        out = {}
        for n in self.order:
            if self.nodes[n]["op"] == "ConcatV2":
                ins = [i.split(":")[0] for i in self.nodes[n]["inputs"]]
                out[n] = dict(inputs=ins[:-1], axis=int(np.asarray(self.attr(ins[-1], "value")).reshape(())))
        return out

    def description(self):
        return dict(output=self.output, placeholders=self.placeholders,
                    ops=sorted(set(self.nodes[n]["op"] for n in self.order)),
                    chain=[[n, self.nodes[n]["op"], self.nodes[n]["inputs"]] for n in self.order],
                    concat=self.concat_description(),
                    epsilon={n: float(self.attr(n, "value")) for n in self.order if n.endswith("batchnorm/add/y")},
                    variables={n: list(self.variables[n].shape) for n in self.order if self.nodes[n]["op"] == "VariableV2"})


class GraphCritic:
    """A critic sub-graph with its three placeholders named by what the file says about them."""

    def __init__(self, nodes, variables, output, scope):
        self.g = SubGraph(nodes, variables, output)
        self.scope = scope
        assert sorted(self.g.placeholders.values()) == [[-1, 1], [-1, 6], [-1, 28]], self.g.placeholders
        self.ph_state, self.ph_action, self.ph_other = self.g.by_width(28), self.g.by_width(1), self.g.by_width(6)
        cc = self.g.concat_description()
        assert len(cc) == 2, cc
        # model_agent_maddpg.py:82: concat([action_input, other_action_input], axis=1) -- outside the critic's scope;
        # :66: concat([x, action_input], axis=-1) inside it: hidden units first, then the 7 actions
        outer = [n for n in cc if not n.startswith(scope + "/")]
        inner = [n for n in cc if n.startswith(scope + "/")]
        assert len(outer) == 1 and len(inner) == 1, cc
        assert cc[outer[0]]["inputs"] == [self.ph_action, self.ph_other] and cc[outer[0]]["axis"] == 1, cc[outer[0]]
        assert cc[inner[0]]["inputs"][1] == outer[0] and cc[inner[0]]["axis"] in (-1, 1), cc[inner[0]]
        assert nodes[cc[inner[0]]["inputs"][0]]["op"] == "Relu", "the first concat input is the hidden layer's ReLU"
        self.concat_outer, self.concat_inner = outer[0], inner[0]

    def run(self, rows, act7, dtype=np.float32):
        act7 = np.asarray(act7, np.float32)
        return self.g.run({self.ph_state: rows, self.ph_action: act7[:, :1], self.ph_other: act7[:, 1:]}, dtype)

    def weights(self):
        return {k: self.g.variables[self.scope + "/" + v] for k, v in KEYS.items()}

    def description(self):
        d = self.g.description()
        d.update(scope=self.scope, state=self.ph_state, action=self.ph_action, other_action=self.ph_other,
                 concat_outer=self.concat_outer, concat_inner=self.concat_inner)
        return d


class GraphTargetActor:
    def __init__(self, nodes, variables):
        self.g = SubGraph(nodes, variables, TARGET_ACTOR_OUT)
        self.scope = "agent1_targetactor"
        assert list(self.g.placeholders.values()) == [[-1, 28]], self.g.placeholders
        self.ph_state = self.g.by_width(28)

    def run(self, rows, dtype=np.float32):
        return self.g.run({self.ph_state: rows}, dtype)

    def weights(self):
        return {k: self.g.variables[self.scope + "/" + v] for k, v in KEYS.items()}


def bootstrap(tactor, tcritic, states, dtype):
    """main.py:253-260 on the graph: all seven rows through the target actor, the target critic on row 0"""
    n = len(states)
    a7 = tactor.run(states.reshape(n * 7, 28), dtype).reshape(n, 7)
    # the reference feeds the actions back through float32 placeholders
    a7_fed = a7.astype(np.float32)
    return a7, tcritic.run(states[:, 0], a7_fed, dtype)


# ------------------------------------------------------------------------------------------------ states
def closed_loop_states(actor, ticks=1000, every=37):
    """`re_state` of the controlled vehicles on the reference's 1000 stream, the decoded acting actor as the policy
    (gen_actor_golden.closed_loop_rows with tick(..., want_state=True))"""
    from oracle.oracle import OracleEnv
    from pve_mcc_amd.arrivals import load_arrival_mat
    arr = load_arrival_mat(os.path.join(HERE, "streams", "arvTimeNewVeh_new_1000_12.mat"))
    env = OracleEnv(arr)
    states, k = [], 0
    for _ in range(ticks):
        vid, c, obs0 = env.alive_view()
        a = np.zeros(len(vid))
        if c.any():
            a[c != 0] = actor.run(obs0[c != 0]).astype(np.float64)
        rec = env.tick(a, want_state=True)
        for st in rec["state"]:
            if k % every == 0:
                states.append(st)
            k += 1
    return np.asarray(states, np.float64).reshape(-1, 7, 28)


def make_states(actor):
    rng = np.random.default_rng(6841)
    cl = closed_loop_states(actor).astype(np.float32)
    parts, kinds = [cl], ["closed_loop"] * len(cl)
    n = 280
    shaped = np.zeros((n, 7, 7, 4), np.float32)                  # [state][row][vehicle of the row][p, v, a, route]
    shaped[..., 0] = rng.uniform(-5, 165, (n, 7, 7))
    shaped[..., 1] = rng.uniform(5, 13, (n, 7, 7))
    shaped[..., 2] = rng.uniform(-3, 3, (n, 7, 7))
    shaped[..., 3] = rng.integers(0, 12, (n, 7, 7))
    shaped = shaped.reshape(n, 7, 28)
    for i in range(n):
        shaped[i, 1 + (i % 7):] = 0                              # 0 .. 6 neighbours present, the absent rows all zero
    parts.append(shaped)
    kinds += ["shaped"] * n
    deg = np.zeros((2, 7, 28), np.float32)
    deg[0, 1:] = shaped[6, 1:]                                   # row 0 all zero (freshly spawned vehicle), six neighbours
    parts.append(deg)                                            # deg[1]: the all-zero state
    kinds += ["degenerate"] * 2
    return np.concatenate(parts).astype(np.float32), np.asarray(kinds)


def sensitivity(tcritic, rows, a7, h=1e-3):
    """sum_k |dQ/da_k| per state, float64 central differences on the graph (the placeholders are float32: the displaced
    actions are rounded to float32 first and the difference quotient uses the displacement that was actually fed)"""
    total = np.zeros(len(rows))
    a7 = np.asarray(a7, np.float32)
    for k in range(7):
        up, dn = a7.copy(), a7.copy()
        up[:, k] += np.float32(h)
        dn[:, k] -= np.float32(h)
        dq = tcritic.run(rows, up, np.float64) - tcritic.run(rows, dn, np.float64)
        total += np.abs(dq / (up[:, k].astype(np.float64) - dn[:, k].astype(np.float64)))
    return total


def main():
    nodes = load_graph(META)
    variables = load_bundle(CKPT)
    actor = GraphActor()
    critic = GraphCritic(nodes, variables, CRITIC_OUT, "agent1_critic")
    tcritic = GraphCritic(nodes, variables, TARGET_CRITIC_OUT, "agent1_target_critic")
    tactor = GraphTargetActor(nodes, variables)
    for c in (critic, tcritic):
        print(c.scope, "placeholders", c.g.placeholders, "concat", c.g.concat_description())
        w = c.weights()
        assert w["w1"].shape == (28, 64) and w["w2"].shape == (71, 64) and w["w3"].shape == (64, 1)
        assert sorted(c.g.description()["variables"]) == sorted(c.scope + "/" + v for v in KEYS.values())
    states, kinds = make_states(actor)
    n = len(states)
    print("%d states:" % n, {k: int((kinds == k).sum()) for k in sorted(set(kinds))})
    a32, q32 = bootstrap(tactor, tcritic, states, np.float32)
    a64, q64 = bootstrap(tactor, tcritic, states, np.float64)
    # the target critic ALONE on the float64 graph's actions (what a device that commits no action error would see), and the
    # online critic on given actions: the stored target-actor actions, and the `re_state` column the reference stores as
    # the 7-action vector (ref :290)
    given = np.concatenate([a64.astype(np.float32), np.ascontiguousarray(states[:, :, 2])])
    grows = np.concatenate([states[:, 0], states[:, 0]])
    c32, c64 = critic.run(grows, given, np.float32), critic.run(grows, given, np.float64)
    t32, t64 = tcritic.run(states[:, 0], a64.astype(np.float32), np.float32), tcritic.run(states[:, 0], a64.astype(np.float32), np.float64)
    spread_critic = float(max(np.abs(c32 - c64).max(), np.abs(t32 - t64).max()))
    spread_bootstrap = float(np.abs(q32 - q64).max())
    sens_all = sensitivity(tcritic, states[:, 0], a64)
    sens = float(sens_all.max())
    print("Q range [%.2f, %.2f]; spread_critic %.3e (online %.3e, target %.3e); spread_bootstrap %.3e; actions |f32 - f64| %.3e; sens %.3f"
          % (q64.min(), q64.max(), spread_critic, np.abs(c32 - c64).max(), np.abs(t32 - t64).max(), spread_bootstrap,
             np.abs(a32 - a64).max(), sens))
    desc = dict(critic=critic.description(), target_critic=tcritic.description(), target_actor=tactor.g.description(),
                spread_critic=spread_critic, spread_bootstrap=spread_bootstrap, sens=sens, sens_step=1e-3, numpy=np.__version__,
                key_names=KEYS)
    out = dict(states=states, kinds=kinds, given_act7=given.astype(np.float32),
               boot_act7_f32=a32.astype(np.float32), boot_act7_f64=a64.astype(np.float64),
               boot_q_f32=q32.astype(np.float32), boot_q_f64=q64.astype(np.float64),
               target_q_f32=t32.astype(np.float32), target_q_f64=t64.astype(np.float64),
               critic_q_f32=c32.astype(np.float32), critic_q_f64=c64.astype(np.float64),
               spread_critic=np.float64(spread_critic), spread_bootstrap=np.float64(spread_bootstrap), sens=np.float64(sens),
               meta=np.array(json.dumps(desc)))
    for net, g in (("critic", critic), ("target_critic", tcritic), ("target_actor", tactor)):
        for k, v in g.weights().items():
            out["%s__%s" % (net, k)] = v.astype(np.float32)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

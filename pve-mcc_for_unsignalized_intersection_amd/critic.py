"""NumPy restatement of the MADDPG critic and of the bootstrap term of the n-step target, as the device computes them
(`BatchedIntersections.critic_q` / `bootstrap_q`, csrc/pve_critic.h).

    critic (model_agent_maddpg.py:52-74):
        x(28) -> LayerNorm -> Dense 28x64 -> LayerNorm -> ReLU -> concat [h(64), own action, 6 other actions]
              -> Dense 71x64 -> LayerNorm -> ReLU -> Dense 64x1
    bootstrap (main.py:253-260): a_k = target_actor(state[k]) for all seven rows k, q = target_critic(state[0], a_0, a_1 .. a_6);
        rows without PVE_F_CTL or with PVE_F_DONE get q = 0 and zero actions (main.py:250-251).

Weights are dicts with the TF variables LayerNorm{,_1,_2}/{gamma,beta} as ln{0,1,2}_{gamma,beta} and dense{,_1,_2}/{kernel,bias}
as w{1,2,3} / b{1,2,3} (kernels in TF layout [in][out]; the critic's w2 is [71][64]).  `dtype` selects the arithmetic:
float32 is the graph's own type, float64 the real-valued semantics of the same graph on the same float32 weights."""
import numpy as np

KEYS = ("ln0_gamma", "ln0_beta", "w1", "b1", "ln1_gamma", "ln1_beta", "w2", "b2", "ln2_gamma", "ln2_beta", "w3", "b3")
N_CRITIC_WEIGHTS = 6841
F_CTL, F_DONE = 0x02, 0x04


def _layer_norm(x, gamma, beta, F):
    mean = x.mean(axis=-1, keepdims=True, dtype=F)
    var = np.mean(np.square(x - mean, dtype=F), axis=-1, keepdims=True, dtype=F)
    inv = (F(1.0) / np.sqrt(var + F(np.float32(1e-12)), dtype=F)) * gamma
    return (x * inv + (beta - mean * inv)).astype(F)


def _w(w, F):
    return {k: np.asarray(w[k], np.float32).astype(F) for k in KEYS}


def flat_critic_weights(w):
    """The 6841 float32 weights in the order pve_set_target_networks expects (include/pve_env.h)."""
    flat = np.concatenate([np.asarray(w[k], np.float32).ravel() for k in KEYS])
    if flat.size != N_CRITIC_WEIGHTS:
        raise ValueError("critic needs %d weights, got %d" % (N_CRITIC_WEIGHTS, flat.size))
    return flat


def actor_forward(w, rows, dtype=np.float32):
    """rows [..., 28] -> action [...] in [-3, 3] (model_agent_maddpg.py:23-49)."""
    F = dtype
    w = _w(w, F)
    x = np.asarray(rows).astype(np.float32).astype(F)
    x = _layer_norm(x, w["ln0_gamma"], w["ln0_beta"], F)
    x = np.maximum(_layer_norm((x @ w["w1"] + w["b1"]).astype(F), w["ln1_gamma"], w["ln1_beta"], F), F(0))
    x = np.maximum(_layer_norm((x @ w["w2"] + w["b2"]).astype(F), w["ln2_gamma"], w["ln2_beta"], F), F(0))
    y = (x @ w["w3"] + w["b3"]).astype(F)[..., 0]
    return (np.tanh(y, dtype=F) * F(3.0)).astype(F)


def critic_forward(w, rows, act7, dtype=np.float32):
    """rows [..., 28], act7 [..., 7] (own action, then the six other actions) -> Q [...]"""
    F = dtype
    w = _w(w, F)
    x = np.asarray(rows).astype(np.float32).astype(F)
    a = np.asarray(act7).astype(np.float32).astype(F)
    x = _layer_norm(x, w["ln0_gamma"], w["ln0_beta"], F)
    x = np.maximum(_layer_norm((x @ w["w1"] + w["b1"]).astype(F), w["ln1_gamma"], w["ln1_beta"], F), F(0))
    x = np.concatenate([x, a], axis=-1)
    x = np.maximum(_layer_norm((x @ w["w2"] + w["b2"]).astype(F), w["ln2_gamma"], w["ln2_beta"], F), F(0))
    return (x @ w["w3"] + w["b3"]).astype(F)[..., 0]


def bootstrap_q(actor_w, critic_w, state, flags=None, dtype=np.float32):
    """state [..., 7, 28], flags [...] or None -> (q [...], act7 [..., 7]); rows the flags exclude hold zeros."""
    state = np.asarray(state)
    lead = state.shape[:-2]
    st = state.reshape((-1, 7, 28))
    ev = np.ones(len(st), bool)
    if flags is not None:
        f = np.asarray(flags).reshape(-1).astype(np.int64)
        ev = (f & (F_CTL | F_DONE)) == F_CTL
    q = np.zeros(len(st), dtype)
    act7 = np.zeros((len(st), 7), dtype)
    if ev.any():
        act7[ev] = actor_forward(actor_w, st[ev], dtype)
        q[ev] = critic_forward(critic_w, st[ev, 0], act7[ev], dtype)
    return q.reshape(lead), act7.reshape(lead + (7,))

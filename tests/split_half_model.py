"""The split-half actor and critic (csrc/pve_actor.h `k_actor_pack` / `actor_tile32`, csrc/pve_critic.h `k_critic_pack` /
`critic_tile32`) restated in NumPy, step by step: the CPU statement of what the f16 half-pair kernels compute.  The emulator runs
`actor_canonical`, the float32 chain; this file is the arithmetic the device really uses, and the reference the device tests of
tests/test_gpu_split_half.py compare against next to float64 pve_mcc_amd.critic.

What is modelled exactly:
  * pack time: the means over the output units in float64, rounded to float32; kernels and biases centred in float32; the
    power-of-two scale rule (`pack_exponent`) on the centred kernel and bias, and the LayerNorm epsilon 1e-12f * 4^e that goes with
    it; the split hi = float16(x), lo = float16(x - float32(hi)) (round to nearest even, f16 subnormals kept, overflow to inf);
  * LayerNorm over the inputs in float32 in the tile's own summation order (sixteen values per lane summed by halves, then the two
    lanes of a vehicle): mean, d = x - mean, fma(d, gamma * rstd, beta);
  * every product block of 16 as three matrix instructions Ah.Bh + Ah.Bl + Al.Bh on float32 accumulators that start at the
    centred bias; K = 28 padded to 32 (two blocks), K = 64 (four blocks), the critic's fifth block with the 7 action rows;
  * the centred LayerNorm without a mean pass, in the tile's summation order; ReLU; the head's dot product in that order.
The stated approximations:
  * inside one matrix instruction the 16 products and the accumulator are added in float64 and rounded to float32 ONCE (the
    matrix core's internal order is not specified);
  * v_rsq_f32 is float32(1 / sqrt(.)) and 3 tanh is float32(3 tanh(z)) of the float32 z: the instructions' own error (1 ulp; the
    head: ACTOR_TANH3_BAR of tests/math_probe_scenarios.py) is not in the model.

`scaled=False` evaluates the packing WITHOUT the scale rule (e = 0, epsilon 1e-12f): what the kernels did before the rule, kept so
that tests/test_split_half_model.py can show that its bars see the loss the rule removes."""
import numpy as np

from pve_mcc_amd.critic import KEYS

F32, F64, F16 = np.float32, np.float64, np.float16
EPS = F32(1e-12)
E_CLAMP = 40


# ---------------------------------------------------------------------------------- the split
def split(x):
    """float32 -> (hi, lo) float16: hi = half(x), lo = half(x - hi), the subtraction exact in float32 (actor_split8)"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(F16)
        lo = (x - hi.astype(F32)).astype(F16)
    return hi, lo


# ---------------------------------------------------------------------------------- pack time
def pack_exponent(m):
    """The scale rule of k_actor_pack / k_critic_pack: m = max |centred kernel| (float32) -> e; kernel and bias are multiplied by
    2^e.  e = 0 while 2^-3 <= m <= 2^12 (and for m = 0); otherwise e = -floor(log2 m), clamped to +-40, which brings m into [1, 2).
    Below 2^-3 the low halves of the small entries sink into f16's subnormal range (step 2^-24) and the pair keeps fewer than 22
    bits; above 2^12 the high halves approach f16's largest number, 65 504."""
    m = float(F32(m))
    if m == 0.0 or not np.isfinite(m) or 2.0 ** -3 <= m <= 2.0 ** 12:
        return 0
    e = -(int(np.frexp(m)[1]) - 1)                                    # frexp: m = f 2^x, f in [0.5, 1): floor(log2 m) = x - 1
    return max(-E_CLAMP, min(E_CLAMP, e))


def _centre(kernel, bias):
    k = np.asarray(kernel, F32)
    cm = (k.astype(F64).sum(axis=1) / k.shape[1]).astype(F32)         # mean over the OUTPUT units, per input row
    b = np.asarray(bias, F32)
    bm = F32(b.astype(F64).sum() / b.size)
    return (k - cm[:, None]).astype(F32), (b - bm).astype(F32)


class Packed:
    """What k_*_pack leaves in the packed buffer, in natural (unit / feature) order"""

    def __init__(self, w, scaled=True):
        w = {k: np.asarray(w[k], F32) for k in KEYS}
        self.w = w
        self.e, self.eps, self.kh, self.kl, self.bias = [], [], [], [], []
        for kk, bk in (("w1", "b1"), ("w2", "b2")):
            kc, bc = _centre(w[kk], w[bk])
            e = pack_exponent(np.abs(kc).max()) if scaled else 0
            s = F32(2.0) ** F32(e)
            kc, bc = (kc * s).astype(F32), (bc * s).astype(F32)       # exact: a power of two
            hi, lo = split(kc)
            self.e.append(e)
            self.eps.append(F32(EPS * F32(4.0) ** F32(e)))
            self.kh.append(hi.astype(F64))
            self.kl.append(lo.astype(F64))
            self.bias.append(bc)


# ---------------------------------------------------------------------------------- the tile's summation orders
def _hsum16(e):
    """[..., 16] float32 -> [...]: (e[0..7] + e[8..15]) -> 8 -> 4 -> 2 -> 1 (actor_hsum16)"""
    a = e[..., :8] + e[..., 8:]
    b = a[..., :4] + a[..., 4:]
    c = b[..., :2] + b[..., 2:]
    return c[..., 0] + c[..., 1]


def _lanes_in(x):
    """[N, 28] features -> [N, hf 2, c 16]: lane hf holds feature 16 (c >> 3) + 8 hf + (c & 7); 28..31 are zeros"""
    p = np.zeros(x.shape[:-1] + (32,), F32)
    p[..., :28] = x
    return p.reshape(x.shape[:-1] + (2, 2, 8)).swapaxes(-3, -2).reshape(x.shape[:-1] + (2, 16))


def _lanes_in_back(v):
    """inverse of _lanes_in on [N, 2, 16] -> [N, 32]"""
    return v.reshape(v.shape[:-2] + (2, 2, 8)).swapaxes(-3, -2).reshape(v.shape[:-2] + (32,))


def _units_to_lanes(h):
    """[N, 64] units -> [N, hf 2, m 2, r 16]: unit 32 m + 8 (r >> 2) + 4 hf + (r & 3)"""
    n = h.shape[:-1]
    return h.reshape(n + (2, 4, 2, 4)).transpose(tuple(range(len(n))) + (len(n) + 2, len(n), len(n) + 1, len(n) + 3)).reshape(n + (2, 2, 16))


def _rsq(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / np.sqrt(v.astype(F64))).astype(F32)


def _fma(a, b, c):
    """float32 fma: the product of two float32 values is exact in float64"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _ln_inputs(x, gamma, beta):
    """LayerNorm over the 28 inputs as the tile does it -> float32 [N, 32] (features 28..31: zeros)"""
    d = _lanes_in(np.asarray(x, F32))
    s = _hsum16(d)
    mean = (s[..., 0] + s[..., 1]) * F32(1.0 / 28.0)
    d = (d - mean[..., None, None]).astype(F32)
    d[..., 1, 12:] = 0
    v = _hsum16(d * d)
    rstd = _rsq((v[..., 0] + v[..., 1]) * F32(1.0 / 28.0) + EPS)
    ga, be = np.asarray(gamma, F32), np.asarray(beta, F32)
    y =_fma(d, _lanes_in(ga) * rstd[..., None, None], np.broadcast_to(_lanes_in(be), d.shape))
    return _lanes_in_back(y)


def _ln_relu_centred(h, gamma, beta, eps):
    """actor_ln_relu32: the input is centred already (no mean pass); float32 [N, 64] -> float32 [N, 64]"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = _units_to_lanes(h)                                        # [N, hf, m, r]
        e = _fma(v[..., 1, :], v[..., 1, :], (v[..., 0, :] * v[..., 0, :]).astype(F32))
        s = _hsum16(e)
        rstd = _rsq((s[..., 0] + s[..., 1]) * F32(1.0 / 64.0) + eps)
        y = _fma(h, np.asarray(gamma, F32) * rstd[..., None], np.broadcast_to(np.asarray(beta, F32), h.shape))
        return np.where(y > 0, y, F32(0)).astype(F32)                 # fmaxf(y, 0): a NaN becomes 0


def _dense(b, kh, kl, bias):
    """float32 activations [N, K] (K a multiple of 16, padded) x the packed kernel [K, 64] -> float32 [N, 64]: per K-block of 16
    three matrix instructions, each one float64 sum rounded once to float32"""
    bh, bl = split(b)
    bh, bl = bh.astype(F64), bl.astype(F64)
    acc = np.broadcast_to(bias, b.shape[:-1] + (64,)).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, b.shape[-1], 16):
            k = slice(k0, k0 + 16)
            acc = (acc.astype(F64) + bh[..., k] @ kh[k]).astype(F32)
            acc = (acc.astype(F64) + bl[..., k] @ kh[k]).astype(F32)
            acc = (acc.astype(F64) + bh[..., k] @ kl[k]).astype(F32)
    return acc


def _pad_rows(k, rows):
    out = np.zeros((rows, k.shape[1]), F64)
    out[:k.shape[0]] = k
    return out


def _head(g, w3, b3):
    """the final dot product in the tile's order -> float32 z"""
    v, w = _units_to_lanes(g), _units_to_lanes(np.asarray(w3, F32).reshape(64))
    pv = _fma(v[..., 1, :], np.broadcast_to(w[..., 1, :], v[..., 1, :].shape), (v[..., 0, :] * w[..., 0, :]).astype(F32))
    s = _hsum16(pv)
    return ((s[..., 0] + s[..., 1]) + F32(np.asarray(b3).reshape(-1)[0])).astype(F32)


def _packed(w, scaled):
    return w if isinstance(w, Packed) else Packed(w, scaled)


def actor_split(w, rows, scaled=True):
    """rows [..., 28] -> action float32 [...]: actor_tile32 on the packed weights `w` (a dict of critic.KEYS, or a Packed)"""
    p = _packed(w, scaled)
    x = np.asarray(rows).astype(F32)
    lead = x.shape[:-1]
    x = x.reshape(-1, 28)
    y = _ln_inputs(x, p.w["ln0_gamma"], p.w["ln0_beta"])
    h = _dense(y, _pad_rows(p.kh[0], 32), _pad_rows(p.kl[0], 32), p.bias[0])
    h = _ln_relu_centred(h, p.w["ln1_gamma"], p.w["ln1_beta"], p.eps[0])
    g = _dense(h, p.kh[1], p.kl[1], p.bias[1])
    g = _ln_relu_centred(g, p.w["ln2_gamma"], p.w["ln2_beta"], p.eps[1])
    z = _head(g, p.w["w3"], p.w["b3"])
    return (3.0 * np.tanh(z.astype(F64))).astype(F32).reshape(lead)


def critic_split(w, rows, act7, scaled=True):
    """rows [..., 28], act7 [..., 7] -> Q float32 [...]: critic_tile32 on the packed weights `w` (w2 is [71][64])"""
    p = _packed(w, scaled)
    x = np.asarray(rows).astype(F32)
    lead = x.shape[:-1]
    x = x.reshape(-1, 28)
    a = np.asarray(act7).astype(F32).reshape(-1, 7)
    y = _ln_inputs(x, p.w["ln0_gamma"], p.w["ln0_beta"])
    h = _dense(y, _pad_rows(p.kh[0], 32), _pad_rows(p.kl[0], 32), p.bias[0])
    h = _ln_relu_centred(h, p.w["ln1_gamma"], p.w["ln1_beta"], p.eps[0])
    in2 = np.zeros((len(x), 80), F32)                                 # K-block 4: the seven actions, then zeros
    in2[:, :64], in2[:, 64:71] = h, a
    g = _dense(in2, _pad_rows(p.kh[1], 80), _pad_rows(p.kl[1], 80), p.bias[1])
    g = _ln_relu_centred(g, p.w["ln2_gamma"], p.w["ln2_beta"], p.eps[1])
    return _head(g, p.w["w3"], p.w["b3"]).reshape(lead)


def bootstrap_split(actor_w, critic_w, state, scaled=True):
    """state [..., 7, 28] -> (q [...], act7 [..., 7]) float32: every row through the actor, row 0 and the actions through the critic"""
    st = np.asarray(state)
    a7 = actor_split(actor_w, st, scaled)
    return critic_split(critic_w, st[..., 0, :], a7, scaled), a7

"""Float64 reference of the extended Adam step (csrc/train_ops.hip:
adam_ex_elem / smer_adam_ex) and the per-element error bound of the fp32
kernel, derived from the kernel's operation sequence.

The step, per element (s = ctl[1] of the guarded step, 1 otherwise):

    G  = g s                      [+ wd p   when coupled]
    P0 = p                        [  p decay_mul   when decoupled]
    M  = m + k1 (G - m)           k1 = 1 - b1
    V  = v b2 + (k2 G) G          k2 = 1 - b2
    D  = sqrt(V) / bc2s + eps
    P  = P0 - (lr / bc1) (M / D)
    E  = e + k3 (P - e)           k3 = 1 - ema_decay

which is torch.optim.AdamW (decoupled) / torch.optim.Adam(weight_decay=)
(coupled, on the clipped gradient) to float64 accuracy
(tests/test_adam_ex_cpu.py).

The bound.  Every fp32 operation returns fl(x) = x (1 + d) + h with |d| <= u =
2^-24 and |h| <= ETA = 2^-150 (half the smallest denormal; sqrt and division
are correctly rounded in the library's build).  `_r(x)` below is that one
rounding, u |x| + ETA.  The kernel's operations, in order, and the absolute
error each one leaves (first order; hats dropped, |.| of the float64 values):

  G   guarded: one product                 eG  = _r(g s)
      coupled: product wd p, then the sum  eG += _r(wd p) + _r(|g s| + |wd p|)
  P0  decoupled: one product               eP0 = _r(p decay_mul)
  M   k1 is one rounding (u k1); G - m is one rounding of at most |G| + |m|;
      k1 (G - m) one more; the sum one more:
        ed = eG + _r(|G| + |m|)
        eM = k1 ed + 2 _r(k1 |G - m|) + _r(|m| + k1 |G - m|)
  V   v b2: one rounding.  (k2 G) G: k2's own rounding, two products, and G's
      error twice; the sum one more:
        eV = _r(v b2) + 3 _r(k2 G^2) + 2 k2 |G| eG + _r(|v b2| + k2 G^2)
  D   |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt(|a - b|)), then the
      root's, the quotient's and the sum's rounding:
        er = min(eV / sqrt(V), sqrt(eV)) + _r(sqrt(V))
        eD = er / bc2s + _r(sqrt(V) / bc2s) + _r(sqrt(V) / bc2s + eps)
  P   M / D with D no smaller than D - eD; lr / bc1 is one rounding, its
      product with the quotient another, the subtraction the last:
        eQ = eM / (D - eD) + |M| eD / (D (D - eD)) + _r(M / D)
        eS = (lr / bc1) eQ + 2 _r((lr / bc1) M / D)
        eP = eP0 + eS + _r(|P0| + |(lr / bc1) M / D|)
  E   k3 one rounding, P - e one, the product one, the sum one:
        ee = eP + _r(|P| + |e|)
        eE = k3 ee + 2 _r(k3 |P - e|) + _r(|e| + k3 |P - e|)

Where the compiler contracts a product into the following sum (v_fma_f32)
that product is not rounded at all: every such term only over-counts.  SLACK
= 1.01 covers the second-order terms (products of two errors, u^2).  Nothing
here is fitted to device output.
"""
import math

import numpy as np

U = 2.0 ** -24  # fp32 unit roundoff
ETA = 2.0 ** -150  # absolute error of a rounding into the denormal range
SLACK = 1.01


def f32(x):
    """The double a C `float` argument holds."""
    return float(np.float32(x))


def kernel_hp(*, lr, b1, b2, eps, step, weight_decay=0.0, decoupled=True, ema_decay=0.0):
    """The scalars smer_adam_ex receives for these host-side values
    (ops.adam_ex forms them in double; the C ABI rounds each to fp32 once)."""
    bc1 = 1.0 - b1 ** step
    bc2s = math.sqrt(1.0 - b2 ** step)
    decay_mul = 1.0 - float(lr) * float(weight_decay) if decoupled else 1.0
    return dict(lr=f32(lr), b1=f32(b1), b2=f32(b2), eps=f32(eps), bc1=f32(bc1), bc2s=f32(bc2s),
                wd=f32(weight_decay), decay_mul=f32(decay_mul), decoupled=bool(decoupled),
                ema_decay=f32(ema_decay))


def _r(x):
    return U * np.abs(x) + ETA


def step64(p, g, m, v, ema=None, *, lr, b1, b2, eps, bc1, bc2s, wd=0.0, decay_mul=1.0, decoupled=True,
           ema_decay=0.0, scale=None, bound=True):
    """One step in float64 from the given state.  scale: ctl[1] of a guarded
    step (None: unguarded).  Returns (values, bounds): dicts of float64
    arrays under 'p', 'm', 'v' and, when ema is given, 'ema'; bounds holds
    the fp32 kernel's per-element absolute error bound (None if not asked)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    zero = np.zeros_like(p)
    G = g * float(scale) if scale is not None else g.copy()
    eG = _r(G) if scale is not None else zero
    if not decoupled and wd != 0:
        w = wd * p
        eG = eG + _r(w) + _r(np.abs(G) + np.abs(w))
        G = G + w
    P0, eP0 = p, zero
    if decoupled:
        P0 = p * decay_mul
        eP0 = _r(P0)
    k1, k2 = 1.0 - b1, 1.0 - b2
    d = G - m
    M = m + k1 * d
    V = v * b2 + (k2 * G) * G
    rt = np.sqrt(V)
    D = rt / bc2s + eps
    step = lr / bc1
    S = step * (M / D)
    P = P0 - S
    out = {"p": P, "m": M, "v": V}
    if ema is not None:
        e = np.asarray(ema, dtype=np.float64)
        k3 = 1.0 - ema_decay
        out["ema"] = e + k3 * (P - e)
    if not bound:
        return out, None
    ed = eG + _r(np.abs(G) + np.abs(m))
    eM = k1 * ed + 2 * _r(k1 * d) + _r(np.abs(m) + k1 * np.abs(d))
    eV = _r(v * b2) + 3 * _r(k2 * G * G) + 2 * k2 * np.abs(G) * eG + _r(np.abs(v * b2) + k2 * G * G)
    with np.errstate(divide="ignore", invalid="ignore"):
        er = np.where(V > 0, np.minimum(eV / np.where(V > 0, rt, 1.0), np.sqrt(eV)), np.sqrt(eV)) + _r(rt)
    eD = er / bc2s + _r(rt / bc2s) + _r(rt / bc2s + eps)
    Dlo = D - eD
    assert (Dlo > 0).all(), "the denominator's error reaches the denominator"
    eQ = eM / Dlo + np.abs(M) * eD / (D * Dlo) + _r(M / D)
    eS = step * eQ + 2 * _r(S)
    eP = eP0 + eS + _r(np.abs(P0) + np.abs(S))
    bnd = {"p": SLACK * eP, "m": SLACK * eM, "v": SLACK * eV}
    if ema is not None:
        ee = eP + _r(np.abs(P) + np.abs(e))
        dd = k3 * np.abs(P - e)
        bnd["ema"] = SLACK * (k3 * ee + 2 * _r(dd) + _r(np.abs(e) + dd))
    return out, bnd


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)

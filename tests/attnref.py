"""float64 reference, bf16 emulation, cases and bounds of the training
attention kernels (csrc/attention.hip: smer_attn_fwd, smer_attn_bwd,
smer_attn_weights).  Plain torch on the CPU; tests/test_attention_ref_cpu.py
checks this file against torch.autograd and derives the bf16 constants below,
tests/test_attention_edges_gpu.py holds the kernels to them.  expected_fwd_plan
and expected_bwd_plan state which kernels a call runs (the training dispatch
of csrc/attn_plan.h, written independently); both test modules hold them
against the library's own answer (smer_attn_fwd_plan / smer_attn_bwd_plan).

Convention (the kernels' and this file's): a query with no visible key has
O = 0, lse = +inf and contributes to no gradient; its dQ row is zero.  A
padded key's dK / dV rows are zero.  `causal` aligns key j with query j also
when Lq != Lk: key j is visible to query i iff j <= i (and it is not padded).

Bound rule.  Every output element is compared with the float64 value
computed from the bits the kernel read, against a bound of that element:

* fp32 kernels: (k + 2) * 2**-24 * T, k the number of accumulated terms
  (Lk + D for O and dQ, Lq + D for dK and dV) and T the summed magnitude of
  the element's terms;
* bf16 kernels: ATTN_REL_x * T + 2**-8 * |ref| (the bf16 store), lse to
  ATTN_ABS_LSE.  Each constant is four times the worst value, over every
  shape of SHAPES under every mask set and dropout rate it is run with, of
  |attn_emulated - attn_ref64| / (T + |ref|), attn_emulated being the same
  formulas in float64 with a bf16 rounding wherever the kernels round.  They
  are never tuned against a kernel's output.

T per output: O: sum_j pd_ij |v_jd|;  dV: sum_i pd_ij |do_id|;
dQ: scale * sum_j w_ij |k_jd|;  dK: scale * sum_i w_ij |q_id|, with
pd = p * keep * drop_scale and
w_ij = p_ij (keep_ij drop_scale sum_d |do_id v_jd| + sum_d |do_id o_id|),
the magnitude of every product behind ds_ij = p_ij (keep drop_scale dp_ij -
delta_i), dp_ij = sum_d do_id v_jd, delta_i = sum_d do_id o_id.  |ds_ij|
itself cannot carry a bound: for a query with a single visible key (every
causal row 0) dp and delta cancel exactly, so |ds| = 0 would ask for
bit-exact zeros of kernels that sum dp and delta in different orders and
form delta from the bf16-rounded O; and |dp_ij| + |delta_i| fails the same
way on the rows where dp itself cancels (the emulation alone then reaches
0.8 of it).  The rounding of O moves delta by up to 2**-9 sum_d |do o|, which
is what w bounds.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from tests.hashref import attn_keep_mask, attn_scale

LOG2E_F = float(np.float32(1.4426950408889634))
LN2_F = float(np.float32(0.6931471805599453))
U = 2.0 ** -24
UB = 2.0 ** -8

# Worst |attn_emulated - attn_ref64| / (T + |ref|) over SHAPES (lse: worst
# absolute difference), measured by tests/test_attention_ref_cpu.py
# (test_bf16_bounds prints them):
#   O 0.00579997  lse 0.00711157  dQ 0.00253722  dK 0.00447855  dV 0.00687401
ATTN_WORST = dict(O=5.80e-3, lse=7.12e-3, dQ=2.54e-3, dK=4.48e-3, dV=6.88e-3)
ATTN_REL_O = 4 * ATTN_WORST["O"]
ATTN_ABS_LSE = 4 * ATTN_WORST["lse"]
ATTN_REL_DQ = 4 * ATTN_WORST["dQ"]
ATTN_REL_DK = 4 * ATTN_WORST["dK"]
ATTN_REL_DV = 4 * ATTN_WORST["dV"]


def f32r(x):
    """A Python scalar as a C `float` parameter holds it."""
    return float(np.float32(x))


def bf16r(x):
    """float64 -> fp32 -> bf16 (round to nearest even) -> float64: the
    kernels round fp32 registers."""
    return x.float().bfloat16().double()


def _heads(x, B, L, H, D):
    return x.double().reshape(B, L, H, D).permute(0, 2, 1, 3)


def _rows(x):
    B, H, L, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * D)


def visible(B, Lq, Lk, kpm, causal):
    """bool [B, 1, Lq, Lk]: key j is visible to query i."""
    vis = torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    if kpm is not None:
        vis &= ~kpm.bool().view(B, 1, 1, Lk)
    if causal:
        vis &= torch.tril(torch.ones(Lq, Lk, dtype=torch.bool)).view(1, 1, Lq, Lk)
    return vis


def _backward_sums(p, pd, keepf, dsc, q, k, v, do, O, scale):
    w = p * (keepf * dsc * (do.abs() @ v.abs().transpose(-1, -2)) + (do * O).abs().sum(-1, keepdim=True))
    return dict(sdQ=_rows(scale * (w @ k.abs())), sdK=_rows(scale * (w.transpose(-1, -2) @ q.abs())),
                sdV=_rows(pd.transpose(-1, -2) @ do.abs()))


def attn_ref64(q, k, v, do, B, H, Lq, Lk, D, kpm, causal, scale, keep=None, drop_scale=1.0):
    """float64 attention forward and backward from the stored inputs.
    q, do: [B*Lq, H*D]; k, v: [B*Lk, H*D]; kpm: [B, Lk] (nonzero = padded) or
    None; keep: bool [B, H, Lq, Lk] or None.  Returns O, dQ [B*Lq, H*D], dK,
    dV [B*Lk, H*D], lse and has (query sees a key) [B, H, Lq], and the summed
    term magnitudes sO, sdQ, sdK, sdV of the module docstring."""
    scale, dsc = f32r(scale), f32r(drop_scale)
    q, k, v, do = _heads(q, B, Lq, H, D), _heads(k, B, Lk, H, D), _heads(v, B, Lk, H, D), _heads(do, B, Lq, H, D)
    vis = visible(B, Lq, Lk, kpm, causal)
    s = (q @ k.transpose(-1, -2)) * scale
    s = torch.where(vis, s, torch.full_like(s, -math.inf))
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    has = l > 0
    p = e / torch.where(has, l, torch.ones_like(l))
    lse = torch.where(has, m + torch.log(torch.where(has, l, torch.ones_like(l))),
                      torch.full_like(l, math.inf)).squeeze(-1)
    keepf = torch.ones(()).double() if keep is None else keep.double()
    pd = p * keepf * dsc
    O = pd @ v
    dp = do @ v.transpose(-1, -2)
    delta = (do * O).sum(-1)
    ds = p * (keepf * dsc * dp - delta.unsqueeze(-1))
    r = SimpleNamespace(O=_rows(O), lse=lse, has=has.squeeze(-1).expand(B, H, Lq), sO=_rows(pd @ v.abs()),
                        dQ=_rows(scale * (ds @ k)), dK=_rows(scale * (ds.transpose(-1, -2) @ q)),
                        dV=_rows(pd.transpose(-1, -2) @ do),
                        **_backward_sums(p, pd, keepf, dsc, q, k, v, do, O, scale))
    return r


def attn_emulated(q, k, v, do, B, H, Lq, Lk, D, kpm, causal, scale, keep=None, drop_scale=1.0):
    """attn_ref64's formulas in float64 with a bf16 round-to-nearest-even at
    every point where the bf16 kernels of csrc/attention.hip round (the MFMA
    sums themselves are fp32 in the kernels, float64 here).  Returns O, lse,
    dQ, dK, dV as attn_ref64 does; the backward consumes the emulated O and
    lse, as the kernels' backward consumes their forward's.

    Forward, attn_fwd_bf16:
     1. c = scale * log2(e) as an fp32 product (l.240); Q is replaced by
        bf16(Q * c) (l.331), so the scores are in log2 units.
     2. p = 2^(s - m) (l.419; the kernel's m is a deferred reference within
        2^8 of the row max, here the row max), l = sum of the unrounded p
        over all visible keys, dropped ones included (l.420).
     3. P is rounded to bf16 for the P.V MFMA (pack2, l.428-429) and dropped
        entries are zeroed (l.439-440 / l.451-452); the survivors' factor is
        not in P but in the final 1 / l (l.506).
     4. O = bf16(acc * drop_scale / l) (l.512); lse = (m + log2 l) * ln 2 in
        fp32 (l.523).
    dQ, attn_bwd_dq_bf16:
     5. Q as in 1 (l.902); lse2 = fp32(lse * log2 e) (l.871);
        delta = sum_d dO * O over the stored bf16 O (l.884).
     6. p = 2^(Qc.K - lse2) (l.970); dS = p (keep * dP * drop_scale - delta)
        (l.973) is rounded to bf16 for the dS.K MFMA (pack_p, l.976-977).
     7. dQ = bf16(acc * scale) (l.1015).
    dK / dV, attn_bwd_dkdv_bf16:
     8. K is replaced by bf16(K * c) (l.657): p = 2^(Q.Kc - lse2) (l.695).
     9. P with the dropped entries zeroed and without the survivors' factor is
        rounded to bf16 for the dV MFMA (l.708, pack_p l.715-716);
        dV = bf16(acc * drop_scale) (l.755).
    10. dS as in 6 from this kernel's p (l.712) rounded to bf16 (l.717-718);
        dK = bf16(acc * scale) (l.754).
    """
    scale, dsc = f32r(scale), f32r(drop_scale)
    c = f32r(np.float32(scale) * np.float32(LOG2E_F))
    q, k, v, do = _heads(q, B, Lq, H, D), _heads(k, B, Lk, H, D), _heads(v, B, Lk, H, D), _heads(do, B, Lq, H, D)
    vis = visible(B, Lq, Lk, kpm, causal)
    keepf = torch.ones(()).double() if keep is None else keep.double()
    ninf = lambda x: torch.full_like(x, -math.inf)  # noqa: E731
    # forward
    qc = bf16r(q * c)                                                # 1
    s2 = qc @ k.transpose(-1, -2)
    s2 = torch.where(vis, s2, ninf(s2))
    m = s2.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp2(s2 - m)                                           # 2
    l = p.sum(-1, keepdim=True)
    has = l > 0
    l1 = torch.where(has, l, torch.ones_like(l))
    pb = bf16r(p) * keepf                                            # 3
    O = bf16r((pb @ v) * (dsc / l1))                                 # 4
    lse = torch.where(has, ((m + torch.log2(l1)) * LN2_F).float().double(), torch.full_like(l, math.inf))
    # backward
    lse2 = (lse * LOG2E_F).float().double()                          # 5
    delta = (do * O).sum(-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    g = keepf * dp * dsc - delta
    pq = torch.where(vis, torch.exp2(s2 - lse2), torch.zeros_like(s2))  # 6
    dQ = bf16r((bf16r(pq * g) @ k) * scale)                          # 7
    kc = bf16r(k * c)                                                # 8
    sk = q @ kc.transpose(-1, -2)
    pk = torch.where(vis, torch.exp2(sk - lse2), torch.zeros_like(sk))
    dV = bf16r((bf16r(pk * keepf).transpose(-1, -2) @ do) * dsc)     # 9
    dK = bf16r((bf16r(pk * g).transpose(-1, -2) @ q) * scale)        # 10
    return SimpleNamespace(O=_rows(O), lse=lse.squeeze(-1), dQ=_rows(dQ), dK=_rows(dK), dV=_rows(dV))


def weights_ref64(q, k, lse, B, H, Lq, Lk, D, kpm, causal, scale):
    """smer_attn_weights in float64 from the lse it is given: the mean over
    heads of exp(s - lse) on the visible keys, 0 elsewhere.  A query without a
    visible key gets a zero row: attn_weights_kernel adds nothing for an
    invisible key and never reads that query's lse (+inf).  Returns the
    weights [B, Lq, Lk] and, for the bounds, the head means of p_ij and of
    p_ij * scale * sum_d |q_id k_jd|."""
    scale = f32r(scale)
    q, k = _heads(q, B, Lq, H, D), _heads(k, B, Lk, H, D)
    vis = visible(B, Lq, Lk, kpm, causal).expand(B, H, Lq, Lk)
    s = (q @ k.transpose(-1, -2)) * scale
    lse = lse.double().view(B, H, Lq, 1)
    fin = torch.isfinite(lse)
    p = torch.where(vis & fin, torch.exp(s - torch.where(fin, lse, torch.zeros_like(lse))), torch.zeros_like(s))
    sabs = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    return p.mean(1), (p * sabs).mean(1)


def f32_lse_bound(q, k, ref, B, H, Lq, Lk, D, scale):
    """Bound of the fp32 forward's lse, [B, H, Lq]: a score is an fp32 sum of
    D products ((D + 2) u of their summed magnitude, the row's largest), the
    normaliser a sum of Lk terms, and m + log l two more roundings."""
    q, k = _heads(q, B, Lq, H, D), _heads(k, B, Lk, H, D)
    smax = ((q.abs() @ k.abs().transpose(-1, -2)) * f32r(scale)).max(-1).values
    lse = torch.where(ref.has, ref.lse, torch.zeros_like(ref.lse))
    return (D + 2) * U * smax + (Lk + 2) * U + 4 * U * lse.abs().clamp_min(1.0)


# ------------------------------------------------------------------ cases
MASK_KINDS = ("none", "tail", "first64", "first70", "tile1", "third", "all")


def mask_kinds(Lk):
    """The padding patterns that Lk allows."""
    ks = ["none"]
    if Lk >= 3:
        ks.append("tail")      # the last third
    if Lk > 64:
        ks.append("first64")   # the first 64-key tile wholly padded
    if Lk > 70:
        ks.append("first70")   # ... and the first visible key mid-tile
    if Lk > 128:
        ks.append("tile1")     # an interior tile (keys 64..127) wholly padded
    if Lk >= 2:
        ks.append("third")     # isolated holes: every third key, key 0 included
    ks.append("all")           # no visible key in the sequence
    return ks


def mask_row(kind, Lk):
    r = torch.zeros(Lk, dtype=torch.uint8)
    if kind == "tail":
        r[Lk - Lk // 3:] = 1
    elif kind == "first64":
        r[:64] = 1
    elif kind == "first70":
        r[:70] = 1
    elif kind == "tile1":
        r[64:128] = 1
    elif kind == "third":
        r[0::3] = 1
    elif kind == "all":
        r[:] = 1
    return r


def mask_sets(B, Lk):
    """Lists of B kinds, one per sequence, that together carry every kind Lk
    allows: one list when B is large enough, else consecutive groups of B."""
    ks = mask_kinds(Lk)
    if B >= len(ks):
        return [[ks[b % len(ks)] for b in range(B)]]
    return [[ks[(i + b) % len(ks)] for b in range(B)] for i in range(0, len(ks), B)]


def make_kpm(kinds, Lk):
    return torch.stack([mask_row(kd, Lk) for kd in kinds])


def _shape_table():
    t = []
    for Lq, Lk in ((1, 1), (1, 65), (17, 1)):
        t += [(2, 3, Lq, Lk, D, False) for D in (32, 64, 128)]
    for Lq, Lk in ((15, 63), (16, 64), (17, 65), (130, 70), (70, 130)):
        t += [(2, 3, Lq, Lk, D, cz) for D in (32, 64, 128) for cz in (False, True)]
    t += [(2, 3, 129, 129, D, True) for D in (64, 128)]
    t += [(64, 8, 70, 70, D, cz) for D in (32, 64) for cz in (False, True)]
    t += [(64, 8, 64, 64, 64, True)]
    t += [(32, 8, 200, 130, 64, cz) for cz in (False, True)]
    t += [(64, 8, 70, 200, 64, False), (64, 8, 200, 70, 64, False), (64, 8, 70, 70, 128, False)]
    return t


SHAPES = _shape_table()   # (B, H, Lq, Lk, D, causal)
DROP_SEED = 77


def drop_rates(B, H, Lq, Lk, D, causal):
    """Dropout rates a shape is also run with: the ragged shapes and the
    two-group shapes at p = 0.1, one of them at p = 0.5 as well."""
    ragged = (Lq, Lk) in ((17, 65), (70, 130), (130, 70)) and D == 64
    two_group = B * H >= 256 and D <= 64
    if not (ragged or two_group):
        return ()
    return (0.1, 0.5) if (B, Lq, Lk, causal) == (2, 70, 130, False) else (0.1,)


def shape_id(s):
    return "B%dH%d-%dx%d-D%d-%s" % (s[0], s[1], s[2], s[3], s[4], "causal" if s[5] else "full")


def inputs(shape, dtype, exact=False):
    """Deterministic CPU inputs of a shape: q, do [B*Lq, H*D], k, v
    [B*Lk, H*D] in `dtype`.  exact: the mask test's inputs (Q = 0, V small
    integers: every visible p is 1 and the sums are exact)."""
    B, H, Lq, Lk, D, causal = shape
    g = torch.Generator().manual_seed(1000 * Lq + Lk + 7 * D + B)
    q = torch.randn(B * Lq, H * D, generator=g).to(dtype)
    k = torch.randn(B * Lk, H * D, generator=g).to(dtype)
    v = torch.randn(B * Lk, H * D, generator=g).to(dtype)
    do = torch.randn(B * Lq, H * D, generator=g).to(dtype)
    if exact:
        q = torch.zeros_like(q)
        v = torch.randint(-4, 5, (B * Lk, H * D), generator=g).to(dtype)
    return q, k, v, do


def keep_mask(shape, p):
    B, H, Lq, Lk, D, causal = shape
    return torch.from_numpy(attn_keep_mask(DROP_SEED, p, B * H * Lq, Lk)).view(B, H, Lq, Lk)


def scale_of(D):
    return 1.0 / math.sqrt(D)


@functools.lru_cache(maxsize=2)
def reference(shape, kinds, dtype, p=0.0):
    """attn_ref64 of inputs(shape, dtype) under the masks `kinds` (a tuple,
    one kind per sequence) and dropout rate p; shared, do not modify."""
    B, H, Lq, Lk, D, causal = shape
    q, k, v, do = inputs(shape, dtype)
    keep = keep_mask(shape, p) if p else None
    return attn_ref64(q, k, v, do, B, H, Lq, Lk, D, make_kpm(kinds, Lk), causal, scale_of(D), keep, attn_scale(p))


def f32_bounds(ref, Lq, Lk, D):
    """Per-element bounds of the fp32 kernels (module docstring)."""
    return dict(O=(Lk + D + 2) * U * ref.sO, dQ=(Lk + D + 2) * U * ref.sdQ,
                dK=(Lq + D + 2) * U * ref.sdK, dV=(Lq + D + 2) * U * ref.sdV)


def bf16_bounds(ref):
    return dict(O=ATTN_REL_O * ref.sO + UB * ref.O.abs(), dQ=ATTN_REL_DQ * ref.sdQ + UB * ref.dQ.abs(),
                dK=ATTN_REL_DK * ref.sdK + UB * ref.dK.abs(), dV=ATTN_REL_DV * ref.sdV + UB * ref.dV.abs())


# --------------------------------------------------------------- dispatch
F32, BF16 = torch.float32, torch.bfloat16
FAMILIES = ("bf16_flash", "f32_mfma", "f32_valu")   # smer_attn_fwd_plan's family ids
FwdPlan = namedtuple("FwdPlan", "family D QG DROP MIN Q8 grid block lds mask_gen")
BwdKernel = namedtuple("BwdKernel", "D G DROP MSK CAUSAL grid")
BwdPlan = namedtuple("BwdPlan", "family dq dkdv dq_first delta_pass block f32_grids")
PLAN_DROP, PLAN_MASK, PLAN_MASK_IN, PLAN_Q8, PLAN_F32_ALIGNED, PLAN_CAUSAL = 1, 2, 4, 8, 16, 32   # include/smer_hip.h


def _cdiv(a, b):
    return -(-a // b)


def two_groups(L, B, H, D):
    """Two query (or key) groups per wave: enough 128-row blocks to fill the
    chip, head dim up to 64."""
    return _cdiv(L, 128) * B * H >= 512 and D <= 64


def expected_fwd_plan(dtype, B, H, Lq, Lk, D, drop=False, mask=False, mask_in=False, q8=False, aligned=True,
                      f32_mfma=True):
    """What smer_attn_fwd (q8: smer_attn_fwd_fp8) launches.  drop: the rate is
    not 0; mask: a keep-word buffer is passed, mask_in: already filled;
    aligned (fp32): q, k 16-B aligned with row strides % 4 == 0; f32_mfma: the
    SMER_ATTN_F32_MFMA switch.  bf16: attn_fwd_bf16<D, QG, DROP, MIN, Q8> on
    ceil(Lq / (64 QG)) x B H blocks, the mask generator first when the forward
    reads a buffer (MIN) the caller did not fill."""
    if dtype == F32:
        if D == 64 and not drop and aligned and f32_mfma:
            return FwdPlan("f32_mfma", D, 1, False, False, False, (_cdiv(Lq, 64), B * H), 256, 0, False)
        return FwdPlan("f32_valu", D, 1, drop, False, False, (_cdiv(Lq, 4), B * H), 256, 16 * Lk, False)
    QG = 2 if two_groups(Lq, B, H, D) else 1
    MIN = drop and mask and (mask_in or QG == 1)
    return FwdPlan("bf16_flash", D, QG, drop, MIN, q8 and D == 64, (_cdiv(Lq, 64 * QG), B * H), 256, 0,
                   MIN and not mask_in)


def expected_bwd_plan(dtype, B, H, Lq, Lk, D, drop=False, mask=False, causal=False):
    """What smer_attn_bwd launches.  bf16: attn_bwd_dq_bf16<D, DROP, QG, MSK,
    CAUSAL> first (it forms delta), then attn_bwd_dkdv_bf16<D, DROP, KG, MSK,
    CAUSAL>, MSK when the forward's keep words are passed; fp32: delta, P / dS,
    dK / dV, dQ on one thread per element."""
    if dtype == F32:
        n = (B * H * Lq, B * H * Lq * Lk, B * H * Lk * D, B * H * Lq * D)
        return BwdPlan("f32_valu", None, None, False, False, 256, tuple(_cdiv(x, 256) for x in n))

    def kernel(L):
        G = 2 if two_groups(L, B, H, D) else 1
        return BwdKernel(D, G, drop, drop and mask, causal, (_cdiv(L, 64 * G), B * H))
    return BwdPlan("bf16_flash", kernel(Lq), kernel(Lk), True, False, 256, (0, 0, 0, 0))


def _facts(drop, mask, mask_in=False, q8=False, aligned=False, causal=False):
    return (PLAN_DROP * bool(drop) | PLAN_MASK * bool(mask) | PLAN_MASK_IN * bool(mask_in) | PLAN_Q8 * bool(q8)
            | PLAN_F32_ALIGNED * bool(aligned) | PLAN_CAUSAL * bool(causal))


def library_fwd_plan(lib, dtype, B, H, Lq, Lk, D, drop=False, mask=False, mask_in=False, q8=False, aligned=True):
    """The library's own decision (smer_attn_fwd_plan: the attn_fwd_plan the
    launcher runs; nothing launched, no HIP call; SMER_ATTN_F32_MFMA from the
    environment) in the form of expected_fwd_plan."""
    import ctypes
    out = (ctypes.c_int * 11)()
    rc = lib.smer_attn_fwd_plan(1 if dtype == BF16 else 0, B, H, Lq, Lk, D, _facts(drop, mask, mask_in, q8, aligned), out)
    assert rc == 0, lib.smer_last_error()
    fam, D_, QG, DROP, MIN, Q8, gx, gy, block, lds, gen = out
    return FwdPlan(FAMILIES[fam], D_, QG, bool(DROP), bool(MIN), bool(Q8), (gx, gy), block, lds, bool(gen))


def library_bwd_plan(lib, dtype, B, H, Lq, Lk, D, drop=False, mask=False, causal=False):
    import ctypes
    out = (ctypes.c_int * 22)()
    rc = lib.smer_attn_bwd_plan(1 if dtype == BF16 else 0, B, H, Lq, Lk, D, _facts(drop, mask, causal=causal), out)
    assert rc == 0, lib.smer_last_error()
    o = list(out)
    kern = lambda v: BwdKernel(v[0], v[1], bool(v[2]), bool(v[3]), bool(v[4]), (v[5], v[6]))  # noqa: E731
    f32 = FAMILIES[o[0]] == "f32_valu"
    return BwdPlan(FAMILIES[o[0]], None if f32 else kern(o[4:11]), None if f32 else kern(o[11:18]), bool(o[1]),
                   bool(o[2]), o[3], tuple(o[18:22]))


def plan_mismatches(lib, setenv):
    """Every call of the table where library and mirror differ: SHAPES in
    both dtypes, without dropout and at the shape's drop_rates, with no mask
    buffer, one to fill and a filled one, the e4m3 copy on and off at
    D = 64 (bf16), fp32 with SMER_ATTN_F32_MFMA on and off (through
    `setenv(value or None)`) and with the alignment fact broken."""
    bad = []
    for mfma in (None, "1", "0"):
        setenv(mfma)
        for shape in SHAPES:
            B, H, Lq, Lk, D, causal = shape
            for dtype in (BF16, F32) if mfma is None else (F32,):
                for drop in (False,) + tuple(bool(p) for p in drop_rates(*shape)):
                    for mask, mask_in in ((False, False), (True, False), (True, True)):
                        if mask and not drop:
                            continue
                        for q8 in (False, True) if dtype == BF16 and D == 64 else (False,):
                            for al in (True, False) if dtype == F32 else (True,):
                                kw = dict(drop=drop, mask=mask, mask_in=mask_in, q8=q8, aligned=al)
                                m = expected_fwd_plan(dtype, B, H, Lq, Lk, D, f32_mfma=mfma != "0", **kw)
                                l = library_fwd_plan(lib, dtype, B, H, Lq, Lk, D, **kw)
                                if m != l:
                                    bad.append(("fwd", shape, dtype, kw, m, l))
                        kw = dict(drop=drop, mask=mask, causal=causal)
                        m, l = expected_bwd_plan(dtype, B, H, Lq, Lk, D, **kw), library_bwd_plan(lib, dtype, B, H, Lq, Lk, D, **kw)
                        if m != l:
                            bad.append(("bwd", shape, dtype, kw, m, l))
    setenv(None)
    return bad

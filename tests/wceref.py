"""The label-smoothed weighted cross entropy of smer_wce_fwd_bwd_ex, written
from torch's definition and independently of the kernel, in float64 (or, for
the calibration, in fp32), with the inputs the CPU and GPU tests share.

For one row with logits x[0..V), target y, p = softmax(x), lp = log_softmax(x),
summed criterion weights w and W = sum_c w[c]:

    y == 0:  row_loss = row_nll = 0, grad = 0
    else:    row_nll  = w[y] * -lp[y]
             row_loss = (1-e) * row_nll + e/V * sum_c w[c] * -lp[c]
             grad[c]  = grad_scale/denom * ((1-e) * w[y] * (p[c] - [c == y])
                                            + e/V * (W * p[c] - w[c]))

which is sum_k CrossEntropyLoss(ignore_index=0, weight=w_k, reduction='none',
label_smoothing=e) for w = sum_k w_k (tests/test_label_smoothing_cpu.py holds
it against twelve such modules).  Scalars enter as the C-ABI's `float`
parameters hold them.
"""
import math

import numpy as np
import torch

LS_LD, LS_GS = 320, 0.37
LS_ROWS = [1, 2, 3, 5, 333]     # partial workgroups of the four-rows-per-block layout
LS_VS = [5, 64, 65, 309]        # less than a wave of columns, one, one plus one, the real size
LS_EPS = [0.1, 0.9]

# Worst error of wce_ls in fp32 torch (CPU) against its float64 evaluation over
# every (R, V, e) of LS_ROWS x LS_VS x LS_EPS, relative to the summed magnitude
# of the element's terms, measured by fp32_chain_worst_ls(): row_loss 1.95e-7,
# row_nll 1.28e-7, gradient 1.21e-6 (torch's vectorised fp32 exp is that far off
# on small probabilities).  The kernel uses the device's expf / logf and may
# contract to FMA, which the fp32 reference does not; four times the measured
# worst, as CE_REL_ROW / CE_REL_GRAD of tests/test_train_ops_gpu.py:
LS_WORST_ROW, LS_WORST_NLL, LS_WORST_GRAD = 1.95e-7, 1.28e-7, 1.21e-6
LS_REL_ROW, LS_REL_NLL, LS_REL_GRAD = 4 * LS_WORST_ROW, 4 * LS_WORST_NLL, 4 * LS_WORST_GRAD


def f32r(x):
    """A Python scalar as the C-ABI's `float` parameter holds it."""
    return float(np.float32(x))


def ls_inputs(R, V):
    """(logits buffer [R, LS_LD] with NaN pad columns, y, w, denom).  Targets
    0 (ignored), 2 and V-1 (w == 0 there, as in the summed criterion weights)
    as far as R allows, rows shifted by +-1e4; every other target has w > 0."""
    g_ = torch.Generator().manual_seed(900 + 7 * R + V)
    lbuf = torch.full((R, LS_LD), math.nan)            # pad columns: NaN, must not be read
    lbuf[:, :V] = torch.randn(R, V, generator=g_) * 3
    y = torch.randint(3, V - 1, (R,), generator=g_)
    if R >= 2:
        y[0], y[1] = 0, 2
        lbuf[1, :V] -= 1e4
    if R >= 3:
        y[2] = V - 1
    if R >= 5:
        lbuf[3, :V] += 1e4
    if R >= 100:
        y[10:17] = 0
        y[R - 1] = 0
        lbuf[20, :V] += 1e4
        lbuf[21, :V] -= 1e4
        y[21], y[22], y[23] = 0, 2, V - 1
        lbuf[23, :V] += 1e4
    w = torch.rand(V, generator=g_) + 0.05
    w[0] = w[2] = w[V - 1] = 0
    ce_all = torch.rand(V, generator=g_) + 0.05
    denom = ce_all[y].double().sum().float().reshape(1)   # an input of the kernel
    return lbuf, y, w, denom


def wce_ls(x, y, w, denom, eps, grad_scale=1.0, dtype=torch.float64):
    """x [R, V] logits, y int64 [R], w fp32 [V], denom [1], in `dtype`.
    Returns (row_loss, row_nll, grad) and, as ce_formula of
    tests/test_train_ops_gpu.py does, each one's summed term magnitudes
    (row_scale, nll_scale, grad_scale)."""
    x = x.to(dtype)
    R, V = x.shape
    rows = torch.arange(R)
    zero = torch.zeros((), dtype=dtype)
    e = torch.tensor(np.float32(eps)).to(dtype)
    gs = torch.tensor(np.float32(grad_scale)).to(dtype)
    wd = w.to(dtype)
    live = y != 0
    wy = torch.where(live, wd[y], zero)
    lp = torch.log_softmax(x, dim=1)
    p = torch.softmax(x, dim=1)
    nll = torch.where(live, wy * -lp[rows, y], zero)
    smooth = (wd[None, :] * -lp).sum(1)
    uni = e / V
    row = torch.where(live, (1 - e) * nll + uni * smooth, zero)
    onehot = torch.zeros_like(x)
    onehot[rows, y] = 1
    cy = (gs * (1 - e) * wy / denom.to(dtype))[:, None]
    cu = torch.where(live, gs * uni / denom.to(dtype), zero)[:, None]
    W = wd.sum()
    grad = cy * (p - onehot) + cu * (W * p - wd[None, :])
    # -lp[c] = log(se) - (x[c] - max): the two terms of every log-probability.
    # se >= 1 is itself a rounded sum, and a relative error u of se is an
    # absolute error u of log(se) however small log(se) is (se = 1 + tiny when
    # one logit dominates, as happens at V = 5): log(se) counts as 1 + |log(se)|
    mx = x.max(dim=1).values
    lse_c = torch.log(torch.exp(x - mx[:, None]).sum(1))
    mag = (1 + lse_c.abs())[:, None] + (x - mx[:, None]).abs()
    nll_scale = wy * mag[rows, y]
    row_scale = torch.where(live, (1 - e) * nll_scale + uni * (wd[None, :] * mag).sum(1), zero)
    grad_sc = cy.abs() * (p + onehot) + cu.abs() * (W * p + wd[None, :])
    return row, nll, grad, row_scale, nll_scale, grad_sc


def fp32_chain_worst_ls():
    """The calibration of LS_REL_ROW / _NLL / _GRAD (no GPU, no kernel output)."""
    worst = [0.0, 0.0, 0.0]
    for R in LS_ROWS:
        for V in LS_VS:
            lbuf, y, w, denom = ls_inputs(R, V)
            for eps in LS_EPS:
                hi = wce_ls(lbuf[:, :V], y, w, denom, eps, LS_GS, torch.float64)
                lo = wce_ls(lbuf[:, :V], y, w, denom, eps, LS_GS, torch.float32)
                for k in range(3):
                    err = (lo[k].double() - hi[k]).abs()
                    sc = hi[3 + k]
                    ok = sc > 0
                    assert torch.equal(err[~ok], torch.zeros_like(err[~ok]))
                    if ok.any():
                        worst[k] = max(worst[k], (err[ok] / sc[ok]).max().item())
    return worst

"""Label smoothing in the fused cross entropy, without a GPU: the float64
definition the GPU tests compare against (tests/wceref.py) is torch's own,
the argument checks of Trainer(label_smoothing=), and the calibration of the
GPU tests' bounds."""
import math

import pytest
import torch

from tests import wceref
from tests.wceref import LS_GS, LS_VS, ls_inputs, wce_ls

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']
V = 309


def _criteria():
    from smer_music_generation_amd.train import criterion_vectors
    from smer_music_generation_amd.vocab import WordVocab
    w, ce_all = criterion_vectors(WordVocab(0, CTRL), 0.8)
    assert len(w) == 12 and all(t.shape == (V,) for t in w.values())
    return w, ce_all


def _rows():
    """40 rows of logits with targets 0, 2 and V-1 among them."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(40, V, generator=g) * 3).double()
    y = torch.randint(1, V, (40,), generator=g)
    y[0] = y[7] = y[39] = 0
    y[1] = y[8] = 2
    y[2] = y[9] = V - 1
    x[8] += 1e4
    x[9] -= 1e4
    return x, y


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_wceref_is_the_sum_of_twelve_torch_criteria(eps):
    """Loss per row and the autograd gradient of sum(row_loss) / denom, in
    float64: twelve real CrossEntropyLoss(ignore_index=0, weight=w_k,
    reduction='none', label_smoothing=eps) modules against wce_ls on their
    summed weights.  eps as the kernel receives it (rounded to fp32)."""
    w, ce_all = _criteria()
    x, y = _rows()
    e = wceref.f32r(eps)
    denom = ce_all[y].double().sum().reshape(1)
    xt = x.clone().requires_grad_(True)
    crits = [torch.nn.CrossEntropyLoss(ignore_index=0, weight=wk.double(), reduction="none", label_smoothing=e)
             for wk in w.values()]
    rows_t = sum(c(xt, y) for c in crits)
    (rows_t.sum() / denom[0]).backward()
    w_total = sum(w.values())
    row, nll, grad, row_sc, _, grad_sc = wce_ls(x, y, w_total, denom, eps)
    tiny = 64 * 2.0 ** -53   # both sides are float64 sums of a few hundred terms
    assert ((row - rows_t.detach()).abs() <= tiny * row_sc).all()
    assert ((grad - xt.grad).abs() <= tiny * grad_sc).all()
    pad = y == 0
    assert pad.sum() == 3 and torch.equal(row[pad], torch.zeros(3, dtype=torch.float64))
    assert torch.equal(grad[pad], torch.zeros(3, V, dtype=torch.float64))
    zw = (y == 2) | (y == V - 1)
    nz = int(zw.sum())
    assert nz >= 4 and torch.equal(w_total[y[zw]], torch.zeros(nz))
    assert torch.equal(nll[zw], torch.zeros(nz, dtype=torch.float64))
    if eps > 0:   # torch smooths a row whose target has no weight
        assert (rows_t.detach()[zw] > 0).all() and (row[zw] > 0).all()
        assert (xt.grad[zw].abs().sum(1) > 0).all()
    else:
        assert torch.equal(row[zw], torch.zeros(nz, dtype=torch.float64))


@pytest.mark.parametrize("R", [2, 333])
def test_wceref_at_zero_is_the_plain_formula(R):
    """eps = 0 reproduces ce_formula's definition (tests/test_train_ops_gpu.py)
    on that module's own inputs, and row_nll is row_loss."""
    from tests.test_train_ops_gpu import CE_GS, CE_V, ce_formula, ce_inputs
    lbuf, y, w, denom = ce_inputs(R)
    if R >= 100:
        lbuf[22, :CE_V] = torch.nan_to_num(lbuf[22, :CE_V], neginf=-50.0)  # finite for both formulas
    row0, grad0, _, _ = ce_formula(lbuf, y, w, denom, torch.float64)
    row, nll, grad, _, _, _ = wce_ls(lbuf[:, :CE_V], y, w, denom, 0.0, CE_GS)
    assert torch.equal(row, nll)
    assert ((row - row0).abs() <= 8 * 2.0 ** -53 * row0.abs()).all()
    assert ((grad - grad0).abs() <= 8 * 2.0 ** -53 * grad0.abs()).all()


@pytest.mark.parametrize("bad", [-0.1, 1.0, math.nan, True, "0.1", None])
def test_trainer_refuses_a_bad_label_smoothing_before_any_device_work(bad):
    """The check runs before the model is touched: no model is given."""
    from smer_music_generation_amd.train import Trainer, check_label_smoothing
    with pytest.raises(ValueError, match="label_smoothing"):
        Trainer(None, None, label_smoothing=bad)
    with pytest.raises(ValueError, match="label_smoothing"):
        check_label_smoothing(bad)


def test_label_smoothing_values_accepted():
    from smer_music_generation_amd.train import check_label_smoothing
    import numpy as np
    assert check_label_smoothing(0) == 0.0 and check_label_smoothing(0.1) == 0.1
    assert check_label_smoothing(np.float32(0.5)) == 0.5
    assert check_label_smoothing(math.nextafter(1.0, 0.0)) < 1.0


def test_calibration_constants_are_the_measured_ones():
    """fp32_chain_worst_ls(): the formula in fp32 torch against float64 on the
    GPU test's inputs.  The recorded constants (of which the GPU bounds are
    four times) are what this measures, within the factor of two that
    torch's vectorised fp32 exp may differ by between CPU instruction sets."""
    worst = wceref.fp32_chain_worst_ls()
    print("fp32 chain worst: row_loss %.3g, row_nll %.3g, gradient %.3g" % tuple(worst))
    for got, rec in zip(worst, (wceref.LS_WORST_ROW, wceref.LS_WORST_NLL, wceref.LS_WORST_GRAD)):
        assert 0.5 * rec <= got <= 2 * rec, (got, rec)
    assert (wceref.LS_REL_ROW, wceref.LS_REL_NLL, wceref.LS_REL_GRAD) == (
        4 * wceref.LS_WORST_ROW, 4 * wceref.LS_WORST_NLL, 4 * wceref.LS_WORST_GRAD)


@pytest.mark.parametrize("Vv", LS_VS)
def test_inputs_hold_the_cases_the_gpu_test_names(Vv):
    lbuf, y, w, denom = ls_inputs(333, Vv)
    assert torch.isnan(lbuf[:, Vv:]).all() and torch.isfinite(lbuf[:, :Vv]).all()
    for t in (0, 2, Vv - 1):
        assert (y == t).any() and w[t] == 0
    assert (w[y[(y != 0) & (y != 2) & (y != Vv - 1)]] > 0).all()
    assert (lbuf[:, 0] > 5e3).any() and (lbuf[:, 0] < -5e3).any() and denom.item() > 0
    row, nll, grad, _, _, _ = wce_ls(lbuf[:, :Vv], y, w, denom, 0.1, LS_GS)
    assert torch.isfinite(row).all() and torch.isfinite(grad).all()
    zw = (y == 2) | (y == Vv - 1)
    assert (row[zw] > 0).all() and torch.equal(nll[zw], torch.zeros(int(zw.sum()), dtype=torch.float64))

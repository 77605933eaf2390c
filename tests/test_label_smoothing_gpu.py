"""Label smoothing inside the fused cross-entropy kernel
(smer_wce_fwd_bwd_ex) and through Trainer(label_smoothing=) on the GPU.

The kernel is held element by element to the float64 definition of
tests/wceref.py (which tests/test_label_smoothing_cpu.py holds against
torch's own criteria), at LS_REL_* times the summed magnitude of the
element's terms: four times the worst error of the same formula in fp32
torch on these inputs (see wceref), plus 2**-8 of the value for a bf16
store."""
import math

import numpy as np
import pytest
import torch

from tests.test_adam_ex_gpu import _micro
from tests.test_rccl_gpu import nccl_group  # noqa: F401  (the world-size-1 RCCL group)
from tests.test_train_ops_gpu import (BF16, F32, U, UB, assert_same_bits, assert_within, pads_intact)
from tests.wceref import (LS_EPS, LS_GS, LS_LD, LS_REL_GRAD, LS_REL_NLL, LS_REL_ROW, LS_ROWS, LS_VS, ls_inputs,
                          wce_ls)

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from smer_music_generation_amd import _lib as L
    L.load()


def ops():
    from smer_music_generation_amd import ops as O
    return O


def _call(inputs, V, dtype, eps, with_grad=True, with_loss=True, with_nll=True, entry="ex"):
    """One launch on sentinel-filled outputs; (row_loss, loss, dlogits buffer, row_nll)."""
    O = ops()
    lbuf, y, w, denom = inputs
    R = lbuf.shape[0]
    ldev, ydev, wdev, ddev = lbuf.to(dev), y.to(dev), w.to(dev), denom.to(dev)
    row = torch.full((R,), math.nan, device=dev)
    nll = torch.full((R,), math.nan, device=dev) if with_nll else None
    loss = torch.full((1,), math.nan, device=dev) if with_loss else None
    dl = torch.full((R, LS_LD), -7.0, device=dev, dtype=dtype) if with_grad else None
    dlv = dl[:, :V] if with_grad else None
    if entry == "ex":
        O.wce_fwd_bwd_ex(ldev[:, :V], ydev, wdev, ddev, row, loss, dlv, V=V, grad_scale=LS_GS,
                         label_smoothing=eps, row_nll=nll)
    else:
        O.wce_fwd_bwd(ldev[:, :V], ydev, wdev, ddev, row, loss, dlv, V=V, grad_scale=LS_GS)
    torch.cuda.synchronize()
    return row, loss, dl, nll


@pytest.mark.parametrize("eps", LS_EPS)
@pytest.mark.parametrize("V", LS_VS)
@pytest.mark.parametrize("R", LS_ROWS)
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_smoothed_ce_matches_float64(dtype, R, V, eps):
    """ldl = ldd = 320 > V with NaN pad columns in the logits and a sentinel
    in dlogits' pad columns; R = 1, 2, 3, 5: partial workgroups; targets 0, 2
    and V-1; rows shifted by +-1e4; grad_scale = 0.37; then the same call
    without dlogits, without loss_out and without row_nll."""
    inputs = ls_inputs(R, V)
    lbuf, y, w, denom = inputs
    row_ref, nll_ref, grad_ref, row_sc, nll_sc, grad_sc = wce_ls(lbuf[:, :V], y, w, denom, eps, LS_GS)
    loss_ref = row_ref.sum() / denom.double()
    assert torch.isfinite(row_ref).all() and torch.isfinite(grad_ref).all()
    pad = y == 0
    zw = (y == 2) | (y == V - 1)
    npad, nzw = int(pad.sum()), int(zw.sum())
    assert R < 3 or (npad > 0 and nzw > 1)

    def check(row, loss, dl, nll, what):
        assert_within(row, row_ref, LS_REL_ROW * row_sc, what + " row_loss")
        assert torch.equal(row.cpu()[pad], torch.zeros(npad)), what + ": row_loss on pad rows"
        assert (row.cpu()[zw] > 0).all(), what + ": a target without weight keeps the smoothing term"
        if nll is not None:
            assert_within(nll, nll_ref, LS_REL_NLL * nll_sc, what + " row_nll")
            assert torch.equal(nll.cpu()[pad | zw], torch.zeros(npad + nzw)), what + ": row_nll where w[y] = 0"
        if loss is not None:
            # R row losses (each within LS_REL_ROW of its terms) summed in fp32, one division
            lb = ((R + 2) * U * row_ref.abs().sum() + LS_REL_ROW * row_sc.sum()) / denom.double() + U * loss_ref.abs()
            assert_within(loss, loss_ref, lb, what + " loss")
        if dl is not None:
            gb = LS_REL_GRAD * grad_sc + (UB * grad_ref.abs() if dtype == BF16 else 0)
            assert_within(dl[:, :V], grad_ref, gb, what + " dlogits")
            g = dl[:, :V].float().cpu()
            assert torch.equal(g[pad], torch.zeros_like(g[pad])), what + ": gradient on pad rows"
            assert (g[zw].abs().sum(1) > 0).all(), what + ": gradient of a target without weight"
            pads_intact(dl, V, -7.0, what + " dlogits")

    row, loss, dl, nll = _call(inputs, V, dtype, eps)
    check(row, loss, dl, nll, "wce_ex")
    row2, loss2, _, nll2 = _call(inputs, V, dtype, eps, with_grad=False)
    check(row2, loss2, None, nll2, "wce_ex without dlogits")
    row3, _, dl3, nll3 = _call(inputs, V, dtype, eps, with_loss=False)
    check(row3, None, dl3, nll3, "wce_ex without loss_out")
    row4, loss4, dl4, _ = _call(inputs, V, dtype, eps, with_nll=False)
    check(row4, loss4, dl4, None, "wce_ex without row_nll")
    for what, got, want in (("without dlogits: row_loss", row2, row), ("without dlogits: loss", loss2, loss),
                            ("without dlogits: row_nll", nll2, nll), ("without loss_out: row_loss", row3, row),
                            ("without loss_out: dlogits", dl3, dl), ("without loss_out: row_nll", nll3, nll),
                            ("without row_nll: row_loss", row4, row), ("without row_nll: loss", loss4, loss),
                            ("without row_nll: dlogits", dl4, dl)):
        assert_same_bits(got, want, "wce_ex " + what)


@pytest.mark.parametrize("R,V", [(333, 309), (5, 65)])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_zero_smoothing_through_the_ex_entry_is_the_old_entry(dtype, R, V):
    """label_smoothing = 0: row_loss, loss and dlogits have smer_wce_fwd_bwd's
    bits and row_nll is row_loss -- also with a -inf logit off the target,
    which the plain loss does not see (no smoothing sum is formed)."""
    lbuf, y, w, denom = ls_inputs(R, V)
    r = 4
    assert y[r] != 0
    lbuf[r, (int(y[r]) + 1) % V] = -math.inf
    inputs = (lbuf, y, w, denom)
    row0, loss0, dl0, _ = _call(inputs, V, dtype, 0.0, entry="old")
    row, loss, dl, nll = _call(inputs, V, dtype, 0.0)
    assert torch.isfinite(row0).all() and torch.isfinite(dl0[:, :V].float()).all()
    assert_same_bits(row, row0, "row_loss")
    assert_same_bits(loss, loss0, "loss")
    assert_same_bits(dl, dl0, "dlogits")
    assert_same_bits(nll, row, "row_nll")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_one_minus_inf_logit_makes_that_row_inf_and_no_other(dtype):
    """x[c] = -inf with w[c] > 0 and label_smoothing > 0: +inf in torch, +inf
    here, in that row alone."""
    R, V, eps = 5, 309, 0.1
    lbuf, y, w, denom = ls_inputs(R, V)
    r = 4
    c = 5 if y[r] != 5 else 6
    assert y[r] != 0 and w[c] > 0
    lbuf[r, c] = -math.inf
    row_ref, nll_ref, grad_ref, row_sc, nll_sc, grad_sc = wce_ls(lbuf[:, :V], y, w, denom, eps, LS_GS)
    assert row_ref[r] == math.inf and torch.isfinite(nll_ref).all()
    row, loss, dl, nll = _call((lbuf, y, w, denom), V, dtype, eps)
    assert row[r].item() == math.inf and loss.item() == math.inf
    rest = torch.arange(R) != r
    assert_within(row.cpu()[rest], row_ref[rest], LS_REL_ROW * row_sc[rest], "row_loss of the other rows")
    assert_within(nll, nll_ref, LS_REL_NLL * nll_sc, "row_nll")
    gb = LS_REL_GRAD * grad_sc + (UB * grad_ref.abs() if dtype == BF16 else 0)
    assert_within(dl[:, :V].cpu()[rest], grad_ref[rest], gb[rest], "dlogits of the other rows")
    pads_intact(dl, V, -7.0, "dlogits")


def test_ex_entry_refuses_bad_arguments():
    O = ops()
    lbuf, y, w, denom = (t.to(dev) for t in ls_inputs(2, 64))
    row = torch.zeros(2, device=dev)
    for bad in (-0.1, 1.0, math.nan, math.inf):
        with pytest.raises(RuntimeError, match="label_smoothing"):
            O.wce_fwd_bwd_ex(lbuf[:, :64], y, w, denom, row, V=64, label_smoothing=bad)
    with pytest.raises(RuntimeError, match="null pointer"):
        O.wce_fwd_bwd_ex(lbuf[:, :64], y, w, denom, None, V=64, label_smoothing=0.1)


# --- Trainer -----------------------------------------------------------------
def _weights(m):
    return m.flat_parameters().detach().clone()


def _trainer(golden_dir, precision="bf16", **kw):
    from smer_music_generation_amd.train import Trainer
    m, v, bt, meta = _micro(golden_dir, precision)
    kw.setdefault("lr", 1e-3)
    return Trainer(m, v, eos_weight=meta["eos_weight"], **kw), m, bt, meta


def test_trainer_without_smoothing_is_the_step_as_it_was(golden_dir, monkeypatch):
    """label_smoothing=0.0 and no keyword: the same weights after two steps,
    bit for bit, and the extended entry is never called."""
    from smer_music_generation_amd import ops as O
    monkeypatch.setattr(O, "wce_fwd_bwd_ex", lambda *a, **k: pytest.fail("the plain step calls wce_fwd_bwd"))
    t0, m0, bt, _ = _trainer(golden_dir)
    t1, m1, _, _ = _trainer(golden_dir, label_smoothing=0.0)
    assert t0.label_smoothing == 0.0 and t1.label_smoothing == 0.0
    for _ in range(2):
        l0, l1 = t0.step(bt), t1.step(bt)
        assert_same_bits(l1, l0, "loss")
    t1.eval_step(bt, smoothed=True)
    assert_same_bits(_weights(m1), _weights(m0), "weights")
    sd = t1.state_dict()   # a constructor hyper-parameter, not optimizer state
    assert set(sd) == {"state", "param_groups"} and all("label_smoothing" not in g for g in sd["param_groups"])


def _float64_step(m, bt, meta, eps):
    """Loss and gradients of the twelve torch criteria with label_smoothing
    on a float64 copy of the model (the CPU restatement of the forward)."""
    from oracle import ref_cpu
    from smer_music_generation_amd.train import criterion_vectors
    from smer_music_generation_amd.vocab import WordVocab
    from tests.test_adam_ex_gpu import CTRL
    c = meta["config"]
    cfg = dict(d_model=c["d_model"], nhead=c["nhead"], num_encoder_layers=c["num_encoder_layers"],
               num_decoder_layers=c["num_decoder_layers"])
    params = {k: t.detach().cpu().double().requires_grad_(True) for k, t in m.named_parameters()}
    full = dict(params)
    full["pos_enc.pe"] = m.pos_enc.pe.detach().cpu().double()
    b = {k: t.cpu() for k, t in bt.items()}
    w, ce_all = criterion_vectors(WordVocab(0, CTRL), meta["eos_weight"])
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)   # the restatement builds its masks in the default dtype
    try:
        T = b["target_in"].shape[1]
        mask = ref_cpu.nopeek_mask(T).unsqueeze(0).repeat(b["input"].shape[0], 1, 1)
        logits, _ = ref_cpu.forward(full, cfg, b["input"], b["target_in"], b["input_pad_mask"],
                                    b["target_pad_mask"], b["input_pad_mask"].clone(), mask, training=False)
    finally:
        torch.set_default_dtype(old)
    assert logits.dtype == torch.float64
    x = logits.reshape(-1, logits.shape[-1])
    y = b["target_out"].reshape(-1).long()
    denom = ce_all[y].double().sum()
    loss = sum(torch.nn.CrossEntropyLoss(ignore_index=0, weight=wk.double(), reduction="none",
                                         label_smoothing=eps)(x, y).sum() / denom for wk in w.values())
    loss.backward()
    return loss.item(), {k: p.grad.numpy() for k, p in params.items()}


def test_trainer_smoothed_step_matches_float64_torch_criteria(golden_dir):
    """One fp32 step at lr = 0, dropout 0, label_smoothing = 0.1 against a
    float64 autograd model with the twelve torch criteria built with
    label_smoothing=0.1 and the same normaliser, at the tolerances
    tests/test_model_gpu.py grants the plain step on this fixture; then the
    two evaluation losses."""
    from tests.test_model_gpu import fro_rel
    eps = 0.1
    tr, m, bt, meta = _trainer(golden_dir, "fp32", lr=0.0, label_smoothing=eps)
    before = _weights(m)
    ref_loss, ref_grads = _float64_step(m, bt, meta, eps)
    plain_loss, _ = _float64_step(m, bt, meta, 0.0)
    assert abs(ref_loss - plain_loss) > 1e-3 * abs(plain_loss)   # the two objectives are apart
    loss = tr.step(bt)
    torch.cuda.synchronize()
    assert_same_bits(_weights(m), before, "weights after a step at lr = 0")
    assert abs(loss.item() - ref_loss) < 1e-5 * max(1.0, abs(ref_loss)), (loss.item(), ref_loss)
    for name, p in m.named_parameters():
        err = fro_rel(p.grad.cpu().numpy().astype(np.float64), ref_grads[name])
        assert err < 2e-3, (name, err)
    t0, _, _, _ = _trainer(golden_dir, "fp32")
    e_plain, parts, counts = tr.eval_step(bt)
    e0, parts0, counts0 = t0.eval_step(bt)
    assert_same_bits(e_plain, e0, "eval_step loss")
    assert torch.equal(counts, counts0)
    for k in parts0:
        assert_same_bits(parts[k], parts0[k], "eval_step part " + k)
    assert abs(e_plain.item() - plain_loss) < 1e-5 * max(1.0, abs(plain_loss))
    e_smooth, parts_s, _ = tr.eval_step(bt, smoothed=True)
    assert abs(e_smooth.item() - ref_loss) < 1e-5 * max(1.0, abs(ref_loss)), (e_smooth.item(), ref_loss)
    for k in parts0:
        assert_same_bits(parts_s[k], parts0[k], "eval_step(smoothed=True) part " + k)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_parts_under_smoothing_are_the_plain_parts(golden_dir, precision):
    ts, _, bt, _ = _trainer(golden_dir, precision, label_smoothing=0.1)
    t0, _, _, _ = _trainer(golden_dir, precision)
    ls, ps = ts.step(bt, return_parts=True)
    l0, p0 = t0.step(bt, return_parts=True)
    assert ps.keys() == p0.keys() and len(p0) == 12
    for k in p0:
        assert_same_bits(ps[k], p0[k], "part " + k)
    assert ls.item() != l0.item()


def test_label_smoothing_set_between_steps_is_read_by_the_next_step(golden_dir):
    t0, m0, bt, _ = _trainer(golden_dir)
    ts, ms, _, _ = _trainer(golden_dir, label_smoothing=0.1)
    ta, ma, _, _ = _trainer(golden_dir, label_smoothing=0.1)
    ta.label_smoothing = 0     # before the first step: the old bits again
    assert ta.label_smoothing == 0.0
    tb, mb, _, _ = _trainer(golden_dir)
    tb.label_smoothing = 0.1
    for t in (t0, ts, ta, tb):
        t.step(bt)
    assert_same_bits(_weights(ma), _weights(m0), "set to 0: weights")
    assert_same_bits(_weights(mb), _weights(ms), "set to 0.1: weights")
    assert not torch.equal(_weights(ms), _weights(m0))
    ts.label_smoothing = 0.0   # after a smoothed step: the plain step from these weights
    tc, mc, _, _ = _trainer(golden_dir)
    with torch.no_grad():
        mc.flat_parameters().copy_(ms.flat_parameters())
    mc.engine.mark_params_updated()
    tc.load_state_dict(ts.state_dict())
    ts.step(bt)
    tc.step(bt)
    assert_same_bits(_weights(ms), _weights(mc), "plain step after a smoothed one")
    with pytest.raises(ValueError, match="label_smoothing"):
        ts.label_smoothing = 1.0
    assert ts.label_smoothing == 0.0


def test_dp_world1_smoothed_step_equals_plain_smoothed_step(golden_dir, nccl_group):  # noqa: F811
    """Trainer(dp=True) over the world-size-1 RCCL group: the normaliser
    all-reduce ahead of the smoothed kernel and the bucketed gradient
    all-reduces are identities."""
    plain, m0, bt, _ = _trainer(golden_dir, label_smoothing=0.1)
    dp, m1, _, _ = _trainer(golden_dir, label_smoothing=0.1, dp=True)
    assert plain.dp is False and dp.dp is True and dp.world == 1
    for _ in range(2):
        l0, l1 = plain.step(bt), dp.step(bt)
        torch.cuda.synchronize()
        assert_same_bits(l1, l0, "loss")
        assert_same_bits(m1.flat_grad(), m0.flat_grad(), "gradient")
    assert_same_bits(_weights(m1), _weights(m0), "weights")

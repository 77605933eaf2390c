"""Host-side contract of the extended Adam step (include/smer_hip.h:
smer_adam_ex; train.Trainer weight_decay / decoupled_weight_decay /
ema_decay): the float64 reference of tests/adamref.py against torch's own
optimizers, the symbol and the argument checks that refuse a call before
anything is launched, FusedAdam's state dict in AdamW's format, and the
Trainer's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import adamref
from tests.dp_engine_common import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HOST_BUF = (ctypes.c_uint8 * 4096)()
INVALID = -1
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# --- the reference against torch ---------------------------------------------
@pytest.mark.parametrize("decoupled", [True, False], ids=["AdamW", "Adam_weight_decay"])
def test_reference_matches_torch_in_float64(decoupled):
    """5 steps on 1000 elements in float64.  The coupled form runs on a
    gradient that was scaled first, as clip_grad_norm_ leaves it: the decay
    term joins after the clip scale."""
    rng = np.random.default_rng(17 + decoupled)
    n, wd, scale = 1000, 0.01, 0.37
    p0 = rng.standard_normal(n)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([tp], lr=HP["lr"], betas=(HP["b1"], HP["b2"]), eps=HP["eps"], weight_decay=wd)
    p, m, v, e = p0.copy(), np.zeros(n), np.zeros(n), p0.copy()
    te = torch.from_numpy(p0.copy())
    for t in range(1, 6):
        g = rng.standard_normal(n) * 10 ** rng.uniform(-3, 1, n)
        tp.grad = torch.from_numpy(g * scale)  # what clip_grad_norm_ leaves in .grad
        opt.step()
        te.lerp_(tp.detach(), 1 - 0.9)
        out, _ = adamref.step64(p, g, m, v, e, **HP, bc1=1 - HP["b1"] ** t, bc2s=np.sqrt(1 - HP["b2"] ** t),
                                wd=wd, decay_mul=1 - HP["lr"] * wd, decoupled=decoupled, ema_decay=0.9,
                                scale=scale, bound=False)
        p, m, v, e = out["p"], out["m"], out["v"], out["ema"]
        st = opt.state[tp]
        assert _rel(p, tp.detach().numpy()) <= 1e-12, t
        assert _rel(m, st["exp_avg"].numpy()) <= 1e-12, t
        assert _rel(v, st["exp_avg_sq"].numpy()) <= 1e-12, t
        assert _rel(e, te.numpy()) <= 1e-12, t
    assert float(np.abs(p - p0).max()) > 1e-3  # it moved


def test_reference_forms_differ_and_decay_comes_before_the_update():
    """Guards the test above against a reference that ignores its flags."""
    rng = np.random.default_rng(2)
    p, g = rng.standard_normal(100), rng.standard_normal(100)
    z = np.zeros(100)
    kw = dict(**HP, bc1=0.1, bc2s=np.sqrt(0.001), wd=0.1, decay_mul=1 - 1e-3 * 0.1, bound=False)
    a, _ = adamref.step64(p, g, z, z, decoupled=True, **kw)
    b, _ = adamref.step64(p, g, z, z, decoupled=False, **kw)
    c, _ = adamref.step64(p, g, z, z, decoupled=False, **dict(kw, wd=0.0))
    assert np.array_equal(a["m"], c["m"]) and not np.array_equal(a["p"], c["p"])
    assert not np.array_equal(b["m"], c["m"])
    assert np.allclose(a["p"] - c["p"], -1e-4 * p, rtol=1e-9, atol=0)


def test_bound_is_a_few_ulps_and_zero_state_is_exact():
    rng = np.random.default_rng(3)
    n = 64
    p, g = rng.standard_normal(n), rng.standard_normal(n)
    m, v = rng.standard_normal(n) * 1e-2, rng.standard_normal(n) ** 2 * 1e-3
    hp = adamref.kernel_hp(**HP, step=10, weight_decay=0.01, ema_decay=0.999)
    out, bnd = adamref.step64(p, g, m, v, p, scale=0.5, **hp)
    for k in ("p", "m", "v", "ema"):
        rel = bnd[k] / np.abs(out[k])
        assert (rel > adamref.U / 2).all() and (rel < 64 * adamref.U).all(), (k, rel.max())
    z = np.zeros(n)
    out, bnd = adamref.step64(z, z, z, z, z, **hp)
    for k in ("p", "m", "v", "ema"):
        assert not out[k].any() and bnd[k].max() < 1e-20, k


# --- the C ABI ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from smer_music_generation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ptr():
    """A 16-byte aligned dummy address inside a live host buffer (never dereferenced)."""
    return (ctypes.addressof(_HOST_BUF) + 15) & ~15


def test_header_signature_and_library_hold_the_name(lib):
    from smer_music_generation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smer_hip.h")).read()
    assert "smer_adam_ex" in set(re.findall(r"\b(smer_[a-z0-9_]+)\(", hdr))
    assert "smer_adam_ex" in _lib.SIGNATURES and hasattr(lib, "smer_adam_ex")
    assert "smer_adam_ex" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_adam_ex_statuses_before_any_launch(lib, ptr):
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03)
    tail = (None, 0.01, 1.0, 1, None, 0.0, None)  # ctl, wd, decay_mul, decoupled, ema, ema_decay, stream
    for k in range(4):  # p, g, m, v
        a = [ptr] * 4
        a[k] = None
        assert lib.smer_adam_ex(16, *a, None, *hp, *tail) == INVALID
        assert b"smer_adam_ex" in lib.smer_last_error()
    assert lib.smer_adam_ex(-1, ptr, ptr, ptr, ptr, None, *hp, *tail) == INVALID
    for bad in (float("nan"), float("inf"), -float("inf")):
        for slot in (1, 2, 5):  # wd, decay_mul, ema_decay
            t = list(tail)
            t[slot] = bad
            assert lib.smer_adam_ex(16, ptr, ptr, ptr, ptr, None, *hp, *t) == INVALID, (bad, slot)
            assert b"finite" in lib.smer_last_error()
    assert lib.smer_adam_ex(16, ptr + 2, ptr, ptr, ptr, None, *hp, *tail) == INVALID  # not 4-B aligned
    # nothing to do, nothing launched: with and without a control block and an average
    assert lib.smer_adam_ex(0, ptr, ptr, ptr, ptr, None, *hp, *tail) == 0
    assert lib.smer_adam_ex(0, ptr + 4, ptr, ptr + 8, ptr, ptr, *hp, ptr, 0.0, 1.0, 0, ptr, 0.9, None) == 0


# --- FusedAdam ---------------------------------------------------------------
def _torch_opt_after_steps(model, cls, n=2, **kw):
    params = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    opt = cls(params, lr=1e-4, **kw)
    g = torch.Generator().manual_seed(0)
    for _ in range(n):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return params, opt


def test_adamw_state_roundtrips_through_fused_trainer():
    from smer_music_generation_amd.train import Trainer
    m, v = build("cpu")
    _, opt = _torch_opt_after_steps(m, torch.optim.AdamW, weight_decay=0.01)
    tr = Trainer(m, v)
    g0 = tr.optimizer.param_groups[0]
    assert g0["weight_decay"] == 0 and g0["decoupled_weight_decay"] is True
    tr.load_state_dict(opt.state_dict())
    assert g0["weight_decay"] == 0.01 and g0["decoupled_weight_decay"] is True and tr.t == 2
    sd = tr.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.01
    assert sd["param_groups"][0]["decoupled_weight_decay"] is True
    params2 = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    opt2 = torch.optim.AdamW(params2, lr=1.0, weight_decay=0.5)
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["weight_decay"] == 0.01 and opt2.param_groups[0]["lr"] == 1e-4
    for p1, p2 in zip(opt.param_groups[0]["params"], params2):
        a, b = opt.state[p1], opt2.state[p2]
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
        assert float(a["step"]) == float(b["step"]) == 2.0


def test_coupled_adam_state_loads_as_coupled_and_bad_groups_raise():
    from smer_music_generation_amd.train import Trainer
    m, v = build("cpu")
    _, opt = _torch_opt_after_steps(m, torch.optim.Adam, weight_decay=0.02)
    tr = Trainer(m, v, weight_decay=0.3)  # decoupled by default, overwritten by the load
    sd = opt.state_dict()
    tr.load_state_dict(sd)
    g0 = tr.optimizer.param_groups[0]
    assert g0["weight_decay"] == 0.02 and g0["decoupled_weight_decay"] is False
    sd["param_groups"][0].pop("decoupled_weight_decay", None)  # a checkpoint of an older torch
    tr2 = Trainer(m, v)
    tr2.load_state_dict(sd)
    assert tr2.optimizer.param_groups[0]["decoupled_weight_decay"] is False
    _, ams = _torch_opt_after_steps(m, torch.optim.AdamW, weight_decay=0.01, amsgrad=True)
    with pytest.raises(ValueError):
        tr.load_state_dict(ams.state_dict())
    _, mx = _torch_opt_after_steps(m, torch.optim.AdamW, weight_decay=0.01, maximize=True)
    with pytest.raises(ValueError):
        tr.load_state_dict(mx.state_dict())
    for bad in (-0.1, float("nan"), float("inf")):
        sd["param_groups"][0]["weight_decay"] = bad
        with pytest.raises(ValueError):
            tr.load_state_dict(sd)


# --- Trainer arguments -------------------------------------------------------
@pytest.mark.parametrize("good", [None, 0, 0.0, 0.5, 0.9999, np.float32(0.99)])
def test_check_ema_decay_accepts(good):
    from smer_music_generation_amd.train import check_ema_decay
    got = check_ema_decay(good)
    assert got is None if good is None else (isinstance(got, float) and got == float(good))


@pytest.mark.parametrize("bad", [1.0, -0.1, float("nan"), 1.5, float("inf"), "0.9", [0.9], True])
def test_check_ema_decay_refuses(bad):
    from smer_music_generation_amd.train import Trainer, check_ema_decay
    with pytest.raises(ValueError):
        check_ema_decay(bad)
    with pytest.raises(ValueError):
        Trainer(None, None, ema_decay=bad)  # refused before the model is touched


def test_trainer_keeps_weight_decay_in_the_param_group_and_the_average_lazily():
    from smer_music_generation_amd.train import Trainer
    m, v = build("cpu")
    with pytest.raises(ValueError):
        Trainer(m, v, weight_decay=-1.0)
    tr = Trainer(m, v, weight_decay=0.05, decoupled_weight_decay=False)
    g0 = tr.optimizer.param_groups[0]
    assert g0["weight_decay"] == 0.05 and g0["decoupled_weight_decay"] is False
    assert tr.ema is None and tr.ema_decay is None
    with pytest.raises(RuntimeError):
        tr.ema_state_dict()
    with pytest.raises(RuntimeError):
        with tr.ema_weights():
            pass
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            tr.ema_decay = bad
    assert tr.ema is None
    tr.ema_decay = 0.9
    flat = m.flat_parameters().detach()
    assert tr.ema_decay == 0.9 and tr.ema.shape == flat.shape and tr.ema.dtype == torch.float32
    assert torch.equal(tr.ema, flat) and tr.ema.data_ptr() != flat.data_ptr()
    tr.ema_decay = None  # the buffer stays, it just stops following
    assert tr.ema is not None


def test_ema_state_dict_and_swap_on_the_host():
    """The parts of the EMA access that need no kernel: the state dict's
    format and round trip, the exchange and its undoing on an exception."""
    from smer_music_generation_amd.train import Trainer
    m, v = build("cpu")
    tr = Trainer(m, v, ema_decay=0.5)
    orig = m.flat_parameters().detach().clone()
    tr.ema.mul_(2.0)  # an average that differs from the weights
    avg = tr.ema.clone()
    sd = tr.ema_state_dict()
    assert list(sd.keys()) == list(m.state_dict().keys())
    for name, p in m.named_parameters():
        assert torch.equal(sd[name], 2.0 * p.detach()), name
    assert torch.equal(sd["pos_enc.pe"], m.state_dict()["pos_enc.pe"])
    with pytest.raises(KeyError):
        with tr.ema_weights():
            assert torch.equal(m.flat_parameters().detach(), avg) and torch.equal(tr.ema, orig)
            with pytest.raises(RuntimeError):
                tr.step({})
            inside = tr.ema_state_dict()  # still the average
            assert all(torch.equal(inside[k], sd[k]) for k in sd)
            raise KeyError("leaves the context")
    assert torch.equal(m.flat_parameters().detach(), orig) and torch.equal(tr.ema, avg)
    tr2 = Trainer(m, v)
    tr2.load_ema_state_dict(sd)
    assert tr2.ema_decay is None and torch.equal(tr2.ema, avg)
    with pytest.raises(ValueError):
        tr2.load_ema_state_dict({k: t for k, t in sd.items() if not k.startswith("embedding.")})

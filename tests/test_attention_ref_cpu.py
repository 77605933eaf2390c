"""tests/attnref.py checked on the CPU: attn_ref64 against float64
torch.autograd, and the bf16 bound constants (ATTN_REL_*, ATTN_ABS_LSE)
derived from attn_emulated alone: over every shape, mask set and dropout rate
that tests/test_attention_edges_gpu.py runs, the worst
|attn_emulated - attn_ref64| / (T + |ref|) per output (T: the summed term
magnitudes of attnref's docstring; lse: absolute) must stay within a quarter
of its constant, and the constant may not be more than 1.5 times wider than
that rule gives.  No kernel output enters these numbers."""
import math

import pytest
import torch

from tests import attnref as A
from tests.hashref import attn_scale

BF16 = torch.bfloat16


def _runs(shape):
    B, H, Lq, Lk, D, causal = shape
    for kinds in A.mask_sets(B, Lk):
        for p in (0.0,) + tuple(A.drop_rates(*shape)):
            yield tuple(kinds), p


def _autograd(q, k, v, do, B, H, Lq, Lk, D, kpm, causal, scale, keep, dsc, has):
    """softmax attention through torch.autograd in float64.  Queries without
    a visible key (excluded: torch gives NaN there) see every key instead and
    get a zero dO, so they reach no gradient."""
    scale, dsc = A.f32r(scale), A.f32r(dsc)
    qh, kh, vh = (A._heads(t, B, L, H, D).clone().requires_grad_(True) for t, L in ((q, Lq), (k, Lk), (v, Lk)))
    doh = A._heads(do, B, Lq, H, D) * has.unsqueeze(-1)
    vis = A.visible(B, Lq, Lk, kpm, causal) | ~has.unsqueeze(-1)
    s = (qh @ kh.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, -math.inf)
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep.double() * dsc
    o = pr @ vh
    o.backward(doh)
    return A._rows(o.detach()), torch.logsumexp(s.detach(), -1), A._rows(qh.grad), A._rows(kh.grad), A._rows(vh.grad)


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("shape", A.SHAPES, ids=A.shape_id)
def test_ref64_matches_autograd(shape):
    B, H, Lq, Lk, D, causal = shape
    q, k, v, do = A.inputs(shape, BF16)
    for kinds, p in _runs(shape):
        kpm = A.make_kpm(kinds, Lk)
        keep = A.keep_mask(shape, p) if p else None
        r = A.reference(shape, kinds, BF16, p)
        o, lse, dq, dk, dv = _autograd(q, k, v, do, B, H, Lq, Lk, D, kpm, causal, A.scale_of(D), keep,
                                       attn_scale(p), r.has)
        hq = r.has.permute(0, 2, 1).reshape(B * Lq, H, 1).expand(B * Lq, H, D).reshape(B * Lq, H * D)
        assert _rel(r.O * hq, o * hq) < 1e-12, (kinds, p)
        assert ((r.lse - lse).abs()[r.has].max().item() if r.has.any() else 0.0) < 1e-12, (kinds, p)
        for name, got, want in (("dQ", r.dQ, dq), ("dK", r.dK, dk), ("dV", r.dV, dv)):
            if want.abs().max() > 0:
                assert _rel(got, want) < 1e-12, (name, kinds, p)
            else:
                assert got.abs().max() == 0, (name, kinds, p)
        # the convention: nothing from or to a query without a visible key
        assert (r.O * (1 - hq.double())).abs().max() == 0 and (r.dQ * (1 - hq.double())).abs().max() == 0
        assert torch.isinf(r.lse[~r.has]).all()


_worst = dict(O=0.0, lse=0.0, dQ=0.0, dK=0.0, dV=0.0)
_seen = set()


@pytest.mark.parametrize("shape", A.SHAPES, ids=A.shape_id)
def test_emulation_within_quarter_of_bounds(shape):
    B, H, Lq, Lk, D, causal = shape
    q, k, v, do = A.inputs(shape, BF16)
    w = dict.fromkeys(_worst, 0.0)
    for kinds, p in _runs(shape):
        kpm = A.make_kpm(kinds, Lk)
        keep = A.keep_mask(shape, p) if p else None
        r = A.reference(shape, kinds, BF16, p)
        e = A.attn_emulated(q, k, v, do, B, H, Lq, Lk, D, kpm, causal, A.scale_of(D), keep, attn_scale(p))
        assert torch.equal(torch.isinf(e.lse), ~r.has)
        if r.has.any():
            w["lse"] = max(w["lse"], (e.lse - r.lse).abs()[r.has].max().item())
        for name, t in (("O", r.sO), ("dQ", r.sdQ), ("dK", r.sdK), ("dV", r.sdV)):
            ref, emu = getattr(r, name), getattr(e, name)
            den = t + ref.abs()
            err = (emu - ref).abs()
            assert (err[den == 0] == 0).all(), (name, kinds, p)
            w[name] = max(w[name], (err / den.clamp_min(1e-300)).max().item())
    print("worst emulation error %s: " % A.shape_id(shape) + "  ".join("%s %.6g" % kv for kv in w.items()))
    for name, const in (("O", A.ATTN_REL_O), ("lse", A.ATTN_ABS_LSE), ("dQ", A.ATTN_REL_DQ),
                        ("dK", A.ATTN_REL_DK), ("dV", A.ATTN_REL_DV)):
        assert w[name] <= const / 4, (name, w[name], const)
        _worst[name] = max(_worst[name], w[name])
    _seen.add(shape)


def test_bf16_bounds():
    """Runs after the cases above (file order): the constants are four times
    the overall worst values, as recorded in attnref.ATTN_WORST."""
    print("overall worst: " + "  ".join("%s %.6g" % kv for kv in _worst.items()))
    for name, const in (("O", A.ATTN_REL_O), ("lse", A.ATTN_ABS_LSE), ("dQ", A.ATTN_REL_DQ),
                        ("dK", A.ATTN_REL_DK), ("dV", A.ATTN_REL_DV)):
        assert const == 4 * A.ATTN_WORST[name]
        if len(_seen) == len(A.SHAPES):  # (else some of the cases above were deselected)
            assert _worst[name] <= const / 4 <= 1.5 * _worst[name], (name, _worst[name], const)


def test_mask_sets_carry_every_kind():
    for shape in A.SHAPES:
        B, Lk = shape[0], shape[3]
        sets = A.mask_sets(B, Lk)
        assert all(len(s) == B for s in sets)
        assert {kd for s in sets for kd in s} == set(A.mask_kinds(Lk))
    assert set(A.mask_kinds(200)) == set(A.MASK_KINDS)
    assert A.make_kpm(["first64"], 130)[0, :64].all() and not A.make_kpm(["first64"], 130)[0, 64:].any()

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


# ---------------------------------------------------------------- dispatch
TWO_GROUP = [s for s in A.SHAPES if s[0] * s[1] >= 256 and s[4] <= 64]


def test_shape_table_reaches_the_two_group_kernels():
    """What the shape table is there for: its B*H >= 256 shapes with D <= 64
    (drop_rates' two_group class) run the QG = 2 forward and dQ kernels and
    the KG = 2 dK/dV kernel, (64, 8, 70, 70, 128) does not; the rule flips
    between 511 and 512 blocks and between D = 64 and 128."""
    assert TWO_GROUP and all(A.drop_rates(*s) for s in TWO_GROUP)
    for s in TWO_GROUP:
        B, H, Lq, Lk, D, causal = s
        assert A.expected_fwd_plan(A.BF16, B, H, Lq, Lk, D).QG == 2, s
        b = A.expected_bwd_plan(A.BF16, B, H, Lq, Lk, D, causal=causal)
        assert b.dq.G == 2 and b.dkdv.G == 2 and b.dq.CAUSAL == b.dkdv.CAUSAL == causal, s
    assert (64, 8, 70, 70, 128, False) in A.SHAPES
    assert A.expected_fwd_plan(A.BF16, 64, 8, 70, 70, 128).QG == 1
    b = A.expected_bwd_plan(A.BF16, 64, 8, 70, 70, 128)
    assert b.dq.G == 1 and b.dkdv.G == 1
    # 511 | 512 blocks: by B*H, and by a second 128-row block
    for H, L, QG in ((511, 70, 1), (512, 70, 2), (256, 128, 1), (256, 129, 2)):
        f = A.expected_fwd_plan(A.BF16, 1, H, L, L, 64)
        assert f.QG == QG and f.grid == (-(-L // (64 * QG)), H)
        b = A.expected_bwd_plan(A.BF16, 1, H, L, 3, 64)
        # (the key side has one 128-row block: two groups from B*H = 512 on)
        assert b.dq.G == QG and b.dkdv.G == (2 if H == 512 else 1) and b.dq.grid == f.grid and b.dkdv.grid == (1, H)
    assert A.expected_fwd_plan(A.BF16, 1, 512, 70, 70, 64).QG == 2 and A.expected_fwd_plan(A.BF16, 1, 512, 70, 70, 128).QG == 1


def test_mask_and_family_rules():
    """MIN (the forward reads the keep words) exactly when a mask buffer is
    passed and (it is filled or the wave holds one group), the generator first
    exactly when it is not filled; the fp32 MFMA forward needs D = 64, no
    dropout, the alignment fact and the switch."""
    for B, QG in ((2, 1), (64, 2)):
        for drop in (False, True):
            for mask, mask_in in ((False, False), (True, False), (True, True)):
                f = A.expected_fwd_plan(A.BF16, B, 8, 70, 70, 64, drop=drop, mask=mask and drop, mask_in=mask_in and drop)
                assert f.QG == QG and f.DROP == drop
                assert f.MIN == (drop and mask and (mask_in or QG == 1))
                assert f.mask_gen == (f.MIN and not mask_in)
                b = A.expected_bwd_plan(A.BF16, B, 8, 70, 70, 64, drop=drop, mask=mask)
                assert b.dq.MSK == b.dkdv.MSK == (drop and mask) and b.dq_first and not b.delta_pass
    ok = dict(drop=False, aligned=True, f32_mfma=True)
    assert A.expected_fwd_plan(A.F32, 2, 3, 70, 130, 64, **ok).family == "f32_mfma"
    for D, change in ((32, {}), (64, dict(drop=True)), (64, dict(aligned=False)), (64, dict(f32_mfma=False))):
        f = A.expected_fwd_plan(A.F32, 2, 3, 70, 130, D, **dict(ok, **change))
        assert f.family == "f32_valu" and f.lds == 16 * 130 and f.grid == (18, 6)


def test_plan_matches_mirror(monkeypatch):
    """The library's dispatch (smer_attn_fwd_plan / smer_attn_bwd_plan: no HIP
    call, nothing launched) and the mirror agree over attnref.plan_mismatches'
    table.  Skips only where libsmer_hip.so is not built or cannot be loaded
    without a GPU; tests/test_attention_edges_gpu.py compares every call it
    launches on the device."""
    import os
    from smer_music_generation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libsmer_hip.so is not built")
    try:
        lib = L.load()
    except OSError as e:
        if torch.cuda.is_available():
            raise
        pytest.skip("libsmer_hip.so does not load without a GPU: %s" % e)

    def setenv(v):
        monkeypatch.delenv("SMER_ATTN_F32_MFMA", raising=False) if v is None else monkeypatch.setenv("SMER_ATTN_F32_MFMA", v)

    bad = A.plan_mismatches(lib, setenv)
    assert not bad, bad[:10]

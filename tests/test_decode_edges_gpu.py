"""The decode kernels (csrc/attention.hip: smer_attn_decode, _qln, _shared,
_shared_qln, _split_f32, _split_qln_f32, smer_kv_scatter, _heads;
csrc/gemm.hip: smer_linear_decode_ln, _ln_f32) against float64, per element,
at their dispatch edges.  Reference, cases, data and bounds: tests/decoderef.py
(its module docstring states the bound rule; tests/test_decode_ref_cpu.py
derives the constants and shows that the exact-input expectations follow from
the arithmetic).

Every launch: queries / pre-norm rows, weights and outputs live in buffers
wider than their data; output pads hold a sentinel that must come back bit
for bit, output interiors are prefilled with NaN; one cache slot is used by no
row and is NaN.  Key counts per case are the edges of its kernel
(decoderef.edge_nkeys): 0, 1, KPB - 1, KPB, KPB + 1, KPB * UNR - 1, KPB * UNR,
KPB * UNR + 1, 2 * KPB * UNR + 1, cap - 1, cap.  Data kinds: "parity" (peaky
random scores), "decoy" (every position past a row's key count holds a key
scoring >= 40 above its valid ones), "census" (q = 0, one-hot V: exact
integer counts), "needle" (one key 40 above the rest: the output is its V row
bit for bit).
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import decoderef as R

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16, F32 = R.BF16, R.F32
U, UB, SENT = R.U, R.UB, R.SENT
PAD = 8


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import os
    for name in R.ENV_SWITCHES:   # decoderef.variant_of mirrors the default selection
        assert name not in os.environ, name + " is set: the case labels would not describe what runs"
    from smer_music_generation_amd import _lib as L
    L.load()


def ops():
    from smer_music_generation_amd import ops as O
    return O


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def within(got, ref, bound, what):
    got, ref = got.detach().cpu().double(), ref.double()
    bound = bound.double() if torch.is_tensor(bound) else bound
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)   # (NaN fails)
    if err.numel():
        print("%s: worst error / bound = %.3g over %d elements" % (what, (err / (bound + 1e-300)).max().item(), err.numel()))
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError("%s: %d of %d elements out of bound, first at flat index %d: got %r, ref %r" % (
            what, int(bad.sum()), err.numel(), i, got.flatten()[i].item(), ref.flatten()[i].item()))


def frame_in(data, dtype, pad=PAD):
    """Device buffer [rows, cols + pad] with NaN pads; returns (buffer, view)."""
    n, w = data.shape
    buf = torch.full((n, w + pad), float("nan"), dtype=dtype)
    buf[:, :w] = data.to(dtype)
    buf = buf.to(dev)
    return buf, buf[:, :w]


def frame_out(n, w, dtype, pad=PAD):
    buf = torch.full((n, w + pad), SENT, dtype=dtype)
    buf[:, :w] = float("nan")
    buf = buf.to(dev)
    return buf, buf[:, :w]


def pads_intact(buf, w, what):
    p = buf[:, w:].cpu()
    assert torch.equal(bits(p), bits(torch.full_like(p, SENT))), what + ": pad columns overwritten"


def qln_params(case):
    g = R._gen(case.id, "qln")
    dm, HD = case.dmodel, case.H * case.D
    gamma = (1 + 0.1 * torch.randn(dm, generator=g)).float()
    beta = (0.1 * torch.randn(dm, generator=g)).float()
    wq = (torch.randn(HD, dm, generator=g) / math.sqrt(dm)).to(case.dtype)
    bq = (0.1 * torch.randn(HD, generator=g)).float()
    return gamma, beta, wq, bq


def run(case, q, K, V, nk, req, tab, n_slots, scale, qln=None):
    """Launch the case's entry point.  q: queries [rows, H*D] (direct
    entries) or None; qln = (y, gamma, beta, wq, bq) for the prologue entries.
    Returns (O or partial records on the CPU, x_out or None)."""
    O = ops()
    lay = R.make_layout(case, n_slots)
    kc, vc = R.pack_cache(K, V, lay, case.dtype)
    kcd = kc.to(dev)
    vcd = kcd[lay.v_off:] if lay.kind == "head" else vc.to(dev)
    n, HD = len(nk), case.H * case.D
    nkd, reqd = torch.from_numpy(nk).to(dev), torch.from_numpy(req).to(dev)
    kw = dict(H=case.H, D=case.D, row_stride=lay.row_stride, req_stride=lay.req_stride,
              head_stride=lay.head_stride if lay.kind == "head" else 0, scale=scale)
    split = case.entry.startswith("split")
    if split:
        out = torch.full((n, case.H, R.DEC_SPLITS, 4 + case.D), float("nan"), device=dev)
        obuf = None
    else:
        obuf, out = frame_out(n, HD, case.dtype)
    xbuf = xo = None
    if qln is not None:
        y, gamma, beta, wq, bq = qln
        _, yv = frame_in(y, case.dtype)
        _, wv = frame_in(wq, case.dtype)
        xbuf, xo = frame_out(n, case.dmodel, case.dtype)
        args = (yv, gamma.to(dev), beta.to(dev), wv, bq.to(dev), kcd, vcd, reqd, nkd)
        if case.entry == "qln":
            O.attn_decode_qln(*args, out, x_out=xo, **kw)
        elif case.entry == "shared_qln":
            O.attn_decode_shared_qln(*args, torch.from_numpy(tab).to(dev), out, x_out=xo, **kw)
        else:
            O.attn_decode_split_qln_f32(*args, out, x_out=xo, **kw)
    else:
        _, qv = frame_in(q, case.dtype)
        if case.entry == "decode":
            O.attn_decode(qv, kcd, vcd, reqd, nkd, out, **kw)
        elif case.entry == "shared":
            O.attn_decode_shared(qv, kcd, vcd, reqd, nkd, torch.from_numpy(tab).to(dev), out, **kw)
        else:
            O.attn_decode_split_f32(qv, kcd, vcd, reqd, nkd, out, **kw)
    torch.cuda.synchronize()
    if obuf is not None:
        pads_intact(obuf, HD, case.id + " O")
    if xbuf is not None:
        pads_intact(xbuf, case.dmodel, case.id + " x_out")
    return out.cpu(), (xo.cpu() if xo is not None else None), (kc, vc, lay)


def check_split_records(case, part, q, kc, vc, nk, req, lay, scale):
    """Every (row, head, slice) record {m, l, acc} against the float64 partial
    of the slice's key range; a slice with no key is {-inf, 0, 0}."""
    n, H, D = len(nk), case.H, case.D
    for z in range(R.DEC_SPLITS):
        lo = np.array([R.split_chunks(int(x))[z][0] for x in nk])
        hi = np.array([R.split_chunks(int(x))[z][1] for x in nk])
        rz = R.decode_attn_ref64(q, kc, vc, req, hi, lay, scale, lo=lo)
        m, l, acc = part[:, :, z, 0].double(), part[:, :, z, 1].double(), part[:, :, z, 4:].double().reshape(n, H * D)
        empty = torch.from_numpy(hi <= lo).view(n, 1).expand(n, H)
        assert (m[empty] == -math.inf).all() and (l[empty] == 0).all(), "empty slice record"
        assert (acc[empty.repeat_interleave(D, 1)] == 0).all(), "empty slice acc"
        ms = torch.where(empty, torch.zeros_like(m), m)
        within(ms, torch.where(empty, torch.zeros_like(m), rz.m), (D + 2) * U * rz.S + 1e-300, "%s slice %d m" % (case.id, z))
        sh = torch.where(empty, torch.zeros_like(m), torch.exp(rz.m - ms))   # float64 partial relative to the kernel's m
        cnt = torch.from_numpy(hi - lo).double().view(n, 1)
        E = (D + 2) * rz.S + 1.25 * rz.X + 2 * (cnt / 32 + 4)
        within(l, rz.l * sh, (cnt + 2 + E) * U * rz.l * sh, "%s slice %d l" % (case.id, z))
        within(acc, rz.acc * sh.repeat_interleave(D, 1),
               ((cnt + D + 2 + E) * U).repeat_interleave(D, 1) * rz.Tacc * sh.repeat_interleave(D, 1),
               "%s slice %d acc" % (case.id, z))


def launch_data(case, kind):
    nk, req, tab, live, n_slots = R.rows_of(case)
    n = len(nk)
    qln = None
    if case.dmodel:
        gamma, beta, wq, bq = qln_params(case)
        g = R._gen(case.id, "y", kind)
        y = torch.randn(n, case.dmodel, generator=g).to(case.dtype)
        if kind == "decoy":
            y = y[:1].repeat(n, 1)
        if kind == "census":
            wq, bq = torch.zeros_like(wq), torch.zeros_like(bq)
        qln = (y, gamma, beta, wq, bq)
        xe, qe = R.emulate_qln(y, gamma, beta, 1e-5, wq, bq, case.H, case.D, case.dtype, nk)
        qfull = R.emulate_qln(y, gamma, beta, 1e-5, wq, bq, case.H, case.D, case.dtype, np.full(n, 2))[1]
    if kind == "parity":
        q, K, V, scale = R.data_parity(case, n_slots, n)
    elif kind == "decoy":
        q, K, V, scale = R.data_decoy(case, n_slots, n, nk, q=qfull if case.dmodel else None)
    else:
        q, K, V, scale = R.data_census(case, n_slots, n)
    if case.dmodel:
        q = qe   # the reference is evaluated at the emulated (bf16-rounded) query
    return SimpleNamespace(nk=nk, req=req, tab=tab, live=live, n_slots=n_slots, q=q.to(case.dtype) if not case.dmodel else q,
                           K=K, V=V, scale=scale, qln=qln)


@pytest.mark.parametrize("kind", ["parity", "decoy", "census"])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_decode_attention_edges(case, kind):
    """(a), (b), (c decoy / census): every element of O (the merged records
    for the split entries, and each record itself) within the bound of
    decoderef; x_out within the float64 LayerNorm bound; rows of no group
    (shared entries) keep their NaN prefill."""
    d = launch_data(case, kind)
    assert launch_variant(case, len(d.nk), 0 if d.tab is None else len(d.tab)).label == case.label
    out, xo, (kc, vc, lay) = run(case, None if case.dmodel else d.q, d.K, d.V, d.nk, d.req, d.tab, d.n_slots, d.scale, d.qln)
    n = len(d.nk)
    qref = d.q.float()
    if case.entry.startswith("split"):
        check_split_records(case, out, qref, kc, vc, d.nk, d.req, lay, d.scale)
        out = R.split_merge_ref64(out).view(n, -1)
    lv = torch.from_numpy(d.live)
    assert torch.isnan(out[~lv].float()).all(), "rows of no group were written"
    if kind == "census":
        want = R.census_expected(case, d.nk)
        within(out[lv], want[lv], R.census_bound(want, case.dtype)[lv], case.id + " census O")
    else:
        ref = R.decode_attn_ref64(qref, kc, vc, d.req, d.nk, lay, d.scale)
        within(out[lv], ref.O[lv], R.o_bound(case, ref, d.nk)[lv], "%s %s O" % (case.id, kind))
    if xo is not None:
        y, gamma, beta = d.qln[:3]
        xr, xb = R.ln_ref64(y, gamma, beta)
        if case.dtype == BF16:
            xb = xb + UB * xr.abs()
        if case.entry == "shared_qln":   # rows of no group: not normalised
            assert torch.isnan(xo[~lv].float()).all()
        within(xo[lv], xr[lv], xb[lv], case.id + " x_out")


def launch_variant(case, n_rows, n_groups=0):
    """The mirror's variant of a launch of `n_rows` rows of the case, asserted
    equal to the library's own plan for it (nothing is launched)."""
    q = R.case_query(case, n_rows, PAD)[:12] + (n_groups,)
    from smer_music_generation_amd import _lib as L
    m, l = R.variant_of(*q), R.library_variant(L.load(), *q)
    assert m == l, (case.id, n_rows, m, l)
    return m


def test_plan_matches_mirror(monkeypatch):
    """decoderef.plan_mismatches on the device's library: every case and the
    whole query grid, at the defaults and with each switch off."""
    from smer_music_generation_amd import _lib as L

    def setenv(env):
        for k in R.ENV_SWITCHES:
            monkeypatch.setenv(k, env[k]) if k in env else monkeypatch.delenv(k, raising=False)

    bad = R.plan_mismatches(L.load(), setenv, skln_process=True)
    assert not bad, bad[:10]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_decode_attention_needle(case):
    """(c needle) in every case: at every edge key count, with the needle at
    0, nk - 1 and every key of the last key step (the first and last key of
    every lane group, wave and unroll slot), the output row is V[p] bit for
    bit.  The prologue entries form the row's query from a one-hot y row
    (decoderef.needle_launch); every launch reaches the case's instantiation."""
    for nk in [x for x in R.edge_nkeys(case) if x > 0]:
        pos = R.needle_positions(case, nk)
        for b in range(0, len(pos), R.needle_rows(case)):
            pp = pos[b:b + R.needle_rows(case)]
            d = R.needle_launch(case, nk, pp)
            n = len(d.req)
            nkv = np.full(n, nk, np.int32)
            tab = d.tab if case.entry in ("shared", "shared_qln") else None
            assert launch_variant(case, n, 0 if tab is None else len(tab)).label == case.label, (case.id, n)
            out, _, _ = run(case, d.q, d.K, d.V, nkv, d.req, tab, 3, d.scale, d.qln)
            if case.entry.startswith("split"):
                out = R.split_merge_ref64(out).view(n, -1).float()
            assert torch.equal(bits(out.to(case.dtype)), bits(d.want.to(case.dtype))), (case.id, nk, pp)


# ------------------------------------------- (b) merge + Linear against float64
@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("N", [512, 309])
def test_linear_decode_merge_f32(H, N):
    """smer_linear_decode_merge_f32 against float64 (decoderef.merge_linear_bound:
    merge the records, Linear, bias, residual) at M = 1, 2, 16, 17, 64; records
    with slices of no key, one (row, head) with no key at all (O = 0), NaN in
    the records' pad floats, a strided weight and residual, a framed output."""
    O = ops()
    K = 64 * H
    for M in (1, 2, 16, 17, 64):
        g = torch.Generator().manual_seed(1000 * H + N + M)
        part = torch.full((M, H, R.DEC_SPLITS, 68), float("nan"))
        part[..., 0] = torch.randn(M, H, R.DEC_SPLITS, generator=g) * 4
        part[..., 1] = torch.rand(M, H, R.DEC_SPLITS, generator=g) * 20 + 0.5
        part[..., 4:] = torch.randn(M, H, R.DEC_SPLITS, 64, generator=g) * part[..., 1:2]
        empty = torch.rand(M, H, R.DEC_SPLITS, generator=g) < 0.3
        empty[M - 1, H - 1] = True   # a (row, head) without any key
        part[..., 0][empty], part[..., 1][empty] = -math.inf, 0.0
        part[..., 4:][empty] = 0.0
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        use_res = M != 2
        _, wv = frame_in(w, F32)
        rv = frame_in(res, F32)[1] if use_res else None
        cbuf, c = frame_out(M, N, F32)
        O.linear_decode_merge_f32(part.to(dev), wv, bias.to(dev), M=M, residual=rv, out=c)
        torch.cuda.synchronize()
        what = "merge_f32 M%d N%d K%d" % (M, N, K)
        pads_intact(cbuf, N, what)
        ref, bound = R.merge_linear_bound(part, w, bias, res if use_res else None)
        within(c, ref, bound, what)


# ------------------------------------------------------------- (d) scatter
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_kv_scatter_whole_cache(dtype):
    """smer_kv_scatter and _heads: the whole cache equals the expectation,
    element for element (written and untouched); repeated slots, first and
    last position, a strided source, n_rows = 0."""
    O = ops()
    g = torch.Generator().manual_seed(11)
    Rq, cap, H, D = 3, 40, 3, 32
    width = H * D
    rows = [(0, 0), (0, cap - 1), (2, 0), (2, 17), (0, 5), (1, cap - 1), (2, cap - 1)]
    req = np.array([r for r, _ in rows], np.int32)
    pos = np.array([p for _, p in rows], np.int32)
    n = len(rows)
    sent = (torch.arange(Rq * cap * (width + PAD)) % 251 - 125).to(dtype)
    src_buf, src = frame_in(torch.randn(n, width, generator=g), dtype, pad=24)
    for nr in (n, 0):
        cache = sent.clone().view(Rq, cap, width + PAD).to(dev)
        O.kv_scatter(src[:nr], cache, torch.from_numpy(req[:nr]).to(dev), torch.from_numpy(pos[:nr]).to(dev),
                     row_stride=width + PAD, req_stride=cap * (width + PAD))
        torch.cuda.synchronize()
        want = sent.clone().view(Rq, cap, width + PAD)
        for i in range(nr):
            want[req[i], pos[i], :width] = src[i].cpu()
        assert torch.equal(bits(cache), bits(want)), "kv_scatter, %d rows" % nr
    sent2 = (torch.arange(Rq * 2 * H * cap * D) % 251 - 125).to(dtype)
    src_buf, src = frame_in(torch.randn(n, 2 * width, generator=g), dtype, pad=24)
    for nr in (n, 0):
        cache = sent2.clone().view(Rq, 2, H, cap, D).to(dev)
        O.kv_scatter_heads(src[:nr], cache, torch.from_numpy(req[:nr]).to(dev), torch.from_numpy(pos[:nr]).to(dev),
                           H=H, D=D, req_stride=2 * H * cap * D, kv_stride=H * cap * D, head_stride=cap * D)
        torch.cuda.synchronize()
        want = sent2.clone().view(Rq, 2, H, cap, D)
        for i in range(nr):
            want[req[i], :, :, pos[i]] = src[i].cpu().view(2, H, D)
        assert torch.equal(bits(cache), bits(want)), "kv_scatter_heads, %d rows" % nr


# --------------------------------------------------- (e) LN-prologue Linear
def _ln_linear(dtype, M, N, K, epi, seed):
    O = ops()
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(dtype)
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).float()
    beta = (0.1 * torch.randn(K, generator=g)).float()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    bias = torch.randn(N, generator=g).float()
    res = torch.randn(M, N, generator=g).to(dtype) if epi == "residual" else None
    _, yv = frame_in(y, dtype)
    _, wv = frame_in(w, dtype)
    xbuf, xo = frame_out(M, K, dtype)
    f32out = epi == "f32out" or dtype == F32
    cbuf, c = frame_out(M, N, F32 if f32out else dtype)
    kw = {}
    Rq, cap = 3, 128   # one (slot, position) per row
    if epi.startswith("kv"):
        col0 = 0 if epi == "kv0" else (N - 1) // 8 * 8
        wk = N - col0
        sent = (torch.arange(Rq * cap * (wk + PAD)) % 251 - 125).to(dtype)
        cache = sent.clone().view(Rq, cap, wk + PAD).to(dev)
        kreq = np.array([i % 2 for i in range(M)], np.int32)         # slot 2 untouched
        kpos = np.array([cap - 1 - i // 2 for i in range(M)], np.int32)
        kw = dict(kv=cache, kv_req=torch.from_numpy(kreq).to(dev), kv_pos=torch.from_numpy(kpos).to(dev),
                  kv_row_stride=wk + PAD, kv_req_stride=cap * (wk + PAD), kv_col0=col0)
    rv = frame_in(res, dtype)[1] if res is not None else None
    O.linear_decode_ln(yv, gamma.to(dev), beta.to(dev), wv, bias.to(dev), x_out=xo, relu=epi == "relu", residual=rv,
                       out=None if (f32out and dtype == BF16) else c, out_f32=c if (f32out and dtype == BF16) else None, **kw)
    torch.cuda.synchronize()
    what = "ln_linear %s M%d N%d K%d %s" % ("bf16" if dtype == BF16 else "f32", M, N, K, epi)
    pads_intact(xbuf, K, what + " x_out")
    pads_intact(cbuf, N, what + " C")
    xr, xb = R.ln_ref64(y, gamma, beta)
    within(xo, xr, xb + (UB * xr.abs() if dtype == BF16 else 0.0), what + " x_out")
    # the product at the LayerNorm output as the kernel rounded it (held to float64 just above)
    v, t = R.ln_linear_ref64(xo.cpu(), w, bias, epi == "relu", res)
    within(c, v, (K + 8) * U * t + (0.0 if f32out else UB * v.abs()), what + " C")
    if epi.startswith("kv"):
        want = sent.clone().view(Rq, cap, wk + PAD)
        cc = c.cpu()
        for i in range(M):   # the appended columns are the stored output's
            want[kreq[i], kpos[i], :wk] = cc[i, col0:].to(dtype)
        assert torch.equal(bits(cache), bits(want)), what + " cache"


@pytest.mark.parametrize("K", R.SKLN_K)
def test_linear_decode_ln_edges(K):
    """smer_linear_decode_ln in every instantiation (K = 512 / 1024 / 2048 the
    K-full forms, 264 and 520 the guarded ones) over M in {1, 15, 16, 17, 64,
    256} and N in {16, 24, 309, 1536}: x_out against the float64 LayerNorm,
    the product against float64 at the stored x_out, epilogues in turn."""
    from smer_music_generation_amd import _lib as L
    assert R.library_skln_label(L.load(), K, None) == R.skln_label(K)
    epis = ["plain", "relu", "residual", "kv0", "kvlast"]
    i = 0
    for M in (1, 15, 16, 17, 64, 256):
        for N in (16, 24, 309, 1536):
            epi = "f32out" if N == 309 else epis[i % len(epis)]
            i += 1
            _ln_linear(BF16, M, N, K, epi, 100 + i)


@pytest.mark.parametrize("K", [264, 1024, 2048])
def test_linear_decode_ln_f32_edges(K):
    i = 0
    for M in (1, 16, 17, 64):
        for N in (16, 309):
            i += 1
            _ln_linear(F32, M, N, K, ("plain", "relu", "residual")[i % 3], 200 + i)

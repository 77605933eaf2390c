"""Parity of the training-tail kernels (csrc/train_ops.hip and the embedding /
fp8-LayerNorm / scale kernels of csrc/norm_embed.hip) at the shapes where
their dispatch changes.

Every reference is float64 on the CPU, computed from the very bits the kernel
read (bf16 widened; scalars as the C-ABI receives them, i.e. rounded to
fp32).  Every comparison is per element, against a bound of that element:

* results that are determined exactly (casts, e4m3 bytes, amax bits, scales,
  counts, untouched padding, Adam's bf16 shadow) are compared bit for bit;
* a kernel that accumulates k terms in fp32 is held to
  (k + 2) * 2**-24 * sum(|terms|) per output (+ 2**-8 * |ref| for a bf16
  store);
* the elementwise fp32 chains (Adam, the cross entropy) are held to
  ADAM_REL_* / CE_REL_* times the summed magnitude of the element's own
  terms; each constant is four times the worst error of the same formula
  evaluated in fp32 torch on the CPU on these tests' inputs (see there).
"""
import math

import numpy as np
import pytest
import torch

from tests.hashref import drop_scale, keep_mask

pytestmark = pytest.mark.gpu

dev = "cuda"
U = 2.0 ** -24   # fp32 unit roundoff
UB = 2.0 ** -8   # bound of a bf16 store, relative
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from smer_music_generation_amd import _lib as L
    L.load()


def ops():
    from smer_music_generation_amd import ops as O
    return O


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f64(t):
    return t.detach().cpu().double()


def f32r(x):
    """A Python scalar as the C-ABI's `float` parameter holds it."""
    return float(np.float32(x))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound for every element (a zero bound asks for equality)."""
    got, ref, bound = f64(got), f64(ref), f64(bound) if torch.is_tensor(bound) else bound
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)  # (NaN fails)
    ratio = (err / (bound + 1e-300)).max().item() if err.numel() else 0.0
    print("%s: worst error / bound = %.3g over %d elements" % (what, ratio, err.numel()))
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        b = bound.flatten()[i].item() if torch.is_tensor(bound) and bound.dim() else float(bound)
        raise AssertionError("%s: %d of %d elements out of bound, first at flat index %d: got %r, "
                             "ref %r, bound %.3g" % (what, int(bad.sum()), err.numel(), i,
                                                     got.flatten()[i].item(), ref.flatten()[i].item(), b))


def assert_same_bits(got, want, what):
    g, w = bits(got), bits(want)
    if not torch.equal(g, w):
        bad = (g != w).flatten().nonzero().flatten()
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at flat index %d: %r vs %r" % (
            what, bad.numel(), g.numel(), i, got.detach().cpu().flatten()[i].item(),
            want.detach().cpu().flatten()[i].item()))


def padded(rows, cols, ld, dtype, fill, g=None, scale=1.0, shift=0.0):
    """(buffer [rows, ld] filled with `fill`, its [rows, cols] view holding
    random data) on the CPU."""
    buf = torch.full((rows, ld), fill, dtype=dtype)
    if g is not None:
        buf[:, :cols] = (torch.randn(rows, cols, generator=g) * scale + shift).to(dtype)
    return buf


def pads_intact(buf_dev, cols, fill, what):
    pad = buf_dev[:, cols:].cpu()
    assert_same_bits(pad, torch.full_like(pad, fill), what + ": pad columns")


# ------------------------------------------------------------------ 1. Adam
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
# Worst error of adam_formula in fp32 torch (CPU) against its float64
# evaluation, over every case of test_adam, relative to the summed magnitude
# of the element's terms (adam_scales), measured by fp32_chain_worst_adam():
# p 3.14e-7, m 1.51e-7, v 1.38e-7.  The kernel may contract to FMA, which the
# fp32 reference does not; four times the measured worst:
ADAM_REL_P, ADAM_REL_M, ADAM_REL_V = 4 * 3.14e-7, 4 * 1.51e-7, 4 * 1.38e-7


def adam_inputs(n, seed=11):
    g_ = gen(seed + n % 1000)
    p = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_)
    m = torch.randn(n, generator=g_) * 0.1
    v = torch.rand(n, generator=g_) * 0.1
    b = n // 8
    s1 = slice(n // 2, n // 2 + b)           # g = 0, v = 0, m != 0: den = eps
    s2 = slice(n // 2 + b, n // 2 + 2 * b)   # g = m = v = 0: p must not move
    g[s1] = 0
    v[s1] = 0
    g[s2] = 0
    v[s2] = 0
    m[s2] = 0
    return p, g, m, v, s1, s2


def adam_formula(p, g, m, v, step, dtype):
    """torch.optim.Adam's _single_tensor_adam in `dtype`, with the scalars the
    kernel receives (ops.adam rounds lr, b1, b2, eps, bc1, sqrt(bc2) to fp32)."""
    hp = ADAM_HP
    c = lambda x: torch.tensor(np.float32(x), dtype=torch.float32).to(dtype)  # noqa: E731
    lr, b1, b2, eps = c(hp["lr"]), c(hp["b1"]), c(hp["b2"]), c(hp["eps"])
    bc1, bc2s = c(1.0 - hp["b1"] ** step), c(math.sqrt(1.0 - hp["b2"] ** step))
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    one = torch.ones((), dtype=dtype)
    m1 = m + (one - b1) * (g - m)                  # exp_avg.lerp_(grad, 1 - beta1)
    v1 = v * b2 + (one - b2) * g * g               # exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
    den = v1.sqrt() / bc2s + eps
    upd = (lr / bc1) * (m1 / den)
    return p - upd, m1, v1, upd


def adam_scales(p, g, m, v, step):
    """Summed magnitude of each output's terms (float64)."""
    p1, m1, v1, upd = adam_formula(p, g, m, v, step, torch.float64)
    w1 = 1.0 - f32r(ADAM_HP["b1"])
    return f64(p).abs() + upd.abs(), f64(m).abs() + w1 * (f64(g) - f64(m)).abs(), v1


ADAM_CASES = [(n, step) for n in (1, 257, 100003, 8192 * 256 + 1000) for step in (1, 3)]


def fp32_chain_worst_adam():
    """The calibration of ADAM_REL_P / _M / _V (no GPU, no kernel output)."""
    worst = [0.0, 0.0, 0.0]
    for n, step in ADAM_CASES:
        p, g, m, v, _, _ = adam_inputs(n)
        ref = adam_formula(p, g, m, v, step, torch.float64)
        lo = adam_formula(p, g, m, v, step, torch.float32)
        for k, sc in enumerate(adam_scales(p, g, m, v, step)):
            e = (lo[k].double() - ref[k]).abs()
            ok = sc > 0
            assert torch.equal(e[~ok], torch.zeros_like(e[~ok]))
            if ok.any():
                worst[k] = max(worst[k], (e[ok] / sc[ok]).max().item())
    return worst


def _run_adam(n, step, shadow):
    O = ops()
    p0, g, m0, v0, s1, s2 = adam_inputs(n)
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    pb = torch.full((n,), 3.0, device=dev, dtype=BF16) if shadow else None
    O.adam(p, g.to(dev), m, v, pb, step=step, **ADAM_HP)
    torch.cuda.synchronize()
    pr, mr, vr, _ = adam_formula(p0, g, m0, v0, step, torch.float64)
    ps, ms, vs = adam_scales(p0, g, m0, v0, step)
    assert_within(p, pr, ADAM_REL_P * ps, "adam p")
    assert_within(m, mr, ADAM_REL_M * ms, "adam m")
    assert_within(v, vr, ADAM_REL_V * vs, "adam v")
    if n >= 16:
        assert_same_bits(p[s2], p0[s2], "adam: p where g = m = v = 0")
        assert torch.equal(v[s1].cpu(), torch.zeros(s1.stop - s1.start))
        assert torch.equal(m[s2].cpu(), torch.zeros(s2.stop - s2.start))
    if shadow:
        assert_same_bits(pb, p.to(BF16), "adam: bf16 shadow of p")


@pytest.mark.parametrize("n,step", ADAM_CASES)
def test_adam(n, step):
    """n = 8192 * 256 + 1000 runs the grid-stride loop (the grid is capped at
    8192 blocks); step 1 has bc1 = 1 - b1; the g = v = 0 block divides by eps."""
    _run_adam(n, step, True)


def test_adam_without_bf16_shadow():
    _run_adam(100003, 3, False)


# ------------------------------------------------------- 2. cast and cast2d
def _f32_specials():
    tie_even_nb, tie_odd_nb = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8   # halfway: to 1 (even) / to 1 + 2**-6
    fmax = float(np.finfo(np.float32).max)                        # rounds to inf in bf16
    vals = [0.0, -0.0, math.inf, -math.inf, math.nan, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149),
            float(np.float32(1.1754942e-38)), 2.0 ** -126, tie_even_nb, tie_odd_nb, -tie_even_nb,
            -tie_odd_nb, fmax, -fmax, 2.0 ** -133 * 1.5, 2.0 ** -134,   # ties among bf16 denormals
            3.3895314e38, 1.0, -1.0, 65504.0, 1e-3]
    t = torch.tensor(vals, dtype=F32)
    up = torch.nextafter(t, torch.full_like(t, math.inf))
    dn = torch.nextafter(t, torch.full_like(t, -math.inf))
    return torch.cat([t, up, dn])


def _bf16_specials():
    raw = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x8001, 0x007F, 0x0080, 0x7F7F, 0xFF7F,
           0x3F80, 0x3F81, 0xBF80, 0x4049]
    return torch.from_numpy(np.array(raw, dtype=np.uint16).view(np.int16)).view(BF16)


def cast_source(n, dtype, seed):
    g_ = gen(seed)
    x = (torch.randn(n, generator=g_) * torch.exp(torch.randn(n, generator=g_) * 8)).to(dtype)
    sp = _f32_specials() if dtype == F32 else _bf16_specials()
    if n == 1:
        x[0] = 1 + 3 * 2.0 ** -8 if dtype == F32 else sp[13]
        return x
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    x[n - k:] = sp[:k].flip(0)          # the tail of the last pass
    if n > 8192 * 256 + k:
        x[8192 * 256:8192 * 256 + k] = sp[:k]   # first elements of the second grid-stride pass
    return x


def assert_cast_equal(got, src_cpu, what):
    want = src_cpu.to(got.dtype)   # torch's CPU cast: nearest-even, NaN kept NaN
    got = got.detach().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what + ": NaN positions"
    assert_same_bits(got[~nan], want[~nan], what)


@pytest.mark.parametrize("n", [1, 8192 * 256 + 77])
@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)])
def test_cast(src, dst, n):
    """All four dtype pairs, one element and the grid-stride loop; +-0, +-inf,
    NaN, denormals, bf16 ties to an even and to an odd neighbour, the largest
    finite fp32 (-> inf in bf16), each also one ulp up and down."""
    O = ops()
    x = cast_source(n, src, 5)
    out = torch.full((n,), 3.0, device=dev, dtype=dst)
    O.cast(x.to(dev), out)
    torch.cuda.synchronize()
    assert_cast_equal(out, x, "cast %s -> %s" % (src, dst))


@pytest.mark.parametrize("rows,cols", [(1, 1), (37, 309), (300, 1)])
@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)])
def test_cast2d(src, dst, rows, cols):
    """Views of wider buffers on both sides (lds != ldd, both > cols); the
    destination's pad columns keep their sentinel."""
    O = ops()
    lds, ldd = cols + 5, cols + 3
    sbuf = torch.full((rows, lds), math.nan, dtype=src)
    sbuf[:, :cols] = cast_source(rows * cols, src, 6).view(rows, cols)
    sdev = sbuf.to(dev)
    dbuf = torch.full((rows, ldd), -7.0, device=dev, dtype=dst)
    O.cast2d(sdev[:, :cols], dbuf[:, :cols])
    torch.cuda.synchronize()
    assert_cast_equal(dbuf[:, :cols], sbuf[:, :cols], "cast2d %s -> %s" % (src, dst))
    pads_intact(dbuf, cols, -7.0, "cast2d")


# ---------------------------------------------------------------- 3. colsum
@pytest.mark.parametrize("dtype,M,N,ld,acc,off", [
    (F32, 1, 8, 8, False, 0),          # a single row
    (F32, 77, 309, 312, True, 0),      # 16-B loader with a 5-wide tail; 16-row unroll, then 4-row tail
    (BF16, 77, 309, 312, False, 0),    # the same, bf16
    (BF16, 4096, 520, 520, True, 0),   # exactly 64 row blocks (one reduce stage), two column blocks
    (F32, 4100, 520, 528, False, 0),   # 65 row blocks: two-stage reduce, second chunk of one block
    (BF16, 200, 64, 72, True, 1),      # base one element off 16-B alignment: scalar loader
])
def test_colsum(dtype, M, N, ld, acc, off):
    O = ops()
    g_ = gen(M * 1000 + N)
    flat = torch.full((M * ld + 8,), math.nan, dtype=dtype)   # pad columns: NaN, never summed
    xcpu = flat[off:off + M * ld].view(M, ld)
    xcpu[:, :N] = (torch.randn(M, N, generator=g_) + 0.25).to(dtype)
    x = flat.to(dev)[off:off + M * ld].view(M, ld)[:, :N]
    assert (x.data_ptr() % 16 != 0) == bool(off)
    pre = torch.randn(N, generator=g_) if acc else torch.full((N,), math.nan)
    out = pre.to(dev)
    O.colsum(x, out, accumulate=acc)
    torch.cuda.synchronize()
    xr = f64(xcpu[:, :N])
    ref, mag = xr.sum(0), xr.abs().sum(0)
    k = M
    if acc:
        ref, mag, k = ref + f64(pre), mag + f64(pre).abs(), M + 1
    assert_within(out, ref, (k + 2) * U * mag, "colsum")


# ------------------------------------------------------------- 4. embed_bwd
EMB_V, EMB_ABSENT, EMB_HOT = 309, 200, 7


def _emb_ids(n, g_):
    ids = torch.randint(0, EMB_V - 1, (n,), generator=g_)
    ids[ids >= EMB_ABSENT] += 1    # EMB_ABSENT occurs in no segment
    return ids


def _emb_bwd_check(dtype, d, segs_cpu):
    """segs_cpu: [(ids, dx buffer [n, ld] or None, p, seed)]; dx = buffer[:, :d]."""
    O = ops()
    g_ = gen(d)
    scale = math.sqrt(d)
    pre = torch.randn(EMB_V, d, generator=g_)
    dt = pre.to(dev)
    segs = []
    s32 = float(np.float32(scale))
    ref = torch.zeros(EMB_V, d, dtype=torch.float64)
    mag = torch.zeros(EMB_V, d, dtype=torch.float64)
    cnt = torch.zeros(EMB_V, dtype=torch.float64)
    for ids, buf, p, seed in segs_cpu:
        if ids is None:
            segs.append((None, None, 0.0, 0))
            continue
        segs.append((ids.to(dev), buf.to(dev)[:, :d], p, seed))
        gx = f64(buf[:, :d])
        if p > 0:
            keep = torch.from_numpy(keep_mask(seed, p, ids.numel(), d))
            gx = torch.where(keep, gx * f32r(drop_scale(p)), torch.zeros_like(gx))
        ref.index_add_(0, ids, gx * s32)
        mag.index_add_(0, ids, gx.abs() * s32)
        cnt.index_add_(0, ids, torch.ones(ids.numel(), dtype=torch.float64))
    O.embed_bwd(dt, scale, segs)
    torch.cuda.synchronize()
    # k = the row's tokens + the prefill it is added to
    k = (cnt + 1)[:, None]
    assert_within(dt, f64(pre) + ref, (k + 2) * U * (mag + f64(pre).abs()), "embed_bwd dtable")
    assert cnt[EMB_ABSENT] == 0 and cnt[EMB_HOT] >= 200
    assert_same_bits(dt[EMB_ABSENT], pre[EMB_ABSENT], "embed_bwd: row of an id in no segment")


@pytest.mark.parametrize("d", [64, 768, 1024])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_embed_bwd_three_chunks(dtype, d):
    """1091 tokens = two full 512-token chunks + 67 (one full and one partial
    64-token group of wave 0); the segment boundary (700) inside a group;
    tokens 100..299 one id (fully hit groups, batches of four); dx0 strided
    with NaN pad columns, dropped at p = 0.1; dtable pre-filled; d = 1024
    fills both 16-B chunk slots of every lane, d = 64 leaves 56 lanes idle."""
    g_ = gen(100 + d)
    n0, n1 = 700, 391
    ids0, ids1 = _emb_ids(n0, g_), _emb_ids(n1, g_)
    ids0[100:300] = EMB_HOT
    dx0 = padded(n0, d, d + 8, dtype, math.nan, g_)
    dx1 = padded(n1, d, d, dtype, 0.0, g_)
    _emb_bwd_check(dtype, d, [(ids0, dx0, 0.1, 1234), (ids1, dx1, 0.0, 0)])


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_embed_bwd_missing_first_segment(dtype):
    """No first segment; 513 tokens: a second chunk of one token; the second
    segment's dropout rows count from its own first token."""
    d, n1 = 768, 513
    g_ = gen(77)
    ids1 = _emb_ids(n1, g_)
    ids1[100:310] = EMB_HOT
    dx1 = padded(n1, d, d, dtype, 0.0, g_)
    _emb_bwd_check(dtype, d, [(None, None, 0.0, 0), (ids1, dx1, 0.1, 4321)])


# ------------------------------------------------------------- 5. embed_fwd
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("d", [132, 768])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_embed_fwd_positions(dtype, d, p):
    """Explicit non-monotone positions reaching the last PE row (the decoder's
    path), out a view with ldo = d + 8; d = 132: 33 float4 per token, so a
    workgroup straddles tokens.

    Bound: e * scale + pe is two fp32 roundings (one if contracted),
    2 * 2**-24 * (|e * scale| + |pe|); a survivor of the dropout is scaled by
    ds in one more fp32 product, so with p > 0 the bound is ds times that plus
    2**-24 * |ref|; dropped elements are exactly zero; bf16 adds 2**-8 |ref|."""
    O = ops()
    g_ = gen(d + int(p * 100))
    V, n_tok, Lpe, seed = 309, 77, 100, 9
    table = torch.randn(V, d, generator=g_)
    pe = torch.randn(Lpe, d, generator=g_)
    ids = torch.randint(0, V, (n_tok,), generator=g_)
    pos = torch.randint(0, Lpe, (n_tok,), generator=g_).to(torch.int32)
    pos[5], pos[6], pos[n_tok - 1] = Lpe - 1, 0, 3
    assert pos.max().item() == Lpe - 1 and (pos[1:] < pos[:-1]).any()
    scale = math.sqrt(d)
    buf = torch.full((n_tok, d + 8), -7.0, device=dev, dtype=dtype)
    O.embed(ids.to(dev), table.to(dev), pe.to(dev), buf[:, :d], positions=pos.to(dev), scale=scale,
            drop_p=p, seed=seed)
    torch.cuda.synchronize()
    es, pp = f64(table)[ids] * f32r(scale), f64(pe)[pos.long()]
    ref, bound = es + pp, 2 * U * (es.abs() + pp.abs())
    if p > 0:
        keep = torch.from_numpy(keep_mask(seed, p, n_tok, d))
        ds = f32r(drop_scale(p))
        ref = torch.where(keep, ref * ds, torch.zeros_like(ref))
        bound = torch.where(keep, bound * ds + U * ref.abs(), torch.zeros_like(bound))
    if dtype == BF16:
        bound = bound + UB * ref.abs()
    assert_within(buf[:, :d], ref, bound, "embed_fwd")
    pads_intact(buf, d, -7.0, "embed_fwd")


# ----------------------------------------------------------- 6. weighted CE
CE_V, CE_LD, CE_GS = 309, 320, 0.37
# Worst error of ce_formula in fp32 torch (CPU) against its float64 evaluation
# over every case of test_weighted_ce, relative to the summed magnitude of the
# element's terms, measured by fp32_chain_worst_ce(): row_loss 2.70e-7,
# gradient 1.27e-6 (torch's vectorised fp32 exp is that far off on small
# probabilities).  The kernel uses the device's expf / logf and may contract
# to FMA, which the fp32 reference does not; four times the measured worst:
CE_REL_ROW, CE_REL_GRAD = 4 * 2.70e-7, 4 * 1.27e-6


def ce_inputs(R):
    g_ = gen(600 + R)
    V = CE_V
    lbuf = torch.full((R, CE_LD), math.nan)            # pad columns: NaN, must not be read
    lbuf[:, :V] = torch.randn(R, V, generator=g_) * 3
    y = torch.randint(1, V, (R,), generator=g_)
    if R >= 2:
        y[0] = 0                                       # pad target
        lbuf[1, :V] -= 1e4
    if R >= 100:
        y[3:10] = 0
        y[R - 1] = 0
        lbuf[20, :V] += 1e4
        lbuf[21, :V] -= 1e4
        col = (int(y[22]) + 5) % V                     # a single -inf off the target
        lbuf[22, col] = -math.inf
    w = torch.rand(V, generator=g_) + 0.05
    w[0] = 0
    ce_all = torch.rand(V, generator=g_) + 0.05
    denom = ce_all[y].double().sum().float().reshape(1)   # an input of smer_wce_fwd_bwd
    return lbuf, y, w, denom


def ce_formula(lbuf, y, w, denom, dtype):
    """row_loss = -w[y] log_softmax(x)[y] (0 on pad rows), grad = grad_scale *
    w[y] / denom * (softmax(x) - onehot(y)) in `dtype`; also each one's
    summed term magnitude."""
    x = lbuf[:, :CE_V].to(dtype)
    R = x.shape[0]
    wy = torch.where(y == 0, torch.zeros((), dtype=dtype), w.to(dtype)[y])
    lp = torch.log_softmax(x, dim=1)
    sm = torch.softmax(x, dim=1)
    row = wy * -lp[torch.arange(R), y]
    row = torch.where(y == 0, torch.zeros((), dtype=dtype), row)
    onehot = torch.zeros_like(x)
    onehot[torch.arange(R), y] = 1
    coef = (torch.tensor(np.float32(CE_GS)).to(dtype) * wy / denom.to(dtype))[:, None]
    grad = coef * (sm - onehot)
    # log(se) and (x[y] - max) are the row loss's two terms
    mx = x.max(dim=1).values
    lse_c = torch.log(torch.exp(x - mx[:, None]).sum(1))
    row_scale = wy * (lse_c.abs() + (x[torch.arange(R), y] - mx).abs())
    return row, grad, row_scale, coef.abs() * (sm + onehot)


CE_ROWS = [1, 2, 333]


def fp32_chain_worst_ce():
    """The calibration of CE_REL_ROW / CE_REL_GRAD (no GPU, no kernel output)."""
    worst = [0.0, 0.0]
    for R in CE_ROWS:
        lbuf, y, w, denom = ce_inputs(R)
        row, grad, rs, gs = ce_formula(lbuf, y, w, denom, torch.float64)
        row32, grad32, _, _ = ce_formula(lbuf, y, w, denom, torch.float32)
        for k, (lo, hi, sc) in enumerate(((row32, row, rs), (grad32, grad, gs))):
            e = (lo.double() - hi).abs()
            ok = sc > 0
            assert torch.equal(e[~ok], torch.zeros_like(e[~ok]))
            if ok.any():
                worst[k] = max(worst[k], (e[ok] / sc[ok]).max().item())
    return worst


@pytest.mark.parametrize("R", CE_ROWS)
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_weighted_ce(dtype, R):
    """ldl = ldd = 320 > V; R = 1, 2: a partial workgroup; pad targets; rows
    shifted by +-1e4 and a -inf logit; grad_scale = 0.37; then the same call
    without dlogits (the eval path) and without loss_out."""
    O = ops()
    V = CE_V
    lbuf, y, w, denom = ce_inputs(R)
    ldev, ydev, wdev, ddev = lbuf.to(dev), y.to(dev), w.to(dev), denom.to(dev)
    row_ref, grad_ref, row_sc, grad_sc = ce_formula(lbuf, y, w, denom, torch.float64)
    loss_ref = row_ref.sum() / denom.double()
    assert torch.isfinite(row_ref).all() and torch.isfinite(grad_ref).all()
    pad = y == 0

    def call(with_grad, with_loss):
        row = torch.full((R,), math.nan, device=dev)
        loss = torch.full((1,), math.nan, device=dev) if with_loss else None
        dl = torch.full((R, CE_LD), -7.0, device=dev, dtype=dtype) if with_grad else None
        O.wce_fwd_bwd(ldev[:, :V], ydev, wdev, ddev, row, loss, dl[:, :V] if with_grad else None,
                      V=V, grad_scale=CE_GS)
        torch.cuda.synchronize()
        return row, loss, dl

    def check(row, loss, dl, what):
        assert_within(row, row_ref, CE_REL_ROW * row_sc, what + " row_loss")
        assert torch.equal(row.cpu()[pad], torch.zeros(int(pad.sum()))), what + ": row_loss on pad rows"
        if loss is not None:
            # R row losses (each within CE_REL_ROW of its terms) summed in fp32, one division
            lb = ((R + 2) * U * row_ref.abs().sum() + CE_REL_ROW * row_sc.sum()) / denom.double() + U * loss_ref.abs()
            assert_within(loss, loss_ref, lb, what + " loss")
        if dl is not None:
            gb = CE_REL_GRAD * grad_sc + (UB * grad_ref.abs() if dtype == BF16 else 0)
            assert_within(dl[:, :V], grad_ref, gb, what + " dlogits")
            g = dl[:, :V].float().cpu()
            assert torch.equal(g[pad], torch.zeros_like(g[pad])), what + ": gradient on pad rows"
            pads_intact(dl, V, -7.0, what + " dlogits")

    row, loss, dl = call(True, True)
    check(row, loss, dl, "wce")
    row2, loss2, _ = call(False, True)
    check(row2, loss2, None, "wce without dlogits")
    assert_same_bits(row2, row, "wce without dlogits: row_loss")
    assert_same_bits(loss2, loss, "wce without dlogits: loss")
    row3, _, dl3 = call(True, False)
    check(row3, None, dl3, "wce without loss_out")
    assert_same_bits(row3, row, "wce without loss_out: row_loss")
    assert_same_bits(dl3, dl, "wce without loss_out: dlogits")


@pytest.mark.parametrize("n", [1, 255, 700])
def test_wce_denom(n):
    O = ops()
    g_ = gen(40 + n)
    y = torch.randint(0, CE_V, (n,), generator=g_)
    ce_all = torch.rand(CE_V, generator=g_) + 0.05
    denom = torch.full((1,), math.nan, device=dev)
    O.wce_denom(y.to(dev), ce_all.to(dev), denom)
    torch.cuda.synchronize()
    terms = f64(ce_all)[y]
    assert_within(denom, terms.sum().reshape(1), (n + 2) * U * terms.abs().sum(), "wce_denom")


# ----------------------------------------------------- 7. layernorm_fwd_fp8
LN_AMAX = 15.75   # scale 448 / 15.75: many products on e4m3 midpoints


def _ln_fp8_run(M, N, amax0, nan_at=None):
    from tests.test_kernels_gpu import _e4m3_ref
    O = ops()
    g_ = gen(M + N)
    ld = N + 8
    xbuf = padded(M, N, ld, BF16, math.nan, g_, 3.0, 1.0)
    if nan_at is not None:
        xbuf[nan_at[0], nan_at[1]] = math.nan
    gamma, beta = torch.randn(N, generator=g_), torch.randn(N, generator=g_)
    xdev, gdev, bdev = xbuf.to(dev), gamma.to(dev), beta.to(dev)
    ybuf = torch.full((M, ld), -7.0, device=dev, dtype=BF16)
    qbuf = torch.full((M, ld), 0xAB, device=dev, dtype=torch.uint8)
    mean = torch.full((M,), math.nan, device=dev)
    rstd = torch.full((M,), math.nan, device=dev)
    qs = torch.from_numpy(np.array([np.float32(448.0) / np.float32(LN_AMAX)], dtype=np.float32)).to(dev)
    amax = torch.tensor([amax0], dtype=torch.int32, device=dev)
    O.layernorm_fp8(xdev[:, :N], gdev, bdev, ybuf[:, :N], mean, rstd, qbuf[:, :N], qs, amax)
    # the plain bf16 LayerNorm of the same input
    y2 = torch.full((M, ld), -7.0, device=dev, dtype=BF16)
    mean2, rstd2 = torch.empty(M, device=dev), torch.empty(M, device=dev)
    O.layernorm(xdev[:, :N], gdev, bdev, y2[:, :N], mean2, rstd2)
    torch.cuda.synchronize()
    pads_intact(ybuf, N, -7.0, "layernorm_fp8 y")
    pads_intact(qbuf, N, 0xAB, "layernorm_fp8 q8")
    y = ybuf[:, :N].cpu()
    return dict(x=xbuf[:, :N], gamma=gamma, beta=beta, y=y, q8=qbuf[:, :N].cpu(), mean=mean.cpu(),
                rstd=rstd.cpu(), amax=amax.cpu(), y2=y2[:, :N].cpu(), mean2=mean2.cpu(),
                rstd2=rstd2.cpu(), q8_ref=_e4m3_ref(y, LN_AMAX))


def _float_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


@pytest.mark.parametrize("M,N", [(37, 64), (300, 520), (130, 2048), (8197, 768)])
def test_layernorm_fwd_fp8(M, N):
    """(8197, 768): 2050 row groups on a grid capped at 2048 workgroups, so
    the row loop runs a second, partial pass; N = 520 / 2048: the 2- and
    4-chunk instantiations.  y / mean / rstd are the plain LayerNorm's bits,
    the e4m3 copy is the nearest-even cast of the stored bf16 y times
    448 / 15.75, the amax slot ends as the bits of max |y|."""
    r = _ln_fp8_run(M, N, 0)
    assert_same_bits(r["y"], r["y2"], "layernorm_fp8 y vs layernorm")
    assert_same_bits(r["mean"], r["mean2"], "layernorm_fp8 mean vs layernorm")
    assert_same_bits(r["rstd"], r["rstd2"], "layernorm_fp8 rstd vs layernorm")
    # the statistics against float64: mean sums N terms; rstd = rsqrt(q / N + eps),
    # q a sum of N squares d * d (3 roundings each): (N + 2 + 3 + 2) / 2 roundings
    # through the square root, + 4 for a 2-ulp rsqrtf
    x = f64(r["x"])
    mu = x.mean(1)
    assert_within(r["mean"], mu, (N + 2) * U * x.abs().sum(1) / N, "layernorm_fp8 mean")
    rs = 1.0 / torch.sqrt(((x - mu[:, None]) ** 2).mean(1) + f32r(1e-5))
    assert_within(r["rstd"], rs, (N / 2 + 8) * U * rs, "layernorm_fp8 rstd")
    assert_same_bits(r["q8"], r["q8_ref"], "layernorm_fp8 e4m3 copy")
    ymax = r["y"].float().abs().max().item()
    assert r["amax"].item() == _float_bits(ymax)
    # a slot already above max |y| stays as it is (and the copy is the same)
    above = _float_bits(ymax * 4)
    r2 = _ln_fp8_run(M, N, above)
    assert r2["amax"].item() == above
    assert_same_bits(r2["q8"], r["q8"], "layernorm_fp8 e4m3 copy, slot above")


def test_layernorm_fwd_fp8_nan_input():
    """One NaN in x: its row of y is NaN, the amax slot reports +inf (the
    next step's scale then falls back to 1); the other rows are unaffected."""
    M, N, row = 37, 64, 17
    r = _ln_fp8_run(M, N, 0, nan_at=(row, 9))
    assert torch.isnan(r["y"][row].float()).all()
    others = torch.arange(M) != row
    assert not torch.isnan(r["y"][others].float()).any()
    assert_same_bits(r["y"][others], r["y2"][others], "layernorm_fp8 y vs layernorm")
    assert_same_bits(r["q8"][others], r["q8_ref"][others], "layernorm_fp8 e4m3 copy")
    assert r["amax"].item() == 0x7F800000


# ------------------------------------------------------------ 8. fp8_scales
def _scales_check(prev_bits):
    O = ops()
    n = prev_bits.size
    prev = torch.from_numpy(prev_bits.view(np.int32).copy()).to(dev)
    qs = torch.full((n,), math.nan, device=dev)
    inv = torch.full((n,), math.nan, device=dev)
    nxt = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    O.fp8_scales(prev, qs, inv, nxt)
    torch.cuda.synchronize()
    a = prev_bits.view(np.float32)
    with np.errstate(all="ignore"):
        ok = (a > np.float32(0)) & (a < np.float32(3.0e38))
        safe = np.where(ok, a, np.float32(1))
        want_qs = np.where(ok, np.float32(448) / safe, np.float32(1)).astype(np.float32)
        want_inv = np.where(ok, safe / np.float32(448), np.float32(1)).astype(np.float32)
    assert_same_bits(qs, torch.from_numpy(want_qs), "fp8_scales qs")
    assert_same_bits(inv, torch.from_numpy(want_inv), "fp8_scales inv")
    assert torch.equal(nxt.cpu(), torch.zeros(n, dtype=torch.int32))
    assert torch.equal(prev.cpu(), torch.from_numpy(prev_bits.view(np.int32).copy()))
    return ok


SCALE_EDGES = np.array([0.0, 1e-40, 15.75, 1e-3, 2.9e38, 3.0e38, np.inf, np.nan], dtype=np.float32)


def test_fp8_scales():
    """qs = 448 / amax and inv = amax / 448 by IEEE fp32 division; 1 and 1
    outside (0, 3.0e38): zero, the bound itself, +inf, NaN.  n = 1 per edge
    value, n = 300 (two workgroups) with the edges among random amaxes."""
    for v in SCALE_EDGES:
        ok = _scales_check(np.array([v], dtype=np.float32).view(np.uint32))
        assert bool(ok[0]) == (v in SCALE_EDGES[[1, 2, 3, 4]])
    rng = np.random.default_rng(8)
    a = np.exp(rng.standard_normal(300) * 6).astype(np.float32)
    a[:8], a[256:264], a[292:] = SCALE_EDGES, SCALE_EDGES, SCALE_EDGES
    ok = _scales_check(a.view(np.uint32))
    assert ok.sum() == 300 - 12


# ------------------------------------------------------- 9. argmax_accuracy
def test_argmax_accuracy_ties_nan_and_classes():
    """The prediction is torch.argmax's: first index among ties (across lanes,
    within a lane, lower index in the higher lane), 0 on an all -inf row, the
    first NaN when there is one.  R = 7: a full and a partial workgroup; pad
    rows are skipped, a target of class -1 counts in the total only."""
    O = ops()
    g_ = gen(90)
    V, ld, R, ncls, pad = 309, 320, 7, 3, 5
    buf = torch.full((R, ld), math.nan)
    buf[:, :V] = torch.randn(R, V, generator=g_)
    x = buf[:, :V]
    x[0, 10] = x[0, 20] = 9.0                 # tie in lanes 10 and 20
    x[1, 10] = x[1, 74] = 9.0                 # tie inside lane 10
    x[2, 65] = x[2, 3] = 9.0                  # lower index (3) in the higher lane
    x[3, :] = -math.inf                       # predicts 0
    x[4, 11] = 9.0                            # pad target: skipped
    x[5, 12] = 9.0                            # target of class -1
    x[6, 40], x[6, 200] = math.nan, 50.0      # a NaN beats the larger finite value
    y = torch.tensor([10, 74, 3, 0, pad, 12, 40])
    cls = (torch.arange(V) % ncls).to(torch.int32)
    cls[12], cls[100], cls[308] = -1, -1, -1
    pred = torch.argmax(x, dim=1)
    assert pred.tolist() == [10, 10, 3, 0, 11, 12, 40]

    def expected(rows, start):
        c = list(start)
        for r in rows:
            if int(y[r]) == pad:
                continue
            hit = int(pred[r] == y[r])
            k = int(cls[y[r]])
            if 0 <= k < ncls:
                c[2 * k] += 1
                c[2 * k + 1] += hit
            c[2 * ncls] += 1
            c[2 * ncls + 1] += hit
        return c

    xdev, ydev, cdev = buf.to(dev), y.to(dev), cls.to(dev)
    start = list(range(3, 3 + 2 * ncls + 2))   # the kernel adds to what is there
    counts = torch.tensor(start, dtype=torch.int32, device=dev)
    O.argmax_accuracy(xdev[:, :V], ydev, cdev, ncls, pad, counts)
    per_row = []
    for r in range(R):   # each row alone, to name the row that departs
        c1 = torch.zeros(2 * ncls + 2, dtype=torch.int32, device=dev)
        O.argmax_accuracy(xdev[r:r + 1, :V], ydev[r:r + 1], cdev, ncls, pad, c1)
        per_row.append(c1)
    torch.cuda.synchronize()
    names = ["tie across lanes", "tie in one lane", "lower index in higher lane", "all -inf",
             "pad target", "class -1 target", "NaN logit"]
    for r in range(R):
        assert per_row[r].tolist() == expected([r], [0] * (2 * ncls + 2)), names[r]
    assert counts.tolist() == expected(range(R), start)

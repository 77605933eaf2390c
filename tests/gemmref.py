"""float64 reference, exact input classes, frames, bounds, dispatch mirror and
shape table of the GEMM kernels (csrc/gemm.hip: smer_gemm in bf16 and fp32,
smer_gemm_wgrad_bias / _ex), and the dispatch mirror of the e4m3 products
(smer_gemm_fp8 / _q / _ex / _gate8, smer_gemm_wgrad_fp8).  Plain torch on the CPU;
tests/test_gemm_ref_cpu.py checks this file, tests/test_gemm_edges_gpu.py
holds the kernels to it.

Exact inputs.  When every product and every partial sum of an output element
is exactly representable in fp32, the result does not depend on the summation
order, on the MFMA's internal rounding, on split-K or on FMA contraction: the
kernel must return the float64 result bit for bit, at any K.  Class S holds
integers in [-8, 8]; class F holds m * 2**-7, |m| <= 255 (all eight mantissa
bits of bf16 live), each entry nonzero with probability min(1, sqrt(128 / K)).
The epilogue operands of the exact classes are integers (bias [-16, 16],
residual and Cf0 [-64, 64], gate in {-1, 0, 1}; in class F, whose products
alone come to 0.79 * 2**22 grid units, the same integers times 1/4), alpha and
gate_scale are 0.5 or 2 and drop_p = 0.5 (threshold 32768, survivor scale
exactly 2).
Precondition (asserted by the tests, `exact_units`): for every output element
sum_k |a b| + |bias| + |residual| + |Cf0|, in units of the product grid (1 for
S, 2**-14 for F), is <= 2**22, a factor of four below 2**24 for alpha, the
survivor scale and the gate scale.

Class R (randn, B scaled by 0.05, alpha 0.3, gate_scale 1.25, drop_p 0.1)
checks the scalars with full mantissas and the rounding of the store against
the any-order fp32 summation bound of the element (`r_bound`), which no kernel
output enters:
    T = ((|alpha| sum_k |a b| + |bias| + |residual|) * gate_scale + |Cf0|) * drop_scale
    bound = (K + 8) * 2**-24 * T    (+ 2**-8 |ref| for a bf16 store).

Frames.  Every operand is a view into a flat buffer (`Buf`): inputs with a row
stride beyond their width and two guard rows, pads and guards NaN (the header
promises nothing about pad contents, so a result that depends on them is a
bug); outputs with ld = N + 8, N or N + 3 and two guard rows of a sentinel
that must come back bit for bit, the interior prefilled with NaN unless the
call accumulates.
"""
import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

from tests.hashref import drop_threshold, keep_mask

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24
UB = 2.0 ** -8
EXACT_LIMIT = 2 ** 22
SENT = 123.0          # sentinel around the outputs (exact in bf16)
SEED = 4321           # dropout seed of every case
WS_BYTES = 64 << 20   # ops.SPLITK_WS_BYTES
TICKET_BYTES = 64 * 1024
DEVICE_PRODUCT_FLOP = 2e9   # above: the float64 product may be taken on the device
F_CLASS_FLOP = 0.5e9        # class F runs on the cases up to this size

# environment switches csrc/gemm.hip reads on every call
ENV_SWITCHES = ("SMER_GEMM64", "SMER_GEMM256", "SMER_GEMM256S", "SMER_G256_NONPERSIST",
                "SMER_GEMM_F32_MFMA", "SMER_SPLITK_FUSED", "SMER_WGRAD256S", "SMER_FP8_Q8_FAST",
                "SMER_GEMM256S_FP8")


def f32r(x):
    """A Python scalar as a C `float` parameter holds it."""
    return float(np.float32(x))


def drop_scale32(p):
    """csrc/common.h smer_drop_scale16 of smer_drop_thr16(float p), an fp32."""
    t = drop_threshold(f32r(p))
    return f32r(65536.0 / (65536.0 - t)) if t else 1.0


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------- reference
def epilogue64(acc, *, alpha=1.0, bias=None, relu=False, drop_p=0.0, seed=0, residual=None,
               gate=None, gate_scale=1.0, cf0=None, accumulate=False):
    """The epilogue of include/smer_hip.h in float64, in the order of
    csrc/gemm.hip epi_apply: alpha * acc, + bias, relu, dropout, + residual,
    gate.  Returns v (what C stores, rounded by the caller) and Cf =
    (accumulate ? Cf0 : 0) + v."""
    M, N = acc.shape
    v = acc.double() * f32r(alpha)
    if bias is not None:
        v = v + bias.double().view(1, N)
    if relu:
        v = v.clamp_min(0.0)
    if f32r(drop_p) > 0:
        keep = torch.from_numpy(_keep(seed, f32r(drop_p), M, N))
        v = torch.where(keep, v * drop_scale32(drop_p), torch.zeros_like(v))
    if residual is not None:
        v = v + residual.double()
    if gate is not None:
        v = torch.where(gate.double() > 0, v * f32r(gate_scale), torch.zeros_like(v))
    return v, (v + cf0.double() if accumulate else v)


@functools.lru_cache(maxsize=2)
def _keep(seed, p, M, N):
    return keep_mask(seed, p, M, N)


def to_dtype(v, dtype):
    """float64 -> fp32 (-> bf16), round to nearest even at each step, as the
    kernels round an fp32 register."""
    v = v.float()
    return v.bfloat16() if dtype == BF16 else v


# --------------------------------------------------------- epilogue sets
def _E(**kw):
    e = dict(alpha=False, bias=False, relu=False, drop=False, residual=False, gate=False,
             C=True, Cf=False, accumulate=False)
    e.update(kw)
    return SimpleNamespace(**e)


EPI = {
    "none": _E(),
    "alpha": _E(alpha=True),
    "brdr": _E(bias=True, relu=True, drop=True, residual=True),
    "gate": _E(gate=True),
    "resgate": _E(residual=True, gate=True),
    "cfacc": _E(C=False, Cf=True, accumulate=True),
    "ccf": _E(Cf=True),
    # weight gradients through smer_gemm
    "cf": _E(C=False, Cf=True),
    "cf_alpha": _E(alpha=True, C=False, Cf=True),
    "cfacc_alpha": _E(alpha=True, C=False, Cf=True, accumulate=True),
    # class R
    "full": _E(alpha=True, bias=True, relu=True, drop=True, residual=True, gate=True, Cf=True,
               accumulate=True),
    "fullc": _E(alpha=True, bias=True, relu=True, drop=True, residual=True),
    # smer_gemm_wgrad_bias_ex: dW and db, accumulate off / on
    "wb": _E(C=False, Cf=True),
    "wbacc": _E(C=False, Cf=True, accumulate=True),
}
SEVEN = ("none", "alpha", "brdr", "gate", "resgate", "cfacc", "ccf")
SHORT = ("none", "brdr", "resgate")


def scalars(epi_name, cls):
    """alpha, gate_scale, drop_p of an epilogue set in an input class."""
    e = EPI[epi_name]
    if cls == "R":
        return (0.3 if e.alpha else 1.0, 1.25 if e.gate else 1.0, 0.1 if e.drop else 0.0)
    alpha = (2.0 if epi_name == "cfacc_alpha" else 0.5) if e.alpha else 1.0
    gs = (0.5 if e.residual else 2.0) if e.gate else 1.0
    return alpha, gs, (0.5 if e.drop else 0.0)


# frames: row strides (beyond N) of C, Cf, residual, gate -- pairwise different
FRAMES = {
    "vec8": dict(ldc=8, ldcf=16, ldr=24, ldg=32),    # every stride % 8 == 0 when N % 8 == 0
    "tight": dict(ldc=0, ldcf=0, ldr=8, ldg=16),      # contiguous outputs (C and Cf are separate buffers)
    "odd": dict(ldc=3, ldcf=1, ldr=5, ldg=7),         # breaks e.vec: the scalar epilogue
    "cf4": dict(ldc=8, ldcf=4, ldr=24, ldg=32),       # lddw = N + 4: float4 rows, e.vec = 0
}


def Run(epi, frame="vec8", bias_off=0, max_wg=0, api=None):
    """One call of a case: epilogue set, frame, bias view offset (floats),
    max_workgroups, and the entry point ("gemm" or "wgrad_bias")."""
    return SimpleNamespace(epi=epi, frame=frame, bias_off=bias_off, max_wg=max_wg,
                           api=api or ("wgrad_bias" if epi in ("wb", "wbacc") else "gemm"))


def run_id(r):
    return "%s-%s%s%s" % (r.epi, r.frame, "-boff%d" % r.bias_off if r.bias_off else "",
                          "-wg%d" % r.max_wg if r.max_wg else "")


# ------------------------------------------------------------ the table
def _case(cid, dtype, lay, M, N, K, runs, env=None, a_ld=None, a_off=0, exact_cf0=True):
    ak, bk = lay[0] == "N", lay[1] == "T"   # NT: A [M,K], B [N,K]; a 'T' first / 'N' second: column image
    return SimpleNamespace(id=cid, dtype=dtype, lay=lay, ak=ak, bk=bk, M=M, N=N, K=K, runs=tuple(runs),
                           env=dict(env or {}), a_ld=a_ld, a_off=a_off, exact_cf0=exact_cf0,
                           flop=2.0 * M * N * K)


def _runs(names, extra=()):
    return [Run(n) for n in names] + list(extra)


ALL_RUNS = _runs(SEVEN, [Run("brdr", "odd"), Run("none", "tight")])
SHORT_RUNS = _runs(SHORT, [Run("brdr", "odd")])
WGRAD_RUNS = [Run("wb", "tight"), Run("wbacc", "vec8"), Run("wb", "cf4"), Run("cf", "vec8"), Run("cfacc", "tight")]
WGRAD_GEMM_RUNS = [Run("cf", "vec8"), Run("cfacc", "tight"), Run("cf", "cf4")]
ALPHA_RUNS = [Run("cf_alpha", "vec8"), Run("cfacc_alpha", "tight")]


def _table():
    t = []

    def bf(cid, lay, M, N, K, runs, **kw):
        t.append(_case(cid, BF16, lay, M, N, K, runs, **kw))

    def ff(cid, lay, M, N, K, runs, **kw):
        t.append(_case(cid, F32, lay, M, N, K, runs, **kw))

    # bf16 NT, skinny (M <= 256)
    bf("sk-1x16x32", "NT", 1, 16, 32, SHORT_RUNS)
    bf("sk-255x24x8", "NT", 255, 24, 8, SHORT_RUNS)
    bf("sk-2x309x520", "NT", 2, 309, 520, ALL_RUNS)
    bf("sk-16x512x512", "NT", 16, 512, 512, ALL_RUNS + [Run("brdr", "vec8", bias_off=1)])
    bf("sk-17x512x544", "NT", 17, 512, 544, SHORT_RUNS)
    bf("sk-80x1536x512", "NT", 80, 1536, 512, SHORT_RUNS)
    bf("sk-81x1536x512", "NT", 81, 1536, 512, ALL_RUNS)
    bf("sk-81x1536x520", "NT", 81, 1536, 520, SHORT_RUNS)   # the 64-row strip in its guarded form
    bf("sk-256x1544x2048", "NT", 256, 1544, 2048, SHORT_RUNS)
    # leaving skinny
    bf("g64-257x512x512", "NT", 257, 512, 512, ALL_RUNS)
    bf("g128-257x512x512", "NT", 257, 512, 512, ALL_RUNS, env={"SMER_GEMM64": "0"})
    bf("g128-257x512x520", "NT", 257, 512, 520, ALL_RUNS)
    for lay in ("NT", "NN", "TT", "TN"):
        bf("lay%s-200x309x136" % lay, lay, 200, 309, 136, SHORT_RUNS)
        bf("lay%s-264x136x200" % lay, lay, 264, 136, 200, SHORT_RUNS)
    # persistent grids
    bf("g64-4150x1530x64", "NT", 4150, 1530, 64, SHORT_RUNS)
    bf("g128-4150x2056x72", "NT", 4150, 2056, 72, SHORT_RUNS)
    bf("g128-4096x4096x128", "NT", 4096, 4096, 128, SHORT_RUNS, env={"SMER_GEMM256": "0", "SMER_GEMM64": "0"})
    # 256x256 two-stage
    bf("g256-4096x4096x64", "NT", 4096, 4096, 64, ALL_RUNS)
    bf("g256not-3840x4096x64", "NT", 3840, 4096, 64, SHORT_RUNS)
    bf("g256-4100x4096x128", "NT", 4100, 4096, 128, ALL_RUNS)
    bf("g256-NN-4096x4104x128", "NN", 4096, 4104, 128, SHORT_RUNS)
    bf("g256-np2-4096x4096x128", "NT", 4096, 4096, 128, SHORT_RUNS, env={"SMER_G256_NONPERSIST": "2"})
    # 256x256 staggered
    bf("g256s-NN-4096x4096x128", "NN", 4096, 4096, 128, ALL_RUNS)
    bf("g256s-NN-4096x4096x192", "NN", 4096, 4096, 192, SHORT_RUNS)
    bf("g256s-NN-4352x4096x128", "NN", 4352, 4096, 128, SHORT_RUNS)
    bf("g256s-on-4096x4096x128", "NT", 4096, 4096, 128, SHORT_RUNS, env={"SMER_GEMM256S": "1"})
    bf("g256s-4096x4096x1024", "NT", 4096, 4096, 1024, SHORT_RUNS)
    # weight gradients (TN: A = dy [K, M], B = x [K, N]), 128x128 kernel
    bf("w-200x136x96", "TN", 200, 136, 96, WGRAD_RUNS + ALPHA_RUNS)
    bf("w-8x8x2048", "TN", 8, 8, 2048, WGRAD_RUNS)
    bf("w-512x512x2056", "TN", 512, 512, 2056, WGRAD_RUNS)
    bf("w-512x512x4160", "TN", 512, 512, 4160, WGRAD_RUNS + ALPHA_RUNS +
       [Run("wb", "vec8", max_wg=w) for w in (8, 100, 1000)])
    bf("w-200x309x2048", "TN", 200, 309, 2048, WGRAD_GEMM_RUNS)
    bf("w-201x309x2048", "TN", 201, 309, 2048, WGRAD_RUNS)
    # 64 K = 2**22 already: no room for Cf0 in the exact classes
    bf("w-128x128x65536", "TN", 128, 128, 65536, [Run("wb", "vec8"), Run("cf", "tight")], exact_cf0=False)
    # weight gradients, 256x256 kernels
    bf("w256-768x768x11328", "TN", 768, 768, 11328, WGRAD_RUNS +
       [Run("wb", "vec8", max_wg=w) for w in (8, 100, 1000)])
    bf("w256-two-768x768x11328", "TN", 768, 768, 11328, WGRAD_RUNS, env={"SMER_WGRAD256S": "0"})
    bf("w256-776x768x11328", "TN", 776, 768, 11328, WGRAD_RUNS)
    bf("w256-4096x4096x64", "TN", 4096, 4096, 64, [Run("wb", "vec8"), Run("cfacc", "tight")])
    bf("w256not-1536x768x4096", "TN", 1536, 768, 4096, [Run("wb", "vec8"), Run("cfacc", "tight")])
    # SMER_SPLITK_FUSED=1 on the split cases of the 128x128 kernel
    for M, N, K in ((8, 8, 2048), (512, 512, 2056), (512, 512, 4160), (128, 128, 65536)):
        bf("wfused-%dx%dx%d" % (M, N, K), "TN", M, N, K, [Run("wb", "vec8"), Run("cf", "cf4")],
           env={"SMER_SPLITK_FUSED": "1"}, exact_cf0=K < 65536)
    # fp32
    for M, N, K in ((1, 4, 4), (2, 309, 512), (37, 100, 100), (64, 512, 2048), (64, 512, 2052), (2, 512, 4096),
                    (65, 64, 64), (200, 309, 60), (200, 309, 136), (130, 264, 1040), (200, 309, 192),
                    (200, 309, 66)):
        ff("f32-%dx%dx%d" % (M, N, K), "NT", M, N, K, ALL_RUNS if M in (37, 64, 130) or K == 66 else SHORT_RUNS)
    ff("f32-lda1-200x309x136", "NT", 200, 309, 136, SHORT_RUNS, a_ld=137)
    ff("f32-aoff-200x309x136", "NT", 200, 309, 136, SHORT_RUNS, a_off=1)
    for lay in ("NN", "TT", "TN"):
        ff("f32-%s-200x309x136" % lay, lay, 200, 309, 136, SHORT_RUNS)
    ff("f32-valu-200x309x136", "NT", 200, 309, 136, SHORT_RUNS, env={"SMER_GEMM_F32_MFMA": "0"})
    return t


CASES = _table()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# (case whose neighbour must take another kernel, the neighbour, the run)
NOT_EDGES = (("g256not-3840x4096x64", "g256-4096x4096x64", "none"),
             ("w256not-1536x768x4096", "w256-768x768x11328", "wb"),
             ("w-201x309x2048", "w-200x309x2048", "cf"),
             ("sk-81x1536x512", "sk-80x1536x512", "none"),
             ("g64-257x512x512", "sk-256x1544x2048", "none"),
             ("f32-65x64x64", "f32-64x512x2048", "none"),
             ("f32-64x512x2052", "f32-64x512x2048", "none"))

# class R: one case per kernel name, with the fullest epilogue that kernel takes
R_RUNS = (
    ("sk-16x512x512", Run("full")), ("sk-2x309x520", Run("full")),
    ("sk-81x1536x512", Run("full")), ("sk-81x1536x520", Run("full", "odd")),
    ("g64-257x512x512", Run("full")), ("g128-257x512x512", Run("full")), ("g128-257x512x520", Run("full", "odd")),
    ("g256-4096x4096x64", Run("fullc")), ("g256-4100x4096x128", Run("full")),
    ("g256s-NN-4096x4096x128", Run("fullc")),
    ("w-200x136x96", Run("cfacc_alpha", "tight")), ("w-512x512x4160", Run("cfacc_alpha", "vec8")),
    ("w-512x512x4160", Run("wbacc")), ("wfused-512x512x2056", Run("wbacc")),
    ("w256-768x768x11328", Run("wbacc")), ("w256-776x768x11328", Run("wbacc")),
    ("f32-37x100x100", Run("full")), ("f32-64x512x2052", Run("full")), ("f32-130x264x1040", Run("full")),
    ("f32-200x309x66", Run("full", "odd")),
)

# every kernel the tables must reach (tests/test_gemm_ref_cpu.py), in the
# library's order: CASES the bf16 / fp32 ones, F8_CASES the e4m3 ones
F8_KERNEL_NAMES = ("f8_generic", "f8_stream", "f8_q8_generic", "f8_q8_stream", "f8_q8_gate8", "f8_g256s",
                   "f8_wgrad256s")
KERNEL_NAMES = ("skinny_m16_kf", "skinny_m16_guard", "skinny_s64_kf", "skinny_s64_guard", "gemm64",
                "g128_glds", "g128_reg", "g256_stream", "g256_generic", "g256s", "splitk_reduce",
                "splitk_fused", "wgrad256", "wgrad256s", "f32_rows", "f32_skinny", "f32_mfma",
                "f32_tile") + F8_KERNEL_NAMES


def classes(case):
    """Input classes of the exact test for a case."""
    return ("S", "F") if case.flop <= F_CLASS_FLOP else ("S",)


# ------------------------------------------------------ dispatch mirror
def lds_of(case, run):
    """Row strides of C, Cf, residual, gate for a run (elements)."""
    return {k: case.N + v for k, v in FRAMES[run.frame].items()}


def epi_flags(case, run):
    """What the launcher sees of a run: the GemmEpi fields the dispatch
    reads, e.vec as smer_gemm / smer_gemm_wgrad_bias_ex compute it (buffers
    are 16-B aligned but for a bias view offset by a float), whether a
    workspace is passed (ops._gemm_call) and the row-sum output."""
    e = EPI[run.epi]
    ld = lds_of(case, run)
    rowsum = run.api == "wgrad_bias"
    drop = e.drop
    if rowsum:
        vec = ld["ldcf"] % 8 == 0
    else:
        vec = ((not e.bias or run.bias_off % 4 == 0) and (not e.residual or ld["ldr"] % 8 == 0) and
               (not e.gate or ld["ldg"] % 8 == 0) and (not e.C or ld["ldc"] % 8 == 0) and
               (not e.Cf or ld["ldcf"] % 8 == 0))
    ws = rowsum or (e.Cf and not e.C and not e.bias and not e.residual and not e.gate)
    return SimpleNamespace(C=e.C, Cf=e.Cf, bias=e.bias, relu=e.relu, drop=drop, residual=e.residual, gate=e.gate,
                           vec=vec, rowsum=rowsum, ws=ws, ldcf=ld["ldcf"], max_wg=run.max_wg,
                           lda=case.a_ld, a_off=case.a_off)


def _cdiv(a, b):
    return (a + b - 1) // b


def expected_kernel(dtype, ak, bk, M, N, K, epi, env, cus):
    """The kernel name of expected_plan."""
    return expected_plan(dtype, ak, bk, M, N, K, epi, env, cus).name


def expected_plan(dtype, ak, bk, M, N, K, epi, env, cus):
    """Pure-Python mirror of the GEMM dispatch (csrc/gemm_plan.h gemm_plan,
    an independent statement held against the library's smer_gemm_plan by
    the tests) with every cached switch at its default: `name`, the kernel a
    call runs on, as one of KERNEL_NAMES, a split-K launch being
    "<kernel>+splitk_reduce" or "<kernel>+splitk_fused"; `split` and `kchunk`
    of the weight-gradient paths (None where the mirror computes none)."""
    P = lambda name, split=None, kchunk=None: SimpleNamespace(name=name, split=split, kchunk=kchunk)  # noqa: E731
    env = env or {}
    on = lambda k: env.get(k, "")[:1] != "0"  # noqa: E731
    if dtype == F32:
        al = K % 4 == 0 and (epi.lda or 0) % 4 == 0 and not epi.a_off
        if ak and bk and M <= 64 and al:
            return P("f32_rows" if K <= 2048 else "f32_skinny")
        if ak and bk and al and on("SMER_GEMM_F32_MFMA"):
            return P("f32_mfma")
        return P("f32_tile")
    rowsum = epi.rowsum
    if ak and bk and M <= 256 and not rowsum:
        m16 = _cdiv(N, 16) * _cdiv(M, 16) <= 2 * cus
        return P("skinny_%s_%s" % ("m16" if m16 else "s64", "kf" if K % 32 == 0 else "guard"))
    # smer_gemm_wgrad_bias_ex max_workgroups (wgrad_cap), the pure Cf (+)= A B^T epilogue, slabs that fit
    cap = (lambda v: max(8, min(v, epi.max_wg))) if epi.max_wg > 0 else (lambda v: v)
    cf_only = epi.Cf and not (epi.C or epi.bias or epi.residual or epi.gate or epi.relu or epi.drop)
    fit = ((WS_BYTES - TICKET_BYTES) if epi.ws else 0) // ((M * N + M) * 4)
    t2 = _cdiv(M, 256) * _cdiv(N, 256)
    whole = M % 256 == 0 and N % 256 == 0
    if ak and not rowsum and K % 64 == 0 and on("SMER_GEMM256") and t2 >= cus:
        s = env.get("SMER_GEMM256S", "")[:1]
        stag = s == "1" or (s != "0" and (K >= 1024 or (not bk and N >= 1024)))
        ok = epi.vec and epi.C and not epi.Cf and whole and not (epi.residual and epi.gate)
        if stag and ok and K % 32 == 0 and K // 32 >= 4:
            return P("g256s")
        return P("g256_stream" if ok else "g256_generic")
    if not ak and not bk and K % 64 == 0 and epi.ws and (M * N >= 1536 * 768 or (M >= 768 and N >= 768)):
        ns = min(cap(cus) // max(1, t2), K // 512, fit)
        ns = max(1, min(ns, 64))
        if cf_only and (M * N) % 4 == 0 and t2 * ns * 4 >= 3 * cus:
            kchunk = _cdiv(_cdiv(K, ns), 64) * 64
            split = _cdiv(K, kchunk)
            name = "wgrad256s" if on("SMER_WGRAD256S") and whole and epi.vec else "wgrad256"
            return P(name + ("+splitk_reduce" if split > 1 else ""), split, kchunk)
    tiles = _cdiv(M, 128) * _cdiv(N, 128)
    split = 1
    if cf_only and epi.ws and not (tiles >= 512 or K < 1024 or (M * N) % 4 != 0):
        split = max(1, min(cap(max(8, 2 * cus)) // tiles, K // 1024, fit, 64))
    if ak and not rowsum and split == 1 and K % 64 == 0 and tiles <= 4 * cus and M > 256 and on("SMER_GEMM64"):
        return P("gemm64")
    kchunk = K
    if split > 1:
        kchunk = _cdiv(_cdiv(K, split), 64) * 64
        split = _cdiv(K, kchunk)
    name = "g128_glds" if K % 64 == 0 and kchunk % 64 == 0 else "g128_reg"
    if split > 1:
        fused = env.get("SMER_SPLITK_FUSED", "")[:1] == "1" and N % 4 == 0 and epi.ldcf % 4 == 0 and \
            tiles * 4 <= TICKET_BYTES
        name += "+splitk_fused" if fused else "+splitk_reduce"
    return P(name, split, kchunk)


def mirror_plan(case, run, cus):
    f = epi_flags(case, run)
    if case.dtype == F32:
        f.lda = case.a_ld if case.a_ld is not None else in_ld(case, "A")
    return expected_plan(case.dtype, case.ak, case.bk, case.M, case.N, case.K, f, case.env, cus)


def label(case, run, cus):
    return mirror_plan(case, run, cus).name


# include/smer_hip.h SMER_PLAN_*, by the field of epi_flags that sets each
PLAN_BITS = dict(C=0x1, Cf=0x2, bias=0x4, relu=0x8, drop=0x10, residual=0x20, gate=0x40, vec=0x80,
                 rowsum=0x800, ws=0x1000)
PLAN_CF_ALIGNED16, PLAN_F32_ALIGNED = 0x400, 0x2000


def library_plan(lib, case, run, cus):
    """What the library's own dispatch would launch for a run (smer_gemm_plan:
    nothing is launched; cus = 0 asks for the current device's CU count), in
    the form of expected_plan.  smer_gemm_plan takes the facts of a call as
    plain ints, so this is the library's plan for this module's MODEL of the
    call (epi_flags: e.vec, the workspace of ops._gemm_call / linear_wgrad;
    16-B aligned buffers but for a_off, the strides of input_bufs), not for
    the pointers tests/test_gemm_edges_gpu.py execute() passes: it holds the
    library's decision against the mirror's, and a fact that epi_flags
    mis-models is wrong on both sides alike."""
    import ctypes
    f = epi_flags(case, run)
    facts = sum(bit for k, bit in PLAN_BITS.items() if getattr(f, k)) | PLAN_CF_ALIGNED16
    if case.dtype == F32:
        lda = case.a_ld if case.a_ld is not None else in_ld(case, "A")
        if lda % 4 == 0 and in_ld(case, "B") % 4 == 0 and case.a_off % 4 == 0:
            facts |= PLAN_F32_ALIGNED
    out = (ctypes.c_int * 8)()
    rc = lib.smer_gemm_plan(1 if case.dtype == BF16 else 0, int(case.ak), int(case.bk), case.M, case.N, case.K,
                            facts, f.ldcf, WS_BYTES if f.ws else 0, run.max_wg, cus, out)
    assert rc == 0, lib.smer_last_error()
    kernel, _, _, _, _, split, kchunk, reduce = out
    name = "+".join(lib.smer_gemm_kernel_name(i).decode() for i in (kernel, reduce) if i >= 0)
    return SimpleNamespace(name=name, split=split, kchunk=kchunk)


# ------------------------------------------------- e4m3 dispatch mirror
F8 = 2                      # include/smer_hip.h SMER_F8
PLAN_Q8, PLAN_GATE8 = 0x200, 0x4000
F8_LDS_GENERIC = 128 << 10  # two 64-KiB operand stages
F8_LDS_STREAM = 160 << 10   # + 64 epilogue rows of 256 bf16
F8_LDS_WGRAD = 128 << 10    # four 32-KiB slots


def expected_plan_f8(fwd, M, N, K, *, vec=True, q8=False, gate8=False, ws_bytes=WS_BYTES, max_wg=0,
                     env=None, cus=256):
    """Pure-Python mirror of the e4m3 dispatch (csrc/gemm_plan.h plan_f8),
    written from its rules: the forward / dgrad products (fwd; M, N % 256 ==
    0, K % 128 == 0) by epilogue on min(tiles, CUs rounded down to 8)
    workgroups; the weight gradient (K % 64 == 0) on its one kernel, split
    over K like the bf16 256x256 weight gradient but for N / 256 rows of M
    bias partials per slice.  name, split, kchunk as expected_plan; grid and
    dynamic LDS bytes."""
    env = env or {}
    tiles = (M // 256) * (N // 256)

    def persistent(nwg, room):
        return nwg if nwg <= room else room // 8 * 8

    def P(name, lds, grid, split=1, kchunk=K):
        return SimpleNamespace(name=name, split=split, kchunk=kchunk, grid=grid, lds=lds)

    if fwd:
        grid = persistent(tiles, cus)
        if env.get("SMER_GEMM256S_FP8", "")[:1] == "1" and vec and not q8 and K % 64 == 0 and K // 64 >= 4:
            return P("f8_g256s", F8_LDS_STREAM, grid)
        if not vec:
            return P("f8_generic", F8_LDS_GENERIC, grid)
        if gate8:
            return P("f8_q8_gate8", F8_LDS_STREAM, grid)
        if q8 and env.get("SMER_FP8_Q8_FAST", "")[:1] == "0":
            return P("f8_q8_generic", F8_LDS_GENERIC, grid)
        return P("f8_q8_stream" if q8 else "f8_stream", F8_LDS_STREAM, grid)
    room = max(8, min(cus, max_wg)) if max_wg > 0 else cus
    slice_bytes = 4 * (M * N + (N // 256) * M)
    ns = min(room // tiles, K // 512, max(0, ws_bytes - TICKET_BYTES) // slice_bytes, 64)
    split, kchunk = 1, K
    if ns > 1:
        kchunk = _cdiv(_cdiv(K, ns), 64) * 64
        split = _cdiv(K, kchunk)
    return P("f8_wgrad256s" + ("+splitk_reduce" if split > 1 else ""), F8_LDS_WGRAD,
             persistent(tiles * split, room), split, kchunk)


def library_plan_f8(lib, fwd, M, N, K, *, vec=True, q8=False, gate8=False, ws_bytes=WS_BYTES, max_wg=0, cus=0):
    """smer_gemm_plan's answer for the e4m3 call expected_plan_f8 describes,
    under the current environment (cus = 0: the current device's count)."""
    import ctypes
    facts = PLAN_BITS["C"] if fwd else PLAN_BITS["Cf"] | PLAN_CF_ALIGNED16
    facts |= (PLAN_BITS["vec"] if vec else 0) | (PLAN_Q8 if q8 else 0)
    facts |= (PLAN_GATE8 | PLAN_BITS["gate"] if gate8 else 0) | (PLAN_BITS["ws"] if not fwd and ws_bytes else 0)
    out = (ctypes.c_int * 8)()
    rc = lib.smer_gemm_plan(F8, int(fwd), int(fwd), M, N, K, facts, N, 0 if fwd else ws_bytes, max_wg, cus, out)
    assert rc == 0, lib.smer_last_error()
    kernel, _, grid, _, lds, split, kchunk, reduce = out
    name = "+".join(lib.smer_gemm_kernel_name(i).decode() for i in (kernel, reduce) if i >= 0)
    return SimpleNamespace(name=name, split=split, kchunk=kchunk, grid=grid, lds=lds)


def _f8_table():
    """Plan-only cases (no operands) at the edges where plan_f8 decides."""
    t = []

    def add(cid, fwd, M, N, K, env=None, **facts):
        t.append(SimpleNamespace(id=cid, fwd=fwd, M=M, N=N, K=K, env=dict(env or {}), facts=facts))

    stag = {"SMER_GEMM256S_FP8": "1"}
    add("f8-stream", True, 512, 768, 768)
    add("f8-generic-bias-off4", True, 512, 768, 768, vec=False)     # e.g. a bias view at a 4-byte offset
    add("f8-q8", True, 512, 768, 768, q8=True)
    add("f8-q8-fast1", True, 512, 768, 768, q8=True, env={"SMER_FP8_Q8_FAST": "1"})
    add("f8-q8-fast0", True, 512, 768, 768, q8=True, env={"SMER_FP8_Q8_FAST": "0"})
    add("f8-fast0-no-copy", True, 512, 768, 768, env={"SMER_FP8_Q8_FAST": "0"})
    add("f8-gate8", True, 512, 768, 256, q8=True, gate8=True)
    add("f8-g256s-K256", True, 512, 768, 256, env=stag)              # the four-step minimum
    add("f8-g256s-K128", True, 512, 768, 128, env=stag)              # below it
    add("f8-g256s-q8", True, 512, 768, 768, env=stag, q8=True)       # the e4m3 copy is not staggered
    add("f8-g256s-novec", True, 512, 768, 768, env=stag, vec=False)
    add("f8-g256s-off", True, 512, 768, 768, env={"SMER_GEMM256S_FP8": "0"})
    add("f8-bf16-switch", True, 512, 768, 768, env={"SMER_GEMM256S": "1"})   # the bf16 switch of the same prefix
    # tile counts one below, at and one above 64 / 256 / 304 CUs
    for tm, tn in ((7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (1, 257), (3, 101), (16, 19), (5, 61)):
        add("f8-tiles%d" % (tm * tn), True, 256 * tm, 256 * tn, 128)
        add("f8w-tiles%d" % (tm * tn), False, 256 * tm, 256 * tn, 64)
    # weight gradients
    add("f8w-T64", False, 256, 256, 64)                              # one slice
    add("f8w-depth", False, 768, 768, 2048)                          # K / 512 = 4 binds
    add("f8w-ws", False, 2304, 768, 65536, ws_bytes=16 << 20)        # two slices fit
    # N / 256 = 2: three slices of M * N + 2 M floats fit, four of bf16's M * N + M would
    add("f8w-partials", False, 256, 512, 8192, ws_bytes=TICKET_BYTES + 16 * (256 * 512 + 2 * 256) - 4)
    add("f8w-64slices", False, 256, 256, 65536)
    for w in (4, 8, 100, 1000):                                      # 4: the cap's floor of 8 workgroups
        add("f8w-wg%d" % w, False, 768, 768, 8192, max_wg=w)
    add("f8w-wg100-over", False, 2304, 3072, 8192, max_wg=100)       # 108 tiles on 96 = 100 rounded down to 8
    add("f8w-no-ws", False, 768, 768, 8192, ws_bytes=0)
    add("f8w-tickets-only", False, 768, 768, 8192, ws_bytes=TICKET_BYTES)
    add("f8w-c4", False, 768, 3072, 65536)
    return t


F8_CASES = _f8_table()
assert len({c.id for c in F8_CASES}) == len(F8_CASES)


def f8_mirror(case, cus):
    return expected_plan_f8(case.fwd, case.M, case.N, case.K, env=case.env, cus=cus, **case.facts)


def plan_mismatches(lib, cus, setenv, lib_cus=None):
    """Every (case, run) of the table whose mirror and library plans differ at
    `cus` CUs (the library asked with lib_cus when given: 0 is the device's
    own count), the case's env applied through `setenv(env)`:
    [(case id, run id, mirror, library)]; of F8_CASES, the cases that differ
    in name, split, kchunk, grid or LDS bytes."""
    bad = []
    for case in F8_CASES:
        setenv(case.env)
        m = f8_mirror(case, cus)
        l = library_plan_f8(lib, case.fwd, case.M, case.N, case.K, cus=cus if lib_cus is None else lib_cus,
                            **case.facts)
        if vars(m) != vars(l):
            bad.append((case.id, "", vars(m), vars(l)))
    for case in CASES:
        setenv(case.env)
        for run in case.runs:
            m = mirror_plan(case, run, cus)
            l = library_plan(lib, case, run, cus if lib_cus is None else lib_cus)
            same = m.name == l.name and (m.split is None or (m.split, m.kchunk) == (l.split, l.kchunk))
            if not same:
                bad.append((case.id, run_id(run), vars(m), vars(l)))
    return bad


def all_runs():
    """Every (case, class, run) of the exact test."""
    return [(c, cls, r) for c in CASES for cls in classes(c) for r in c.runs]


# ---------------------------------------------------------------- frames
class Buf:
    """A [rows, cols] view at `offset` into a flat buffer of (rows + 2) rows
    of `ld` elements, everything outside the view holding `fill`."""

    def __init__(self, data, ld=None, fill=math.nan, offset=0):
        self.rows, self.cols = data.shape
        self.ld = ld if ld is not None else self.cols
        assert self.ld >= self.cols
        self.offset, self.fill = offset, fill
        self.flat = torch.full((offset + (self.rows + 2) * self.ld,), fill, dtype=data.dtype)
        self._grid(self.flat)[:self.rows, :self.cols] = data
        self.dev = None

    def _grid(self, flat):
        return flat[self.offset:].view(self.rows + 2, self.ld)

    def to(self, device):
        self.dev = self.flat.to(device)
        return self.view()

    def view(self):
        return torch.as_strided(self.dev, (self.rows, self.cols), (self.ld, 1), self.offset)

    def parts(self):
        """(interior, everything else flattened) of the device buffer, on the CPU."""
        flat = self.dev.cpu()
        g = self._grid(flat)
        rest = torch.cat([flat[:self.offset], g[:self.rows, self.cols:].reshape(-1), g[self.rows:].reshape(-1)])
        return g[:self.rows, :self.cols], rest


def in_ld(case, which):
    """Row stride of an input operand: the width + 8 (bf16) / + 4 (fp32) for
    a row image, round_up(rows, 8) + 8 for a column image."""
    kc = case.ak if which == "A" else case.bk
    rows = case.M if which == "A" else case.N
    if kc:
        return case.K + (8 if case.dtype == BF16 else 4)
    return round_up(rows, 8) + 8


def input_bufs(case, ins):
    """NaN-framed buffers of A and B in the layout of the case."""
    a = ins.A if case.ak else ins.A.t().contiguous()
    b = ins.B if case.bk else ins.B.t().contiguous()
    a_ld = case.a_ld if case.a_ld is not None else in_ld(case, "A")
    return Buf(a, a_ld, offset=case.a_off), Buf(b, in_ld(case, "B"))


# ---------------------------------------------------------------- inputs
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, shape, lo, hi, dtype):
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def _operand(g, cls, rows, K, dtype, scale):
    if cls == "S":
        return _ints(g, (rows, K), -8, 8, dtype)
    if cls == "F":
        m = torch.randint(-255, 256, (rows, K), generator=g)
        nz = torch.rand(rows, K, generator=g) < min(1.0, math.sqrt(128.0 / K))
        return (m * nz).to(dtype) * 2.0 ** -7
    return (torch.randn(rows, K, generator=g) * scale).to(dtype)


@functools.lru_cache(maxsize=2)
def _inputs(cid, cls):
    c = BY_ID[cid]
    g = _gen(c.M, c.N, c.K, c.lay, str(c.dtype), cls)
    M, N, K, dt = c.M, c.N, c.K, c.dtype
    r = SimpleNamespace(A=_operand(g, cls, M, K, dt, 1.0), B=_operand(g, cls, N, K, dt, 0.05))
    if cls == "R":
        r.bias = torch.randn(N, generator=g)
        r.residual = torch.randn(M, N, generator=g).to(dt)
        r.gate = torch.randn(M, N, generator=g).to(dt)
        r.gate[torch.rand(M, N, generator=g) < 0.1] = 0
        r.cf0 = torch.randn(M, N, generator=g)
        r.db0 = torch.randn(M, generator=g)
    else:
        q = EPI_SCALE[cls]
        r.bias = _ints(g, (N,), -16, 16, F32) * q
        r.residual = _ints(g, (M, N), -64, 64, dt) * q
        r.gate = _ints(g, (M, N), -1, 1, dt)
        r.cf0 = _ints(g, (M, N), -64, 64, F32) * q
        r.db0 = _ints(g, (M,), -64, 64, F32) * q
    return r


def inputs(case, cls):
    """Deterministic CPU inputs of a case in a class (logical orientation:
    A [M, K], B [N, K]); shared, do not modify."""
    return _inputs(case.id, cls)


GRID = {"S": 1.0, "F": 2.0 ** -14}
# Class F: sum_k |a b| alone reaches 0.79 * 2**22 grid units (about 200 at
# K >= 128), which leaves room for 53: the integer epilogue operands are
# scaled by 1/4 there (bias <= 4, residual and Cf0 <= 16: 36 in all)
EPI_SCALE = {"S": 1.0, "F": 0.25}


def _terms(case):
    """Which epilogue operands some exact run of the case passes."""
    es = [EPI[r.epi] for r in case.runs]
    return any(e.bias for e in es), any(e.residual for e in es), any(e.accumulate for e in es)


def s_units(case):
    """Analytic worst case of the S class: sum_k |a b| <= 64 K plus the
    largest epilogue terms (bias 16, residual 64, Cf0 64) of the case's runs."""
    bias, res, cf0 = _terms(case)
    return 64 * case.K + 16 * bias + 64 * res + 64 * cf0


def exact_units(case, cls, sabs=None):
    """max over the outputs of sum_k |a b| + |bias| + |residual| + |Cf0| (the
    operands some run of the case passes) in grid units, from the inputs
    (sabs = |A| @ |B|^T in float64, computed here when not given).  The row
    sum db (sum_k |dy| + |db0|) is far below it."""
    ins = inputs(case, cls)
    bias, res, cf0 = _terms(case)
    t = sabs if sabs is not None else ins.A.double().abs() @ ins.B.double().abs().t()
    if bias:
        t = t + ins.bias.double().abs().view(1, -1)
    if res:
        t = t + ins.residual.double().abs()
    if cf0:
        t = t + ins.cf0.double().abs()
    return t.max().item() / GRID[cls]


# ------------------------------------------------------------- reference
def product64(case, cls, device=None):
    """float64 A B^T and |A| |B|^T on the CPU; with `device` and a case above
    DEVICE_PRODUCT_FLOP the two products alone are taken by torch.matmul in
    float64 there (independent of the code under test; exact for S and F in
    any order, every sum being far below 2**53)."""
    ins = inputs(case, cls)
    dev = device if device is not None and case.flop > DEVICE_PRODUCT_FLOP else "cpu"
    a, b = ins.A.to(dev).double(), ins.B.to(dev).double()
    p = (a @ b.t()).cpu()
    s = (a.abs() @ b.abs().t()).cpu() if cls == "R" else None
    return p, s


def reference(case, cls, run, prod):
    """Expected outputs of a run from the float64 product `prod`: v (C before
    its store), cf, db (float64; None where the run has none), and the
    operands the run passes."""
    ins, e = inputs(case, cls), EPI[run.epi]
    alpha, gs, p = scalars(run.epi, cls)
    use = SimpleNamespace(bias=ins.bias if e.bias else None, residual=ins.residual if e.residual else None,
                          gate=ins.gate if e.gate else None, cf0=ins.cf0 if e.accumulate else None,
                          db0=ins.db0 if e.accumulate else None, alpha=alpha, gate_scale=gs, drop_p=p)
    v, cf = epilogue64(prod, alpha=alpha, bias=use.bias, relu=e.relu, drop_p=p, seed=SEED, residual=use.residual,
                       gate=use.gate, gate_scale=gs, cf0=use.cf0, accumulate=e.accumulate)
    db = None
    if run.api == "wgrad_bias":
        db = ins.A.double().sum(1) + (ins.db0.double() if e.accumulate else 0.0)
    return SimpleNamespace(v=v if e.C else None, cf=cf if e.Cf else None, db=db, use=use)


def r_bound(case, run, ref, sabs):
    """Per-element bounds of the R class (module docstring) for C, Cf, db."""
    ins, e, use = inputs(case, "R"), EPI[run.epi], ref.use
    K = case.K
    t = abs(f32r(use.alpha)) * sabs
    if use.bias is not None:
        t = t + use.bias.double().abs().view(1, -1)
    if use.residual is not None:
        t = t + use.residual.double().abs()
    t = t * f32r(use.gate_scale)
    if use.cf0 is not None:
        t = t + use.cf0.double().abs()
    t = t * drop_scale32(use.drop_p)
    b = (K + 8) * U * t
    out = SimpleNamespace(C=None, Cf=None, db=None)
    if e.C:
        out.C = b + (UB * ref.v.abs() if case.dtype == BF16 else 0.0)
    if e.Cf:
        out.Cf = b
    if ref.db is not None:
        tb = ins.A.double().abs().sum(1) + (use.db0.double().abs() if use.db0 is not None else 0.0)
        out.db = (K + 8) * U * tb
    return out

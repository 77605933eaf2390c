"""smer_gemm (bf16 and fp32) and smer_gemm_wgrad_bias_ex (csrc/gemm.hip)
against the float64 reference of tests/gemmref.py, element by element, at the
shapes where launch_bf16 / launch_f32 change kernel or template arguments
(gemmref.CASES; before each run the library's own plan for the call,
smer_gemm_plan, must name the kernel gemmref.expected_kernel expects at the
device's CU count).

 * test_plan_matches_mirror: the library's dispatch against the mirror over
   the whole table, at the device's CU count and at 64 / 256 / 304.

 * test_exact: inputs whose every product and partial sum is exact in fp32
   (classes S and F, gemmref's docstring; the precondition is asserted): C,
   Cf and db must equal the float64 result rounded to the output type bit for
   bit, whatever the summation order, split-K or MFMA internals.
 * test_bound: randn inputs, alpha 0.3, gate_scale 1.25, drop_p 0.1 against
   the any-order fp32 bound (K + 8) * 2**-24 * T of the element (+ 2**-8 |ref|
   for a bf16 store), T the summed magnitude of its terms.
 * test_deterministic_and_variants: weight gradients twice with identical
   bits, the fused split-K reduce against the separate one (tickets zero
   afterwards), SMER_WGRAD256S 1 against 0.
Every output is a strided view into a sentinel-framed buffer that must come
back intact, prefilled with NaN unless the call accumulates; every input's
pads and guard rows hold NaN.
"""
import math
from types import SimpleNamespace

import pytest
import torch

from tests import gemmref as G
from tests.test_train_ops_gpu import assert_same_bits, assert_within, bits

pytestmark = pytest.mark.gpu

dev = "cuda"
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


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def set_env(monkeypatch, env):
    for k in G.ENV_SWITCHES:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def planned(case, run):
    """The library's plan for a run as gemmref models the call execute()
    makes (G.library_plan), on this device and under the current
    environment; printed as the run's label."""
    from smer_music_generation_amd import _lib as L
    name = G.library_plan(L.load(), case, run, 0).name
    print("%s %s -> %s" % (case.id, G.run_id(run), name))
    return name


@pytest.mark.parametrize("ncus", [0, 64, 256, 304], ids=lambda n: "cus%d" % n if n else "device")
def test_plan_matches_mirror(monkeypatch, ncus):
    """The library's dispatch (smer_gemm_plan: the very gemm_plan the
    launchers run, nothing launched) and gemmref's mirror agree on every
    (case, run) of the table, split-K slices and depth included, and on every
    plan-only e4m3 case (gemmref.F8_CASES), at this device's CU count and at
    64 / 256 / 304; the library's kernel names are gemmref.KERNEL_NAMES."""
    from smer_music_generation_amd import _lib as L
    lib = L.load()
    names = [lib.smer_gemm_kernel_name(i) for i in range(len(G.KERNEL_NAMES) + 1)]
    assert names == [n.encode() for n in G.KERNEL_NAMES] + [None]
    bad = G.plan_mismatches(lib, ncus or cus(), lambda env: set_env(monkeypatch, env), lib_cus=ncus)
    assert not bad, bad


class Operands:
    """Device copies of a case's A and B in NaN-framed buffers."""

    def __init__(self, case, cls):
        self.case, self.cls = case, cls
        self.a, self.b = G.input_bufs(case, G.inputs(case, cls))
        self.A, self.B = self.a.to(dev), self.b.to(dev)


def frame_intact(buf, what):
    """(interior of an output buffer on the CPU); its pads and guard rows
    must hold the sentinel bit for bit and the interior no NaN."""
    inner, rest = buf.parts()
    assert_same_bits(rest, torch.full_like(rest, G.SENT), what + ": sentinel around the output")
    assert not torch.isnan(inner).any(), what + ": NaN left in the output"
    return inner


def execute(opnd, run, ref):
    """One call of a run on the device; returns the outputs' interiors
    (C, Cf, db; None where absent) after checking their frames."""
    case, e, use = opnd.case, G.EPI[run.epi], ref.use
    M, N, K = case.M, case.N, case.K
    ld = G.lds_of(case, run)
    what = "%s %s %s" % (case.id, opnd.cls, G.run_id(run))
    nan = lambda dt, *s: torch.full(s, math.nan, dtype=dt)  # noqa: E731
    C = G.Buf(nan(case.dtype, M, N), ld["ldc"], G.SENT) if e.C else None
    Cf = G.Buf(use.cf0 if e.accumulate else nan(F32, M, N), ld["ldcf"], G.SENT) if e.Cf else None
    O = ops()
    db = None
    if run.api == "wgrad_bias":
        db = G.Buf((use.db0 if e.accumulate else nan(F32, M)).view(1, M), M + 8, G.SENT)
        O.linear_wgrad(opnd.A, opnd.B, Cf.to(dev), accumulate=e.accumulate, db=db.to(dev).view(M),
                       max_wg=run.max_wg)
    else:
        res = G.Buf(use.residual, ld["ldr"]).to(dev) if e.residual else None
        gate = G.Buf(use.gate, ld["ldg"]).to(dev) if e.gate else None
        bias = None
        if e.bias:  # a view offset by bias_off floats: 4-byte, not 16-byte aligned when bias_off = 1
            bias = G.Buf(use.bias.view(1, N), N + 8, offset=run.bias_off).to(dev).view(N)
        O.gemm(opnd.A, opnd.B, M=M, N=N, K=K, a_kcontig=case.ak, b_kcontig=case.bk,
               out=C.to(dev) if C else None, out_f32=Cf.to(dev) if Cf else None, accumulate=e.accumulate,
               bias=bias, alpha=use.alpha, relu=e.relu, residual=res, gate=gate, gate_scale=use.gate_scale,
               drop_p=use.drop_p, seed=G.SEED, dtype=case.dtype)
    torch.cuda.synchronize()
    return SimpleNamespace(C=frame_intact(C, what + " C") if C else None,
                           Cf=frame_intact(Cf, what + " Cf") if Cf else None,
                           db=frame_intact(db, what + " db").reshape(M) if db else None, what=what)


def check_exact(out, ref, case):
    if out.C is not None:
        assert_same_bits(out.C, G.to_dtype(ref.v, case.dtype), out.what + " C")
    if out.Cf is not None:
        assert_same_bits(out.Cf, G.to_dtype(ref.cf, F32), out.what + " Cf")
    if out.db is not None:
        assert_same_bits(out.db, G.to_dtype(ref.db, F32), out.what + " db")


def tickets_zero(what):
    O = ops()
    ws = O.splitk_workspace(torch.device(dev, torch.cuda.current_device()))
    assert not ws[-G.TICKET_BYTES:].any().item(), what + ": split-K tickets not zero after the call"


EXACT = [(c, cls) for c in G.CASES for cls in G.classes(c)]


@pytest.mark.parametrize("case,cls", EXACT, ids=["%s-%s" % (c.id, cls) for c, cls in EXACT])
def test_exact(monkeypatch, case, cls):
    set_env(monkeypatch, case.env)
    assert G.s_units(case) <= G.EXACT_LIMIT
    if cls == "F":
        assert G.exact_units(case, cls) <= G.EXACT_LIMIT
    opnd = Operands(case, cls)
    prod, _ = G.product64(case, cls, dev)
    for run in case.runs:
        assert planned(case, run) == G.label(case, run, cus()), "%s %s %s" % (case.id, cls, G.run_id(run))
        ref = G.reference(case, cls, run, prod)
        check_exact(execute(opnd, run, ref), ref, case)
        if "SMER_SPLITK_FUSED" in case.env:
            tickets_zero(case.id)


@pytest.mark.parametrize("cid,run", G.R_RUNS, ids=["%s-%s" % (c, G.run_id(r)) for c, r in G.R_RUNS])
def test_bound(monkeypatch, cid, run):
    case = G.BY_ID[cid]
    set_env(monkeypatch, case.env)
    assert planned(case, run) == G.label(case, run, cus()), "%s R %s" % (case.id, G.run_id(run))
    prod, sabs = G.product64(case, "R", dev)
    ref = G.reference(case, "R", run, prod)
    bound = G.r_bound(case, run, ref, sabs)
    out = execute(Operands(case, "R"), run, ref)
    if out.C is not None:
        assert_within(out.C, ref.v, bound.C, out.what + " C")
    if out.Cf is not None:
        assert_within(out.Cf, ref.cf, bound.Cf, out.what + " Cf")
    if out.db is not None:
        assert_within(out.db, ref.db, bound.db, out.what + " db")


WGRADS = [c for c in G.CASES if c.lay == "TN" and c.dtype == BF16 and c.id.startswith("w") and not c.env]


@pytest.mark.parametrize("case", WGRADS, ids=lambda c: c.id)
def test_deterministic_and_variants(monkeypatch, case):
    """S inputs: a second run gives the same bits; with SMER_SPLITK_FUSED=1
    the last-arriver reduce gives the bits of the separate reduce and leaves
    the tickets zero; SMER_WGRAD256S=0 and 1 both give the reference's bits;
    every max_workgroups cap gives the reference's bits (the caps need not
    agree with each other in general: these inputs are exact)."""
    set_env(monkeypatch, {})
    opnd = Operands(case, "S")
    prod, _ = G.product64(case, "S", dev)
    for run in [r for r in case.runs if r.frame in ("vec8", "cf4") and not G.EPI[r.epi].alpha]:
        ref = G.reference(case, "S", run, prod)
        first = execute(opnd, run, ref)
        check_exact(first, ref, case)
        variants = [("again", {})]
        lab = G.label(case, run, cus())
        if "splitk_reduce" in lab and lab.startswith("g128"):
            variants.append(("fused", {"SMER_SPLITK_FUSED": "1"}))
        if lab.startswith("wgrad256"):
            variants += [("two-stage", {"SMER_WGRAD256S": "0"}), ("staggered", {"SMER_WGRAD256S": "1"})]
        for name, env in variants:
            set_env(monkeypatch, env)
            out = execute(opnd, run, ref)
            for k in ("Cf", "db"):
                if getattr(first, k) is not None:
                    assert torch.equal(bits(getattr(out, k)), bits(getattr(first, k))), \
                        "%s %s: %s differs from the first run" % (out.what, name, k)
            tickets_zero("%s %s" % (out.what, name))
        set_env(monkeypatch, {})

"""tests/gemmref.py checked on the CPU: its float64 epilogue against a
straightforward expression, the exactness precondition of every exact case of
the shape table, the dispatch mirror's coverage of the GEMM kernels at 256
CUs, and the class R bound against the same product evaluated in fp32."""
import numpy as np
import pytest
import torch

from tests import gemmref as G
from tests.hashref import drop_threshold, keep_mask

CUS = 256


# ------------------------------------------------------------ epilogue64
@pytest.mark.parametrize("cls", ["S", "R"])
@pytest.mark.parametrize("name", sorted(G.EPI))
def test_epilogue64(name, cls):
    e = G.EPI[name]
    M, N = 37, 40
    g = torch.Generator().manual_seed(5)
    acc = torch.randn(M, N, generator=g).double() * 7
    bias, res, gate = torch.randn(N, generator=g), torch.randn(M, N, generator=g).bfloat16(), \
        torch.randint(-1, 2, (M, N), generator=g).bfloat16()
    cf0 = torch.randn(M, N, generator=g)
    alpha, gs, p = G.scalars(name, cls)
    v, cf = G.epilogue64(acc, alpha=alpha, bias=bias if e.bias else None, relu=e.relu, drop_p=p, seed=9,
                         residual=res if e.residual else None, gate=gate if e.gate else None, gate_scale=gs,
                         cf0=cf0, accumulate=e.accumulate)
    # residual + dropout(relu(alpha * acc + bias)), then the gate mask
    a32, gs32, p32 = float(np.float32(alpha)), float(np.float32(gs)), float(np.float32(p))
    w = acc * a32 + (bias.double() if e.bias else 0.0)
    w = torch.relu(w) if e.relu else w
    if e.drop:
        thr = drop_threshold(p32)
        scale = float(np.float32(65536.0 / (65536.0 - thr)))
        w = w * torch.from_numpy(keep_mask(9, p32, M, N)).double() * scale
        assert (thr, scale) == ((32768, 2.0) if cls == "S" else (6554, scale)) and 1.0 < scale <= 2.0
    w = w + (res.double() if e.residual else 0.0)
    if e.gate:
        w = w * (gate.double() > 0) * gs32
    assert torch.equal(v + 0.0, w + 0.0)
    assert torch.equal(cf + 0.0, (w + (cf0.double() if e.accumulate else 0.0)) + 0.0)


# ---------------------------------------------------------- precondition
def _on_grid(t, grid):
    m = t.double() / grid
    return bool((m == m.round()).all()) and torch.equal(t.double(), t.bfloat16().double())


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_exact_precondition(case):
    """Every exact case of the table stays within 2**22 grid units: S from
    64 K (analytic), F from |A| @ |B|^T; its values are on the grid and exact
    in bf16; a case without room for Cf0 lists no accumulating run."""
    assert G.s_units(case) <= G.EXACT_LIMIT, (case.id, G.s_units(case))
    if not case.exact_cf0:
        assert not any(G.EPI[r.epi].accumulate for r in case.runs)
    for cls in G.classes(case):
        ins = G.inputs(case, cls)
        lim = 8 if cls == "S" else 255 * 2.0 ** -7
        for t in (ins.A, ins.B):
            assert _on_grid(t, 1.0 if cls == "S" else 2.0 ** -7) and t.abs().max() <= lim
        q = G.EPI_SCALE[cls]
        assert _on_grid(ins.bias, q) and _on_grid(ins.residual, q) and _on_grid(ins.cf0, q) and _on_grid(ins.gate, 1)
        assert ins.bias.abs().max() <= 16 * q and ins.residual.abs().max() <= 64 * q and ins.cf0.abs().max() <= 64 * q
        if case.M * case.N >= 64:
            assert (ins.gate > 0).any() and (ins.gate < 0).any() and (ins.gate == 0).any()
        if cls == "F":
            units = G.exact_units(case, cls)
            print("%s F: %.0f of %d grid units" % (case.id, units, G.EXACT_LIMIT))
            assert units <= G.EXACT_LIMIT, (case.id, units)
            if case.K >= 64:
                assert ((ins.A.double() * 128).long() % 2 == 1).any()  # odd m: all eight mantissa bits live
        elif case.flop <= G.F_CLASS_FLOP:
            assert G.exact_units(case, cls) <= G.s_units(case)


# -------------------------------------------------------- dispatch mirror
def _names(label):
    return label.split("+")


def test_every_kernel_is_reached():
    seen = set()
    for case in G.CASES:
        for run in case.runs:
            seen.update(_names(G.label(case, run, CUS)))
    table = set(G.KERNEL_NAMES) - set(G.F8_KERNEL_NAMES)
    assert seen == table, (table - seen, seen - table)
    rseen = set()
    for cid, run in G.R_RUNS:
        rseen.update(_names(G.label(G.BY_ID[cid], run, CUS)))
    assert rseen == table, table - rseen
    # the e4m3 kernels: each named by some plan-only case, so no branch of plan_f8 goes unmirrored
    f8seen = set()
    for case in G.F8_CASES:
        f8seen.update(_names(G.f8_mirror(case, CUS).name))
    assert len(G.F8_KERNEL_NAMES) == 7 and f8seen == set(G.F8_KERNEL_NAMES) | {"splitk_reduce"}, f8seen


def test_f8_table_edges():
    """The splits and grids the comments of gemmref.F8_CASES claim."""
    by = {c.id: c for c in G.F8_CASES}
    plan = lambda cid, cus=CUS: G.f8_mirror(by[cid], cus)  # noqa: E731
    assert [plan(c).name for c in ("f8-stream", "f8-g256s-K256", "f8-g256s-K128", "f8-bf16-switch")] == \
        ["f8_stream", "f8_g256s", "f8_stream", "f8_stream"]
    assert plan("f8-q8-fast0").name == "f8_q8_generic" and plan("f8-fast0-no-copy").name == "f8_stream"
    for cus in (64, 256, 304):
        below, at, above = {64: (63, 64, 65), 256: (255, 256, 257), 304: (303, 304, 305)}[cus]
        assert [plan("f8-tiles%d" % t, cus).grid for t in (below, at, above)] == [below, at, cus]
        assert [plan("f8w-tiles%d" % t, cus).grid for t in (below, at, above)] == [below, at, cus]
    assert (plan("f8w-T64").split, plan("f8w-depth").split, plan("f8w-ws").split) == (1, 4, 2)
    p = plan("f8w-partials")
    assert (p.split, p.kchunk) == (3, 2752)   # M * N + M floats per slice would give (4, 2048)
    assert plan("f8w-64slices").split == 64 and plan("f8w-64slices", 64).split == 64
    assert [(plan("f8w-wg%d" % w).split, plan("f8w-wg%d" % w).grid) for w in (4, 8, 100, 1000)] == \
        [(1, 8), (1, 8), (11, 99), (16, 144)]
    assert plan("f8w-wg100-over").grid == 96
    assert plan("f8w-no-ws").split == plan("f8w-tickets-only").split == 1


@pytest.mark.parametrize("edge", G.NOT_EDGES, ids=lambda e: e[0])
def test_not_edges(edge):
    cid, neighbour, epi = edge
    a, b = G.BY_ID[cid], G.BY_ID[neighbour]
    la = {G.label(a, r, CUS) for r in a.runs if r.epi == epi and not r.max_wg}
    lb = {G.label(b, r, CUS) for r in b.runs if r.epi == epi and not r.max_wg}
    assert la and lb and not (la & lb), (la, lb)


def test_table_edges_at_256_cus():
    """The grid and split arithmetic the table's comments claim."""
    lab = lambda cid, i=0: G.label(G.BY_ID[cid], G.BY_ID[cid].runs[i], CUS)  # noqa: E731
    assert lab("sk-80x1536x512") == "skinny_m16_kf" and lab("sk-81x1536x512") == "skinny_s64_kf"
    assert 96 * 5 <= 2 * CUS < 96 * 6
    assert lab("g256-4096x4096x64") == "g256_stream" and lab("g256not-3840x4096x64") == "gemm64"
    assert lab("g256-4100x4096x128") == "g256_generic" and lab("g256s-NN-4096x4096x128") == "g256s"
    assert lab("w-512x512x2056") == "g128_reg+splitk_reduce" and lab("w-512x512x4160") == "g128_glds+splitk_reduce"
    assert lab("w-201x309x2048") == "g128_glds" and lab("w-200x309x2048") == "g128_glds+splitk_reduce"
    assert lab("w256-768x768x11328") == "wgrad256s+splitk_reduce"
    assert lab("w256-two-768x768x11328") == lab("w256-776x768x11328") == "wgrad256+splitk_reduce"
    assert lab("w256-4096x4096x64") == "wgrad256s" and lab("w256not-1536x768x4096") == "g128_glds+splitk_reduce"
    # the strided frames keep e.vec where N % 8 == 0 and break it in "odd" and with an offset bias
    c = G.BY_ID["sk-16x512x512"]
    assert [G.epi_flags(c, r).vec for r in c.runs] == [True] * 7 + [False, True, False]


def _library():
    """libsmer_hip.so; skips only where it is not built or cannot be loaded
    without a GPU."""
    import os
    from smer_music_generation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libsmer_hip.so is not built")
    try:
        return L.load()
    except OSError as e:
        if torch.cuda.is_available():
            raise
        pytest.skip("libsmer_hip.so does not load without a GPU: %s" % e)


def _setenv(monkeypatch, env):
    for k in G.ENV_SWITCHES:
        monkeypatch.setenv(k, env[k]) if k in env else monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("ncus", [64, 256, 304])
def test_plan_matches_mirror(monkeypatch, ncus):
    """The library's dispatch (smer_gemm_plan with an explicit CU count: no
    HIP call, nothing launched) and the mirror agree on every (case, run) of
    the table, split-K slices and depth included, and on every plan-only
    e4m3 case (gemmref.F8_CASES), grid and LDS bytes included.
    tests/test_gemm_edges_gpu.py runs the same comparison on the device."""
    lib = _library()
    setenv = lambda env: _setenv(monkeypatch, env)  # noqa: E731
    names = [lib.smer_gemm_kernel_name(i) for i in range(len(G.KERNEL_NAMES) + 1)]
    assert names == [n.encode() for n in G.KERNEL_NAMES] + [None]
    bad = G.plan_mismatches(lib, ncus, setenv)
    assert not bad, bad


def test_f8_persistent_grid_is_a_multiple_of_eight(monkeypatch):
    """64, 256 and 304 are multiples of 8, so the rounding of the e4m3
    products' persistent grids shows only at another CU count: 100."""
    lib = _library()
    _setenv(monkeypatch, {})
    grids = {True: set(), False: set()}
    for case in G.F8_CASES:
        if case.id.startswith(("f8-tiles", "f8w-tiles")):
            m = G.f8_mirror(case, 100)
            l = G.library_plan_f8(lib, case.fwd, case.M, case.N, case.K, cus=100, **case.facts)
            assert vars(m) == vars(l), (case.id, vars(m), vars(l))
            grids[case.fwd].add(l.grid)
    assert grids[True] == grids[False] == {63, 64, 65, 96}


# --------------------------------------------------------------- frames
def test_buf_frames():
    d = torch.arange(12.0).view(3, 4)
    b = G.Buf(d, 7, offset=1)
    b.dev = b.flat.clone()
    assert torch.equal(b.view(), d) and b.view().stride() == (7, 1) and b.view().storage_offset() == 1
    inner, rest = b.parts()
    assert torch.equal(inner, d) and rest.numel() == 1 + 5 * 7 - 12 and torch.isnan(rest).all()
    for case in G.CASES:
        for w in "AB":
            ld = case.a_ld if w == "A" and case.a_ld is not None else G.in_ld(case, w)
            kc = case.ak if w == "A" else case.bk
            assert ld > (case.K if kc else G.round_up(case.M if w == "A" else case.N, 8) - 1)
        for r in case.runs:
            ld = G.lds_of(case, r)
            assert len({ld["ldr"], ld["ldg"], ld["ldc"]}) == 3 and len({ld["ldr"], ld["ldg"], ld["ldcf"]}) == 3


# -------------------------------------------------------------- R bound
@pytest.mark.parametrize("cid,run", G.R_RUNS, ids=["%s-%s" % (c, G.run_id(r)) for c, r in G.R_RUNS])
def test_r_bound_holds_fp32_torch(cid, run):
    """The same product in fp32 torch on the CPU, through the same epilogue,
    stays within the class R bound of the float64 reference."""
    case = G.BY_ID[cid]
    ins = G.inputs(case, "R")
    prod, sabs = G.product64(case, "R")
    ref = G.reference(case, "R", run, prod)
    bound = G.r_bound(case, run, ref, sabs)
    p32 = (ins.A.float() @ ins.B.float().t()).double()
    got = G.reference(case, "R", run, p32)
    for name, g, r, b in (("C", got.v, ref.v, bound.C), ("Cf", got.cf, ref.cf, bound.Cf)):
        if r is None:
            continue
        g = G.to_dtype(g, case.dtype if name == "C" else G.F32).double()
        worst = ((g - r).abs() / (b + 1e-300)).max().item()
        print("%s %s: fp32 torch error / bound = %.3g" % (cid, name, worst))
        assert worst <= 1.0
    if ref.db is not None:
        d32 = ins.A.float().sum(1).double() + (ref.use.db0.double() if ref.use.db0 is not None else 0.0)
        assert ((d32 - ref.db).abs() <= bound.db).all()

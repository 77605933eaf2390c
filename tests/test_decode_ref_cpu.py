"""tests/decoderef.py checked on the CPU: the float64 reference against
torch.softmax, the fp32 emulation against the reference within the bounds,
the constants against a fresh measurement, the coverage of variant_of, the
exact-input constructions (needle, decoy, census) on the emulation, and the
sensitivity of those checks to five mutations of the emulated kernel."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import decoderef as R

BF16, F32 = R.BF16, R.F32

# one case per distinct arithmetic (label, head dim, capacity): the shared
# kernels and the query-prologue forms run attn_decode_vec_kernel's arithmetic
# per row (decode_attn_emulated takes the query as given)
ARITH = {}
for _c in R.CASES:
    _l = R.parse_label(_c.label)
    _key = (_c.dtype, _c.D, _c.cap, _l[:3] if _l else None, _l[3] if _l else 0, _c.lay == "skew")
    ARITH.setdefault(_key, _c)
ARITH = list(ARITH.values())


def _launch(case, kind):
    """(q, kc, vc, nk, req, lay, scale) of the case's launch on `kind` data."""
    nk, req, tab, live, n_slots = R.rows_of(case)
    lay = R.make_layout(case, n_slots)
    if kind == "parity":
        q, K, V, scale = R.data_parity(case, n_slots, len(nk))
    elif kind == "decoy":
        q, K, V, scale = R.data_decoy(case, n_slots, len(nk), nk)
    else:
        q, K, V, scale = R.data_census(case, n_slots, len(nk))
    kc, vc = R.pack_cache(K, V, lay, case.dtype)
    return q.to(case.dtype), kc, vc, nk, req, lay, scale, live


def _emulate(case, L, mutate=None, rows=None):
    q, kc, vc, nk, req, lay, scale, live = L
    lab = case.label
    if case.entry in ("shared", "shared_qln"):   # per row the per-row kernel's arithmetic, no row permutation
        rows = [int(i) for i in np.nonzero(live)[0]]   # (rows of no group are not served)
    return R.decode_attn_emulated(q, kc, vc, req, nk, lay, scale, lab, case.dtype, mutate=mutate, rows=rows)


@pytest.mark.parametrize("lay", ["side", "head", "skew"])
def test_reference_is_softmax(lay):
    case = R._mk("x", "decode", F32, 24, lay, 50, 6, 3, "generic f32")
    g = torch.Generator().manual_seed(5)
    K, V = torch.randn(3, 50, 3, 24, generator=g), torch.randn(3, 50, 3, 24, generator=g)
    q = torch.randn(6, 72, generator=g)
    L = R.make_layout(case, 3)
    kc, vc = R.pack_cache(K, V, L, F32)
    nk, req = np.array([0, 1, 7, 49, 50, 33]), np.array([0, 1, 2, 0, 1, 2])
    r = R.decode_attn_ref64(q, kc, vc, req, nk, L, 0.3)
    for i in range(6):
        n, s = int(nk[i]), int(req[i])
        for h in range(3):
            sl = slice(24 * h, 24 * h + 24)
            if n == 0:
                assert r.O[i, sl].abs().max() == 0 and r.lse[i, h] == -math.inf
                continue
            sc = (K[s, :n, h].double() @ q[i, sl].double()) * R.f32r(0.3)
            p = torch.softmax(sc, 0)
            assert torch.allclose(r.O[i, sl], p @ V[s, :n, h].double(), rtol=1e-12, atol=1e-14)
            assert torch.allclose(r.T[i, sl], p @ V[s, :n, h].double().abs(), rtol=1e-12, atol=1e-14)
            assert abs(r.lse[i, h] - torch.logsumexp(sc, 0)) < 1e-12
    # split partials recombine to the whole
    part = torch.zeros(6, 3, 8, 4 + 24, dtype=torch.float64)
    part[..., 0] = -math.inf
    for z in range(8):
        lo = np.array([R.split_chunks(int(n))[z][0] for n in nk])
        hi = np.array([R.split_chunks(int(n))[z][1] for n in nk])
        rz = R.decode_attn_ref64(q, kc, vc, req, hi, L, 0.3, lo=lo)
        part[:, :, z, 0], part[:, :, z, 1], part[:, :, z, 4:] = rz.m, rz.l, rz.acc.view(6, 3, 24)
    assert torch.allclose(R.split_merge_ref64(part).view(6, 72), r.O, rtol=1e-12, atol=1e-14)


def test_variant_coverage():
    """The mirror alone (no library): over decoderef.decode_queries() the
    reachable instantiations are exactly the case labels (and skln_label's
    over K exactly those of SKLN_K); variant_of gives every case its label and
    every case holds its kernel's edge key counts; each threshold of the
    dispatch flips the label exactly between its two neighbouring grid values."""
    qs = R.decode_queries()
    assert {R.variant_of(*q).label for _, q in qs} == {c.label for c in R.CASES}
    assert ({R.skln_label(K, kf) for K in range(8, 2049, 8) for kf in (True, False)}
            == {R.skln_label(K) for K in R.SKLN_K})
    assert {R.skln_label(K, False) for K in range(8, 2049, 8)} == {"skln U2 NC4", "skln U4 NC4"}
    for c in R.CASES:
        nk = R.rows_of(c)[0]
        assert R.variant_of(*R.case_query(c)).label == c.label, c.id
        # every launch holds every edge key count of its kernel
        assert set(R.edge_nkeys(c)) <= set(int(x) for x in nk), c.id
    # thresholds: along each axis of the grid, the label changes between these
    # neighbours and between no others
    lab = {key: R.variant_of(*q).label for key, q in qs}
    few_off = {key: R.variant_of(*q, switches=dict(R.SWITCH_DEFAULTS, SMER_DEC_PIPE_SMALL=False)).label for key, q in qs}
    for (entry, dtype, D, cap, blocks, dm, ok), l in lab.items():
        vec = ok and (D // (8 if dtype == BF16 else 4) in (4, 8, 16)) and D % (8 if dtype == BF16 else 4) == 0
        split, qln = entry.startswith("split"), entry.endswith("qln")
        i = R.GRID_CAP.index(cap)
        if i:   # capacity: 511 | 512 (not the prologue entries), 2047 | 2048
            flips = vec and not split and ((cap == 512 and not qln) or (cap == 2048 and (blocks > 128 or qln)))
            assert (l != lab[(entry, dtype, D, R.GRID_CAP[i - 1], blocks, dm, ok)]) == flips, (entry, D, cap, blocks)
        if blocks == 129:   # blocks: 128 | 129 for big caches below the pipelined capacity
            flips = vec and not split and not qln and 512 <= cap < 2048
            assert (l != lab[(entry, dtype, D, cap, 128, dm, ok)]) == flips, (entry, D, cap)
            assert few_off[(entry, dtype, D, cap, 128, dm, ok)] == l   # the switch takes the few-blocks term out
        if entry == "decode":   # the vector layout and the lanes per key
            assert l.startswith("vec" if vec else "generic"), (dtype, D, ok)
        if dm:
            assert ("q%d" % dm) in l


def test_plan_matches_mirror(monkeypatch):
    """The library's dispatch (smer_attn_decode_plan, smer_linear_decode_ln_plan:
    no HIP call, nothing launched) and the mirror agree on label, grid, block,
    LDS bytes and the odd-rows-first flag at every case and grid point, at the
    defaults and with each of the three switches off.  Skips only where
    libsmer_hip.so is not built or cannot be loaded without a GPU;
    tests/test_decode_edges_gpu.py runs the same comparison on the device."""
    from smer_music_generation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libsmer_hip.so is not built")
    try:
        lib = L.load()
    except OSError as e:
        if torch.cuda.is_available():
            raise
        pytest.skip("libsmer_hip.so does not load without a GPU: %s" % e)

    def setenv(env):
        for k in R.ENV_SWITCHES:
            monkeypatch.setenv(k, env[k]) if k in env else monkeypatch.delenv(k, raising=False)

    bad = R.plan_mismatches(lib, setenv)
    assert not bad, bad[:10]


@functools.lru_cache(maxsize=None)
def _measure(cid, kind):
    """(dtype tag, worst ratio, all within bound) of the emulation against
    float64 on one launch: bf16 |err| / (T + |ref|), fp32 |err| / bound."""
    case = R.case_by_id(cid)
    L = _launch(case, kind)
    q, kc, vc, nk, req, lay, scale, live = L
    ns = (R.parse_label(case.label) or (0, 0, 0, 0))[3]
    ref = R.decode_attn_ref64(q, kc, vc, req, nk, lay, scale)
    em = torch.from_numpy(_emulate(case, L)).double()
    if ns:
        em = R.split_merge_ref64(em).view(len(nk), -1)
    lv = torch.from_numpy(live)
    em, ref.O, ref.T, ref.S, ref.X = em[lv], ref.O[lv], ref.T[lv], ref.S[lv], ref.X[lv]
    nk = nk[live]
    err = (em - ref.O).abs()
    assert torch.isfinite(em).all()
    bound = R.o_bound(case, ref, nk)
    if case.dtype == BF16:
        return "O", (err / (ref.T + ref.O.abs() + 1e-300)).max().item(), bool((err <= bound).all())
    return "f32", (err / (bound + 1e-300)).max().item(), bool((err <= bound).all())


@pytest.mark.parametrize("case", ARITH, ids=lambda c: c.id)
@pytest.mark.parametrize("kind", ["parity", "decoy"])
def test_emulation_within_bounds(case, kind):
    """The emulation against float64: fp32 within a quarter of its bound,
    bf16 within DEC_REL_O * T + 2**-8 |ref|."""
    tag, ratio, ok = _measure(case.id, kind)
    assert ok
    if tag == "f32":
        assert ratio <= 0.25, ratio


def test_constants():
    """DEC_WORST is the fresh measurement (to 3 digits) over every case and
    data kind; the constants are four times it."""
    res = [_measure(c.id, kind) for c in ARITH for kind in ("parity", "decoy")]
    wo = max(r for t, r, _ in res if t == "O")
    wf = max(r for t, r, _ in res if t == "f32")
    print("measured worst: bf16 O %.6f   fp32 error / bound %.4f" % (wo, wf))
    assert abs(wo - R.DEC_WORST["O"]) <= 0.005 * wo, (wo, R.DEC_WORST)
    assert R.DEC_REL_O == 4 * R.DEC_WORST["O"]
    assert wf <= 0.25


# ------------------------------------------------------ exact constructions
def _needle_fails(case, mutate=None, nks=None):
    """Number of needle rows whose emulated output is not V[p] bit for bit."""
    bad = tot = 0
    for nk in (nks or [n for n in R.edge_nkeys(case) if n > 0]):
        pos = R.needle_positions(case, nk)
        for b in range(0, len(pos), R.needle_rows(case)):
            pp = pos[b:b + R.needle_rows(case)]
            d = R.needle_launch(case, nk, pp)
            K, V, scale, want = d.K, d.V, d.scale, d.want
            lay = R.make_layout(case, 3)
            kc, vc = R.pack_cache(K, V, lay, case.dtype)
            n = len(d.req)
            nkv = np.full(n, nk, np.int32)
            if case.dmodel:   # the query as the prologue forms it
                y, gamma, beta, wq, bq = d.qln
                q = R.emulate_qln(y, gamma, beta, 1e-5, wq, bq, case.H, case.D, case.dtype, nkv)[1]
            else:
                q = d.q.to(case.dtype)
            em = R.decode_attn_emulated(q, kc, vc, d.req, nkv,
                                        lay, scale, case.label, case.dtype, mutate=mutate,
                                        rows=None if mutate == "odd_first_q" else list(range(n)))
            if R.parse_label(case.label) and R.parse_label(case.label)[3]:
                em = R.split_merge_ref64(em).view(n, -1).float().numpy()
            bad += int((torch.from_numpy(em).view(torch.int32) != want.float().view(torch.int32)).any(1).sum())
            tot += n
    return bad, tot


def _census_fails(case, mutate=None):
    L = _launch(case, "census")
    nk = L[3]
    em = torch.from_numpy(_emulate(case, L, mutate, rows=None if mutate == "odd_first_q" else list(range(len(nk)))))
    if R.parse_label(case.label) and R.parse_label(case.label)[3]:
        em = R.split_merge_ref64(em).view(len(nk), -1)
    want = R.census_expected(case, nk)
    lv = torch.from_numpy(L[7])
    return int((~((em.double() - want).abs() <= R.census_bound(want, case.dtype)))[lv].sum())


def _decoy_fails(case, mutate=None):
    L = _launch(case, "decoy")
    q, kc, vc, nk, req, lay, scale, live = L
    ref = R.decode_attn_ref64(q, kc, vc, req, nk, lay, scale)
    em = torch.from_numpy(_emulate(case, L, mutate, rows=None if mutate == "odd_first_q" else list(range(len(nk)))))
    if R.parse_label(case.label) and R.parse_label(case.label)[3]:
        em = R.split_merge_ref64(em).view(len(nk), -1)
    return int((~((em.double() - ref.O).abs() <= R.o_bound(case, ref, nk)))[torch.from_numpy(live)].sum())


EXACT = [c for c in ARITH if c.cap in (300, 600) or c.entry == "split"] + [
    R.case_by_id(i) for i in ("qln-dm512-cap600", "shq-dm768-cap600", "qln-dm1024-cap2100", "splitq-cap600")]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.id)
def test_exact_constructions_hold_on_the_emulation(case):
    """Needle: the output is V[p] bit for bit (the rest of the row weighs
    <= 4096 e**-40 * 4, below half an fp32 ulp of a value >= 1); census: within
    2 fp32 ulp (+ the bf16 rounding) of count / nk.  Both follow from the
    arithmetic, not from a kernel run."""
    assert 4096 * 4 * math.exp(-40) < 2.0 ** -25
    bad, tot = _needle_fails(case)
    assert bad == 0 and tot > 0, (bad, tot)
    if not case.dmodel:   # (census data is the same for the prologue entries: q = 0)
        assert _census_fails(case) == 0


# ---------------------------------------------------------------- mutations
MUT_CASES = [R.case_by_id(i) for i in ("dec-bf16-D64-cap300", "dec-f32-D64-cap600-few", "dec-bf16-D64-cap2100")]


def _old_test_passes(mutate, cap, dtype):
    """test_kernels_gpu.py::test_decode_attention's data and criterion (N(0,1)
    inputs, scale 0.125, 5 rows, rel_err < 1e-2 / 1e-5 against fp32 softmax)
    applied to the (mutated) emulation."""
    H, D = 4, 64
    g = torch.Generator().manual_seed(0)
    K, V = torch.randn(3, cap, H, D, generator=g), torch.randn(3, cap, H, D, generator=g)
    q = torch.randn(5, H * D, generator=g).to(dtype)
    case = R._mk("old", "decode", dtype, D, "side", cap, 5, H, R.variant_of(
        "decode", dtype, D, H * D, cap * H * D, 0, H * D, H * D, cap, 5, H).label)
    lay = R.make_layout(case, 3)
    kc, vc = R.pack_cache(K, V, lay, dtype)
    req, nk = np.array([0, 1, 1, 2, 2]), np.array([1, 17, 18, cap, 64])
    em = torch.from_numpy(R.decode_attn_emulated(q, kc, vc, req, nk, lay, 0.125, case.label, dtype, mutate=mutate))
    ref = R.decode_attn_ref64(q, kc, vc, req, nk, lay, 0.125).O
    rel = ((em.double() - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    return rel < (1e-2 if dtype == BF16 else 1e-5), rel


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_mutations_are_caught(mutate):
    """Each mutation of the emulated kernel fails the needle, decoy or census
    check at the case table's shapes.  The guard mutations (j <= nk, j < nk - 1)
    sit in the last unrolled slot, `drop_wave` leaves the last wave out of the
    LDS merge, `rescale_per_key` applies the step's rescale factor once per
    key of the step, `odd_first_q` permutes row_nkeys / the cache / the output
    row but reads the query of the unpermuted row."""
    caught = {}
    for case in MUT_CASES:
        n = _needle_fails(case, mutate)[0]   # (its launches have even and odd row counts)
        caught[case.id] = (n, _decoy_fails(case, mutate), _census_fails(case, mutate))
    print(mutate, caught)
    assert caught and all(any(v) for v in caught.values()), caught


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_old_criterion_on_mutations(mutate):
    """The norm-wise rel_err < 1e-2 criterion of test_decode_attention on data
    of that test's distribution (N(0,1), scale 0.125, its 5 rows; bf16, both
    capacities), applied to each mutated emulation.  It is blind to the
    unpermuted query (5 rows: the permutation is off): asserted.  The other
    outcomes are printed, not asserted: one key too many or too few moves a
    300 / 1000-key row by 0.4 % .. 4 % in norm depending on that key's score
    (3.8 % / 2.1 % for j <= nk on this draw), so that criterion catches it
    only by the luck of the draw; a wave left out and the per-key rescale
    move a row far more."""
    res = {cap: _old_test_passes(mutate, cap, BF16) for cap in (300, 1000)}
    print(mutate, res)
    if mutate == "odd_first_q":
        assert all(ok for ok, _ in res.values()), res

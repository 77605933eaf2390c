"""float64 reference, fp32 emulation, cases and bounds of the decode kernels
(csrc/attention.hip: smer_attn_decode, _qln, _shared, _shared_qln, _split_f32,
_split_qln_f32, smer_kv_scatter, _heads; csrc/gemm.hip: smer_linear_decode_ln,
_ln_f32, smer_linear_decode_merge_f32).  Plain torch / numpy on the CPU;
tests/test_decode_ref_cpu.py checks this file and measures the constants
below, tests/test_decode_edges_gpu.py holds the kernels to them.

Convention: a row with no key has O = 0 (every kernel codes l > 0 ? 1/l : 0),
its log-sum-exp is -inf.  A key slice with no key has the partial record
m = -inf, l = 0, acc = 0.

Bound rule.  Every output element is compared with the float64 value computed
from the bits the kernel read, against a bound of that element; no element is
skipped.  T = sum_j p_j |v_jd| is the summed magnitude of the element's terms.

* fp32 kernels: (k + 2 + E) * 2**-24 * T, k = nk + D the number of accumulated
  terms (nk weighted values behind a D-term score) and
      E = 2 * ((D + 2) * S + 1.25 * X + 2 * links).
  A weight is p_j = e_j / l, e_j the product of the fast exponentials on key
  j's path (its own step, every later rescale of its lane group, the group
  merges, the wave merge).  Their arguments are all <= 0 and telescope to
  s_j - m, so their magnitudes sum to |s_j - m| <= X, the largest |s - m| of
  the row.  __expf(x) is exp2(fl(x * log2e)): the rounded product moves the
  exponent by |x log2e| 2**-24, i.e. the result by |x| 2**-24 relative, and
  the fp32 log2e constant is off by 0.24 * 2**-24 relative, another
  0.24 |x| 2**-24: 1.25 X in all.  Each of the `links` exponentials
  (key steps + log2(groups per wave) + 2) adds one ulp of exp2 and one
  rounded multiply: 2 * links.  The fp32 score carries the any-order error
  (D + 2) 2**-24 S, S = max_j scale sum_d |q_d k_jd| (D products, the scale
  multiply), which enters e_j as a relative error of the same size.  The
  factor 2: l carries the same errors as the numerator.  The partial records
  of the split kernel have no division: E / 2 there.
* bf16 kernels: DEC_REL_O * T + 2**-8 * |ref|.  DEC_REL_O is four times the
  worst |decode_attn_emulated - decode_attn_ref64| / (T + |ref|) over CASES,
  measured by tests/test_decode_ref_cpu.py (which prints it); never tuned
  against a kernel's output.  The fp32 rule is checked the same way: the fp32
  emulation stays within a quarter of its bound on every case.
* LayerNorm outputs (x_out): from the training-tail suite's statistics bounds
  (tests/test_train_ops_gpu.py: mean to (N + 2) 2**-24 sum|x| / N, rstd to
  (N / 2 + 8) 2**-24 rstd) propagated through y = (x - mu) rs g + b:
      |g| (dmu rs + |x - mu| drs) + 3 * 2**-24 (|(x - mu) rs g| + |b|)
  (+ 2**-8 |ref| for the bf16 store).  No new constant.
* Linear products: gemmref's any-order rule, (K + 8) 2**-24 T (+ 2**-8 |ref|
  for a bf16 store), T the summed magnitude of the output's terms, evaluated
  at the LayerNorm output as the kernel rounds it.

decode_attn_emulated is the kernels' algorithm in numpy fp32, operation for
operation (key-to-lane-group assignment, one rescale per UNR keys, exp as
float32(exp2(float32(x * log2e))), group merge in xor order, wave merge in
wave order, the * inv multiply, bf16 rounding of the stored output).  An fma
is taken in float64 and rounded once; where the compiler is free to contract
a * b + c the emulation contracts.  It derives the constants and justifies
the exact-input tests; no kernel is ever compared with it as a pass criterion.
"""
import math
import re
import zlib
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24
UB = 2.0 ** -8
LOG2E_F = np.float32(1.4426950408889634)
SENT = 123.0   # sentinel of the pad columns (exact in bf16)
DEC_SHARED_G = 4
DEC_SPLITS = 8
f32 = np.float32

# Worst |emulated - ref64| / (T + |ref|) of the bf16 output over CASES (parity
# and decoy data), measured by tests/test_decode_ref_cpu.py::test_constants
# (it prints them); and the worst fp32 emulation error / bound (must stay
# below 0.25):
#   bf16 O 0.001943   fp32 error / bound 0.0148
DEC_WORST = dict(O=1.943e-3)
DEC_REL_O = 4 * DEC_WORST["O"]


def f32r(x):
    """A Python scalar as a C `float` parameter holds it."""
    return float(np.float32(x))


def bf16r_np(x):
    """fp32 numpy -> bf16 (nearest even) -> fp32 numpy."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


# ------------------------------------------------------------------ variants
def label(kind, dtype=None, L=0, Un=0, W=0, pipe=False, qp=0, ns=0):
    if kind == "generic":
        return "generic %s" % ("bf16" if dtype == BF16 else "f32")
    head = "shared" if kind == "shared" else "vec %s" % ("bf16" if dtype == BF16 else "f32")
    s = "%s L%d U%d W%d" % (head, L, Un, W)
    if pipe:
        s += " pipe"
    if qp:
        s += " q%d" % qp
    if ns:
        s += " ns%d" % ns
    return s


ENTRIES = ("decode", "qln", "shared", "shared_qln", "split", "split_qln")   # smer_attn_decode_plan's entry ids
ENTRY_DTYPE = dict(qln=BF16, shared=BF16, shared_qln=BF16, split=F32, split_qln=F32)   # (decode takes both)
ENV_SWITCHES = ("SMER_DEC_PIPE_SMALL", "SMER_DECODE_ODD_FIRST", "SMER_SKINNY_KF")
SWITCH_DEFAULTS = dict.fromkeys(ENV_SWITCHES, True)
# what an entry launches: the instantiation as a label, the grid, the block,
# the generic kernel's LDS bytes, the odd-rows-first argument
Variant = namedtuple("Variant", "label grid block lds odd")


def variant_of(entry, dtype, D, row_stride, req_stride, head_stride, ldq, ldo, cap, n_rows, H, dmodel=0,
               n_groups=0, switches=SWITCH_DEFAULTS, aligned=True):
    """What an entry point launches: a Python mirror, written independently,
    of the decode dispatch of csrc/attn_plan.h (attn_decode_plan: smer_attn_decode,
    _qln, _shared, _shared_qln and the two split entries).  It is held against
    the library's own answer (library_variant, smer_attn_decode_plan) at every
    case and over decode_queries() by tests/test_decode_ref_cpu.py and, on the
    device, tests/test_decode_edges_gpu.py.

    `switches`: the values of ENV_SWITCHES (True = on, the default):
    SMER_DEC_PIPE_SMALL=0 turns the pipelined form off for small grids,
    SMER_DECODE_ODD_FIRST=0 the row permutation, SMER_SKINNY_KF=0 the K-full
    forms of the LayerNorm-prologue Linear (skln_label).  `aligned`: q, the
    caches and o are 16-B aligned."""
    dtype = ENTRY_DTYPE.get(entry, dtype)
    if head_stride <= 0:
        head_stride = D
    cap_rows = (head_stride if head_stride != D else req_stride) // max(row_stride, 1)
    assert cap_rows == cap, (cap_rows, cap)
    if entry in ("split", "split_qln"):
        return Variant(label("vec", F32, 16, 2, 4, True, 512 if entry == "split_qln" else 0, DEC_SPLITS),
                       (H, n_rows, DEC_SPLITS), 256, 0, 0)
    odd = int(switches["SMER_DECODE_ODD_FIRST"])
    shared_grid = (H, n_rows // DEC_SHARED_G + n_groups)
    if entry == "qln":
        return Variant(label("vec", BF16, 8, 4, 8, cap_rows >= 2048, dmodel), (H, n_rows), 512, 0, odd)
    if entry == "shared_qln":
        return Variant(label("shared", None, 8, 4, 8, cap_rows >= 2048, dmodel), shared_grid, 512, 0, 0)
    big = cap_rows >= 512
    pipe = cap_rows >= 2048 or (big and n_rows * H <= 128 and switches["SMER_DEC_PIPE_SMALL"])
    Un, W = (4, 8) if big else (2, 4)
    if entry == "shared":
        return Variant(label("shared", None, D // 8, Un, W, pipe), shared_grid, 64 * W, 0, 0)
    assert entry == "decode"
    vec = 8 if dtype == BF16 else 4
    ok = (aligned and D % vec == 0 and ldq % vec == 0 and ldo % vec == 0 and row_stride % vec == 0
          and req_stride % vec == 0 and head_stride % vec == 0 and D // vec in (4, 8, 16))
    if not ok:
        return Variant(label("generic", dtype), (n_rows, H), 256, 4 * cap_rows, 0)
    return Variant(label("vec", dtype, D // vec, Un, W, pipe), (H, n_rows), 64 * W, 0, odd)


def library_variant(lib, entry, dtype, D, row_stride, req_stride, head_stride, ldq, ldo, cap, n_rows, H, dmodel=0,
                    n_groups=0, aligned=True):
    """The library's own decision for the same call (smer_attn_decode_plan:
    the attn_decode_plan the launchers run; nothing is launched, no HIP call),
    in the form of variant_of; the switches are the environment's.  The plan
    query takes smer_attn_decode's "vector layout ok" fact as a flag: it is
    formed here from the strides and `aligned` as the launcher forms it from
    the call's strides and pointers."""
    import ctypes
    dtype = ENTRY_DTYPE.get(entry, dtype)
    vec = 8 if dtype == BF16 else 4
    vec_ok = aligned and all(x % vec == 0 for x in (ldq, ldo, row_stride, req_stride, max(head_stride, 0)))
    out = (ctypes.c_int * 14)()
    rc = lib.smer_attn_decode_plan(ENTRIES.index(entry), 1 if dtype == BF16 else 0, D, n_rows, H, n_groups, dmodel,
                                   row_stride, req_stride, head_stride, int(vec_ok), out)
    assert rc == 0, lib.smer_last_error()
    kind, f32_, L, Un, W, pipe, qp, ns, gx, gy, gz, block, lds, odd = out
    lab = label(("generic", "vec", "shared")[kind], F32 if f32_ else BF16, L, Un, W, bool(pipe), qp, ns)
    return Variant(lab, (gx, gy) if gz == 1 else (gx, gy, gz), block, lds, odd)


def skln_label(K, skinny_kf=True):
    """smer_linear_decode_ln's instantiation of gemm_skinny_ln_kernel."""
    if K % 32 == 0 and skinny_kf:
        return "skln U2 NC1 kf" if K <= 512 else "skln U4 NC2 kf" if K <= 1024 else "skln U4 NC4 kf"
    return "skln U4 NC4" if (K + 31) // 32 > 16 else "skln U2 NC4"


def library_skln_label(lib, K, skinny_kf):
    """smer_linear_decode_ln_plan as a label; skinny_kf True / False, or None
    for the switch as the process read it."""
    import ctypes
    out = (ctypes.c_int * 3)()
    rc = lib.smer_linear_decode_ln_plan(K, -1 if skinny_kf is None else int(skinny_kf), out)
    assert rc == 0, lib.smer_last_error()
    return "skln U%d NC%d%s" % (out[0], out[1], " kf" if out[2] else "")


def parse_label(lab):
    """(L, UNR, NW, NS) of a vec / shared label; None for the generic kernel."""
    m = re.search(r"L(\d+) U(\d+) W(\d+)", lab)
    if not m:
        return None
    ns = re.search(r"ns(\d+)", lab)
    return int(m.group(1)), int(m.group(2)), int(m.group(3)), int(ns.group(1)) if ns else 0


# --------------------------------------------------------------------- cases
def _mk(cid, entry, dtype, D, lay, cap, n_rows, H, lab, dmodel=0):
    return SimpleNamespace(id=cid, entry=entry, dtype=dtype, D=D, lay=lay, cap=cap, n_rows=n_rows, H=H,
                           label=lab, dmodel=dmodel)


def _table():
    """The shape table: (entry, dtype, D, layout, cap, rows, H) and the
    instantiation the row is meant to reach.  Layouts: "side" (heads side by
    side in a key row, head_stride = D), "head" (head-major [R][2][H][cap][D])
    and "skew" (side by side with a row stride that is no multiple of the
    vector width: the generic kernel by misalignment).  Row counts are even
    (odd_first live) and odd (off) in turn."""
    c = []
    for dt, dn in ((BF16, "bf16"), (F32, "f32")):
        # the vector path takes 4, 8 or 16 lanes of 16 B per key: D = 32 / 64 /
        # 128 in bf16, 16 / 32 / 64 in fp32 (fp32 D = 128 is the generic kernel)
        for L in (4, 8, 16):
            D = L * (8 if dt == BF16 else 4)
            c.append(_mk("dec-%s-D%d-cap300" % (dn, D), "decode", dt, D, "head", 300, 12 if L != 8 else 13, 2,
                         label("vec", dt, L, 2, 4)))
            c.append(_mk("dec-%s-D%d-cap600-few" % (dn, D), "decode", dt, D, "head" if L == 4 else "side", 600,
                         13 if L != 8 else 14, 2, label("vec", dt, L, 4, 8, True)))
            c.append(_mk("dec-%s-D%d-cap600-many" % (dn, D), "decode", dt, D, "side" if L == 4 else "head", 600,
                         34 if L != 4 else 33, 4, label("vec", dt, L, 4, 8)))
            c.append(_mk("dec-%s-D%d-cap2100" % (dn, D), "decode", dt, D, "side", 2100, 12 if L == 8 else 13, 2,
                         label("vec", dt, L, 4, 8, True)))
        c.append(_mk("dec-%s-D64-cap40" % dn, "decode", dt, 64, "side", 40, 12 if dt == BF16 else 11, 3, label("vec", dt, 64 // (8 if dt == BF16 else 4), 2, 4)))
        if dt == F32:
            c.append(_mk("dec-f32-D128-cap300", "decode", dt, 128, "head", 300, 12, 2, label("generic", dt)))
        c.append(_mk("dec-%s-D24-cap300" % dn, "decode", dt, 24, "side", 300, 12, 3, label("generic", dt)))
        c.append(_mk("dec-%s-D64-skew-cap600" % dn, "decode", dt, 64, "skew", 600, 13, 2, label("generic", dt)))
    for dm in (512, 768, 1024):
        c.append(_mk("qln-dm%d-cap600" % dm, "qln", BF16, 64, "head", 600, 12 if dm != 768 else 13, 2,
                     label("vec", BF16, 8, 4, 8, False, dm), dm))
        c.append(_mk("qln-dm%d-cap2100" % dm, "qln", BF16, 64, "head", 2100, 13 if dm != 768 else 12, 2,
                     label("vec", BF16, 8, 4, 8, True, dm), dm))
        c.append(_mk("shq-dm%d-cap600" % dm, "shared_qln", BF16, 64, "head", 600, 0, 2,
                     label("shared", None, 8, 4, 8, False, dm), dm))
        c.append(_mk("shq-dm%d-cap2100" % dm, "shared_qln", BF16, 64, "head", 2100, 0, 2,
                     label("shared", None, 8, 4, 8, True, dm), dm))
    for D in (32, 64):
        c.append(_mk("sh-D%d-cap40" % D, "shared", BF16, D, "head", 40, 0, 2, label("shared", None, D // 8, 2, 4)))
        c.append(_mk("sh-D%d-cap600-few" % D, "shared", BF16, D, "head", 600, 0, 2,
                     label("shared", None, D // 8, 4, 8, True)))
        c.append(_mk("sh-D%d-cap600-many" % D, "shared", BF16, D, "head", 600, 0, 6,
                     label("shared", None, D // 8, 4, 8, False)))
        c.append(_mk("sh-D%d-cap2100" % D, "shared", BF16, D, "head", 2100, 0, 2,
                     label("shared", None, D // 8, 4, 8, True)))
    for cap in (40, 600, 2100):
        c.append(_mk("split-cap%d" % cap, "split", F32, 64, "head" if cap != 600 else "side", cap, 12 if cap != 600 else 13,
                     2, label("vec", F32, 16, 2, 4, True, 0, 8)))
        c.append(_mk("splitq-cap%d" % cap, "split_qln", F32, 64, "head", cap, 13 if cap != 600 else 12, 2,
                     label("vec", F32, 16, 2, 4, True, 512, 8), 512))
    return c


CASES = _table()
SKLN_K = (512, 1024, 2048, 264, 520)   # smer_linear_decode_ln: the three K-full forms, both guarded ones


def case_by_id(cid):
    return next(c for c in CASES if c.id == cid)


# The query grid of the dispatch: every value on either side of a threshold
GRID_D = (16, 24, 32, 64, 128)
GRID_CAP = (40, 511, 512, 600, 2047, 2048, 2100)
GRID_BLOCKS = ((64, 2), (43, 3))   # (n_rows, H): 128 and 129 blocks
GRID_DMODEL = (512, 768, 1024)


def entry_accepts(entry, dtype, D, dmodel):
    """The entry point's own argument checks: what it refuses never reaches
    the dispatch."""
    if entry == "decode":
        return dmodel == 0
    if dtype != ENTRY_DTYPE[entry]:
        return False
    if entry == "shared":
        return D in (32, 64) and dmodel == 0
    if entry == "split":
        return D == 64 and dmodel == 0
    return D == 64 and (dmodel == 512 if entry == "split_qln" else dmodel in GRID_DMODEL)


def query(entry, dtype, D, cap, n_rows, H, dmodel=0, ok=True, n_groups=3):
    """The arguments of variant_of / library_variant (without the switches) of
    a call on the side-by-side layout, or with `ok` False on the skewed one
    (a row stride that is no multiple of 16 B)."""
    case = SimpleNamespace(H=H, D=D, cap=cap, dtype=dtype, lay="side" if ok else "skew")
    lay = make_layout(case, 3)
    ld = H * D + 8
    shared = entry in ("shared", "shared_qln")
    return (entry, dtype, D, lay.row_stride, lay.req_stride, 0, ld, ld, cap, n_rows, H, dmodel, n_groups if shared else 0)


def decode_queries():
    """[(key, query)] over the grid, key = (entry, dtype, D, cap, blocks,
    dmodel, layout ok); the skewed layout for smer_attn_decode alone (the
    other entries refuse it)."""
    out = []
    for entry in ENTRIES:
        for dtype in (BF16, F32):
            for D in GRID_D:
                for dm in (0,) + GRID_DMODEL:
                    if not entry_accepts(entry, dtype, D, dm):
                        continue
                    for cap in GRID_CAP:
                        for n_rows, H in GRID_BLOCKS:
                            for ok in (True, False) if entry == "decode" else (True,):
                                out.append(((entry, dtype, D, cap, n_rows * H, dm, ok),
                                            query(entry, dtype, D, cap, n_rows, H, dm, ok)))
    return out


def case_query(case, n_rows=None, pad=8):
    """The query of a launch of the case (rows_of's row count by default)."""
    nk, req, tab, live, n_slots = rows_of(case)
    lay = make_layout(case, n_slots)
    ld = case.H * case.D + pad
    return (case.entry, case.dtype, case.D, lay.row_stride, lay.req_stride, lay.head_stride if lay.kind == "head" else 0,
            ld, ld, case.cap, len(nk) if n_rows is None else n_rows, case.H, case.dmodel, 0 if tab is None else len(tab))


SWITCH_SETS = [{}] + [{name: "0"} for name in ENV_SWITCHES]   # the defaults, then each switch off


def plan_mismatches(lib, setenv, skln_process=False):
    """Every point where the library's plan and this module's mirror differ:
    the cases and decode_queries() and, for smer_linear_decode_ln, every
    K % 8 == 0 up to 2048, under each of SWITCH_SETS (applied to the
    environment through `setenv(env)`; the read-once SMER_SKINNY_KF is passed
    to the query explicitly, and with skln_process also asked as the process
    read it, which must be the default)."""
    bad = []
    queries = [(c.id, case_query(c)) for c in CASES] + decode_queries()
    for env in SWITCH_SETS:
        setenv(env)
        sw = {name: name not in env for name in ENV_SWITCHES}
        for key, q in queries:
            m, l = variant_of(*q, switches=sw), library_variant(lib, *q)
            if m != l:
                bad.append((env, key, m, l))
        kf = sw["SMER_SKINNY_KF"]
        for K in range(8, 2049, 8):
            got = {library_skln_label(lib, K, kf)} | ({library_skln_label(lib, K, None)} if skln_process and kf else set())
            if got != {skln_label(K, kf)}:
                bad.append((env, "skln K=%d" % K, skln_label(K, kf), got))
    setenv({})
    return bad


def kpb_unr(case):
    """(keys per block step, unrolled steps) of the case's kernel; the generic
    kernel walks 256 keys per pass (its thread count)."""
    p = parse_label(case.label)
    if p is None:
        return 256, 1
    L, un, w, ns = p
    return w * (64 // L), un


def edge_nkeys(case):
    """The key counts at the edges of the case's kernel (module docstring of
    the GPU test), clipped to the capacity, ascending."""
    kpb, un = kpb_unr(case)
    e = {0, 1, kpb - 1, kpb, kpb + 1, kpb * un - 1, kpb * un, kpb * un + 1, 2 * kpb * un + 1, case.cap - 1, case.cap}
    return sorted(x for x in e if 0 <= x <= case.cap)


def shared_layout(case):
    """Rows of a shared launch: groups of 1, 2, G, G + 1 and 2G + 1 rows, a
    session-shaped group (even rows one key, odd rows live), a stray row
    between two groups and one at either end (their slot: the NaN spare one).
    Key counts walk the case's edges, so a chunk mixes long rows with short
    ones.  Returns nk, req, group table, in_group, n_slots."""
    G = DEC_SHARED_G
    edges = edge_nkeys(case)
    order = []
    lo, hi = 0, len(edges) - 1
    while lo <= hi:   # long, short, long, ..
        order.append(edges[hi]); hi -= 1
        if lo <= hi:
            order.append(edges[lo]); lo += 1
    it = 0
    groups = []
    for n in (1, 2, G, G + 1, 2 * G + 1):
        groups.append([order[(it + i) % len(order)] for i in range(n)])
        it += n
    live = edges[-2]
    groups.append([1 if i % 2 == 0 else live for i in range(8)])
    if case.H > 2:   # enough rows for the unpipelined big form (n_rows * H > 128)
        groups.append([order[i % len(order)] for i in range(7)])
    spare = len(groups)
    nk, req, tab = [3], [spare], []
    for g, ks in enumerate(groups):
        if g == 3:
            nk.append(2); req.append(spare)
        tab.append((len(nk), len(ks)))
        nk += ks
        req += [g] * len(ks)
    nk.append(1); req.append(spare)
    nk = [min(x, case.cap) for x in nk]
    in_group = np.zeros(len(nk), dtype=bool)
    for f, n in tab:
        in_group[f:f + n] = True
    return (np.array(nk, np.int32), np.array(req, np.int32), np.array(tab, np.int32), in_group, spare + 1)


def rows_of(case):
    """(row_nkeys, row_req, group_tab or None, live rows, n_slots) of a launch
    of the case.  Per-row entries: 3 slots, rows alternate between slots 0 and
    1, slot 2 is the NaN spare; key counts are the edges, then repeat."""
    if case.entry in ("shared", "shared_qln"):
        return shared_layout(case)
    e = edge_nkeys(case)
    nk = np.array([e[i % len(e)] for i in range(case.n_rows)], np.int32)
    req = np.array([i % 2 for i in range(case.n_rows)], np.int32)
    return nk, req, None, np.ones(case.n_rows, dtype=bool), 3


# -------------------------------------------------------------------- layout
def make_layout(case, n_slots):
    """Strides (elements) of the case's cache and the flat sizes."""
    H, D, cap = case.H, case.D, case.cap
    if case.lay == "head":
        return SimpleNamespace(kind="head", H=H, D=D, cap=cap, row_stride=D, head_stride=cap * D,
                               req_stride=2 * H * cap * D, v_off=H * cap * D, n_slots=n_slots,
                               size=n_slots * 2 * H * cap * D)
    rs = H * D + ((4 if case.dtype == BF16 else 2) if case.lay == "skew" else 0)
    return SimpleNamespace(kind=case.lay, H=H, D=D, cap=cap, row_stride=rs, head_stride=D, req_stride=cap * rs,
                           v_off=None, n_slots=n_slots, size=n_slots * cap * rs)


def pack_cache(K, V, lay, dtype, fill=float("nan")):
    """Logical K, V [slots, cap, H, D] -> (kc, vc) flat tensors of the layout
    (vc a view into kc's buffer for the head-major layout); pads hold `fill`."""
    n, cap, H, D = K.shape
    if lay.kind == "head":
        buf = torch.empty(n, 2, H, cap, D, dtype=dtype)
        buf[:, 0] = K.permute(0, 2, 1, 3).to(dtype)
        buf[:, 1] = V.permute(0, 2, 1, 3).to(dtype)
        flat = buf.reshape(-1)
        return flat, flat[lay.v_off:]
    out = []
    for X in (K, V):
        b = torch.full((n, cap, lay.row_stride), fill, dtype=dtype)
        b[:, :, :H * D] = X.reshape(n, cap, H * D).to(dtype)
        out.append(b.reshape(-1))
    return out[0], out[1]


def gather(c, lay, req, h, n):
    """Keys 0..n-1 of (slot req, head h) of the flat cache c: float64 [n, D]."""
    base = req * lay.req_stride + h * lay.head_stride
    idx = base + torch.arange(n).view(n, 1) * lay.row_stride + torch.arange(lay.D).view(1, -1)
    return c[idx.reshape(-1)].double().view(n, lay.D)


# ----------------------------------------------------------------- reference
def decode_attn_ref64(q, kc, vc, row_req, row_nkeys, lay, scale, lo=None):
    """float64 decode attention from the stored bits.  q [rows, >= H*D];
    kc, vc flat caches of `lay`; lo: optional first key per row (a slice).
    Returns O, T [rows, H*D]; lse, X (largest |s - m|), S (largest
    scale * sum_d |q_d k_jd|), m, l [rows, H] (m, l: max score and
    sum exp(s - m) of the range); a row without keys has O = 0, lse = -inf."""
    H, D = lay.H, lay.D
    n = len(row_nkeys)
    sc = f32r(scale)
    r = SimpleNamespace(O=torch.zeros(n, H * D, dtype=torch.float64), T=torch.zeros(n, H * D, dtype=torch.float64),
                        lse=torch.full((n, H), -math.inf, dtype=torch.float64), X=torch.zeros(n, H, dtype=torch.float64),
                        S=torch.zeros(n, H, dtype=torch.float64), m=torch.full((n, H), -math.inf, dtype=torch.float64),
                        l=torch.zeros(n, H, dtype=torch.float64), acc=torch.zeros(n, H * D, dtype=torch.float64),
                        Tacc=torch.zeros(n, H * D, dtype=torch.float64))
    for i in range(n):
        nk, k0 = int(row_nkeys[i]), 0 if lo is None else int(lo[i])
        if nk <= k0:
            continue
        for h in range(H):
            qh = q[i, h * D:(h + 1) * D].double() * sc
            k = gather(kc, lay, int(row_req[i]), h, nk)[k0:]
            v = gather(vc, lay, int(row_req[i]), h, nk)[k0:]
            s = k @ qh
            m = s.max()
            e = torch.exp(s - m)
            l = e.sum()
            sl = slice(h * D, (h + 1) * D)
            r.O[i, sl] = (e / l) @ v
            r.T[i, sl] = (e / l) @ v.abs()
            r.acc[i, sl] = e @ v
            r.Tacc[i, sl] = e @ v.abs()
            r.lse[i, h] = m + torch.log(l)
            r.m[i, h], r.l[i, h] = m, l
            r.X[i, h] = (m - s.min())
            r.S[i, h] = (k.abs() @ qh.abs()).max()
    return r


def split_chunks(nk, kpb=16, ns=DEC_SPLITS):
    """[lo, hi) of the ns key slices of a row with nk keys (the kernel's
    chunk rule: ceil(nk / ns) rounded up to the keys of a block step)."""
    chunk = ((nk + ns - 1) // ns + kpb - 1) // kpb * kpb
    return [(min(nk, z * chunk), min(nk, min(nk, z * chunk) + chunk)) for z in range(ns)]


def split_merge_ref64(part):
    """part [..., NS, 4 + D] (float64 or fp32): O = sum_z e^(m_z - M) acc_z /
    sum_z e^(m_z - M) l_z, 0 where no slice has a key."""
    p = torch.as_tensor(part).double()
    m, l, acc = p[..., 0], p[..., 1], p[..., 4:]
    M = m.max(-1, keepdim=True).values
    w = torch.where(torch.isfinite(m), torch.exp(m - torch.where(torch.isfinite(M), M, torch.zeros_like(M))),
                    torch.zeros_like(m))
    den = (w * l).sum(-1)
    num = (w.unsqueeze(-1) * acc).sum(-2)
    return torch.where(den.unsqueeze(-1) > 0, num / torch.where(den > 0, den, torch.ones_like(den)).unsqueeze(-1),
                       torch.zeros_like(num))


def ln_ref64(y, gamma, beta, eps=1e-5):
    """float64 LayerNorm rows and the module docstring's bound of them
    (without the bf16 store term)."""
    x = y.double()
    N = x.shape[1]
    g, b = gamma.double(), beta.double()
    mu = x.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + f32r(eps))
    ref = (x - mu) * rs * g + b
    dmu = (N + 2) * U * x.abs().sum(1, keepdim=True) / N
    drs = (N / 2 + 8) * U * rs
    bound = g.abs() * (dmu * rs + (x - mu).abs() * drs) + 3 * U * (((x - mu) * rs * g).abs() + b.abs())
    return ref, bound


def ln_linear_ref64(x, w, bias=None, relu=False, residual=None):
    """float64 x . w^T + bias (ReLU) + residual from the given (already
    normalised and rounded) rows x, and the summed magnitudes of each
    output's terms."""
    xd, wd = x.double(), w.double()
    v = xd @ wd.t()
    t = xd.abs() @ wd.abs().t()
    if bias is not None:
        v = v + bias.double().view(1, -1)
        t = t + bias.double().abs().view(1, -1)
    if relu:
        v = torch.relu(v)
    if residual is not None:
        v = v + residual.double()
        t = t + residual.double().abs()
    return v, t


# ----------------------------------------------------------------- emulation
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _expf(x):
    """__expf: float32(exp2(float32(x * log2e)))."""
    with np.errstate(all="ignore"):
        y = (np.asarray(x, f32) * LOG2E_F).astype(f32)
        return np.exp2(y.astype(np.float64)).astype(f32)


def _tree(s):
    """Butterfly sum over the last axis (xor 1, 2, 4, ..): adjacent pairs."""
    while s.shape[-1] > 1:
        s = (s[..., 0::2] + s[..., 1::2]).astype(f32)
    return s[..., 0]


MUTATIONS = ("le_nk", "lt_nkm1", "drop_wave", "rescale_per_key", "odd_first_q")


def _emul_block(qv, Kh, Vh, kb, nk, L, UNR, NW, mutate=None):
    """One block of attn_decode_vec_kernel over keys [kb, nk): qv the scaled
    query fp32 [D]; Kh, Vh fp32 [cap, D].  Returns (mm, ll, out[D]) before
    normalisation.  mutate: one of MUTATIONS (None: the kernel)."""
    D = qv.shape[0]
    VEC = D // L
    GPW = 64 // L
    KPB = NW * GPW
    cap = Kh.shape[0]
    m = np.full(KPB, -np.inf, f32)
    l = np.zeros(KPB, f32)
    acc = np.zeros((KPB, D), f32)
    grp = np.arange(KPB)
    with np.errstate(all="ignore"):
        for j0 in range(kb, nk, KPB * UNR):
            sc = np.empty((UNR, KPB), f32)
            vv = np.empty((UNR, KPB, D), f32)
            for u in range(UNR):
                j = j0 + u * KPB + grp
                lim = nk
                if u == UNR - 1 and mutate == "le_nk":
                    lim = nk + 1
                if u == UNR - 1 and mutate == "lt_nkm1":
                    lim = nk - 1
                ok = j < lim
                jj = np.minimum(np.where(ok, j, 0), cap - 1)
                kv = Kh[jj].reshape(KPB, L, VEC)
                s = np.zeros((KPB, L), f32)
                for i in range(VEC):
                    s = _fma(qv.reshape(L, VEC)[None, :, i], kv[:, :, i], s)
                sc[u] = np.where(ok, _tree(s), -np.inf)
                vv[u] = Vh[jj]
            mx = np.maximum(m, sc.max(0))
            act = mx != -np.inf
            c = _expf(m - mx)
            ln, an = (l * c).astype(f32), (acc * c[:, None]).astype(f32)
            for u in range(UNR):
                if mutate == "rescale_per_key" and u > 0:
                    ln, an = (ln * c).astype(f32), (an * c[:, None]).astype(f32)
                p = _expf(sc[u] - mx)
                ln = (ln + p).astype(f32)
                an = _fma(p[:, None], vv[u], an)
            l = np.where(act, ln, l)
            acc = np.where(act[:, None], an, acc)
            m = np.where(act, mx, m)
        # groups of a wave, xor order
        m, l, acc = m.reshape(NW, GPW), l.reshape(NW, GPW), acc.reshape(NW, GPW, D)
        x = 1
        while x < GPW:
            o = np.arange(GPW) ^ x
            mo, lo, ao = m[:, o], l[:, o], acc[:, o]
            mn = np.maximum(m, mo)
            c0 = np.where(m == -np.inf, f32(0), _expf(m - mn))
            c1 = np.where(mo == -np.inf, f32(0), _expf(mo - mn))
            l = _fma(l, c0, (lo * c1).astype(f32))
            acc = _fma(acc, c0[..., None], (ao * c1[..., None]).astype(f32))
            m = mn
            x *= 2
        rm, rl, ra = m[:, 0], l[:, 0], acc[:, 0]
        mm = rm.max()
        ll, out = f32(0), np.zeros(D, f32)
        for w in range(NW):
            if mutate == "drop_wave" and w == NW - 1:
                continue
            c = f32(0) if rm[w] == -np.inf else _expf(rm[w] - mm)
            ll = _fma(rl[w], c, ll)
            out = _fma(ra[w], c, out)
    return mm, ll, out


def _emul_generic(qv, Kh, Vh, nk, mutate=None):
    """attn_decode_kernel: fp32 scores, max, expf, sum, four key groups."""
    D = qv.shape[0]
    lim = nk + 1 if mutate == "le_nk" else nk - 1 if mutate == "lt_nkm1" else nk
    lim = max(0, min(lim, Kh.shape[0]))
    if lim == 0:
        return np.zeros(D, f32)
    s = np.zeros(lim, f32)
    for d in range(D):
        s = _fma(qv[d], Kh[:lim, d], s)
    e = np.exp((s - s.max()).astype(np.float64)).astype(f32)
    tot = f32(0)
    for j in range(lim):   # (the kernel's order is per thread then butterflies; any order serves the bound)
        tot = f32(tot + e[j])
    parts = []
    for g in range(4):
        a = np.zeros(D, f32)
        for j in range(g, lim, 4):
            a = _fma(e[j], Vh[j], a)
        parts.append(a)
    t = ((parts[0] + parts[1]).astype(f32) + (parts[2] + parts[3]).astype(f32)).astype(f32)
    return (t / tot).astype(f32)


def odd_first_row(yb, ny):
    """Block row yb -> the row it serves (attn_decode_vec_kernel, odd_first)."""
    if ny & 1:
        return yb
    return 2 * yb + 1 if yb < ny // 2 else 2 * (yb - ny // 2)


def _cache_np(c, lay, req, h):
    base = req * lay.req_stride + h * lay.head_stride
    idx = base + torch.arange(lay.cap).view(-1, 1) * lay.row_stride + torch.arange(lay.D).view(1, -1)
    return c[idx.reshape(-1)].float().view(lay.cap, lay.D).numpy()


def decode_attn_emulated(q, kc, vc, row_req, row_nkeys, lay, scale, lab, dtype, mutate=None, rows=None):
    """The kernel named by `lab` in numpy fp32 (module docstring).  q
    [rows, >= H*D] of the kernel's dtype (or fp32 queries already formed by
    emulate_qln).  Returns O [rows, H*D] fp32 (bf16-rounded for bf16), or for
    a split label the partial records [rows, H, NS, 4 + D] (pads 0).
    `rows`: only these rows (others stay NaN)."""
    H, D = lay.H, lay.D
    n = len(row_nkeys)
    p = parse_label(lab)
    ns = p[3] if p else 0
    out = np.full((n, H, ns, 4 + D) if ns else (n, H * D), np.nan, f32)
    qf = q.float().numpy()
    cache = {}
    for yb in (range(n) if rows is None else rows):
        r = odd_first_row(yb, n) if (p and not ns and rows is None) else yb
        rq = yb if mutate == "odd_first_q" else r   # the mutation: q not permuted
        nk, req = int(row_nkeys[r]), int(row_req[r])
        for h in range(H):
            if (req, h) not in cache:
                cache[(req, h)] = (_cache_np(kc, lay, req, h), _cache_np(vc, lay, req, h))
            Kh, Vh = cache[(req, h)]
            qv = (qf[rq, h * D:(h + 1) * D] * f32(scale)).astype(f32)
            if p is None:
                o = _emul_generic(qv, Kh, Vh, nk, mutate)
            elif ns:
                for z, (lo, hi) in enumerate(split_chunks(nk, p[2] * (64 // p[0]), ns)):
                    mm, ll, acc = _emul_block(qv, Kh, Vh, lo, hi, p[0], p[1], p[2], mutate)
                    out[r, h, z, 0], out[r, h, z, 1], out[r, h, z, 2:4], out[r, h, z, 4:] = mm, ll, 0, acc
                continue
            else:
                mm, ll, acc = _emul_block(qv, Kh, Vh, 0, nk, p[0], p[1], p[2], mutate)
                inv = f32(1) / ll if ll > 0 else f32(0)
                o = (acc * inv).astype(f32)
            out[r, h * D:(h + 1) * D] = bf16r_np(o) if dtype == BF16 else o
    return out


def emulate_ln(y, gamma, beta, eps, dtype):
    """ln_stats_loaded / ln_apply in numpy fp32 (lane sums sequential, the
    wave sum as a butterfly), rounded to bf16 for bf16."""
    v = y.float().numpy()
    M, N = v.shape
    nch = N // 8
    g, b = gamma.float().numpy(), beta.float().numpy()

    def wsum(t):   # t [M, nch, 8] -> per-lane sequential, then butterfly over 64 lanes
        lanes = np.zeros((M, 64), f32)
        for c in range((nch + 63) // 64):
            blk = t[:, 64 * c:64 * (c + 1)]
            for i in range(8):
                lanes[:, :blk.shape[1]] = (lanes[:, :blk.shape[1]] + blk[:, :, i]).astype(f32)
        return _tree(lanes)
    mu = (wsum(v.reshape(M, nch, 8)) / f32(N)).astype(f32)
    d = (v - mu[:, None]).astype(f32)
    qq = wsum(_fma(d, d, 0).reshape(M, nch, 8))
    rs = (1.0 / np.sqrt(((qq / f32(N)).astype(f32) + f32(eps)).astype(f32).astype(np.float64))).astype(f32)
    x = _fma((d * rs[:, None]).astype(f32), g[None], b[None])
    return torch.from_numpy(bf16r_np(x) if dtype == BF16 else x)


def emulate_qln(y, gamma, beta, eps, wq, bq, H, D, dtype, row_nkeys):
    """dec_q_prologue / dec_q_prologue_f32: x = LN(y) and the query rows
    (bf16-rounded for bf16; zero for a row with <= 1 key, SMER_DEC_QSKIP),
    with the kernel's split of each dot product over its threads."""
    x = emulate_ln(y, gamma, beta, eps, dtype)
    xn, w = x.numpy(), wq.float().numpy()
    M, DM = xn.shape
    TPO = (512 if dtype == BF16 else 256) // D
    acc = np.zeros((M, H * D, TPO), f32)
    if dtype == BF16:
        KT = DM // TPO
        for pt in range(TPO):
            for k in range(pt * KT, (pt + 1) * KT):
                acc[:, :, pt] = _fma(xn[:, None, k], w[None, :, k], acc[:, :, pt])
    else:
        for j in range(DM // (4 * TPO)):
            for pt in range(TPO):
                for i in range(4):
                    k = 4 * (TPO * j + pt) + i
                    acc[:, :, pt] = _fma(xn[:, None, k], w[None, :, k], acc[:, :, pt])
    qv = (_tree(acc) + bq.float().numpy()[None]).astype(f32)
    if dtype == BF16:
        qv = bf16r_np(qv)
    qv[np.asarray(row_nkeys) <= 1] = 0
    return x, torch.from_numpy(qv)


# -------------------------------------------------------------------- bounds
def links_of(case, nk):
    kpb, un = kpb_unr(case)
    p = parse_label(case.label)
    gpw = 64 // p[0] if p else 1
    return -(-nk // (kpb * un)) + int(math.log2(gpw)) + 2


def o_bound(case, ref, row_nkeys, dtype=None):
    """Per-element bound of O [rows, H*D] (module docstring)."""
    dtype = dtype or case.dtype
    H, D = case.H, case.D
    if dtype == BF16:
        return DEC_REL_O * ref.T + UB * ref.O.abs()
    nk = torch.as_tensor(np.asarray(row_nkeys)).double().view(-1, 1)
    links = torch.tensor([[links_of(case, int(k))] for k in row_nkeys], dtype=torch.float64)
    E = 2 * ((D + 2) * ref.S + 1.25 * ref.X + 2 * links)
    return ((nk + D + 2 + E) * U).repeat_interleave(D, 1) * ref.T


# ---------------------------------------------------------------------- data
def _gen(*key):
    """A CPU generator seeded from the key (stable across processes)."""
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


def _q_frame(qdata, dtype, pad=8):
    """[rows, H*D + pad] buffer, pads NaN (inputs promise nothing of pads)."""
    n, w = qdata.shape
    buf = torch.full((n, w + pad), float("nan"), dtype=dtype)
    buf[:, :w] = qdata.to(dtype)
    return buf


def data_parity(case, n_slots, n_rows):
    """Peaky scores: N(0,1) queries, keys scaled so that max - median of a
    row's scores is about 8 (the std of a score about 3): single keys carry
    a visible share and the running maximum moves during the walk."""
    g = _gen(case.id, "parity")
    H, D, cap = case.H, case.D, case.cap
    scale = 1.0 / math.sqrt(D)
    q = torch.randn(n_rows, H * D, generator=g)
    K = torch.randn(n_slots, cap, H, D, generator=g) * 3.0
    V = torch.randn(n_slots, cap, H, D, generator=g)
    K[n_slots - 1] = float("nan"); V[n_slots - 1] = float("nan")
    return q, K, V, scale


def data_decoy(case, n_slots, n_rows, nks, q=None):
    """Staircase slots: every row of the launch has the same query; key j's
    score is 44 * (number of the launch's key counts <= j) + noise in [-4, 4]
    (+-2 after the keys' rounding), so for a row with nk keys EVERY position
    >= nk (through the end of the slot, a superset of nk .. nk + KPB * UNR - 1)
    holds a key scoring >= 40 above all of its valid ones, with finite V
    (offset by 16 per stair: a decoy that leaks moves the output far).  The
    valid keys of the last stair have uneven scores across several key steps,
    so the rescale is live."""
    g = _gen(case.id, "decoy")
    H, D, cap = case.H, case.D, case.cap
    scale = 1.0 / math.sqrt(D)
    if q is None:
        q1 = torch.randn(1, H * D, generator=g).to(case.dtype).float()
        q = q1.repeat(n_rows, 1)
    qh = q[0].view(H, D).double()
    edges = sorted(set(int(x) for x in nks if 0 < x < cap))
    stair = torch.zeros(cap)
    for e in edges:
        stair[e:] += 1
    tgt = 44.0 * stair.view(1, cap, 1) + (torch.rand(n_slots, cap, H, generator=g) * 8 - 4)
    noise = torch.randn(n_slots, cap, H, D, generator=g) * 0.5
    u = qh / (qh * qh).sum(-1, keepdim=True)          # q . u = 1 per head
    cur = (noise.double() * qh.view(1, 1, H, D)).sum(-1) * scale
    K = noise.double() + ((tgt.double() - cur) / scale).unsqueeze(-1) * u.view(1, 1, H, D)
    V = torch.randn(n_slots, cap, H, D, generator=g) + 16.0 * (stair.view(1, cap, 1, 1) % 3 - 1)
    K[n_slots - 1] = float("nan"); V[n_slots - 1] = float("nan")
    return q, K.float(), V, scale


def needle_positions(case, nk):
    """0, nk - 1 and every key of the last key step: each lane group of each
    wave holds one key per unroll slot there, so this is the first and last
    key of every lane group, wave and unroll slot (ascending)."""
    kpb, un = kpb_unr(case)
    step = kpb * un
    j0 = (nk - 1) // step * step
    return sorted({0, nk - 1} | set(range(j0, nk)))


def _grid_regime(case):
    """"few" / "many" for the capacities where the instantiation depends on
    the grid (512 <= cap < 2048: pipelined up to 128 blocks), else None."""
    if not 512 <= case.cap < 2048 or case.entry not in ("decode", "shared") or case.label.startswith("generic"):
        return None
    return "few" if "pipe" in case.label else "many"


def needle_rows(case):
    """Rows of one needle launch: D - 3 per slot, slots 0 and 1; at most 128
    blocks where the case's instantiation needs a small grid."""
    n = 2 * (case.D - 3)
    return min(n, 128 // case.H) if _grid_regime(case) == "few" else n


def needle_launch(case, nk, positions):
    """Rows of one needle launch: row i's needle is key positions[i] of slot
    i // (D - 3) (slots 0 and 1; slot 2 NaN), in dim 3 + i % (D - 3).
    scale = 1/8; every key is (n1, n2, n3, 0, ..) with n in {-1, 0, 1} in dims
    0..2 plus, for a needle, 41 in its dim; row i's query is (1, -1, 1, 0, ..)
    with 8 in its needle's dim.  A score is (n1 - n2 + n3) / 8 (+ 41 for the
    row's own needle): exact in fp32 in any order, the needle >= 40.25 above
    every other key; the other needles of the slot score like ordinary keys.
    V: the needle rows hold +-(1 + d / 128) * 2**(i % 3) (distinct, bf16-exact,
    magnitude >= 1), every other entry an integer in [-4, 4].

    Query-prologue entries (case.dmodel): the query is formed by the kernel,
    so the launch carries y, gamma = 1, beta = 0, Wq, bq instead: y_i = 16 e_i
    (one-hot), so LN(y_i) is about sqrt(dm - 1) at i and -1 / sqrt(dm - 1)
    elsewhere; Wq[needle dim of row i, i] = 1/2 and bq = (1, -1, 1, 0, ..) per
    head.  Row i's query then has >= 11 in its own needle dim (a score of
    >= 57 for its needle) and about -0.02 in the other needles' dims (their
    keys score -0.11, below the ordinary keys' maximum of 0.375): the margin
    is >= 40 whatever the rounding of LN and of the projection, and the
    needle's weight is exp(0) = 1 exactly.  A row with one key has q = 0
    (SMER_DEC_QSKIP) and the output V[0], the needle again.

    Returns SimpleNamespace(q [rows, H*D] or None, qln or None, K, V
    [3, cap, H, D], scale, want [rows, H*D], req [rows], tab [groups, 2])."""
    g = _gen(case.id, "needle", nk)
    H, D, cap = case.H, case.D, case.cap
    n, per = len(positions), D - 3
    assert n <= 2 * per and len(set(positions)) == n
    K = torch.zeros(3, cap, H, D)
    K[:, :, :, :3] = torch.randint(-1, 2, (3, cap, H, 3), generator=g).float()
    V = torch.randint(-4, 5, (3, cap, H, D), generator=g).float()
    q = torch.zeros(n, H, D)
    q[:, :, 0], q[:, :, 1], q[:, :, 2] = 1, -1, 1
    want = torch.zeros(n, H, D)
    d = torch.arange(D).float()
    hs = torch.tensor([(-1.0) ** h * 2.0 ** (h // 2) for h in range(H)]).view(H, 1)
    req = np.array([i // per for i in range(n)], np.int32)
    for i, p in enumerate(positions):
        K[req[i], p, :, 3 + i % per] = 41
        q[i, :, 3 + i % per] = 8
        row = (1 + d / 128) * torch.where(d.long() % 2 == 0, 1.0, -1.0) * 2.0 ** (i % 3)
        V[req[i], p] = row.view(1, D).expand(H, D) * hs
        want[i] = V[req[i], p]
    K[2] = float("nan"); V[2] = float("nan")
    tab = [[0, min(n, per)]] + ([[per, n - per]] if n > per else [])
    q, want = q.view(n, H * D), want.view(n, H * D)
    n_real = n
    if _grid_regime(case) == "many" and n * H <= 128:   # copies of row 0 until the grid is large
        extra = 128 // H + 1 - n
        q, want = torch.cat([q, q[:1].repeat(extra, 1)]), torch.cat([want, want[:1].repeat(extra, 1)])
        req = np.concatenate([req, np.zeros(extra, np.int32)])
        tab.append([n, extra])
        n += extra
    tab = np.array(tab, np.int32)
    qln = None
    if case.dmodel:
        dm = case.dmodel
        assert n <= dm
        y = torch.zeros(n, dm)
        wq = torch.zeros(H * D, dm)
        bq = torch.zeros(H, D)
        bq[:, 0], bq[:, 1], bq[:, 2] = 1, -1, 1
        for i in range(n_real):
            y[i, i] = 16.0
            for h in range(H):
                wq[h * D + 3 + i % per, i] = 0.5
        qln = (y.to(case.dtype), torch.ones(dm), torch.zeros(dm), wq.to(case.dtype), bq.view(-1))
    return SimpleNamespace(q=None if case.dmodel else q, qln=qln, K=K, V=V, scale=0.125, want=want, req=req, tab=tab)


def merge_linear_bound(part, w, bias, residual):
    """float64 smer_linear_decode_merge_f32 and its bound.  The merged row is
    O = sum_z w_z acc_z / sum_z w_z l_z, w_z = __expf(m_z - M): each weight is
    off by (1.25 Xm + 2) 2**-24 relative (Xm the largest M - m_z of the record,
    the module docstring's fast-exp term, one exponential and one multiply),
    numerator and denominator each sum 8 terms, then one division and one
    multiply: (8 + 2 + 2 (1.25 Xm + 2)) 2**-24 To, To = sum_z w_z |acc_z| / den.
    The Linear adds gemmref's (K + 8) 2**-24 over T = To |W|^T + |bias| +
    |residual|.  Returns (ref [M, N], bound [M, N])."""
    p = torch.as_tensor(part).double()
    M, H = p.shape[:2]
    m, l, acc = p[..., 0], p[..., 1], p[..., 4:]
    fin = torch.isfinite(m)
    top = torch.where(fin, m, torch.full_like(m, -math.inf)).max(-1, keepdim=True).values
    top0 = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    wz = torch.where(fin, torch.exp(m - top0), torch.zeros_like(m))
    den = (wz * l).sum(-1, keepdim=True)
    ok = den > 0
    dsafe = torch.where(ok, den, torch.ones_like(den))
    O = torch.where(ok, (wz.unsqueeze(-1) * acc).sum(-2) / dsafe, torch.zeros(M, H, acc.shape[-1], dtype=torch.float64))
    To = torch.where(ok, (wz.unsqueeze(-1) * acc.abs()).sum(-2) / dsafe, torch.zeros_like(O))
    Xm = torch.where(fin, top0 - m, torch.zeros_like(m)).max(-1).values.max(-1).values.view(M, 1)   # per row
    K = H * acc.shape[-1]
    wd = torch.as_tensor(w).double()
    ref = O.reshape(M, K) @ wd.t()
    T = To.reshape(M, K) @ wd.abs().t()
    if bias is not None:
        ref, T = ref + bias.double().view(1, -1), T + bias.double().abs().view(1, -1)
    if residual is not None:
        ref, T = ref + residual.double(), T + residual.double().abs()
    return ref, (K + 8 + 10 + 2 * (1.25 * Xm + 2)) * U * T


def data_census(case, n_slots, n_rows):
    """q = 0 (every score 0, every weight exactly 1); V[j, d] = 1 if
    d == j % D else 0; K random (finite: 0 * k = 0)."""
    g = _gen(case.id, "census")
    H, D, cap = case.H, case.D, case.cap
    q = torch.zeros(n_rows, H * D)
    K = torch.randn(n_slots, cap, H, D, generator=g)
    V = torch.zeros(n_slots, cap, H, D)
    j = torch.arange(cap)
    V[:, j, :, j % D] = 1.0
    K[n_slots - 1] = float("nan"); V[n_slots - 1] = float("nan")
    return q, K, V, 0.125


def census_expected(case, row_nkeys):
    """float64 count_d / nk [rows, H*D] (0 for nk = 0)."""
    D, H = case.D, case.H
    out = torch.zeros(len(row_nkeys), H, D, dtype=torch.float64)
    d = torch.arange(D)
    for i, nk in enumerate(int(x) for x in row_nkeys):
        if nk:
            cnt = (nk - d + D - 1) // D   # keys j < nk with j % D == d
            out[i] = (cnt.double() / nk).view(1, D)
    return out.view(len(row_nkeys), H * D)


def census_bound(expected, dtype):
    """fp32: 2 ulp (the 1 / l multiply or the division); bf16: half a bf16
    ulp of the value (its rounding) on top."""
    x = expected.float().numpy()
    ulp = torch.from_numpy(np.spacing(x).astype(np.float64))
    return 2 * ulp + (ulp * 2.0 ** 15 if dtype == BF16 else 0.0)

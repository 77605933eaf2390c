"""Chord-following infill on the device decode path (csrc/decode_ops.hip
chord_ban_kernel, smer_chord_ban): the kernel alone against a numpy mirror
written from its contract, the chain ban -> bar clock -> chord -> template ->
grammar entry against the entry on host-edited logits, then `chords=` on the C2
model: the device decode against the host loop, and the '+bar+chord' graphs
beside the ones without the node."""
import numpy as np
import pytest
import torch

from tests.test_barclock_gpu import _biased, _codes, _mirror, _units, c2, c2_bf16  # noqa: F401  (c2*: fixtures)
from tests.test_template_gpu import (_Log, _case, _per_mask, _session, _t, _tables, _take,
                                     spans)  # noqa: F401  (spans: a fixture)
from tests.test_template_gpu import L as TPL_L
from tests.test_template_gpu import NM as TPL_NM
from tests.test_template_gpu import NM_T as TPL_NM_T

pytestmark = pytest.mark.gpu
dev = "cuda"
NST, CAP, NM, POS, ROWS = 12, 6, 4, 64, 16
FRAME = 8  # sentinel words in front of and behind every table
LIVE = ("end=0", "seg-first", "seg-before", "pending-sep", "open-group", "end>=L", "k=15", "one-pitch")
QUIET = ("done", "chord_len=0", "k=-1", "control-span", "past-masks", "c>cap")
KINDS = LIVE + QUIET


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _framed(shape, dtype, sent):
    n = int(np.prod(shape))
    frame = np.full(FRAME + n + FRAME, sent, dtype=dtype)
    return frame, frame[FRAME:FRAME + n].reshape(shape)


def _bits(rows):
    from smer_music_generation_amd.generation import ban_bits
    return ban_bits(rows)


def _chord_mirror(V, big, st, tg, clock, chord_len, chord_at, rows, cap):
    """smer_chord_ban on the host, from its contract: the framed logits `big`
    edited in place (rows: the bit rows as booleans [R, 16, 512]).  Returns
    {request: the row k it applied}."""
    active = {}
    for r in range(st.shape[0]):
        done, midx, c = int(st[r, 5]), int(st[r, 3]), int(st[r, 7])
        T, P, A, fl = (int(x) for x in clock[r, :4])
        end = ((T - P) if (fl >> 1) & 1 else T) + A
        L = int(chord_len[r])
        if done or L <= 0 or not 0 <= midx < tg.shape[1] or tg[r, midx] != 0 or c > cap:
            continue
        k = int(chord_at[r, midx, min(max(end, 0), min(L, POS) - 1)])
        if 0 <= k < ROWS:
            big[2 * r + 1, :V][rows[r, k, :V]] = np.float32(-100.0)
            active[r] = k
    return active


def _chord_case(V, R, L, shift):
    """R requests, request r of kind KINDS[(r + shift) % 14].  Every mask's bar
    has two segments, row 0 up to L // 2 and row 1 from there, except where the
    kind says otherwise; the clock words are (T, P, A, G | S << 1)."""
    v, keep, cls, rej = _tables(V)
    rng = np.random.default_rng(9000 * V + 100 * R + 10 * L + shift)
    pitch = np.asarray(v.pitch_indices)
    H = L // 2
    ldl = V + 3
    big = (rng.standard_normal((2 * R, ldl)) * 3).astype(np.float32)
    big[:, V:] = np.float32(777.0)
    st = np.zeros((R, NST), dtype=np.int32)
    tg = np.zeros((R, NM), dtype=np.int8)
    f_len, chord_len = _framed((R,), np.int32, 16)        # a stray read finds a live bar
    f_at, chord_at = _framed((R, NM, POS), np.int8, 5)     # ... a row that bans
    f_bits, bits = _framed((R, ROWS, 16), np.int32, -1)         # ... every token
    f_ck, clock = _framed((R, 8), np.int32, 4)
    rows = np.zeros((R, ROWS, 512), dtype=bool)
    rows[:, :, pitch] = rng.random((R, ROWS, len(pitch))) < 0.6
    rows[:, :, V - 1] = True  # (the last token of the row, whatever its class: the i < V edge)
    chord_len[:] = L
    chord_at[:, :, :H], chord_at[:, :, H:] = 0, 1
    kinds, want_k = [], {}
    for r in range(R):
        kind = KINDS[(r + shift) % len(KINDS)]
        kinds.append(kind)
        c, midx, words = 2 + r % 3, r % NM, (3, 2, 0, 0)
        if kind == "end=0":
            words, want_k[r] = (0, 0, 0, 0), 0
        elif kind == "seg-first":
            words, want_k[r] = (H, 2, 0, 0), 1
        elif kind == "seg-before":
            words, want_k[r] = (H - 1, 2, 0, 0), 0
        elif kind == "pending-sep":  # T past the boundary, the rewound position before it
            words, want_k[r] = (H + 2, 4, 0, 2), 0
        elif kind == "open-group":   # T before the boundary, the open group reaches it
            words, want_k[r] = (H - 2, 1, 2, 1), 1
        elif kind == "end>=L":       # clamped to the bar's last sixteenth, not read past it
            words, want_k[r] = (L + 3, 2, 0, 0), 2
            chord_at[r, midx, L - 1], chord_at[r, midx, L:] = 2, 3
        elif kind == "k=15":
            chord_at[r, midx, :], want_k[r] = 15, 15
        elif kind == "one-pitch":
            rows[r, 1, :] = False
            rows[r, 1, pitch] = True
            rows[r, 1, pitch[(7 * r) % len(pitch)]] = False
            words, want_k[r] = (H + 1, 1, 0, 0), 1
        elif kind == "done":
            st[r, 5] = 1
        elif kind == "chord_len=0":
            chord_len[r] = 0
        elif kind == "k=-1":
            chord_at[r, midx, :] = -1
        elif kind == "control-span":
            tg[r, midx] = 1 + r % 4
        elif kind == "past-masks":
            midx = NM
        elif kind == "c>cap":
            c = CAP + 1
        st[r, 0], st[r, 2], st[r, 3], st[r, 4], st[r, 7] = 10 + r, 5, midx, NM, c
        clock[r, :4], clock[r, 4], clock[r, 5:] = words, c, 0
    for r in range(R):
        bits[r] = _bits(rows[r]).view(np.int32)
    return dict(v=v, V=V, R=R, L=L, big=big, st=st, tg=tg, chord_len=chord_len, chord_at=chord_at, rows=rows,
                clock=clock, frames=(f_len, f_at, f_bits, f_ck), kinds=kinds, want_k=want_k, pitch=pitch)


def _shifts(R):
    return range(len(KINDS)) if R == 1 else (0, 5, 10) if R < len(KINDS) else (0,)


@pytest.mark.parametrize("L", [12, 16])
@pytest.mark.parametrize("V", [309, 512])
@pytest.mark.parametrize("R", [1, 5, 33])
def test_chord_ban_kernel_alone(V, R, L):
    """The framed logits after smer_chord_ban against the mirror, every 32-bit
    word; the state and the four framed tables (the clock among them) stay bit
    for bit; the quiet kinds leave their logits row alone; each live kind bans
    exactly the bits of the row its position selects."""
    from smer_music_generation_amd import ops as O
    seen = set()
    for shift in _shifts(R):
        c = _chord_case(V, R, L, shift)
        f_t = [_t(f) for f in c["frames"]]
        len_t = f_t[0][FRAME:-FRAME]
        at_t = f_t[1][FRAME:-FRAME].view(R, NM, POS)
        bits_t = f_t[2][FRAME:-FRAME].view(R, ROWS, 16)
        ck_t = f_t[3][FRAME:-FRAME].view(R, 8)
        big_t, s_t, tg_t = _t(c["big"]), _t(c["st"]), _t(c["tg"])
        O.chord_ban(big_t[:, :V], s_t, tg_t, ck_t, len_t, at_t, bits_t, cap=CAP)
        torch.cuda.synchronize()
        want = c["big"].copy()
        active = _chord_mirror(V, want, c["st"], c["tg"], c["clock"], c["chord_len"], c["chord_at"], c["rows"], CAP)
        got = big_t.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert np.array_equal(s_t.cpu().numpy(), c["st"]) and np.array_equal(tg_t.cpu().numpy(), c["tg"])
        for f, ft in zip(c["frames"], f_t):
            assert np.array_equal(ft.cpu().numpy(), f)
        assert (got[:, V:] == np.float32(777.0)).all() and np.array_equal(got[0::2], c["big"][0::2])
        for r, kind in enumerate(c["kinds"]):
            seen.add(kind)
            row, row0 = got[2 * r + 1, :V], c["big"][2 * r + 1, :V]
            if kind in QUIET:
                assert r not in active and np.array_equal(row.view(np.int32), row0.view(np.int32))
                continue
            k = c["want_k"][r]
            assert active[r] == k
            banned = c["rows"][r, k, :V]
            assert (banned[V - 1] or kind == "one-pitch") and (row[banned] == np.float32(-100.0)).all()
            assert np.array_equal(row[~banned].view(np.int32), row0[~banned].view(np.int32))
            if kind == "one-pitch":
                assert (row[c["pitch"]] != np.float32(-100.0)).sum() == 1
    assert seen == set(KINDS)


def test_chord_ban_checks_its_arguments():
    from smer_music_generation_amd import _lib
    from smer_music_generation_amd import ops as O
    R, V = 2, 309

    def z(*shape, dt=torch.int32):
        return torch.zeros(*shape, dtype=dt, device=dev)
    a0 = dict(lg=torch.zeros(2 * R, V, device=dev), st=z(R, NST), tg=z(R, 4, dt=torch.int8), ck=z(R, 8), cl=z(R),
              at=z(R, 4, POS, dt=torch.int8), bits=z(R, ROWS, 16))

    def run(a, cap=8):
        O.chord_ban(a["lg"], a["st"], a["tg"], a["ck"], a["cl"], a["at"], a["bits"], cap=cap)
    run(a0)
    for bad in (dict(lg=torch.zeros(2 * R, 513, device=dev)), dict(lg=a0["lg"][:3]), dict(ck=z(R, 7)), dict(cl=z(R + 1)),
                dict(at=z(R, 4, 63, dt=torch.int8)), dict(at=z(R, 5, POS, dt=torch.int8)), dict(at=z(R, 4, POS)),
                dict(bits=z(R, 15, 16)), dict(bits=z(R, ROWS, 16, dt=torch.int64)), dict(tg=z(1, 4, dt=torch.int8))):
        with pytest.raises(RuntimeError):
            run(dict(a0, **bad))
    with pytest.raises(RuntimeError):
        run(a0, cap=0)
    lib = _lib.load()
    p = [a0[k].data_ptr() for k in ("lg", "st", "tg", "ck", "cl", "at", "bits")]

    def raw(R=R, V=V, ldl=V, nst=NST, nm=4, cap=8, null=None):
        q = [None if i == null else x for i, x in enumerate(p)]
        return lib.smer_chord_ban(R, V, q[0], ldl, q[1], nst, q[2], nm, cap, q[3], q[4], q[5], q[6], None)
    assert raw() == 0
    for kw in (dict(V=513, ldl=513), dict(R=0), dict(ldl=V - 1), dict(nst=8), dict(nm=0), dict(cap=0), dict(null=0),
               dict(null=3), dict(null=4), dict(null=5), dict(null=6)):
        assert raw(**kw) == -1, kw
        assert b"smer_chord_ban" in lib.smer_last_error()
    assert lib.smer_abi_version() == 1


# ---------------------------------------------------------------------------
# ban -> bar clock -> chord -> template -> entry against the entry on host-edited logits
# ---------------------------------------------------------------------------
def _chain_host_edit(c, big, st, out, bar_len, clock, ch):
    """The four kernels on the host, in the captured step's order.  Returns
    {request: chord row applied}."""
    V, is_pitch = c["V"], (c["cls"] & 2).astype(bool)
    for r in range(c["R"]):  # smer_logits_ban
        midx = int(st[r, 3])
        if not st[r, 5] and 0 <= midx < TPL_NM and c["bom"][r, midx] >= 0:
            big[2 * r + 1, :V][c["ban"][r, c["bom"][r, midx]]] = np.float32(-100.0)
    _mirror(V, c["v"].eos_index, c["cls"], c["units"], big, st, c["tg"], out, bar_len, clock, CAP)
    used = _chord_mirror(V, big, st, c["tg"], clock, ch["len"], ch["at"], ch["rows"], CAP)
    for r in range(c["R"]):  # smer_logits_template
        midx, at = int(st[r, 3]), int(st[r, 2]) - 1
        if st[r, 5] or not (0 <= midx < TPL_NM_T and 0 <= at < TPL_L):
            continue
        e, row = int(c["tape"][r, midx, at]), big[2 * r + 1, :V]
        if 0 <= e < V:
            row[:] = np.float32(-100.0)
            row[e] = np.float32(0.0)
        elif e == -2:
            row[~is_pitch] = np.float32(-100.0)
    return used


@pytest.mark.parametrize("V", [309, 512])
@pytest.mark.parametrize("R", [1, 5, 33])
@pytest.mark.parametrize("entry", ["greedy", "greedy_ring", "stream", "rows"])
def test_ban_bar_chord_template_then_grammar_entry_equals_entry_on_edited_logits(entry, V, R):
    """Three steps in a row (fresh logits before each, as the projection
    writes them) on the request mix of tests/test_template_gpu.py, every
    request with a clock in some state, a bar of 12, 16 or 0 and chords over a
    bar of 16, 12 or none whose every sixteenth is a segment of its own (row pos
    % 16): state rows, out_tok with the fail bit, ids / meta, all 625 words of
    every MT stream, the live count and the clock words, bit for bit.  Some
    request's governing row changes between the steps: a token the device drew
    moved its onset across a segment boundary."""
    from smer_music_generation_amd import ops as O
    n_active = n_cross = 0
    for shift in ((0, 1, 3, 7) if R == 1 else (0, 5) if R < 10 else (0,)):
        c = _case(V, R, shift)
        v = c["v"]
        c["units"] = _units(v, V)
        rng = np.random.default_rng(77 * V + 3 * R + shift)
        bar_len = np.asarray([(12, 16, 0)[r % 3] for r in range(R)], dtype=np.int32)
        # (requests 0 and 1 mod 3 are chorded: among them, at every R, a row whose tape forces a duration
        # token, so that its onset moves -- tests/test_template_gpu.py's kinds "min-logit" and "below-100")
        ch = dict(len=np.asarray([(16, 12, 0)[r % 3] for r in range(R)], dtype=np.int32),
                  at=np.tile((np.arange(POS) % ROWS).astype(np.int8), (R, TPL_NM, 1)),
                  rows=np.zeros((R, ROWS, 512), dtype=bool))
        ch["rows"][:, :, c["pitch"]] = rng.random((R, ROWS, len(c["pitch"]))) < 0.5
        clock0 = np.zeros((R, 8), dtype=np.int32)
        for r in range(R):
            T = (5 * r + shift) % 11
            clock0[r, :5] = (T, min(T, r % 3), 0, 0, c["st"][r, 7])
        frame_t = _t(c["frame"])
        dv = dict(keep=_t(c["keep"]), cls=_t(c["cls"]), rej=_t(c["rej"]), tg=_t(c["tg"]), sl=_t(c["src_len"]),
                  tp=_t(c["tp"]), bom=_t(c["bom"]), units=_t(c["units"]), bl=_t(bar_len),
                  bits=_t(np.stack([_bits(c["ban"][r]) for r in range(R)]).view(np.int32)),
                  tape=frame_t[8:-8].view(R, TPL_NM_T, TPL_L), cl=_t(ch["len"]), cat=_t(ch["at"]),
                  cbits=_t(np.stack([_bits(ch["rows"][r]) for r in range(R)]).view(np.int32)))
        gargs = dict(eos=v.eos_index, m0=v.char2index('m_0'), trash_pos=200)
        use_ring = entry.endswith("_ring")
        res = {}
        for on_device in (True, False):
            s_t = _t(c["st"])
            out_t = torch.zeros(R, CAP, dtype=torch.int32, device=dev)
            ctl = torch.zeros(3, dtype=torch.int32, device=dev)
            ring = torch.full((4,), -1, dtype=torch.int32).pin_memory() if use_ring else None
            m_t = _t((c["mt"] if entry == "rows" else c["mt"][0, :625]).view(np.int32))
            ck_t, ck_h = _t(clock0), clock0.copy()
            steps, used = [], []
            for step in range(3):
                big = c["big"].copy()
                if not on_device:
                    used.append(_chain_host_edit(c, big, s_t.cpu().numpy(), out_t.cpu().numpy(), bar_len, ck_h, ch))
                big_t = _t(big)
                lg_t = big_t[:, :V]
                if on_device:
                    O.logits_ban(lg_t, s_t, dv["bom"], dv["bits"])
                    O.bar_clock(lg_t, s_t, dv["tg"], out_t, dv["cls"], dv["units"], dv["bl"], ck_t, eos=v.eos_index)
                    O.chord_ban(lg_t, s_t, dv["tg"], ck_t, dv["cl"], dv["cat"], dv["cbits"], cap=CAP)
                    O.logits_template(lg_t, s_t, dv["cls"], dv["tape"])
                ids_t = torch.full((2 * R,), -7, dtype=torch.int64, device=dev)
                meta_t = torch.full((4, 2 * R), -9, dtype=torch.int32, device=dev)
                if entry.startswith("greedy"):
                    O.grammar_greedy_step(lg_t, s_t, dv["tg"], dv["keep"], dv["cls"], dv["sl"], ids_t, meta_t,
                                          out_t, ctl, ring=ring, **gargs)
                elif entry == "stream":
                    O.grammar_sample_step(lg_t, s_t, dv["tg"], dv["keep"], dv["rej"], dv["cls"], dv["sl"], ids_t,
                                          meta_t, out_t, m_t, ctl, tp=dv["tp"], **gargs)
                else:
                    O.grammar_sample_step_rows(lg_t, s_t, dv["tg"], dv["keep"], dv["rej"], dv["cls"], dv["sl"],
                                               ids_t, meta_t, out_t, m_t, ctl, tp=dv["tp"], **gargs)
                torch.cuda.synchronize()
                live = int(ring[step]) if use_ring else int(ctl[0].item())
                steps.append((ids_t.cpu().numpy(), meta_t.cpu().numpy(), live, s_t.cpu().numpy(),
                              (ck_t.cpu().numpy() if on_device else ck_h.copy())))
            res[on_device] = (steps, out_t.cpu().numpy(), m_t.cpu().numpy())
            assert np.array_equal(frame_t.cpu().numpy(), c["frame"])
            if not on_device:
                n_active += sum(len(u) for u in used)
                n_cross += sum(1 for r in range(R) if len({u[r] for u in used if r in u}) > 1)
        a, b = res[True], res[False]
        for (ia, ma, la, sa, ca), (ib, mb, lb, sb, cb) in zip(a[0], b[0]):
            assert np.array_equal(ia, ib) and np.array_equal(ma, mb) and la == lb and np.array_equal(sa, sb)
            assert np.array_equal(ca, cb)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert n_active >= 3 and n_cross >= 1  # not vacuous: rows were chorded, and one crossed a segment boundary


# ---------------------------------------------------------------------------
# the calls on the C2 model
# ---------------------------------------------------------------------------
SPLIT = 8


def _prog(G):
    """F major for two beats, then C7, within two octaves."""
    return [(0, G.pitch_set(48, 72, G.chord_tones(5, 'maj'))), (SPLIT, G.pitch_set(48, 72, G.chord_tones(0, '7')))]


def _set_at(prog, onset, L):
    return [s for a, s in prog if a <= min(onset, L - 1)][-1]


def _pitches_of(G, v, rec, codes):
    """[(onset, midi)] of every pitch drawn in a note span of the take."""
    rows = _per_mask(rec)
    return [om for k, t in enumerate(codes) if t == 0 and k in rows for om in G.pitch_onsets(v, rows[k])]


MODES = {"greedy": (dict(greedy=True), "greedy+bar+chord"),
         "rows": (dict(greedy=False, seed=[3, 4, 5], t=0.9, p=0.95), "rows+bar+chord"),
         "stream": (dict(greedy=False), "stream+bar+chord")}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", list(MODES))
def test_device_decode_equals_the_host_loop_under_chords(c2, c2_bf16, spans, mode, prec):  # noqa: F811
    """A batch of three: request 0 with chords and fill_bar (the biased model's
    greedy take is empty without the bar line), request 1 with neither, request
    2 with chords alone (bar_len 0: the clock runs, the bar line bans nothing).
    The device decode (the '+bar+chord' graph of the mode) and the host loop
    emit the same tokens, log lines and stats['chords']; unseeded they leave
    np.random in the same state; every pitch drawn in a chorded request lies in
    the set that holds at its onset, at least one was drawn, and the same call
    without chords= draws at least one outside."""
    from smer_music_generation_amd import generation as G
    m, v, ctl, reqs = c2 if prec == "fp32" else c2_bf16
    kw, gname = MODES[mode]
    kw = dict(kw, precision="fp32" if prec == "fp32" else None, fill_bar=[True, False, False])
    batch = [(list(e), t, b) for e, t, b in reqs]
    prog = _prog(G)
    chords = [{b: prog for b in reqs[0][2]}, None, {(b, reqs[2][1][0]): prog for b in reqs[2][2]}]
    G.clear_decode_sessions(m)
    res = {}
    for dg in (False, True):
        np.random.seed(31)
        lg = _Log()
        _, stats = G.generation_batch(m, batch, v, ctl, logger=lg, chords=chords, device_grammar=dg,
                                      return_stats=True, **kw)
        st = np.random.get_state()
        res[dg] = (_take(spans, 3), lg.lines, stats["tokens"], stats["steps"], stats["chords"], stats["bar_fill"],
                   (st[1].copy(), int(st[2])))
    assert res[True][:6] == res[False][:6]
    assert np.array_equal(res[True][6][0], res[False][6][0]) and res[True][6][1] == res[False][6][1]
    recs, logs = res[True][0], res[True][4]
    assert logs[1] is None
    n_in = 0
    for k in (0, 2):
        L = G.bar_units(reqs[k][0])
        drawn = _pitches_of(G, v, recs[k], _codes(G, v, reqs[k]))
        assert all(p in _set_at(prog, o, L) for o, p in drawn), (k, drawn)
        assert [e[:2] for span in logs[k] for e in span] == drawn
        assert all(s == _set_at(prog, o, L) for span in logs[k] for o, _, s in span)
        n_in += len(drawn)
    sess = _session(G, m, 3)
    assert gname in sess._graphs and sess._greedy is sess._graphs[gname]
    assert not any("chord" in k for k in sess._graphs if k != gname)
    np.random.seed(31)
    G.generation_batch(m, batch, v, ctl, logger=_Log(), **kw)
    free = _take(spans, 3)
    n_out = sum(1 for k in (0, 2) for o, p in _pitches_of(G, v, free[k], _codes(G, v, reqs[k]))
                if p not in _set_at(prog, o, G.bar_units(reqs[k][0])))
    print("%s %s: %d pitches drawn in their chords; the call without chords= draws %d outside"
          % (mode, prec, n_in, n_out))
    assert n_in >= 1 and n_out >= 1
    assert gname.replace("+chord", "") in sess._graphs
    if mode != "stream":
        assert free[1] == recs[1]  # the batch-mate without the keyword draws what it draws without it


def test_chords_with_pitches_fill_bar_variations_logprobs_and_a_rhythm_template(c2, spans):  # noqa: F811
    """pitches= + fill_bar + variations=2 + logprobs=True under chords (the
    'rows+ban+bar+chord+score' graph), and one call under rhythm_template
    ('rows+bar+chord+tpl'): device and host loop agree on tokens, stats['chords']
    and, to 2e-3 (the bound of tests/test_barclock_gpu.py: the same step
    kernels), the scores; every pitch is in its chord and in the pitch set; the
    templated take has the source's onsets."""
    from smer_music_generation_amd import generation as G
    m, v, ctl, reqs = c2
    ev, tr, br = reqs[0]
    codes, L = _codes(G, v, reqs[0]), G.bar_units(reqs[0][0])
    G.clear_decode_sessions(m)
    prog = _prog(G)
    chords = {b: prog for b in br}
    low = tuple(range(48, 66))
    tpl = G.rhythm_template(ev, v, tr, br)
    for extra, gname, n in ((dict(pitches=low, fill_bar=True, variations=2, logprobs=True),
                             "rows+ban+bar+chord+score", 2),
                            (dict(template=tpl), "rows+bar+chord+tpl", 1)):
        res = {}
        for dg in (False, True):
            stats = {}
            out = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, seed=21, chords=chords, stats=stats,
                                   device_grammar=dg, **extra)
            assert out is not None
            res[dg] = (_take(spans, n), stats)
        assert res[True][0] == res[False][0]
        assert res[True][1]["chords"] == res[False][1]["chords"] and len(res[True][1]["chords"]) == n
        n_in = 0
        for rec in res[True][0]:
            drawn = _pitches_of(G, v, rec, codes)
            assert all(p in _set_at(prog, o, L) for o, p in drawn)
            n_in += len(drawn)
            if "pitches" in extra:
                assert all(p in low for _, p in drawn)
        assert n_in >= 1
        if "logprobs" in extra:
            assert res[True][1]["bar_fill"] == res[False][1]["bar_fill"]
            for a, b in zip(res[True][1]["logprobs"], res[False][1]["logprobs"]):
                assert len(a) == len(b) and float(np.abs(np.asarray(a) - np.asarray(b)).max()) <= 2e-3
        else:
            bodies = G._template_bodies(ev, v, tr, br, None)[0]
            got = _per_mask(res[True][0][0])
            for k, c in enumerate(codes):
                if c == 0:
                    assert [o for o, _ in G.pitch_onsets(v, got[k])] == [o for o, _ in G.pitch_onsets(v, bodies[k])]
        sess = _session(G, m, n)
        assert gname in sess._graphs


def test_plain_calls_keep_their_graph_and_another_progression_replays_the_chord_graph(c2, spans):  # noqa: F811
    """Warm calls: plain, chords, another progression, plain again.  The plain
    call uses the same `_graphs` entry object before and after and returns the
    same tokens; the second progression replays the '+bar+chord' graph the
    first one captured; the plain graphs own no chord buffer."""
    from smer_music_generation_amd import generation as G
    m, v, ctl, reqs = c2
    ev, tr, br = reqs[2]
    batch = [(list(ev), tr, br)] * 2
    prog = _prog(G)
    other = [(0, G.pitch_set(60, 84, G.chord_tones(2, 'min7'))), (4, G.pitch_set(classes=G.chord_tones(7, '7')))]
    names = {"g_chordlen", "g_chordat", "g_chordbits"}
    G.clear_decode_sessions(m)
    for mode, kw in (("greedy", dict(greedy=True)), ("rows", dict(greedy=False, seed=[11, 12]))):
        def call(**extra):
            G.generation_batch(m, batch, v, ctl, precision="fp32", logger=_Log(), **kw, **extra)
            return _take(spans, 2)
        before = call()
        sess = _session(G, m, 2)
        plain, keys = sess._graphs[mode], set(sess._graphs)
        a = call(chords={b: prog for b in br})
        name = mode + "+bar+chord"
        entry = sess._graphs[name]
        graph = entry.graph
        assert sess._greedy is entry and set(sess._graphs) == keys | {name}
        b = call(chords=[None, {b: other for b in br}])
        assert _session(G, m, 2) is sess
        assert sess._graphs[name] is entry and entry.graph is graph  # replayed
        assert b[0] == before[0]
        L = G.bar_units(ev)
        assert all(p in _set_at(other, o, L) for o, p in _pitches_of(G, v, b[1], _codes(G, v, reqs[2])))
        assert all(p in _set_at(prog, o, L) for rec in a for o, p in _pitches_of(G, v, rec, _codes(G, v, reqs[2])))
        after = call()
        assert after == before
        assert sess._graphs[mode] is plain and sess._greedy is plain
        assert not names & set(plain.bufs) and names | {"g_clock"} <= set(entry.bufs)

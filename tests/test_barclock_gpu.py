"""The bar clock on the device decode path (csrc/decode_ops.hip
bar_clock_kernel, smer_bar_clock): the kernel alone against the `_BarClock`
mirror, the chain ban -> bar -> template -> grammar entry against the entry on
host-edited logits, then `fill_bar=` on the C2 model: the device decode against
the host loop, and the '+bar' graphs beside the ones without the node."""
import types

import numpy as np
import pytest
import torch

from tests.golden.prod_common import C2, CTRL
from tests.test_prod_gpu import prod_model
from tests.test_template_gpu import (_Log, _case, _per_mask, _session, _t, _tables, _take,
                                     spans)  # noqa: F401  (spans: a fixture)
from tests.test_template_gpu import L as TPL_L
from tests.test_template_gpu import NM as TPL_NM
from tests.test_template_gpu import NM_T as TPL_NM_T

pytestmark = pytest.mark.gpu
dev = "cuda"
NST, CAP, NM, TRASH = 12, 6, 4, 200
FRAME = 8  # sentinel words in front of and behind the clock buffer
SENT = 123456
LIVE = ("end=L-1", "end=L", "pending-sep", "sep-first", "open-group", "whole", "span-start", "close-group")
QUIET = ("done", "bar_len=0", "control-span", "past-masks", "c>cap")
KINDS = LIVE + QUIET


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _units(v, V):
    from smer_music_generation_amd.generation import unit_table
    u = np.zeros(V, dtype=np.uint8)
    u[:v.vocab_size] = unit_table(v)
    return u


def _mirror(V, eos, cls, units, big, st, tg, out, bar_len, clock, cap):
    """smer_bar_clock on the host, from its contract: `clock` (int32 [R, 8])
    and the framed logits `big` edited in place.  Returns the rows that were
    active."""
    from smer_music_generation_amd.generation import _BarClock
    fake = types.SimpleNamespace(vocab_size=V, eos_index=eos)
    active = []
    for r in range(st.shape[0]):
        if st[r, 5]:
            continue
        c, midx = int(st[r, 7]), int(st[r, 3])
        ck = _BarClock(int(bar_len[r]), cls, units)
        ck.T, ck.P, ck.A = (int(x) for x in clock[r, :3])
        ck.G, ck.S, seen = int(clock[r, 3]) & 1, (int(clock[r, 3]) >> 1) & 1, int(clock[r, 4])
        if st[r, 2] == 1:
            ck.reset()
        elif c == seen + 1 and 1 <= c <= cap:
            tok = int(out[r, c - 1]) & 0xFFFF
            if tok < V:
                ck.advance(int(cls[tok]), int(units[tok]))
        clock[r, :5] = (ck.T, ck.P, ck.A, ck.G | ck.S << 1, c)
        if bar_len[r] > 0 and 0 <= midx < tg.shape[1] and tg[r, midx] == 0 and c <= cap:
            big[2 * r + 1, :V][ck.banned(fake)] = np.float32(-100.0)
            active.append(r)
    return active


def _clock_case(V, R, L, shift):
    """R requests, request r of kind KINDS[(r + shift) % 13]; the clock words
    are (T, P, A, G | S << 1, seen)."""
    v, keep, cls, rej = _tables(V)
    units = _units(v, V)
    rng = np.random.default_rng(7000 * V + 100 * R + 10 * L + shift)
    tok = {k: v.char2index(k) for k in ('p_60', 'sep', 'quarter', 'rest', 'whole', 'sixteenth', 'eighth')}
    ldl = V + 3
    big = (rng.standard_normal((2 * R, ldl)) * 3).astype(np.float32)
    big[:, V:] = np.float32(777.0)
    st = np.zeros((R, NST), dtype=np.int32)
    tg = np.zeros((R, NM), dtype=np.int8)
    out = rng.integers(0, V, size=(R, CAP)).astype(np.int32)
    bar_len = np.full(R, L, dtype=np.int32)
    frame = np.full(FRAME + 8 * R + FRAME, SENT, dtype=np.int32)
    clock = frame[FRAME:-FRAME].reshape(R, 8)
    kinds = []
    for r in range(R):
        kind = KINDS[(r + shift) % len(KINDS)]
        kinds.append(kind)
        c, ln, midx = 2 + r % 3, 5, r % NM
        words, last = (3, 2, 0, 0), None  # last: the token the step before emitted (advance), None: seen == c
        if kind == "end=L-1":
            words = (L - 1, 1, 0, 0)
        elif kind == "end=L":
            words = (L - 4, 2, 4, 1)
        elif kind == "pending-sep":
            words = (L, 4, 0, 2)
        elif kind == "sep-first":
            words, ln, last = (0, 0, 0, 0), 2, tok['sep'] | 0x10000  # (bit 16: the redraw-failure flag)
        elif kind == "open-group":
            words, last = (4, 4, 2, 1), tok['quarter']
        elif kind == "whole":
            words, ln, last = (0, 0, 0, 0), 2, tok['p_60']
        elif kind == "span-start":
            words, ln, last = (9, 3, 2, 3), 1, tok['quarter']
        elif kind == "close-group":
            words, last = (8, 4, 2, 3), tok['p_60']
        elif kind == "done":
            st[r, 5], last = 1, tok['quarter']
        elif kind == "bar_len=0":
            bar_len[r], last = 0, tok['quarter']
        elif kind == "control-span":
            tg[r, midx], last = 1 + r % 4, tok['eighth']
        elif kind == "past-masks":
            midx, last = NM, tok['eighth']
        elif kind == "c>cap":
            c, words, last = CAP + 1, (L, 4, 0, 0), tok['quarter']
        st[r, 0], st[r, 2], st[r, 3], st[r, 4], st[r, 7] = 10 + r, ln, midx, NM, c
        clock[r, :4] = words
        clock[r, 4] = c if last is None else c - 1
        if last is not None:
            out[r, min(c, CAP) - 1] = last
    return dict(v=v, V=V, R=R, L=L, cls=cls, units=units, big=big, st=st, tg=tg, out=out, bar_len=bar_len,
                frame=frame, clock=clock, kinds=kinds, tok=tok)


def _shifts(R):
    return range(len(KINDS)) if R == 1 else (0, 5, 10) if R < len(KINDS) else (0,)


@pytest.mark.parametrize("L", [12, 16])
@pytest.mark.parametrize("V", [309, 512])
@pytest.mark.parametrize("R", [1, 5, 33])
def test_bar_clock_kernel_alone(V, R, L):
    """The framed logits and the framed clock buffer after smer_bar_clock
    against the mirror, every 32-bit word; the kinds that must write nothing
    leave their logits row bit for bit, a done row its clock words too; a
    second launch changes nothing (seen)."""
    from smer_music_generation_amd import ops as O
    seen = set()
    for shift in _shifts(R):
        c = _clock_case(V, R, L, shift)
        v, tok = c["v"], c["tok"]
        frame_t, big_t, s_t = _t(c["frame"]), _t(c["big"]), _t(c["st"])
        ck_t = frame_t[FRAME:-FRAME].view(R, 8)
        args = (big_t[:, :V], s_t, _t(c["tg"]), _t(c["out"]), _t(c["cls"]), _t(c["units"]), _t(c["bar_len"]), ck_t)
        O.bar_clock(*args, eos=v.eos_index)
        torch.cuda.synchronize()
        want, wframe = c["big"].copy(), c["frame"].copy()
        active = _mirror(V, v.eos_index, c["cls"], c["units"], want, c["st"], c["tg"], c["out"], c["bar_len"],
                         wframe[FRAME:-FRAME].reshape(R, 8), CAP)
        got, gframe = big_t.cpu().numpy(), frame_t.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert np.array_equal(gframe, wframe)
        assert np.array_equal(s_t.cpu().numpy(), c["st"])
        assert (got[:, V:] == np.float32(777.0)).all() and np.array_equal(got[0::2], c["big"][0::2])
        assert (gframe[:FRAME] == SENT).all() and (gframe[-FRAME:] == SENT).all()
        gck = gframe[FRAME:-FRAME].reshape(R, 8)
        assert (gck[:, 5:] == SENT).all()
        O.bar_clock(*args, eos=v.eos_index)  # the same step again: seen == c, nothing moves
        torch.cuda.synchronize()
        assert np.array_equal(big_t.cpu().numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(frame_t.cpu().numpy(), wframe)
        dur = {k: tok[k] for k in ('whole', 'quarter', 'eighth', 'sixteenth')}
        for r, kind in enumerate(c["kinds"]):
            seen.add(kind)
            row, row0 = got[2 * r + 1, :V], c["big"][2 * r + 1, :V]
            banned = (row == np.float32(-100.0)) & (row0 != np.float32(-100.0))
            if kind in QUIET:
                assert r not in active and np.array_equal(row.view(np.int32), row0.view(np.int32))
                if kind == "done":
                    assert np.array_equal(gck[r], c["clock"][r])
                elif kind == "c>cap":
                    assert gck[r].tolist()[:5] == [L, 4, 0, 0, CAP + 1]
                else:
                    assert gck[r, 4] == c["st"][r, 7] and not np.array_equal(gck[r, :4], c["clock"][r, :4])
                continue
            assert r in active
            if kind == "end=L-1":
                assert not banned[dur['sixteenth']] and banned[[dur['eighth'], dur['quarter'], dur['whole']]].all()
                assert banned[v.eos_index] and not banned[tok['p_60']] and not banned[tok['rest']]
            elif kind == "end=L":
                assert not banned[v.eos_index] and not banned[v.density_indices].any()
                assert banned[v.pitch_indices].all() and banned[[tok['rest'], v.continue_index]].all()
                assert banned[list(dur.values())].all() and not banned[tok['sep']]
            elif kind == "pending-sep":
                assert gck[r].tolist()[:4] == [L, 4, 0, 2]
                assert not banned[tok['p_60']] and not banned[dur['quarter']] and not banned[tok['sep']]
                assert banned[v.eos_index] and banned[v.char2index('half')]
            elif kind == "sep-first":
                assert gck[r].tolist()[:5] == [0, 0, 0, 2, c["st"][r, 7]] and banned[v.eos_index]
            elif kind == "open-group":
                assert gck[r].tolist()[:4] == [4, 4, 6, 1]
                assert banned[dur['whole']] == (4 + 6 + 16 > L) and banned[v.eos_index]
            elif kind == "whole":
                assert banned[dur['whole']] == (L == 12) and not banned[v.char2index('half')]
            elif kind == "span-start":
                assert gck[r].tolist()[:5] == [0, 0, 0, 0, c["st"][r, 7]]
                assert banned[v.eos_index] and banned[v.density_indices].all()
                assert banned.sum() == 1 + 20 + (L == 12)  # <eos>, the 20 control tokens of the table, 'whole' in 3/4
            elif kind == "close-group":
                assert gck[r].tolist()[:4] == [6, 2, 0, 0]
    assert seen == set(KINDS)


def test_bar_clock_checks_its_arguments():
    from smer_music_generation_amd import _lib
    from smer_music_generation_amd import ops as O
    R, V = 2, 309

    def z(*shape, dt=torch.int32):
        return torch.zeros(*shape, dtype=dt, device=dev)
    lg, st, tg, out = torch.zeros(2 * R, V, device=dev), z(R, NST), z(R, 4, dt=torch.int8), z(R, 8)
    cls, un, bl, ck = z(V, dt=torch.uint8), z(V, dt=torch.uint8), z(R), z(R, 8)
    O.bar_clock(lg, st, tg, out, cls, un, bl, ck, eos=1)
    for bad in (dict(lg=torch.zeros(2 * R, 513, device=dev), cls=z(513, dt=torch.uint8), un=z(513, dt=torch.uint8)),
                dict(lg=lg[:3]), dict(ck=z(R, 7)), dict(ck=z(1, 8)), dict(bl=z(R + 1)), dict(un=z(100, dt=torch.uint8)),
                dict(un=z(V)), dict(out=z(R, 8, dt=torch.int64)), dict(tg=z(1, 4, dt=torch.int8))):
        a = dict(lg=lg, st=st, tg=tg, out=out, cls=cls, un=un, bl=bl, ck=ck)
        a.update(bad)
        with pytest.raises(RuntimeError):
            O.bar_clock(a["lg"], a["st"], a["tg"], a["out"], a["cls"], a["un"], a["bl"], a["ck"], eos=1)
    lib = _lib.load()
    p = [t.data_ptr() for t in (lg, st, tg, out, cls, un, bl, ck)]

    def raw(R=R, V=V, ldl=V, nst=NST, nm=4, cap=8, eos=1, null=None):
        q = [None if i == null else x for i, x in enumerate(p)]
        return lib.smer_bar_clock(R, V, q[0], ldl, q[1], nst, q[2], nm, q[3], cap, q[4], q[5], eos, q[6], q[7], None)
    assert raw() == 0
    for kw in (dict(V=513, ldl=513), dict(R=0), dict(ldl=V - 1), dict(nst=8), dict(nm=0), dict(cap=0), dict(eos=V),
               dict(eos=-1), dict(null=0), dict(null=5), dict(null=6), dict(null=7)):
        assert raw(**kw) == -1, kw
        assert b"smer_bar_clock" in lib.smer_last_error()
    assert lib.smer_abi_version() == 1


# ---------------------------------------------------------------------------
# ban -> bar -> template -> entry against the entry on host-edited logits
# ---------------------------------------------------------------------------
def _chain_host_edit(c, big, st, out, bar_len, clock):
    """The three kernels on the host, in the captured step's order."""
    V, is_pitch = c["V"], (c["cls"] & 2).astype(bool)
    for r in range(c["R"]):  # smer_logits_ban
        midx = int(st[r, 3])
        if not st[r, 5] and 0 <= midx < TPL_NM and c["bom"][r, midx] >= 0:
            big[2 * r + 1, :V][c["ban"][r, c["bom"][r, midx]]] = np.float32(-100.0)
    active = _mirror(V, c["v"].eos_index, c["cls"], c["units"], big, st, c["tg"], out, bar_len, clock, CAP)
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
    return active


@pytest.mark.parametrize("V", [309, 512])
@pytest.mark.parametrize("R", [1, 5, 33])
@pytest.mark.parametrize("entry", ["greedy", "greedy_ring", "stream", "rows"])
def test_ban_bar_template_then_grammar_entry_equals_entry_on_edited_logits(entry, V, R):
    """Three steps in a row (fresh logits before each, as the projection
    writes them) on the request mix of tests/test_template_gpu.py, every
    request with a clock in some state and a bar of 12, 16 or 0 (none): state
    rows, out_tok with the fail bit, ids / meta, all 625 words of every MT
    stream, the live count and the clock words, bit for bit.  From the second
    step on the clock advances by a token the device drew."""
    from smer_music_generation_amd import ops as O
    from smer_music_generation_amd.generation import ban_bits
    n_active = n_adv = 0
    for shift in ((0, 1, 3, 7) if R == 1 else (0, 5) if R < 10 else (0,)):
        c = _case(V, R, shift)
        v = c["v"]
        c["units"] = _units(v, V)
        bar_len = np.asarray([(12, 16, 0)[r % 3] for r in range(R)], dtype=np.int32)
        clock0 = np.zeros((R, 8), dtype=np.int32)
        for r in range(R):
            T = (5 * r + shift) % 11
            clock0[r, :5] = (T, min(T, r % 3), 0, 0, c["st"][r, 7])
        frame_t = _t(c["frame"])
        dv = dict(keep=_t(c["keep"]), cls=_t(c["cls"]), rej=_t(c["rej"]), tg=_t(c["tg"]), sl=_t(c["src_len"]),
                  tp=_t(c["tp"]), bom=_t(c["bom"]), units=_t(c["units"]), bl=_t(bar_len),
                  bits=_t(np.stack([ban_bits(c["ban"][r]) for r in range(R)]).view(np.int32)),
                  tape=frame_t[8:-8].view(R, TPL_NM_T, TPL_L))
        gargs = dict(eos=v.eos_index, m0=v.char2index('m_0'), trash_pos=TRASH)
        use_ring = entry.endswith("_ring")
        res = {}
        for on_device in (True, False):
            s_t = _t(c["st"])
            out_t = torch.zeros(R, CAP, dtype=torch.int32, device=dev)
            ctl = torch.zeros(3, dtype=torch.int32, device=dev)
            ring = torch.full((4,), -1, dtype=torch.int32).pin_memory() if use_ring else None
            m_t = _t((c["mt"] if entry == "rows" else c["mt"][0, :625]).view(np.int32))
            ck_t, ck_h = _t(clock0), clock0.copy()
            steps = []
            for step in range(3):
                big = c["big"].copy()
                if not on_device:
                    before = ck_h[:, :4].copy()
                    n_active += len(_chain_host_edit(c, big, s_t.cpu().numpy(), out_t.cpu().numpy(), bar_len, ck_h))
                    n_adv += int((before != ck_h[:, :4]).any(axis=1).sum()) if step else 0
                big_t = _t(big)
                lg_t = big_t[:, :V]
                if on_device:
                    O.logits_ban(lg_t, s_t, dv["bom"], dv["bits"])
                    O.bar_clock(lg_t, s_t, dv["tg"], out_t, dv["cls"], dv["units"], dv["bl"], ck_t, eos=v.eos_index)
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
        a, b = res[True], res[False]
        for (ia, ma, la, sa, ca), (ib, mb, lb, sb, cb) in zip(a[0], b[0]):
            assert np.array_equal(ia, ib) and np.array_equal(ma, mb) and la == lb and np.array_equal(sa, sb)
            assert np.array_equal(ca, cb)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert n_active >= 3 and n_adv >= 1  # not vacuous: rows were clocked, and a drawn token moved a clock


# ---------------------------------------------------------------------------
# the calls on the C2 model
# ---------------------------------------------------------------------------
def _span_checks(G, v, ctl, rec, target_codes, fill, L=16):
    """The span assertions of tests/test_barclock_cpu.py.  Returns how many
    note spans ended on a token."""
    rows, notes, ended = _per_mask(rec), [k for k, t in enumerate(target_codes) if t == 0], 0
    assert len(fill) == len(notes)
    for k, (cursor, bar) in zip(notes, fill):
        body = rows[k]
        on_token = body[-1] == v.eos_index or body[-1] in ctl
        kept = body if on_token else body[:-1]
        assert bar == L and cursor == G.bar_fill(v, [i for i in kept if i != v.eos_index])[0]
        assert G.bar_fill(v, kept)[1] <= L and cursor <= L
        if on_token:
            assert cursor == L
            ended += 1
        else:
            assert len(body) == 99
    return ended


def _codes(G, v, req):
    ev, tr, br = req
    return G._template_bodies(ev, v, tr, br, None)[1]


MODES = {"greedy": (dict(greedy=True), "greedy+bar"),
         "rows": (dict(greedy=False, seed=[3, 4, 5], t=0.9, p=0.95), "rows+bar"),
         "stream": (dict(greedy=False), "stream+bar")}


def _biased(prec):
    """The C2 test model with a bias on its vocabulary head, chosen on the
    host from the grammar alone so that a randomly initialised model writes
    bars: durations ahead of <eos>, <eos> ahead of the pitches, 'rest', 'sep'
    and 'continue' behind them.  (Without it the greedy argmax of the random
    model repeats one token up to the cap and no span ever ends on a token.)
    Greedy then writes pitch, durations up to the bar line, <eos>; without the
    clock <eos> wins the first draw, so the clock changes every take."""
    from smer_music_generation_amd.vocab import WordVocab
    v = WordVocab(0, CTRL)
    m = prod_model(C2, prec).eval()
    with torch.no_grad():
        b = m.fc.bias
        b[v.duration_only_indices] += 12.0
        b[v.eos_index] += 11.0
        b[v.pitch_indices] += 10.0
        b[[v.char2index('rest'), v.char2index('sep'), v.continue_index]] += 9.0
    return m


@pytest.fixture(scope="module")
def c2():
    from smer_music_generation_amd.synth import synth_events
    from smer_music_generation_amd.vocab import WordVocab
    v = WordVocab(0, CTRL)
    ctl = v.density_indices + v.occupation_indices + v.polyphony_indices + v.tensile_indices
    # (the request set of tests/test_template_gpu.py: unequal sources and targets, the last track among them)
    reqs = [(list(synth_events(60 + i, n_bars=6 + 2 * i, n_tracks=3)), [2 - i], [4] if i else [2, 3])
            for i in range(3)]
    return _biased("fp32"), v, ctl, reqs


@pytest.fixture(scope="module")
def c2_bf16(c2):
    _, v, ctl, reqs = c2
    return _biased("bf16"), v, ctl, reqs


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", list(MODES))
def test_device_decode_equals_the_host_loop_under_fill_bar(c2, c2_bf16, spans, mode, prec):  # noqa: F811
    """A batch of three, requests 0 and 2 with fill_bar, request 1 without:
    the device decode (the '+bar' graph of the mode) and the host loop emit
    the same tokens, log lines and bar_fill; unseeded they leave np.random in
    the same state; the span assertions hold; request 1 draws what it draws in
    the call without the keyword (seeded and greedy)."""
    from smer_music_generation_amd import generation as G
    m, v, ctl, reqs = c2 if prec == "fp32" else c2_bf16
    kw, gname = MODES[mode]
    kw = dict(kw, precision="fp32" if prec == "fp32" else None)
    batch = [(list(e), t, b) for e, t, b in reqs]
    G.clear_decode_sessions(m)
    res = {}
    for dg in (False, True):
        np.random.seed(31)
        lg = _Log()
        _, stats = G.generation_batch(m, batch, v, ctl, logger=lg, fill_bar=[True, False, True],
                                      device_grammar=dg, return_stats=True, **kw)
        st = np.random.get_state()
        res[dg] = (_take(spans, 3), lg.lines, stats["tokens"], stats["steps"], stats["bar_fill"],
                   (st[1].copy(), int(st[2])))
    assert res[True][:5] == res[False][:5]
    assert np.array_equal(res[True][5][0], res[False][5][0]) and res[True][5][1] == res[False][5][1]
    recs, fills = res[True][0], res[True][4]
    assert fills[1] is None
    ended = sum(_span_checks(G, v, set(ctl), recs[k], _codes(G, v, reqs[k]), fills[k]) for k in (0, 2))
    print("%s %s: %d note spans ended on a token, bar_fill %r" % (mode, prec, ended, fills))
    assert ended >= 1
    sess = _session(G, m, 3)
    assert gname in sess._graphs and sess._greedy is sess._graphs[gname]
    assert not any("bar" in k for k in sess._graphs if k != gname)
    if mode != "stream":
        G.generation_batch(m, batch, v, ctl, logger=_Log(), **kw)
        free = _take(spans, 3)
        assert free[1] == recs[1] and free[0] != recs[0] and free[2] != recs[2]
        assert gname.replace("+bar", "") in sess._graphs


def test_fill_bar_with_pitches_variations_logprobs_and_a_template(c2, spans):  # noqa: F811
    """pitches= + variations=2 + logprobs=True under fill_bar (the
    'rows+ban+bar+score' graph), and one call under opening_template(keep=2)
    ('rows+bar+tpl'): device and host loop agree on tokens, bar_fill and, to
    2e-3 (the step-versus-step bound of tests/test_score_gpu.py is exact here:
    the same step kernels), the scores."""
    from smer_music_generation_amd import generation as G
    m, v, ctl, reqs = c2
    ev, tr, br = reqs[0]
    codes = _codes(G, v, reqs[0])
    G.clear_decode_sessions(m)
    octave = tuple(range(48, 73))
    tpl = G.opening_template(ev, v, tr, br, keep=2)
    for extra, gname, n in ((dict(pitches=octave, variations=2, logprobs=True), "rows+ban+bar+score", 2),
                            (dict(template=tpl), "rows+bar+tpl", 1)):
        res = {}
        for dg in (False, True):
            stats = {}
            out = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, seed=21, fill_bar=True, stats=stats,
                                   device_grammar=dg, **extra)
            assert out is not None
            res[dg] = (_take(spans, n), stats)
        assert res[True][0] == res[False][0]
        assert res[True][1]["bar_fill"] == res[False][1]["bar_fill"] and len(res[True][1]["bar_fill"]) == n
        for rec, fill in zip(res[True][0], res[True][1]["bar_fill"]):
            _span_checks(G, v, set(ctl), rec, codes, fill)
        if "logprobs" in extra:
            ok = {v.char2index('p_%d' % k) for k in octave}
            assert all(i in ok for rec in res[True][0] for _, i in rec if G._pitch_mask(v)[i])
            for a, b in zip(res[True][1]["logprobs"], res[False][1]["logprobs"]):
                assert len(a) == len(b) and float(np.abs(np.asarray(a) - np.asarray(b)).max()) <= 2e-3
        else:
            bodies = G._template_bodies(ev, v, tr, br, None)[0]
            got = _per_mask(res[True][0][0])
            assert all(got[k][:2] == bodies[k][:2] for k, c in enumerate(codes) if c == 0)
        sess = _session(G, m, n)
        assert gname in sess._graphs


def test_plain_calls_keep_their_graph_and_another_mix_replays_the_bar_graph(c2, spans):  # noqa: F811
    """Warm calls: plain, fill_bar, fill_bar with another request mix, plain
    again.  The plain call uses the same `_graphs` entry object before and
    after and returns the same tokens; the second fill_bar call replays the
    '+bar' graph the first one captured; the plain graphs own no clock
    buffer."""
    from smer_music_generation_amd import generation as G
    m, v, ctl, reqs = c2
    batch = [(list(reqs[2][0]), reqs[2][1], reqs[2][2])] * 2
    G.clear_decode_sessions(m)
    for mode, kw in (("greedy", dict(greedy=True)), ("rows", dict(greedy=False, seed=[11, 12]))):
        def call(**extra):
            G.generation_batch(m, batch, v, ctl, precision="fp32", logger=_Log(), **kw, **extra)
            return _take(spans, 2)
        before = call()
        sess = _session(G, m, 2)
        plain, keys = sess._graphs[mode], set(sess._graphs)
        a = call(fill_bar=True)
        entry = sess._graphs[mode + "+bar"]
        graph = entry.graph
        assert sess._greedy is entry and set(sess._graphs) == keys | {mode + "+bar"}
        b = call(fill_bar=[False, True])
        assert _session(G, m, 2) is sess
        assert sess._graphs[mode + "+bar"] is entry and entry.graph is graph  # replayed
        assert a[0] != before[0] and b[0] == before[0] and b[1] == a[1]
        after = call()
        assert after == before
        assert sess._graphs[mode] is plain and sess._greedy is plain
        assert not {"g_clock", "g_barlen", "g_units"} & set(plain.bufs)
        assert {"g_clock", "g_barlen", "g_units"} <= set(entry.bufs)

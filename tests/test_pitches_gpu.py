"""Pitch constraints on the device decode path (csrc/decode_ops.hip
logits_ban_kernel, smer_logits_ban): the kernel alone, the kernel in front of
each grammar entry against the same entry on host-edited logits, then the
plugin and the batched calls against their host loops and each other."""
import numpy as np
import pytest
import torch

from tests.test_nucleus_gpu import (CTRL, FLAG_SETS, _golden, _Log, _model, _requests, _rng_state,
                                    _same, _state_code, kernel_rows)

pytestmark = pytest.mark.gpu
dev = "cuda"
NST, CAP, TRASH = 12, 4, 200


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(rows):
    from smer_music_generation_amd.generation import ban_bits
    return ban_bits(rows)


# ---------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------
def _patterns(V, pitch):
    """The ban rows of the kernel test: empty, only bit 0, only bit V - 1,
    bits 31 and 32 (a word boundary), all pitches but one."""
    pats = np.zeros((5, V), dtype=bool)
    pats[1, 0] = True
    pats[2, V - 1] = True
    pats[3, [31, 32]] = True
    pats[4, pitch] = True
    pats[4, pitch[40]] = False
    return pats


@pytest.mark.parametrize("V", [309, 512])
@pytest.mark.parametrize("R", [1, 2, 33])
def test_logits_ban_kernel_alone(V, R):
    """Banned entries of the odd rows become exactly -100.f; every other
    32-bit word of the buffer (even rows, columns V .. ldl - 1, unbanned
    entries; NaN payloads and -0.0 included) and the state stay as they are.
    Done rows, masks without a ban row and mask indices past the table are
    left alone; a mask index of 1 reads the request's second ban row.  Thirty
    shifts of the row kinds, so R = 1 meets every one of them."""
    from smer_music_generation_amd import ops as O
    from smer_music_generation_amd.vocab import WordVocab
    v = WordVocab(0, CTRL)
    pats = _patterns(V, np.asarray(v.pitch_indices))
    K, NM, ldl = 3, 4, V + 5
    rng = np.random.default_rng(V + R)
    seen = set()
    for shift in range(30):
        big = (rng.standard_normal((2 * R, ldl)) * 4).astype(np.float32)
        words = big.view(np.int32)
        words[:, 3] = 0x7FC01234            # a NaN with a payload
        words[:, 7] = np.int32(-2 ** 31)    # -0.0
        words[:, V - 1] = np.int32(-8388608 + 77)  # 0xFF80004D: a negative NaN in the last column
        st = rng.integers(0, 50, (R, NST)).astype(np.int32)
        bom = np.zeros((R, NM), dtype=np.int8)
        rows = np.zeros((R, K, V), dtype=bool)
        for r in range(R):
            st[r, 5] = int((r + shift) % 7 == 6)      # done
            st[r, 3] = (r + shift) % 6                # mask index: 4 and 5 lie past the table
            for k in range(K):
                rows[r, k] = pats[(r + shift // 6 + 2 * k) % 5]
            bom[r] = [0, 1, -1, 2] if (r + shift) % 11 != 10 else [-1, -1, -1, -1]
        want = big.copy()
        for r in range(R):
            midx = int(st[r, 3])
            if st[r, 5] or midx >= NM or bom[r, midx] < 0:
                seen.add("done" if st[r, 5] else "past" if midx >= NM else "none")
                continue
            ban = rows[r, bom[r, midx]]
            want[2 * r + 1, :V][ban] = -100.0
            seen.add(("row", int(bom[r, midx]), (r + shift // 6 + 2 * int(bom[r, midx])) % 5))
        big_t, st_t = _t(big), _t(st)
        bits = np.stack([_bits(rows[r]) for r in range(R)]).view(np.int32)
        O.logits_ban(big_t[:, :V], st_t, _t(bom), _t(bits))
        torch.cuda.synchronize()
        got = big_t.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert np.array_equal(st_t.cpu().numpy(), st)
        hit = want.view(np.int32) != big.view(np.int32)
        assert (want[hit] == np.float32(-100.0)).all() and not hit[0::2].any() and not hit[:, V:].any()
    assert {"done", "past", "none"} <= seen
    for pat in range(5):  # every pattern was the live ban row, and the second row was read
        assert any(x[0] == "row" and x[2] == pat for x in seen if isinstance(x, tuple))
    assert any(x[0] == "row" and x[1] == 1 for x in seen if isinstance(x, tuple))


def test_logits_ban_checks_its_arguments():
    from smer_music_generation_amd import _lib
    from smer_music_generation_amd import ops as O
    R = 2
    lg = torch.zeros(2 * R, 309, device=dev)
    st = torch.zeros(R, NST, dtype=torch.int32, device=dev)
    bom = torch.full((R, 4), -1, dtype=torch.int8, device=dev)
    bits = torch.zeros(R, 2, 16, dtype=torch.int32, device=dev)
    O.logits_ban(lg, st, bom, bits)
    with pytest.raises(RuntimeError):  # V > 512
        O.logits_ban(torch.zeros(2 * R, 513, device=dev), st, bom, bits)
    with pytest.raises(RuntimeError):  # one logits row pair per request
        O.logits_ban(lg[:3], st, bom, bits)
    with pytest.raises(RuntimeError):
        O.logits_ban(lg, st, bom, bits[:, :, :8].contiguous())
    lib = _lib.load()
    assert lib.smer_logits_ban(R, 513, lg.data_ptr(), 513, st.data_ptr(), NST, 4, bom.data_ptr(),
                               bits.data_ptr(), 2, None) == -1
    assert b"smer_logits_ban" in lib.smer_last_error()
    assert lib.smer_abi_version() == 1


# ---------------------------------------------------------------------------
# the kernel in front of each grammar entry
# ---------------------------------------------------------------------------
def _entry_case():
    """9 requests of four masks: ban row 0, ban row 1, none, ban row 0 again
    (requests 2 and 4 start at their second mask).  Rows 0-4: random halves of the pitches
    banned, the row's best kept token among them where it is a pitch; row 5:
    a pitch state whose maximum logit is banned; row 6: the in-continue state
    (after a continue token only pitches pass the redraw check), the other
    kept tokens at exactly -100 and every pitch but one banned -- everything
    kept but that pitch sits at -100; row 7: a nucleus row (p = 0.5) whose
    neighbours of the threshold crossing are banned; row 8: done."""
    from smer_music_generation_amd.generation import grammar_tables, reject_table
    from smer_music_generation_amd.vocab import WordVocab
    v = WordVocab(0, CTRL)
    V = v.vocab_size
    keep, cls = grammar_tables(v, v.density_indices + v.occupation_indices)
    rej = reject_table(v)
    pitch = np.asarray(v.pitch_indices)
    R = 9
    rows, tps = kernel_rows(V, n_rows=40, seed=21)
    rng = np.random.default_rng(5)
    st = np.zeros((R, NST), dtype=np.int32)
    tg = np.zeros((R, 4), dtype=np.int8)
    lg = (rng.standard_normal((2 * R, V)) * 3).astype(np.float32)
    tp = np.zeros((R, 2), dtype=np.float64)
    ban = np.zeros((R, 2, V), dtype=bool)
    fsets = [FLAG_SETS[i] for i in (2, 4, 6, 0, 1)] + [(4, 5, 0), (2, 5, 0), (2, 5, 0), (4, 5, 0)]
    for r in range(R):
        f, ln, tgc = fsets[r]
        st[r, 0] = 10 + r % 3
        st[r, 1], st[r, 2] = f, ln
        st[r, 4] = 4
        st[r, 7] = r % 3
        tg[r] = (tgc, 0, 1, 0)
        st[r, 3] = int(r in (2, 4))
        if r < 5:
            i = (6, 13, 20, 27, 34)[r]  # five (t, p) kinds, three row kinds
            lg[2 * r + 1] = rows[i]
            t, p = tps[i]
            tp[r] = (t, -1.0 if p is None else p)
        else:
            tp[r] = (1.0, 0.5 if r == 7 else -1.0)
        kp = keep[_state_code(f, ln, tgc)].astype(bool)
        row = lg[2 * r + 1]
        for k in range(2):
            ban[r, k, rng.choice(pitch, size=44, replace=False)] = True
        best = int(np.argmax(np.where(kp, row, -np.inf)))
        if r == 5:
            row[pitch[30]] = row.max() + 2.0   # the row's maximum: a pitch, banned
            best = int(pitch[30])
        if best in pitch:
            ban[r, st[r, 3], best] = True
        if r == 6:
            keep_pitch = row[pitch].copy()
            row[:] = -100.0
            row[pitch] = keep_pitch
            ban[r, 0, pitch] = True
            ban[r, 0, pitch[50]] = False
        if r == 7:
            ban[r, 0] = False
            x = np.where(kp, row.astype(np.float64), -100.0)
            e = np.exp(x)
            q = e / e.sum()
            order = np.argsort(q)[::-1]
            c = int(np.flatnonzero(np.cumsum(q[order]) > 0.5)[0])
            near = [int(order[j]) for j in (c - 2, c - 1, c + 1, c + 2) if j >= 0 and order[j] in pitch]
            assert near
            ban[r, 0, near] = True
    st[8, 5] = 1
    assert ban[5, 0, pitch[30]] and ban[6, 0].sum() == len(pitch) - 1
    bom = np.tile(np.array([0, 1, -1, 0], dtype=np.int8), (R, 1))
    src_len = (3 + np.arange(R) % 5).astype(np.int32)
    mt = np.zeros((R, 640), dtype=np.uint32)
    for r in range(R):
        s0 = np.random.RandomState(100 + r).get_state()
        mt[r, :624], mt[r, 624] = s0[1], 624
    return dict(v=v, V=V, R=R, keep=keep, cls=cls, rej=rej, st=st, tg=tg, lg=lg, tp=tp, ban=ban, bom=bom,
                src_len=src_len, mt=mt)


@pytest.mark.parametrize("entry", ["greedy", "greedy_ring", "stream", "rows", "rows_ring"])
def test_ban_kernel_then_grammar_entry_equals_entry_on_edited_logits(entry):
    """smer_logits_ban + the entry, two steps in a row (fresh logits before
    each step, as the projection writes them), against the entry alone on
    logits edited on the host with np.where from the state the step starts
    in: state rows, out_tok with the fail bit, ids / meta, all 625 words of
    every MT stream and the live count, bit for bit."""
    from smer_music_generation_amd import ops as O
    c = _entry_case()
    v, R = c["v"], c["R"]
    keep_t, cls_t, rej_t = _t(c["keep"]), _t(c["cls"]), _t(c["rej"])
    bits = np.stack([_bits(c["ban"][r]) for r in range(R)]).view(np.int32)
    bom_t, bits_t, tg_t, sl_t, tp_t = _t(c["bom"]), _t(bits), _t(c["tg"]), _t(c["src_len"]), _t(c["tp"])
    gargs = dict(eos=v.eos_index, m0=v.char2index('m_0'), trash_pos=TRASH)
    use_ring = entry.endswith("_ring")
    res = {}
    edited_rows = 0
    for device_ban in (True, False):
        s_t = _t(c["st"])
        out_t = torch.zeros(R, CAP, dtype=torch.int32, device=dev)
        ctl = torch.zeros(3, dtype=torch.int32, device=dev)
        ring = torch.full((4,), -1, dtype=torch.int32).pin_memory() if use_ring else None
        m_t = _t((c["mt"] if entry.startswith("rows") else c["mt"][0, :625]).view(np.int32))
        steps = []
        for step in range(2):
            lg = c["lg"].copy()
            if not device_ban:
                sh = s_t.cpu().numpy()
                for r in range(R):
                    k = c["bom"][r, sh[r, 3]] if sh[r, 3] < 4 else -1
                    if not sh[r, 5] and k >= 0:
                        lg[2 * r + 1] = np.where(c["ban"][r, k], np.float32(-100.0), lg[2 * r + 1])
                        edited_rows += 1
            lg_t = _t(lg)
            if device_ban:
                O.logits_ban(lg_t, s_t, bom_t, bits_t)
            ids_t = torch.full((2 * R,), -7, dtype=torch.int64, device=dev)
            meta_t = torch.full((4, 2 * R), -9, dtype=torch.int32, device=dev)
            if entry.startswith("greedy"):
                O.grammar_greedy_step(lg_t, s_t, tg_t, keep_t, cls_t, sl_t, ids_t, meta_t, out_t, ctl,
                                      ring=ring, **gargs)
            elif entry == "stream":
                O.grammar_sample_step(lg_t, s_t, tg_t, keep_t, rej_t, cls_t, sl_t, ids_t, meta_t, out_t, m_t,
                                      ctl, tp=tp_t, **gargs)
            else:
                O.grammar_sample_step_rows(lg_t, s_t, tg_t, keep_t, rej_t, cls_t, sl_t, ids_t, meta_t, out_t,
                                           m_t, ctl, ring=ring, tp=tp_t, **gargs)
            torch.cuda.synchronize()
            live = int(ring[step]) if use_ring else int(ctl[0].item())
            steps.append((ids_t.cpu().numpy(), meta_t.cpu().numpy(), live, s_t.cpu().numpy()))
        res[device_ban] = (steps, out_t.cpu().numpy(), m_t.cpu().numpy())
    a, b = res[True], res[False]
    for (ia, ma, la, sa), (ib, mb, lb, sb) in zip(a[0], b[0]):
        assert np.array_equal(ia, ib) and np.array_equal(ma, mb) and la == lb and np.array_equal(sa, sb)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # not vacuous: rows were edited on both steps, the requests drew, some moved to their second mask
    assert edited_rows > R and a[0][0][2] == 8 and a[0][1][2] == 8
    final = a[0][1][3]
    assert (final[:8, 7] == c["st"][:8, 7] + 2).all() and final[8, 7] == c["st"][8, 7]
    # no banned token came out of the first step, except through the e^-100 tail (never here)
    first = a[1][np.arange(R), c["st"][:, 7] % CAP] & 0xFFFF
    for r in range(8):
        assert not c["ban"][r, c["st"][r, 3], first[r]], (r, int(first[r]))
    assert first[6] == c["v"].pitch_indices[50] and first[5] != c["v"].pitch_indices[30]


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _str(res):
    if res is None:
        return None
    return (None if res[0] is None else [str(x) for x in res[0]], res[1], res[2])


def _sessions(G, m, R):
    return [s for s in G._BATCH_SESSIONS.values() if s.R == R and s.model is m]


@pytest.fixture(scope="module")
def micro(golden_dir):
    from smer_music_generation_amd.synth import synth_events
    from smer_music_generation_amd.vocab import WordVocab
    z, meta = _golden(golden_dir)
    reqs, ctl = _requests(golden_dir, 5)
    two = (synth_events(61, n_bars=7, n_tracks=3), [0, 2], [2])  # two masked tracks, the last among them
    return _model(z, meta, "fp32"), WordVocab(0, CTRL), reqs, ctl, two


@pytest.fixture
def spans(monkeypatch):
    """Every _Span made during the test, each with `rec`: its committed
    (mask index, id) pairs -- the emitted tokens with the span they belong
    to, whatever the final splice makes of them (the micro model now and then
    draws an 'm_0' inside a span, which the splice rejects: the reference's
    IndexError)."""
    from smer_music_generation_amd import generation as G
    made = []
    init, commit, splice = G._Span.__init__, G._Span.commit, G.restore_marked_input

    def init2(self, *a, **k):
        init(self, *a, **k)
        self.rec = []
        made.append(self)

    def commit2(self, idx):
        self.rec.append((self.mask_idx, int(idx)))
        return commit(self, idx)

    def lenient(src, gen):
        try:
            return [str(x) for x in splice(src, gen)]
        except IndexError:
            return None
    monkeypatch.setattr(G._Span, "__init__", init2)
    monkeypatch.setattr(G._Span, "commit", commit2)
    monkeypatch.setattr(G, "restore_marked_input", lenient)
    return made


def _take(made, n=1):
    """The records of the last n spans made (a device call that falls back to
    the host loop makes fresh ones), and forget them all."""
    out = [list(sp.rec) for sp in made[-n:]]
    kept = list(made[-n:])
    del made[:]
    return out, kept


def _ok_ids(v, notes):
    return {v.char2index('p_%d' % n) for n in notes}


def _inside(v, sp, rec, allowed):
    """Every pitch token emitted in a span of a constrained track is in that
    track's set.  allowed: {ban row: set of token ids}.  Returns the number of
    pitch tokens checked."""
    pitch = set(v.pitch_indices)
    n = 0
    for midx, idx in rec:
        k = sp.ban_of_mask[midx] if sp.ban_of_mask is not None and midx < len(sp.ban_of_mask) else -1
        if k >= 0 and idx in pitch:
            assert idx in allowed[k], (midx, idx)
            n += 1
    return n


OCTAVE = tuple(range(60, 72))
LOW = tuple(range(36, 48))
MID = tuple(range(48, 84))
HIGH = tuple(range(84, 97))

# The micro model ends most 'r' spans on their first token, and more often
# under a constraint, so the requests, sets and seeds below are ones whose
# HOST-LOOP run emits pitches in the constrained spans (fp32: reproducible);
# every test asserts that it does.  name: (keywords, pitches, request: an
# index into the fixture's list, or "two")
PLUGIN_CASES = {
    "greedy": (dict(greedy=True), HIGH, 4),
    "t1": (dict(seed=11), OCTAVE, 0),
    "tp": (dict(seed=7, t=0.8, p=0.9), OCTAVE, 0),
    "dict": (dict(seed=7), {2: LOW}, "two"),
}


@pytest.mark.parametrize("case", list(PLUGIN_CASES))
def test_plugin_paths_agree_under_a_constraint(micro, spans, case):
    """generation_all(pitches=..., seed=s) at fp32: the device path, the host
    loop and use_kv_cache=False emit the same tokens span by span, log the
    same redraw lines and take the same steps; np.random is left alone; every
    pitch of a constrained span is in its set (on the host loop first).  The
    greedy plugin call runs the host loop by design, so its device leg is the
    batched greedy call on the one request (the 'greedy+ban' graph)."""
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl, two = micro
    kw, pit, which = PLUGIN_CASES[case]
    ev, tr, br = two if which == "two" else reqs[which]
    allowed = {0: _ok_ids(v, pit[2] if case == "dict" else pit)}
    G.clear_decode_sessions(m)
    np.random.seed(3)
    st0 = _rng_state()
    runs = []
    for path in (dict(device_grammar=False), dict(use_kv_cache=False), dict()):
        lg, stats = _Log(), {}
        res = G.generation_all(m, list(ev), dev, v, lg, ctl, tr, br, pitches=pit, stats=stats, **kw, **path)
        (rec,), (sp,) = _take(spans)
        n = _inside(v, sp, rec, allowed)
        assert n > 0 and sp.done
        runs.append((rec, lg.lines, stats["steps"], _str(res)))
        assert _same(_rng_state(), st0)
        assert stats["pitches"] == G._check_pitches(pit, tr)
    assert runs[0] == runs[1] and runs[0] == runs[2]
    if case == "dict":  # track 0 is unconstrained, and drew outside track 2's set
        assert sp.ban_of_mask == [-1] * 4 + [0] * 5
        assert any(i in v.pitch_indices and i not in allowed[0] for k, i in runs[0][0] if k < 4)
    if case == "greedy":
        for dg in (True, False):
            lg = _Log()
            _, stats = G.generation_batch(m, [(list(ev), tr, br)], v, ctl, greedy=True, logger=lg,
                                          precision="fp32", pitches=pit, device_grammar=dg,
                                          return_stats=True)
            (rec,), _ = _take(spans)
            assert (rec, lg.lines, stats["steps"]) == runs[0][:3]
        sess = _sessions(G, m, 1)
        assert sess and "greedy+ban" in sess[0]._graphs and "greedy" not in sess[0]._graphs
    else:
        sess = _sessions(G, m, 1)
        assert sess and set(sess[0]._graphs) == {"rows+ban"}
    # the constraint matters: without it the same call leaves the set
    res = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, **kw)
    (free,), _ = _take(spans)
    assert free != runs[0][0]


def test_unseeded_device_and_host_loop_share_the_stream(micro, spans):
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl, _ = micro
    ev, tr, br = reqs[0]
    G.clear_decode_sessions(m)
    res = {}
    for dg in (False, True):
        np.random.seed(4)
        lg = _Log()
        G.generation_all(m, list(ev), dev, v, lg, ctl, tr, br, pitches=OCTAVE, t=0.9, device_grammar=dg)
        (rec,), (sp,) = _take(spans)
        assert _inside(v, sp, rec, {0: _ok_ids(v, OCTAVE)}) > 0
        res[dg] = (rec, lg.lines, _rng_state())
    assert res[True][:2] == res[False][:2] and _same(res[True][2], res[False][2])
    np.random.seed(4)
    assert not _same(_rng_state(), res[True][2])  # draws were taken from np.random
    sess = _sessions(G, m, 1)
    assert sess and set(sess[0]._graphs) == {"stream+ban"}


def test_batch_with_one_constraint_per_request(micro, spans):
    """pitches=[None, A, {track: B}].  Seeded: request 0 draws what the call
    without pitches draws, each constrained request what its own single call
    draws.  Unseeded (the shared stream): the device batch is the host-loop
    batch, tokens, redraw lines and final np.random state."""
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl, _ = micro
    reqs = reqs[:3]
    batch = [(list(e), t, b) for e, t, b in reqs]
    pit = [None, OCTAVE, {2: MID}]
    allowed = [None, {0: _ok_ids(v, OCTAVE)}, {0: _ok_ids(v, MID)}]
    seeds = [6, 7, 8]
    G.clear_decode_sessions(m)
    np.random.seed(2)
    st0 = _rng_state()
    _, stats = G.generation_batch(m, batch, v, ctl, greedy=False, seed=seeds, precision="fp32", pitches=pit,
                                  return_stats=True)
    recs, sps = _take(spans, 3)
    assert _same(_rng_state(), st0)
    assert stats["pitches"] == [None, {1: OCTAVE}, {2: MID}]
    assert sps[0].ban_of_mask is None
    for i in (1, 2):
        assert _inside(v, sps[i], recs[i], allowed[i]) > 0
    sess = _sessions(G, m, 3)
    assert sess and set(sess[0]._graphs) == {"rows+ban"}
    G.generation_batch(m, batch, v, ctl, greedy=False, seed=seeds, precision="fp32")
    free, _ = _take(spans, 3)
    assert free[0] == recs[0] and free[1] != recs[1] and free[2] != recs[2]
    for i in (1, 2):
        ev, tr, br = reqs[i]
        G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, seed=seeds[i], pitches=pit[i])
        (rec,), _ = _take(spans)
        assert rec == recs[i]
    res = {}
    for dg in (False, True):
        np.random.seed(15)
        lg = _Log()
        _, stats = G.generation_batch(m, batch, v, ctl, greedy=False, logger=lg, precision="fp32",
                                      pitches=pit, t=[1.0, 0.7, 1.3], p=[None, 0.9, 0.5],
                                      device_grammar=dg, return_stats=True)
        recs, sps = _take(spans, 3)
        for i in (1, 2):
            assert _inside(v, sps[i], recs[i], allowed[i]) > 0
        res[dg] = (recs, lg.lines, stats["tokens"], stats["steps"], _rng_state())
    assert res[True][:4] == res[False][:4] and _same(res[True][4], res[False][4])
    assert "stream+ban" in sess[0]._graphs


def test_another_set_replays_and_unconstrained_calls_keep_their_tokens(micro, spans):
    """Warm plugin calls: unconstrained, constrained, another set,
    unconstrained again (seeded), and the same round on the batched greedy
    call.  The second set replays the '+ban' entry the first one captured;
    the unconstrained graph is another entry, untouched by the constrained
    calls, and gives the tokens it gave before them."""
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl, _ = micro
    G.clear_decode_sessions(m)
    np.random.seed(1)

    def seeded(**kw):
        ev, tr, br = reqs[0]
        G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, seed=11, **kw)
        (rec,), (sp,) = _take(spans)
        return rec, sp

    def greedy(**kw):
        ev, tr, br = reqs[3]
        G.generation_batch(m, [(list(ev), tr, br)], v, ctl, greedy=True, precision="fp32", logger=_Log(),
                           **kw)
        (rec,), (sp,) = _take(spans)
        return rec, sp
    for call, mode, A, B in ((seeded, "rows", OCTAVE, LOW), (greedy, "greedy", HIGH, MID)):
        before, _ = call()
        sess = _sessions(G, m, 1)[0]
        plain = sess._graphs[mode]
        a, sp_a = call(pitches=A)
        entry = sess._graphs[mode + "+ban"]
        graph = entry.graph
        assert sess._greedy is entry
        b, sp_b = call(pitches=B)
        assert _sessions(G, m, 1)[0] is sess
        assert sess._graphs[mode + "+ban"] is entry and entry.graph is graph  # replayed
        assert _inside(v, sp_a, a, {0: _ok_ids(v, A)}) > 0
        assert _inside(v, sp_b, b, {0: _ok_ids(v, B)}) > 0
        assert a != b and a != before
        after, _ = call()
        assert after == before
        assert sess._graphs[mode] is plain and sess._greedy is plain


def test_takes_of_a_constrained_request_share_its_constraint(micro, spans):
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl, _ = micro
    ev, tr, br = reqs[0]
    stats = {}
    G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, variations=3, pitches=MID, seed=16,
                     stats=stats)
    takes, sps = _take(spans, 3)
    assert stats["seeds"] == [16, 17, 18] and stats["pitches"] == {0: MID}
    for k in range(3):
        assert _inside(v, sps[k], takes[k], {0: _ok_ids(v, MID)}) > 0
        G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, pitches=MID, seed=16 + k)
        (rec,), _ = _take(spans)
        assert rec == takes[k]
    assert len({tuple(t) for t in takes}) > 1  # the takes differ

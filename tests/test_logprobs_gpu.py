"""Take scores on the device decode path (csrc/decode_ops.hip
logprob_stage_kernel / logprob_commit_kernel, smer_logprob_stage /
smer_logprob_commit): the kernels alone against generation.token_logprobs,
the pair around each grammar entry (which must not notice it), then the
plugin and the batched calls against their host loops and each other."""
import numpy as np
import pytest
import torch

from tests.test_nucleus_gpu import CTRL, _golden, _Log, _model, _requests, _rng_state, _same, _state_code
from tests.test_pitches_gpu import OCTAVE, _entry_case, _sessions, _str, _take, spans  # noqa: F401 (spans: a fixture)

pytestmark = pytest.mark.gpu
dev = "cuda"
NST, CAP, TRASH, NM = 12, 4, 200, 4
TOL = 1e-9  # <= 512 float64 terms err by about 1e-13: four orders of margin
NAN64 = np.int64(0x7FF8000000001234)  # a float64 NaN with a payload: "never written"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _lp(row, keep):
    from smer_music_generation_amd.generation import token_logprobs
    return token_logprobs(row, keep)


# ---------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------
# (flags, len, target, no_whole) of the 13 grammar states, in code order
STATES = [(1, 5, 0, 0), (2, 5, 0, 0), (4, 5, 0, 0), (4, 5, 0, 1), (8, 5, 0, 0), (8, 5, 0, 1),
          (0, 1, 1, 0), (0, 1, 2, 0), (0, 1, 3, 0), (0, 1, 4, 0), (0, 1, 0, 1), (0, 7, 2, 0), (0, 7, 2, 1)]
KINDS = ("random", "plus800", "kept-300", "ties-100", "done", "overcap")


def _code(f, ln, tg, nw):
    return (0 if f & 1 else 1 if f & 2 else 2 + nw if f & 4 else 4 + nw if f & 8 else
            (10 if tg == 0 else 5 + tg) if ln == 1 else 11 + nw)


def _keep_table(V):
    """The vocabulary's own table at V = 309, a random one at 512; column
    `mcol` is masked in every state (a NaN logit is planted there)."""
    if V == 309:
        from smer_music_generation_amd.generation import grammar_tables
        from smer_music_generation_amd.vocab import WordVocab
        v = WordVocab(0, CTRL)
        keep, _ = grammar_tables(v, v.density_indices + v.occupation_indices)
        keep = keep.astype(bool)
    else:
        keep = np.random.default_rng(V).random((13, V)) < 0.6
        keep[:, 5] = False
        keep[:, V - 1] = True
    mcol = int(np.flatnonzero(~keep.any(axis=0))[0])
    assert all(2 <= k.sum() < V for k in keep)
    return keep, mcol


@pytest.mark.parametrize("V", [309, 512])
@pytest.mark.parametrize("R", [1, 2, 33])
def test_logprob_kernels_alone(V, R):
    """Stage: the scratch rows of the live requests are token_logprobs of the
    odd logits rows under the keep of the state's grammar code, the stage
    slots their counts (-1: done, scratch row untouched); logits (even rows,
    columns >= V, NaN payloads, -0.0) and state are bit for bit what they
    were.  Commit, on a hand-filled out_tok: exactly the entries of the
    requests that drew in this step change, each to the scratch value at id &
    0xFFFF.  Twenty-six shifts of the six row kinds and the thirteen states:
    R = 1 meets every kind, and every state in a live request."""
    from smer_music_generation_amd import ops as O
    keep, mcol = _keep_table(V)
    keep_t = _t(keep.astype(np.uint8))
    ldl, ldp = V + 5, V + 3
    rng = np.random.default_rng(100 * V + R)
    seen_kind, seen_code, worst, wrote, masked_hit = set(), set(), 0.0, 0, 0
    for shift in range(26):
        big = (rng.standard_normal((2 * R, ldl)) * 2).astype(np.float32)
        words = big.view(np.int32)
        words[0::2, 3] = 0x7FC01234             # NaN payloads in the rows of the first fed tokens
        words[:, V + 1] = np.int32(-8388608 + 77)  # and past the vocabulary
        words[1::2, 7] = np.int32(-2 ** 31)     # -0.0 in the rows that are read
        words[1::2, mcol] = 0x7FC00055          # a NaN under the mask: never looked at
        st = rng.integers(0, 50, (R, NST)).astype(np.int32)
        tg = rng.integers(0, 5, (R, NM)).astype(np.int8)
        kinds, codes = [], []
        for r in range(R):
            kind = KINDS[(r + shift) % 6]
            f, ln, tgc, nw = STATES[(r + shift) % 13]
            code = _code(f, ln, tgc, nw)
            st[r, 1], st[r, 2], st[r, 6] = f, ln, nw
            st[r, 3] = (r + shift) % NM
            tg[r, st[r, 3]] = tgc
            st[r, 5] = int(kind == "done")
            st[r, 7] = CAP + r % 3 if kind == "overcap" else (r + shift) % CAP
            row, kp = big[2 * r + 1, :V], keep[code]
            kept = np.flatnonzero(kp)
            if kind == "plus800":
                row[kept[[0, -1]]] = 800.0
            elif kind == "kept-300":   # the masked entries, at -100, dominate
                row[kept] = -300.0
            elif kind == "ties-100":   # kept entries tie with the masked ones, but one
                row[kept] = -100.0
                row[kept[len(kept) // 2]] = 2.5
            kinds.append(kind)
            codes.append(code)
            seen_kind.add(kind)
            if kind != "done":
                seen_code.add(code)
        words = words.copy()
        big_t, st_t, tg_t = _t(big), _t(st), _t(tg)
        scr_t = _t(np.full((R, ldp), NAN64).view(np.float64))
        stage_t = torch.full((R,), -7, dtype=torch.int32, device=dev)
        O.logprob_stage(big_t[:, :V], st_t, tg_t, keep_t, scr_t, stage_t)
        torch.cuda.synchronize()
        assert np.array_equal(big_t.cpu().numpy().view(np.int32), words)
        assert np.array_equal(st_t.cpu().numpy(), st) and np.array_equal(tg_t.cpu().numpy(), tg)
        scr, stage = scr_t.cpu().numpy(), stage_t.cpu().numpy()
        assert (scr.view(np.int64)[:, V:] == NAN64).all()
        for r in range(R):
            if kinds[r] == "done":
                assert stage[r] == -1 and (scr[r].view(np.int64) == NAN64).all()
                continue
            assert stage[r] == st[r, 7]
            want = _lp(big[2 * r + 1, :V], keep[codes[r]])
            assert np.isfinite(want).all() and np.isfinite(scr[r, :V]).all()
            err = float(np.abs(scr[r, :V] - want).max())
            print("stage V=%d R=%d shift=%d r=%d %s code=%d err=%.3g" % (V, R, shift, r, kinds[r], codes[r], err))
            worst = max(worst, err)
            assert err < TOL, (kinds[r], codes[r], err)
            assert abs(np.exp(scr[r, :V]).sum() - 1.0) < 1e-9
        # commit: most requests "drew" (count + 1), every fifth did not
        st2 = st.copy()
        drew = np.array([(r + shift) % 5 != 4 for r in range(R)])
        st2[drew, 7] += 1
        tok = rng.integers(0, V, (R, CAP)).astype(np.int32)
        for r in range(R):
            if (r + shift) % 4 == 1:  # a masked id at the entry this step wrote
                tok[r, st[r, 7] % CAP] = int(np.flatnonzero(~keep[codes[r]])[-1])
        fail = rng.random((R, CAP)) < 0.4
        out_tok = tok | (fail.astype(np.int32) << 16)
        lp_t = _t(np.full((R, CAP), NAN64).view(np.float64))
        st2_t, tok_t = _t(st2), _t(out_tok)
        O.logprob_commit(st2_t, stage_t, tok_t, scr_t, lp_t, V=V)
        torch.cuda.synchronize()
        want = np.full((R, CAP), NAN64)
        for r in range(R):
            c = int(st[r, 7])
            if kinds[r] in ("done", "overcap") or not drew[r]:
                continue
            want[r, c] = scr[r, tok[r, c]].view(np.int64)
            wrote += 1
            masked_hit += int(not keep[codes[r]][tok[r, c]])
            assert fail[r, c] == bool(out_tok[r, c] >> 16)
        assert np.array_equal(lp_t.cpu().numpy().view(np.int64), want)
        assert np.array_equal(st2_t.cpu().numpy(), st2) and np.array_equal(tok_t.cpu().numpy(), out_tok)
        assert np.array_equal(scr_t.cpu().numpy().view(np.int64), scr.view(np.int64))
        assert np.array_equal(stage_t.cpu().numpy(), stage)
    assert seen_kind == set(KINDS) and seen_code == set(range(13))
    assert wrote > 0 and masked_hit > 0 and worst < TOL


def test_logprob_entries_check_their_arguments():
    from smer_music_generation_amd import _lib
    from smer_music_generation_amd import ops as O
    R, V = 2, 309

    def bufs(V=V, ldp=512):
        return dict(lg=torch.zeros(2 * R, V, device=dev),
                    st=torch.zeros(R, NST, dtype=torch.int32, device=dev),
                    tg=torch.zeros(R, NM, dtype=torch.int8, device=dev),
                    keep=torch.ones(13, V, dtype=torch.uint8, device=dev),
                    scr=torch.zeros(R, ldp, dtype=torch.float64, device=dev),
                    stage=torch.zeros(R, dtype=torch.int32, device=dev),
                    tok=torch.zeros(R, CAP, dtype=torch.int32, device=dev),
                    lp=torch.zeros(R, CAP, dtype=torch.float64, device=dev))
    b = bufs()
    O.logprob_stage(b["lg"], b["st"], b["tg"], b["keep"], b["scr"], b["stage"])
    O.logprob_commit(b["st"], b["stage"], b["tok"], b["scr"], b["lp"], V=V)
    torch.cuda.synchronize()
    assert b["stage"].cpu().tolist() == [0, 0]
    assert np.allclose(b["scr"][:, :V].cpu().numpy(), -np.log(V), atol=1e-12)
    big = bufs(V=513, ldp=600)
    with pytest.raises(RuntimeError):  # V > 512
        O.logprob_stage(big["lg"], big["st"], big["tg"], big["keep"], big["scr"], big["stage"])
    with pytest.raises(RuntimeError):
        O.logprob_commit(big["st"], big["stage"], big["tok"], big["scr"], big["lp"], V=513)
    with pytest.raises(RuntimeError):  # a wrong dtype
        O.logprob_stage(b["lg"], b["st"], b["tg"], b["keep"], b["scr"].float(), b["stage"])
    with pytest.raises(RuntimeError):
        O.logprob_commit(b["st"], b["stage"], b["tok"], b["scr"], b["lp"].float(), V=V)
    with pytest.raises(RuntimeError):
        O.logprob_stage(b["lg"].double(), b["st"], b["tg"], b["keep"], b["scr"], b["stage"])
    short = bufs(ldp=V - 1)
    with pytest.raises(RuntimeError):  # a short scratch row
        O.logprob_stage(b["lg"], b["st"], b["tg"], b["keep"], short["scr"], b["stage"])
    with pytest.raises(RuntimeError):
        O.logprob_commit(b["st"], b["stage"], b["tok"], short["scr"], b["lp"], V=V)
    with pytest.raises(RuntimeError):  # one logits row pair per request
        O.logprob_stage(b["lg"][:3], b["st"], b["tg"], b["keep"], b["scr"], b["stage"])
    lib = _lib.load()
    p = {k: x.data_ptr() for k, x in b.items()}
    assert lib.smer_logprob_stage(R, 513, p["lg"], 513, p["st"], NST, p["tg"], NM, p["keep"], p["scr"], 600,
                                  p["stage"], None) == -1
    assert b"smer_logprob_stage" in lib.smer_last_error()
    assert lib.smer_logprob_stage(R, V, p["lg"], V, p["st"], NST, p["tg"], NM, p["keep"], p["scr"], V - 1,
                                  p["stage"], None) == -1
    assert b"smer_logprob_stage" in lib.smer_last_error()
    assert lib.smer_logprob_commit(R, 513, p["st"], NST, p["stage"], p["tok"], CAP, p["scr"], 600, p["lp"],
                                   None) == -1
    assert b"smer_logprob_commit" in lib.smer_last_error()
    assert lib.smer_logprob_commit(R, V, p["st"], NST, p["stage"], p["tok"], CAP, p["scr"], V - 1, p["lp"],
                                   None) == -1
    assert b"smer_logprob_commit" in lib.smer_last_error()
    assert lib.smer_abi_version() == 1


# ---------------------------------------------------------------------------
# the pair around each grammar entry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["greedy", "greedy_ring", "stream", "rows", "rows_ring"])
def test_entry_between_stage_and_commit_is_the_entry_alone(entry):
    """ban -> stage -> entry -> commit for two steps against ban -> entry:
    state rows, ids / meta, out_tok with the fail bit, all MT words and the
    live count bit for bit; out_lp at the emitted ids is token_logprobs of the
    host-banned logits under the state each step started in."""
    from smer_music_generation_amd import ops as O
    from smer_music_generation_amd.generation import ban_bits
    c = _entry_case()
    v, R, V = c["v"], c["R"], c["V"]
    keep_t, cls_t, rej_t = _t(c["keep"]), _t(c["cls"]), _t(c["rej"])
    bits = np.stack([ban_bits(c["ban"][r]) for r in range(R)]).view(np.int32)
    bom_t, bits_t, tg_t, sl_t, tp_t = _t(c["bom"]), _t(bits), _t(c["tg"]), _t(c["src_len"]), _t(c["tp"])
    gargs = dict(eos=v.eos_index, m0=v.char2index('m_0'), trash_pos=TRASH)
    use_ring = entry.endswith("_ring")
    res, want_lp = {}, []
    for scored in (True, False):
        s_t = _t(c["st"])
        out_t = torch.zeros(R, CAP, dtype=torch.int32, device=dev)
        lp_t = _t(np.full((R, CAP), NAN64).view(np.float64))
        scr_t = torch.zeros(R, 512, dtype=torch.float64, device=dev)
        stage_t = torch.full((R,), -7, dtype=torch.int32, device=dev)
        ctl = torch.zeros(3, dtype=torch.int32, device=dev)
        ring = torch.full((4,), -1, dtype=torch.int32).pin_memory() if use_ring else None
        m_t = _t((c["mt"] if entry.startswith("rows") else c["mt"][0, :625]).view(np.int32))
        steps = []
        for step in range(2):
            lg_t = _t(c["lg"])
            sh = s_t.cpu().numpy()
            O.logits_ban(lg_t, s_t, bom_t, bits_t)
            if scored:
                O.logprob_stage(lg_t, s_t, tg_t, keep_t, scr_t, stage_t)
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
            if scored:
                O.logprob_commit(s_t, stage_t, out_t, scr_t, lp_t, V=V)
            torch.cuda.synchronize()
            live = int(ring[step]) if use_ring else int(ctl[0].item())
            steps.append((ids_t.cpu().numpy(), meta_t.cpu().numpy(), live, s_t.cpu().numpy()))
            if scored:  # the expected numbers, from the state the step started in
                out = out_t.cpu().numpy()
                for r in range(R):
                    if sh[r, 5]:
                        continue
                    k = c["bom"][r, sh[r, 3]] if sh[r, 3] < 4 else -1
                    row = c["lg"][2 * r + 1].copy()
                    if k >= 0:
                        row[c["ban"][r, k]] = -100.0
                    code = _state_code(int(sh[r, 1]), int(sh[r, 2]), int(c["tg"][r, sh[r, 3]]))
                    cnt = int(sh[r, 7])
                    want_lp.append((r, cnt, _lp(row, c["keep"][code].astype(bool))[out[r, cnt] & 0xFFFF]))
        res[scored] = (steps, out_t.cpu().numpy(), m_t.cpu().numpy(), lp_t.cpu().numpy())
    a, b = res[True], res[False]
    for (ia, ma, la, sa), (ib, mb, lb, sb) in zip(a[0], b[0]):
        assert np.array_equal(ia, ib) and np.array_equal(ma, mb) and la == lb and np.array_equal(sa, sb)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[0][0][2] == 8 and a[0][1][2] == 8  # eight live requests drew on both steps
    got = a[3]
    written = np.zeros((R, CAP), dtype=bool)
    assert len(want_lp) == 16
    for r, cnt, w in want_lp:
        err = abs(got[r, cnt] - w)
        print("entry %s r=%d cnt=%d lp=%.6f err=%.3g" % (entry, r, cnt, w, err))
        assert err < TOL
        written[r, cnt] = True
    assert (got.view(np.int64)[~written] == NAN64).all()  # nothing else, the done request included
    assert min(w for _, _, w in want_lp) < -0.1


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def micro(golden_dir):
    from smer_music_generation_amd.vocab import WordVocab
    z, meta = _golden(golden_dir)
    reqs, ctl = _requests(golden_dir, 5)
    return _model(z, meta, "fp32"), WordVocab(0, CTRL), reqs, ctl


@pytest.fixture
def host_scores(monkeypatch, spans):  # noqa: F811
    """token_logprobs on the logits every sampling() call was given, kept for
    the id the span then commits: (id, value) per committed token."""
    from smer_music_generation_amd import generation as G
    rec, last = [], {}
    samp, commit = G.sampling, G._Span.commit

    def samp2(logit, vocab, p=None, t=1.0, greedy=False, rng=np.random, ban=None, **flags):
        lg = logit.squeeze().detach().cpu().numpy() if isinstance(logit, torch.Tensor) else np.asarray(logit)
        keep = G.allowed_ids(vocab, **flags)
        if ban is not None:
            keep = keep & ~np.asarray(ban, dtype=bool)
        last["lp"] = G.token_logprobs(lg.copy(), keep)
        return samp(logit, vocab, p=p, t=t, greedy=greedy, rng=rng, ban=ban, **flags)

    def commit2(self, idx):
        if "lp" in last:
            rec.append((int(idx), float(last.pop("lp")[int(idx)])))
        return commit(self, idx)
    monkeypatch.setattr(G, "sampling", samp2)
    monkeypatch.setattr(G._Span, "commit", commit2)
    return rec


def _plugin(G, m, v, reqs, ctl, spans, which=0, **kw):  # noqa: F811
    ev, tr, br = reqs[which]
    lg, stats = _Log(), {}
    res = G.generation_all(m, list(ev), dev, v, lg, ctl, tr, br, stats=stats, **kw)
    n = kw.get("variations") or 1
    recs, _ = _take(spans, n)
    return recs, lg.lines, stats, res


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.dtype == np.float64
    err = float(np.abs(a - b).max()) if a.size else 0.0
    print("logprob max err %.3g over %d tokens" % (err, a.size))
    return err < TOL


@pytest.mark.parametrize("pitches", [None, OCTAVE], ids=["free", "pitches"])
def test_seeded_plugin_call_scores_the_same_on_every_path(micro, spans, host_scores, pitches):  # noqa: F811
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    G.clear_decode_sessions(m)
    np.random.seed(3)
    st0 = _rng_state()
    kw = dict(seed=11, logprobs=True, pitches=pitches)
    plain = _plugin(G, m, v, reqs, ctl, spans, seed=11, pitches=pitches)
    assert "logprobs" not in plain[2] and "scores" not in plain[2] and "order" not in plain[2]
    del host_scores[:]
    d = _plugin(G, m, v, reqs, ctl, spans, **kw)
    assert host_scores == []  # the device path drew nothing on the host
    h = _plugin(G, m, v, reqs, ctl, spans, device_grammar=False, **kw)
    del host_scores[:]
    f = _plugin(G, m, v, reqs, ctl, spans, use_kv_cache=False, **kw)
    full = list(host_scores)
    for run in (d, h, f):  # tokens, redraw lines, steps, result: the unscored call's
        assert run[0] == plain[0] and run[1] == plain[1] and run[2]["steps"] == plain[2]["steps"]
        assert _str(run[3]) == _str(plain[3])
        lp = run[2]["logprobs"]
        assert len(lp) == 1 and lp[0].dtype == np.float64 and len(lp[0]) == run[2]["steps"] > 0
        assert run[2]["scores"] == [float(np.sum(lp[0]))] and run[2]["seeds"] == [11]
        assert (lp[0] <= 0).all() and np.isfinite(lp[0]).all()
    assert _same(_rng_state(), st0)
    assert _close(d[2]["logprobs"][0], h[2]["logprobs"][0])
    # the full-forward leg has logits of its own: against token_logprobs on those
    assert [i for i, _ in full] == [i for _, i in f[0][0]]
    assert _close(f[2]["logprobs"][0], [x for _, x in full])
    assert (d[2]["logprobs"][0] < -0.1).any()
    sess = _sessions(G, m, 1)
    mode = "rows" if pitches is None else "rows+ban"
    assert sess and set(sess[0]._graphs) == {mode, mode + "+score"}
    G.clear_decode_sessions(m)
    _plugin(G, m, v, reqs, ctl, spans, **kw)
    assert set(_sessions(G, m, 1)[0]._graphs) == {mode + "+score"}


def test_unseeded_scored_call_leaves_the_stream_where_the_unscored_one_does(micro, spans):  # noqa: F811
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    G.clear_decode_sessions(m)
    res = {}
    for name, kw in (("scored", dict(logprobs=True)), ("host", dict(logprobs=True, device_grammar=False)),
                     ("plain", dict())):
        if name == "plain":
            assert set(_sessions(G, m, 1)[0]._graphs) == {"stream+score"}
        np.random.seed(4)
        recs, lines, stats, out = _plugin(G, m, v, reqs, ctl, spans, t=0.9, p=0.95, **kw)
        res[name] = (recs, lines, stats, _rng_state())
    for name in ("scored", "host"):
        assert res[name][:2] == res["plain"][:2] and _same(res[name][3], res["plain"][3])
        assert res[name][2]["steps"] == res["plain"][2]["steps"] == len(res[name][2]["logprobs"][0])
    assert _close(res["scored"][2]["logprobs"][0], res["host"][2]["logprobs"][0])
    np.random.seed(4)
    assert not _same(_rng_state(), res["plain"][3])  # draws were taken from np.random
    assert set(_sessions(G, m, 1)[0]._graphs) == {"stream+score", "stream"}


def test_batched_greedy_scores_match_its_host_loop(micro, spans):  # noqa: F811
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    batch = [(list(e), t, b) for e, t, b in reqs[:3]]
    G.clear_decode_sessions(m)
    res = {}
    for dg in (True, False):
        lg = _Log()
        _, stats = G.generation_batch(m, batch, v, ctl, greedy=True, logger=lg, precision="fp32",
                                      device_grammar=dg, return_stats=True, logprobs=True)
        recs, _ = _take(spans, 3)
        res[dg] = (recs, lg.lines, stats)
    assert res[True][:2] == res[False][:2]
    a, b = res[True][2], res[False][2]
    assert a["tokens"] == b["tokens"] == sum(len(x) for x in a["logprobs"])
    for k in range(3):
        assert len(a["logprobs"][k]) == len(res[True][0][k]) > 0
        assert _close(a["logprobs"][k], b["logprobs"][k])
        assert a["scores"][k] == float(np.sum(a["logprobs"][k]))
    assert set(_sessions(G, m, 3)[0]._graphs) == {"greedy+score"}
    _, plain = G.generation_batch(m, batch, v, ctl, greedy=True, logger=_Log(), precision="fp32",
                                  return_stats=True)
    recs, _ = _take(spans, 3)
    assert recs == res[True][0] and "logprobs" not in plain and "scores" not in plain and "order" not in plain
    assert set(_sessions(G, m, 3)[0]._graphs) == {"greedy+score", "greedy"}


def test_unscored_calls_keep_their_graph_and_their_tokens(micro, spans):  # noqa: F811
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    G.clear_decode_sessions(m)
    before = _plugin(G, m, v, reqs, ctl, spans, seed=11)
    sess = _sessions(G, m, 1)[0]
    plain = sess._graphs["rows"]
    graph, bufs = plain.graph, dict(plain.bufs)
    assert set(sess._graphs) == {"rows"}
    assert not any(k in bufs for k in ("g_lp_row", "g_lp_stage", "g_logp"))
    a = _plugin(G, m, v, reqs, ctl, spans, seed=11, logprobs=True)
    entry = sess._graphs["rows+score"]
    assert sess._greedy is entry and {"g_lp_row", "g_lp_stage", "g_logp"} <= set(entry.bufs)
    b = _plugin(G, m, v, reqs, ctl, spans, seed=12, logprobs=True)
    assert sess._graphs["rows+score"] is entry  # another seed replays it
    assert a[0] == before[0] and b[0] != a[0]
    after = _plugin(G, m, v, reqs, ctl, spans, seed=11)
    assert _sessions(G, m, 1)[0] is sess and sess._graphs["rows"] is plain and sess._greedy is plain
    assert plain.graph is graph and set(plain.bufs) == set(bufs)
    assert all(plain.bufs[k] is bufs[k] for k in bufs)
    assert after[0] == before[0] and after[1] == before[1] and _str(after[3]) == _str(before[3])


def test_ranked_variations(micro, spans):  # noqa: F811
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    s = 16
    recs, lines, stats, out = _plugin(G, m, v, reqs, ctl, spans, variations=3, seed=s, rank=True)
    lps, scores, order = stats["logprobs"], stats["scores"], stats["order"]
    assert stats["seeds"] == [s, s + 1, s + 2] and len(lps) == len(scores) == 3 and len(out) == 3
    singles = []
    for k in range(3):
        rec, _, st1, res = _plugin(G, m, v, reqs, ctl, spans, seed=s + k, logprobs=True)
        assert rec[0] == recs[k] and len(lps[k]) == len(recs[k]) == st1["steps"]
        assert _close(lps[k], st1["logprobs"][0])
        assert scores[k] == float(np.sum(lps[k]))
        singles.append(res)
    mean = [scores[k] / len(lps[k]) for k in range(3)]
    assert order == sorted(range(3), key=lambda k: (-mean[k], k))
    assert [_str(x) for x in out] == [_str(singles[k]) for k in order]
    # not vacuous: the takes differ, in tokens and in score, and some token was a real choice
    assert len({tuple(r) for r in recs}) > 1 and len(set(scores)) > 1
    assert min(float(a.min()) for a in lps) < -0.1
    # the batched call: one order per request, the rest in take order.  (A
    # session of five slots runs other GEMM shapes than one of three: its
    # fp32 logits, hence its scores, are its own, so the ranked call is held
    # against the same call without rank.)
    batch = [(list(e), t, b) for e, t, b in reqs[:2]]
    bkw = dict(greedy=False, precision="fp32", variations=[3, 2], seed=[s, 40], return_stats=True)
    outs, bs = G.generation_batch(m, batch, v, ctl, rank=True, **bkw)
    brec, _ = _take(spans, 5)
    flat, fs = G.generation_batch(m, batch, v, ctl, logprobs=True, **bkw)
    frec, _ = _take(spans, 5)
    assert brec == frec and brec[:3] == recs and bs["seeds"] == fs["seeds"] == [s, s + 1, s + 2, 40, 41]
    assert "order" not in fs and len(bs["order"]) == 2 and len(bs["logprobs"]) == 5
    assert bs["generated"] == fs["generated"]
    k0 = 0
    for i, n in enumerate((3, 2)):
        mi = [bs["scores"][k0 + k] / len(bs["logprobs"][k0 + k]) for k in range(n)]
        assert bs["order"][i] == sorted(range(n), key=lambda k: (-mi[k], k))
        assert [_str(x) for x in outs[i]] == [_str(flat[i][k]) for k in bs["order"][i]]
        for k in range(n):
            assert len(bs["logprobs"][k0 + k]) == len(brec[k0 + k])
            assert _close(bs["logprobs"][k0 + k], fs["logprobs"][k0 + k])
        k0 += n
    # logprobs without rank: take order, no 'order'
    _, _, st2, out2 = _plugin(G, m, v, reqs, ctl, spans, variations=3, seed=s, logprobs=True)
    assert "order" not in st2 and [_str(x) for x in out2] == [_str(x) for x in singles]

"""Per-request seeds on the device decode path (csrc/decode_ops.hip
grammar_sample_kernel<.., ROWS>, smer_grammar_sample_step_rows): the rows
kernel against the serial entry run once per row, then the plugin and the
batched calls against their host loops, the global stream and each other."""
import numpy as np
import pytest
import torch

from tests.test_nucleus_gpu import (CTRL, FLAG_SETS, _golden, _Log, _model, _requests, _rng_state,
                                    _same, kernel_rows)

pytestmark = pytest.mark.gpu
dev = "cuda"
NST, CAP, TRASH = 12, 4, 200
POSITIONS = (624, 0, 623, 622)  # fresh; start of a block; one uniform straddles a twist; the next


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tables(V):
    """The SMER grammar tables, padded with kept, never-rejected, classless
    tokens up to V columns (V = 512: the widest row the sampler takes)."""
    from smer_music_generation_amd.generation import grammar_tables, reject_table
    from smer_music_generation_amd.vocab import WordVocab
    v = WordVocab(0, CTRL)
    keep, cls = grammar_tables(v, v.density_indices + v.occupation_indices)
    rej = reject_table(v)
    pad = V - v.vocab_size
    assert pad >= 0
    keep = np.concatenate([keep, np.ones((13, pad), np.uint8)], axis=1)
    rej = np.concatenate([rej, np.zeros((13, pad), np.uint8)], axis=1)
    cls = np.concatenate([cls, np.zeros(pad, np.uint8)])
    return v, np.ascontiguousarray(keep), np.ascontiguousarray(rej), cls


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# (V, R, ring, ldmt, tp): every size with and without a ring at both strides,
# and the tp = NULL form ({1.0, None} for every row) on two of them
KERNEL_CASES = [(V, R, ring, ldmt, True) for V, R in ((309, 1), (309, 2), (309, 33), (512, 5))
                for ring in (True, False) for ldmt in (625, 640)]
KERNEL_CASES += [(309, 2, True, 640, False), (309, 33, False, 625, False)]


@pytest.mark.parametrize("V,R,use_ring,ldmt,with_tp", KERNEL_CASES)
def test_rows_kernel_equals_the_serial_entry_row_by_row(V, R, use_ring, ldmt, with_tp):
    """Two steps in a row of smer_grammar_sample_step_rows over R requests,
    each on its own MT19937 stream, against smer_grammar_sample_step[_tp] with
    R = 1 on every row alone: the state rows, out_tok (fail bit included), the
    rows' ids / meta slots and all 625 words of every stream, bit for bit;
    done rows keep their stream and write nothing; the published live count
    is the number of rows still live after the step, on both steps (the
    ticket words reset)."""
    from smer_music_generation_amd import ops as O
    v, keep, rej, cls = _tables(V)
    rows, tps = kernel_rows(V, n_rows=40 + R, seed=3 + R)
    off = 7  # rows off .. off + R - 1: every (t, p) kind and flag set turns up at R = 33
    case = (R + ldmt + int(use_ring)) % 4
    st = np.zeros((R, NST), dtype=np.int32)
    tg = np.zeros((R, 2), dtype=np.int8)
    lg = np.zeros((2 * R, V), dtype=np.float32)
    tp = np.zeros((R, 2), dtype=np.float64)
    mt = np.zeros((R, ldmt), dtype=np.uint32)
    mt[:, 625:] = 0xABCD0000  # the padding words are nobody's to write
    src_len = (3 + np.arange(R) % 5).astype(np.int32)
    for r in range(R):
        f, ln, tgc = FLAG_SETS[(off + r) % len(FLAG_SETS)]
        st[r, 0] = 10 + r % 3                 # decoder position
        st[r, 1], st[r, 2] = f, ln
        st[r, 4] = 2 - r % 2                  # two masks or one: a span end is or is not the request's end
        st[r, 5] = int(r % 4 == 2 or (R == 2 and r == 0))   # done
        st[r, 7] = r % 3                      # ids emitted so far
        tg[r] = (tgc, 4)
        lg[2 * r + 1] = rows[off + r]
        t, p = tps[off + r]
        tp[r] = (t, -1.0 if p is None else p)
        s0 = np.random.RandomState(100 + r).get_state()
        mt[r, :624] = s0[1]
        assert s0[2] == 624
        mt[r, 624] = POSITIONS[(r + case) % 4]
    n_done = int(st[:, 5].sum())
    assert n_done < R and (R < 3 or n_done > 0)
    keep_t, rej_t, cls_t = _t(keep), _t(rej), _t(cls)
    gargs = dict(eos=v.eos_index, m0=v.char2index('m_0'), trash_pos=TRASH)

    # the reference: the serial entry, one launch per row and step
    ref = dict(st=st.copy(), mt=mt.copy(), out=np.zeros((R, CAP), np.int32),
               ids=np.full((2, 2 * R), -7, np.int64), meta=np.full((2, 4, 2 * R), -9, np.int32),
               live=[0, 0])
    for r in range(R):
        s_t, m_t = _t(st[r:r + 1]), _t(mt[r, :625].view(np.int32))
        out_t = torch.zeros(1, CAP, dtype=torch.int32, device=dev)
        for step in range(2):
            ids_t = torch.full((2,), -7, dtype=torch.int64, device=dev)
            meta_t = torch.full((4, 2), -9, dtype=torch.int32, device=dev)
            ctl = torch.zeros(3, dtype=torch.int32, device=dev)
            O.grammar_sample_step(_t(lg[2 * r:2 * r + 2]), s_t, _t(tg[r:r + 1]), keep_t, rej_t, cls_t,
                                  _t(src_len[r:r + 1]), ids_t, meta_t, out_t, m_t, ctl,
                                  tp=_t(tp[r:r + 1]) if with_tp else None, **gargs)
            ref["ids"][step, 2 * r:2 * r + 2] = ids_t.cpu().numpy()
            ref["meta"][step, :, 2 * r:2 * r + 2] = meta_t.cpu().numpy()
            ref["live"][step] += int(ctl[0].item())
        ref["st"][r] = s_t.cpu().numpy()[0]
        ref["out"][r] = out_t.cpu().numpy()[0]
        ref["mt"][r, :625] = m_t.cpu().numpy().view(np.uint32)
    for r in range(R):  # the serial entry left done rows alone, and their stream
        if st[r, 5]:
            assert np.array_equal(ref["st"][r], st[r]) and np.array_equal(ref["mt"][r], mt[r])
            assert (ref["ids"][:, 2 * r:2 * r + 2] == -7).all() and not ref["out"][r].any()
    # the request index column of meta: 0 in a launch of one row, r in the batch
    want_meta = ref["meta"].copy()
    for r in range(R):
        if not st[r, 5]:
            for step in range(2):
                for k in range(2):
                    if want_meta[step, 1, 2 * r + k] != -9:
                        assert want_meta[step, 1, 2 * r + k] == 0
                        want_meta[step, 1, 2 * r + k] = r

    # the rows entry: all requests in one launch, twice on the same ctl / ring
    s_t, m_t = _t(st), _t(mt.view(np.int32))
    out_t = torch.zeros(R, CAP, dtype=torch.int32, device=dev)
    ctl = torch.zeros(3, dtype=torch.int32, device=dev)
    ring = torch.full((4,), -1, dtype=torch.int32).pin_memory() if use_ring else None
    lg_t, tg_t, sl_t = _t(lg), _t(tg), _t(src_len)
    tp_t = _t(tp) if with_tp else None
    for step in range(2):
        ids_t = torch.full((2 * R,), -7, dtype=torch.int64, device=dev)
        meta_t = torch.full((4, 2 * R), -9, dtype=torch.int32, device=dev)
        O.grammar_sample_step_rows(lg_t, s_t, tg_t, keep_t, rej_t, cls_t, sl_t, ids_t, meta_t, out_t,
                                   m_t, ctl, ring=ring, tp=tp_t, **gargs)
        torch.cuda.synchronize()
        c = ctl.cpu().numpy()
        if use_ring:
            assert int(ring[step]) == ref["live"][step]
            assert c.tolist() == [0, 0, step + 1]  # count and tickets reset, the step advanced
        else:
            assert int(c[0]) == ref["live"][step]
        assert np.array_equal(ids_t.cpu().numpy(), ref["ids"][step])
        assert np.array_equal(meta_t.cpu().numpy(), want_meta[step])
    assert np.array_equal(s_t.cpu().numpy(), ref["st"])
    assert np.array_equal(out_t.cpu().numpy(), ref["out"])
    assert np.array_equal(m_t.cpu().numpy().view(np.uint32), ref["mt"])
    # the case is not vacuous: live rows drew (their streams moved) and some are still live
    moved = [not np.array_equal(ref["mt"][r], mt[r]) for r in range(R)]
    assert moved == [not bool(x) for x in st[:, 5]]
    assert ref["live"][0] > 0 and ref["live"][0] <= R - n_done


def test_rows_entry_checks_its_arguments():
    from smer_music_generation_amd import ops as O
    v, keep, rej, cls = _tables(309)
    R = 2
    args = lambda mt: (torch.zeros(2 * R, 309, device=dev),  # noqa: E731
                       torch.ones(R, NST, dtype=torch.int32, device=dev),
                       torch.zeros(R, 1, dtype=torch.int8, device=dev), _t(keep), _t(rej), _t(cls),
                       torch.ones(R, dtype=torch.int32, device=dev),
                       torch.zeros(2 * R, dtype=torch.int64, device=dev),
                       torch.zeros(4, 2 * R, dtype=torch.int32, device=dev),
                       torch.zeros(R, CAP, dtype=torch.int32, device=dev), mt,
                       torch.zeros(3, dtype=torch.int32, device=dev))
    kw = dict(eos=v.eos_index, m0=v.char2index('m_0'), trash_pos=TRASH)
    with pytest.raises(RuntimeError):  # a row of 624 words has no room for the position
        O.grammar_sample_step_rows(*args(torch.zeros(R, 624, dtype=torch.int32, device=dev)), **kw)
    with pytest.raises(RuntimeError):  # one stream per request
        O.grammar_sample_step_rows(*args(torch.zeros(625, dtype=torch.int32, device=dev)), **kw)
    from smer_music_generation_amd import _lib
    lib = _lib.load()
    assert lib.smer_grammar_sample_step_rows(R, 309, None, 309, None, NST, None, 1, None, None,
                                             None, 0, 0, TRASH, 100, None, None, None, None, CAP, None,
                                             624, None, None, 0, None, None) == -1
    assert b"ldmt" in lib.smer_last_error()


def _str(res):
    """A result with its tokens as str; None (nothing masked, or the
    reference's print-and-return-None) stays None."""
    return None if res is None else ([str(x) for x in res[0]], res[1], res[2])


def _sessions(G, m, R):
    return [s for s in G._BATCH_SESSIONS.values() if s.R == R and s.model is m]


@pytest.fixture(scope="module")
def micro(golden_dir):
    from smer_music_generation_amd.vocab import WordVocab
    z, meta = _golden(golden_dir)
    reqs, ctl = _requests(golden_dir, 3)
    return _model(z, meta, "fp32"), WordVocab(0, CTRL), reqs, ctl


def test_seeded_batch_on_device_matches_host_loop(micro):
    """generation_batch(greedy=False, seed=[..]) with one (t, p) per request:
    the rows kernel gives the host loop's outputs, redraw lines, tokens and
    steps; neither path touches np.random."""
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    G.clear_decode_sessions(m)
    np.random.seed(31)
    st0 = _rng_state()
    res = {}
    for dg in (True, False):
        lg = _Log()
        out, stats = G.generation_batch(m, [(list(e), t, b) for e, t, b in reqs], v, ctl, greedy=False,
                                        logger=lg, device_grammar=dg, t=[1.0, 0.7, 1.3],
                                        p=[None, 0.9, 0.5], seed=[5, 6, 7], precision="fp32",
                                        return_stats=True)
        res[dg] = ([_str(o) for o in out], lg.lines, stats["tokens"], stats["steps"], stats["seeds"])
        assert _same(_rng_state(), st0)
    assert res[True] == res[False]
    assert res[True][2] > 0 and res[True][4] == [5, 6, 7]
    sess = _sessions(G, m, 3)
    assert sess and "g_mt_rows" in sess[0]._graphs["rows"].bufs  # the rows kernel ran
    assert not any(k.startswith("stream") for k in sess[0]._graphs)  # and the shared-stream one did not


@pytest.mark.parametrize("tp", [dict(), dict(t=0.8, p=0.9)], ids=["default", "t0.8p0.9"])
def test_seed_is_todays_global_stream(micro, tp):
    """generation_all(..., seed=11) == np.random.seed(11); generation_all(...)
    for each of the three requests -- also where the draws of the micro model
    end in the reference's print-and-return-None (an 'm_0' drawn inside a
    span) -- and on the host paths for the first request that gives tokens."""
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    host_checked = False
    for ev, tr, br in reqs:
        np.random.seed(11)
        want = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, **tp)
        np.random.seed(4)
        st0 = _rng_state()
        stats = {}
        got = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, seed=11, stats=stats, **tp)
        assert (got is None) == (want is None)
        assert _same(_rng_state(), st0)
        assert stats["seeds"] == [11] and stats["steps"] > 0
        if want is None or host_checked:
            continue
        assert _str(got) == _str(want)
        for kw in (dict(device_grammar=False), dict(use_kv_cache=False)):  # the host paths too
            res = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, seed=11, **tp, **kw)
            assert _str(res) == _str(want)
            assert _same(_rng_state(), st0)
        host_checked = True
    assert host_checked


def test_seeded_request_does_not_depend_on_its_batch(micro, monkeypatch):
    """The three requests reordered with their seeds, and each alone through
    generation_all(seed=s): the same tokens per request (fp32).  The micro
    model's draws at these seeds put an 'm_0' inside a span of one request,
    which the final splice rejects (the reference's IndexError, raised by
    generation_batch): the comparison is on the generated tokens the splice
    is handed, recorded here, and on the spliced result where there is one."""
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    seeds = [5, 6, 7]
    splice, handed = G.restore_marked_input, []

    def recording(src, gen):
        handed.append(list(gen))
        try:
            return [str(x) for x in splice(src, gen)]
        except IndexError:
            return None
    monkeypatch.setattr(G, "restore_marked_input", recording)

    def batch(order):
        del handed[:]
        out = G.generation_batch(m, [(list(reqs[i][0]), reqs[i][1], reqs[i][2]) for i in order], v, ctl,
                                 greedy=False, seed=[seeds[i] for i in order], precision="fp32")
        assert len(handed) == 3
        return list(zip(handed[:], out))
    a = batch([0, 1, 2])
    order = [1, 2, 0]  # request i now sits at position [2, 0, 1][i]
    b = batch(order)
    for pos, i in enumerate(order):
        assert b[pos] == a[i]
    assert all(len(g) > 3 for g, _ in a) and len({tuple(g) for g, _ in a}) == 3
    for i, (ev, tr, br) in enumerate(reqs):
        del handed[:]
        res = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, seed=seeds[i])
        assert len(handed) == 1 and (handed[0], res) == a[i]


def test_seeded_variations_are_the_expanded_list(micro):
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    A, B = [(list(e), t, b) for e, t, b in reqs[:2]]
    out, stats = G.generation_batch(m, [A, B], v, ctl, greedy=False, variations=[3, 1], seed=[20, 40],
                                    precision="fp32", return_stats=True)
    flat, fstats = G.generation_batch(m, [A, A, A, B], v, ctl, greedy=False, seed=[20, 21, 22, 40],
                                      precision="fp32", return_stats=True)
    assert [[_str(o) for o in takes] for takes in out] == [[_str(o) for o in flat[:3]], [_str(flat[3])]]
    assert stats["seeds"] == [20, 21, 22, 40] and stats["sources"] == 2
    assert fstats["seeds"] == [20, 21, 22, 40] and fstats["sources"] == 4
    assert stats["generated"] == fstats["generated"]
    assert len({tuple(o[0]) for o in flat[:3]}) > 1  # the takes differ
    assert _str(G.generation_all(m, A[0], dev, v, None, ctl, A[1], A[2], seed=21)) == _str(out[0][1])
    takes = G.generation_all(m, A[0], dev, v, None, ctl, A[1], A[2], seed=20, variations=3)
    assert [_str(o) for o in takes] == [_str(o) for o in out[0]]


def test_seeded_and_unseeded_graphs_live_side_by_side(micro):
    """Warm plugin calls seeded, unseeded, seeded, unseeded with other seeds
    and (t, p): one session, one captured graph per mode, both replayed from
    the third call on; every result is its host loop's, and the unseeded
    calls leave np.random where the host loop leaves it."""
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    ev, tr, br = reqs[0]
    calls = [dict(seed=3, t=0.7, p=0.5), dict(t=1.3), dict(seed=900, p=0.999), dict(t=0.9, p=0.8)]
    host = []
    np.random.seed(8)
    for kw in calls:
        res = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, device_grammar=False, **kw)
        host.append((_str(res), _rng_state()))
    G.clear_decode_sessions(m)
    np.random.seed(8)
    seen = []
    for kw, (want, st_want) in zip(calls, host):
        res = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, **kw)
        assert _str(res) == want
        assert _same(_rng_state(), st_want)
        sess = _sessions(G, m, 1)
        assert len(sess) == 1
        mode = "rows" if "seed" in kw else "stream"
        assert sess[0]._greedy is sess[0]._graphs[mode]
        seen.append((sess[0], {k: e.graph for k, e in sess[0]._graphs.items()}))
    assert set(seen[0][1]) == {"rows"} and set(seen[1][1]) == {"rows", "stream"}
    for s, graphs in seen[2:]:
        assert s is seen[1][0]
        assert all(graphs[k] is seen[1][1][k] for k in ("rows", "stream")) and len(graphs) == 2
    assert sess[0]._graphs["stream"].bufs["g_mt"] is not None
    assert sess[0]._graphs["rows"].bufs["g_mt_rows"] is not None


def test_seed_none_spelled_out_equals_omitted(micro):
    from smer_music_generation_amd import generation as G
    m, v, reqs, ctl = micro
    res = {}
    for kw in ({}, dict(seed=None)):
        G.clear_decode_sessions(m)
        np.random.seed(19)
        outs = []
        for ev, tr, br in reqs[:2]:
            outs.append(_str(G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, **kw)))
        b, stats = G.generation_batch(m, [(list(e), t, q) for e, t, q in reqs], v, ctl, greedy=False,
                                      return_stats=True, **kw)
        outs.append([_str(o) for o in b])
        assert stats["seeds"] is None
        res[bool(kw)] = (outs, _rng_state())
        sess = _sessions(G, m, 3)  # the shared-stream sampler, as before
        assert sess and sess[0]._graphs["stream"].bufs["g_mt"] is not None
        assert not any(k.startswith("rows") for k in sess[0]._graphs)
        assert "g_mt_rows" not in sess[0]._graphs["stream"].bufs
    assert res[True][0] == res[False][0]
    assert _same(res[True][1], res[False][1])


def test_grammar_graphs_are_recaptured_after_the_positional_table_moved(micro):
    """A second session whose capacity exceeds the model's positional table
    reallocates it (pos_enc.extend), and the warm session's captured step +
    grammar graphs address the freed one.  The next calls run on the same
    warm session with newly captured graphs and return what they returned
    before: tokens equal, log-probabilities bit for bit."""
    from smer_music_generation_amd import generation as G
    from smer_music_generation_amd.decode import DecodeSession
    m, v, reqs, ctl = micro
    G.clear_decode_sessions(m)

    def calls():
        res = []
        for kw in (dict(greedy=True), dict(greedy=False, seed=[5, 6, 7], t=[1.0, 0.7, 1.3], p=[None, 0.9, 0.5])):
            out, st = G.generation_batch(m, [(list(e), t, b) for e, t, b in reqs], v, ctl, precision="fp32",
                                         logprobs=True, return_stats=True, **kw)
            res.append(([_str(o) for o in out], st["generated"], st["steps"],
                        [a.tobytes() for a in st["logprobs"]]))
        (sess,) = _sessions(G, m, 3)
        return res, sess, {k: e.graph for k, e in sess._graphs.items()}
    calls()
    want, sess, graphs = calls()  # warm: the session and both graphs of the first round
    assert set(graphs) == {"greedy+score", "rows+score"}
    assert all(sum(len(g) for g in r[1]) > 0 and r[2] > 0 for r in want)
    pe = m.pos_enc.pe
    old_ptr, rows = pe.data_ptr(), pe.shape[0]
    other = DecodeSession(m, 1, rows + 8, 8)  # extends the table
    assert m.pos_enc.pe.data_ptr() != old_ptr and m.pos_enc.pe.shape[0] >= rows + 8
    del pe
    junk = [torch.full((rows, 1, m.pos_enc.pe.shape[2]), 1e4, device=dev) for _ in range(8)]
    got, sess2, graphs2 = calls()
    del junk, other
    assert sess2 is sess and set(graphs2) == set(graphs)
    assert all(graphs2[k] is not graphs[k] for k in graphs)
    assert sess._greedy is sess._graphs["rows+score"]
    assert got == want

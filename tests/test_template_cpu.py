"""`template=` on the host: the public calls validate it before the model or
np.random is touched; a templated draw is `sampling()` of a row edited by
hand; a template made of a take's own tokens reproduces the take on every
host path and scores what `score_infill` scores; `rhythm_template` keeps the
rhythm and `opening_template` the opening; the host paths agree token for
token.  The model is a stand-in whose logits depend on the decoder row alone,
so every path (the KV-cached single request, the batched host loop,
use_kv_cache=False, the full forward of score_infill) reads the same rows."""
import types

import numpy as np
import pytest
import torch

from smer_music_generation_amd import generation as G
from smer_music_generation_amd.generation import ANY_PITCH, opening_template, rhythm_template
from smer_music_generation_amd.synth import synth_events
from smer_music_generation_amd.vocab import WordVocab
from tests.test_nucleus_gpu import FLAG_SETS, _state_code, kernel_rows

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']
TRACKS, BARS = [0, 2], [2]  # masks: r d o p of track 0, then r d o p t of track 2 (the last track)
N_MASKS = 9


class _Sentinel:
    """Stands in for the model: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the model was touched (%s)" % name)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _vocab():
    v = WordVocab(0, CTRL)
    return v, v.density_indices + v.occupation_indices + v.polyphony_indices + v.tensile_indices


def _events():
    return list(synth_events(61, n_bars=7, n_tracks=3))


# --------------------------------------------------------------------------
# validation
# --------------------------------------------------------------------------
def _row0(row):
    """A template whose first note span (mask 0) has `row`."""
    return [row] + [None] * (N_MASKS - 1)


def _bad_templates(v):
    dens, occ = v.index2char(v.density_indices[0]), v.index2char(v.occupation_indices[0])
    return {
        "too few rows": [None] * (N_MASKS - 1),
        "too many rows": [None] * (N_MASKS + 1),
        "not a list": 7,
        "a string": "p_60",
        "row is a string": _row0("p_60"),
        "control row empty": [None, [], None, None, None, None, None, None, None],
        "control row of two": [None, [dens, dens]] + [None] * 7,
        "control row of another class": [None, [occ]] + [None] * 7,
        "control row holds a pitch": [None, ['p_60']] + [None] * 7,
        "control row any pitch": [None, [ANY_PITCH]] + [None] * 7,
        "control row eos": [None, ['<eos>']] + [None] * 7,
        "duration first (outside keep)": _row0(['quarter']),
        "eos after a pitch (outside keep)": _row0(['p_60', '<eos>']),
        "control after a pitch (redraw check)": _row0(['p_60', dens]),
        "any pitch after rest": _row0(['rest', ANY_PITCH]),
        "m_0": _row0(['p_60', 'm_0']),
        "unknown token": _row0(['p_60', 'no_such_token']),
        "id past the vocabulary": _row0([v.vocab_size]),
        "negative id": _row0([-2]),
        "a bool": _row0([True]),
        "a float": _row0([60.0]),
        "eos first of two": _row0(['<eos>', 'p_60']),
        "items after a control token": _row0([dens, 'p_60']),
        "99 body items": _row0(['p_60', 'eighth'] * 49 + ['p_60']),
        "98 body items, then a token": _row0(['p_60', 'eighth'] * 49 + ['p_62']),
    }


BAD = list(_bad_templates(WordVocab(0, CTRL)))


@pytest.mark.parametrize("name", BAD)
def test_bad_templates_raise_before_anything_is_touched(name):
    v, ctl = _vocab()
    bad = _bad_templates(v)[name]
    ev = _events()
    np.random.seed(5)
    st0 = np.random.get_state()
    for fn in (G.generation_all, G.infill):
        for kw in (dict(), dict(greedy=True), dict(seed=3), dict(variations=2), dict(use_kv_cache=False),
                   dict(logprobs=True)):
            with pytest.raises(ValueError):
                fn(_Sentinel(), list(ev), "cpu", v, None, ctl, TRACKS, BARS, template=bad, **kw)
    for kw in (dict(greedy=False), dict(greedy=True), dict(greedy=False, seed=[1, 2]),
               dict(greedy=False, variations=2)):
        with pytest.raises(ValueError):
            G.generation_batch(_Sentinel(), [(list(ev), TRACKS, BARS)] * 2, v, ctl, template=[None, bad], **kw)
    assert _same_state(np.random.get_state(), st0)


def test_batch_takes_one_template_per_request():
    v, ctl = _vocab()
    ev = _events()
    good = [None] * N_MASKS
    for bad in (good, [good], [good] * 3, "x", 5):  # one template is not a list of two
        with pytest.raises(ValueError):
            G.generation_batch(_Sentinel(), [(list(ev), TRACKS, BARS)] * 2, v, ctl, template=bad)


def test_check_template_normalises_and_knows_the_pitch_ban():
    v, ctl = _vocab()
    ev = _events()
    src, _, _, target, no_whole = G._prepare(list(ev), v, TRACKS, BARS)
    C = lambda t, bans=None: G._check_template(t, v, src, target, ctl, no_whole, bans)  # noqa: E731
    assert C(None) is None
    p60, eighth, dens = v.char2index('p_60'), v.char2index('eighth'), v.density_indices[2]
    rows = C([['p_60', eighth, ANY_PITCH, np.int64(eighth), '<eos>'], [dens], None, None, (), None, None, None,
              None])
    assert rows == [(p60, eighth, -2, eighth, v.eos_index), (dens,), None, None, (), None, None, None, None]
    assert all(type(x) is int for x in rows[0])
    long_row = ['p_60', 'eighth'] * 49
    assert len(C(_row0(long_row))[0]) == 98 and len(C(_row0(long_row + ['<eos>']))[0]) == 99
    # pitches=: a token item outside the track's set, and ANY_PITCH where the set leaves nothing
    bans = G._request_bans(v, ev, TRACKS, BARS, G._check_pitches({0: [62]}, TRACKS))
    assert C(_row0(['p_62', 'eighth', ANY_PITCH]), bans)[0] == (v.char2index('p_62'), eighth, -2)
    assert C([None] * 4 + [['p_60']] + [None] * 4, bans)[4] == (p60,)  # track 2 is unconstrained
    with pytest.raises(ValueError):
        C(_row0(['p_60']), bans)
    none_left = (bans[0], np.zeros_like(bans[1]))
    none_left[1][0, v.pitch_indices] = True
    with pytest.raises(ValueError):
        C(_row0([ANY_PITCH]), none_left)
    with pytest.raises(ValueError):
        C(_row0(['rest', 'eighth', ANY_PITCH]), none_left)


# --------------------------------------------------------------------------
# the definition: a templated draw is sampling() of a row edited by hand
# --------------------------------------------------------------------------
KINDS = [("greedy", dict(greedy=True)), ("t1", dict(t=1.0, p=None)), ("t0.8 p0.9", dict(t=0.8, p=0.9))]


@pytest.mark.parametrize("kind", [k for k, _ in KINDS])
def test_templated_draw_equals_sampling_of_hand_edited_logits(kind):
    """Every grammar state of FLAG_SETS: a token item (the state's least
    likely kept token, and one whose own logit is below -100) and ANY_PITCH
    (where the state keeps a pitch) against sampling() of the row edited with
    np.where, on the same seeded stream: the same index, the same stream
    afterwards."""
    v, _ = _vocab()
    kw = dict(KINDS)[kind]
    rows, _ = kernel_rows(v.vocab_size)
    V, pitch = v.vocab_size, G._pitch_mask(v)
    n = n_any = 0
    for fi, (f, ln, tg) in enumerate(FLAG_SETS):
        flags, check, _ = G.grammar_spec(v, _state_code(f, ln, tg))
        keep = G.allowed_ids(v, **flags)
        ok = [i for i in np.flatnonzero(keep) if check is None or not check(int(i))]
        row = rows[(7 * fi) % len(rows)].copy()
        tok = int(ok[int(np.argmin(row[ok]))])
        low = row.copy()
        low[tok] = np.float32(-250.0)
        cases = [(row, tok, np.where(np.arange(V) == tok, np.float32(0.0), np.float32(-100.0))),
                 (low, tok, np.where(np.arange(V) == tok, np.float32(0.0), np.float32(-100.0)))]
        if (keep & pitch).any():
            top = row.copy()
            top[np.flatnonzero(keep & ~pitch)[0]] = row.max() + np.float32(6.0)  # the maximum is no pitch
            cases.append((top, ANY_PITCH, np.where(pitch, top, np.float32(-100.0))))
            n_any += 1
        for lg, item, edited in cases:
            res = []
            for r, extra in ((lg, dict(force=item)), (edited, dict())):
                np.random.seed(300 + n)
                idx = G.sampling(r.copy(), v, rng=np.random, **kw, **extra, **flags)
                res.append((int(idx), np.random.get_state()))
            assert res[0][0] == res[1][0] and _same_state(res[0][1], res[1][1]), (f, ln, tg, item)
            assert res[0][0] == tok if item is not ANY_PITCH else pitch[res[0][0]]
            n += 1
    assert n_any >= 3 and n > 2 * len(FLAG_SETS)


# --------------------------------------------------------------------------
# a stand-in model: logits by decoder row
# --------------------------------------------------------------------------
def _table(v, ctl):
    """Logits rows indexed by decoder row (prefix length - 1): control tokens
    and m_0 out of reach inside note spans, pitches and durations ahead of the
    rest (so that no state's redraw check runs out, greedy included), <eos>
    the winner of every seventh row, so note spans end on a drawn <eos> after a
    handful of tokens."""
    rows = (np.random.default_rng(9).standard_normal((1200, v.vocab_size)) * 2.0).astype(np.float32)
    rows[:, ctl] -= np.float32(25.0)
    rows[:, v.pitch_indices] += np.float32(8.0)
    rows[:, v.duration_only_indices] += np.float32(10.0)  # (few against 88 pitches: or a span is all pitches)
    rows[:, v.mask_indices] = np.float32(-40.0)
    rows[:, v.eos_index] = np.float32(-40.0)
    rows[4::7, v.eos_index] = np.float32(30.0)
    return rows


class _Session:
    """The part of a DecodeSession the host loops use."""
    Tmax, prefill_rows, phase_s = 1201, 0, {}

    def __init__(self, rows):
        self.rows = rows

    def prefill(self, slots, srcs):
        pass

    def prefill_takes(self, srcs, takes):
        pass

    def step(self, feeds):
        return np.stack([self.rows[p0 + len(toks) - 1] for _, toks, p0 in feeds])


class _Model:
    """forward() gives row j of the table at decoder position j, whatever the
    source: the rows the session above serves."""
    precision, need_weights = "fp32", False

    def __init__(self, rows):
        self.rows = torch.from_numpy(rows)
        self.embedding = types.SimpleNamespace(weight=torch.zeros(1))

    def eval(self):
        return self

    def set_precision(self, p):
        self.precision = p

    def forward(self, src, tgt, **kw):
        return self.rows[:tgt.shape[1]].unsqueeze(0).repeat(tgt.shape[0], 1, 1), None


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


@pytest.fixture
def host(monkeypatch):
    """(model, vocab, controls, events, made): the stand-in model behind every
    host path, and every _Span made during the test with `rec`, its committed
    (mask index, id) pairs."""
    v, ctl = _vocab()
    rows = _table(v, ctl)
    made = []
    init, commit = G._Span.__init__, G._Span.commit

    def init2(self, *a, **k):
        init(self, *a, **k)
        self.rec = []
        made.append(self)

    def commit2(self, idx):
        self.rec.append((self.mask_idx, int(idx)))
        return commit(self, idx)
    monkeypatch.setattr(G._Span, "__init__", init2)
    monkeypatch.setattr(G._Span, "commit", commit2)
    monkeypatch.setattr(G, "_batch_session", lambda *a, **k: _Session(rows))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    return _Model(rows), v, ctl, _events(), made


def _last(made, n=1):
    out = [list(sp.rec) for sp in made[-n:]]
    del made[:]
    return out


PATHS = ["single", "no_kv_cache", "batch"]


def _run(host, path, *, n=1, **kw):
    """One call on a host path.  Returns per request (rec, log lines are
    shared), and the stats."""
    m, v, ctl, ev, made = host
    lg, stats = _Log(), {}
    if path == "batch":
        for key in ("seed", "template", "pitches"):
            if key in kw and kw[key] is not None:
                kw[key] = [kw[key]] * n
        out, stats = G.generation_batch(m, [(list(ev), TRACKS, BARS)] * n, v, ctl, logger=lg, precision="fp32",
                                        device_grammar=False, return_stats=True,
                                        **{"greedy": False, **kw})
        assert all(o is not None for o in out)
    else:
        assert n == 1
        res = G.generation_all(m, list(ev), "cpu", v, lg, ctl, TRACKS, BARS, stats=stats,
                               use_kv_cache=path != "no_kv_cache", device_grammar=False, **kw)
        assert res is not None
    return _last(made, n), lg.lines, stats


def _rows_of(rec):
    """The whole-span template of a take: per mask its drawn ids, the <eos>
    that ended a note span included."""
    rows = [[] for _ in range(N_MASKS)]
    for k, i in rec:
        rows[k].append(i)
    return rows


@pytest.mark.parametrize("kw", [dict(greedy=True), dict(seed=12), dict(seed=5, t=0.8, p=0.9)],
                         ids=["greedy", "t1", "t0.8 p0.9"])
def test_a_take_forced_back_whole_reproduces_itself_and_its_scores(host, kw):
    """The take of an untemplated call, forced back token for token (<eos>
    included) on every host path, under another seed: the same tokens; and
    its logprobs are score_infill's of the take to 1e-12 (both are
    token_logprobs of the same rows: the score is taken before the template
    is applied -- from the row after it every entry would be ~0)."""
    m, v, ctl, ev, made = host
    (take,), lines, _ = _run(host, "single", **kw)
    assert not lines and len(take) > 12  # no redraw ran out: every token passes its state's check
    tpl = _rows_of(take)
    assert all(len(r) >= 1 for r in tpl) and all(len(r) < 99 for r in tpl)
    assert all(tpl[k][-1] == v.eos_index for k in (0, 4)) and any(len(tpl[k]) > 3 for k in (0, 4))
    other = dict(kw, seed=kw["seed"] + 100) if "seed" in kw else kw
    content = [[i for i in r if i != v.eos_index] for r in tpl]
    want = G.score_infill(m, list(ev), "cpu", v, ctl, TRACKS, BARS, content=content, device_score=False)
    assert want.tokens.tolist() == [i for _, i in take]
    for path in PATHS:
        (rec,), lines, stats = _run(host, path, template=tpl, logprobs=True, **other)
        assert rec == take and not lines, path
        got = np.asarray(stats["logprobs"][0])
        assert got.shape == want.logprobs.shape
        err = float(np.abs(got - want.logprobs).max())
        print("%s: %d entries, max |dlogprob| %.3g" % (path, len(got), err))
        assert err <= 1e-12
        assert got.min() < -1.0  # the model's own numbers, not the forced row's


def test_whole_span_template_consumes_the_stream_like_any_other_step(host):
    """Unseeded: the forced run draws from np.random once per step (no redraw
    here), as the free run does."""
    m, v, ctl, ev, made = host
    np.random.seed(21)
    (take,), _, _ = _run(host, "single")
    after_free = np.random.get_state()
    np.random.seed(21)
    (rec,), _, _ = _run(host, "single", template=_rows_of(take))
    assert rec == take and _same_state(np.random.get_state(), after_free)
    np.random.seed(21)
    assert not _same_state(np.random.get_state(), after_free)


# --------------------------------------------------------------------------
# the builders
# --------------------------------------------------------------------------
def _source_bodies(v, ev):
    src, _, _, target, _ = G._prepare(list(ev), v, TRACKS, BARS)
    bodies, codes = G._template_bodies(ev, v, TRACKS, BARS, None)
    assert codes == [G._target_code(t) for t in target] and len(bodies) == N_MASKS
    return bodies, codes


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pitches", [None, tuple(range(60, 72))], ids=["free", "octave"])
def test_rhythm_template_keeps_the_rhythm(host, path, pitches):
    m, v, ctl, ev, made = host
    bodies, codes = _source_bodies(v, ev)
    tpl = rhythm_template(ev, v, TRACKS, BARS)
    pitch = G._pitch_mask(v)
    for body, code, row in zip(bodies, codes, tpl):
        if code:
            assert row is None
        else:
            assert len(row) == len(body) + 1 and row[-1] == v.eos_index
            assert [x for x in row[:-1] if x is not ANY_PITCH] == [x for x in body if not pitch[x]]
            assert sum(1 for x in row if x is ANY_PITCH) == int(pitch[body].sum()) > 0
    (rec,), lines, _ = _run(host, path, template=tpl, seed=4, pitches=pitches)
    got = _rows_of(rec)
    ok = {v.char2index('p_%d' % n) for n in (pitches or range(21, 109))}
    changed = 0
    for k in (0, 4):  # the note spans: the source's length, its non-pitch tokens in place, pitches of the model's
        assert len(got[k]) == len(bodies[k]) + 1 and got[k][-1] == v.eos_index
        for a, b in zip(got[k], bodies[k]):
            assert pitch[a] == pitch[b] and (pitch[a] or a == b)
            assert not pitch[a] or a in ok
            changed += int(a != b)
    assert changed > 0 and not lines
    assert all(len(got[k]) == 1 for k in range(N_MASKS) if codes[k])  # control spans: drawn freely
    # the same rows from explicit content
    assert rhythm_template(ev, v, TRACKS, BARS, content=bodies) == tpl


def test_opening_template_keeps_the_opening(host):
    m, v, ctl, ev, made = host
    bodies, codes = _source_bodies(v, ev)
    tpl = opening_template(ev, v, TRACKS, BARS, keep=3)
    assert [None if r is None else list(r) for r in tpl] == \
        [None if c else b[:3] for b, c in zip(bodies, codes)]
    assert opening_template(ev, v, TRACKS, BARS, keep=[1, 0])[0] == bodies[0][:1]
    assert opening_template(ev, v, TRACKS, BARS, keep=[1, 0])[4] == []
    for bad in (-1, 99, True, 2.0, [1], [1, 2, 3]):
        with pytest.raises(ValueError):
            opening_template(ev, v, TRACKS, BARS, keep=bad)
    takes = []
    for seed in (1, 2, 3):
        (rec,), _, _ = _run(host, "single", template=tpl, seed=seed)
        got = _rows_of(rec)
        assert got[0][:3] == bodies[0][:3] and got[4][:3] == bodies[4][:3]
        takes.append(rec)
    assert len({tuple(t) for t in takes}) > 1  # after the opening the model draws freely


@pytest.mark.parametrize("path", PATHS)
def test_an_empty_template_is_the_unconstrained_call(host, path):
    """keep=0, an all-None template and template=None: the same tokens, log
    lines and final np.random state (unseeded)."""
    m, v, ctl, ev, made = host
    res = []
    for tpl in (None, opening_template(ev, v, TRACKS, BARS, keep=0), [None] * N_MASKS):
        np.random.seed(8)
        recs, lines, _ = _run(host, path, n=2 if path == "batch" else 1, template=tpl, t=1.3)
        res.append((recs, lines, np.random.get_state()))
    for r in res[1:]:
        assert r[0] == res[0][0] and r[1] == res[0][1] and _same_state(r[2], res[0][2])


@pytest.mark.parametrize("kw", [dict(greedy=True), dict(seed=9), dict(seed=9, t=0.8, p=0.9)],
                         ids=["greedy", "t1", "t0.8 p0.9"])
def test_host_paths_agree_under_a_template(host, kw):
    """The single request, use_kv_cache=False and the batched host loop (two
    requests: the template and none), token for token; the untemplated
    batch-mate draws what it draws alone."""
    m, v, ctl, ev, made = host
    tpl = rhythm_template(ev, v, TRACKS, BARS)
    tpl[0] = tpl[0][:5]  # an opening only: the rest of the span is the model's
    runs = [_run(host, path, template=tpl, **kw)[0][0] for path in ("single", "no_kv_cache")]
    assert runs[0] == runs[1]
    (free,), _, _ = _run(host, "single", **kw)
    assert free != runs[0]
    lg = _Log()
    bkw = dict(kw, seed=[kw["seed"]] * 2) if "seed" in kw else kw
    G.generation_batch(m, [(list(ev), TRACKS, BARS)] * 2, v, ctl, logger=lg, precision="fp32",
                       device_grammar=False, template=[tpl, None], **{"greedy": False, **bkw})
    a, b = _last(made, 2)
    assert a == runs[0] and b == free


def test_variations_share_the_template(host):
    m, v, ctl, ev, made = host
    tpl = opening_template(ev, v, TRACKS, BARS, keep=2)
    out = G.generation_all(m, list(ev), "cpu", v, None, ctl, TRACKS, BARS, variations=3, seed=30, template=tpl,
                           device_grammar=False)
    assert len(out) == 3
    takes = _last(made, 3)
    bodies, _ = _source_bodies(v, ev)
    for rec in takes:
        got = _rows_of(rec)
        assert got[0][:2] == bodies[0][:2] and got[4][:2] == bodies[4][:2]
    assert len({tuple(t) for t in takes}) > 1

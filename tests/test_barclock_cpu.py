"""`fill_bar=` on the host: the bar clock (`_BarClock`, the cursor rule of
codec._Writer in integer sixteenths) finds every source bar of the committed
fixtures exactly full and the infilled ones not; no reachable state of the
grammar and the clock together is a dead end; every host path draws the same
tokens under it, every note span stays inside its bar and every span that
ended on a token fills it; the scores, the batch-mates without the keyword and
the validation are what the call documents.  The model is the stand-in of
tests/test_template_cpu.py (logits by decoder row)."""
import json
import os
import re
from collections import deque

import numpy as np
import pytest

from smer_music_generation_amd import generation as G
from smer_music_generation_amd.generation import ANY_PITCH, _BarClock, bar_fill, bar_units
from tests.test_template_cpu import (BARS, N_MASKS, PATHS, TRACKS, _events, _last, _rows_of, _run, _same_state,
                                     _Sentinel, _vocab, host)  # noqa: F401  (host: a fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOTE_MASKS = (0, 4)  # the 'r' spans among the nine masks of TRACKS x BARS


# --------------------------------------------------------------------------
# the fixtures: every source bar is exactly full, the infilled ones are not
# --------------------------------------------------------------------------
def _track_bars(events):
    """The tokens of every track of every bar."""
    events, out, cur = list(events), [], None
    for e in events[events.index('bar'):]:
        if e == 'bar':
            cur = None
        elif re.fullmatch(r'track_\d+', e):
            cur = []
            out.append(cur)
        elif cur is not None:
            cur.append(e)
    return out


def _fill_counts(v, events):
    """(exact, under, over) track-bars of `events`, and the peak end."""
    L, n, peak = bar_units(events), [0, 0, 0], 0
    for tb in _track_bars(events):
        cursor, pk = bar_fill(v, tb)
        n[0 if cursor == L else 1 if cursor < L else 2] += 1
        peak = max(peak, pk)
    return n, peak, L


# fixture -> (source track-bars, all exact), (restored: exact, under, over)
TABLE = {"infill_c2.json": (108, (104, 4, 0)), "infill_micro.json": (58, (49, 8, 1)),
         "infill_c2_sampled.json": (648, (625, 19, 4)), "mask_bar_and_track.json": (17, None)}


@pytest.mark.parametrize("name", list(TABLE))
def test_fixture_sources_fill_their_bars_and_the_infilled_bars_do_not(name):
    v, _ = _vocab()
    with open(os.path.join(GOLDEN, name)) as f:
        d = json.load(f)
    cases = d["cases"] if isinstance(d, dict) else d
    src, res = [0, 0, 0], [0, 0, 0]
    for c in cases:
        n, peak, L = _fill_counts(v, c["events"])
        assert L == 16 and peak <= L  # no group ever crosses the bar line
        src = [a + b for a, b in zip(src, n)]
        if "restored" in c:
            res = [a + b for a, b in zip(res, _fill_counts(v, c["restored"])[0])]
    want_src, want_res = TABLE[name]
    assert src == [want_src, 0, 0]
    assert tuple(res) == (want_res or (0, 0, 0))


def test_bar_units_and_bar_fill():
    v, _ = _vocab()
    assert bar_units(['4/4']) == 16 and bar_units(['3/4']) == 12 and bar_units(['6/8']) == 12
    assert bar_units(['2/4']) == 8
    # groups sum, sep rewinds by the previous group, a trailing sep rewinds nothing
    assert bar_fill(v, ['p_60', 'quarter', 'eighth', 'p_62', 'half']) == (14, 14)
    assert bar_fill(v, ['p_60', 'quarter', 'sep', 'p_64', 'half', 'rest', 'half']) == (16, 16)
    assert bar_fill(v, ['p_60', 'whole', 'sep']) == (16, 16)
    assert bar_fill(v, [v.char2index('rest'), v.char2index('whole'), v.char2index('sixteenth')]) == (17, 17)
    assert bar_fill(v, []) == (0, 0)


# --------------------------------------------------------------------------
# no dead end: breadth-first search over grammar flags x clock
# --------------------------------------------------------------------------
def _flags_after(fl, kind):
    """_Span.commit's flag updates: fl = (sep, continue, pitch, rest)."""
    s, c, p, r = fl
    if kind == 'continue':
        c, s = True, False
    if kind == 'pitch':
        p, s, c = True, False, False
    if kind == 'dur':
        r, p = False, False
    if kind == 'sep':
        s = True
    if kind == 'rest':
        r = True
    return (s, c, p, r)


def _code(fl, first, nw):
    s, c, p, r = fl
    return 0 if s else 1 if c else 2 + nw if p else 4 + nw if r else 10 if first else 11 + nw


@pytest.mark.parametrize("one_pitch", [False, True], ids=["all pitches", "one pitch"])
@pytest.mark.parametrize("no_whole", [0, 1])
@pytest.mark.parametrize("L", [12, 16])
def test_no_reachable_state_is_a_dead_end(L, no_whole, one_pitch):
    """Tokens collapsed to their classes and unit values (one representative
    each): from the start of a note span, over every token the grammar mask,
    the pitch ban and the clock allow, every reachable (grammar flags, span
    start or not, T, P, A, G, S) keeps a candidate that also passes the
    state's redraw check; end <= L everywhere; <eos> is allowed only at end ==
    L."""
    v, ctl = _vocab()
    cls, units = G.grammar_tables(v, ctl)[1], G.unit_table(v)
    reps = {v.char2index('p_60'): 'pitch', v.continue_index: 'continue', v.char2index('rest'): 'rest',
            v.char2index('sep'): 'sep', v.eos_index: 'end', ctl[0]: 'end', v.char2index('k_3'): 'other',
            v.pad_index: 'other'}
    reps.update({i: 'dur' for i in v.duration_only_indices})
    pban = np.zeros(v.vocab_size, dtype=bool)
    if one_pitch:
        pban[v.pitch_indices] = True
        pban[v.char2index('p_60')] = False
    start = ((False,) * 4, True, 0, 0, 0, 0, 0)
    seen, todo, n_eos = {start}, deque([start]), 0
    while todo:
        fl, first, T, P, A, Gp, S = todo.popleft()
        ck = _BarClock(L, cls, units)
        ck.T, ck.P, ck.A, ck.G, ck.S = T, P, A, Gp, S
        assert 0 <= ck.end <= L and 0 <= ck.T <= L
        flags, check, _ = G.grammar_spec(v, _code(fl, first, no_whole))
        ok = G.allowed_ids(v, **flags) & ~pban & ~ck.banned(v)
        assert any(check is None or not check(int(i)) for i in np.flatnonzero(ok)), (fl, first, T, P, A, Gp, S)
        if ok[v.eos_index]:
            assert ck.end == L
            n_eos += 1
        for i, kind in reps.items():
            if not ok[i] or kind == 'end':
                continue
            nk = _BarClock(L, cls, units)
            nk.T, nk.P, nk.A, nk.G, nk.S = T, P, A, Gp, S
            nk.advance(int(cls[i]), int(units[i]))
            nxt = (_flags_after(fl, kind), False, nk.T, nk.P, nk.A, nk.G, nk.S)
            if nxt not in seen:
                seen.add(nxt)
                todo.append(nxt)
    print("L %d no_whole %d: %d states, %d allow <eos>" % (L, no_whole, len(seen), n_eos))
    assert len(seen) > 200 and n_eos > 0


# --------------------------------------------------------------------------
# the host paths under fill_bar (stand-in model)
# --------------------------------------------------------------------------
MODES = [("greedy", dict(greedy=True), None), ("seeded", dict(seed=12), None),
         ("seeded t0.8 p0.9", dict(seed=5, t=0.8, p=0.9), None), ("shared stream", dict(), 31)]


def _check_spans(v, rec, fill, L=16):
    """The span assertions: every note span has cursor <= L, every one that
    ended on a token cursor == L; `fill` is what stats['bar_fill'] reported.
    Returns how many spans ended on a token."""
    ctrl = set(v.density_indices + v.occupation_indices + v.polyphony_indices + v.tensile_indices)
    rows, ended = _rows_of(rec), 0
    assert len(fill) == len(NOTE_MASKS)
    for k, (cursor, bar) in zip(NOTE_MASKS, fill):
        body = rows[k]
        on_token = body[-1] == v.eos_index or body[-1] in ctrl
        kept = body if on_token else body[:-1]  # the cap drops the last draw
        assert (cursor, bar) == (bar_fill(v, [i for i in kept if i != v.eos_index])[0], L)
        assert bar_fill(v, kept)[1] <= L and cursor <= L
        if on_token:
            assert cursor == L
            ended += 1
        else:
            assert len(body) == 99
    return ended


@pytest.mark.parametrize("pitches", [None, tuple(range(60, 72))], ids=["free", "octave"])
@pytest.mark.parametrize("mode", [m[0] for m in MODES])
def test_host_paths_agree_under_fill_bar(host, mode, pitches):  # noqa: F811
    m, v, ctl, ev, made = host
    kw, unseeded = {k: (a, b) for k, a, b in MODES}[mode]
    runs = []
    for path in PATHS:
        if unseeded is not None:
            np.random.seed(unseeded)
        (rec,), _, stats = _run(host, path, fill_bar=True, pitches=pitches, **kw)
        runs.append((rec, np.random.get_state() if unseeded is not None else None))
        fill = stats["bar_fill"][0]
        ended = _check_spans(v, rec, fill)
        assert ended >= 1, "no span of this mode ended on a token"
        if pitches is not None:
            ok = {v.char2index('p_%d' % n) for n in pitches}
            assert all(i in ok for _, i in rec if G._pitch_mask(v)[i])
    assert runs[0][0] == runs[1][0] == runs[2][0]
    if unseeded is not None:
        assert all(_same_state(r[1], runs[0][1]) for r in runs)
    if unseeded is not None:
        np.random.seed(unseeded)
    (plain,), _, st = _run(host, "single", pitches=pitches, **kw)
    assert plain != runs[0][0] and "bar_fill" not in st  # the clock changed the take


@pytest.mark.parametrize("kw", [dict(greedy=True), dict(greedy=False, seed=[7, 8, 9])], ids=["greedy", "seeded"])
def test_a_batch_mate_without_fill_bar_draws_the_plain_tokens(host, kw):  # noqa: F811
    m, v, ctl, ev, made = host
    reqs = [(list(ev), TRACKS, BARS)] * 3
    common = dict(logger=None, precision="fp32", device_grammar=False, return_stats=True)
    _, st = G.generation_batch(m, reqs, v, ctl, **common, **kw)
    plain = _last(made, 3)
    assert "bar_fill" not in st
    _, st = G.generation_batch(m, reqs, v, ctl, fill_bar=[True, False, True], **common, **kw)
    mixed = _last(made, 3)
    assert mixed[1] == plain[1] and mixed[0] != plain[0] and mixed[2] != plain[2]
    assert st["bar_fill"][1] is None
    for k in (0, 2):
        _check_spans(v, mixed[k], st["bar_fill"][k])
    _, st = G.generation_batch(m, reqs, v, ctl, fill_bar=False, **common, **kw)
    assert _last(made, 3) == plain and "bar_fill" not in st


@pytest.mark.parametrize("path", PATHS)
def test_logprobs_under_fill_bar_are_score_infill_of_the_take(host, path):  # noqa: F811
    """The score is taken from the unclocked keep: the model, the grammar
    mask and the pitch ban, the number score_infill gives for the take."""
    m, v, ctl, ev, made = host
    pitches = tuple(range(55, 80))
    (rec,), _, stats = _run(host, path, fill_bar=True, logprobs=True, seed=12, pitches=pitches)
    rows = _rows_of(rec)
    content = [[i for i in r[:98] if i != v.eos_index] for r in rows]
    want = G.score_infill(m, list(ev), "cpu", v, ctl, TRACKS, BARS, content=content, pitches=pitches,
                          device_score=False)
    got = np.asarray(stats["logprobs"][0])
    keep = np.asarray([j for j, (k, _) in enumerate(rec)
                       if not (len(rows[k]) == 99 and j == max(q for q, (kk, _) in enumerate(rec) if kk == k))])
    assert want.tokens.tolist() == [rec[j][1] for j in keep]
    err = float(np.abs(got[keep] - want.logprobs).max())
    print("%s: %d entries, max |dlogprob| %.3g" % (path, len(keep), err))
    assert err <= 1e-12


def test_variations_share_fill_bar(host):  # noqa: F811
    m, v, ctl, ev, made = host
    stats = {}
    out = G.generation_all(m, list(ev), "cpu", v, None, ctl, TRACKS, BARS, variations=3, seed=30, fill_bar=True,
                           device_grammar=False, stats=stats)
    assert len(out) == 3 and len(stats["bar_fill"]) == 3
    takes = _last(made, 3)
    for rec, fill in zip(takes, stats["bar_fill"]):
        _check_spans(v, rec, fill)
    assert len({tuple(t) for t in takes}) > 1


# --------------------------------------------------------------------------
# templates under the clock, and validation
# --------------------------------------------------------------------------
def _row0(row):
    return [row] + [None] * (N_MASKS - 1)


def test_check_template_replays_its_rows_with_the_clock():
    v, ctl = _vocab()
    ev = _events()
    src, _, _, target, no_whole = G._prepare(list(ev), v, TRACKS, BARS)
    C = lambda t, L: G._check_template(t, v, src, target, ctl, no_whole, None, L)  # noqa: E731
    full = ['p_60', 'half', 'p_62', 'half']
    for bad in (['p_60', 'half', 'p_62', 'half', 'sixteenth'],      # a row that overruns
                ['p_60', 'whole', 'sep', 'p_64', 'half', 'quarter', 'eighth', 'sixteenth', 'sixteenth', 'sixteenth'],
                ['rest', 'half', 'quarter', '<eos>'],                # a closing <eos> on a bar that is not full
                ['<eos>'],
                full + [ANY_PITCH],                                  # ANY_PITCH at a full bar
                full + ['rest'], full + ['continue'], full + ['p_64'],
                ['p_60', 'quarter', v.index2char(ctl[0])]):          # a control token ends the span, as <eos> does
        with pytest.raises(ValueError):
            C(_row0(bad), 16)
    # what the clock allows: an exact bar closed by <eos>, a sep chord inside the bar, an opening
    for good in (full + ['<eos>'], ['p_60', 'whole', 'sep', 'p_64', 'half', 'rest', 'half', '<eos>'],
                 ['p_60', 'quarter', ANY_PITCH], ['rest', 'half', 'quarter']):
        assert C(_row0(good), 16)[0] is not None
    # the same rows pass without the keyword (the grammar alone), and 3/4 is a shorter bar
    assert C(_row0(['rest', 'half', 'quarter', '<eos>']), 0)[0] is not None
    assert C(_row0(['rest', 'half', 'quarter', '<eos>']), 12)[0] is not None
    with pytest.raises(ValueError):
        C(_row0(full + ['<eos>']), 12)
    # through the public call
    with pytest.raises(ValueError):
        G.generation_all(_Sentinel(), list(ev), "cpu", v, None, ctl, TRACKS, BARS, fill_bar=True,
                         template=_row0(['rest', 'half', 'quarter', '<eos>']))


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0, [True], (False,)], ids=repr)
def test_bad_fill_bar_raises_before_anything_is_touched(bad):
    v, ctl = _vocab()
    ev = _events()
    np.random.seed(5)
    st0 = np.random.get_state()
    for fn in (G.generation_all, G.infill):
        for kw in (dict(), dict(greedy=True), dict(seed=3), dict(variations=2), dict(use_kv_cache=False)):
            with pytest.raises(ValueError):
                fn(_Sentinel(), list(ev), "cpu", v, None, ctl, TRACKS, BARS, fill_bar=bad, **kw)
    reqs = [(list(ev), TRACKS, BARS)] * 2
    for b in ([bad, True], [True], [True] * 3) + (() if isinstance(bad, (list, tuple)) else (bad,)):
        for kw in (dict(greedy=True), dict(greedy=False, seed=[1, 2])):
            with pytest.raises(ValueError):
                G.generation_batch(_Sentinel(), reqs, v, ctl, fill_bar=b, **kw)
    assert _same_state(np.random.get_state(), st0)


def test_a_bar_that_is_no_whole_number_of_sixteenths_raises(monkeypatch):
    v, ctl = _vocab()
    ev = _events()
    real = G.durations_for_events

    def odd(events):  # a bar of 16.5 sixteenths
        a, b, c, bar = real(events)
        return a, b, c, bar + a['sixteenth'] / 2
    np.random.seed(6)
    st0 = np.random.get_state()
    for fake in (odd, lambda e: (real(e)[0], None, None, 300 * real(e)[0]['sixteenth']),
                 lambda e: (real(e)[0], None, None, 0.0)):
        monkeypatch.setattr(G, "durations_for_events", fake)
        with pytest.raises(ValueError):
            bar_units(ev)
        with pytest.raises(ValueError):
            G.generation_all(_Sentinel(), list(ev), "cpu", v, None, ctl, TRACKS, BARS, fill_bar=True)
        with pytest.raises(ValueError):
            G.generation_batch(_Sentinel(), [(list(ev), TRACKS, BARS)] * 2, v, ctl, fill_bar=[False, True])
    assert _same_state(np.random.get_state(), st0)

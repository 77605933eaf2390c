"""`chords=` on the host: the validation (`_check_chords`) raises before the
model or np.random is touched; `pitch_onsets` places every pitch by the
`_BarClock` rule; every host path draws the same tokens under a progression,
every pitch of a constrained span lies in the set that holds at its onset, the
spans without an entry are left alone, the scores are `score_infill`'s; under
`rhythm_template` a bar is reharmonised on its own rhythm; and with the bar
clock no reachable state is a dead end.  The model is the stand-in of
tests/test_template_cpu.py (logits by decoder row)."""
from collections import deque

import numpy as np
import pytest

from smer_music_generation_amd import generation as G
from smer_music_generation_amd.generation import ANY_PITCH, _BarClock, chord_tones, pitch_onsets, pitch_set
from tests.test_barclock_cpu import _code, _flags_after
from tests.test_template_cpu import (BARS, N_MASKS, PATHS, TRACKS, _events, _last, _rows_of, _run, _same_state,
                                     _Sentinel, _vocab, host)  # noqa: F401  (host: a fixture)

NOTE_MASKS = (0, 4)  # the 'r' spans among the nine masks of TRACKS x BARS: track 0, track 2
F_MAJ = pitch_set(classes=chord_tones(5, 'maj'))
C_7 = pitch_set(classes=chord_tones(0, '7'))
SPLIT = 8  # the second segment starts mid-bar (a bar of 16 sixteenths)
PROG = [(0, F_MAJ), (SPLIT, C_7)]


def _set_at(onset, prog=PROG, L=16):
    """The set of the last segment with start <= min(onset, L - 1), from the definition."""
    tau = min(onset, L - 1)
    return [s for a, s in prog if a <= tau][-1]


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------
def test_chord_tones_and_pitch_onsets():
    v, _ = _vocab()
    assert chord_tones(5, 'maj') == (5, 9, 0) and chord_tones(0, '7') == (0, 4, 7, 10)
    assert chord_tones(62, 'min') == (2, 5, 9) and chord_tones(11, 'dim') == (11, 2, 5)
    assert chord_tones(0, 'aug') == (0, 4, 8) and chord_tones(0, 'maj7') == (0, 4, 7, 11)
    assert chord_tones(9, 'min7') == (9, 0, 4, 7)
    for bad in ((True, 'maj'), (0.0, 'maj'), (0, 'sus4'), ('C', 'maj')):
        with pytest.raises(ValueError):
            chord_tones(*bad)
    assert set(F_MAJ) == {n for n in range(21, 109) if n % 12 in (5, 9, 0)}
    # a first pitch at 0
    assert pitch_onsets(v, ['p_60', 'quarter']) == [(0, 60)]
    # a two-token duration group: the next pitch sounds after their sum
    assert pitch_onsets(v, ['p_60', 'quarter', 'eighth', 'p_62', 'half']) == [(0, 60), (6, 62)]
    # a two-pitch chord: the second pitch reads the first one's position
    assert pitch_onsets(v, ['rest', 'half', 'p_60', 'p_64', 'quarter', 'p_65', 'quarter']) == \
        [(8, 60), (8, 64), (12, 65)]
    # sep: the pitch after it reads the rewound position
    assert pitch_onsets(v, ['p_60', 'quarter', 'p_62', 'half', 'sep', 'p_64', 'half', 'p_65', 'quarter']) == \
        [(0, 60), (4, 62), (4, 64), (12, 65)]
    ids = [v.char2index(t) for t in ('rest', 'eighth', 'p_72', 'eighth')]
    assert pitch_onsets(v, np.asarray(ids)) == [(2, 72)] and pitch_onsets(v, []) == []


# --------------------------------------------------------------------------
# validation
# --------------------------------------------------------------------------
def _bad_chords():
    many = [(k, [60 + k]) for k in range(16)]
    return {
        "not a dict": [(0, F_MAJ)],
        "a bar outside bars_to_generate": {5: PROG},
        "a (bar, track) bar outside": {(3, 0): PROG},
        "a track outside tracks_to_generate": {(2, 1): PROG},
        "a key of three": {(2, 0, 0): PROG},
        "a bool bar": {True: PROG},
        "a float bar": {2.0: PROG},
        "a float track": {(2, 0.0): PROG},
        "a string key": {"2": PROG},
        "a bool start": {2: [(False, F_MAJ)]},
        "a float start": {2: [(0.0, F_MAJ)]},
        "a float pitch": {2: [(0, [60.0])]},
        "a bool pitch": {2: [(0, [True])]},
        "a pitch out of range": {2: [(0, [20])]},
        "pitches no collection": {2: [(0, 60)]},
        "a segment of three": {2: [(0, F_MAJ, 1)]},
        "an empty segment list": {2: []},
        "segments no sequence": {2: 7},
        "a first start that is not 0": {2: [(4, F_MAJ)]},
        "starts that do not ascend": {2: [(0, F_MAJ), (8, C_7), (8, F_MAJ)]},
        "starts that descend": {2: [(0, F_MAJ), (8, C_7), (4, F_MAJ)]},
        "a negative start": {2: [(0, F_MAJ), (-1, C_7)]},
        "a start at L": {2: [(0, F_MAJ), (16, C_7)]},
        "an empty set": {2: [(0, [])]},
        "seventeen distinct sets": {2: many, (2, 2): [(0, [100])]},
    }


BAD = list(_bad_chords())


def _raises_everywhere(bad, **extra):
    v, ctl = _vocab()
    ev = _events()
    np.random.seed(5)
    st0 = np.random.get_state()
    for fn in (G.generation_all, G.infill):
        for kw in (dict(), dict(greedy=True), dict(seed=3), dict(variations=2), dict(use_kv_cache=False),
                   dict(fill_bar=True)):
            with pytest.raises(ValueError):
                fn(_Sentinel(), list(ev), "cpu", v, None, ctl, TRACKS, BARS, chords=bad, **extra, **kw)
    for kw in (dict(greedy=True), dict(greedy=False, seed=[1, 2]), dict(greedy=False, variations=2)):
        for b in (bad, [None, bad]):
            with pytest.raises(ValueError):
                G.generation_batch(_Sentinel(), [(list(ev), TRACKS, BARS)] * 2, v, ctl, chords=b, **extra, **kw)
    assert _same_state(np.random.get_state(), st0)


@pytest.mark.parametrize("name", BAD)
def test_bad_chords_raise_before_anything_is_touched(name):
    _raises_everywhere(_bad_chords()[name])


def test_an_effective_set_emptied_by_pitches_raises():
    _raises_everywhere({2: [(0, [60, 62])]}, pitches=[64, 65])
    _raises_everywhere({2: [(0, [60, 64]), (8, [62])]}, pitches={0: [60, 64]})  # track 0: the second segment


def test_a_bar_longer_than_64_sixteenths_raises(monkeypatch):
    v, ctl = _vocab()
    ev = _events()
    real = G.durations_for_events
    monkeypatch.setattr(G, "durations_for_events", lambda e: (real(e)[0], None, None, 65 * real(e)[0]['sixteenth']))
    assert G.bar_units(ev) == 65
    with pytest.raises(ValueError):
        G.generation_all(_Sentinel(), list(ev), "cpu", v, None, ctl, TRACKS, BARS, chords={2: PROG})
    monkeypatch.setattr(G, "durations_for_events", lambda e: (real(e)[0], None, None, 64 * real(e)[0]['sixteenth']))
    rec = G._check_chords({2: [(0, F_MAJ), (63, C_7)]}, [(ev, TRACKS, BARS)], [None], v)
    assert rec.L == 64 and rec.at[0, 62] == 0 and rec.at[0, 63] == 1


def test_per_request_and_one_for_all_forms():
    v, ctl = _vocab()
    ev = _events()
    reqs = [(list(ev), TRACKS, BARS)] * 2
    C = lambda x, n=2, alw=(None, None): G._check_chords(x, reqs[:n or 1], list(alw), v, n)  # noqa: E731
    assert C(None) == [None, None] and C({}) == [None, None]
    both = C({2: PROG})
    assert all(r is not None and r.L == 16 for r in both)
    one = C([None, {2: PROG}])
    assert one[0] is None and np.array_equal(one[1].at, both[0].at)
    for bad in ([{2: PROG}], [{2: PROG}] * 3, ({2: PROG},)):
        with pytest.raises(ValueError):
            C(bad)
    with pytest.raises(ValueError):  # the plugin call takes one dict
        C([{2: PROG}], None, (None,))
    with pytest.raises(ValueError):
        G.generation_all(_Sentinel(), list(ev), "cpu", v, None, ctl, TRACKS, BARS, chords=[{2: PROG}])
    # the record: rows per mask, only the note spans carry any; (bar, track) replaces the bar's entry
    rec = C({2: PROG, (2, 2): [(0, [60, 64, 67])]}, None, (None,))
    assert rec.at.shape == (N_MASKS, G.CHORD_POS) and rec.sets == (F_MAJ, C_7, (60, 64, 67))
    assert rec.at[0, :SPLIT].tolist() == [0] * SPLIT and (rec.at[0, SPLIT:] == 1).all() and (rec.at[4] == 2).all()
    assert (rec.at[[1, 2, 3, 5, 6, 7, 8]] == -1).all()
    pitch = G._pitch_mask(v)
    for k, s in enumerate(rec.sets):
        kept = {int(v.index2char(i)[2:]) for i in np.flatnonzero(pitch & ~rec.rows[k])}
        assert kept == set(s) and not rec.rows[k][~pitch].any()
    assert rec.row_at(0, 7) == 0 and rec.row_at(0, 8) == 1 and rec.row_at(0, 40) == 1 and rec.row_at(1, 0) == -1
    assert rec.row_at(N_MASKS, 0) == -1 and rec.row_at(0, -3) == 0
    # the effective set is the segment's set within the track's pitches= set; equal ones share a row
    alw = G._check_pitches({0: list(range(60, 72))}, TRACKS)
    rec = C({2: PROG}, None, (alw,))
    f0, c0 = tuple(p for p in F_MAJ if 60 <= p < 72), tuple(p for p in C_7 if 60 <= p < 72)
    assert rec.sets == (f0, c0, F_MAJ, C_7) and rec.at[0, 0] == 0 and rec.at[4, 0] == 2 and rec.at[4, 15] == 3


# --------------------------------------------------------------------------
# the rule on the host paths (stand-in model)
# --------------------------------------------------------------------------
MODES = [("greedy", dict(greedy=True), None), ("seeded", dict(seed=12), None),
         ("seeded t0.8 p0.9", dict(seed=5, t=0.8, p=0.9), None), ("shared stream", dict(), 31)]
KEYS = {"bar": {2: PROG}, "track 2": {(2, 2): PROG}}
# (the stand-in model ends track 2's span at once: an opening gives it three pitches of the
# model's choice, at 0, 8 and 12, in the chorded call and in the plain one alike)
OPENING = [None] * 4 + [[ANY_PITCH, 'half', ANY_PITCH, 'quarter', ANY_PITCH]] + [None] * 4


def _check_chorded(v, rec, log, constrained):
    """Every (onset, midi) of every constrained span is in its segment's set,
    and `log` (stats['chords'] of the take) is exactly that list.  Returns the
    number of pitches checked."""
    rows, n = _rows_of(rec), 0
    assert len(log) == len(constrained)
    for k, entries in zip(constrained, log):
        body = rows[k] if len(rows[k]) < 99 else rows[k][:-1]  # the cap drops the last draw... from the result only
        want = [(o, m, _set_at(o)) for o, m in pitch_onsets(v, rows[k])]
        assert entries == want, k
        for o, m in pitch_onsets(v, body):
            assert m in _set_at(o), (k, o, m)
            n += 1
    return n


@pytest.mark.parametrize("key", list(KEYS))
@pytest.mark.parametrize("mode", [m[0] for m in MODES])
def test_host_paths_agree_under_chords(host, mode, key):  # noqa: F811
    m, v, ctl, ev, made = host
    kw, unseeded = {k: (a, b) for k, a, b in MODES}[mode]
    kw = dict(kw, template=OPENING)
    constrained = NOTE_MASKS if key == "bar" else (4,)
    runs = []
    for path in PATHS:
        if unseeded is not None:
            np.random.seed(unseeded)
        (rec,), _, stats = _run(host, path, chords=KEYS[key], **kw)
        runs.append((rec, np.random.get_state() if unseeded is not None else None))
        assert "bar_fill" not in stats  # the clock runs, the bar line bans nothing
        assert _check_chorded(v, rec, stats["chords"][0], constrained) >= 3
        assert [o for o, _ in pitch_onsets(v, _rows_of(rec)[4])][:3] == [0, 8, 12]  # both segments are met
    assert runs[0][0] == runs[1][0] == runs[2][0]
    if unseeded is not None:
        assert all(_same_state(r[1], runs[0][1]) for r in runs)
        np.random.seed(unseeded)
    (plain,), _, st = _run(host, "single", **kw)
    assert "chords" not in st and plain != runs[0][0]
    outside = [(o, p) for k in constrained for o, p in pitch_onsets(v, _rows_of(plain)[k]) if p not in _set_at(o)]
    assert outside  # the plain call leaves the progression: the keyword changed the take
    # the spans without an entry, up to the first constrained draw, are the plain call's
    first = min(j for j, (k, _) in enumerate(runs[0][0]) if k in constrained)
    assert runs[0][0][:first] == plain[:first]
    if key != "bar":
        assert first > 0 and [x for x in runs[0][0] if x[0] < 4] == [x for x in plain if x[0] < 4]


def test_chords_with_fill_bar_pitches_and_variations(host):  # noqa: F811
    m, v, ctl, ev, made = host
    octave = tuple(range(55, 80))
    res = []
    for path in PATHS:
        (rec,), _, stats = _run(host, path, chords={2: PROG}, fill_bar=True, pitches=octave, seed=12)
        res.append(rec)
        assert len(stats["bar_fill"][0]) == 2
        rows = _rows_of(rec)
        for k, entries in zip(NOTE_MASKS, stats["chords"][0]):
            assert entries and all(p in s and set(s) <= set(octave) for _, p, s in entries)
            assert all(p in _set_at(o) and p in octave for o, p in pitch_onsets(v, rows[k]))
    assert res[0] == res[1] == res[2]
    stats = {}
    out = G.generation_all(m, list(ev), "cpu", v, None, ctl, TRACKS, BARS, variations=3, seed=30, chords={2: PROG},
                           device_grammar=False, stats=stats)
    takes = _last(made, 3)
    assert len(out) == 3 and len(stats["chords"]) == 3 and len({tuple(t) for t in takes}) > 1
    for rec, log in zip(takes, stats["chords"]):
        _check_chorded(v, rec, log, NOTE_MASKS)
    # a batch-mate without chords draws the plain tokens
    reqs = [(list(ev), TRACKS, BARS)] * 2
    common = dict(logger=None, precision="fp32", device_grammar=False, return_stats=True, greedy=False, seed=[7, 8])
    _, st = G.generation_batch(m, reqs, v, ctl, **common)
    plain = _last(made, 2)
    _, st = G.generation_batch(m, reqs, v, ctl, chords=[{2: PROG}, None], **common)
    mixed = _last(made, 2)
    assert mixed[1] == plain[1] and mixed[0] != plain[0] and st["chords"][1] is None
    _check_chorded(v, mixed[0], st["chords"][0], NOTE_MASKS)


@pytest.mark.parametrize("path", PATHS)
def test_logprobs_under_chords_are_score_infill_of_the_take(host, path):  # noqa: F811
    """The score is read before the clock and chord bans: the number
    score_infill gives for the take."""
    m, v, ctl, ev, made = host
    (rec,), _, stats = _run(host, path, chords={2: PROG}, logprobs=True, seed=12)
    rows = _rows_of(rec)
    content = [[i for i in r[:98] if i != v.eos_index] for r in rows]
    want = G.score_infill(m, list(ev), "cpu", v, ctl, TRACKS, BARS, content=content, device_score=False)
    got = np.asarray(stats["logprobs"][0])
    keep = np.asarray([j for j, (k, _) in enumerate(rec)
                       if not (len(rows[k]) == 99 and j == max(q for q, (kk, _) in enumerate(rec) if kk == k))])
    assert want.tokens.tolist() == [rec[j][1] for j in keep]
    err = float(np.abs(got[keep] - want.logprobs).max())
    print("%s: %d entries, max |dlogprob| %.3g" % (path, len(keep), err))
    assert err <= 1e-12


# --------------------------------------------------------------------------
# templates
# --------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_rhythm_template_reharmonises_a_bar_on_its_own_rhythm(host, path):  # noqa: F811
    m, v, ctl, ev, made = host
    bodies, codes = G._template_bodies(ev, v, TRACKS, BARS, None)
    tpl = G.rhythm_template(ev, v, TRACKS, BARS)
    (rec,), _, stats = _run(host, path, chords={2: PROG}, template=tpl, seed=9)
    rows, pitch, n_out = _rows_of(rec), G._pitch_mask(v), 0
    for k in NOTE_MASKS:
        src_on = [o for o, _ in pitch_onsets(v, bodies[k])]
        got = pitch_onsets(v, rows[k])
        assert [o for o, _ in got] == src_on  # the onsets are the source's
        assert any(o < SPLIT for o in src_on) and any(o >= SPLIT for o in src_on)  # one in each segment
        assert all(p in _set_at(o) for o, p in got)  # the pitches follow the segment
        assert [i for i in rows[k] if not pitch[i]] == [i for i in bodies[k] if not pitch[i]] + [v.eos_index]
        n_out += sum(p not in _set_at(o) for o, p in pitch_onsets(v, bodies[k]))
    assert n_out >= 1  # the source bar itself leaves the progression
    assert [e[:2] for e in stats["chords"][0][0]] == pitch_onsets(v, rows[0])


def _row0(row):
    return [row] + [None] * (N_MASKS - 1)


def test_check_template_rejects_a_pitch_outside_its_onsets_chord():
    v, ctl = _vocab()
    ev = _events()
    src, _, _, target, no_whole = G._prepare(list(ev), v, TRACKS, BARS)
    rec = G._check_chords({2: PROG}, [(ev, TRACKS, BARS)], [None], v)
    C = lambda t, ch=rec, L=0: G._check_template(t, v, src, target, ctl, no_whole, None, L, ch)  # noqa: E731
    # p_65 (F) holds in the first half, p_64 (E, of C7) in the second; p_60 (C) in both
    good = ['p_65', 'half', 'p_64', 'half', '<eos>']
    assert C(_row0(good))[0] is not None and C(_row0(good), rec, 16)[0] is not None
    for bad in (['p_64', 'half'],                       # E at 0 under F major
                ['p_65', 'half', 'p_65', 'half'],       # F at 8 under C7
                ['p_65', 'half', 'p_64', 'p_65'],       # the second note of a chord reads the first one's onset
                ['p_60', 'half', 'p_64', 'half', 'sep', 'p_65', 'quarter'],  # after sep: back at 8
                ['rest', 'quarter', 'eighth', 'sixteenth', 'p_64', 'quarter']):  # at 7: still F major
        with pytest.raises(ValueError):
            C(_row0(bad))
        assert C(_row0(bad), None)[0] is not None  # the grammar alone takes the row
    assert C(_row0(['rest', 'half', 'p_64', 'quarter']))[0] is not None  # at 8
    assert C(_row0(['p_65', 'half', 'sep', 'p_69', 'half']))[0] is not None  # after sep: back at 0
    # ANY_PITCH is always satisfiable; a span without an entry takes any pitch
    assert C(_row0(['p_65', 'half', ANY_PITCH, 'half', ANY_PITCH]))[0] == (
        v.char2index('p_65'), v.char2index('half'), -2, v.char2index('half'), -2)
    only2 = G._check_chords({(2, 2): PROG}, [(ev, TRACKS, BARS)], [None], v)
    assert C(_row0(['p_64', 'half']), only2)[0] is not None
    with pytest.raises(ValueError):
        C([None] * 4 + [['p_64', 'half']] + [None] * 4, only2)
    with pytest.raises(ValueError):  # through the public call
        G.generation_all(_Sentinel(), list(ev), "cpu", v, None, ctl, TRACKS, BARS, chords={2: PROG},
                         template=_row0(['p_64', 'half']))


# --------------------------------------------------------------------------
# no dead end: the search of tests/test_barclock_cpu.py with a chord ban
# --------------------------------------------------------------------------
@pytest.mark.parametrize("no_whole", [0, 1])
@pytest.mark.parametrize("L", [12, 16])
def test_no_reachable_state_is_a_dead_end_under_a_chord(L, no_whole):
    """The construction of test_no_reachable_state_is_a_dead_end with a
    position-dependent pitch ban that leaves ONE pitch: p_60 in the first half
    of the bar, p_67 in the second.  keep & ~clock & ~chord & ~reject is
    non-empty in every reachable (grammar flags, span start, T, P, A, G, S)."""
    v, ctl = _vocab()
    cls, units = G.grammar_tables(v, ctl)[1], G.unit_table(v)
    reps = {v.char2index('p_60'): 'pitch', v.char2index('p_67'): 'pitch', v.continue_index: 'continue',
            v.char2index('rest'): 'rest', v.char2index('sep'): 'sep', v.eos_index: 'end', ctl[0]: 'end',
            v.char2index('k_3'): 'other', v.pad_index: 'other'}
    reps.update({i: 'dur' for i in v.duration_only_indices})
    rows = np.zeros((2, v.vocab_size), dtype=bool)  # (the record is built by hand: L is not the fixture's)
    rows[:, v.pitch_indices] = True
    rows[0, v.char2index('p_60')] = rows[1, v.char2index('p_67')] = False
    at = np.full((1, G.CHORD_POS), 1, dtype=np.int8)
    at[0, :L // 2] = 0
    rec = G._Chords(L, at, rows, ((60,), (67,)))
    start = ((False,) * 4, True, 0, 0, 0, 0, 0)
    seen, todo, n_pitch = {start}, deque([start]), [0, 0]
    while todo:
        fl, first, T, P, A, Gp, S = todo.popleft()
        ck = _BarClock(L, cls, units)
        ck.T, ck.P, ck.A, ck.G, ck.S = T, P, A, Gp, S
        assert 0 <= ck.end <= L
        flags, check, _ = G.grammar_spec(v, _code(fl, first, no_whole))
        chord = rec.rows[rec.row_at(0, ck.end)]
        ok = G.allowed_ids(v, **flags) & ~ck.banned(v) & ~chord
        assert any(check is None or not check(int(i)) for i in np.flatnonzero(ok)), (fl, first, T, P, A, Gp, S)
        for i, kind in reps.items():
            if not ok[i] or kind == 'end':
                continue
            if kind == 'pitch':
                assert i == v.char2index('p_60' if ck.end < L // 2 else 'p_67')
                n_pitch[ck.end >= L // 2] += 1
            nk = _BarClock(L, cls, units)
            nk.T, nk.P, nk.A, nk.G, nk.S = T, P, A, Gp, S
            nk.advance(int(cls[i]), int(units[i]))
            nxt = (_flags_after(fl, kind), False, nk.T, nk.P, nk.A, nk.G, nk.S)
            if nxt not in seen:
                seen.add(nxt)
                todo.append(nxt)
    print("L %d no_whole %d: %d states, pitches drawn per half %r" % (L, no_whole, len(seen), n_pitch))
    assert len(seen) > 200 and min(n_pitch) > 0

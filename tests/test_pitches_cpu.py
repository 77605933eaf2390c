"""`pitches=` on the host: the public calls validate it before the model or
np.random is touched, `pitch_set` builds ranges and scales, `sampling(...,
ban=)` draws what `sampling()` draws from logits whose banned entries were
set to -100 by hand, and a `_Span` carrying ban rows keeps a constrained
track inside its set and leaves the other track alone."""
import itertools

import numpy as np
import pytest

from smer_music_generation_amd import generation as G
from smer_music_generation_amd.vocab import WordVocab
from tests.test_nucleus_gpu import FLAG_SETS, PS, TS, _state_code, kernel_rows

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']


class _Sentinel:
    """Stands in for the model: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the model was touched (%s)" % name)


def _requests():
    from smer_music_generation_amd.synth import synth_events
    return [(list(synth_events(60 + i, n_bars=6 + i, n_tracks=3)), [i % 3], [4]) for i in range(3)]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# an empty set, below and above the pitch tokens, a float, a bool, a track
# that is not generated (the requests mask tracks 0, 1, 2 in turn: 7 is in none)
BAD = [[], set(), [20], [60, 109], [60.0], [True], {7: [60]}, {0: []}, {0: [60.5]}, "60", 60,
       np.array([60.0])]


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_generation_all_rejects_bad_pitches(bad):
    v = WordVocab(0, CTRL)
    ev, tr, br = _requests()[0]
    np.random.seed(5)
    st0 = np.random.get_state()
    for fn in (G.generation_all, G.infill):
        for kw in (dict(), dict(greedy=True), dict(seed=3), dict(variations=2), dict(use_kv_cache=False)):
            with pytest.raises(ValueError):
                fn(_Sentinel(), list(ev), "cpu", v, None, [], tr, br, pitches=bad, **kw)
    assert _same_state(np.random.get_state(), st0)


@pytest.mark.parametrize("bad", BAD + [[None, [60]], [[60], [62]], [None] * 4, [[60], None, {2: [60]}, None],
                                       [None, {0: [60]}, None], [[60], 62, None], [None, [60], [True]]],
                         ids=repr)
def test_generation_batch_rejects_bad_pitches(bad):
    """Also a per-request list of the wrong length (2 and 4 entries for 3
    requests), a dict key that is not among ITS request's tracks (request 1
    masks track 1), and a list that mixes ints with per-request entries."""
    v = WordVocab(0, CTRL)
    np.random.seed(6)
    st0 = np.random.get_state()
    for kw in (dict(greedy=False), dict(greedy=True), dict(greedy=False, seed=[1, 2, 3]),
               dict(greedy=False, variations=2)):
        with pytest.raises(ValueError):
            G.generation_batch(_Sentinel(), _requests(), v, [], pitches=bad, **kw)
    assert _same_state(np.random.get_state(), st0)


def test_check_pitches_normalises_to_sorted_tuples():
    C = G._check_pitches
    assert C(None, [0, 1]) is None
    assert C([64, 60, 62, 60], [0, 1]) == {0: (60, 62, 64), 1: (60, 62, 64)}
    assert C({62, 60}, [2]) == {2: (60, 62)}
    assert C(range(21, 109), [1]) == {1: tuple(range(21, 109))}
    assert C(np.array([108, 21], dtype=np.int16), [0]) == {0: (21, 108)}
    assert C({1: (72, 60)}, [0, 1]) == {1: (60, 72)}
    assert C({0: [np.int64(40)], 1: frozenset([41])}, [0, 1]) == {0: (40,), 1: (41,)}
    assert C({}, [0]) is None
    out = C(np.array([60, 61]), [0])
    assert all(type(x) is int for x in out[0])
    # batched: one value for all requests, or one per request
    trk = [[0], [1], [0, 2]]
    assert C(None, trk, 3) == [None, None, None]
    assert C([60, 62, 64], trk, 3) == [{0: (60, 62, 64)}, {1: (60, 62, 64)}, {0: (60, 62, 64), 2: (60, 62, 64)}]
    assert C((60,), trk, 3) == [{0: (60,)}, {1: (60,)}, {0: (60,), 2: (60,)}]
    assert C([None, [61, 60], {2: [70]}], trk, 3) == [None, {1: (60, 61)}, {2: (70,)}]
    assert C([[60, 62, 64]] * 3, trk, 3)[2] == {0: (60, 62, 64), 2: (60, 62, 64)}
    assert C({0: [60]}, [[0], [0, 1]], 2) == [{0: (60,)}, {0: (60,)}]
    with pytest.raises(ValueError):  # one dict for all requests: its keys must fit every request
        C({0: [60]}, trk, 3)


def test_pitch_set():
    P = G.pitch_set
    assert P() == tuple(range(21, 109))
    assert P(28, 60) == tuple(range(28, 61))
    assert P(classes=[0]) == (24, 36, 48, 60, 72, 84, 96, 108)
    c_major = P(classes=(0, 2, 4, 5, 7, 9, 11))
    assert len(c_major) == 52 and all(n % 12 in (0, 2, 4, 5, 7, 9, 11) for n in c_major)
    assert P(60, 72, classes=(0, 7)) == (60, 67, 72)
    assert P(0, 23) == (21, 22, 23) and P(107, 200) == (107, 108) and P(-5, 500) == P()
    assert P(lo=100) == tuple(range(100, 109)) and P(hi=22) == (21, 22)
    assert list(P(40, 50)) == sorted(P(40, 50)) and isinstance(P(40, 50), tuple)
    for kw in (dict(lo=70, hi=60), dict(lo=109), dict(hi=20), dict(classes=()), dict(lo=61, hi=62, classes=[0])):
        with pytest.raises(ValueError):
            P(**kw)
    assert G._check_pitches(P(28, 60), [0]) == {0: P(28, 60)}


def _ban_for(v, rng, row, keep):
    """A random half of the pitch tokens, always with the row's best kept
    token when that is a pitch."""
    ban = np.zeros(v.vocab_size, dtype=bool)
    ban[rng.choice(v.pitch_indices, size=44, replace=False)] = True
    best = int(np.argmax(np.where(keep, row, -np.inf)))
    if best in v.pitch_indices:
        ban[best] = True
    return ban


def test_sampling_with_a_ban_equals_sampling_of_hand_edited_logits():
    """Every grammar state of FLAG_SETS x every (t, p) of the kernel test's
    grid, and greedy: the index and the stream afterwards are those of
    sampling() on a copy of the row whose banned entries are -100; an empty
    ban is no ban."""
    v = WordVocab(0, CTRL)
    rows, _ = kernel_rows(v.vocab_size)
    rng = np.random.default_rng(8)
    kinds = [(t, p, False) for t, p in itertools.product(TS, PS)] + [(1.0, None, True)]
    n = hit_best = 0
    for fi, (f, ln, tg) in enumerate(FLAG_SETS):
        flags = G.grammar_spec(v, _state_code(f, ln, tg))[0]
        keep = G.allowed_ids(v, **flags)
        for ki, (t, p, greedy) in enumerate(kinds):
            row = rows[(fi * len(kinds) + ki) % len(rows)]
            ban = _ban_for(v, rng, row, keep)
            edited = row.copy()
            edited[ban] = -100.0
            res = []
            for lg, kw in ((row, dict(ban=ban)), (edited, dict()), (row, dict()),
                           (row, dict(ban=np.zeros(v.vocab_size, dtype=bool)))):
                np.random.seed(1000 + n)
                idx = G.sampling(lg.copy(), v, p, t, greedy=greedy, **kw, **flags)
                res.append((int(idx), np.random.get_state()))
            assert res[0][0] == res[1][0] and _same_state(res[0][1], res[1][1]), (f, ln, tg, t, p)
            assert res[2][0] == res[3][0] and _same_state(res[2][1], res[3][1])
            hit_best += int(ban[int(np.argmax(np.where(keep, row, -np.inf)))])
            n += 1
    assert n == len(FLAG_SETS) * 31 and hit_best > 20  # the best kept token was banned in many rows


def _drive(v, sp, rows, own=None):
    """Run a span to its end on logits that depend on the span's position
    alone (mask index, tokens so far), so two spans that emit different
    tokens on one track still see the same rows on the other.  own: a
    RandomState restarted at every mask, so the other track's draws compare
    too.  Returns the ids per mask."""
    per_mask, last = {}, -1
    while not sp.done:
        k = sp.mask_idx
        if own is not None and k != last:
            own.seed(500 + k)
            last = k
        row = rows[(k * 101 + len(sp.this_in)) % len(rows)]
        per_mask.setdefault(k, []).append(sp.advance(row))
    return per_mask


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
def test_span_keeps_the_constrained_track_inside_its_set(greedy):
    v = WordVocab(0, CTRL)
    ctl = v.density_indices + v.occupation_indices
    ev = _requests()[1][0]
    tracks, bars = [0, 2], [2, 3]
    allowed = G._check_pitches({2: G.pitch_set(60, 71)}, tracks)
    bans = G._request_bans(v, ev, tracks, bars, allowed)
    of_mask, ban_rows = bans
    # for each bar: track 0's r, d, o, p, then track 2's r, d, o, p, t (the last track)
    assert of_mask == ([-1] * 4 + [0] * 5) * 2 and ban_rows.shape == (1, v.vocab_size)
    ok = {v.char2index('p_%d' % n) for n in range(60, 72)}
    assert set(np.flatnonzero(~ban_rows[0])) & set(v.pitch_indices) == ok
    assert not ban_rows[0][[i for i in range(v.vocab_size) if i not in v.pitch_indices]].any()
    src, _, _, target, no_whole = G._prepare(list(ev), v, tracks, bars)
    assert len(target) == len(of_mask)
    # synthetic logits whose largest entries are banned pitches
    rows = (np.random.default_rng(4).standard_normal((4000, v.vocab_size)) * 2.0).astype(np.float32)
    rows[:, np.flatnonzero(ban_rows[0])] += np.float32(5.0)
    own_a, own_b = np.random.RandomState(1), np.random.RandomState(1)
    free = G._Span(v, src, target, ctl, no_whole, greedy, None, rng=own_a)
    held = G._Span(v, src, target, ctl, no_whole, greedy, None, rng=own_b, bans=bans)
    a, b = _drive(v, free, rows, own_a), _drive(v, held, rows, own_b)
    pitch = set(v.pitch_indices)
    seen_ok = seen_banned = 0
    for k, kb in enumerate(of_mask):
        if kb < 0:  # the other track: the unconstrained draw
            assert a[k] == b[k]
        else:
            got = [i for i in b[k] if i in pitch]
            assert all(i in ok for i in got)
            seen_ok += len(got)
            seen_banned += sum(1 for i in a[k] if i in pitch and i not in ok)
    assert seen_ok > 0 and seen_banned > 0  # the constraint changed something
    assert any(i in pitch and i not in ok for k, kb in enumerate(of_mask) if kb < 0 for i in b[k])


def test_span_with_every_pitch_allowed_is_the_unconstrained_span():
    v = WordVocab(0, CTRL)
    ctl = v.density_indices + v.occupation_indices
    ev, tr, _ = _requests()[1]
    bars = [2, 3]
    src, _, _, target, no_whole = G._prepare(list(ev), v, tr, bars)
    bans = G._request_bans(v, ev, tr, bars, G._check_pitches(range(21, 109), tr))
    assert bans is not None and not bans[1].any()
    rows = (np.random.default_rng(4).standard_normal((4000, v.vocab_size)) * 3.0).astype(np.float32)
    res = []
    for kw in (dict(), dict(bans=bans)):
        np.random.seed(99)
        sp = G._Span(v, src, target, ctl, no_whole, False, None, 0.9, 0.95, **kw)
        got = []
        while not sp.done:
            got.append(sp.advance(rows[len(got)]))
        res.append((got, sp.total, np.random.get_state()))
    assert res[0][0] == res[1][0] and len(res[0][0]) > 10 and res[0][1] == res[1][1]
    assert _same_state(res[0][2], res[1][2])


def test_ban_bits_layout():
    rows = np.zeros((2, 309), dtype=bool)
    rows[0, [0, 31, 32, 308]] = True
    rows[1, 65] = True
    bits = G.ban_bits(rows)
    assert bits.shape == (2, 16) and bits.dtype == np.uint32
    assert bits[0, 0] == (1 | 1 << 31) and bits[0, 1] == 1 and bits[0, 9] == 1 << (308 - 288)
    assert bits[1, 2] == 2 and bits[1].sum() == 2 and bits[0, 2:9].sum() == 0

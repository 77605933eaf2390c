"""Scores of given content on the host: the scoring plan (`_forced_plan`)
replays content through a `_Span` exactly as the decode drew it -- same
tokens, same masks, same numbers from the same logits rows -- counts its
entries by the documented rule, takes the events' own content by default,
refuses bad input before the model or np.random is touched, and scores an
out-of-grammar token from -100 instead of refusing it."""
import numpy as np
import pytest
import torch

from smer_music_generation_amd import generation as G
from smer_music_generation_amd.generation import InfillScore, score_batch, score_infill
from smer_music_generation_amd.synth import synth_events
from smer_music_generation_amd.vocab import WordVocab
from smer_music_generation_amd.wire import decoder_targets, mask_targets

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']
TRACKS, BARS = [0, 2], [2, 3]  # track 2 is the last one: its bars end in a 't' span


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


def _bodies(v, tgt_inp):
    """The spans of a decoder input [m_0, body...]*, without their m_0."""
    m0, out = v.char2index('m_0'), []
    for x in tgt_inp:
        if x == m0:
            out.append([])
        else:
            out[-1].append(int(x))
    return out


# --------------------------------------------------------------------------
# the plan against the span loop that drew the content
# --------------------------------------------------------------------------
def _table(v, ctl, ban_rows):
    """Logits rows indexed by decoder row (prefix length - 1).  <eos> is out
    of reach on the first 130 rows, so the first note span (rows 0 .. 98)
    runs into the 100-token cap, and wins every seventh row after them, so
    later note spans end on a drawn <eos>; control tokens sit low, so a note
    span never ends on one (a control span admits nothing else)."""
    rows = (np.random.default_rng(9).standard_normal((2000, v.vocab_size)) * 2.0).astype(np.float32)
    rows[:, ctl] -= np.float32(15.0)
    rows[:, np.flatnonzero(ban_rows[0])] += np.float32(3.0)  # banned pitches among the largest
    rows[:, v.mask_indices] = np.float32(-30.0)  # (no state masks m_0: a body must not hold one)
    rows[:, v.eos_index] = np.float32(-30.0)
    rows[np.arange(130, 2000)[5::7], v.eos_index] = np.float32(12.0)
    return rows


def _decode(v, ctl, src, target, no_whole, rows, bans, greedy):
    """A scoring span to its end on the table: per draw (mask, id, logp)."""
    np.random.seed(1)
    rng = None if greedy else np.random.RandomState(8)
    sp = G._Span(v, src, target, ctl, no_whole, greedy, None, 1.0, None, rng if rng is not None else np.random,
                 bans, score=True)
    draws = []
    while not sp.done:
        k = sp.mask_idx
        idx = sp.advance(rows[len(sp.prefix()) - 1])
        draws.append((k, int(idx)))
    assert len(sp.logp) == len(draws)
    return sp, [(k, i, lp) for (k, i), lp in zip(draws, sp.logp)]


CASES = [("greedy", True, False), ("greedy+ban", True, True), ("seeded", False, False),
         ("seeded+ban", False, True)]


@pytest.fixture(scope="module")
def span_runs():
    v, ctl = _vocab()
    ev = _events()
    allowed = G._check_pitches({2: G.pitch_set(60, 71)}, TRACKS)
    bans = G._request_bans(v, ev, TRACKS, BARS, allowed)
    src, _, _, target, no_whole = G._prepare(list(ev), v, TRACKS, BARS)
    rows = _table(v, ctl, bans[1])
    np.random.seed(77)
    st0 = np.random.get_state()
    runs = {}
    for name, greedy, ban in CASES:
        bn = bans if ban else None
        sp, draws = _decode(v, ctl, src, target, no_whole, rows, bn, greedy)
        np.random.seed(77)
        plan = G._forced_plan(v, src, target, ctl, no_whole, _bodies(v, sp.tgt_inp), bn)
        lp, arg = G._host_scores(v, plan, rows)
        assert _same_state(np.random.get_state(), st0)
        runs[name] = (sp, draws, plan, lp, arg)
    return v, ctl, target, rows, runs


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_plan_scores_what_the_span_loop_drew(span_runs, name):
    v, ctl, target, rows, runs = span_runs
    sp, draws, plan, lp, arg = runs[name]
    assert plan.tgt == sp.tgt_inp
    n_masks = len(target)
    per_mask = [[d for d in draws if d[0] == k] for k in range(n_masks)]
    kept = []
    for k, ds in enumerate(per_mask):
        assert len(ds) <= 99
        if len(ds) == 99:  # the cap ended the span: its 99th draw is dropped on the decode side
            assert target[k] == 'r'
            mine = np.flatnonzero(plan.mask_index == k)
            assert len(mine) == 98
            assert plan.ids[mine].tolist() == [i for _, i, _ in ds[:98]]
            assert np.abs(lp[mine] - np.array([x for _, _, x in ds[:98]])).max() <= 1e-12
            ds = ds[:98]
        kept += ds
    assert plan.ids.tolist() == [i for _, i, _ in kept]
    assert plan.mask_index.tolist() == [k for k, _, _ in kept]
    assert plan.ids.dtype == np.int64 and plan.mask_index.dtype == np.int32 and lp.dtype == np.float64
    err = float(np.abs(lp - np.array([x for _, _, x in kept])).max())
    print("%s: %d entries, max |dlogprob| %.3g" % (name, len(kept), err))
    assert err <= 1e-12
    if name.startswith("greedy"):  # the argmax of the masked row is what the greedy loop drew
        assert arg.tolist() == plan.ids.tolist()
    if name.endswith("+ban"):
        assert (plan.ban_idx >= 0).any() and (plan.ban_idx == -1).any()
    else:
        assert (plan.ban_idx == -1).all()
    # the row that predicts a token is the row of the input token before it
    m0 = v.char2index('m_0')
    for n in range(len(plan.ids)):
        if plan.ids[n] != v.eos_index:
            assert plan.tgt[plan.row[n] + 1] == plan.ids[n]
        else:
            assert plan.row[n] + 1 == len(plan.tgt) or plan.tgt[plan.row[n] + 1] == m0


def test_the_cases_cover_eos_cap_and_every_control_kind(span_runs):
    v, ctl, target, rows, runs = span_runs
    eos_spans = capped = 0
    kinds = set()
    for sp, draws, plan, lp, arg in runs.values():
        for k, tc in enumerate(target):
            ds = [d for d in draws if d[0] == k]
            if tc != 'r':
                assert len(ds) == 1 and ds[0][1] in ctl
                kinds.add(tc)
            elif len(ds) == 99:
                capped += 1
            elif ds[-1][1] == v.eos_index and len(ds) >= 3:
                eos_spans += 1
    print("note spans ended by a drawn <eos> after >= 2 tokens: %d, capped: %d, kinds %s"
          % (eos_spans, capped, sorted(kinds)))
    assert eos_spans >= 1 and capped >= 1 and kinds == {'d', 'o', 'p', 't'}


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_entry_count(span_runs, name):
    """Sum over note spans of n + 1 (98 at the cap) plus the control spans."""
    v, ctl, target, rows, runs = span_runs
    sp, draws, plan, lp, arg = runs[name]
    bodies = _bodies(v, sp.tgt_inp)
    want = 0
    for tc, b in zip(target, bodies):
        if tc == 'r':
            assert not b or b[-1] not in ctl  # (a span a control token ended would score no <eos>)
            want += 98 if len(b) == 98 else len(b) + 1
        else:
            want += 1
    assert len(plan.ids) == len(lp) == want
    assert np.bincount(plan.mask_index, minlength=len(target)).tolist() == [
        1 if tc != 'r' else (98 if len(b) == 98 else len(b) + 1) for tc, b in zip(target, bodies)]


# --------------------------------------------------------------------------
# the public calls on a stand-in model (host scoring: the definition)
# --------------------------------------------------------------------------
class _TableModel:
    """A model whose logits depend on the position alone: row t of `table`
    for every request; records what forward was given."""
    precision = "fp32"

    def __init__(self, table):
        self.table = torch.from_numpy(table)
        self.embedding = type("E", (), {"weight": torch.zeros(1)})()
        self.need_weights = True
        self.calls = []

    def eval(self):
        return self

    def set_precision(self, p):
        self.precision = p

    def forward(self, src, tgt, src_key_padding_mask, tgt_key_padding_mask, memory_key_padding_mask,
                tgt_mask):
        assert not torch.is_grad_enabled() and not self.need_weights
        self.calls.append((src.clone(), tgt.clone(), src_key_padding_mask.clone(),
                           tgt_key_padding_mask.clone(), memory_key_padding_mask.clone(), tgt_mask.clone()))
        B, T = tgt.shape
        return self.table[:T].unsqueeze(0).repeat(B, 1, 1), None


def _own_bodies(v, ev, tracks, bars):
    _, pos = mask_targets(ev, tracks, bars)
    stream = decoder_targets(ev, v, pos, bars)
    m0, eos, out = v.char2index('m_0'), v.eos_index, []
    for x in stream:
        if x == m0:
            out.append([])
        elif x != eos:
            out[-1].append(x)
    return out


def test_content_none_is_the_events_own_content():
    v, ctl = _vocab()
    ev = _events()
    table = (np.random.default_rng(3).standard_normal((600, v.vocab_size)) * 2).astype(np.float32)
    m = _TableModel(table)
    np.random.seed(5)
    st0 = np.random.get_state()
    a = score_infill(m, list(ev), "cpu", v, ctl, TRACKS, BARS)
    bodies = _own_bodies(v, ev, TRACKS, BARS)
    b = score_infill(m, list(ev), "cpu", v, ctl, TRACKS, BARS, content=bodies)
    c = score_infill(m, list(ev), "cpu", v, ctl, TRACKS, BARS,
                     content=[[v.index2char(i) for i in body] for body in bodies])
    assert _same_state(np.random.get_state(), st0)
    assert isinstance(a, InfillScore) and len(a.tokens) > len(bodies)
    for other in (b, c):
        for x, y in zip(a, other):
            assert np.array_equal(x, y)
    assert a.score == float(np.sum(a.logprobs)) and a.logprobs.dtype == np.float64
    assert a.tokens.dtype == np.int64 and a.mask_index.dtype == np.int32 and a.greedy.dtype == np.int64
    assert sorted(set(a.mask_index.tolist())) == list(range(len(bodies)))
    # it is token_logprobs on the table's rows, at the grammar state of every position
    src, _, _, target, no_whole = G._prepare(list(ev), v, TRACKS, BARS)
    plan = G._forced_plan(v, src, target, ctl, no_whole, bodies)
    lp, arg = G._host_scores(v, plan, table)
    assert np.array_equal(a.logprobs, lp) and np.array_equal(a.greedy, arg)
    assert np.array_equal(a.tokens, plan.ids)
    assert m.need_weights is True and len(m.calls) == 3


def test_score_batch_pads_under_the_three_masks():
    v, ctl = _vocab()
    reqs = [(list(synth_events(60 + i, n_bars=6 + i, n_tracks=3)), [i % 3], [2, 3] if i % 2 else [4])
            for i in range(3)]
    table = (np.random.default_rng(4).standard_normal((600, v.vocab_size)) * 2).astype(np.float32)
    m = _TableModel(table)
    out = score_batch(m, reqs, v, ctl, pitches=[None, G.pitch_set(48, 72), None])
    assert len(out) == 3 and len(m.calls) == 1
    src, tgt, skpm, tkpm, mkpm, mask = m.calls[0]
    lens_s = [len(G._prepare(list(e), v, t, b)[0]) for e, t, b in reqs]
    assert src.shape == (3, max(lens_s)) and len(set(lens_s)) > 1
    assert [int((~r).sum()) for r in skpm] == lens_s and torch.equal(skpm, mkpm)
    lens_t = [int((~r).sum()) for r in tkpm]
    assert tgt.shape == (3, max(lens_t)) and len(set(lens_t)) > 1
    assert torch.equal(mask[0], G.gen_nopeek_mask(tgt.shape[1]))
    singles = [score_infill(_TableModel(table), list(e), "cpu", v, ctl, t, b,
                            pitches=None if i != 1 else G.pitch_set(48, 72))
               for i, (e, t, b) in enumerate(reqs)]
    for x, y in zip(out, singles):
        for f, g in zip(x, y):
            assert np.array_equal(f, g)


def test_out_of_grammar_token_scores_from_minus_100():
    v, ctl = _vocab()
    ev = _events()
    table = (np.random.default_rng(6).standard_normal((600, v.vocab_size)) * 2).astype(np.float32)
    bodies = _own_bodies(v, ev, [0], [2])
    assert len(bodies) == 4 and len(bodies[0]) >= 2
    base = score_infill(_TableModel(table), list(ev), "cpu", v, ctl, [0], [2], content=bodies)
    # a structure token is kept by no state; as the second token of the note span
    bad = v.structure_indices[0]
    edited = [list(b) for b in bodies]
    edited[0][1] = bad
    got = score_infill(_TableModel(table), list(ev), "cpu", v, ctl, [0], [2], content=edited)
    assert got.tokens[1] == bad and np.isfinite(got.logprobs).all()
    src, _, _, target, no_whole = G._prepare(list(ev), v, [0], [2])
    plan = G._forced_plan(v, src, target, ctl, no_whole, edited)
    keep = G.allowed_ids(v, **G.grammar_spec(v, int(plan.code[1]))[0])
    assert not keep[bad]
    x = np.where(keep, table[plan.row[1]].astype(np.float64), -100.0)
    lse = x.max() + np.log(np.sum(np.exp(x - x.max())))
    assert abs(got.logprobs[1] - (-100.0 - lse)) <= 1e-12 and got.logprobs[1] < -90
    assert got.logprobs[0] == base.logprobs[0] and got.greedy[1] == base.greedy[1]
    # a pitch banned under pitches= scores from -100 too
    pitch = next(i for i in bodies[0] if i in v.pitch_indices)
    n = bodies[0].index(pitch)
    midi = int(v.index2char(pitch)[2:])
    other = [p for p in range(40, 80) if p != midi]
    banned = score_infill(_TableModel(table), list(ev), "cpu", v, ctl, [0], [2], content=bodies, pitches=other)
    assert banned.tokens[n] == pitch and banned.logprobs[n] < -90 and base.logprobs[n] > -50


# --------------------------------------------------------------------------
# errors: before the model or np.random is touched
# --------------------------------------------------------------------------
def _bad_contents(v, bodies):
    note = next(k for k, b in enumerate(bodies) if len(b) > 1)
    ctl_k = next(k for k, b in enumerate(bodies) if len(b) == 1)

    def edit(k, new):
        out = [list(b) for b in bodies]
        out[k] = new
        return out
    filler = [v.pitch_indices[3], v.duration_only_indices[2]]
    return {
        "one span short": bodies[:-1],
        "one span more": bodies + [[bodies[ctl_k][0]]],
        "empty control span": edit(ctl_k, []),
        "two-token control span": edit(ctl_k, bodies[ctl_k] * 2),
        "99-token note body": edit(note, (filler * 50)[:99]),
        "m_0 in a body": edit(note, [bodies[note][0], v.char2index('m_0')]),
        "<eos> in a body": edit(note, bodies[note] + [v.eos_index]),
        "'<eos>' in a body": edit(note, [v.index2char(i) for i in bodies[note]] + ['<eos>']),
        "unknown token": edit(note, ['p_60x']),
        "id past the vocabulary": edit(note, [v.vocab_size]),
        "negative id": edit(note, [-1]),
        "a float": edit(note, [3.0]),
        "a string for a span": edit(note, "p_60"),
        "not a list": 7,
    }


def test_errors_are_raised_before_the_model_is_touched():
    v, ctl = _vocab()
    ev = _events()
    bodies = _own_bodies(v, ev, TRACKS, BARS)
    np.random.seed(11)
    st0 = np.random.get_state()
    for why, content in _bad_contents(v, bodies).items():
        with pytest.raises(ValueError):
            score_infill(_Sentinel(), list(ev), "cpu", v, ctl, TRACKS, BARS, content=content)
            pytest.fail(why)
        with pytest.raises(ValueError):
            score_batch(_Sentinel(), [(list(ev), TRACKS, BARS)], v, ctl, contents=[content])
    for bad in ([], [20], [60.0], [True], {1: [60]}, "C4"):  # a bad pitches
        with pytest.raises(ValueError):
            score_infill(_Sentinel(), list(ev), "cpu", v, ctl, TRACKS, BARS, pitches=bad)
        with pytest.raises(ValueError):
            score_batch(_Sentinel(), [(list(ev), TRACKS, BARS)], v, ctl, pitches=[bad])
    for tr, br in (([], BARS), (TRACKS, [])):  # nothing masked
        with pytest.raises(ValueError):
            score_infill(_Sentinel(), list(ev), "cpu", v, ctl, tr, br)
    with pytest.raises(ValueError):
        score_batch(_Sentinel(), [], v, ctl)
    with pytest.raises(ValueError):  # one contents value per request
        score_batch(_Sentinel(), [(list(ev), TRACKS, BARS)], v, ctl, contents=[None, None])
    with pytest.raises(ValueError):
        score_batch(_Sentinel(), [(list(ev), TRACKS, BARS)], v, ctl, device_score=1)
    with pytest.raises(ValueError):
        score_batch(_Sentinel(), [(list(ev), TRACKS, BARS)], v, ctl, precision="fp16")
    assert _same_state(np.random.get_state(), st0)


def test_a_98_token_body_is_accepted_and_scores_no_end_token():
    v, ctl = _vocab()
    ev = _events()
    bodies = _own_bodies(v, ev, [0], [2])
    table = (np.random.default_rng(8).standard_normal((600, v.vocab_size)) * 2).astype(np.float32)
    full = [list(b) for b in bodies]
    full[0] = [v.pitch_indices[3], v.duration_only_indices[2]] * 49
    got = score_infill(_TableModel(table), list(ev), "cpu", v, ctl, [0], [2], content=full)
    assert int((got.mask_index == 0).sum()) == 98 and v.eos_index not in got.tokens[:98].tolist()
    short = [list(b) for b in full]
    short[0] = full[0][:97]
    got = score_infill(_TableModel(table), list(ev), "cpu", v, ctl, [0], [2], content=short)
    assert int((got.mask_index == 0).sum()) == 98 and got.tokens[97] == v.eos_index

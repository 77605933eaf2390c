"""Take scores on the host: `logprobs=` / `rank=` are validated before the
model or np.random is touched, `token_logprobs` is the log of the
distribution `sampling()` builds at t = 1 (and stays finite where a naive
softmax overflows), and a `_Span` that scores emits exactly what it emits
without, with the helper's value at every emitted id."""
import numpy as np
import pytest

from smer_music_generation_amd import generation as G
from smer_music_generation_amd.vocab import WordVocab
from tests.test_nucleus_gpu import FLAG_SETS, _state_code, kernel_rows

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']


class _Sentinel:
    """Stands in for the model: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the model was touched (%s)" % name)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _requests():
    from smer_music_generation_amd.synth import synth_events
    return [(list(synth_events(60 + i, n_bars=6 + i, n_tracks=3)), [i % 3], [4]) for i in range(3)]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


BAD = [1, 0, None, "yes", 1.0, [True], (), np.array([True])]


@pytest.mark.parametrize("bad", BAD, ids=repr)
@pytest.mark.parametrize("name", ["logprobs", "rank"])
def test_generation_all_rejects_bad_logprobs_and_rank(name, bad):
    v = WordVocab(0, CTRL)
    ev, tr, br = _requests()[0]
    np.random.seed(5)
    st0 = np.random.get_state()
    for fn in (G.generation_all, G.infill):
        for kw in (dict(), dict(greedy=True), dict(seed=3), dict(variations=2), dict(use_kv_cache=False),
                   dict(variations=2, logprobs=True) if name == "rank" else dict(variations=2, rank=True)):
            with pytest.raises(ValueError):
                fn(_Sentinel(), list(ev), "cpu", v, None, [], tr, br, **{name: bad}, **kw)
    assert _same_state(np.random.get_state(), st0)


@pytest.mark.parametrize("bad", BAD, ids=repr)
@pytest.mark.parametrize("name", ["logprobs", "rank"])
def test_generation_batch_rejects_bad_logprobs_and_rank(name, bad):
    v = WordVocab(0, CTRL)
    np.random.seed(6)
    st0 = np.random.get_state()
    for kw in (dict(greedy=False), dict(greedy=True), dict(greedy=False, seed=[1, 2, 3]),
               dict(greedy=False, variations=2), dict(greedy=False, variations=[1, 2, 3])):
        with pytest.raises(ValueError):
            G.generation_batch(_Sentinel(), _requests(), v, [], **{name: bad}, **kw)
    assert _same_state(np.random.get_state(), st0)


def test_rank_without_variations_is_an_error():
    v = WordVocab(0, CTRL)
    ev, tr, br = _requests()[0]
    np.random.seed(7)
    st0 = np.random.get_state()
    for kw in (dict(), dict(logprobs=True), dict(seed=3), dict(greedy=True), dict(use_kv_cache=False)):
        for fn in (G.generation_all, G.infill):
            with pytest.raises(ValueError):
                fn(_Sentinel(), list(ev), "cpu", v, None, [], tr, br, rank=True, **kw)
        if "use_kv_cache" not in kw:
            with pytest.raises(ValueError):
                G.generation_batch(_Sentinel(), _requests(), v, [], rank=True, **kw)
    assert _same_state(np.random.get_state(), st0)


def test_token_logprobs_is_the_log_of_the_reference_softmax():
    """The kernel test's rows (kept logits below -100, rows around -80, exact
    -100 ties) under every grammar state of FLAG_SETS."""
    v = WordVocab(0, CTRL)
    rows, _ = kernel_rows(v.vocab_size)
    worst = 0.0
    for i, row in enumerate(rows):
        f, ln, tg = FLAG_SETS[i % 8]
        keep = G.allowed_ids(v, **G.grammar_spec(v, _state_code(f, ln, tg))[0])
        lp = G.token_logprobs(row, keep)
        assert lp.dtype == np.float64 and lp.shape == (v.vocab_size,)
        ref = np.log(G.softmax_with_temperature(np.where(keep, row.astype(np.float64), -100.0), 1.0))
        assert np.isfinite(np.exp(lp)).all() and np.isfinite(lp).all()
        worst = max(worst, float(np.abs(lp - ref).max()))
        assert abs(np.exp(lp).sum() - 1.0) < 1e-12
    assert worst < 1e-12


def test_token_logprobs_survives_logits_a_naive_exp_overflows_on():
    v = WordVocab(0, CTRL)
    V = v.vocab_size
    keep = G.allowed_ids(v, **G.grammar_spec(v, 11)[0])
    kept = np.flatnonzero(keep)
    row = (np.random.default_rng(1).standard_normal(V) * 4).astype(np.float32)
    row[kept[[3, 40]]] = 800.0
    with np.errstate(over="ignore", invalid="ignore"):
        naive = G.softmax_with_temperature(np.where(keep, row.astype(np.float64), -100.0), 1.0)
    assert not np.isfinite(naive).all()
    lp = G.token_logprobs(row, keep)
    assert np.isfinite(lp).all()
    assert abs(np.exp(lp).sum() - 1.0) < 1e-12
    assert abs(lp[kept[3]] - np.log(0.5)) < 1e-12 and lp[kept[3]] == lp[kept[40]]


@pytest.mark.parametrize("value", [0.0, 3.5, 800.0])
def test_token_logprobs_of_a_lone_kept_entry_is_zero(value):
    V = 309
    keep = np.zeros(V, dtype=bool)
    keep[17] = True
    row = np.full(V, 5.0, dtype=np.float32)  # the masked ones would win unmasked
    row[17] = value
    lp = G.token_logprobs(row, keep)
    assert abs(lp[17]) < 1e-12  # 308 masked entries at e^-100 of it
    assert np.allclose(lp[~keep], -100.0 - value, atol=1e-9)


def test_token_logprobs_widens_from_float32():
    """A float64 row is rounded to float32 first, as sampling() does."""
    rng = np.random.default_rng(2)
    row = rng.standard_normal(309) * 3
    keep = rng.random(309) < 0.7
    assert np.array_equal(G.token_logprobs(row, keep), G.token_logprobs(row.astype(np.float32), keep))
    assert not np.array_equal(row, row.astype(np.float32).astype(np.float64))


def _span_case():
    v = WordVocab(0, CTRL)
    ctl = v.density_indices + v.occupation_indices
    ev = _requests()[1][0]
    tracks, bars = [0, 2], [2, 3]
    bans = G._request_bans(v, ev, tracks, bars, G._check_pitches({2: G.pitch_set(60, 71)}, tracks))
    src, _, _, target, no_whole = G._prepare(list(ev), v, tracks, bars)
    rows = (np.random.default_rng(4).standard_normal((4000, v.vocab_size)) * 2.0).astype(np.float32)
    rows[:, np.flatnonzero(bans[1][0])] += np.float32(3.0)  # banned pitches among the largest
    # every third row: one density token far above everything, so the states
    # whose redraw check rejects it draw it twelve times and give up
    rows[::3, v.density_indices[2]] = np.float32(60.0)
    return v, ctl, src, target, no_whole, bans, rows


def _run(v, ctl, src, target, no_whole, rows, *, score, seeded, bans, greedy=False, t=1.0, p=None):
    """A span to its end on rows picked by its position; with score, the
    expected log-probabilities from the keep of each draw."""
    lg = _Log()
    np.random.seed(31)
    rng = np.random.RandomState(8) if seeded else np.random
    kw = dict(score=True) if score else {}
    sp = G._Span(v, src, target, ctl, no_whole, greedy, lg, t, p, rng, bans, **kw)
    ids, want, banned_draws = [], [], 0
    while not sp.done:
        row = rows[(sp.mask_idx * 101 + len(sp.this_in)) % len(rows)]
        keep = G.allowed_ids(v, **sp.spec()[0])
        ban = sp.ban()
        if ban is not None:
            keep = keep & ~ban
            banned_draws += 1
        idx = sp.advance(row)
        ids.append(int(idx))
        want.append(G.token_logprobs(row, keep)[idx])
    own = rng.get_state()
    return sp, ids, lg.lines, own, np.random.get_state(), want, banned_draws


@pytest.mark.parametrize("kind", ["seeded", "global", "seeded+ban", "global+ban", "greedy+ban", "tp+ban"])
def test_span_with_scoring_emits_what_it_emits_without(kind):
    v, ctl, src, target, no_whole, bans, rows = _span_case()
    kw = dict(seeded=kind.startswith("seeded"), bans=bans if kind.endswith("+ban") else None,
              greedy=kind.startswith("greedy"))
    if kind.startswith("tp"):
        kw.update(t=0.7, p=0.9)
    a = _run(v, ctl, src, target, no_whole, rows, score=False, **kw)
    b = _run(v, ctl, src, target, no_whole, rows, score=True, **kw)
    assert a[1] == b[1] and len(a[1]) > 20
    assert a[2] == b[2]
    assert _same_state(a[3], b[3]) and _same_state(a[4], b[4])
    assert a[0].total == b[0].total
    assert a[0].logp == [] and not a[0].score
    # a redraw loop gave up (the same lines with and without scoring)
    assert any("failed" in x for x in b[2])
    got = np.asarray(b[0].logp, dtype=np.float64)
    assert got.shape == (len(b[1]),)
    assert np.array_equal(got, np.asarray(b[5]))
    assert (got <= 0).all() and (got < -0.1).any() and np.isfinite(got).all()
    if kind.endswith("+ban"):
        assert b[6] > 0
    if kind == "tp+ban":  # the score is taken at t = 1 over the whole distribution, whatever t and p
        c = _run(v, ctl, src, target, no_whole, rows, score=True, seeded=False, bans=bans)
        first = G.token_logprobs(rows[(0 * 101 + 1) % len(rows)], G.allowed_ids(v, **G.grammar_spec(v, 10)[0]))
        assert b[0].logp[0] == first[b[1][0]] and c[0].logp[0] == first[c[1][0]]


def test_rank_order_is_by_mean_logprob_with_ties_to_the_lower_index():
    lps = [np.array([-1.0, -1.0]), np.array([-0.5]), np.array([-1.0]), np.array([-0.25, -0.75])]
    assert G._rank_order(lps) == [1, 3, 0, 2]  # means -1, -.5, -1, -.5
    assert G._rank_order([np.array([-2.0])] * 3) == [0, 1, 2]
    # a long take is not punished for its length: the sum would order these the other way
    assert G._rank_order([np.array([-0.3]), np.full(10, -0.1)]) == [1, 0]

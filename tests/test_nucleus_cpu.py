"""Temperature and nucleus sampling on the host: `sampling(..., p, t)` draws
what the reference's own `sampling` drew (tests/golden/nucleus_draws.npz,
written by tests/golden/make_golden_nucleus.py), the public calls validate
`t` and `p` before anything is drawn, and `_Span` hands both to `sampling`."""
import os

import numpy as np
import pytest

from smer_music_generation_amd import generation as G
from smer_music_generation_amd.vocab import WordVocab

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_sampling_with_t_and_p_matches_reference_draws(golden_dir):
    z = np.load(os.path.join(golden_dir, "nucleus_draws.npz"))
    v = WordVocab(0, CTRL)
    rows, flags, names = z["rows"], z["flags"], [str(x) for x in z["flag_names"]]
    assert rows.dtype == np.float32 and rows.shape[1] == v.vocab_size and len(rows) <= 64
    assert set(z["t"].tolist()) == {0.5, 0.8, 1.0, 1.3}
    assert set(z["p"].tolist()) == {-1.0, 0.0, 0.5, 0.9, 0.999}
    np.random.seed(int(z["seed"]))
    got = []
    for i in range(len(rows)):
        fl = {n: True for n, on in zip(names, flags[i]) if on}
        p = None if z["p"][i] < 0 else float(z["p"][i])
        got.append(int(G.sampling(rows[i], v, p=p, t=float(z["t"][i]), **fl)))
    assert got == z["ids"].tolist()
    st = np.random.get_state()
    assert int(st[2]) == int(z["mt_pos"]) and np.array_equal(st[1], z["mt_key"])


def _request():
    from smer_music_generation_amd.synth import synth_events
    return list(synth_events(61, n_bars=6, n_tracks=3)), [1], [2, 3]


@pytest.mark.parametrize("kw", [dict(t=0), dict(t=-1), dict(t=float("nan")), dict(t=float("inf")),
                                dict(p=-0.1), dict(p=float("nan"))])
def test_bad_t_or_p_raises_before_anything_is_drawn(kw):
    """The model is never reached (None stands in for it): validation comes
    first, raises ValueError (generation_all prints and swallows every later
    error, as the reference does) and leaves np.random alone."""
    v = WordVocab(0, CTRL)
    ctl = v.density_indices + v.occupation_indices
    ev, tr, br = _request()
    np.random.seed(5)
    st0 = np.random.get_state()
    with pytest.raises(ValueError):
        G.generation_all(None, list(ev), "cpu", v, None, ctl, tr, br, **kw)
    with pytest.raises(ValueError):
        G.infill(None, list(ev), "cpu", v, None, ctl, tr, br, **kw)
    with pytest.raises(ValueError):
        G.generation_batch(None, [(list(ev), tr, br)] * 2, v, ctl, greedy=False, **kw)
    per_request = {k: [1.0 if k == "t" else None, x] for k, x in kw.items()}
    with pytest.raises(ValueError):
        G.generation_batch(None, [(list(ev), tr, br)] * 2, v, ctl, greedy=False, **per_request)
    assert _same_state(np.random.get_state(), st0)


def test_generation_batch_wants_one_t_and_p_per_request():
    v = WordVocab(0, CTRL)
    ev, tr, br = _request()
    with pytest.raises(ValueError):
        G.generation_batch(None, [(list(ev), tr, br)] * 2, v, v.density_indices, greedy=False,
                           t=[1.0, 0.8, 0.7])


@pytest.mark.parametrize("t,p", [(0.8, 0.9), (1.3, None), (0.5, 0.0), (1.0, 0.5)])
def test_span_draws_with_its_t_and_p(t, p):
    """_Span(t, p).advance over synthetic logit rows == a hand-written loop
    over sampling(row, v, p, t) + the redraw loop on the same seed."""
    v = WordVocab(0, CTRL)
    ctl = v.density_indices + v.occupation_indices
    ev, tr, br = _request()
    src, _, _, target, no_whole = G._prepare(list(ev), v, tr, br)
    rng = np.random.default_rng(9)
    rows = (rng.standard_normal((4000, v.vocab_size)) * 3.0).astype(np.float32)

    np.random.seed(123)
    sp = G._Span(v, src, target, ctl, no_whole, False, None, t, p)
    assert sp.n_masks > 0
    got = []
    while not sp.done:
        got.append(sp.advance(rows[len(got)]))
    st_got = np.random.get_state()

    np.random.seed(123)
    ref = G._Span(v, src, target, ctl, no_whole, False, None)  # state machine only: never draws
    want = []
    while not ref.done:
        flags, check, _ = ref.spec()
        row = rows[len(want)]
        idx = G.sampling(row, v, p, t, **flags)
        n = 0
        while check is not None and check(idx):
            idx = G.sampling(row, v, p, t, **flags)
            n += 1
            if n > 10:
                break
        want.append(ref.commit(idx))
    assert got == want and len(got) > 10
    assert _same_state(np.random.get_state(), st_got)
    assert sp.total == ref.total

"""The per-vocabulary tables of generation.py (`_VocabTables`): they die with
their vocabulary, and every vocabulary is served its own."""
import gc
import weakref

import numpy as np

from smer_music_generation_amd import generation as G
from smer_music_generation_amd.synth import synth_events
from smer_music_generation_amd.vocab import WordVocab


def _controls(v):
    return v.density_indices + v.occupation_indices + v.polyphony_indices + v.tensile_indices


def _touch_everything(v):
    """Every table of the vocabulary, through the public lookups."""
    ctl = _controls(v)
    for c in range(G.N_GRAMMAR_STATES):
        G.allowed_ids(v, **G.grammar_spec(v, c)[0])
    G.grammar_tables(v, ctl)
    G.reject_table(v)
    G.unit_table(v)
    G._pitch_mask(v)
    ev = list(synth_events(61, n_bars=7, n_tracks=3))
    assert G._request_bans(v, ev, [0], [2], {0: (30, 40)}) is not None
    sp = G._Span(v, *[G._prepare(list(ev), v, [0], [2])[k] for k in (0, 3)], ctl, False, True, None, bar_len=16)
    sp.governs()


def test_tables_do_not_outlive_their_vocabulary():
    v = WordVocab(0, ['key', 'tensile', 'density', 'polyphony', 'occupation'])
    _touch_everything(v)
    assert G._tables(v).owner() is v and len(G._tables(v)) > 15
    key, ref = id(v), weakref.ref(v)
    del v
    gc.collect()
    assert ref() is None
    assert key not in G._TABLES


def test_two_live_vocabularies_get_their_own_tables():
    a = WordVocab(0, ['key', 'tensile', 'density', 'polyphony', 'occupation'])
    b = WordVocab(0, ['occupation', 'polyphony', 'density', 'tensile', 'key'])
    b.pitch_indices = b.pitch_indices[:40]  # (so that the two differ in every table that knows a pitch)
    controls = {id(a): _controls(a), id(b): b.density_indices + b.occupation_indices}
    for v in (a, b, a, b):  # interleaved: the second pass reads what is cached
        _touch_everything(v)
        ctl = controls[id(v)]
        assert G._tables(v).owner() is v
        for c in range(G.N_GRAMMAR_STATES):
            flags, check, msg = G.grammar_spec(v, c)
            f2, c2, m2 = G._grammar_spec(v, c)
            assert flags == f2 and msg == m2 and (check is None) == (c2 is None)
            if check is not None:
                assert [bool(check(i)) for i in range(v.vocab_size)] == [bool(c2(i)) for i in range(v.vocab_size)]
            assert np.array_equal(G.allowed_ids(v, **flags), G._allowed_ids(v, flags.get))
        for got, want in zip(G.grammar_tables(v, ctl), G._grammar_tables(v, tuple(ctl))):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        assert G.grammar_tables(v, ctl[:3])[1].sum() != G.grammar_tables(v, ctl)[1].sum()  # per control set
        assert np.array_equal(G.reject_table(v), G._reject_rows(v))
        assert np.array_equal(G.unit_table(v), G._unit_row(v))
        assert np.array_equal(G._pitch_mask(v), G._pitch_row(v))
        assert int(G._pitch_mask(v).sum()) == len(v.pitch_indices)
        assert G._table(v, "midi", None) == {int(v.index2char(i)[2:]): i for i in v.pitch_indices}

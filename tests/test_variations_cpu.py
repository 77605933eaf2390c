"""`variations=` argument checks of generation_batch / generation_all: a bad
value raises ValueError before the model or np.random is touched (the calls
run with model=None)."""
import numpy as np
import pytest

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']
BAD = [0, -1, 1.5, "2", [1, 2], [1, 0, 1]]


def _requests():
    from smer_music_generation_amd.synth import synth_events
    return [(synth_events(60 + i, n_bars=6 + i, n_tracks=3), [i % 3], [4]) for i in range(3)]


def _state():
    st = np.random.get_state()
    return st[1].copy(), int(st[2])


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_generation_batch_rejects_bad_variations(bad):
    from smer_music_generation_amd.generation import generation_batch
    from smer_music_generation_amd.vocab import WordVocab
    v = WordVocab(0, CTRL)
    np.random.seed(5)
    before = _state()
    with pytest.raises(ValueError):
        generation_batch(None, _requests(), v, [], greedy=False, variations=bad)
    after = _state()
    assert before[1] == after[1] and np.array_equal(before[0], after[0])


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_generation_all_rejects_bad_variations(bad):
    from smer_music_generation_amd.generation import generation_all, infill
    from smer_music_generation_amd.vocab import WordVocab
    v = WordVocab(0, CTRL)
    ev, tr, br = _requests()[0]
    np.random.seed(6)
    before = _state()
    for fn in (generation_all, infill):
        with pytest.raises(ValueError):
            fn(None, ev, "cpu", v, None, [], tr, br, variations=bad)
    after = _state()
    assert before[1] == after[1] and np.array_equal(before[0], after[0])


def test_good_variations_pass_the_check():
    from smer_music_generation_amd.generation import _check_variations
    assert _check_variations(2, 3) == [2, 2, 2]
    assert _check_variations([3, 1, 2], 3) == [3, 1, 2]
    assert _check_variations(np.int64(4)) == 4

"""The host infill paths give what they gave when tests/golden/
generation_pinned.npz was recorded (tests/golden/make_golden_generation_
pinned.py lists the cases: draw mode x constraints x call path): tokens,
steps, log-probabilities bit for bit, order, bar_fill, redraw log lines and
np.random's state afterwards, all compared for equality."""
import os

import numpy as np

from tests.golden.make_golden_generation_pinned import CONSTRAINTS, MODES, NAME, run_cases
from tests.test_template_cpu import host  # noqa: F401


def test_redraw_loop_keeps_the_twelfth_id_unchecked_and_logs(host, monkeypatch):  # noqa: F811
    """The reference's redraw loop (the pinned cases never exhaust it): a draw
    and up to 11 redraws while the state's check rejects; once 11 ids were
    rejected the 12th stands unchecked and the failure is logged, whether or
    not it would have passed."""
    from smer_music_generation_amd import generation as G
    from tests.test_template_cpu import BARS, TRACKS, _Log
    _, v, ctl, ev, _ = host
    src, _, _, target, no_whole = G._prepare(list(ev), v, TRACKS, BARS)
    bad, good = v.duration_only_indices[1], v.pitch_indices[3]  # state 10 (a note span's first token) rejects a duration
    for n_bad, want_log in ((10, []), (11, ['start failed']), (12, ['start failed'])):
        ids = [bad] * n_bad + [good] * 3
        calls = []
        monkeypatch.setattr(G, "sampling", lambda *a, **k: (calls.append(1), ids[len(calls) - 1])[1])
        lg = _Log()
        sp = G._Span(v, src, target, ctl, no_whole, False, lg)
        got = sp.advance(np.zeros(v.vocab_size, dtype=np.float32))
        assert (got, len(calls), lg.lines) == (ids[min(n_bad, 11)], min(n_bad, 11) + 1, want_log)


def test_plugin_call_keeps_its_order_around_a_request_that_cannot_be_prepared(host, capsys):  # noqa: F811
    """Track 9 does not exist, so `_prepare` fails.  Without a template the
    stats and the use_kv_cache check come first; with one the request is
    prepared first (printed, None)."""
    import pytest
    from smer_music_generation_amd import generation as G
    m, v, ctl, ev, _ = host
    call = lambda **kw: G.generation_all(m, list(ev), "cpu", v, None, ctl, [9], [2], **kw)  # noqa: E731
    with pytest.raises(ValueError, match="variations needs the KV-cached path"):
        call(variations=2, use_kv_cache=False)
    stats = {}
    assert call(seed=4, stats=stats) is None and stats == {"seeds": [4], "pitches": None}
    stats = {}
    assert call(variations=2, use_kv_cache=False, template=[None], stats=stats) is None and stats == {}
    assert capsys.readouterr().out.count("is not in list") == 2


def test_host_paths_replay_the_pinned_cases(host, golden_dir):  # noqa: F811
    m, v, ctl, ev, _ = host
    z = np.load(os.path.join(golden_dir, NAME))
    got = run_cases(m, v, ctl, ev)
    assert sorted(got) == sorted(z.files)
    paths = ("all", "score(all)", "batch", "score(batch)")
    assert {k.split("/")[0] for k in got} == {"%s|%s|%s" % (a, b, c) for a in MODES for b in CONSTRAINTS
                                              for c in paths}
    for key in z.files:
        want, have = z[key], np.asarray(got[key])
        assert have.dtype == want.dtype and have.shape == want.shape, key
        assert np.array_equal(have, want), key
    # the fixture is no row of zeros: scores were taken, spans were clocked, takes were ranked
    assert any(k.endswith("/logprobs_bits") and len(z[k]) > 30 for k in z.files)
    assert any(k.endswith("/bar_fill") and len(z[k]) for k in z.files)
    assert z["seeded|variations+rank|batch/order"].shape == (3, 3)
    assert z["greedy|variations+rank|all/no_kv_cache"].item().startswith("ValueError: variations needs")

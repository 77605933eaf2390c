"""Generate tests/golden/generation_pinned.npz: what the host infill paths of
`smer_music_generation_amd.generation` give, case by case, on the project's
own synthetic events and the stand-in model of tests/test_template_cpu.py
(logits by decoder row, no GPU).  tests/test_generation_pinned_cpu.py replays
the cases and compares every array for equality, so the file pins the host
path across a refactor: RUN IT ON THE COMMIT WHOSE BEHAVIOUR IS TO BE KEPT.

    python tests/golden/make_golden_generation_pinned.py

The cases are the product of
  draw mode    greedy; unseeded sampled (np.random seeded before the call);
               seeded with t = 0.8, p = 0.9
  constraints  none; pitches; template = rhythm_template(..); fill_bar; all
               three with logprobs=True; variations=3 with rank=True
  call path    generation_all(use_kv_cache=False); generation_batch(
               device_grammar=False) with 3 requests; score_batch(
               device_score=False) on each take of the two
(variations needs the KV-cached path: that cell records the ValueError of
use_kv_cache=False and the takes of the KV-cached host loop.)  Recorded per
case: the restored tokens, stats['generated'], steps, the log-probabilities
as float64 bit patterns, order, bar_fill, seeds, the redraw log lines and
np.random's state afterwards.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from smer_music_generation_amd import generation as G  # noqa: E402
from smer_music_generation_amd.synth import synth_events  # noqa: E402

NAME = "generation_pinned.npz"
NP_SEED = 1234
OCTAVE = tuple(range(60, 72))
MODES = {"greedy": dict(greedy=True), "unseeded": dict(greedy=False),
         "seeded": dict(greedy=False, seed=11, t=0.8, p=0.9)}
CONSTRAINTS = ("none", "pitches", "template", "fill_bar", "all+logprobs", "variations+rank")
BATCH_SEEDS = [11, 21, 31]
BATCH_FILL = [True, False, True]  # (one request of the batch runs without its clock)


def requests(ev):
    """The three requests of the batched path; the first is generation_all's."""
    return [(ev, [0, 2], [2]), (ev, [1], [3]), (list(synth_events(62, n_bars=7, n_tracks=3)), [0, 2], [1])]


class Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _ragged(seqs, dtype):
    """A list of sequences (None allowed) as (concatenation, lengths; -1: None)."""
    lens = np.array([-1 if s is None else len(s) for s in seqs], dtype=np.int64)
    flat = [np.asarray(s, dtype=dtype).reshape(len(s), -1) for s in seqs if s is not None and len(s)]
    return (np.concatenate(flat) if flat else np.zeros((0, 1), dtype=dtype)), lens


def _state(out, key):
    """np.random's state after a call that began at np.random.seed(NP_SEED):
    whether it is still that state, and the state itself where it moved."""
    st = np.random.get_state()
    np.random.seed(NP_SEED)
    s0 = np.random.get_state()
    np.random.set_state(st)
    moved = not (np.array_equal(st[1], s0[1]) and st[2:] == s0[2:])
    out[key + "/mt_moved"] = np.bool_(moved)
    if moved:
        out[key + "/mt_key"] = np.asarray(st[1], dtype=np.uint32)
        out[key + "/mt_rest"] = np.array([st[2], st[3]], dtype=np.int64)
        out[key + "/mt_gauss_bits"] = np.array([st[4]], dtype=np.float64).view(np.uint64)


def _put_stats(out, key, stats, lines):
    out[key + "/steps"] = np.int64(stats["steps"])
    out[key + "/log_lines"] = np.array(lines, dtype=str)
    out[key + "/seeds"] = np.array([-1] if stats["seeds"] is None else stats["seeds"], dtype=np.int64)
    if "tokens" in stats:
        out[key + "/tokens_drawn"] = np.int64(stats["tokens"])
    if "generated" in stats:
        out[key + "/generated"], out[key + "/generated_len"] = _ragged(stats["generated"], "<U9")
    if "logprobs" in stats:
        lp, out[key + "/logprobs_len"] = _ragged(stats["logprobs"], np.float64)
        out[key + "/logprobs_bits"] = lp.view(np.uint64)
        out[key + "/scores_bits"] = np.asarray(stats["scores"], dtype=np.float64).view(np.uint64)
    if "order" in stats:
        order = stats["order"]
        out[key + "/order"] = np.asarray(order, dtype=np.int64)
    if "bar_fill" in stats:
        out[key + "/bar_fill"], out[key + "/bar_fill_len"] = _ragged(stats["bar_fill"], np.int64)


def _put_takes(out, key, takes):
    """takes: (restored, mask_track_names, mask_bar_names) or None, one per take."""
    out[key + "/restored"], out[key + "/restored_len"] = _ragged(
        [None if x is None else x[0] for x in takes], "<U9")
    out[key + "/mask_names"] = np.array(
        ["" if x is None else repr((list(map(str, x[1])), list(map(str, x[2])))) for x in takes], dtype=str)


def _put_scores(out, key, m, v, ctl, takes, reqs, pitches):
    """score_batch(device_score=False) over every take: the restored tokens
    are the events, so the scored content is the take's own."""
    live = [(x, q) for x, q in zip(takes, reqs) if x is not None]
    np.random.seed(NP_SEED)
    try:
        res = G.score_batch(m, [(list(x[0]), q[1], q[2]) for x, q in live], v, ctl, pitches=pitches,
                            device_score=False)
    except ValueError as e:
        out[key + "/error"] = np.array("ValueError: %s" % e)
        return
    lp, out[key + "/logprobs_len"] = _ragged([r.logprobs for r in res], np.float64)
    out[key + "/logprobs_bits"] = lp.view(np.uint64)
    out[key + "/score_bits"] = np.array([r.score for r in res], dtype=np.float64).view(np.uint64)
    out[key + "/tokens"] = _ragged([r.tokens for r in res], np.int64)[0]
    out[key + "/mask_index"] = _ragged([r.mask_index for r in res], np.int64)[0]
    out[key + "/greedy"] = _ragged([r.greedy for r in res], np.int64)[0]
    _state(out, key)


def _constraint_kw(name, v, reqs, batch):
    """The keywords of a constraint: for generation_all (the first request) or
    for the batch."""
    n = len(reqs)
    tpl = [G.rhythm_template(ev, v, tr, br) for ev, tr, br in reqs]
    kw = {}
    if name in ("pitches", "all+logprobs"):
        kw["pitches"] = OCTAVE
    if name in ("template", "all+logprobs"):
        kw["template"] = tpl[:n] if batch else tpl[0]
    if name in ("fill_bar", "all+logprobs"):
        kw["fill_bar"] = BATCH_FILL[:n] if batch else True
    if name == "all+logprobs":
        kw["logprobs"] = True
    if name == "variations+rank":
        kw.update(variations=3, rank=True)
    return kw


def run_cases(m, v, ctl, ev):
    """Every case, as one flat {key: array} dict.  The caller has routed
    G._batch_session to the stand-in session (tests/test_template_cpu.py)."""
    out = {}
    reqs = requests(ev)
    for mode, mkw in MODES.items():
        for cons in CONSTRAINTS:
            base = "%s|%s" % (mode, cons)
            # generation_all(use_kv_cache=False)
            key = base + "|all"
            kw = dict(mkw, **_constraint_kw(cons, v, reqs[:1], False))
            e0, tr0, br0 = reqs[0]
            path_kw = dict(use_kv_cache=False)
            if cons == "variations+rank":
                np.random.seed(NP_SEED)
                try:
                    G.generation_all(m, list(e0), "cpu", v, None, ctl, tr0, br0, use_kv_cache=False, **kw)
                    out[key + "/no_kv_cache"] = np.array("returned")
                except ValueError as e:
                    out[key + "/no_kv_cache"] = np.array("ValueError: %s" % e)
                path_kw = dict(use_kv_cache=True, device_grammar=False)
            lg, stats = Log(), {}
            np.random.seed(NP_SEED)
            res = G.generation_all(m, list(e0), "cpu", v, lg, ctl, tr0, br0, stats=stats, **path_kw, **kw)
            assert res is not None, key
            takes = list(res) if cons == "variations+rank" else [res]
            _state(out, key)
            _put_stats(out, key, stats, lg.lines)
            _put_takes(out, key, takes)
            _put_scores(out, base + "|score(all)", m, v, ctl, takes, [reqs[0]] * len(takes), kw.get("pitches"))
            # generation_batch(device_grammar=False), 3 requests
            key = base + "|batch"
            kw = dict(mkw, **_constraint_kw(cons, v, reqs, True))
            if "seed" in kw:
                kw["seed"] = BATCH_SEEDS
            lg = Log()
            np.random.seed(NP_SEED)
            res, stats = G.generation_batch(m, [(list(e), tr, br) for e, tr, br in reqs], v, ctl, logger=lg,
                                            precision="fp32", device_grammar=False, return_stats=True, **kw)
            _state(out, key)
            _put_stats(out, key, stats, lg.lines)
            if cons == "variations+rank":
                takes = [x for r in res for x in r]
                of = [q for q in reqs for _ in range(3)]
            else:
                takes, of = list(res), reqs
            assert all(x is not None for x in takes), key
            _put_takes(out, key, takes)
            _put_scores(out, base + "|score(batch)", m, v, ctl, takes, of, kw.get("pitches"))
    return out


def main():
    import torch
    from tests.test_template_cpu import _events, _Model, _Session, _table, _vocab
    v, ctl = _vocab()
    rows = _table(v, ctl)
    G._batch_session = lambda *a, **k: _Session(rows)
    torch.cuda.synchronize = lambda *a, **k: None
    out = run_cases(_Model(rows), v, ctl, _events())
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (NAME, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()

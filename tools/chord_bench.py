"""Chord-following infill on the device decode path:
the replayed step of the '+bar+chord' graphs (smer_chord_ban between the bar
clock and the template kernel) against the step of the '+bar' graphs.

    python tools/chord_bench.py [greedy|stream|rows] ...   # C2 request set, 32 requests, bf16; default: all three
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from smer_music_generation_amd import generation  # noqa: E402
from tools.barclock_bench import _ZeroBars, setup  # noqa: E402


class _FreeChords:
    """The '+bar+chord' graph with every chord table free (chord_len 0, no row):
    the node runs, no row is active -- the tokens and the steps of the '+bar'
    leg with bar_len 0, so the two loops differ by the node alone.  (The public
    keyword cannot say this: a call without chords= takes the graphs without
    the node.)"""

    def __enter__(self):
        self.real = generation._device_chords
        generation._device_chords = lambda spans: [None] * len(spans)
        return self

    def __exit__(self, *exc):
        generation._device_chords = self.real
        return False


def progression(reqs):
    """F major for two beats, then C7, on every bar of every request."""
    prog = [(0, generation.pitch_set(classes=generation.chord_tones(5, 'maj'))),
            (8, generation.pitch_set(classes=generation.chord_tones(0, '7')))]
    return [{int(b): prog for b in br} for _, _, br in reqs]


def batch(m, v, ac, reqs, mode, rounds=5):
    """generation_batch on bench.py's C2 infill request set (32 requests,
    bf16, warm session), the three legs interleaved over `rounds` rounds: ms
    per replayed step (the replay loop's wall time over its steps), median and
    range.  'bar0': the '+bar' graph, every bar length 0; 'free': the
    '+bar+chord' graph on all-free tables; 'prog': a real progression, which
    emits other tokens than the other two."""
    n = len(reqs)
    kw0 = {"greedy": dict(greedy=True), "stream": dict(greedy=False),
           "rows": dict(greedy=False, seed=[1000 * (i + 1) for i in range(n)])}[mode]
    chords = progression(reqs)

    def leg(name):
        np.random.seed(0)
        torch.cuda.synchronize()
        if name == "prog":
            _, st = generation.generation_batch(m, reqs, v, ac, return_stats=True, chords=chords, **kw0)
        else:
            with _ZeroBars():
                if name == "free":
                    with _FreeChords():
                        _, st = generation.generation_batch(m, reqs, v, ac, return_stats=True, **kw0)
                else:
                    _, st = generation.generation_batch(m, reqs, v, ac, return_stats=True, **kw0)
        torch.cuda.synchronize()
        return st
    legs = ("bar0", "free", "prog")
    for name in legs:  # warm: session, both captured graphs
        leg(name)
    res, toks = {}, {}
    for _ in range(rounds):
        for name in legs:
            st = leg(name)
            toks.setdefault(name, []).append((st["generated"], st["steps"]))
            res.setdefault(name, []).append(
                {"tokens": st["tokens"], "steps": st["steps"],
                 "loop_ms_per_step": round(1000 * st["decode_phases_s"]["loop_s"] / max(1, st["steps"]), 5)})
    assert toks["bar0"] == toks["free"], "the all-free leg must draw the bar_len = 0 leg's tokens in its steps"
    ms = {k: [r["loop_ms_per_step"] for r in x] for k, x in res.items()}
    med = {k: float(np.median(x)) for k, x in ms.items()}
    print(json.dumps({"mode": mode, "requests": n, "median_loop_ms_per_step": med,
                      "range_loop_ms_per_step": {k: [min(x), max(x)] for k, x in ms.items()},
                      "free_leg_has_the_bar0_tokens": True,
                      "delta_us": {k: round(1000 * (med[k] - med["bar0"]), 3) for k in ("free", "prog")},
                      "result": res}), flush=True)


def main(modes):
    args, v, ac, reqs = setup()
    m = bench.make_model(args, torch.device("cuda:0"), "bf16").eval()
    # a randomly initialised model draws 'm_0' inside some span, which the
    # final splice rejects (the reference's IndexError): not what is timed
    splice = generation.restore_marked_input

    def lenient(src, gen):
        try:
            return splice(src, gen)
        except IndexError:
            return None
    generation.restore_marked_input = lenient
    for mode in modes:
        batch(m, v, ac, reqs, mode)


if __name__ == "__main__":
    main(sys.argv[1:] or ["greedy", "stream", "rows"])

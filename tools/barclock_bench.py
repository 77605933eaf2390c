"""The bar clock on the device decode path: the
replayed step of the '+bar' graphs (smer_bar_clock between the vocabulary
projection and the grammar kernel) against the step without that node (the
parent commit's graphs).

    python tools/barclock_bench.py [greedy|stream|rows] ...   # C2 request set, 32 requests, bf16; default: all three
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from smer_music_generation_amd import generation  # noqa: E402


def setup():
    from smer_music_generation_amd.vocab import WordVocab
    args = bench.parse_args([])
    v = WordVocab(0, bench.CTRL)
    ac = v.density_indices + v.occupation_indices + v.polyphony_indices + v.tensile_indices
    reqs = bench._infill_requests(args.infill_batch, args.seq, 0)
    return args, v, ac, reqs


class _ZeroBars:
    """The '+bar' graph with every bar length 0: the node runs and follows the
    tokens, but no row is active -- the tokens and the steps of the plain leg,
    so the two loops differ by the node alone.  (The public keyword cannot say
    this: a call in which no request sets fill_bar takes the plain graphs.)"""

    def __enter__(self):
        self.real = generation._device_bars
        generation._device_bars = lambda spans: [0] * len(spans)
        return self

    def __exit__(self, *exc):
        generation._device_bars = self.real
        return False


def batch(m, v, ac, reqs, mode, rounds=5):
    """generation_batch on bench.py's C2 infill request set (32 requests,
    bf16, warm session), the three legs interleaved over `rounds` rounds: ms
    per replayed step (the replay loop's wall time over its steps), median and
    range.  The 'on' leg emits other tokens than the other two: its loop is as
    long as the bars it fills."""
    n = len(reqs)
    kw0 = {"greedy": dict(greedy=True), "stream": dict(greedy=False),
           "rows": dict(greedy=False, seed=[1000 * (i + 1) for i in range(n)])}[mode]

    def leg(name):
        np.random.seed(0)
        torch.cuda.synchronize()
        if name == "zero":
            with _ZeroBars():
                _, st = generation.generation_batch(m, reqs, v, ac, return_stats=True, **kw0)
        else:
            _, st = generation.generation_batch(m, reqs, v, ac, return_stats=True, fill_bar=name == "on", **kw0)
        torch.cuda.synchronize()
        return st
    legs = ("plain", "zero", "on")
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
    assert toks["plain"] == toks["zero"], "the bar_len = 0 leg must draw the plain leg's tokens in its steps"
    ms = {k: [r["loop_ms_per_step"] for r in x] for k, x in res.items()}
    med = {k: float(np.median(x)) for k, x in ms.items()}
    print(json.dumps({"mode": mode, "requests": n, "median_loop_ms_per_step": med,
                      "range_loop_ms_per_step": {k: [min(x), max(x)] for k, x in ms.items()},
                      "zero_leg_has_the_plain_tokens": True,
                      "delta_us": {k: round(1000 * (med[k] - med["plain"]), 3) for k in ("zero", "on")},
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

"""Pitch constraints on the device decode path: the
replayed step of the '+ban' graphs (smer_logits_ban between the vocabulary
projection and the grammar kernel) against the unconstrained step (the graphs
without that node: the parent commit's step).

    python tools/pitch_constraint_bench.py batch [greedy|stream|rows]  # C2 request set, 32 requests, bf16
    python tools/pitch_constraint_bench.py kernel                      # smer_logits_ban alone, R = 32
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from smer_music_generation_amd import generation  # noqa: E402


def batch(mode="greedy", rounds=5):
    """generation_batch on bench.py's C2 infill request set (32 requests,
    bf16, warm session), unconstrained, with every request "constrained" to
    all 88 pitches and with every request constrained to one octave, the legs
    interleaved: ms per replayed step (the replay loop's wall time over its
    steps).  The one-octave decode emits other tokens: with a randomly
    initialised model most spans then end at once, and a loop of a dozen
    steps shows its start and drain (the host polls 3 steps behind), not the
    step; the all-pitches leg has the unconstrained leg's steps."""
    from smer_music_generation_amd.vocab import WordVocab
    args = bench.parse_args([])
    dev = torch.device("cuda:0")
    v = WordVocab(0, bench.CTRL)
    m = bench.make_model(args, dev, "bf16").eval()
    ac = v.density_indices + v.occupation_indices + v.polyphony_indices + v.tensile_indices
    reqs = bench._infill_requests(args.infill_batch, args.seq, 0)
    # a randomly initialised model draws 'm_0' inside some span, which the
    # final splice rejects (the reference's IndexError): not what is timed
    splice = generation.restore_marked_input

    def lenient(src, gen):
        try:
            return splice(src, gen)
        except IndexError:
            return None
    generation.restore_marked_input = lenient
    n = len(reqs)
    kw0 = {"greedy": dict(greedy=True), "stream": dict(greedy=False),
           "rows": dict(greedy=False, seed=[1000 * (i + 1) for i in range(n)])}[mode]
    # all_pitches: the '+ban' graph with nothing banned -- the tokens and the
    # step count of the unconstrained leg, so the two differ by the node alone
    legs = (("unconstrained", {}), ("all_pitches", dict(pitches=generation.pitch_set())),
            ("one_octave", dict(pitches=generation.pitch_set(60, 71))))
    for _, kw in legs:  # warm: session, both captured graphs
        np.random.seed(1)
        generation.generation_batch(m, reqs, v, ac, **kw0, **kw)
    res = {}
    for _ in range(rounds):
        for name, kw in legs:
            np.random.seed(0)
            torch.cuda.synchronize()
            _, st = generation.generation_batch(m, reqs, v, ac, return_stats=True, **kw0, **kw)
            torch.cuda.synchronize()
            res.setdefault(name, []).append(
                {"tokens": st["tokens"], "steps": st["steps"],
                 "loop_ms_per_step": round(1000 * st["decode_phases_s"]["loop_s"] / max(1, st["steps"]), 5)})
    med = {k: float(np.median([r["loop_ms_per_step"] for r in x])) for k, x in res.items()}
    print(json.dumps({"mode": mode, "requests": n, "median_loop_ms_per_step": med,
                      "delta_us": {k: round(1000 * (med[k] - med["unconstrained"]), 3)
                                   for k in ("all_pitches", "one_octave")}, "result": res}))


def kernel(calls=400, R=32):
    """smer_logits_ban alone at the C2 vocabulary, R live requests each
    banning every pitch outside one octave: back-to-back launches between two
    events (launch-bound: the kernel moves 64 B of bits and stores <= 76
    floats per request)."""
    from smer_music_generation_amd import ops as O
    from smer_music_generation_amd.vocab import WordVocab
    dev = torch.device("cuda:0")
    v = WordVocab(0, bench.CTRL)
    V = v.vocab_size
    ban = np.zeros((1, V), dtype=bool)
    ban[0, v.pitch_indices] = True
    ban[0, [v.char2index('p_%d' % k) for k in range(60, 72)]] = False
    bits = torch.from_numpy(np.tile(generation.ban_bits(ban).view(np.int32), (R, 4, 1))).to(dev)
    of_mask = torch.zeros(R, 16, dtype=torch.int8, device=dev)
    state = torch.tensor([[0, 4, 5, 0, 1, 0, 0, 0, 0, 0, 0, 0]] * R, dtype=torch.int32, device=dev)
    torch.manual_seed(0)
    logits = torch.randn(2 * R, V, device=dev) * 3
    res = []
    for _ in range(5):
        for _ in range(20):
            O.logits_ban(logits, state, of_mask, bits)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            O.logits_ban(logits, state, of_mask, bits)
        e1.record()
        torch.cuda.synchronize()
        res.append(round(e0.elapsed_time(e1) * 1000.0 / calls, 3))
    print(json.dumps({"R": R, "us_per_call_back_to_back": res}))


if __name__ == "__main__":
    if sys.argv[1] == "batch":
        batch(*sys.argv[2:3])
    else:
        kernel()

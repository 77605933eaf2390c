"""Take scores on the device decode path: the replayed
step of the '+score' graphs (smer_logprob_stage before the grammar kernel,
smer_logprob_commit after it) against the unscored step (the graphs without
those nodes: the parent commit's step), in one process, legs interleaved.

    python tools/logprob_bench.py batch [greedy|stream|rows]  # C2 request set, 32 requests, bf16
    python tools/logprob_bench.py kernel                      # the two kernels alone, R = 32
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
    bf16, warm session) without and with logprobs=True: the same tokens and
    steps, so the two legs differ by the two nodes alone.  ms per replayed
    step: the replay loop's wall time over its steps."""
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
    legs = (("unscored", {}), ("scored", dict(logprobs=True)))
    for _, kw in legs:  # warm: session, both captured graphs
        np.random.seed(1)
        generation.generation_batch(m, reqs, v, ac, **kw0, **kw)
    res, gen = {}, {}
    for _ in range(rounds):
        for name, kw in legs:
            np.random.seed(0)
            torch.cuda.synchronize()
            _, st = generation.generation_batch(m, reqs, v, ac, return_stats=True, **kw0, **kw)
            torch.cuda.synchronize()
            gen[name] = st["generated"]
            res.setdefault(name, []).append(
                {"tokens": st["tokens"], "steps": st["steps"],
                 "loop_ms_per_step": round(1000 * st["decode_phases_s"]["loop_s"] / max(1, st["steps"]), 5)})
            if name == "scored":
                assert sum(len(a) for a in st["logprobs"]) == st["tokens"]
    assert gen["scored"] == gen["unscored"], "a scored call emits the unscored call's tokens"
    med = {k: float(np.median([r["loop_ms_per_step"] for r in x])) for k, x in res.items()}
    print(json.dumps({"mode": mode, "requests": n, "median_loop_ms_per_step": med,
                      "delta_us": round(1000 * (med["scored"] - med["unscored"]), 3),
                      "ratio": round(med["scored"] / med["unscored"], 5), "result": res}))


def kernel(calls=400, R=32):
    """smer_logprob_stage and smer_logprob_commit alone at the C2 vocabulary,
    R live requests: back-to-back launches between two events (stage: 309
    float64 exp and one log per request; commit: one load and one store)."""
    from smer_music_generation_amd import ops as O
    from smer_music_generation_amd.vocab import WordVocab
    dev = torch.device("cuda:0")
    v = WordVocab(0, bench.CTRL)
    V = v.vocab_size
    keep, _ = generation.grammar_tables(v, v.density_indices + v.occupation_indices)
    keep = torch.from_numpy(keep).to(dev)
    targets = torch.zeros(R, 16, dtype=torch.int8, device=dev)
    state = torch.tensor([[0, 4, 5, 0, 1, 0, 0, 0, 0, 0, 0, 0]] * R, dtype=torch.int32, device=dev)
    after = state.clone()
    after[:, 7] = 1
    torch.manual_seed(0)
    logits = torch.randn(2 * R, V, device=dev) * 3
    scratch = torch.zeros(R, 512, dtype=torch.float64, device=dev)
    stage = torch.zeros(R, dtype=torch.int32, device=dev)
    out_tok = torch.randint(0, V, (R, 128), dtype=torch.int32, device=dev)
    out_lp = torch.zeros(R, 128, dtype=torch.float64, device=dev)
    fns = {"stage": lambda: O.logprob_stage(logits, state, targets, keep, scratch, stage),
           "commit": lambda: O.logprob_commit(after, stage, out_tok, scratch, out_lp, V=V)}
    res = {}
    for name, fn in fns.items():
        for _ in range(5):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(name, []).append(round(e0.elapsed_time(e1) * 1000.0 / calls, 3))
    print(json.dumps({"R": R, "us_per_call_back_to_back": res}))


if __name__ == "__main__":
    if sys.argv[1] == "batch":
        batch(*sys.argv[2:3])
    else:
        kernel()

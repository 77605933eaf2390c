"""Per-request seeds on the device decode path: the
seeded sampler (one block per request) against the unseeded one (one wave
walks the requests on the shared stream: the parent commit's sampler).

    python tools/seeded_sampling_bench.py batch       # generation_batch(greedy=False), 32 requests
    python tools/seeded_sampling_bench.py variations  # 4 sources x 8 takes
    python tools/seeded_sampling_bench.py kernel      # the two sampler kernels alone, R = 1 and 32
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from smer_music_generation_amd import generation  # noqa: E402


def _legs(reqs, rounds, variations=None):
    """generation_batch(greedy=False) on the C2 model, bf16, warm session,
    unseeded and seeded runs interleaved."""
    from smer_music_generation_amd.vocab import WordVocab
    args = bench.parse_args([])
    dev = torch.device("cuda:0")
    v = WordVocab(0, bench.CTRL)
    m = bench.make_model(args, dev, "bf16").eval()
    ac = v.density_indices + v.occupation_indices + v.polyphony_indices + v.tensile_indices
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
    legs = (("unseeded", {}), ("seeded", dict(seed=[1000 * (i + 1) for i in range(n)])))
    kw0 = {} if variations is None else dict(variations=variations)
    for _, kw in legs:  # warm: session, both captured graphs
        np.random.seed(1)
        generation.generation_batch(m, reqs, v, ac, greedy=False, **kw0, **kw)
    res = {}
    for _ in range(rounds):
        for name, kw in legs:
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, st = generation.generation_batch(m, reqs, v, ac, greedy=False, return_stats=True, **kw0, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res.setdefault(name, []).append(
                {"tokens": st["tokens"], "steps": st["steps"], "tokens_per_s": round(st["tokens"] / dt, 1),
                 "ms_per_step": round(1000 * st["step_call_s"] / max(1, st["steps"]), 4),
                 "loop_ms_per_step": round(1000 * st["decode_phases_s"]["loop_s"] / max(1, st["steps"]), 4)})
    return res


def batch(rounds=3):
    """(a) / (b): bench.py's C2 infill request set (32 requests)."""
    args = bench.parse_args([])
    reqs = bench._infill_requests(args.infill_batch, args.seq, 0)
    print(json.dumps({"requests": len(reqs), "result": _legs(reqs, rounds)}))


def variations(rounds=3, sources=4, takes=8):
    """(c): the first `sources` requests of that set, `takes` takes each."""
    args = bench.parse_args([])
    reqs = bench._infill_requests(args.infill_batch, args.seq, 0)[:sources]
    print(json.dumps({"sources": sources, "takes": takes, "result": _legs(reqs, rounds, takes)}))


def kernel(calls=200):
    """(d): R live requests at the C2 vocabulary, random rows, (t, p) = (1,
    None) through tp: smer_grammar_sample_step_tp (one wave, the requests in
    turn) against smer_grammar_sample_step_rows (one block per request)."""
    from smer_music_generation_amd import ops as O
    from smer_music_generation_amd.generation import grammar_tables, reject_table
    from smer_music_generation_amd.vocab import WordVocab
    dev = torch.device("cuda:0")
    v = WordVocab(0, bench.CTRL)
    V = v.vocab_size
    keep, cls = grammar_tables(v, v.density_indices)
    kt, rt, ct = (torch.from_numpy(x).to(dev) for x in (keep, reject_table(v), cls))
    kw = dict(eos=v.eos_index, m0=v.char2index('m_0'), trash_pos=200)
    res = {}
    for R in (1, 32):
        s0 = np.random.RandomState(0).get_state()
        row = np.concatenate([s0[1], [s0[2]]]).astype(np.uint32).view(np.int32)
        mt1 = torch.from_numpy(row).to(dev)
        mtr = torch.from_numpy(np.tile(row, (R, 1))).to(dev)
        state0 = torch.tensor([[0, 4, 5, 0, 1, 0, 0, 0, 0, 0, 0, 0]] * R, dtype=torch.int32, device=dev)
        state = state0.clone()
        torch.manual_seed(0)
        head = [torch.randn(2 * R, V, device=dev) * 3, state, torch.zeros(R, 16, dtype=torch.int8, device=dev),
                kt, rt, ct, torch.ones(R, dtype=torch.int32, device=dev),
                torch.zeros(2 * R, dtype=torch.int64, device=dev),
                torch.zeros(4, 2 * R, dtype=torch.int32, device=dev),
                torch.zeros(R, 4, dtype=torch.int32, device=dev)]
        ctl = torch.zeros(3, dtype=torch.int32, device=dev)
        ring = torch.zeros(8, dtype=torch.int32).pin_memory()
        tp = torch.tensor([[1.0, -1.0]] * R, dtype=torch.float64, device=dev)
        for _ in range(3):
            for name, fn, mt in (("serial", O.grammar_sample_step, mt1), ("rows", O.grammar_sample_step_rows, mtr)):
                def run(n):
                    for _ in range(n):
                        state.copy_(state0)  # the requests stay live
                        fn(*head, mt, ctl, ring=ring, tp=tp, **kw)
                run(10)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(calls)
                e1.record()
                torch.cuda.synchronize()
                res.setdefault("R%d_%s" % (R, name), []).append(round(e0.elapsed_time(e1) * 1000.0 / calls, 2))
    print(json.dumps({"us_per_call_incl_state_reset": res}))


if __name__ == "__main__":
    {"batch": batch, "variations": variations, "kernel": kernel}[sys.argv[1]]()

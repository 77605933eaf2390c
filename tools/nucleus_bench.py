"""Cost of temperature / nucleus sampling on the device decode path
(DESIGN.md section 5).

    python tools/nucleus_bench.py plugin   # bench.py's batch-1 plugin line, default vs t=0.8 p=0.9
    python tools/nucleus_bench.py kernel   # the sampler kernel alone, us per call
    python tools/nucleus_bench.py batch    # generation_batch(greedy=False): device sampler vs host loop
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


def plugin(rounds=3):
    """bench.bench_infill_batch1 with the plugin call's (t, p) overridden,
    the settings interleaved."""
    args = bench.parse_args([])
    dev = torch.device("cuda:0")
    orig = generation.generation_all
    res = {}
    for _ in range(rounds):
        for name, kw in (("default", {}), ("t0.8_p0.9", dict(t=0.8, p=0.9))):
            generation.generation_all = lambda *a, _kw=kw, **k: orig(*a, **dict(k, **_kw))
            r = bench.bench_infill_batch1(args, dev, 0)
            res.setdefault(name, []).append({k: r[k] for k in ("value", "ms_per_token", "tokens")})
    generation.generation_all = orig
    print(json.dumps(res))


def kernel(calls=200):
    """One request at the C2 vocabulary, a random row: the plain entry, the
    tp entry at the defaults, a nucleus inside the fast path's set, and a
    nucleus that needs the full sort (p = 1: every token a candidate)."""
    from smer_music_generation_amd import ops as O
    from smer_music_generation_amd.generation import grammar_tables, reject_table
    from smer_music_generation_amd.vocab import WordVocab
    dev = torch.device("cuda:0")
    v = WordVocab(0, bench.CTRL)
    V = v.vocab_size
    keep, cls = grammar_tables(v, v.density_indices)
    kt, rt, ct = (torch.from_numpy(x).to(dev) for x in (keep, reject_table(v), cls))
    np.random.seed(0)
    st0 = np.random.get_state()
    mt = torch.from_numpy(np.concatenate([st0[1], [st0[2]]]).astype(np.uint32).view(np.int32)).to(dev)
    state = torch.tensor([[0, 4, 5, 0, 1, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int32, device=dev)
    zero = torch.zeros_like(state[0, 5])
    torch.manual_seed(0)
    args = [torch.randn(2, V, device=dev) * 3, state, torch.zeros(1, 16, dtype=torch.int8, device=dev), kt, rt,
            ct, torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev),
            torch.zeros(4, 2, dtype=torch.int32, device=dev), torch.zeros(1, 4, dtype=torch.int32, device=dev),
            mt, torch.zeros(3, dtype=torch.int32, device=dev)]
    kw = dict(eos=v.eos_index, m0=v.char2index('m_0'), trash_pos=200)
    res = {}
    for _ in range(3):
        for name, tp in (("plain", None), ("tp_1_none", (1.0, -1.0)), ("tp_0.8_0.9", (0.8, 0.9)),
                         ("tp_0.8_1.0_full_sort", (0.8, 1.0))):
            tp_t = None if tp is None else torch.tensor([tp], dtype=torch.float64, device=dev)

            def run(n):
                for _ in range(n):
                    state[0, 5].copy_(zero)  # the request stays live
                    O.grammar_sample_step(*args, tp=tp_t, **kw)
            run(10)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(calls)
            e1.record()
            torch.cuda.synchronize()
            res.setdefault(name, []).append(round(e0.elapsed_time(e1) * 1000.0 / calls, 2))
    print(json.dumps({"us_per_call_incl_state_reset": res}))


def batch(rounds=3):
    """generation_batch(greedy=False) on bench.py's C2 infill request set,
    warm session: the device sampler against the per-step host loop."""
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
    res = {}
    for name, kw in (("default", {}), ("t0.8_p0.9", dict(t=0.8, p=0.9))):
        for dg in (True, False):
            np.random.seed(1)
            generation.generation_batch(m, reqs, v, ac, greedy=False, device_grammar=dg, **kw)  # warm
        for _ in range(rounds):
            for dg in (True, False):
                np.random.seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, st = generation.generation_batch(m, reqs, v, ac, greedy=False, device_grammar=dg,
                                                    return_stats=True, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res.setdefault(name, {}).setdefault("device" if dg else "host_loop", []).append(
                    {"tokens": st["tokens"], "steps": st["steps"], "tokens_per_s": round(st["tokens"] / dt, 1),
                     "ms_per_step": round(1000 * st["step_call_s"] / max(1, st["steps"]), 4)})
    print(json.dumps({"requests": len(reqs), "result": res}))


if __name__ == "__main__":
    {"plugin": plugin, "kernel": kernel, "batch": batch}[sys.argv[1]]()

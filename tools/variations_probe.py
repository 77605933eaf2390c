"""Decode step with shared sources (infill variations), three legs interleaved
in one process on the C2 model (bench.make_model), bf16:

  a  R distinct sources (one per request slot: today's workload)
  b  R / TAKES sources x TAKES takes, per-row cross-attention kernels through
     the source indirection (SMER_DECODE_SHARED=0, the default)
  c  the same split, grouped kernels (attn_decode_shared_kernel,
     SMER_DECODE_SHARED=1)

    python tools/variations_probe.py [R=32] [S=1000] [TAKES=8] [--leg a|b|c]

Every request slot is live (a one-token feed per take), so each step reads
every memory once per row (a, b) or once per chunk of a group's live rows (c).
Per leg: graph-replay time per step (median / min / max over ROUNDS
interleaved rounds of N replays; a 512 MiB buffer is rewritten between timed
batches, so no leg starts on the other's cache contents), prefill time and
the session's device memory.  Also checks that b and c give the same logits
bits.  --leg X: only that leg, replayed 200 times (for a
`rocprofv3 --kernel-trace --stats` or a separate `--pmc` run around it)."""
import os
import sys
import time

import torch

sys.path.insert(0, ".")
import bench  # noqa: E402

ROUNDS, N = 7, 50


def build(m, leg, R, S, takes):
    from smer_music_generation_amd.decode import DecodeSession
    g = torch.Generator().manual_seed(0)
    n_src = R if leg == "a" else R // takes
    srcs = [torch.randint(4, 300, (S - 7 * (i % 4),), generator=g).tolist() for i in range(n_src)]
    os.environ["SMER_DECODE_SHARED"] = "1" if leg == "c" else "0"  # read at capture
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    s = DecodeSession(m, R, S, 600, use_graph=True, max_sources=n_src)
    mem = torch.cuda.memory_allocated() - mem0

    def prefill():
        if leg == "a":
            s.prefill(list(range(R)), srcs)
        else:
            s.prefill_takes(srcs, [takes] * n_src)
    prefill()  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prefill()
    torch.cuda.synchronize()
    t_pre = time.perf_counter() - t0
    logits = s.step([(i, [5], 0) for i in range(R)]).copy()  # captures the step graph
    os.environ.pop("SMER_DECODE_SHARED", None)
    return s, logits, t_pre, mem


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = sys.argv[sys.argv.index("--leg") + 1] if "--leg" in sys.argv else None
    argv = [a for a in argv if a != only]
    R = int(argv[0]) if len(argv) > 0 else 32
    S = int(argv[1]) if len(argv) > 1 else 1000
    takes = int(argv[2]) if len(argv) > 2 else 8
    from smer_music_generation_amd import _lib
    _lib.load()
    dev = torch.device("cuda", 0)
    m = bench.make_model(bench.parse_args([]), dev).eval()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    legs = [only] if only else ["a", "b", "c"]
    with torch.no_grad():
        sess = {leg: build(m, leg, R, S, takes) for leg in legs}
        if only:
            for _ in range(200):
                sess[only][0].graph.replay()
            torch.cuda.synchronize()
            return
        same = bool((sess["b"][1] == sess["c"][1]).all())
        print("R=%d S=%d takes=%d  logits of b and c bit-identical: %s" % (R, S, takes, same))
        res = {leg: [] for leg in legs}   # back to back (caches as the replays leave them)
        cold = {leg: [] for leg in legs}  # every replay after a flush (HIP events)
        for _ in range(ROUNDS):
            for leg in legs:
                g = sess[leg][0].graph
                flush.fill_(1)
                g.replay()  # first replay after the flush untimed
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(N):
                    g.replay()
                torch.cuda.synchronize()
                res[leg].append((time.perf_counter() - t0) * 1e6 / N)
                evs = []
                for _ in range(10):
                    flush.fill_(1)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    g.replay()
                    e1.record()
                    evs.append((e0, e1))
                torch.cuda.synchronize()
                ts = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
                cold[leg].append(ts[len(ts) // 2])
    for leg in legs:
        w, c = sorted(res[leg]), sorted(cold[leg])
        _, _, t_pre, mem = sess[leg]
        print("leg %s: step back-to-back median %.1f min %.1f max %.1f us | flushed median %.1f min %.1f "
              "max %.1f us | prefill %.2f ms | session %.1f MiB"
              % (leg, w[len(w) // 2], w[0], w[-1], c[len(c) // 2], c[0], c[-1], t_pre * 1e3, mem / 2 ** 20))


if __name__ == "__main__":
    main()

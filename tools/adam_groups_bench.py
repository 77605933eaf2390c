"""smer_adam_groups against smer_adam_ex on the C2 flat buffer (bf16 copy, EMA,
guarded), interleaved in one process:
    python tools/adam_groups_bench.py [--rounds 7] [--iters 20]
Three launches over the same buffers: smer_adam_ex, smer_adam_groups with a
one-group map, smer_adam_groups with the two-group map of decay_groups on the
C2 model.  Every round times each of them `iters` times back to back with HIP
events, the order rotating from round to round; the yardstick is smer_adam_ex
in the same run, and the margin its own spread over the rounds.  Prints the
per-round times, min / median / max per launch and one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
opt = ap.parse_args()

import torch  # noqa: E402
from smer_music_generation_amd import ops  # noqa: E402
from smer_music_generation_amd.train import Trainer, decay_groups  # noqa: E402
from smer_music_generation_amd.vocab import WordVocab  # noqa: E402

dev = torch.device("cuda", 0)
model = bench.make_model(bench.parse_args([]), dev, "bf16")
tr = Trainer(model, WordVocab(0, bench.CTRL), lr=1e-4, param_groups=decay_groups(model, 0.01))
gmap2 = tr.group_map
n = model.flat_parameters().numel()
runs = 1 + int((gmap2[1:] != gmap2[:-1]).sum())
print("flat %d elements, %d blocks, %d parameters, %d runs of equal map bytes, %.2f%% of the blocks in group 1"
      % (n, gmap2.numel(), len(list(model.parameters())), runs, 100.0 * float(gmap2.float().mean())))

gen = torch.Generator(device=dev).manual_seed(0)
p = torch.randn(n, device=dev, generator=gen) * 0.1
g = torch.randn(n, device=dev, generator=gen) * 1e-2
m = torch.randn(n, device=dev, generator=gen) * 1e-3
v = torch.rand(n, device=dev, generator=gen) * 1e-4
ema, pb = p.clone(), p.bfloat16()
ctl = torch.tensor([1.0, 0.5, 0.0, 0.0], device=dev)
gmap1 = torch.zeros_like(gmap2)
hp = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, decoupled_weight_decay=True)
two = [dict(hp, weight_decay=0.01), dict(hp, weight_decay=0.0)]
STEP, EMA_D = 1000, 0.999
launches = {
    "adam_ex": lambda: ops.adam_ex(p, g, m, v, pb, ctl, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, step=STEP,
                                   weight_decay=0.01, decoupled=True, ema=ema, ema_decay=EMA_D),
    "groups_one": lambda: ops.adam_groups(p, g, m, v, pb, ctl, gmap1, 0, two[:1], step=STEP, ema=ema, ema_decay=EMA_D),
    "groups_two": lambda: ops.adam_groups(p, g, m, v, pb, ctl, gmap2, 0, two, step=STEP, ema=ema, ema_decay=EMA_D),
}
names = list(launches)
for f in launches.values():  # warm-up: code objects loaded, buffers touched
    for _ in range(3):
        f()
torch.cuda.synchronize()
us = {k: [] for k in names}
for r in range(opt.rounds):
    for k in names[r % 3:] + names[:r % 3]:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(opt.iters):
            launches[k]()
        b.record()
        b.synchronize()
        us[k].append(1000.0 * a.elapsed_time(b) / opt.iters)
    print("round %d: " % r + "  ".join("%s %.1f us" % (k, us[k][-1]) for k in names), flush=True)
res = {k: dict(min=min(x), median=statistics.median(x), max=max(x)) for k, x in us.items()}
for k in names:
    print("%-11s min %.1f  median %.1f  max %.1f us  (%.0f GB/s at the median, 34 B per element)"
          % (k, res[k]["min"], res[k]["median"], res[k]["max"], 34e-3 * n / res[k]["median"]))
spread = res["adam_ex"]["max"] - res["adam_ex"]["min"]
for k in names[1:]:
    d = res[k]["median"] - res["adam_ex"]["median"]
    print("%s - adam_ex at the median: %+.1f us; adam_ex's own spread %.1f us: %s"
          % (k, d, spread, "within" if d <= spread else "OUTSIDE"))
print(json.dumps({"n": n, "rounds": opt.rounds, "iters": opt.iters, "us": res, "adam_ex_spread_us": spread}))

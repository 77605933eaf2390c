"""The C2 bench step with the Trainer's optimizer options (for tools/ab_step.py
c2adam and rocprofv3 kernel traces): bench.py's model, batch and timed region
(20 steps after 3 warm-up), the Trainer built with the given keywords.
    python tools/adam_ex_step.py [weight_decay=0.01] [coupled=1] [ema_decay=0.999] [clip_norm=1.0] [groups=0.01]
                                 [label_smoothing=0.1] [steps=20]
groups=W: param_groups=decay_groups(model, W), the two-group step (smer_adam_groups).
No argument is bench.py's own step (a default Trainer)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

opts = dict(a.split("=", 1) for a in sys.argv[1:] if a)
steps = int(opts.pop("steps", 20))
kw = {}
if "weight_decay" in opts:
    kw["weight_decay"] = float(opts.pop("weight_decay"))
if opts.pop("coupled", "0") == "1":
    kw["decoupled_weight_decay"] = False
if "ema_decay" in opts:
    kw["ema_decay"] = float(opts.pop("ema_decay"))
if "clip_norm" in opts:
    kw["clip_norm"] = float(opts.pop("clip_norm"))
if "label_smoothing" in opts:
    kw["label_smoothing"] = float(opts.pop("label_smoothing"))
groups_wd = float(opts.pop("groups")) if "groups" in opts else None
if opts:
    sys.exit("unknown option(s) %s" % sorted(opts))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from smer_music_generation_amd.synth import synth_training_batch  # noqa: E402
from smer_music_generation_amd.train import Trainer  # noqa: E402
from smer_music_generation_amd.vocab import WordVocab  # noqa: E402

args = bench.parse_args([])
dev = torch.device("cuda", 0)
v = WordVocab(0, bench.CTRL)
m = bench.make_model(args, dev, "bf16")
if groups_wd is not None:
    from smer_music_generation_amd.train import decay_groups
    kw["param_groups"] = decay_groups(m, groups_wd)
tr = Trainer(m, v, lr=1e-4, **kw)
b = synth_training_batch(1000, v, args.batch, args.seq, args.tgt)
bt = {k: torch.from_numpy(np.asarray(x)).to(dev) for k, x in b.items()}
dt, loss = bench.timed_steps(lambda: tr.step(bt), steps, 3, dev, 1)
kw.pop("param_groups", None)
print("c2adam %.3f ms/step" % (1000 * dt / steps), kw, "groups=%s" % groups_wd, "loss %.6f" % float(loss.item()))

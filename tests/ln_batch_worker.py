"""Child process of tests/test_ln_param_batch_engine_gpu.py: SMER_LN_PARAM_BATCH
is read once per process, so each value gets a fresh one.
    python tests/ln_batch_worker.py OUT.pt
One Trainer.step (its own per-range Adam hook), then one forward + backward
with a recording hook that copies its range's gradient slice when called, on
a 2 + 2 layer, d 128 model (B 2, S 64, T 32, dropout 0.1)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']


def main(out):
    from smer_music_generation_amd import ops
    from smer_music_generation_amd.model import ScoreTransformer
    from smer_music_generation_amd.synth import synth_training_batch
    from smer_music_generation_amd.train import Trainer, criterion_vectors, layer_ranges
    from smer_music_generation_amd.vocab import WordVocab
    v = WordVocab(0, CTRL)
    torch.manual_seed(11)
    m = ScoreTransformer(309, 128, 4, 2, 2, 256, 2400, 0.1, 0.1).to("cuda")
    b = synth_training_batch(5, v, 2, 64, 32)
    bt = {k: torch.from_numpy(np.asarray(x)).to("cuda") for k, x in b.items()}
    res = {}
    # 1. the product step
    loss = Trainer(m, v, lr=1e-3).step(bt)
    torch.cuda.synchronize()
    res["loss"] = loss.cpu()
    res["step_grad"] = m.flat_grad().cpu().clone()
    res["step_params"] = m.flat_parameters().detach().cpu().clone()
    # 2. forward + backward with a recording hook
    eng = m.engine
    ranges = layer_ranges(m)
    logits, _, ctx = eng.forward(bt["input"], bt["target_in"], bt["input_pad_mask"], bt["target_pad_mask"],
                                 bt["input_pad_mask"], training=True, need_weights=False, save=True, seed=12345)
    w, ce_all = criterion_vectors(v, 0.8, "cuda")
    y = bt["target_out"].reshape(-1).long()
    denom = torch.empty(1, device="cuda")
    ops.wce_denom(y, ce_all, denom)
    dlog = torch.zeros(y.numel(), eng.Vp, dtype=ctx.dt, device="cuda")
    row = torch.empty(y.numel(), device="cuda")
    ops.wce_fwd_bwd(logits, y, sum(w.values()), denom, row, None, dlog, V=eng.V)
    g = m.flat_grad()
    g.zero_()
    seen = {}

    def hook(name):
        a, e = ranges[name]
        seen[name] = g[a:e].clone()  # queued on the stream the hook runs with
    eng.backward(ctx, dlog, hook=hook)
    torch.cuda.synchronize()
    res["hook_grad"] = g.cpu().clone()
    res["hook_seen"] = {k: t.cpu() for k, t in seen.items()}
    res["ranges"] = dict(ranges)
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1])

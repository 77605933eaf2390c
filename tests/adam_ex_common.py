"""Model, batch and run shared by tests/test_adam_ex_gpu.py and its
data-parallel child process tests/adam_ex_dp_worker.py (no GPU at import)."""
import numpy as np
import torch

from tests.dp_engine_common import build, make_batch

KW = dict(lr=1e-3, weight_decay=0.01, ema_decay=0.9)


def run(steps=2, dp=False, **kw):
    """`steps` steps of a fresh bf16 Trainer(**KW, **kw) on the 2 + 2 layer
    model -> cpu clones of everything the step writes."""
    from smer_music_generation_amd.train import Trainer
    m, v = build("cuda", "bf16")
    bt = {k: torch.from_numpy(np.asarray(x)).to("cuda") for k, x in make_batch(v).items()}
    tr = Trainer(m, v, dp=dp, **dict(KW, **kw))
    for _ in range(steps):
        loss = tr.step(bt)
    torch.cuda.synchronize()
    return {"loss": loss.cpu(), "p": m.flat_parameters().detach().cpu().clone(), "m": tr.m.cpu().clone(),
            "v": tr.v.cpu().clone(), "ema": tr.ema.cpu().clone(), "bf16": m.engine._bf16.cpu().clone()}

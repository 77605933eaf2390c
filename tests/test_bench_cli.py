"""bench.py's command line: a plain run measures the headline step alone,
--full switches the other legs on, --dump-outputs writes what the last
timed step computed.  CPU only (no HIP kernel runs here)."""
import numpy as np
import torch

import bench


def test_full_is_off_by_default_and_dump_takes_a_directory():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "out", "--no-c4"])
    assert a.full and a.dump_outputs == "out" and not a.c4 and a.infill


def _tiny_model():
    from smer_music_generation_amd.model import ScoreTransformer
    torch.manual_seed(3)
    m = ScoreTransformer(309, 32, 2, 1, 1, 64, 2400, 0.0, 0.0)
    g = m.flat_grad()
    g.copy_(torch.arange(g.numel(), dtype=torch.float32) * 0.5)
    return m


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    m = _tiny_model()
    flat = m.flat_parameters().detach().numpy()
    n = flat.size
    loss = torch.tensor([1.25], dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "whole"), m, loss)
    got = {k: np.load(str(tmp_path / "whole" / (k + ".npy"))) for k in ("loss", "params", "grads")}
    assert all(x.dtype == np.float32 for x in got.values())
    assert got["loss"].tolist() == [1.25]
    assert np.array_equal(got["params"], flat)
    assert np.array_equal(got["grads"], np.arange(n, dtype=np.float32) * 0.5)
    # a buffer above the cap: the same sorted sample in every call, the two
    # arrays sampled at the same positions (the gradient encodes its index)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, loss)
    pa, ga = (np.load(str(tmp_path / "a" / f)) for f in ("params.npy", "grads.npy"))
    pb, gb = (np.load(str(tmp_path / "b" / f)) for f in ("params.npy", "grads.npy"))
    assert pa.shape == ga.shape == (1000,) and pa.dtype == ga.dtype == np.float32
    assert np.array_equal(pa, pb) and np.array_equal(ga, gb)
    idx = (ga * 2).astype(np.int64)
    assert np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(pa, flat[idx])

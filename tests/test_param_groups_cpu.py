"""Host-side contract of parameter groups in the fused Adam step
(include/smer_hip.h: smer_adam_groups; train.Trainer param_groups /
decay_groups / group_map): the symbol and the argument checks that refuse a
call before anything is launched, the Trainer's checks of its groups, the
byte map, and FusedAdam's state dict with several groups against torch's own
optimizer, both ways."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import groupsref
from tests.dp_engine_common import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HOST_BUF = (ctypes.c_uint8 * 4096)()
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from smer_music_generation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ptr():
    """A 16-byte aligned dummy address inside a live host buffer (never dereferenced)."""
    return (ctypes.addressof(_HOST_BUF) + 15) & ~15


# --- the C ABI ---------------------------------------------------------------
def test_header_signature_library_and_integration_hold_the_name(lib):
    from smer_music_generation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smer_hip.h")).read()
    assert "smer_adam_groups" in set(re.findall(r"\b(smer_[a-z0-9_]+)\(", hdr))
    assert re.search(r"#define\s+SMER_ADAM_MAX_GROUPS\s+16\b", hdr)
    assert "smer_adam_groups" in _lib.SIGNATURES and hasattr(lib, "smer_adam_groups")
    assert "smer_adam_groups" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _rows(n=3, **edit):
    """n valid rows as ops.adam_group_rows lays them out; edit: field -> (row, value)."""
    from smer_music_generation_amd import ops
    rows = ops.adam_group_rows(groupsref.GROUPS[:1] * n, 3)
    for k, (i, x) in edit.items():
        rows[k][i] = x
    return rows


def test_rows_are_the_scalars_adam_ex_forms():
    from smer_music_generation_amd import ops
    from tests import adamref
    rows = ops.adam_group_rows(groupsref.GROUPS, 3)
    assert rows.dtype.itemsize == 36 and list(rows["wd_mode"]) == [0, 1, 2]
    for r, g in zip(rows, groupsref.GROUPS):
        h = adamref.kernel_hp(**groupsref.adam_ex_kw(g), step=3)
        for a, b in (("lr", "lr"), ("b1", "b1"), ("b2", "b2"), ("eps", "eps"), ("bc1", "bc1"), ("bc2_sqrt", "bc2s"),
                     ("wd", "wd"), ("decay_mul", "decay_mul")):
            assert float(r[a]) == h[b], (a, float(r[a]), h[b])
    for bad in (0, 17):
        with pytest.raises(ValueError):
            ops.adam_group_rows(groupsref.GROUPS[:1] * bad, 3)


def test_adam_groups_statuses_before_any_launch(lib, ptr):
    rows = _rows()

    def call(n=64, p=ptr, g=ptr, m=ptr, v=ptr, pb=None, ctl=None, gmap=ptr, block0=0, rows=rows, ngroups=3,
             ema=None, ema_decay=0.0):
        return lib.smer_adam_groups(n, p, g, m, v, pb, ctl, gmap, block0, rows.ctypes.data if rows is not None else None,
                                    ngroups, ema, ema_decay, None)
    for k in ("p", "g", "m", "v", "gmap"):
        assert call(**{k: None}) == INVALID, k
        assert b"smer_adam_groups" in lib.smer_last_error()
    assert call(n=32) == INVALID and b"smer_adam_groups" in lib.smer_last_error()
    assert call(n=-64) == INVALID
    assert call(p=ptr + 4) == INVALID and b"smer_adam_groups" in lib.smer_last_error()  # 4-B, not 16-B aligned
    assert call(ema=ptr + 8) == INVALID
    assert call(pb=ptr + 4) == INVALID  # the bf16 copy: 8-B
    for bad in (0, 17):
        assert call(ngroups=bad) == INVALID and b"smer_adam_groups" in lib.smer_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(rows=_rows(wd=(1, bad))) == INVALID and b"smer_adam_groups" in lib.smer_last_error(), bad
        assert call(rows=_rows(decay_mul=(2, bad))) == INVALID, bad
        assert call(ema_decay=bad) == INVALID and b"finite" in lib.smer_last_error(), bad
    assert call(rows=_rows(wd_mode=(2, 3))) == INVALID and b"wd_mode" in lib.smer_last_error()
    assert call(rows=_rows(wd_mode=(0, -1))) == INVALID
    # nothing to do, nothing launched
    assert call(n=0) == 0
    assert call(n=0, pb=ptr + 8, ctl=ptr, ema=ptr, ema_decay=0.9, ngroups=1, block0=7) == 0


# --- Trainer(param_groups=) --------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return build("cpu")


def test_param_groups_validation(model):
    from smer_music_generation_amd.train import Trainer, decay_groups
    m, v = model
    names = [n for n, _ in m.named_parameters()]
    rest = [n for n in names if n != "fc.weight"]

    def two(**kw):
        return [{"params": ["fc.weight"]}, dict({"params": rest}, **kw)]
    Trainer(m, v, param_groups=two())  # the partition itself is fine
    bad = {
        "a parameter in two groups": [{"params": ["fc.*"]}, {"params": rest + ["fc.weight"]}],
        "a parameter in none": [{"params": ["fc.weight"]}, {"params": rest[1:]}],
        "a pattern that matches nothing": two() + [{"params": ["*.gain"]}],
        "a name that matches nothing": [{"params": ["fc.weight", "fc.wieght"]}, {"params": rest}],
        "more than 16 groups": [{"params": [n]} for n in names[:16]] + [{"params": names[16:]}],
        "no group": [],
        "amsgrad": two(amsgrad=True),
        "maximize": two(maximize=True),
        "negative weight_decay": two(weight_decay=-0.1),
        "nan weight_decay": two(weight_decay=float("nan")),
        "inf weight_decay": two(weight_decay=float("inf")),
        "beta1 = 1": two(betas=(1.0, 0.999)),
        "beta2 < 0": two(betas=(0.9, -0.1)),
        "nan beta": two(betas=(float("nan"), 0.9)),
        "negative eps": two(eps=-1e-8),
        "nan eps": two(eps=float("nan")),
        "negative lr": two(lr=-1e-4),
        "inf lr": two(lr=float("inf")),
        "a tensor of another model": [{"params": [torch.nn.Parameter(torch.zeros(3))]}, {"params": names}],
        "an unknown key": two(learning_rate=1e-3),
        "not a list": {"params": names},
    }
    for what, groups in bad.items():
        with pytest.raises(ValueError):
            Trainer(m, v, param_groups=groups)
            pytest.fail("accepted: " + what)
    assert len(names[16:]) > 1  # the 17-group case above is a partition


def test_param_groups_take_names_patterns_and_parameters_and_the_trainers_defaults(model):
    from smer_music_generation_amd.train import Trainer
    m, v = model
    named = dict(m.named_parameters())
    emb = named["embedding.weight"]
    tr = Trainer(m, v, lr=2e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05, decoupled_weight_decay=False,
                 param_groups=[{"params": ["transformer.encoder.*"], "lr": 0.0},
                               {"params": [emb, "fc.bias"], "weight_decay": 0.0, "decoupled_weight_decay": True},
                               {"params": ["transformer.decoder.*", "fc.weight"], "betas": (0.5, 0.6), "eps": 1e-3}])
    g = tr.optimizer.param_groups
    assert len(g) == 3
    assert (g[0]["lr"], g[0]["betas"], g[0]["eps"], g[0]["weight_decay"], g[0]["decoupled_weight_decay"]) == (
        0.0, (0.8, 0.99), 1e-7, 0.05, False)
    assert (g[1]["lr"], g[1]["weight_decay"], g[1]["decoupled_weight_decay"]) == (2e-4, 0.0, True)
    assert (g[2]["lr"], g[2]["betas"], g[2]["eps"], g[2]["weight_decay"]) == (2e-4, (0.5, 0.6), 1e-3, 0.05)
    # each group's parameters in named_parameters() order
    order = {id(p): i for i, p in enumerate(named.values())}
    for gr in g:
        idx = [order[id(p)] for p in gr["params"]]
        assert idx == sorted(idx)
    assert [id(p) for p in g[1]["params"]] == [id(emb), id(named["fc.bias"])]
    assert sum(len(gr["params"]) for gr in g) == len(named)


def test_decay_groups_partition_the_model(model):
    from smer_music_generation_amd.train import decay_groups
    m, _ = model
    names = [n for n, _ in m.named_parameters()]
    decay, none = decay_groups(m, 0.1)
    assert decay["weight_decay"] == 0.1 and none["weight_decay"] == 0.0
    assert sorted(decay["params"] + none["params"]) == sorted(names)
    assert not set(decay["params"]) & set(none["params"])
    norms = {n + "." + k for n, mod in m.named_modules() if type(mod).__name__ == "LayerNorm"
             for k, _ in mod.named_parameters()}
    assert len(norms) == 2 * (2 * 2 + 1 + 3 * 2 + 1)
    for n in names:
        if n.endswith("bias") or n in norms or n.startswith("embedding."):
            assert n in none["params"], n
        else:
            assert n in decay["params"] and n.endswith("weight") and m.get_parameter(n).dim() == 2, n
    assert "transformer.decoder.layers.0.multihead_attn.in_proj_bias" in none["params"]
    with pytest.raises(ValueError):
        decay_groups(m, 0.1, no_decay=("*",))


def test_group_map_carries_every_block_of_every_slot(model):
    from smer_music_generation_amd.train import Trainer, decay_groups
    m, v = model
    tr = Trainer(m, v, param_groups=decay_groups(m, 0.1))
    gm = tr.group_map
    flat = m.flat_parameters()
    assert gm.dtype == torch.uint8 and gm.dim() == 1 and gm.numel() == flat.numel() // 64
    assert gm.device == flat.device
    want = np.full(gm.numel(), 255, dtype=np.uint8)
    group_of = {id(p): gi for gi, g in enumerate(tr.optimizer.param_groups) for p in g["params"]}
    covered = 0
    for name, p in m.named_parameters():
        o = m._offsets[name]
        assert o % 64 == 0
        nblk = (p.numel() + 63) // 64  # the slot's padding carries its parameter's group
        want[o // 64: o // 64 + nblk] = group_of[id(p)]
        covered += nblk
    assert covered == gm.numel() and np.array_equal(gm.cpu().numpy(), want)
    assert set(np.unique(want)) == {0, 1}
    # in_proj_bias (384 floats = 6 blocks, group 1) sits between two weight matrices (group 0)
    o = m._offsets["transformer.encoder.layers.0.self_attn.in_proj_bias"] // 64
    assert list(want[o - 1: o + 7]) == [0, 1, 1, 1, 1, 1, 1, 0]
    one = Trainer(m, v)
    assert one.group_map.numel() == gm.numel() and not one.group_map.any()


# --- state dict --------------------------------------------------------------
def _torch_two_groups(m, groups, steps=2, cls=torch.optim.AdamW, **kw):
    """A torch optimizer over copies of the model's parameters in `groups`'
    partition (names), after `steps` steps on seeded gradients."""
    named = dict(m.named_parameters())
    copies = {n: torch.nn.Parameter(p.detach().clone()) for n, p in named.items()}
    opt = cls([dict({k: x for k, x in g.items() if k != "params"}, params=[copies[n] for n in g["params"]])
               for g in groups], lr=1e-4, **kw)
    gen = torch.Generator().manual_seed(0)
    for _ in range(steps):
        for p in copies.values():
            p.grad = torch.randn(p.shape, generator=gen)
        opt.step()
    return copies, opt


def test_two_group_adamw_state_roundtrips_through_fused_trainer(model):
    from smer_music_generation_amd.train import Trainer, decay_groups
    m, v = model
    groups = decay_groups(m, 0.03)
    groups[1]["lr"] = 5e-5
    groups[1]["betas"] = (0.8, 0.9)
    copies, opt = _torch_two_groups(m, groups)
    tr = Trainer(m, v, lr=7.0, weight_decay=0.9, param_groups=decay_groups(m, 0.5))
    tr.load_state_dict(opt.state_dict())
    g = tr.optimizer.param_groups
    assert tr.t == 2 and len(g) == 2
    assert (g[0]["lr"], g[0]["weight_decay"], g[0]["betas"], g[0]["decoupled_weight_decay"]) == (
        1e-4, 0.03, (0.9, 0.999), True)
    assert (g[1]["lr"], g[1]["weight_decay"], tuple(g[1]["betas"]), g[1]["decoupled_weight_decay"]) == (
        5e-5, 0.0, (0.8, 0.9), True)
    # the moments landed in the right parameter's slice of the flat buffers
    for n, p in m.named_parameters():
        o = m._offsets[n]
        st = opt.state[copies[n]]
        assert torch.equal(tr.m[o: o + p.numel()].view(p.shape), st["exp_avg"]), n
        assert torch.equal(tr.v[o: o + p.numel()].view(p.shape), st["exp_avg_sq"]), n
    sd = tr.state_dict()
    # torch's numbering: sequential in group order
    assert [gr["params"] for gr in sd["param_groups"]] == [gr["params"] for gr in opt.state_dict()["param_groups"]]
    assert sd["param_groups"][1]["params"][0] == len(groups[0]["params"])
    fresh = {n: torch.nn.Parameter(p.detach().clone()) for n, p in m.named_parameters()}
    opt2 = torch.optim.AdamW([{"params": [fresh[n] for n in gr["params"]]} for gr in groups], lr=1.0, weight_decay=0.7)
    opt2.load_state_dict(sd)
    for a, b in zip(opt.param_groups, opt2.param_groups):
        for k in ("lr", "betas", "eps", "weight_decay"):
            assert tuple(a[k]) == tuple(b[k]) if k == "betas" else a[k] == b[k], k
    for n in fresh:
        a, b = opt.state[copies[n]], opt2.state[fresh[n]]
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"]), n
        assert float(a["step"]) == float(b["step"]) == 2.0


def test_group_counts_must_match_and_bad_groups_raise(model):
    from smer_music_generation_amd.train import Trainer, decay_groups
    m, v = model
    groups = decay_groups(m, 0.03)
    _, opt2 = _torch_two_groups(m, groups)
    one = Trainer(m, v)
    with pytest.raises(ValueError):
        one.load_state_dict(opt2.state_dict())
    two = Trainer(m, v, param_groups=groups)
    with pytest.raises(ValueError):
        two.load_state_dict(one.state_dict())
    # the same two counts the other way round are not ours either
    _, swapped = _torch_two_groups(m, groups[::-1])
    with pytest.raises(ValueError):
        two.load_state_dict(swapped.state_dict())
    sd = opt2.state_dict()
    sd["param_groups"][1]["amsgrad"] = True
    with pytest.raises(ValueError):
        two.load_state_dict(sd)
    sd["param_groups"][1]["amsgrad"] = False
    sd["param_groups"][1]["weight_decay"] = -1.0
    with pytest.raises(ValueError):
        two.load_state_dict(sd)
    sd["param_groups"][1]["weight_decay"] = 0.0
    # one shared step
    last = sd["param_groups"][1]["params"][-1]
    sd["state"][last]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError):
        two.load_state_dict(sd)
    # a coupled checkpoint (torch.optim.Adam: no flag in older torch) loads as coupled, per group
    _, adam = _torch_two_groups(m, groups, cls=torch.optim.Adam)
    sd = adam.state_dict()
    for g in sd["param_groups"]:
        g.pop("decoupled_weight_decay", None)
    two.load_state_dict(sd)
    assert [g["decoupled_weight_decay"] for g in two.optimizer.param_groups] == [False, False]
    assert [g["weight_decay"] for g in two.optimizer.param_groups] == [0.03, 0.0]


def test_one_group_state_is_what_it_was(model):
    """A one-group trainer, by default or by a list of one, writes and loads
    the single-group format: ids 0..N-1 in named_parameters() order."""
    from smer_music_generation_amd.train import Trainer
    m, v = model
    n = len(list(m.parameters()))
    for tr in (Trainer(m, v), Trainer(m, v, param_groups=[{"params": ["*"], "weight_decay": 0.01}])):
        sd = tr.state_dict()
        assert len(sd["param_groups"]) == 1 and sd["param_groups"][0]["params"] == list(range(n))
        assert [id(p) for p in tr.optimizer.param_groups[0]["params"]] == [id(p) for p in m.parameters()]
        tr.load_state_dict(sd)


# --- lr ----------------------------------------------------------------------
def test_lr_setter_writes_every_group_and_schedulers_drive_every_group(model):
    from smer_music_generation_amd.train import Trainer, decay_groups
    m, v = model
    groups = decay_groups(m, 0.1)
    groups[0]["lr"], groups[1]["lr"] = 4e-4, 1e-4
    tr = Trainer(m, v, lr=9.0, param_groups=groups)
    assert tr.lr == 4e-4 and [g["lr"] for g in tr.optimizer.param_groups] == [4e-4, 1e-4]
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(tr.optimizer, factor=0.5, patience=0)
    sched.step(1.0)
    sched.step(2.0)  # no improvement: every group halves
    assert [g["lr"] for g in tr.optimizer.param_groups] == [2e-4, 5e-5] and tr.lr == 2e-4
    tr.lr = 3e-3
    assert [g["lr"] for g in tr.optimizer.param_groups] == [3e-3, 3e-3]
    assert "every" in type(tr).lr.__doc__ and "scheduler" in type(tr).lr.__doc__

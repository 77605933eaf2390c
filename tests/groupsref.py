"""Per-group reference loops shared by tests/test_param_groups_cpu.py and
tests/test_param_groups_gpu.py (no GPU at import): the expected result of
smer_adam_groups is smer_adam_ex (ops.adam_ex) run once per maximal run of
equal map bytes, and tests/adamref.step64 run once per group."""
import numpy as np

# one group without decay, one coupled, one decoupled; lr, betas and eps all differ
GROUPS = [
    dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False),
    dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.02, decoupled_weight_decay=False),
    dict(lr=2e-3, betas=(0.95, 0.9), eps=1e-7, weight_decay=0.1, decoupled_weight_decay=True),
]
LR = (1e-3, 3e-4)  # decay group, no-decay group


def pattern_groups():
    """Two groups for the 2 + 2 layer model of tests/adam_ex_common.run, by
    patterns alone (no model needed); the no-decay parameters come first, so
    the order differs from decay_groups' too."""
    return [{"params": ["*bias", "*norm*", "embedding.*"], "weight_decay": 0.0, "lr": LR[1]},
            {"params": ["*_weight", "*proj.weight", "*linear?.weight", "fc.weight"], "weight_decay": 0.1}]


def adam_ex_kw(g):
    """ops.adam_ex's / adamref.kernel_hp's keywords for one group dict."""
    return dict(lr=g["lr"], b1=g["betas"][0], b2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"],
                decoupled=bool(g["decoupled_weight_decay"]))


def runs(gmap):
    """[(first block, one past the last block, group id)] of the maximal runs of equal bytes."""
    gmap = np.asarray(gmap)
    cuts = [0] + [int(i) for i in np.nonzero(np.diff(gmap))[0] + 1] + [gmap.size]
    return [(a, b, int(gmap[a])) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def adam_ex_by_runs(bufs, gmap, groups, *, step, ctl=None, ema_decay=0.0):
    """ops.adam_ex on bufs (dict p, g, m, v and optionally pb, ema: device
    tensors, updated in place), one call per run of `gmap` (one byte per 64
    elements of bufs) with that run's group values."""
    from smer_music_generation_amd import ops
    for a, b, k in runs(gmap):
        sl = slice(64 * a, 64 * b)
        ops.adam_ex(bufs["p"][sl], bufs["g"][sl], bufs["m"][sl], bufs["v"][sl],
                    bufs["pb"][sl] if bufs.get("pb") is not None else None, ctl,
                    ema=bufs["ema"][sl] if bufs.get("ema") is not None else None, ema_decay=ema_decay, step=step,
                    **adam_ex_kw(groups[k]))


def step64_by_groups(st, gmap, groups, *, step, scale=None, ema_decay=0.0):
    """adamref.step64 per group on the numpy state st (p, g, m, v, ema) ->
    (values, bounds) assembled over the whole range."""
    from tests import adamref
    elem = np.repeat(np.asarray(gmap), 64)
    out = {k: np.zeros(elem.size) for k in ("p", "m", "v", "ema")}
    bnd = {k: np.zeros(elem.size) for k in out}
    for k, g in enumerate(groups):
        sel = elem == k
        if not sel.any():
            continue
        hp = adamref.kernel_hp(**adam_ex_kw(g), step=step, ema_decay=ema_decay)
        o, b = adamref.step64(st["p"][sel], st["g"][sel], st["m"][sel], st["v"][sel], st["ema"][sel], scale=scale, **hp)
        for key in out:
            out[key][sel], bnd[key][sel] = o[key], b[key]
    return out, bnd

"""Fused training step: forward -> weighted CE -> backward -> (RCCL) -> Adam.

Restates the reference step (`train.py:702-797`) with the same criteria
(`train.py:555-642`), the same normaliser (`train.py:736-742`) and torch
Adam semantics (`train.py:264`), as one stream of gfx950 kernels:

  * the 7-12 CrossEntropyLoss(weight=w_c, ignore_index=0, reduction='none')
    criteria sum to ONE weighted CE with w = sum_c w_c (the classes are
    disjoint), normalised by sum_i ce_weight_all[y_i] -> smer_wce_*;
  * data parallel (new; the reference is single-device): one
    process per GPU; the scalar denominator is all-reduced BEFORE backward,
    so SUM-reduced gradients equal the single-process gradient of the
    concatenated batch; per-layer gradient slices of the flat buffer are
    all-reduced asynchronously (RCCL over xGMI) as soon as backward has
    produced them, overlapping the remaining backward kernels;
  * Adam on the flat fp32 master buffer also refreshes the bf16 working copy;
  * optional (`clip_norm=`): global-norm gradient clipping and a non-finite
    step guard, measured and applied on the device with no host round trip;
  * optional (`weight_decay=`, `ema_decay=`): AdamW's decoupled or Adam's
    coupled weight decay and an exponential moving average of the weights,
    inside the same Adam pass (smer_adam_ex);
  * optional (`param_groups=`): torch's parameter groups -- lr, betas, eps
    and weight decay per group -- still one Adam pass per slice
    (smer_adam_groups reads each 64-element block's group from a byte map);
  * optional (`label_smoothing=`): torch's label smoothing on the twelve
    criteria, inside the fused cross-entropy kernel (smer_wce_fwd_bwd_ex).
"""
from __future__ import annotations

import contextlib
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from . import ops

CRITERIA = ["meta", "time_signature", "program", "tempo", "structure", "pitch", "duration",
            "tensile", "key", "density", "occupation", "polyphony"]


def criterion_vectors(vocab, eos_weight, device="cpu"):
    """(per-criterion weight vectors, ce_weight_all) exactly as train.py:555-642."""
    V = vocab.vocab_size
    w = {}
    meta = torch.zeros(V)
    meta[1] = eos_weight
    w["meta"] = meta
    for name, (a, b) in (("structure", (3, 7)), ("time_signature", (7, 11)), ("tempo", (11, 18)),
                         ("program", (18, 146)), ("pitch", (146, 234)),
                         ("duration", (234, 234 + len(vocab.duration_indices)))):
        t = torch.zeros(V)
        t[a:b] = 1
        w[name] = t
    for name in ("key", "tensile", "density", "polyphony", "occupation"):
        if name in vocab.control_indices:
            idx = vocab.control_indices[name]
            t = torch.zeros(V)
            t[idx[0]: idx[-1] + 1] = 1
            w[name] = t
    ce_all = torch.ones(V)
    ce_all[0] = 0
    ce_all[2] = 0
    ce_all[-1] = 0
    ce_all[1] = eos_weight
    return {k: v.to(device) for k, v in w.items()}, ce_all.to(device)


class GradBucketer:
    """Asynchronous SUM all-reduce of contiguous slices of a flat gradient
    buffer, issued in backward order (works with nccl=RCCL and gloo).

    wire_dtype=torch.bfloat16 (opt-in; fp32 is the parity default) sends each
    slice as bf16: the slice is cast into a persistent bf16 shadow on the
    compute stream, that shadow is all-reduced (half the xGMI bytes: 89 MB
    instead of 178 MB per C2 step), and the sum is widened back
    into the fp32 slice once the collective has finished.  Summation then
    happens in bf16 inside RCCL, so results differ from the fp32 reduction
    by bf16 rounding of the per-rank gradients and of the partial sums."""

    def __init__(self, flat_grad, ranges, group=None, wire_dtype=None):
        self.flat = flat_grad
        self.ranges = ranges  # name -> (start, end)
        self.group = group
        self.pending = []
        self.done = set()
        self.wire_dtype = wire_dtype if wire_dtype not in (None, flat_grad.dtype) else None
        self.shadow = (torch.empty_like(flat_grad, dtype=self.wire_dtype)
                       if self.wire_dtype is not None else None)

    def reduce(self, name):
        if name in self.done or name not in self.ranges:
            return
        a, b = self.ranges[name]
        if self.shadow is None:
            buf = self.flat[a:b]
        else:
            buf = self.shadow[a:b]
            buf.copy_(self.flat[a:b])
        self.pending.append((a, b, dist.all_reduce(buf, op=dist.ReduceOp.SUM,
                                                   group=self.group, async_op=True)))
        self.done.add(name)

    def finish(self):
        for name in self.ranges:
            self.reduce(name)
        for a, b, w in self.pending:
            w.wait()
            if self.shadow is not None:
                self.flat[a:b].copy_(self.shadow[a:b])
        self.pending = []
        self.done = set()


def broadcast_parameters(model, group=None):
    """every rank starts from rank 0's parameters.  The flat fp32
    master is one tensor, so this is a single broadcast; the bf16 working copy
    and every derived weight cache are invalidated afterwards.  The reference
    builds and initialises its model per process (train.py:257-264); without
    this, DP correctness would rest on every rank seeding identically."""
    flat = model.flat_parameters()
    src = dist.get_global_rank(group, 0) if group is not None else 0
    dist.broadcast(flat.data, src=src, group=group)
    if hasattr(model, "engine"):
        model.engine.mark_params_updated()


def layer_ranges(model):
    """Contiguous flat-buffer range per backward hook name (see
    Engine.backward): head = decoder final norm + fc, dec{i}, enc{i} (the
    last encoder layer also owns the encoder final norm), embedding."""
    off = model._offsets
    spec = model._spec
    order = [n for n, _ in spec]
    ends = {}
    for i, (n, shp) in enumerate(spec):
        ends[n] = off[n] + (math.prod(shp) + 63) // 64 * 64
    total = model.flat_parameters().numel()

    def rng(prefix_list):
        names = [n for n in order if any(n.startswith(p) for p in prefix_list)]
        return (min(off[n] for n in names), max(ends[n] for n in names))

    r = {"embedding": rng(["embedding."])}
    n_enc, n_dec = model.num_encoder_layers, model.num_decoder_layers
    for i in range(n_enc):
        pre = ["transformer.encoder.layers.%d." % i]
        if i == n_enc - 1:
            pre.append("transformer.encoder.norm.")
        r["enc%d" % i] = rng(pre)
    for i in range(n_dec):
        r["dec%d" % i] = rng(["transformer.decoder.layers.%d." % i])
    a, _ = rng(["transformer.decoder.norm."])
    r["head"] = (a, total)
    return r


def check_clip_norm(value):
    """`Trainer.clip_norm`: None (no clipping, no guard) or a number > 0,
    `float('inf')` allowed (measure and guard, never scale).  Returns None or
    the float; anything else raises ValueError."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError("clip_norm must be None or a number > 0, got %r" % (value,))
    c = float(value)
    if not c > 0:  # also NaN
        raise ValueError("clip_norm must be > 0 (float('inf') allowed), got %r" % (value,))
    return c


def check_ema_decay(value):
    """`Trainer.ema_decay`: None (no average kept) or a number 0 <= d < 1.
    Returns None or the float; anything else raises ValueError."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError("ema_decay must be None or a number in [0, 1), got %r" % (value,))
    d = float(value)
    if not 0.0 <= d < 1.0:  # also NaN
        raise ValueError("ema_decay must be in [0, 1), got %r" % (value,))
    return d


def check_label_smoothing(value):
    """`Trainer.label_smoothing`: a number 0 <= e < 1 (torch's keyword on
    CrossEntropyLoss).  Returns the float; anything else raises ValueError."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError("label_smoothing must be a number in [0, 1), got %r" % (value,))
    e = float(value)
    if not 0.0 <= e < 1.0:  # also NaN
        raise ValueError("label_smoothing must be in [0, 1), got %r" % (value,))
    return e


def check_weight_decay(value):
    """`param_groups[0]['weight_decay']` as the step reads it: a finite
    number >= 0 (torch's own rule).  Returns the float."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError("weight_decay must be a number >= 0, got %r" % (value,))
    w = float(value)
    if not 0.0 <= w < float("inf"):  # also NaN
        raise ValueError("weight_decay must be finite and >= 0, got %r" % (value,))
    return w


MAX_PARAM_GROUPS = ops.ADAM_MAX_GROUPS
_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay")
# torch's own group keys that change nothing here (amsgrad and maximize must be off)
_GROUP_IGNORED = ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused")


def _check_nonneg(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a number >= 0, got %r" % (name, value))
    x = float(value)
    if not 0.0 <= x < float("inf"):  # also NaN
        raise ValueError("%s must be finite and >= 0, got %r" % (name, value))
    return x


def check_group_values(g):
    """lr, betas, eps, weight_decay, amsgrad and maximize of one parameter
    group as the step reads them; ValueError on anything it cannot run."""
    if g.get("amsgrad") or g.get("maximize"):
        raise ValueError("FusedAdam implements Adam / AdamW without amsgrad / maximize")
    if "lr" in g:
        _check_nonneg("lr", g["lr"])
    if "eps" in g:
        _check_nonneg("eps", g["eps"])
    if "weight_decay" in g:
        check_weight_decay(g["weight_decay"])
    if "betas" in g:
        try:
            b1, b2 = (float(b) for b in g["betas"])
        except (TypeError, ValueError):
            raise ValueError("betas must be two numbers in [0, 1), got %r" % (g["betas"],)) from None
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):  # also NaN
            raise ValueError("betas must be in [0, 1), got %r" % (g["betas"],))


def resolve_param_groups(model, param_groups, defaults):
    """`Trainer(param_groups=)` -> [(parameter names, values)]: torch-shaped
    dicts whose "params" hold parameter names as `model.named_parameters()`
    gives them, fnmatch patterns over those names, or the parameters
    themselves; keys a group leaves out come from `defaults`.  The names of a
    group are in named_parameters() order.  ValueError: no group or more than
    MAX_PARAM_GROUPS, a parameter in two groups or in none, a name or pattern
    that matches nothing, a tensor that is no parameter of the model, an
    unknown key, amsgrad / maximize, or a value check_group_values refuses."""
    import fnmatch
    if isinstance(param_groups, dict) or not isinstance(param_groups, (list, tuple)):
        raise ValueError("param_groups must be a list of dicts, got %r" % type(param_groups).__name__)
    if not 1 <= len(param_groups) <= MAX_PARAM_GROUPS:
        raise ValueError("param_groups: %d groups, 1..%d supported" % (len(param_groups), MAX_PARAM_GROUPS))
    named = list(model.named_parameters())
    names = [n for n, _ in named]
    by_id = {id(p): n for n, p in named}
    known = set(names)
    owner, out = {}, []
    for gi, g in enumerate(param_groups):
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError("param_groups[%d] must be a dict with 'params'" % gi)
        unknown = [k for k in g if k != "params" and k not in _GROUP_KEYS and k not in _GROUP_IGNORED]
        if unknown:
            raise ValueError("param_groups[%d]: unknown keys %s" % (gi, unknown))
        check_group_values(g)
        entries = g["params"]
        if isinstance(entries, (str, torch.Tensor)):
            entries = [entries]
        mine = set()
        for e in entries:
            if isinstance(e, str):
                hit = [e] if e in known else fnmatch.filter(names, e)
                if not hit:
                    raise ValueError("param_groups[%d]: %r matches no parameter" % (gi, e))
            elif isinstance(e, torch.Tensor):
                if id(e) not in by_id:
                    raise ValueError("param_groups[%d]: a tensor that is no parameter of the model" % gi)
                hit = [by_id[id(e)]]
            else:
                raise ValueError("param_groups[%d]: params hold names, patterns or parameters, got %r"
                                 % (gi, type(e).__name__))
            mine.update(hit)
        for n in mine:
            if n in owner:
                raise ValueError("parameter %s is in param_groups[%d] and [%d]" % (n, owner[n], gi))
            owner[n] = gi
        vals = dict(defaults)
        vals.update({k: g[k] for k in _GROUP_KEYS if k in g})
        vals["betas"] = tuple(float(b) for b in vals["betas"])
        vals["decoupled_weight_decay"] = bool(vals["decoupled_weight_decay"])
        out.append(([n for n in names if n in mine], vals))
    missing = [n for n in names if n not in owner]
    if missing:
        raise ValueError("%d parameters are in no group: %s" % (len(missing), missing[:5]))
    return out


def decay_groups(model, weight_decay, no_decay=("*bias", "*norm*", "embedding.*")):
    """The usual two groups for `Trainer(param_groups=)`: the weight matrices
    with `weight_decay`, and everything whose name matches a `no_decay`
    pattern -- by default every bias (nn.MultiheadAttention's `in_proj_bias`
    included, which "*.bias" would miss), every LayerNorm gain and bias and
    the embedding -- with none.  Parameter names, in named_parameters() order."""
    import fnmatch
    names = [n for n, _ in model.named_parameters()]
    skip = [n for n in names if any(fnmatch.fnmatch(n, pat) for pat in no_decay)]
    keep = [n for n in names if n not in set(skip)]
    if not keep or not skip:
        raise ValueError("decay_groups: the patterns %r leave a group empty" % (tuple(no_decay),))
    return [{"params": keep, "weight_decay": weight_decay}, {"params": skip, "weight_decay": 0.0}]


class FusedAdam(torch.optim.Optimizer):
    """`torch.optim.Adam`'s state and param_groups over the Trainer's flat
    moment buffers (train.py:264 builds `Adam(model.parameters(), lr)`).

    The update itself is the Trainer's fused kernel; this object exists so
    that the reference's surrounding code works unchanged:
      * `state_dict()` / `load_state_dict()` in torch Adam's format, so a
        reference checkpoint's `optimizer_state_dict` (train.py:266-303,
        970-971) resumes here and ours resumes in torch Adam;
      * every group's `lr` is read every step, so
        `ReduceLROnPlateau(trainer.optimizer, ...)` (train.py:663-664, 939)
        and `LambdaLR` drive the fused step; `betas`, `eps`, `weight_decay`
        and `decoupled_weight_decay` (True: `torch.optim.AdamW`, False:
        `Adam(weight_decay=)`'s coupled L2) are read every step in the same
        way, so an AdamW checkpoint resumes here too.
    Per-parameter `exp_avg` / `exp_avg_sq` are views of the flat buffers.
    `groups` (resolve_param_groups' result; None: one group of every
    parameter) gives torch's parameter groups, at most MAX_PARAM_GROUPS, each
    with its parameters in named_parameters() order; parameter ids in the
    state dict are sequential in group order, as torch numbers them.
    `group_map` (uint8, one byte per 64-element block of the flat buffer, on
    its device) holds the group of every block, padding of a slot included.
    All groups share one `step`; amsgrad and maximize are not implemented."""

    def __init__(self, model, m, v, lr, betas, eps, weight_decay=0, decoupled_weight_decay=False, groups=None):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False,
                        fused=None, decoupled_weight_decay=bool(decoupled_weight_decay))
        params = dict(model.named_parameters())
        if groups is None:
            groups = [(list(params), {})]
        super().__init__([dict(vals, params=[params[n] for n in names]) for names, vals in groups], defaults)
        self._m, self._v = m, v
        self._views = []  # in group order: the state dict's parameter ids
        flat = model.flat_parameters()
        gmap = np.full(flat.numel() // 64, 255, dtype=np.uint8)
        for gi, (names, _) in enumerate(groups):
            for name in names:
                p = params[name]
                o = model._offsets[name]
                n = p.numel()
                self._views.append((p, m[o: o + n].view(p.shape), v[o: o + n].view(p.shape)))
                gmap[o // 64: (o + n + 63) // 64] = gi
        if gmap.size and int(gmap.max()) >= len(groups):
            raise RuntimeError("FusedAdam: a block of the flat buffer belongs to no parameter")
        self.group_map = torch.from_numpy(gmap).to(flat.device)
        self.t = 0

    def step(self, closure=None):
        raise RuntimeError("FusedAdam is stepped by Trainer.step (fused kernel)")

    def zero_grad(self, set_to_none=False):
        for p, _, _ in self._views:
            if p.grad is not None:
                p.grad.zero_()

    def state_dict(self):
        state = {}
        if self.t > 0:
            for i, (_, ma, va) in enumerate(self._views):
                state[i] = {"step": torch.tensor(float(self.t)), "exp_avg": ma.detach().clone(),
                            "exp_avg_sq": va.detach().clone()}
        groups, first = [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = list(range(first, first + len(g["params"])))
            first += len(g["params"])
            groups.append(d)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        ours = [len(g["params"]) for g in self.param_groups]
        if [len(g["params"]) for g in groups] != ours:
            raise ValueError("optimizer state has %d groups / %s params, expected %d / %s"
                             % (len(groups), [len(g["params"]) for g in groups], len(ours), ours))
        for g in groups:  # before anything is overwritten
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FusedAdam implements Adam / AdamW without amsgrad / maximize")
            if "weight_decay" in g:
                check_weight_decay(g["weight_decay"])
        st = state_dict["state"]
        steps = set()
        slot = 0
        for mine, g in zip(self.param_groups, groups):
            for k in ("lr", "betas", "eps", "weight_decay", "amsgrad"):
                if k in g:
                    mine[k] = g[k]
            # a group without the flag was written by torch.optim.Adam: coupled
            mine["decoupled_weight_decay"] = bool(g.get("decoupled_weight_decay", False))
            for pid in g["params"]:
                s = st.get(pid)
                _, ma, va = self._views[slot]
                slot += 1
                if s is None:
                    ma.zero_()
                    va.zero_()
                    steps.add(0)
                    continue
                ma.copy_(s["exp_avg"].reshape(ma.shape).to(ma.device, ma.dtype))
                va.copy_(s["exp_avg_sq"].reshape(va.shape).to(va.device, va.dtype))
                steps.add(int(float(s["step"])))
        if len(steps) > 1:
            raise ValueError("per-parameter Adam steps differ %s; the fused step shares one" % steps)
        self.t = steps.pop() if steps else 0


class _ClipState:
    __slots__ = ("slots", "part", "nparts", "ctl")


class Trainer:
    """One optimizer step per `step(batch)`; DP across the default process
    group when torch.distributed is initialised (world_size > 1)."""

    def __init__(self, model, vocab, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, eos_weight=0.8,
                 group=None, grad_wire_dtype=None, broadcast=True, dp=None, clip_norm=None,
                 weight_decay=0.0, decoupled_weight_decay=True, ema_decay=None, param_groups=None,
                 label_smoothing=0.0):
        """clip_norm: None (default) is the plain step.  A number c > 0 is
        the guarded step: the global L2 norm of the whole flat gradient is
        taken on the device, Adam runs on the gradient scaled by
        min(1, c / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_'s rule in
        fp32; float('inf') never scales), and a step whose norm is inf or NaN
        is skipped on the device: master weights, moments and the bf16 copy
        keep their bits and `skipped_steps` goes up by one.  The host is not
        consulted, so `t` advances on a skipped step too.  Settable per step
        like `lr`; see `grad_norm`, `clip_scale`, `skipped_steps`.
        `model.flat_grad()` holds the raw, unscaled gradient after the step.
        weight_decay, decoupled_weight_decay: torch's two forms, under
        torch's names in `optimizer.param_groups[0]` (read every step like
        `lr`).  Decoupled (default, `torch.optim.AdamW`): p *= 1 - lr * wd
        before the update.  Coupled (`torch.optim.Adam(weight_decay=)`):
        g += wd * p, after the clip scale.  Without param_groups every
        parameter decays alike.
        param_groups: None (default) is one group of every parameter, the
        step as it was.  Otherwise torch's list of dicts, at most
        MAX_PARAM_GROUPS: {"params": [...], "lr": ..., "betas": ..., "eps":
        ..., "weight_decay": ..., "decoupled_weight_decay": ...}, where
        params holds parameter names as `model.named_parameters()` gives
        them, fnmatch patterns over those names, or the parameters
        themselves, and a key left out takes this constructor's argument.
        Every parameter belongs to exactly one group (`decay_groups` builds
        the usual two).  The groups live in `optimizer.param_groups` and are
        read every step; with more than one, every Adam launch of the step is
        smer_adam_groups on the same slices and streams, which steps each
        element with its own group's values (`group_map`).  clip_norm stays
        global (one norm, one scale) and ema_decay is shared.  All groups
        share one step count, and lr=0 is no freeze: such a group keeps its
        weights' bits while its moments go on (as in torch) and its
        gradients are still computed.
        ema_decay: None (default) or 0 <= d < 1: `ema`, a flat fp32 copy of
        the weights, follows them by e += (1 - d) * (p - e) inside the Adam
        pass of every step that is not skipped; it starts as a copy of the
        weights when ema_decay first becomes a number.  Settable per step.
        See `ema_weights`, `ema_state_dict`, `load_ema_state_dict`.  With
        weight_decay == 0 and ema_decay None the step is the plain one.
        label_smoothing: 0 (default) is the plain loss, the step as it was.
        0 < e < 1 is torch's `label_smoothing=e` on each of the twelve
        CrossEntropyLoss criteria: a row with a target other than pad gets
        (1 - e) * w[y] * -log p[y] + e / V * sum_c w[c] * -log p[c] with
        w the summed criterion weights and V the vocabulary size, also where
        w[y] == 0 (targets 2 and V - 1), exactly as torch; the normaliser
        sum_i ce_weight_all[y_i] is unchanged.  The smoothing mass goes to all
        V classes alike, grammar-invalid ones included.  `step` minimises and
        returns this loss; `eval_step` and `validate` report the plain one.
        Settable per step like `clip_norm`; a constructor hyper-parameter like
        eos_weight, not part of `state_dict()`.
        grad_wire_dtype: None / torch.float32 (default, parity) or
        torch.bfloat16 for the DP gradient all-reduce (see GradBucketer).
        broadcast: under DP, copy rank 0's parameters to every rank here.
        dp: run the data-parallel path (normaliser all-reduce, per-layer
        bucketed gradient all-reduces issued from the backward hooks) --
        default: when the process group has more than one rank; True also
        at world size 1 (the real RCCL calls and stream ordering on one GPU)."""
        self._clip_norm = check_clip_norm(clip_norm)
        self._label_smoothing = check_label_smoothing(label_smoothing)
        ema_decay = check_ema_decay(ema_decay)
        weight_decay = check_weight_decay(weight_decay)
        groups = None
        if param_groups is not None:  # checked before anything is allocated
            groups = resolve_param_groups(model, param_groups, dict(
                lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                decoupled_weight_decay=bool(decoupled_weight_decay)))
        self.model = model
        self.vocab = vocab
        dev = model.flat_parameters().device
        w, ce_all = criterion_vectors(vocab, eos_weight, dev)
        self.crit_w = w
        self.w_total = sum(w.values())
        self.ce_all = ce_all
        n = model.flat_parameters().numel()
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        self.optimizer = FusedAdam(model, self.m, self.v, lr, betas, eps, weight_decay, decoupled_weight_decay,
                                   groups=groups)
        self._ema = None
        self._ema_swapped = False
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if dp and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("Trainer(dp=True) needs an initialised torch.distributed process group")
        self.dp = self.world > 1 if dp is None else bool(dp)
        self._ranges = layer_ranges(model)
        self._seed = 1
        self.grad_wire_dtype = grad_wire_dtype
        self._bucketer = None
        self._clip = None  # guarded step's device state, built by its first step
        if self.dp and broadcast:
            broadcast_parameters(model, group)
        self.ema_decay = ema_decay  # after the broadcast: the average starts from the shared weights

    # hyper-parameters live in the optimizer's param groups (schedulers edit them)
    @property
    def lr(self):
        """Group 0's learning rate.  Setting it writes the value to every
        group: per-group ratios are kept only by editing
        `optimizer.param_groups[i]["lr"]` or by a scheduler on `optimizer`."""
        return self.optimizer.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value):
        for g in self.optimizer.param_groups:
            g["lr"] = float(value)

    @property
    def group_map(self):
        """uint8, one byte per 64-element block of the flat parameter buffer:
        the index in `optimizer.param_groups` of the parameter whose slot
        holds the block (padding included)."""
        return self.optimizer.group_map

    @property
    def clip_norm(self):
        return self._clip_norm

    @clip_norm.setter
    def clip_norm(self, value):
        self._clip_norm = check_clip_norm(value)

    @property
    def label_smoothing(self):
        return self._label_smoothing

    @label_smoothing.setter
    def label_smoothing(self, value):
        self._label_smoothing = check_label_smoothing(value)

    @property
    def ema_decay(self):
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value):
        self._ema_decay = check_ema_decay(value)
        if self._ema_decay is not None:
            self._ema_buffer()

    @property
    def ema(self):
        """Flat fp32 average of `model.flat_parameters()` (same layout), None
        until `ema_decay` has been a number once."""
        return self._ema

    def _ema_buffer(self):
        if self._ema is None:
            self._ema = self.model.flat_parameters().detach().clone()
        return self._ema

    @contextlib.contextmanager
    def ema_weights(self):
        """The model on the averaged weights: exchanges the contents of the
        flat parameters and `ema` (so `eval_step`, `validate`, `generation_*`
        run on the average unchanged) and exchanges them back on exit, also on
        an exception.  `step` raises inside."""
        if self._ema is None:
            raise RuntimeError("ema_weights: no average is kept (ema_decay has never been set)")
        if self._ema_swapped:
            raise RuntimeError("ema_weights: already inside the context")
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    def _swap_ema(self):
        flat = self.model.flat_parameters().data
        with torch.no_grad():
            tmp = flat.clone()
            flat.copy_(self._ema)
            self._ema.copy_(tmp)
        self._ema_swapped = not self._ema_swapped
        self.model.engine.mark_params_updated()

    def ema_state_dict(self):
        """The average in `model.state_dict()`'s format (buffers as the model
        holds them)."""
        if self._ema is None:
            raise RuntimeError("ema_state_dict: no average is kept (ema_decay has never been set)")
        model = self.model
        src = model.flat_parameters().detach() if self._ema_swapped else self._ema
        sd = type(model.state_dict())((k, t.detach().clone()) for k, t in model.state_dict().items())
        for name, p in model.named_parameters():
            o = model._offsets[name]
            sd[name] = src[o: o + p.numel()].view(p.shape).clone()
        return sd

    def load_ema_state_dict(self, state_dict):
        """Restore the average from `ema_state_dict()`'s format (a
        `model.state_dict()`; entries that are not parameters are ignored)."""
        model = self.model
        missing = [n for n, _ in model.named_parameters() if n not in state_dict]
        if missing:
            raise ValueError("load_ema_state_dict: missing %s" % missing[:5])
        dst = model.flat_parameters().data if self._ema_swapped else self._ema_buffer()
        with torch.no_grad():
            for name, p in model.named_parameters():
                o = model._offsets[name]
                dst[o: o + p.numel()].copy_(state_dict[name].reshape(-1).to(dst.device, dst.dtype))
        if self._ema_swapped:
            model.engine.mark_params_updated()

    # the last guarded step's control block (device views, no sync until
    # read); None until a guarded step has run
    @property
    def grad_norm(self):
        """0-dim fp32: the pre-clip global gradient norm of the last guarded step."""
        return self._clip.ctl[0] if self._clip is not None else None

    @property
    def clip_scale(self):
        """0-dim fp32: the scale Adam applied; exactly 1.0 when nothing was
        clipped, 0.0 on a skipped step."""
        return self._clip.ctl[1] if self._clip is not None else None

    @property
    def skipped_steps(self):
        """0-dim fp32: guarded steps skipped so far (non-finite norm)."""
        return self._clip.ctl[3] if self._clip is not None else None

    def _clip_state(self, grad):
        """Partials buffer with one fixed slot range per layer range (the
        same partition in every mode, so the norm's bits do not depend on
        the mode) and the control block [norm, scale, skip, skip count]."""
        st = self._clip
        if st is None:
            st = self._clip = _ClipState()
            st.slots, off = {}, 0
            for name, (a, b) in self._ranges.items():
                k = ops.grad_sqnorm_nparts(b - a)
                st.slots[name] = (off, off + k)
                off += k
            st.part = torch.zeros(max(1, off), device=grad.device)
            st.nparts = off
            st.ctl = torch.zeros(4, device=grad.device)
        return st

    @property
    def t(self):
        return self.optimizer.t

    @t.setter
    def t(self, value):
        self.optimizer.t = int(value)

    def state_dict(self):
        """torch Adam format (`optimizer_state_dict` of train.py:970-971)."""
        return self.optimizer.state_dict()

    def load_state_dict(self, state_dict):
        self.optimizer.load_state_dict(state_dict)
        self.model.engine.mark_params_updated()  # weights may have been reloaded too

    def set_eos_weight(self, eos_weight):
        """Pretrain -> finetune switch (train.py:670-676)."""
        self.crit_w["meta"][1] = eos_weight
        self.w_total = sum(self.crit_w.values())
        self.ce_all[1] = eos_weight

    def step(self, batch, return_parts=False):
        """batch: dict of device tensors input/target_in/target_out/
        input_pad_mask/target_pad_mask (dataset.py:856-862).  Returns the
        (local-share) loss as a device scalar; no host sync.  With
        label_smoothing > 0 that is the smoothed loss, the quantity being
        minimised; the per-criterion parts of return_parts=True stay the plain
        ones (each row's w[y] * -log p[y], no smoothing term), so they compare
        across runs with different label_smoothing and do not sum to the
        returned loss."""
        if self._ema_swapped:
            raise RuntimeError("Trainer.step inside ema_weights(): the model holds the averaged weights")
        model = self.model
        eng = model.engine
        model.train()
        src, tin, tout = batch["input"], batch["target_in"], batch["target_out"]
        skpm, tkpm = batch["input_pad_mask"], batch["target_pad_mask"]
        B, T = tin.shape
        dropout = model.pos_dropout > 0 or model.trans_dropout > 0
        seed = 0
        if dropout:
            self._seed = (self._seed * 1103515245 + 12345) & 0x7FFFFFFF
            seed = self._seed
        logits, _, ctx = eng.forward(src, tin, skpm, tkpm, skpm, training=True,
                                     need_weights=False, save=True, seed=seed)
        y = tout.reshape(-1).contiguous().long()
        denom = torch.empty(1, device=logits.device)
        ops.wce_denom(y, self.ce_all, denom)
        if self.dp:
            dist.all_reduce(denom, group=self.group)
        dlog = torch.zeros(B * T, eng.Vp, dtype=ctx.dt, device=logits.device)
        row_loss = torch.empty(B * T, device=logits.device)
        loss = torch.empty(1, device=logits.device)
        row_nll = row_loss
        if self._label_smoothing > 0:
            row_nll = torch.empty(B * T, device=logits.device)
            ops.wce_fwd_bwd_ex(logits, y, self.w_total, denom, row_loss, loss, dlog, V=eng.V,
                               label_smoothing=self._label_smoothing, row_nll=row_nll)
        else:
            ops.wce_fwd_bwd(logits, y, self.w_total, denom, row_loss, loss, dlog, V=eng.V)
        grad = model.flat_grad()
        grad.zero_()
        hook = None
        bucketer = None
        self.t += 1
        work = eng._bf16 if eng.act_dtype() == torch.bfloat16 and eng._bf16 is not None else None
        groups = self.optimizer.param_groups
        g = groups[0]
        flat = model.flat_parameters()

        hp = dict(lr=g["lr"], b1=g["betas"][0], b2=g["betas"][1], eps=g["eps"], step=self.t)
        wd = check_weight_decay(g.get("weight_decay", 0))
        ema = self._ema_buffer() if self._ema_decay is not None else None
        # weight decay or an average: every Adam launch of the step is the
        # extended kernel, same slices on the same streams; otherwise the
        # plain step's own calls
        ex = None
        if wd != 0 or ema is not None:
            ex = dict(weight_decay=wd, decoupled=bool(g.get("decoupled_weight_decay", False)),
                      ema_decay=self._ema_decay if ema is not None else 0.0)

        # more than one parameter group: every Adam launch of the step is the
        # grouped kernel instead, same slices on the same streams
        rows = None
        if len(groups) > 1:
            for gr in groups:
                check_weight_decay(gr.get("weight_decay", 0))
            rows = ops.adam_group_rows(groups, self.t)
            gmap = self.optimizer.group_map

        def adam(a=None, b=None, ctl=None):
            sl = slice(a, b)
            bufs = (flat[sl], grad[sl], self.m[sl], self.v[sl], work[sl] if work is not None else None)
            if rows is not None:
                ops.adam_groups(*bufs, ctl, gmap, (a or 0) // 64, rows, step=self.t,
                                ema=ema[sl] if ema is not None else None,
                                ema_decay=self._ema_decay if ema is not None else 0.0)
            elif ex is not None:
                ops.adam_ex(*bufs, ctl, ema=ema[sl] if ema is not None else None, **ex, **hp)
            elif ctl is not None:
                ops.adam_guarded(*bufs, ctl, **hp)
            else:
                ops.adam(*bufs, **hp)
        stepped = None
        clip = self._clip_state(grad) if self._clip_norm is not None else None

        def sqnorm(name):
            a, b = self._ranges[name]
            o, e = clip.slots[name]
            ops.grad_sqnorm_part(grad[a:b], clip.part[o:e])
        if self.dp:
            if self._bucketer is None or self._bucketer.flat is not grad:
                # persistent: the bf16 shadow is allocated once
                self._bucketer = GradBucketer(grad, self._ranges, self.group,
                                              wire_dtype=self.grad_wire_dtype)
            bucketer = self._bucketer
            hook = bucketer.reduce
        elif clip is not None:
            # the sum of squares of each layer range as soon as its gradients
            # are final, on the stream that wrote them (Engine._hook: the
            # weight-gradient stream is current and every gradient write of
            # the range is queued on it; the embedding's hook runs on the main
            # stream after the join).  No Adam before the norm is whole, so
            # SMER_ADAM_OVERLAP does not apply.
            stepped = set()

            def hook(name):
                if name in self._ranges:
                    sqnorm(name)
                    stepped.add(name)
        elif os.environ.get("SMER_ADAM_OVERLAP", "1") != "0":
            # Adam of each layer range as soon as its gradients are final: the
            # hook runs with the weight-gradient stream current, which first
            # waits for everything the main stream has queued (that layer's
            # dgrads still read its working weights); elementwise, so the
            # result is the same bits as one Adam over the flat buffers
            main = torch.cuda.current_stream(flat.device)
            stepped = set()

            def hook(name):
                if name not in self._ranges or name == "embedding":
                    return
                torch.cuda.current_stream(flat.device).wait_stream(main)
                adam(*self._ranges[name])
                stepped.add(name)
        eng.backward(ctx, dlog, hook=hook)
        if bucketer is not None:
            bucketer.finish()
        if clip is not None:
            # DP: the reduced gradient is the same on every rank, so is the
            # norm and the skip decision -- no further collective
            for name in self._ranges:
                if stepped is None or name not in stepped:
                    sqnorm(name)
            ops.clip_scale(clip.part[:clip.nparts], self._clip_norm, clip.ctl)
            adam(ctl=clip.ctl)
        elif stepped is None:
            adam()
        else:  # the ranges no hook stepped (the embedding), on the main stream
            for name, (a, b) in self._ranges.items():
                if name not in stepped:
                    adam(a, b)
        if work is not None:
            eng.mark_bf16_fresh()
        else:
            eng.mark_params_updated()
        if return_parts:
            return loss, self.loss_parts(row_nll, y, denom)
        return loss

    def _class_table(self, dev):
        """int32 [V] token class id of every vocabulary index (vocab
        get_token_classes), the class names in id order."""
        ct = getattr(self, "_cls", None)
        if ct is None or ct[0].device != dev:
            v = self.vocab
            names = sorted(set(v.token_class_ranges.values()))
            ids = {n: i for i, n in enumerate(names)}
            # -1: an index with no token class (the reference's `accuracy`
            # raises KeyError on such a target and validate() skips the batch)
            tab = torch.tensor([ids.get(v.token_class_ranges.get(i), -1) for i in range(v.vocab_size)],
                               dtype=torch.int32)
            ct = self._cls = (tab.to(dev), names)
        return ct

    def eval_step(self, batch, smoothed=False):
        """The validation pass of one batch (train.py:1037-1195 `validate`
        body + `accuracy`, train.py:988-1034) on device, no backward: eval
        forward (no dropout), the fused criteria (no gradient written) and the
        argmax accuracy counts.  Returns (loss, {criterion: loss}, counts)
        as device tensors, no host sync; counts int32 [2 * n_classes + 2]
        (rows, hits per token class in `accuracy_from_counts`' class order,
        then the total).  The loss is the plain one whatever
        `label_smoothing` is (what perplexity and a scheduler on the
        validation loss want); smoothed=True returns the training objective
        instead.  The per-criterion losses are the plain ones either way."""
        model = self.model
        eng = model.engine
        was_training = model.training
        model.eval()
        src, tin, tout = batch["input"], batch["target_in"], batch["target_out"]
        skpm, tkpm = batch["input_pad_mask"], batch["target_pad_mask"]
        B, T = tin.shape
        try:
            with torch.no_grad():
                logits, _, _ = eng.forward(src, tin, skpm, tkpm, skpm, training=False,
                                           need_weights=False, save=False, seed=0)
                y = tout.reshape(-1).contiguous().long()
                denom = torch.empty(1, device=logits.device)
                ops.wce_denom(y, self.ce_all, denom)
                row_loss = torch.empty(B * T, device=logits.device)
                loss = torch.empty(1, device=logits.device)
                row_nll = row_loss
                if smoothed and self._label_smoothing > 0:
                    row_nll = torch.empty(B * T, device=logits.device)
                    ops.wce_fwd_bwd_ex(logits, y, self.w_total, denom, row_loss, loss, None, V=eng.V,
                                       label_smoothing=self._label_smoothing, row_nll=row_nll)
                else:
                    ops.wce_fwd_bwd(logits, y, self.w_total, denom, row_loss, loss, None, V=eng.V)
                parts = self.loss_parts(row_nll, y, denom)
                cls, names = self._class_table(logits.device)
                counts = torch.zeros(2 * len(names) + 2, dtype=torch.int32, device=logits.device)
                ops.argmax_accuracy(logits, y, cls, len(names), self.vocab.pad_index, counts)
        finally:
            if was_training:
                model.train()
        return loss, parts, counts

    def accuracy_from_counts(self, counts):
        """{token class: accuracy, 'total': accuracy} as train.py:1022-1026
        forms it (a class with no target rows keeps 0)."""
        _, names = self._class_table(self.model.flat_parameters().device)
        c = counts.detach().to("cpu").numpy().astype(np.int64)
        out = {}
        for i, n in enumerate(names + ["total"]):
            out[n] = float(c[2 * i + 1]) / float(c[2 * i]) if c[2 * i] else 0
        return out

    def loss_parts(self, row_loss, y, denom):
        """Per-criterion losses for logging (train.py:788-797), on device."""
        out = {}
        for name in CRITERIA:
            if name in self.crit_w:
                sel = self.crit_w[name][y] > 0
                out[name] = (row_loss * sel).sum() / denom[0]
        return out


def validate(valid_loader, trainer, device=None):
    """`validate` (train.py:1037-1195) over a loader of collated batches
    (dataset.py:856-862 keys) with the fused device pass: per batch the
    criteria and the accuracy counts stay on device; the dictionaries are
    averaged over batches as the reference averages them (per-batch loss and
    per-batch class accuracy, each divided by the number of batches).
    Returns (total_loss, total_accuracy)."""
    dev = device or trainer.model.flat_parameters().device
    total_loss, total_acc, steps = {}, {}, 0
    for data in iter(valid_loader):
        bt = {k: (torch.as_tensor(np.asarray(data[k])) if not torch.is_tensor(data[k]) else data[k]).to(dev)
              for k in ("input", "target_in", "target_out", "input_pad_mask", "target_pad_mask")}
        loss, parts, counts = trainer.eval_step(bt)
        steps += 1
        total_loss["total"] = total_loss.get("total", 0.0) + float(loss.item())
        for k, v in parts.items():
            total_loss[k] = total_loss.get(k, 0.0) + float(v.item())
        for k, v in trainer.accuracy_from_counts(counts).items():
            total_acc[k] = total_acc.get(k, 0.0) + v
    for d in (total_loss, total_acc):
        for k in d:
            d[k] /= max(steps, 1)
    return total_loss, total_acc

"""KV-cached, batched incremental decoder for the infill loop.

The reference re-runs the whole encoder over S source tokens and the whole
decoder over the t-token prefix for EVERY generated token
(`generation.py:542-545` -> `model_generate`, `generation.py:209-225`).
Here, per request:
  * prefill: the encoder runs once; every decoder layer's cross-attention
    K/V of the memory (`transformer.py:463`) is computed once into a cache;
  * step: only the new token(s) go through the decoder; their self-attention
    K/V are appended to a per-layer cache that persists ACROSS spans (the
    prefix accumulates, `generation.py:686`), positions continue.
Mathematically identical to the full recompute (causal attention: earlier
positions never see later tokens); fp32 mode reproduces the reference logits
to ~1e-6 and its greedy token ids exactly.

Fixed-shape step: every request owns TWO row slots per step (a feed is one
token, or two right after a control span: the control token + the next
m_0).  Unused slots are dummies that write their K/V into a reserved trash
position (Tmax-1, never attended).  The step shape is therefore constant and
is captured ONCE into a HIP graph (torch.cuda.CUDAGraph drives stream
capture; every kernel is a libsmer_hip.so launch on the captured stream) and
replayed per token: one H2D of the row table, one replay, one D2H.
"""
from __future__ import annotations

import math
import os
import time
from typing import NamedTuple

import numpy as np
import torch

from . import ops


def _capture(stream, fn):
    """Capture fn()'s launches on `stream` into a HIP graph.  Not the
    torch.cuda.graph context manager: its __enter__ empties the caching
    allocator (hipFree of every cached segment -- 40-140 ms after a training
    step had filled the cache, the whole cold-call capture cost in the
    round-3 bench), which a decode step allocating a few small buffers in
    the graph's private pool does not need."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        g.capture_begin()
        try:
            fn()
        finally:
            g.capture_end()
    return g


class _StepPlan(NamedTuple):
    """How a session's decoder step runs (DecodeSession._plan): every field
    follows from the precision, the shapes and the SMER_DECODE_* switches."""
    # post-norm LayerNorms in the prologue of the Linear that consumes them
    # (ops.linear_decode_ln: LN3 -> next QKV, LN1 -> cross Q, LN2 -> FFN1, final
    # norm -> vocab head; the LN output also stored as the next residual, the
    # LayerNorm kernel's bits) and the new K/V appended by the QKV epilogue:
    # bf16 7-8 launches per layer (11 in round 1), fp32 8 instead of 12.
    # False: one kernel per LayerNorm, kv_scatter after the QKV Linear.
    fused: bool
    # LN1 + the cross query projection inside the cross-attention blocks.
    # bf16: re-reads the head's Wq slice per (row, head) block: 329 vs 342 us
    # per replayed step at R = 32, 484 vs 480 at R = 64
    # (tools/decode_host_probe.py).  It rounds q in a different order than the
    # Linear, so the choice must not depend on the batch (a request's tokens
    # may not depend on its batch-mates): on whenever the shape allows it.
    # fp32: inside the split attention blocks, few rows only (batch 1-2: one
    # launch fewer per layer; each block re-reads its head's 128 KB of Wq from
    # L2, so not for many rows).
    qln: bool
    # cross attention reads the row's SOURCE slot: takes that share a source
    # share one prefill and one memory, and the per-row kernels read it through
    # the indirection.  shared (SMER_DECODE_SHARED=1, fewer sources than
    # requests, bf16): the grouped kernels instead, which load each K / V key
    # step once per chunk of a group's rows and write the per-row kernels'
    # bits.  Off by default: measured slower (C2 shapes, 4 sources x 8 takes:
    # 426 vs 289 us per replayed step, tools/variations_probe.py) --
    # the repeated reads of the per-row blocks hit in the caches, and the
    # grouped form leaves 64 walking blocks for 256 CUs.  Never with two
    # chains: a half's group table would be another one.  (fp32 has no grouped
    # kernel: takes run the per-row kernels on the source's slot.)
    shared: bool
    # fp32 cross attention as flash-decoding (8 key slices per (row, head),
    # merged in the out-projection's prologue): the unsplit form runs
    # 2 * R * H blocks, 16 at batch 1.  (The self attention stays unsplit: its
    # <= ~400-key caches measured 0.306 vs 0.296 ms per step split.)
    split_f32: bool
    # request chains per step.  SMER_DECODE_CHAINS=2 (bf16) splits the requests
    # into two halves on two graph branches; measured slower (C2 364 vs 326 us
    # per replay, C5 888 vs 871: tools/decode_chain_probe.py), so one chain is
    # the default.
    chains: int


class _Sampler(NamedTuple):
    """The sampler's inputs of one call (host arrays)."""
    reject: np.ndarray   # uint8 [13, V]: generation.reject_table
    mt: np.ndarray       # uint32 MT19937 key + position: [625], per_request [R, LDMT]
    tp: np.ndarray       # float64 [R, 2]: temperature, nucleus p (-1 = none)
    per_request: bool    # one stream per request (the "rows" graphs)


class DecodeResult(NamedTuple):
    """What greedy_decode / sampled_decode return; None where a field does not
    apply to the call."""
    ids: list       # per request the emitted token ids
    steps: int
    err: np.ndarray  # per request: bit 0 prefix exceeds max_tgt, bit 1 probabilities missed 1
    step_ms: list   # GPU end time of each step from the loop's start
    fails: list = None  # sampled: per request, per id, 1 = the redraws ran out
    logp: list = None   # score: per request the float64 log-probabilities of its ids

    @classmethod
    def empty(cls, n, sampled, score):
        return cls([[] for _ in range(n)], 0, np.zeros(n, dtype=np.int32), [],
                   [[] for _ in range(n)] if sampled else None,
                   [np.zeros(0) for _ in range(n)] if score else None)


class _GrammarGraph:
    """One captured (decoder step + grammar) graph of a session and the
    buffers it addresses, which are its own: the graphs of the other modes
    keep theirs.  mode: "greedy", "stream" (the sampler on the one shared
    MT19937 stream) or "rows" (the sampler on one stream per request).
    ban: the graph runs smer_logits_ban between the decoder step and the
    grammar kernel.  score: it also takes the log-probability of every drawn
    token (smer_logprob_stage before the grammar kernel, smer_logprob_commit
    after it) into g_logp float64 [R, cap], entry for entry with g_out.
    tpl: the graph runs smer_logits_template in front of the grammar kernel
    (after the score stage, which therefore sees the row the model gave), on
    g_tape int16 [R, nm, TPL_LEN].
    bar: the graph runs smer_bar_clock between the score stage and the
    template kernel, on g_barlen int32 [R] (0: the request has no clock),
    g_units uint8 [V] and g_clock int32 [R, CLOCK_WORDS], which follows the
    tokens of g_out and is zeroed per call as g_out is.
    chord: the graph (which always has the bar node) runs smer_chord_ban between
    the clock and the template kernel, on g_chordlen int32 [R] (0: the request
    has no chords), g_chordat int8 [R, nm, CHORD_POS] (-1: no row) and
    g_chordbits int32 [R, CHORD_ROWS, 16]; it reads g_clock and writes only
    logits.
    Construction allocates; load() writes a call's inputs, before the capture
    and before every later call alike."""

    def __init__(self, sess, key, mode, nm, keep_shape, cls_shape, *, eos, m0, lookahead, max_span,
                 use_ring, ban, score, tpl=False, bar=False, chord=False):
        self.key, self.mode, self.ban, self.score, self.tpl, self.bar = key, mode, ban, score, tpl, bar
        self.chord = chord
        self.graph = None
        R, cap, dev = sess.R, sess.Tmax, sess.dev

        def zeros(*shape, dtype=torch.int32):
            return torch.zeros(*shape, dtype=dtype, device=dev)
        b = self.bufs = dict(
            g_state=zeros(R, sess.N_STATE), g_targets=zeros(R, nm, dtype=torch.int8),
            g_keep=zeros(keep_shape, dtype=torch.uint8), g_cls=zeros(cls_shape, dtype=torch.uint8),
            g_srclen=zeros(R), g_out=zeros(R, cap))
        if mode != "greedy":
            b["g_reject"] = zeros(keep_shape, dtype=torch.uint8)
            b["g_tp"] = zeros(R, 2, dtype=torch.float64)
            if mode == "rows":
                b["g_mt_rows"] = zeros(R, sess.LDMT)
            else:
                b["g_mt"] = zeros(625)
        if ban:
            b["g_banmask"] = zeros(R, nm, dtype=torch.int8)
            b["g_banbits"] = zeros(R, sess.BAN_K, ops.BAN_WORDS)
        if score:
            b["g_lp_row"] = zeros(R, 512, dtype=torch.float64)
            b["g_lp_stage"] = torch.full((R,), -1, dtype=torch.int32, device=dev)
            b["g_logp"] = zeros(R, cap, dtype=torch.float64)
        if tpl:
            b["g_tape"] = torch.full((R, nm, ops.TPL_LEN), ops.TPL_FREE, dtype=torch.int16, device=dev)
        if bar:
            b["g_barlen"] = zeros(R)
            b["g_units"] = zeros(cls_shape, dtype=torch.uint8)
            b["g_clock"] = zeros(R, ops.CLOCK_WORDS)
        if chord:
            b["g_chordlen"] = zeros(R)
            b["g_chordat"] = torch.full((R, nm, ops.CHORD_POS), -1, dtype=torch.int8, device=dev)
            b["g_chordbits"] = zeros(R, ops.CHORD_ROWS, ops.BAN_WORDS)
        # live counts: the step's grammar kernel publishes its count into a
        # pinned host ring itself (no per-step memset / D2H copy between the
        # replays); SMER_GRAMMAR_RING=0: memset + copy per step (A/B)
        self.ring = torch.zeros(2 * lookahead + 2, dtype=torch.int32).pin_memory()
        self.rv = self.ring.numpy()
        b["g_alive"] = zeros(3 if use_ring else 1)
        self.gargs = dict(eos=eos, m0=m0, trash_pos=sess.Tmax - 1, max_span=max_span,
                          ring=self.ring if use_ring else None)

    def load(self, st, tg, keep, cls, src_len, ban=None, sampler=None, tape=None, bar=None, chord=None):
        """Write one call's inputs (host arrays) and clear its outputs."""
        b = self.bufs

        def up(name, a):
            b[name].copy_(torch.from_numpy(a))
        up("g_state", st)
        up("g_targets", tg)
        up("g_keep", np.ascontiguousarray(keep, dtype=np.uint8))
        up("g_cls", np.ascontiguousarray(cls, dtype=np.uint8))
        up("g_srclen", src_len.astype(np.int32))
        if self.ban:
            up("g_banmask", ban[0])
            up("g_banbits", ban[1].view(np.int32))
        if self.tpl:
            up("g_tape", tape)
        if self.bar:
            up("g_barlen", bar[0])
            up("g_units", bar[1])
            b["g_clock"].zero_()
        if self.chord:
            up("g_chordlen", chord[0])
            up("g_chordat", chord[1])
            up("g_chordbits", chord[2].view(np.int32))
        if self.mode != "greedy":
            up("g_reject", np.ascontiguousarray(sampler.reject, dtype=np.uint8))
            up("g_mt_rows" if self.mode == "rows" else "g_mt", sampler.mt.view(np.int32))
            up("g_tp", sampler.tp)
        b["g_out"].zero_()
        if self.score:
            b["g_logp"].zero_()
        b["g_alive"].zero_()
        self.ring.zero_()

    def step(self, logits, ids, meta):
        """The launches that follow the decoder step inside the graph: they
        pick every request's token from `logits` and write the next step's
        feed into the session's row tables `ids` and `meta`."""
        b = self.bufs
        state, targets, keep = b["g_state"], b["g_targets"], b["g_keep"]
        if self.ban:  # banned logits -> -100 ahead of the grammar kernel
            ops.logits_ban(logits, state, b["g_banmask"], b["g_banbits"])
        if self.score:  # the row's log-softmax while the row exists, the drawn token's entry after
            ops.logprob_stage(logits, state, targets, keep, b["g_lp_row"], b["g_lp_stage"])
        if self.bar:  # the bar clock: follows the token the step before drew, then bans by the cursor
            ops.bar_clock(logits, state, targets, b["g_out"], b["g_cls"], b["g_units"], b["g_barlen"],
                          b["g_clock"], eos=self.gargs["eos"])
        if self.chord:  # the chord at the onset the clock just computed: the pitches outside it -> -100
            ops.chord_ban(logits, state, targets, b["g_clock"], b["g_chordlen"], b["g_chordat"],
                          b["g_chordbits"], cap=b["g_out"].shape[1])
        if self.tpl:  # the given opening of a span: forced after the score saw the model's row
            ops.logits_template(logits, state, b["g_cls"], b["g_tape"])
        if self.mode == "greedy":
            ops.grammar_greedy_step(logits, state, targets, keep, b["g_cls"], b["g_srclen"], ids, meta,
                                    b["g_out"], b["g_alive"], **self.gargs)
        else:
            rows = self.mode == "rows"
            (ops.grammar_sample_step_rows if rows else ops.grammar_sample_step)(
                logits, state, targets, keep, b["g_reject"], b["g_cls"], b["g_srclen"], ids, meta,
                b["g_out"], b["g_mt_rows" if rows else "g_mt"], b["g_alive"], tp=b["g_tp"], **self.gargs)
        if self.score:
            ops.logprob_commit(state, b["g_lp_stage"], b["g_out"], b["g_lp_row"], b["g_logp"],
                               V=keep.shape[1])


class DecodeSession:
    def __init__(self, model, max_requests, max_src, max_tgt, precision=None, use_graph=True,
                 max_sources=None):
        if precision is not None:
            model.set_precision(precision)
        self.model = model
        self.eng = model.engine
        eng = self.eng
        self.dt = eng.act_dtype()
        dev = model.flat_parameters().device
        if dev.type != "cuda":
            raise RuntimeError("DecodeSession needs the model on a ROCm GPU")
        self.dev = dev
        self.R, self.Smax = int(max_requests), int(max_src)
        # encoded sources are slots of their own: several request slots (the
        # takes of one request) may be bound to one source slot and then share
        # its cross-attention memory.  Default: one source slot per request.
        self.NS = self.R if max_sources is None else int(max_sources)
        if not 1 <= self.NS <= self.R:
            raise ValueError("max_sources must be in 1..max_requests")
        self.Tmax = int(max_tgt) + 1  # + trash slot
        d = eng.d
        self.d = d
        if max(self.Smax, self.Tmax) > model.pos_enc.pe.shape[0]:
            model.pos_enc.extend(max(self.Smax, self.Tmax))
        self.self_kv = [torch.zeros(self.R, self.Tmax, 2 * d, dtype=self.dt, device=dev)
                        for _ in range(eng.n_dec)]
        # cross-attention memory, head-major [sources, K|V, H, Smax, D]: each
        # (source, head) is one contiguous key run per decode step
        H, D = eng.H, eng.D
        self.cross_kv = [torch.zeros(self.NS, 2, H, self.Smax, D, dtype=self.dt, device=dev)
                         for _ in range(eng.n_dec)]
        self.src_len = np.zeros(self.R, dtype=np.int64)
        self.W = eng.weights(self.dt)
        # static step buffers: 2 slots per request
        M = 2 * self.R
        self.M = M
        self.ids_t = torch.zeros(M, dtype=torch.int64, device=dev)
        self.meta_t = torch.zeros(4, M, dtype=torch.int32, device=dev)
        # the request-to-source binding, device data written at prefill and
        # read by the cross attention of the captured step (never baked into
        # a graph, and outside meta_t, which the grammar kernels rewrite every
        # step): src_t[row] = source slot of the row's request; grp_t[g] =
        # (first row, row count) of the g-th run of requests on one source
        self.req_src = np.minimum(np.arange(self.R), self.NS - 1).astype(np.int32)
        self.src_t = torch.zeros(M, dtype=torch.int32, device=dev)
        self.grp_t = torch.zeros(self.NS, 2, dtype=torch.int32, device=dev)
        self.prefill_rows = 0
        self._bind()
        self.ids_h = torch.zeros(M, dtype=torch.int64).pin_memory()
        self.meta_h = torch.zeros(4, M, dtype=torch.int32).pin_memory()
        self.logits_h = torch.zeros(M, eng.V, dtype=torch.float32).pin_memory()
        self.use_graph = use_graph
        self.graph = None
        # step(): the row-table H2D and logits D2H copies inside the step graph
        self._graph_copies = os.environ.get("SMER_DECODE_GRAPH_COPY", "1") == "1"
        self.logits_t = torch.empty(M, eng.V, device=dev)
        # the positional table the captured graphs address (pos_enc.extend()
        # by a later session reallocates it: _pe_guard drops stale graphs)
        self._pe_ptr = model.pos_enc.pe.data_ptr()
        self.plan = None      # the _StepPlan of the last _run (None: no step has run yet)
        self._side = None     # the second chain's stream, made on first use
        self._graphs = {}     # name ("greedy", "stream+ban", "rows+ban+bar+chord+tpl+score", ..) -> _GrammarGraph
        self._greedy = None   # the _GrammarGraph of the last call
        self.phase_s = {}     # host seconds of the last device loop's phases (bench / probes)

    def _pe_guard(self):
        """Drop the captured step / greedy graphs when the model's
        positional table moved since they were captured (another session's
        pos_enc.extend() freed the buffer they read)."""
        ptr = self.model.pos_enc.pe.data_ptr()
        if ptr != self._pe_ptr:
            self.graph, self._graphs, self._greedy, self._pe_ptr = None, {}, None, ptr

    def refresh_weights(self):
        self.W = self.eng.weights(self.dt)
        self.graph = None

    # ------------------------------------------------------------------
    def _bind(self):
        """Write the request-to-source binding (self.req_src) to the device:
        the per-row source index and the group table (ordinary copies)."""
        runs = []
        for r, s in enumerate(self.req_src.tolist()):
            if runs and runs[-1][0] == s:
                runs[-1][2] += 1
            else:
                runs.append([s, r, 1])
        if len(runs) > self.NS or len({s for s, _, _ in runs}) != len(runs):
            raise ValueError("the request slots of a source must be consecutive")
        tab = np.zeros((self.NS, 2), dtype=np.int32)
        for g, (_, r0, n) in enumerate(runs):
            tab[g] = (2 * r0, 2 * n)
        self.src_t.copy_(torch.from_numpy(np.repeat(self.req_src, 2)))
        self.grp_t.copy_(torch.from_numpy(tab))

    def prefill(self, slots, srcs):
        """Encode `srcs` (list of 1-D int arrays) into request `slots`:
        request slot s is bound to source slot s."""
        slots = [int(s) for s in slots]
        if slots and max(slots) >= self.NS:
            raise ValueError("request slot %d has no source slot of its own (max_sources %d)"
                             % (max(slots), self.NS))
        lens = self._encode(slots, srcs)
        for b, s in enumerate(slots):
            self.req_src[s] = s
            self.src_len[s] = lens[b]
        self._bind()

    def prefill_takes(self, srcs, takes):
        """Encode srcs[i] ONCE into source slot i and bind takes[i]
        consecutive request slots to it (request slots 0, 1, .. in order):
        the takes of one source share its cross-attention memory.  Slots past
        sum(takes) stay bound to the last source (they are never live)."""
        takes = [int(n) for n in takes]
        if len(takes) != len(srcs) or any(n < 1 for n in takes):
            raise ValueError("prefill_takes: one take count >= 1 per source")
        if len(srcs) > self.NS or sum(takes) > self.R:
            raise ValueError("prefill_takes: %d sources / %d takes exceed the session (%d / %d)"
                             % (len(srcs), sum(takes), self.NS, self.R))
        lens = self._encode(list(range(len(srcs))), srcs)
        r = 0
        for i, n in enumerate(takes):
            self.req_src[r:r + n] = i
            self.src_len[r:r + n] = lens[i]
            r += n
        self.req_src[r:] = len(srcs) - 1
        self._bind()

    def _encode(self, slots, srcs):
        """Run the encoder over `srcs` and scatter every decoder layer's
        cross-attention K / V of the memories into source `slots`.  Returns
        the source lengths."""
        eng, W, dt, dev, d = self.eng, self.W, self.dt, self.dev, self.d
        H, D = eng.H, eng.D
        B = len(slots)
        lens = [len(s) for s in srcs]
        S = max(lens)
        if S > self.Smax:
            raise ValueError("source length %d exceeds session max_src %d" % (S, self.Smax))
        src = np.zeros((B, S), dtype=np.int64)
        for b, s in enumerate(srcs):
            src[b, :len(s)] = np.asarray(s, dtype=np.int64)
        src_t = torch.from_numpy(src).to(dev)
        kpm = None
        if min(lens) != S:
            kpm = torch.from_numpy((np.arange(S)[None, :] >= np.array(lens)[:, None]).astype(np.uint8)).to(dev)
        pe = self.model.pos_enc.pe
        pe2 = pe.view(pe.shape[0], pe.shape[2])
        x = torch.empty(B * S, d, dtype=dt, device=dev)
        ops.embed(src_t.view(-1), W.emb, pe2, x, L=S, scale=math.sqrt(d))
        scale = 1.0 / math.sqrt(D)
        for L in W.enc:
            qkv = ops.linear(x, L.in_w, L.in_b)
            o = torch.empty(B * S, d, dtype=dt, device=dev)
            lse = torch.empty(B, H, S, device=dev)
            ops.attn_fwd(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], o, lse, B=B, H=H, Lq=S,
                         Lk=S, D=D, kpm=kpm, causal=False, scale=scale)
            y1 = ops.linear(o, L.out_w, L.out_b, residual=x)
            x1, _, _ = eng._ln(y1, L.n1, dt)
            h = ops.linear(x1, L.l1_w, L.l1_b, relu=True)
            y2 = ops.linear(h, L.l2_w, L.l2_b, residual=x1)
            x, _, _ = eng._ln(y2, L.n2, dt)
        mem, _, _ = eng._ln(x, W.enc_norm, dt)
        # all B*S memory rows go to the caches (rows past a source's length
        # land beyond its src_len and are never attended)
        req = np.repeat(np.asarray(slots, dtype=np.int32), S)
        pos = np.tile(np.arange(S, dtype=np.int32), B)
        req_t = torch.from_numpy(req).to(dev)
        pos_t = torch.from_numpy(pos).to(dev)
        for li, L in enumerate(W.dec):
            kvc = ops.linear(mem, L.ckv_w, L.ckv_b)
            ops.kv_scatter_heads(kvc, self.cross_kv[li], req_t, pos_t, H=H, D=D,
                                 req_stride=2 * H * self.Smax * D, kv_stride=H * self.Smax * D,
                                 head_stride=self.Smax * D)
        self.prefill_rows = B * S
        return lens

    # ------------------------------------------------------------------
    def _plan(self):
        """The step plan of this session under the current switches."""
        d, M, D = self.d, self.M, self.eng.D
        if self.dt == torch.float32:
            # the fused fp32 layers need the LayerNorm-prologue Linear's limits
            # (K = d_model a multiple of 8, at most 2048); other widths unfused
            fused = (M <= 64 and d % 8 == 0 and d <= 2048
                     and os.environ.get("SMER_DECODE_F32_FUSED", "1") == "1")
            split = fused and D == 64 and os.environ.get("SMER_DECODE_SPLIT_F32", "1") == "1"
            qln = split and d == 512 and M <= 4 and os.environ.get("SMER_DECODE_QLN_F32", "1") == "1"
            return _StepPlan(fused, qln, False, split, 1)
        if self.dt != torch.bfloat16:
            return _StepPlan(False, False, False, False, 1)
        chains = 2 if self.R >= 2 and os.environ.get("SMER_DECODE_CHAINS", "1") == "2" else 1
        qln = D == 64 and d in (512, 768, 1024) and os.environ.get("SMER_DECODE_QLN", "1") == "1"
        shared = (self.NS < self.R and D in (32, 64) and chains == 1
                  and os.environ.get("SMER_DECODE_SHARED", "0") == "1")
        return _StepPlan(True, qln, shared, False, chains)

    def _run(self):
        """The fixed-shape decoder step on the static buffers."""
        eng, W, d, M = self.eng, self.W, self.d, self.M
        plan = self.plan = self._plan()
        pe = self.model.pos_enc.pe
        pe2 = pe.view(pe.shape[0], pe.shape[2])
        x = torch.empty(M, d, dtype=self.dt, device=self.dev)
        ops.embed(self.ids_t, W.emb, pe2, x, positions=self.meta_t[0], scale=math.sqrt(d))
        if plan.chains == 1:
            self._run_layers(plan, x, 0, M)
            return
        # Two independent request halves on two streams (graph branches),
        # meant to overlap one half's HBM-bound cross attention with the
        # other half's latency-bound Linears.  Every kernel computes a row
        # the same way whatever rows share its launch (logits bit-identical
        # either way).
        h = 2 * (self.R // 2)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        main = torch.cuda.current_stream(self.dev)
        self._side.wait_stream(main)
        self._run_layers(plan, x, 0, h)
        with torch.cuda.stream(self._side):
            self._run_layers(plan, x, h, M)
        main.wait_stream(self._side)

    def _run_layers(self, plan, x, r0, r1):
        """The decoder layers and the vocabulary head on step rows r0..r1 (all
        of them, or one chain's half) as `plan` says; logits into
        self.logits_t[r0:r1].  The launches of a configuration, their operands
        and the order of the allocations are fixed: they make its logits bits
        and the size of a captured step's private pool."""
        eng, W, dt, dev, d = self.eng, self.W, self.dt, self.dev, self.d
        H, D, M = eng.H, eng.D, r1 - r0
        pos_t, req_t, nks_t, nkc_t = (self.meta_t[0, r0:r1], self.meta_t[1, r0:r1],
                                      self.meta_t[2, r0:r1], self.meta_t[3, r0:r1])
        src_t = self.src_t[r0:r1]  # cross attention: the row's SOURCE slot
        x = x[r0:r1]
        scale = 1.0 / math.sqrt(D)
        sstride = self.Tmax * 2 * d
        fused, bf16 = plan.fused, dt == torch.bfloat16
        skw = dict(H=H, D=D, row_stride=2 * d, req_stride=sstride, scale=scale)
        ckw = dict(H=H, D=D, row_stride=D, req_stride=2 * H * self.Smax * D, head_stride=self.Smax * D,
                   scale=scale)

        def new():
            return torch.empty(M, d, dtype=dt, device=dev)
        y = n = None  # the layer below's FFN output and its LN3, which the next Linear in line applies
        for li, L in enumerate(W.dec):
            cache, cc = self.self_kv[li], self.cross_kv[li]
            # QKV projection (of LN3 of the layer below), the new K/V appended
            if not fused:
                if y is not None:
                    x, _, _ = eng._ln(y, n, dt)
                qkv = ops.linear(x, L.sa_w, L.sa_b)
                ops.kv_scatter(qkv[:, d:], cache, req_t, pos_t, row_stride=2 * d, req_stride=sstride)
            else:
                kv = dict(kv=cache, kv_req=req_t, kv_pos=pos_t, kv_row_stride=2 * d,
                          kv_req_stride=sstride, kv_col0=d)
                if y is None:  # layer 0: x is the embedding (no norm in front)
                    qkv = ops.linear_decode(x, L.sa_w, L.sa_b, **kv)
                else:
                    x = new()
                    qkv = ops.linear_decode_ln(y, n[0], n[1], L.sa_w, L.sa_b, x_out=x, **kv)
            o = new()
            ops.attn_decode(qkv[:, :d], cache, cache.view(-1)[d:], req_t, nks_t, o, **skw)
            y1 = ops.linear(o, L.sa_ow, L.sa_ob, residual=x)
            # x1 = LN1(y1); cross attention of x1 . Wq over the source's memory; out-projection + x1
            lnq = (y1, L.n1[0], L.n1[1], L.cq_w, L.cq_b)
            mem = (cc, cc.view(-1)[H * self.Smax * D:], src_t, nkc_t)  # K half, V half, row -> slot, keys
            if fused:
                x1 = new()
            else:
                x1, _, _ = eng._ln(y1, L.n1, dt)
            if plan.split_f32:  # 8 key slices per (row, head), merged by the out-projection
                if not plan.qln:
                    qc = ops.linear_decode_ln(*lnq, x_out=x1)
                part = torch.empty(M, H, ops.DEC_SPLITS, 68, device=dev)
                if plan.qln:
                    ops.attn_decode_split_qln_f32(*lnq, *mem, part, x_out=x1, **ckw)
                else:
                    ops.attn_decode_split_f32(qc, *mem, part, **ckw)
                y2 = ops.linear_decode_merge_f32(part, L.ca_ow, L.ca_ob, M=M, residual=x1)
            else:
                if bf16:  # (the bf16 step takes oc ahead of the projection, the fp32 ones after it)
                    oc = new()
                if not plan.qln:
                    qc = ops.linear_decode_ln(*lnq, x_out=x1) if fused else ops.linear(x1, L.cq_w, L.cq_b)
                if not bf16:
                    oc = new()
                if plan.qln and plan.shared:
                    ops.attn_decode_shared_qln(*lnq, *mem, self.grp_t, oc, x_out=x1, **ckw)
                elif plan.qln:
                    ops.attn_decode_qln(*lnq, *mem, oc, x_out=x1, **ckw)
                elif plan.shared:
                    ops.attn_decode_shared(qc, *mem, self.grp_t, oc, **ckw)
                else:
                    ops.attn_decode(qc, *mem, oc, **ckw)
                y2 = ops.linear(oc, L.ca_ow, L.ca_ob, residual=x1)
            # x2 = LN2(y2); FFN + x2
            if fused:
                x2 = new()
                h = ops.linear_decode_ln(y2, L.n2[0], L.n2[1], L.l1_w, L.l1_b, relu=True, x_out=x2)
            else:
                x2, _, _ = eng._ln(y2, L.n2, dt)
                h = ops.linear(x2, L.l1_w, L.l1_b, relu=True)
            y, n = ops.linear(h, L.l2_w, L.l2_b, residual=x2), L.n3
        x, _, _ = eng._ln(y, n, dt)  # the last LN3, then the final norm into the vocabulary head
        if fused:
            ops.linear_decode_ln(x, W.dec_norm[0], W.dec_norm[1], W.fc_w, W.fc_b,
                                 out_f32=self.logits_t[r0:r1])
        else:
            out, _, _ = eng._ln(x, W.dec_norm, dt)
            ops.gemm(out, W.fc_w, M=M, N=eng.V, K=d, out_f32=self.logits_t[r0:r1], bias=W.fc_b, dtype=dt)

    def _ensure_graph(self):
        if self.graph is not None or not self.use_graph:
            return
        # warm up eagerly once (allocator, library load), then capture; the
        # step graph also holds the row-table H2D copies and the logits D2H
        # copy (memcpy nodes: no separate copy launches per token)
        self._run()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        self.graph = _capture(s, self._run_with_copies if self._graph_copies else self._run)
        torch.cuda.current_stream().wait_stream(s)

    def _run_with_copies(self):
        self.ids_t.copy_(self.ids_h, non_blocking=True)
        self.meta_t.copy_(self.meta_h, non_blocking=True)
        self._run()
        self.logits_h.copy_(self.logits_t, non_blocking=True)

    def _load_feeds(self, feeds, copy=True):
        """Host-built step rows: feeds = [(slot, new_token_ids (1 or 2),
        first_position)]; every other row is a dummy into the trash slot.
        Returns the rows of each feed's last token.  copy=False: the pinned
        host rows only (the captured step graph copies them itself)."""
        Tm = self.Tmax
        ids = self.ids_h.numpy()
        meta = self.meta_h.numpy()
        ids[:] = 0
        slots = np.arange(self.M, dtype=np.int32) // 2
        meta[0] = Tm - 1           # dummy rows -> trash position
        meta[1] = slots
        meta[2] = 1                # dummy rows attend one key
        meta[3] = 1
        last = []
        for slot, toks, p0 in feeds:
            n = len(toks)
            if n > 2:
                raise ValueError("a feed carries at most 2 new tokens")
            if p0 + n > Tm - 1:
                raise ValueError("decoder prefix exceeds session max_tgt %d" % (Tm - 1))
            r0 = 2 * slot + (2 - n)
            for k in range(n):
                ids[r0 + k] = int(toks[k])
                meta[0, r0 + k] = p0 + k
                meta[2, r0 + k] = p0 + k + 1
                meta[3, r0 + k] = max(int(self.src_len[slot]), 1)
            last.append(2 * slot + 1)
        if copy:
            self.ids_t.copy_(self.ids_h, non_blocking=True)
            self.meta_t.copy_(self.meta_h, non_blocking=True)
        return last

    def step(self, feeds):
        """feeds: list of (slot, new_token_ids (1 or 2), first_position).
        Returns fp32 logits [len(feeds), V] (numpy) of each feed's LAST new
        token.  Slots not fed this step are dummies."""
        self._pe_guard()
        if self.use_graph:
            # the first call's eager warm-up reads the device row tables
            first = self.graph is None
            last = self._load_feeds(feeds, copy=first or not self._graph_copies)
            self._ensure_graph()
            self.graph.replay()
            if not self._graph_copies:
                self.logits_h.copy_(self.logits_t, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return self.logits_h.numpy()[last]
        last = self._load_feeds(feeds)
        self._run()
        self.logits_h.copy_(self.logits_t, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self.logits_h.numpy()[last]

    # ------------------------------------------------------------------
    # greedy decode with the grammar on device (csrc/decode_ops.hip)
    # ------------------------------------------------------------------
    N_STATE = 12
    LDMT = 640  # words per request of a rows graph's g_mt_rows (625 used: rows start 256-byte aligned)
    # ban rows per request of the '+ban' graphs (pitch constraints): one per
    # constrained track, and a request masks at most the vocabulary's three
    # tracks (track_0 .. track_2) -- rounded up to a power of two
    BAN_K = 4

    def _capture_grammar(self, gg):
        """Capture (decoder step + gg.step) into gg.graph.  The decoder step
        is warmed eagerly first (dummy rows only); the grammar kernel never
        runs outside the graph.  Returns the host seconds of the two phases."""
        t_a = time.perf_counter()
        self._load_feeds([])
        self._run()
        torch.cuda.synchronize()
        t_b = time.perf_counter()
        gs = torch.cuda.Stream()
        gs.wait_stream(torch.cuda.current_stream())
        gg.graph = _capture(gs, lambda: (self._run(), gg.step(self.logits_t, self.ids_t, self.meta_t)))
        torch.cuda.current_stream().wait_stream(gs)
        torch.cuda.synchronize()
        return t_b - t_a, time.perf_counter() - t_b

    def sampled_decode(self, spans, keep, reject, cls, *, eos, m0, lookahead=3, max_span=100,
                       t=1.0, p=None, seeds=None, bans=None, score=False, templates=None, bars=None,
                       chords=None):
        """The sampled infill loop (the reference's sampling(): softmax with
        temperature, then weighted_sampling or, with p, nucleus, and its
        redraws) on device: each step is one replay of the captured
        decoder step + csrc/decode_ops.hip grammar_sample_kernel, which draws
        from numpy's global MT19937 stream -- its state is handed to the
        device here and handed back to np.random afterwards, so the host
        stream continues exactly as if the host had drawn.  t, p: scalars or
        one value per span (p None = the whole distribution); the kernel
        reads them from a device buffer on every step, so calls with other
        values replay the same captured graph.
        seeds (one int in [0, 2**32) per span): span r draws from its own
        stream np.random.RandomState(seeds[r]) instead, built here on the host
        and copied to the device; the step then ends in the one-block-per-
        request form of the kernel (smer_grammar_sample_step_rows), the "rows"
        graph kept beside the unseeded "stream" one, and np.random is neither
        read nor written.  Other seeds replay that graph.
        bans, score, templates, bars, chords: as greedy_decode's; the scores are taken at
        t = 1 over the whole masked distribution, whatever t and p are.
        Returns a DecodeResult whose `fails` flag the ids whose redraws ran
        out."""
        if all(sp.done for sp in spans):  # nothing to draw: np.random stays untouched
            return DecodeResult.empty(len(spans), True, score)
        n = len(spans)
        ts = list(t) if isinstance(t, (list, tuple, np.ndarray)) else [t] * n
        ps = list(p) if isinstance(p, (list, tuple, np.ndarray)) else [p] * n
        if len(ts) != n or len(ps) != n:
            raise ValueError("sampled_decode: one t and one p per span")
        tp_h = np.empty((self.R, 2), dtype=np.float64)
        tp_h[:, 0], tp_h[:, 1] = 1.0, -1.0
        for r in range(n):
            tp_h[r, 0] = float(ts[r])
            tp_h[r, 1] = -1.0 if ps[r] is None else float(ps[r])
        if not (np.isfinite(tp_h).all() and (tp_h[:, 0] > 0).all() and
                all(q is None or float(q) >= 0 for q in ps)):
            raise ValueError("sampled_decode: t must be finite and > 0, p None or finite and >= 0")
        if seeds is not None:
            if len(seeds) != n:
                raise ValueError("sampled_decode: one seed per span")
            # a freshly seeded state: the key after init_genrand, position 624
            # (the first draw twists); slots past the spans are done and only
            # need some valid state
            mt_h = np.zeros((self.R, self.LDMT), dtype=np.uint32)
            for r in range(self.R):
                s0 = np.random.RandomState(int(seeds[r]) if r < n else 0).get_state()
                mt_h[r, :624] = s0[1]
                mt_h[r, 624] = int(s0[2])
        else:
            st0 = np.random.get_state()
            if st0[0] != "MT19937":
                raise RuntimeError("sampled_decode: np.random is not MT19937")
            mt_h = np.empty(625, dtype=np.uint32)
            mt_h[:624] = st0[1]
            mt_h[624] = int(st0[2])
        res = self._grammar_decode(spans, keep, cls, eos=eos, m0=m0, lookahead=lookahead, max_span=max_span,
                                   sampler=_Sampler(reject, mt_h, tp_h, seeds is not None), bans=bans,
                                   score=score, templates=templates, bars=bars, chords=chords)
        if seeds is None:  # the stream goes on where the device left it
            m = self._greedy.bufs["g_mt"].cpu().numpy().view(np.uint32)
            np.random.set_state(("MT19937", m[:624].copy(), int(m[624]), st0[3], st0[4]))
        return res._replace(ids=[[x & 0xFFFF for x in q] for q in res.ids],
                            fails=[[(x >> 16) & 1 for x in q] for q in res.ids])

    def greedy_decode(self, spans, keep, cls, *, eos, m0, lookahead=3, max_span=100, bans=None,
                      score=False, templates=None, bars=None, chords=None):
        """Run the greedy infill loop of `spans` (generation._Span, one per
        request slot 0..len-1, freshly started, sources prefilled) entirely
        on device: each step is one replay of the captured decoder step +
        grammar kernel; the host only polls the live count, `lookahead`
        steps behind.  Returns a DecodeResult; the caller replays the ids
        through its host spans.
        bans (pitch constraints): per span None or (ban_of_mask row: the ban
        row of each mask, -1 for none; bit rows uint32 [k <= BAN_K, 16]: bit v
        of row j set = token v banned).  With any span constrained the call
        replays the '+ban' graph of its mode (_GrammarGraph); both tables are
        device data refreshed per call, so other constraints replay that
        graph.  None (or all None): the graphs without that node, as ever.
        score: the call replays the '+score' graph of its mode (after '+ban',
        if constrained) and the result's `logp` holds, per request, the float64
        log-probabilities of its emitted ids (generation.token_logprobs at each
        id, t = 1, the whole masked distribution).  Without it: the graphs
        without those nodes, as ever.
        templates (infill templates): per span None or its rows, one per mask:
        None, or the items of the span's opening (a token id, or ops.TPL_PITCH),
        at most ops.TPL_LEN of them.  With any span templated the call replays
        the '+tpl' graph of its mode (after '+ban', before '+score'), whose
        extra node (smer_logits_template) forces the items from a tape that is
        device data refreshed per call: other templates replay that graph, and
        a span without one gets an all-free tape.  None (or all None): the
        graphs without that node, as ever.
        bars (the bar clock): per span its bar length in sixteenths, 0 for a
        span without a clock.  With any span clocked the call replays the
        '+bar' graph of its mode (after '+ban', before '+tpl'), whose extra
        node (smer_bar_clock) sits between the score stage and the template
        kernel; the lengths and the unit table are device data refreshed per
        call, and the clock words are zeroed per call.  None: the graphs
        without that node, as ever (generation passes None when no request
        sets fill_bar; a list of zeros runs the node on rows it leaves alone,
        which is how tools/barclock_bench.py prices it).
        chords (chord-following infill): per span None or (L: the bar's length in
        sixteenths, 1..CHORD_POS; the positions' table int8 [masks, CHORD_POS]: the
        bit row that governs each position of each mask's bar, -1 for none; bit
        rows uint32 [k <= CHORD_ROWS, 16]).  Needs `bars` (zeros will do: the
        node reads the clock's words).  With any span chorded -- or a list of
        None, which runs the node on all-free tables -- the call replays the
        '+bar+chord' graph of its mode, whose extra node (smer_chord_ban) sits
        between the clock and the template kernel; the three tables are the
        graph's own buffers refreshed per call, so another progression replays
        that graph.  None: the graphs without that node, as ever."""
        return self._grammar_decode(spans, keep, cls, eos=eos, m0=m0, lookahead=lookahead,
                                    max_span=max_span, bans=bans, score=score, templates=templates,
                                    bars=bars, chords=chords)

    def _grammar_decode(self, spans, keep, cls, *, eos, m0, lookahead, max_span, sampler=None, bans=None,
                        score=False, templates=None, bars=None, chords=None):
        """greedy_decode, or with `sampler` (a _Sampler) sampled_decode."""
        R = len(spans)
        if R > self.R:
            raise ValueError("more spans than session slots")
        self._pe_guard()
        # mask-target table capacity: a power of two >= 16, so calls whose
        # requests have different mask counts replay the same captured graph
        # (a capture costs ~10 ms; the kernels read the table by its row
        # stride, which is the capacity)
        need = max(1, max(s.n_masks for s in spans))
        nm = 16
        while nm < need:
            nm *= 2
        cap = self.Tmax
        st = np.zeros((self.R, self.N_STATE), dtype=np.int32)
        tg = np.zeros((self.R, nm), dtype=np.int8)
        from .generation import _target_code, unit_table  # late import: generation imports decode
        feeds = []
        for r, sp in enumerate(spans):
            st[r, 2] = 1                      # this_in = [m_0]
            st[r, 4] = sp.n_masks
            st[r, 5] = 1 if sp.done else 0
            st[r, 6] = int(bool(sp.no_whole))
            for k, t in enumerate(sp.mask_target[:nm]):
                tg[r, k] = _target_code(t)
            if not sp.done:
                st[r, 0] = 1                  # m_0 is fed at position 0 below
                feeds.append((r, [m0], 0))
        st[R:, 5] = 1
        if not feeds:
            return DecodeResult.empty(R, sampler is not None, score)
        use_ring = os.environ.get("SMER_GRAMMAR_RING", "1") != "0" or sampler is not None
        # one captured graph per mode, side by side: a process that alternates
        # between greedy, unseeded and seeded calls replays, never recaptures
        mode = "greedy" if sampler is None else "rows" if sampler.per_request else "stream"
        gkey = (nm, int(max_span), int(eos), int(m0), int(lookahead), use_ring, keep.shape, cls.shape,
                mode)
        # pitch constraints: a graph of its own per mode (mode + "+ban", the
        # ban kernel in front of the grammar kernel); a call without any
        # replays the graphs above, which never contain that node
        ban = None
        if bans is not None and any(b is not None for b in bans):
            if len(bans) != R:
                raise ValueError("one bans entry (or None) per span")
            K = self.BAN_K
            bm_h = np.full((self.R, nm), -1, dtype=np.int8)
            bb_h = np.zeros((self.R, K, ops.BAN_WORDS), dtype=np.uint32)
            for r, b in enumerate(bans):
                if b is None:
                    continue
                row = np.asarray(b[0], dtype=np.int64)[:nm]
                bits = np.asarray(b[1], dtype=np.uint32).reshape(-1, ops.BAN_WORDS)
                if len(bits) > K or (len(row) and not -1 <= row.min() <= row.max() < len(bits)):
                    raise ValueError("bans: at most %d ban rows per request, indices -1 .. rows - 1" % K)
                bm_h[r, :len(row)] = row
                bb_h[r, :len(bits)] = bits
            ban = (bm_h, bb_h)
            gkey += (K,)
        gname = mode if ban is None else mode + "+ban"
        # the bar clock: a graph of its own again, whose lengths, unit table and
        # clock words are its own buffers; a call without any replays the
        # graphs that never held the node
        bar = None
        if bars is not None:
            if len(bars) != R:
                raise ValueError("one bars entry per span")
            if keep.shape[1] > 512:
                raise ValueError("bars: the device path serves vocabularies up to 512 tokens")
            bl_h = np.zeros(self.R, dtype=np.int32)
            bl_h[:R] = [int(x) for x in bars]
            if bl_h.min() < 0 or bl_h.max() > 255:
                raise ValueError("bars: a bar length is 0 (no clock) or 1..255 sixteenths")
            bar = (bl_h, np.array(unit_table(spans[0].v), dtype=np.uint8))  # (a writable copy: the table is read-only)
            gname += "+bar"
            gkey += ("bar",)
        # chord-following infill: a graph of its own after the clock, whose three
        # tables are its own buffers; a call without any replays the graphs that
        # never held the node
        chord = None
        if chords is not None:
            if len(chords) != R:
                raise ValueError("one chords entry (or None) per span")
            if bar is None:
                raise ValueError("chords: the chord node reads the bar clock (pass bars, zeros will do)")
            cl_h = np.zeros(self.R, dtype=np.int32)
            ca_h = np.full((self.R, nm, ops.CHORD_POS), -1, dtype=np.int8)
            cb_h = np.zeros((self.R, ops.CHORD_ROWS, ops.BAN_WORDS), dtype=np.uint32)
            for r, ch in enumerate(chords):
                if ch is None:
                    continue
                at = np.asarray(ch[1], dtype=np.int8).reshape(-1, ops.CHORD_POS)[:nm]
                bits = np.asarray(ch[2], dtype=np.uint32).reshape(-1, ops.BAN_WORDS)
                if not 1 <= int(ch[0]) <= ops.CHORD_POS or len(bits) > ops.CHORD_ROWS or \
                        (at.size and not -1 <= at.min() <= at.max() < len(bits)):
                    raise ValueError("chords: a bar of 1..%d sixteenths, at most %d bit rows, indices -1 .. rows - 1"
                                     % (ops.CHORD_POS, ops.CHORD_ROWS))
                cl_h[r] = int(ch[0])
                ca_h[r, :len(at)] = at
                cb_h[r, :len(bits)] = bits
            chord = (cl_h, ca_h, cb_h)
            gname += "+chord"
            gkey += ("chord", ops.CHORD_POS, ops.CHORD_ROWS)
        # infill templates: once more a graph of its own, whose tape is device
        # data; a call without any replays the graphs that never held the node
        tape = None
        if templates is not None and any(x is not None for x in templates):
            if len(templates) != R:
                raise ValueError("one templates entry (or None) per span")
            if keep.shape[1] > 512:
                raise ValueError("templates: the device path serves vocabularies up to 512 tokens")
            tape = np.full((self.R, nm, ops.TPL_LEN), ops.TPL_FREE, dtype=np.int16)
            for r, rows in enumerate(templates):
                for k, row in enumerate(rows or ()):
                    if row is None or not len(row):
                        continue
                    if k >= nm or len(row) > ops.TPL_LEN:
                        raise ValueError("templates: at most %d rows of at most %d items per request"
                                         % (nm, ops.TPL_LEN))
                    tape[r, k, :len(row)] = row
            gname += "+tpl"
            gkey += ("tpl", ops.TPL_LEN)
        if score:  # take scores: again a graph of its own, with buffers of its own
            if keep.shape[1] > 512:
                raise ValueError("score: the device path scores vocabularies up to 512 tokens")
            gname += "+score"
            gkey += ("score",)
        inputs = (st, tg, keep, cls, self.src_len, ban, sampler, tape, bar, chord)
        gg = self._graphs.get(gname)
        if gg is not None and gg.key == gkey:
            # the captured step + grammar graph of an earlier call with the
            # same shapes: refresh its inputs in place and replay
            t_b = time.perf_counter()
            self.eng.weights(self.dt)  # re-casts the bf16 weights in place if they moved
            gg.load(*inputs)
            torch.cuda.synchronize()
            warm_s, capture_s = 0.0, time.perf_counter() - t_b
        else:
            gg = self._greedy = None
            self._graphs.pop(gname, None)  # a stale graph's buffers go before the new ones are made
            gg = _GrammarGraph(self, gkey, mode, nm, keep.shape, cls.shape, eos=eos, m0=m0,
                               lookahead=lookahead, max_span=max_span, use_ring=use_ring,
                               ban=ban is not None, score=score, tpl=tape is not None, bar=bar is not None,
                               chord=chord is not None)
            gg.load(*inputs)
            warm_s, capture_s = self._capture_grammar(gg)
            self._graphs[gname] = gg
        self._greedy = gg  # the graph of this call
        t_c = time.perf_counter()
        self._load_feeds(feeds)
        max_steps = max([s.n_masks for s in spans] + [0]) * (max_span + 1) + 2
        graph, rv = gg.graph, gg.rv
        inflight = []
        events = []
        steps = None
        issued = 0
        ev_start = torch.cuda.Event(enable_timing=True)
        ev_start.record()
        while steps is None:
            if len(inflight) > lookahead or (issued >= max_steps and inflight):
                j, ev, slot = inflight.pop(0)
                ev.synchronize()
                if rv[slot] == 0:
                    steps = j + 1
                    break
                continue
            if issued >= max_steps:
                raise RuntimeError("greedy_decode: no convergence within %d steps" % max_steps)
            graph.replay()
            slot = issued % len(rv)
            if not use_ring:
                gg.ring[slot:slot + 1].copy_(gg.bufs["g_alive"], non_blocking=True)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
            inflight.append((issued, ev, slot))
            issued += 1
        torch.cuda.synchronize()
        self.phase_s = {"warm_s": warm_s, "capture_s": capture_s, "loop_s": time.perf_counter() - t_c}
        st = gg.bufs["g_state"].cpu().numpy()
        out = gg.bufs["g_out"].cpu().numpy()
        ids = [out[r, :min(int(st[r, 7]), cap)].tolist() for r in range(R)]
        logp = None
        if score:
            lp = gg.bufs["g_logp"].cpu().numpy()
            logp = [lp[r, :len(ids[r])].copy() for r in range(R)]
        return DecodeResult(ids, steps, st[:R, 8].copy(), [ev_start.elapsed_time(e) for e in events[:steps]],
                            None, logp)

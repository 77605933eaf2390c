"""Infill variations: several decodes of one encoded source.

Kernel tests: the grouped decode cross attention (csrc/attention.hip
attn_decode_shared_kernel, smer_attn_decode_shared / _shared_qln) against
the per-row entry points given a row_req whose rows point at the same slot,
bit for bit.  Model tests: generation_batch(variations=...) /
generation_all(variations=n) against the same calls on the expanded request
list: tokens, redraw log lines, np.random state, token and step counts."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']
bf = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------
# kernel tests
# ---------------------------------------------------------------------------
def _layout(cap, G, seed):
    """Rows, their key counts and slots, and the group table of one launch:
    groups of 1, 2, 3, 5 and 2G+1 rows with random key counts; a group laid
    out like a session (even rows one key, odd rows live); a group of one-key
    rows; groups at 37 keys, at the full capacity and at capacity - 1.  Two
    rows in front, one between the groups and two at the end belong to no
    group (their slot is the NaN-filled spare one)."""
    rng = np.random.default_rng(seed)
    groups = []
    for n in (1, 2, 3, 5, 2 * G + 1):
        groups.append([int(x) for x in rng.integers(1, cap + 1, n)])
    live = int(rng.integers(2, cap + 1))
    groups.append([1 if i % 2 == 0 else live for i in range(8)])
    groups.append([1] * (G + 2))
    groups.append([37, 1, 37])
    groups.append([cap, 5, cap, 1, cap])
    groups.append([cap - 1, cap - 1])
    spare = len(groups)
    nk, req, tab = [1, 3], [spare, spare], []
    for g, ks in enumerate(groups):
        if g == 4:  # a stray row between two groups
            nk.append(2)
            req.append(spare)
        tab.append((len(nk), len(ks)))
        nk += ks
        req += [g] * len(ks)
    nk += [1, min(cap, 9)]
    req += [spare, spare]
    in_group = np.zeros(len(nk), dtype=bool)
    for f, n in tab:
        in_group[f:f + n] = True
    return (np.array(nk, dtype=np.int32), np.array(req, dtype=np.int32),
            np.array(tab, dtype=np.int32), in_group, spare + 1)


def _cache(n_slots, H, cap, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = torch.randn(n_slots, 2, H, cap, D, generator=g).to(bf)
    c[n_slots - 1] = float("nan")  # the slot no group uses
    return c.to(dev)


@pytest.mark.parametrize("cap", [40, 600, 2100])
@pytest.mark.parametrize("D", [32, 64])
def test_shared_decode_attention_plain_is_the_per_row_kernel(cap, D):
    from smer_music_generation_amd import ops as O
    H = 2
    nk, req, tab, in_group, n_slots = _layout(cap, O.DEC_SHARED_G, seed=cap + D)
    M = len(nk)
    cache = _cache(n_slots, H, cap, D, seed=1)
    g = torch.Generator(device="cpu").manual_seed(2)
    q = torch.randn(M, H * D, generator=g).to(bf).to(dev)
    nk_t, req_t, tab_t = (torch.from_numpy(a).to(dev) for a in (nk, req, tab))
    kw = dict(H=H, D=D, row_stride=D, req_stride=2 * H * cap * D, head_stride=cap * D,
              scale=1.0 / np.sqrt(D))
    vc = cache.view(-1)[H * cap * D:]
    ref = torch.full((M, H * D), float("nan"), dtype=bf, device=dev)
    O.attn_decode(q, cache, vc, req_t, nk_t, ref, **kw)
    got = torch.full((M, H * D), float("nan"), dtype=bf, device=dev)
    O.attn_decode_shared(q, cache, vc, req_t, nk_t, tab_t, got, **kw)
    torch.cuda.synchronize()
    ing = torch.from_numpy(in_group).to(dev)
    assert torch.isfinite(ref[ing].float()).all() and torch.isfinite(got[ing].float()).all()
    bad = (got[ing].view(torch.int16) != ref[ing].view(torch.int16)).any(dim=1)
    print("rows differing: %d of %d" % (int(bad.sum()), int(ing.sum())))
    assert torch.equal(got[ing].view(torch.int16), ref[ing].view(torch.int16))
    assert torch.isnan(got[~ing].float()).all()  # rows of no group: the canary


@pytest.mark.parametrize("cap,dm", [(40, 512), (600, 512), (2100, 512), (40, 768)])
def test_shared_decode_attention_with_query_prologue_is_the_per_row_kernel(cap, dm):
    from smer_music_generation_amd import ops as O
    H, D = 8, 64
    nk, req, tab, in_group, n_slots = _layout(cap, O.DEC_SHARED_G, seed=cap + dm)
    M = len(nk)
    cache = _cache(n_slots, H, cap, D, seed=3)
    g = torch.Generator(device="cpu").manual_seed(4)
    y = (torch.randn(M, dm, generator=g) * 2).to(bf).to(dev)
    gam, bet = torch.randn(dm, generator=g).to(dev), torch.randn(dm, generator=g).to(dev)
    wq = (torch.randn(H * D, dm, generator=g) / np.sqrt(dm)).to(bf).to(dev)
    bq = (torch.randn(H * D, generator=g) * 0.1).to(dev)
    nk_t, req_t, tab_t = (torch.from_numpy(a).to(dev) for a in (nk, req, tab))
    kw = dict(H=H, D=D, row_stride=D, req_stride=2 * H * cap * D, head_stride=cap * D, scale=0.125)
    vc = cache.view(-1)[H * cap * D:]

    def nan(w):
        return torch.full((M, w), float("nan"), dtype=bf, device=dev)
    ref, xref, got, xgot = nan(H * D), nan(dm), nan(H * D), nan(dm)
    O.attn_decode_qln(y, gam, bet, wq, bq, cache, vc, req_t, nk_t, ref, x_out=xref, **kw)
    O.attn_decode_shared_qln(y, gam, bet, wq, bq, cache, vc, req_t, nk_t, tab_t, got, x_out=xgot, **kw)
    torch.cuda.synchronize()
    ing = torch.from_numpy(in_group).to(dev)
    for a in (ref, xref, got, xgot):
        assert torch.isfinite(a[ing].float()).all()
    bad = (got[ing].view(torch.int16) != ref[ing].view(torch.int16)).any(dim=1)
    print("rows differing: %d of %d" % (int(bad.sum()), int(ing.sum())))
    assert torch.equal(got[ing].view(torch.int16), ref[ing].view(torch.int16))
    assert torch.equal(xgot[ing].view(torch.int16), xref[ing].view(torch.int16))
    assert torch.isnan(got[~ing].float()).all() and torch.isnan(xgot[~ing].float()).all()


# ---------------------------------------------------------------------------
# model tests
# ---------------------------------------------------------------------------
TAKES = [3, 1, 2]
T3, P3 = [1.0, 0.7, 1.3], [None, 0.9, 0.5]
_MODELS = {}
_RUNS = {}


def _micro(golden_dir, precision):
    from smer_music_generation_amd.model import ScoreTransformer
    z = np.load(os.path.join(golden_dir, "forward_train_micro.npz"))
    c = json.load(open(os.path.join(golden_dir, "forward_train_micro.json")))["config"]
    m = ScoreTransformer(309, c["d_model"], c["nhead"], c["num_encoder_layers"],
                         c["num_decoder_layers"], c["dim_feedforward"], c["max_seq_length"], 0.0,
                         0.0, precision=precision)
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    sd["pos_enc.pe"] = m.pos_enc.pe.clone()
    m.load_state_dict(sd)
    return m.to(dev)


def _model(golden_dir, name):
    """'micro' (golden weights, D = 32: bf16 takes the plain grouped kernel,
    fp32 the ungrouped paths) or 'wide' (seeded random d_model 512, 8 heads:
    bf16 takes the query-prologue form); built once per module."""
    if name not in _MODELS:
        if name == "micro":
            _MODELS[name] = _micro(golden_dir, "bf16")
        else:
            from smer_music_generation_amd.model import ScoreTransformer
            torch.manual_seed(0)
            _MODELS[name] = ScoreTransformer(309, 512, 8, 1, 1, 512, 2400, 0.0, 0.0).to(dev)
    return _MODELS[name]


def _requests(golden_dir, n=3):
    from smer_music_generation_amd.synth import synth_events
    g = json.load(open(os.path.join(golden_dir, "infill_micro.json")))
    reqs = [(synth_events(60 + i, n_bars=6 + i, n_tracks=3), [i % 3], [2, 3] if i % 2 else [4])
            for i in range(n)]
    return reqs, g["all_controls"]


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _rng_state():
    st = np.random.get_state()
    return st[1].copy(), int(st[2])


def _same(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0])


def _expand(xs, takes):
    return [x for x, n in zip(xs, takes) for _ in range(n)]


def _flat(out, nested):
    if nested:
        out = [o for takes in out for o in takes]
    return [([str(x) for x in o[0]], o[1], o[2]) for o in out]


def _batch(m, v, reqs, ctl, takes, *, expanded, seed=31, t=T3, p=P3, **kw):
    """One generation_batch call, either with variations=takes or on the
    expanded list: (flat results, log lines, RNG state, tokens, steps, stats)."""
    from smer_music_generation_amd import generation as G
    rq = [(list(e), tr, b) for e, tr, b in reqs]
    np.random.seed(seed)
    lg = _Log()
    if expanded:
        out, st = G.generation_batch(m, _expand(rq, takes), v, ctl, logger=lg, t=_expand(t, takes),
                                     p=_expand(p, takes), return_stats=True, **kw)
    else:
        out, st = G.generation_batch(m, rq, v, ctl, logger=lg, t=t, p=p, variations=takes,
                                     return_stats=True, **kw)
        assert [len(o) for o in out] == list(takes)
    return _flat(out, not expanded), lg.lines, _rng_state(), st["tokens"], st["steps"], st


def _expanded_ref(golden_dir, name, takes=TAKES, **kw):
    """The expanded-list run of a configuration, computed once and shared."""
    from smer_music_generation_amd.vocab import WordVocab
    key = (name, tuple(takes), tuple(sorted(kw.items())))
    if key not in _RUNS:
        reqs, ctl = _requests(golden_dir)
        _RUNS[key] = _batch(_model(golden_dir, name), WordVocab(0, CTRL), reqs, ctl, takes,
                            expanded=True, **kw)
    return _RUNS[key]


def _assert_same_run(a, b):
    assert a[0] == b[0]
    assert a[1] == b[1]
    assert _same(a[2], b[2])
    assert a[3:5] == b[3:5] and a[3] > 0


@pytest.mark.parametrize("name,kw", [
    ("micro", dict(greedy=False)),
    ("wide", dict(greedy=False)),
    ("micro", dict(greedy=False, precision="fp32")),
    ("wide", dict(greedy=False, device_grammar=False)),
    ("micro", dict(greedy=True)),
], ids=["micro-bf16", "wide-bf16", "micro-fp32", "wide-hostloop", "micro-greedy"])
def test_batch_variations_equal_the_expanded_list(golden_dir, name, kw, monkeypatch):
    """variations=[3, 1, 2] against the expanded 6-request list, with the
    grouped cross-attention kernels switched on (bf16; the default, per-row
    kernels through the source indirection, is
    test_default_and_switch_off_run_the_per_row_kernels below)."""
    from smer_music_generation_amd import generation as G
    from smer_music_generation_amd.vocab import WordVocab
    m, v = _model(golden_dir, name), WordVocab(0, CTRL)
    reqs, ctl = _requests(golden_dir)
    if kw.get("precision") == "fp32":
        kw = dict(kw, seed=32)  # (seed 31's expanded fp32 run samples a stray m_0)
    try:
        want = _expanded_ref(golden_dir, name, **kw)
        G.clear_decode_sessions(m)
        monkeypatch.setenv("SMER_DECODE_SHARED", "1")
        got = _batch(m, v, reqs, ctl, TAKES, expanded=False, **kw)
        _assert_same_run(got, want)
        # prefill and session shape
        st = got[5]
        S = max(len(G._prepare(list(e), v, tr, b)[0]) for e, tr, b in reqs)
        assert st["sources"] == 3 and st["prefill_rows"] == 3 * S
        assert want[5]["sources"] == 6 and want[5]["prefill_rows"] == 6 * S
        sess = [s for s in G._BATCH_SESSIONS.values() if s.model is m and s.R == 6 and s.NS == 3]
        assert len(sess) == 1
        assert sess[0].cross_kv[0].shape[0] == 3 and sess[0].self_kv[0].shape[0] == 6
        if kw.get("precision") is None and kw.get("device_grammar", True):
            assert sess[0].plan.shared  # the grouped kernels ran
    finally:
        G.clear_decode_sessions(m)
        m.set_precision("bf16")


def test_takes_of_one_request_differ(golden_dir):
    """Request 2 (t = 1.3, two takes) on the 512-wide model: its takes are
    different draws of one stream."""
    want = _expanded_ref(golden_dir, "wide", greedy=False)
    assert want[0][4][0] != want[0][5][0]
    from smer_music_generation_amd.vocab import WordVocab
    reqs, ctl = _requests(golden_dir)
    got = _batch(_model(golden_dir, "wide"), WordVocab(0, CTRL), reqs, ctl, TAKES, expanded=False,
                 greedy=False)
    assert got[0][4][0] != got[0][5][0]


def test_plugin_variations_equal_the_batch_of_copies(golden_dir):
    from smer_music_generation_amd import generation as G
    from smer_music_generation_amd.vocab import WordVocab
    m, v = _model(golden_dir, "micro"), WordVocab(0, CTRL)
    reqs, ctl = _requests(golden_dir, 1)
    ev, tr, br = reqs[0]
    try:
        np.random.seed(9)
        want = G.generation_batch(m, [(list(ev), tr, br)] * 4, v, ctl, greedy=False, precision="fp32",
                                  t=0.8, p=0.9)
        st_want = _rng_state()
        m.set_precision("bf16")
        for fn in (G.generation_all, G.infill):
            np.random.seed(9)
            got = fn(m, list(ev), dev, v, None, ctl, tr, br, variations=4, t=0.8, p=0.9)
            assert isinstance(got, list) and len(got) == 4
            assert _flat(got, False) == _flat(want, False)
            assert _same(_rng_state(), st_want)
            assert m.precision == "bf16"  # the call's fp32 does not stick
        np.random.seed(10)
        one = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, t=0.8, p=0.9)
        st_one = _rng_state()
        np.random.seed(10)
        got1 = G.generation_all(m, list(ev), dev, v, None, ctl, tr, br, t=0.8, p=0.9, variations=1)
        assert isinstance(got1, list) and len(got1) == 1
        assert _flat(got1, False) == _flat([one], False)
        assert _same(_rng_state(), st_one)
    finally:
        m.set_precision("bf16")


@pytest.mark.parametrize("switch", ["1", None], ids=["grouped", "default"])
def test_other_splits_replay_the_same_captured_graph(golden_dir, switch, monkeypatch):
    """The binding is device data (per-row source index, group table): another
    split of the same (R, sources) replays the graph captured for the first."""
    from smer_music_generation_amd import generation as G
    from smer_music_generation_amd.vocab import WordVocab
    m, v = _model(golden_dir, "wide"), WordVocab(0, CTRL)
    reqs, ctl = _requests(golden_dir)
    wants = [_expanded_ref(golden_dir, "wide", takes=takes, greedy=False)
             for takes in ([3, 1, 2], [1, 3, 2])]
    G.clear_decode_sessions(m)
    if switch is None:
        monkeypatch.delenv("SMER_DECODE_SHARED", raising=False)
    else:
        monkeypatch.setenv("SMER_DECODE_SHARED", switch)
    graphs = []
    try:
        for takes, want in zip(([3, 1, 2], [1, 3, 2]), wants):
            got = _batch(m, v, reqs, ctl, takes, expanded=False, greedy=False)
            _assert_same_run(got, want)
            sess = [s for s in G._BATCH_SESSIONS.values() if s.model is m and s.R == 6 and s.NS == 3]
            assert len(sess) == 1 and sess[0].plan.shared == (switch == "1")
            graphs.append(sess[0]._greedy.graph)
    finally:
        G.clear_decode_sessions(m)
    assert graphs[1] is graphs[0]


@pytest.mark.parametrize("switch", ["0", None], ids=["off", "default"])
@pytest.mark.parametrize("name", ["micro", "wide"])
def test_default_and_switch_off_run_the_per_row_kernels(golden_dir, name, switch, monkeypatch):
    """SMER_DECODE_SHARED=0, and the default (the grouped kernels measured
    slower and ship off): the per-row kernels through the source indirection,
    still one memory per source; the expanded list's tokens and RNG state."""
    from smer_music_generation_amd import generation as G
    from smer_music_generation_amd.vocab import WordVocab
    m, v = _model(golden_dir, name), WordVocab(0, CTRL)
    reqs, ctl = _requests(golden_dir)
    want = _expanded_ref(golden_dir, name, greedy=False)
    G.clear_decode_sessions(m)
    if switch is None:
        monkeypatch.delenv("SMER_DECODE_SHARED", raising=False)
    else:
        monkeypatch.setenv("SMER_DECODE_SHARED", switch)
    try:
        got = _batch(m, v, reqs, ctl, TAKES, expanded=False, greedy=False)
        sess = [s for s in G._BATCH_SESSIONS.values() if s.model is m and s.NS == 3]
        assert len(sess) == 1 and not sess[0].plan.shared
        assert sess[0].cross_kv[0].shape[0] == 3
    finally:
        G.clear_decode_sessions(m)
    assert got[0] == want[0] and _same(got[2], want[2])

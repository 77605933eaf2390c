"""Infill call surface of the plugin (reference `generation.py`).

Same names, signatures, return values and error behaviour as the
reference: `model_generate` (209-225), `generation_all` (468-696),
`sampling` (41-95), `softmax_with_temperature` (28-30), `weighted_sampling`
(33-38), `nucleus` (11-25), `gen_nopeek_mask` (193-206), plus the wire
helpers (`mask_bar_and_track`, `restore_marked_input`, `fill_empty_bars`,
`change_controls`) and the north-star alias `infill = generation_all`.

Differences, all opt-in keywords with reference defaults:
  * `generation_all(..., use_kv_cache=True)`: decode through the KV-cached
    `DecodeSession` (one encoder pass per request) instead of re-running the
    full model per token; `use_kv_cache=False` is the reference algorithm.
  * `greedy=False`: True replaces `weighted_sampling` by argmax.
  * `generation_all(..., precision="fp32")`: the plugin call decodes in
    fp32 whatever precision the model trains in (bit-exact ids); None
    decodes at the model's own precision.
  * `generation_batch(...)`: many requests decoded in lockstep.
  * `t=1.0, p=None` on `generation_all` / `infill` / `generation_batch`: the
    temperature and nucleus threshold of the reference's `sampling()`, which
    its own `generation_all` never passes on.
  * `seed=None` on the same three: an int (or, batched, one per request)
    gives every request its own `np.random.RandomState(seed)` stream instead
    of the global `np.random` one, so its tokens depend on its seed and its
    logits alone (not on the batch around it), and `np.random` is left alone.
  * `pitches=None` on the same three: the MIDI note numbers a request (or
    each of its tracks) may use; the other pitch tokens are masked like a
    banned token class (`pitch_set` builds ranges and scales).
  * `logprobs=False, rank=False` on the same three: the log-probability of
    every drawn token (`token_logprobs`: t = 1, the whole masked
    distribution) and each take's sum in `stats`; `rank=True` orders the
    takes of `variations=` by their mean log-probability per token.
  * `score_infill(...)` / `score_batch(...)`: the same log-probabilities for
    GIVEN content (the bar that was there, an edited take, another
    checkpoint's take), teacher-forced: one full forward, no step loop.
  * `template=None` on `generation_all` / `infill` / `generation_batch`: the
    opening of a span is given -- token by token, or as ANY_PITCH, "a pitch of
    the model's choice" -- and the model writes the rest (`rhythm_template`
    keeps a bar's rhythm, `opening_template` its first tokens).
  * `fill_bar=False` on the same three: True makes every infilled note span
    fill its bar exactly (a clock in sixteenths follows the tokens drawn and
    masks what would pass the bar line or end the span beside it);
    `bar_units` and `bar_fill` are its public helpers.
  * `chords=None` on the same three: the harmony of the infilled bars, a
    pitch set per segment of a bar; the set that holds at a note's onset (the
    bar clock's position) masks the other pitches (`chord_tones` and
    `pitch_onsets` are its public helpers).
The grammar state machine, the -100 logit masking, the float64 softmax and
the numpy RNG consumption are the reference's, so with the same
`np.random` state the same token ids come out.
"""
from __future__ import annotations

import time
import weakref
from collections import namedtuple
from typing import NamedTuple

import numpy as np
import torch

from .decode import DecodeSession
from .durations import durations_for_events
from .ops import TPL_PITCH
from .wire import (change_controls, decoder_targets, fill_empty_bars, mask_bar_and_track,  # noqa: F401
                   mask_targets, restore_marked_input, track_names_of)


# --------------------------------------------------------------------------
# sampling (generation.py:11-95)
# --------------------------------------------------------------------------
def nucleus(probs, p, rng=np.random):
    probs /= (sum(probs) + 1e-5)
    sorted_probs = np.sort(probs)[::-1]
    sorted_index = np.argsort(probs)[::-1]
    csum = np.cumsum(sorted_probs)
    after = csum > p
    if sum(after) > 0:
        cand = sorted_index[:np.where(after)[0][0] + 1]
    else:
        cand = sorted_index[:]
    cp = np.array([probs[i] for i in cand])
    cp /= sum(cp)
    return rng.choice(cand, size=1, p=cp)[0]


def softmax_with_temperature(logits, temperature):
    e = np.exp(logits / temperature)
    return e / np.sum(e)


def weighted_sampling(probs, rng=np.random):
    # the reference's builtin sum() adds left to right from 0: the last
    # element of the (sequential) cumulative sum is that number exactly, in
    # 1/12 of the time; probs[argsort] holds np.sort's values (ties are
    # equal values), so one sort serves both.  `probs` is float64 here
    # (sampling() widens the logits before the softmax), so builtin sum()
    # adds float64 scalars under NumPy 1.x and 2.x alike: no promotion-rule
    # dependence; a float32 input is rejected rather than silently diverging
    if probs.dtype != np.float64:
        raise TypeError("weighted_sampling expects float64 probabilities")
    probs /= np.add.accumulate(probs)[-1]
    sorted_index = np.argsort(probs)[::-1]
    return _choice1(sorted_index, probs[sorted_index], rng)


def _choice1(a, p, rng=np.random):
    """rng.choice(a, size=1, p=p)[0] (rng: a RandomState, or the np.random
    module, whose functions are the global RandomState's methods), without
    its argument checks (a third of the per-token host time): NumPy's legacy
    `RandomState.choice` with replacement draws ONE `random_sample` and
    returns a[searchsorted(cdf / cdf[-1], u, side='right')], so the same
    uniform gives the same index and leaves the same generator state.  Any
    input its checks would reject (a negative or NaN entry, a sum off 1)
    goes to np.random.choice itself, so the errors are NumPy's own
    (tests/test_sampling.py compares the two on seeded streams)."""
    cdf = np.cumsum(p)
    total = cdf[-1]
    if not (abs(total - 1.0) <= 1e-9) or not (p >= 0.0).all():
        return rng.choice(a, size=1, p=p)[0]
    cdf /= total
    u = rng.random_sample(1)
    return a[cdf.searchsorted(u, side='right')][0]


_FLAG_NAMES = ("no_pitch", "no_duration", "no_rest", "no_whole_duration", "no_eos",
               "no_continue", "no_sep", "is_density", "is_polyphony", "is_occupation",
               "is_tensile", "no_control")


# --------------------------------------------------------------------------
# the tables of one vocabulary
# --------------------------------------------------------------------------
class _VocabTables(dict):
    """What the host path derives from ONE vocabulary, built on first use:
    (flags..) `allowed_ids`' keep rows, ('spec', code), ('grammar', controls),
    'pitch', 'units', 'reject', and 'midi', the MIDI number -> pitch id map.
    The vocabulary is held weakly (`owner`) and no entry refers to it: the
    tables die with it, and `_tables` serves them to that very object alone
    (another vocabulary at a reused address gets tables of its own)."""

    def __init__(self, vocab):
        super().__init__()
        store, key = _TABLES, id(vocab)

        def drop(ref):  # (closes over locals only: it may run while the interpreter shuts down)
            t = store.get(key)
            if t is not None and t.owner is ref:
                del store[key]
        self.owner = weakref.ref(vocab, drop)


_TABLES = {}  # id(vocab) -> _VocabTables, for the vocabularies that are alive


def _tables(vocab):
    t = _TABLES.get(id(vocab))
    if t is None or t.owner() is not vocab:
        t = _TABLES[id(vocab)] = _VocabTables(vocab)
    return t


def _table(vocab, key, build):
    """Entry `key` of the vocabulary's tables; build(vocab) makes it once."""
    t = _tables(vocab)
    hit = t.get(key)
    if hit is None:
        hit = t[key] = build(vocab)
    return hit


def _frozen(a):
    a.setflags(write=False)
    return a


def allowed_ids(vocab, **flags):
    """Boolean [V]: logits `sampling` keeps (others are masked).  The
    reference's `no_control` test (`i in dict.values()`) never matches
    (SURVEY Q1), so it is a no-op here too."""
    g = flags.get
    t, key = _tables(vocab), tuple(map(bool, map(g, _FLAG_NAMES)))  # (every draw comes here: no _table() detour)
    hit = t.get(key)
    if hit is None:
        hit = t[key] = _allowed_ids(vocab, g)
    return hit


def _allowed_ids(vocab, g):
    V = vocab.vocab_size
    keep = np.ones(V, dtype=bool)
    if g("no_pitch"):
        keep[vocab.pitch_indices] = False
    if g("no_duration"):
        keep[vocab.duration_only_indices] = False
    if g("no_continue"):
        keep[vocab.continue_index] = False
    if g("no_rest"):
        keep[vocab.rest_indices] = False
    if g("no_sep"):
        keep[vocab.sep_indices] = False
    if g("no_whole_duration"):
        keep[vocab.duration_only_indices[0]] = False
    if g("no_eos"):
        keep[vocab.eos_index] = False
    for flag, attr in (("is_density", "density_indices"), ("is_occupation", "occupation_indices"),
                       ("is_polyphony", "polyphony_indices"), ("is_tensile", "tensile_indices")):
        if g(flag):
            only = np.zeros(V, dtype=bool)
            only[getattr(vocab, attr)] = True
            keep &= only
    keep[vocab.program_indices + vocab.structure_indices + vocab.time_signature_indices +
         vocab.tempo_indices] = False
    return _frozen(keep)


class _AnyPitch:
    """The type of ANY_PITCH."""
    __slots__ = ()

    def __repr__(self):
        return "ANY_PITCH"


# A template item (`template=`): any pitch token, and only a pitch token.
ANY_PITCH = _AnyPitch()


def _pitch_row(vocab):
    m = np.zeros(vocab.vocab_size, dtype=bool)
    m[vocab.pitch_indices] = True
    return _frozen(m)


def _pitch_mask(vocab):
    """Boolean [V]: the pitch tokens."""
    return _table(vocab, "pitch", _pitch_row)


def _forced(x, vocab, item):
    """A template item applied to the masked row x (`masked_row` up to the
    clock ban, float64 or float32) ahead of the division by t.  A token id: 0.0
    at the token and -100.0 at every other entry.  TPL_PITCH: -100.0 at every
    entry that is no pitch token; the pitch entries keep what the grammar mask
    and the pitch ban gave them."""
    if item == TPL_PITCH:
        return np.where(_pitch_mask(vocab), x, x.dtype.type(-100.0))
    out = np.full_like(x, -100.0)
    out[item] = 0.0
    return out


def masked_row(logit, keep, clock_ban=None, force=None, vocab=None, dtype=np.float64):
    """THE masked row of a draw; every host path builds it here, in this
    order: 1. the float32 logits widened to `dtype`; 2. -100 wherever `keep`
    (boolean [V]: the state's grammar keep less the pitch ban, `_state_keep`)
    is False -- THE SCORE READS THIS ROW (`token_logprobs(logit, keep)`), so
    neither clock nor template shows in it; 3. -100 wherever the bar clock
    bans (clock_ban, boolean [V]); 4. the template item (force: a token id,
    TPL_PITCH or ANY_PITCH; needs vocab).  The division by t is the caller's.
    Steps 1-2 also take stacked rows [n, V]; a row that has passed them takes
    3-4 alone with keep=True (the greedy batched loop)."""
    x = np.where(keep, np.asarray(logit, dtype=np.float32).astype(dtype), dtype(-100.0))
    if clock_ban is not None:
        x[clock_ban] = -100.0
    if force is not None:
        x = _forced(x, vocab, TPL_PITCH if force is ANY_PITCH else int(force))
    return x


def sampling(logit, vocab, p=None, t=1.0, greedy=False, rng=np.random, ban=None, force=None, **flags):
    """`generation.py:41-95` with vectorised masking.  rng: the stream the
    draw comes from (np.random: the global one, as the reference).  ban
    (boolean [V], True = banned; None: nothing): `keep &= ~ban`, a banned
    token's logit is masked exactly as a masked class's is.  force (a template
    item: a token id, or ANY_PITCH; None: nothing): the masked row is
    rewritten by `_forced` before the softmax; the draw itself, and what it
    takes from rng, is the draw of any other row."""
    if isinstance(logit, torch.Tensor):
        logit = logit.squeeze().detach().cpu().numpy()
    keep = allowed_ids(vocab, **flags)
    if ban is not None:
        keep = keep & ~np.asarray(ban, dtype=bool)
    probs = softmax_with_temperature(masked_row(logit, keep, None, force, vocab), t)
    if greedy:
        return int(np.argmax(probs))
    if p is not None:
        return nucleus(probs, p, rng)
    return weighted_sampling(probs, rng)


def token_logprobs(logit, keep):
    """float64 [V]: the log of the distribution `sampling()` builds from the
    float32 row `logit` at t = 1, before any nucleus cut or redraw: x =
    masked_row(logit, keep) = where(keep, float64(float32(logit)), -100.0),
    x - logsumexp(x).  keep (boolean [V]) is what the draw used: `allowed_ids`
    of the grammar state, `& ~ban` under a pitch constraint.  The maximum is
    subtracted before the exp, so a row of large logits stays finite where
    the softmax itself overflows.  A masked entry scores from its -100 like
    any other."""
    x = masked_row(logit, np.asarray(keep, dtype=bool))
    m = np.max(x)
    return x - (m + np.log(np.sum(np.exp(x - m))))


def _check_score(logprobs, rank, variations):
    """Validated `logprobs` / `rank` of a call: both bools, rank only with
    variations.  Returns whether the call takes scores.  Raises ValueError;
    touches neither the model nor np.random."""
    for name, x in (("logprobs", logprobs), ("rank", rank)):
        if not isinstance(x, (bool, np.bool_)):
            raise ValueError("%s must be True or False (got %r)" % (name, x))
    if rank and variations is None:
        raise ValueError("rank=True orders the takes of a request: it needs variations")
    return bool(logprobs) or bool(rank)


def _rank_order(logps):
    """Take indices in descending mean log-probability per drawn token (sum /
    count; a take that drew nothing goes last), ties to the lower index."""
    mean = [float(np.sum(a)) / len(a) if len(a) else -np.inf for a in logps]
    return sorted(range(len(logps)), key=lambda k: (-mean[k], k))


def _per_request(x, n, one, name, what, here=None):
    """The 'one value, or one per request' rule of a keyword: x is one value
    for all n requests or a list, tuple or array of n; each goes through one().
    n None (the plugin call): a sequence is an error, one(x) comes back."""
    if isinstance(x, (list, tuple, np.ndarray)):
        if n is None:
            raise ValueError(here or "%s is one %s here" % (name, what))
        if len(x) != n:
            raise ValueError("%s: one %s, or one per request (%d)" % (name, what, n))
        return [one(y) for y in x]
    return one(x) if n is None else [one(x)] * n


def _check_tp(t, p, n=None):
    """Validated (t, p) of a call; with n, one pair per request (scalars are
    repeated, sequences must have n entries).  t finite and > 0; p None, or
    finite and >= 0.  Raises ValueError; draws nothing."""
    ts, ps = (_per_request(x, n, lambda y: y, "t and p", "value", here="t and p are scalars here")
              for x in (t, p))
    if n is None:
        ts, ps = [ts], [ps]
    out = []
    for a, b in zip(ts, ps):
        try:
            a = float(a)
            b = None if b is None else float(b)
        except (TypeError, ValueError):
            raise ValueError("t must be a number, p a number or None") from None
        if not (np.isfinite(a) and a > 0.0):
            raise ValueError("temperature t must be finite and > 0 (got %r)" % a)
        if b is not None and not (np.isfinite(b) and b >= 0.0):
            raise ValueError("nucleus threshold p must be None, or finite and >= 0 (got %r)" % b)
        out.append((a, b))
    return out[0] if n is None else out


def _check_variations(variations, n=None):
    """Validated take counts of a call: an int >= 1 (n None: the plugin call,
    returns it), or with n requests an int or one int per request (returns
    the list).  Raises ValueError; touches neither the model nor np.random."""
    def one(x):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError("variations must be an int >= 1 (got %r)" % (x,))
        return int(x)
    return _per_request(variations, n, one, "variations", "int")


SEED_MAX = 2 ** 32 - 1


def _check_seed(seed, n=None, takes=None):
    """Validated seeds of a call.  None stays None (the global np.random
    stream, today's behaviour); otherwise the list of effective seeds, one
    per request slot in the expanded order: an int in [0, 2**32 - 1] (n None:
    the plugin call), or with n requests an int for all of them or one int
    per request -- a None inside a sequence is an error, a call is seeded
    throughout or not at all.  takes (an int for the plugin call, else one
    count per request): take k (0-based) of a request seeded s draws from
    seed s + k, so it can be regenerated alone with seed=s + k, and s + takes
    - 1 must not exceed 2**32 - 1.  Derived seeds of different requests may
    coincide: keeping them apart is the caller's business.  Raises
    ValueError; touches neither the model nor np.random."""
    if seed is None:
        return None

    def one(x):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or \
                not 0 <= x <= SEED_MAX:
            raise ValueError("seed must be an int in [0, 2**32 - 1] (got %r)" % (x,))
        return int(x)
    seeds = _per_request(seed, n, one, "seed", "int")
    if n is None:
        seeds = [seeds]
    if takes is None:
        return seeds
    counts = [takes] * len(seeds) if isinstance(takes, (int, np.integer)) else list(takes)
    for s0, k in zip(seeds, counts):
        if s0 + k - 1 > SEED_MAX:
            raise ValueError("seed %d with %d variations: take seeds run past 2**32 - 1" % (s0, k))
    return [s0 + j for s0, k in zip(seeds, counts) for j in range(k)]


PITCH_MIN, PITCH_MAX = 21, 108  # the MIDI numbers of the pitch tokens p_21 .. p_108


def pitch_set(lo=None, hi=None, classes=None):
    """The sorted tuple of MIDI note numbers in [max(lo, 21), min(hi, 108)]
    whose pitch class n % 12 is in `classes` (None: all twelve), for
    `pitches=`: pitch_set(28, 60) a bass range, pitch_set(classes=(0, 2, 4, 5,
    7, 9, 11)) the C major scale.  An empty result raises ValueError."""
    a = PITCH_MIN if lo is None else max(int(lo), PITCH_MIN)
    b = PITCH_MAX if hi is None else min(int(hi), PITCH_MAX)
    cl = None if classes is None else {int(c) % 12 for c in classes}
    out = tuple(n for n in range(a, b + 1) if cl is None or n % 12 in cl)
    if not out:
        raise ValueError("pitch_set(%r, %r, %r) is empty" % (lo, hi, classes))
    return out


def _is_collection(x):
    return isinstance(x, (list, tuple, set, frozenset, range, np.ndarray))


def _midi_set(x, name):
    """The sorted tuple of the MIDI numbers of the collection x (`pitches=`, or a
    segment of `chords=`): every entry an int in [21, 108] (no bool, no float),
    and at least one.  Raises ValueError."""
    out = set()
    for e in (x.tolist() if isinstance(x, np.ndarray) else x):
        if isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, np.integer)) or \
                not PITCH_MIN <= e <= PITCH_MAX:
            raise ValueError("%s: every entry is an int in [%d, %d] (got %r)" % (name, PITCH_MIN, PITCH_MAX, e))
        out.add(int(e))
    if not out:
        raise ValueError("%s: an empty set allows no note" % name)
    return tuple(sorted(out))


def _check_pitches(pitches, tracks, n=None):
    """Validated pitch constraints of a call.  n None (the plugin call):
    `tracks` is its tracks_to_generate and the result None (unconstrained) or
    the effective {track number: sorted tuple of allowed MIDI numbers}: a
    collection (list, tuple, set, frozenset, range or array) of ints
    constrains every track of tracks_to_generate, a dict {track number:
    collection} the listed tracks only (a key that is not in
    tracks_to_generate is an error).  With n requests, `tracks` holds one
    tracks_to_generate per request and the result one such value per request:
    a list or tuple whose entries are all None, collections or dicts is the
    per-request form and must have n entries; anything else (a collection of
    ints, a dict) is one constraint applied to every request.  So a bare list
    of ints is always one pitch set for all requests, whatever its length,
    and [[60, 62, 64]] * n is that set spelled per request.  Every entry of a
    set is an int in [21, 108] (no bool, no float) and every set is
    non-empty.  Raises ValueError; touches neither the model nor np.random."""
    coll = _is_collection

    def one_set(x):
        if not coll(x):
            raise ValueError("pitches: a collection of MIDI note numbers, or a dict of them per "
                             "track (got %r)" % (x,))
        return _midi_set(x, "pitches")

    def one_request(x, trk):
        if x is None:
            return None
        trk = [int(t) for t in trk]
        if isinstance(x, dict):
            eff = {}
            for k, val in x.items():
                if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or \
                        int(k) not in trk:
                    raise ValueError("pitches: track %r is not in tracks_to_generate %r" % (k, trk))
                eff[int(k)] = one_set(val)
            return eff or None
        s = one_set(x)
        return {t: s for t in trk} or None

    if n is None:
        return one_request(pitches, tracks)
    if pitches is None:
        return [None] * n
    if isinstance(pitches, (list, tuple)) and len(pitches) > 0 and \
            all(x is None or isinstance(x, dict) or coll(x) for x in pitches):
        if len(pitches) != n:
            raise ValueError("pitches: one value, or one per request (%d)" % n)
        return [one_request(x, trk) for x, trk in zip(pitches, tracks)]
    return [one_request(pitches, trk) for trk in tracks]


def _request_bans(vocab, events, tracks_to_generate, bars_to_generate, allowed):
    """The ban rows of one request from its effective constraint `allowed`
    ({track number: allowed MIDI numbers}, or None): (ban_of_mask, rows), or
    None.  rows boolean [k, V], one per constrained track in ascending track
    number, True on every pitch token outside the track's set; ban_of_mask:
    per mask, in the order `mask_targets` builds (generation.py:488-492: for
    each bar, for each track, r, d, o, p, and t after the last track), the row
    of the mask's track or -1.  (Only an 'r' span can draw a pitch; the row
    rides on the track's other spans too, which never admit one.)"""
    if not allowed:
        return None
    order = sorted(allowed)
    midi = _table(vocab, "midi", lambda v: {int(v.index2char(i)[2:]): i for i in v.pitch_indices})
    rows = np.zeros((len(order), vocab.vocab_size), dtype=bool)
    for k, trk in enumerate(order):
        rows[k, vocab.pitch_indices] = True
        rows[k, [midi[n] for n in allowed[trk]]] = False
    names = track_names_of(events)
    of_mask = []
    for _ in bars_to_generate:
        for t in tracks_to_generate:
            k = order.index(int(t)) if int(t) in allowed else -1
            of_mask += [k] * (5 if names.index('track_%d' % t) == len(names) - 1 else 4)
    return of_mask, rows


def ban_bits(rows):
    """Boolean ban rows [k, V <= 512] as the device's bit rows uint32 [k, 16]:
    token v is bit v % 32 of word v // 32."""
    rows = np.asarray(rows, dtype=bool)
    pad = np.zeros((rows.shape[0], 512), dtype=bool)
    pad[:, :rows.shape[1]] = rows
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder='little')).view('<u4')


def gen_nopeek_mask(length):
    m = (torch.triu(torch.ones(length, length)) == 1).transpose(0, 1)
    return m.float().masked_fill(m == 0, float("-inf")).masked_fill(m == 1, 0.0)


def model_generate(model, src, tgt, device, return_weights=False):
    """`generation.py:209-225`: batch-1 full forward; logits [t, V] on CPU."""
    src = torch.as_tensor(src).clone().detach().unsqueeze(0).long().to(device)
    tgt = torch.tensor(tgt).unsqueeze(0).to(device)
    mask = gen_nopeek_mask(tgt.shape[1]).unsqueeze(0).to(device)
    with torch.no_grad():
        out, w = model.forward(src, tgt, src_key_padding_mask=None, tgt_key_padding_mask=None,
                               memory_key_padding_mask=None, tgt_mask=mask)
    if return_weights:
        return out.squeeze(0).to("cpu"), (w.squeeze(0).to("cpu") if w is not None else None)
    return out.squeeze(0).to("cpu")


# --------------------------------------------------------------------------
# the per-span grammar state machine (generation.py:528-687)
# --------------------------------------------------------------------------
N_GRAMMAR_STATES = 13


def _target_code(tc):
    """Control target of a mask: 'r' 0, 'd' 1, 'o' 2, 'p' 3, anything else
    't' 4 (the reference's `else: is_tensile`, generation.py:575-583)."""
    return {'r': 0, 'd': 1, 'o': 2, 'p': 3}.get(tc, 4)


def grammar_spec(v, code):
    """(sampling flags, redraw check, failure message) of grammar state
    `code`, built once per (vocab, code) (the per-token host replay of the
    device decode calls this for every emitted id)."""
    t = _tables(v)
    hit = t.get(("spec", code))
    if hit is None:
        hit = t["spec", code] = _grammar_spec(v, code)
    return hit


def _grammar_spec(v, code):
    """(sampling flags, redraw check, failure message) of grammar state
    `code` (generation.py:549-630):
    0 sep, 1 continue, 2/3 pitch, 4/5 rest (+no_whole), 6-9 first token of a
    d/o/p/t control span, 10 first token of a note span, 11/12 free.  The
    checks read the vocabulary's index lists, not the vocabulary (its tables
    must not keep it alive)."""
    rest, eos, pitch, dur = v.rest_indices, v.eos_index, v.pitch_indices, v.duration_only_indices
    if code == 0:
        return (dict(no_rest=True, no_sep=True, no_eos=True, no_whole_duration=True,
                     no_control=True),
                lambda i: i in rest or i == eos or i == dur[0], "in sep failed")
    if code == 1:
        return (dict(no_rest=True, no_sep=True, no_duration=True, no_continue=True,
                     no_eos=True, no_control=True),
                lambda i: i not in pitch, 'in continue failed')
    if code in (2, 3):
        return (dict(no_rest=True, no_sep=True, no_continue=True,
                     no_whole_duration=code == 3, no_eos=True, no_control=True),
                lambda i: i not in dur and i not in pitch, 'in pitch failed')
    if code in (4, 5):
        return (dict(no_pitch=True, no_rest=True, no_sep=True, no_continue=True,
                     no_whole_duration=code == 5, no_eos=True, no_control=True),
                lambda i: i not in dur, 'in rest failed')
    if 6 <= code <= 9:
        return {('is_density', 'is_occupation', 'is_polyphony', 'is_tensile')[code - 6]: True}, None, ''
    if code == 10:
        return (dict(no_duration=True, no_control=True), lambda i: i in dur, 'start failed')
    return dict(no_whole_duration=code == 12, no_control=True), None, ''


def _state_keep(vocab, code, ban=None):
    """Boolean [V]: what grammar state `code` keeps, with the pitch-ban row
    `ban` (boolean [V], or None) removed: the `keep` of `masked_row`."""
    keep = allowed_ids(vocab, **grammar_spec(vocab, code)[0])
    return keep if ban is None else keep & ~np.asarray(ban, dtype=bool)


def grammar_tables(vocab, all_controls):
    """Device tables of the greedy grammar kernel: keep uint8 [13, V]
    (allowed_ids of every state) and token classes cls uint8 [V]
    (1 continue, 2 pitch, 4 duration-only, 8 'sep', 16 'rest', 32 control).
    Built once per (vocabulary, control set); every call gets copies of its
    own (a few KB), as ever, so a caller that writes into one harms no other."""
    ctrl = tuple(sorted({int(c) for c in all_controls}))
    keep, cls = _table(vocab, ("grammar", ctrl), lambda v: _grammar_tables(v, ctrl))
    return keep.copy(), cls.copy()


def _grammar_tables(vocab, all_controls):
    V = vocab.vocab_size
    keep = np.stack([allowed_ids(vocab, **grammar_spec(vocab, c)[0])
                     for c in range(N_GRAMMAR_STATES)]).astype(np.uint8)
    cls = np.zeros(V, dtype=np.uint8)
    if getattr(vocab, "continue_index", None) is not None:
        cls[vocab.continue_index] |= 1
    cls[vocab.pitch_indices] |= 2
    cls[vocab.duration_only_indices] |= 4
    for i in range(V):
        ch = vocab.index2char(i)
        if ch == 'sep':
            cls[i] |= 8
        if ch == 'rest':
            cls[i] |= 16
    cls[[int(c) for c in all_controls]] |= 32
    return _frozen(keep), _frozen(cls)


# --------------------------------------------------------------------------
# the bar clock (`fill_bar=`): how much of its bar a note span has filled
# --------------------------------------------------------------------------
BAR_UNITS = {'whole': 16, 'half': 8, 'quarter': 4, 'eighth': 2, 'sixteenth': 1}  # in sixteenths


def _unit_row(vocab):
    u = np.zeros(vocab.vocab_size, dtype=np.uint8)
    for i in vocab.duration_only_indices:
        u[i] = BAR_UNITS.get(vocab.index2char(i), 0)
    return _frozen(u)


def unit_table(vocab):
    """uint8 [V]: the length of every token in sixteenths (BAR_UNITS for the
    duration tokens, 0 for every other token)."""
    return _table(vocab, "units", _unit_row)


def bar_units(events):
    """The length L of a bar of `events` in sixteenths: bar_duration /
    name_to_time['sixteenth'] of durations_for_events (16 for 4/4, 12 for 3/4
    and 6/8).  A length that is no integer in 1..255 raises ValueError."""
    try:
        name_to_time, _, _, bar_duration = durations_for_events(events)
        L = float(bar_duration) / float(name_to_time['sixteenth'])
    except (KeyError, IndexError, TypeError, ValueError, ZeroDivisionError):
        raise ValueError("fill_bar: the events carry no usable time signature") from None
    if not (np.isfinite(L) and L == int(L) and 1 <= L <= 255):
        raise ValueError("fill_bar: a bar of %r sixteenths (an integer in 1..255 is needed)" % (L,))
    return int(L)


class _BarClock:
    """The cursor of one note span in sixteenths (the `_Writer` rule of
    codec.py: consecutive duration tokens sum into one group, 'sep' rewinds by
    the previous group), and what it bans so that the span never passes the
    bar line and can end only on it.  T cursor, P the previous group's length,
    A the pending duration sum, G a duration group is open, S a 'sep' is
    pending.  cls: grammar_tables' class bits per token, units: unit_table.
    Pure: integers in, a boolean row out."""
    __slots__ = ("L", "cls", "units", "T", "P", "A", "G", "S")

    def __init__(self, L, cls, units):
        self.L, self.cls, self.units = int(L), np.asarray(cls), np.asarray(units)
        self.T = self.P = self.A = self.G = self.S = 0

    def reset(self):
        self.T = self.P = self.A = self.G = self.S = 0

    @property
    def base(self):
        return self.T - self.P if self.S else self.T

    @property
    def end(self):
        return self.base + self.A

    @property
    def cursor(self):
        """Where the span's cursor stands once an open group is closed (a
        'sep' that no group follows rewinds nothing)."""
        return self.end if self.G else self.T

    def advance(self, cls_bits, units):
        """Follow one emitted token: its class bits and its length."""
        if cls_bits & 4:  # a duration token: the group grows
            self.A += int(units)
            self.G = 1
            return
        if self.G:  # any other token first closes an open group (_Writer.flush)
            self.T, self.P = self.base + self.A, self.A
            self.A = self.S = self.G = 0
        if cls_bits & 8:
            self.S = 1

    def advance_id(self, idx):
        self.advance(int(self.cls[idx]), int(self.units[idx]))

    def banned(self, vocab):
        """Boolean [V]: the candidates the clock bans in its current state."""
        L, cls, units = self.L, self.cls, self.units
        base, end = self.base, self.end
        ban = np.zeros(vocab.vocab_size, dtype=bool)
        dur = (cls & 4) != 0
        ban[dur] = end + units[dur].astype(np.int64) > L
        if end >= L:  # each needs at least a sixteenth after it
            ban[(cls & (1 | 2 | 16)) != 0] = True
        if (base if self.G else self.T - self.P) >= L:
            ban[(cls & 8) != 0] = True
        if end != L:
            ban[(cls & 32) != 0] = True
            ban[vocab.eos_index] = True
        return ban


def bar_fill(vocab, tokens):
    """(final cursor, peak end) in sixteenths of one span's tokens (strings or
    ids; m_0 and <eos> count as any other non-duration token): where the
    `_Writer` rule leaves the cursor once the last group is closed, and the
    furthest a group reached on the way."""
    table = vocab._char2idx
    cls = np.zeros(vocab.vocab_size, dtype=np.uint8)
    cls[vocab.duration_only_indices] |= 4
    cls[vocab.sep_indices] |= 8
    ck = _BarClock(255, cls, unit_table(vocab))
    peak = 0
    for x in (tokens.tolist() if isinstance(tokens, np.ndarray) else tokens):
        ck.advance_id(table[x] if isinstance(x, str) else int(x))
        peak = max(peak, ck.end)
    return ck.cursor, peak


def _check_fill_bar(fill_bar, n=None):
    """Validated `fill_bar` of a call: a bool (n None: the plugin call), or
    with n requests a bool for all of them or one per request.  Raises
    ValueError; touches neither the model nor np.random."""
    def one(x):
        if not isinstance(x, (bool, np.bool_)):
            raise ValueError("fill_bar must be True or False (got %r)" % (x,))
        return bool(x)
    return _per_request(fill_bar, n, one, "fill_bar", "bool")


# --------------------------------------------------------------------------
# chord-following infill (`chords=`): the pitch set that holds at a note's onset
# --------------------------------------------------------------------------
CHORD_POS, CHORD_SETS = 64, 16  # the longest bar under chords= in sixteenths; distinct effective sets per request
_CHORD_KINDS = {'maj': (0, 4, 7), 'min': (0, 3, 7), 'dim': (0, 3, 6), 'aug': (0, 4, 8), '7': (0, 4, 7, 10),
                'maj7': (0, 4, 7, 11), 'min7': (0, 3, 7, 10)}


def chord_tones(root, kind='maj'):
    """The pitch classes of a chord, for pitch_set(classes=...): root is a pitch
    class or a MIDI number (taken mod 12), kind one of 'maj' 'min' 'dim' 'aug'
    '7' 'maj7' 'min7'.  chord_tones(5, 'maj') is F major: (5, 9, 0)."""
    if isinstance(root, (bool, np.bool_)) or not isinstance(root, (int, np.integer)):
        raise ValueError("chord_tones: root is an int (got %r)" % (root,))
    if kind not in _CHORD_KINDS:
        raise ValueError("chord_tones: kind is one of %s (got %r)" % (" ".join(sorted(_CHORD_KINDS)), kind))
    return tuple((int(root) + i) % 12 for i in _CHORD_KINDS[kind])


def pitch_onsets(vocab, tokens):
    """[(onset, midi), ...] of one span's tokens (strings or ids): every pitch
    token with the position in sixteenths from the bar line at which it sounds,
    by the `_BarClock` rule -- the clock's `end` before the token: a pitch first
    closes an open duration group and sounds where the next one starts, a pitch
    after 'sep' at the rewound position, the second pitch of a chord at the
    first one's."""
    table = vocab._char2idx
    cls = np.zeros(vocab.vocab_size, dtype=np.uint8)
    cls[vocab.duration_only_indices] |= 4
    cls[vocab.sep_indices] |= 8
    ck = _BarClock(255, cls, unit_table(vocab))
    pitch, out = _pitch_mask(vocab), []
    for x in (tokens.tolist() if isinstance(tokens, np.ndarray) else tokens):
        i = table[x] if isinstance(x, str) else int(x)
        if pitch[i]:
            out.append((ck.end, int(vocab.index2char(i)[2:])))
        ck.advance_id(i)
    return out


class _Chords(namedtuple("_Chords", "L at rows sets")):
    """The resolved `chords=` of one request: L the bar's length in sixteenths;
    at int8 [masks, CHORD_POS], the ban row that governs each position of each
    mask's bar (-1: none; only note spans carry any); rows boolean [k <=
    CHORD_SETS, V], True on every pitch token outside the row's effective set;
    sets, the sorted tuple of MIDI numbers of each row."""
    __slots__ = ()

    def row_at(self, mask_idx, end):
        """The ban row that governs a pitch drawn at clock value `end`, or -1."""
        if not 0 <= mask_idx < len(self.at):
            return -1
        return int(self.at[mask_idx, min(max(int(end), 0), min(self.L, CHORD_POS) - 1)])


def _mask_layout(events, tracks_to_generate, bars_to_generate):
    """(bar, track, first mask index) of every masked track-bar in the order
    `mask_targets` builds the masks (for each bar, for each track: r, d, o, p,
    and t after the last track), and the number of masks."""
    names = track_names_of(events)
    out, at = [], 0
    for b in bars_to_generate:
        for t in tracks_to_generate:
            out.append((int(b), int(t), at))
            at += 5 if names.index('track_%d' % t) == len(names) - 1 else 4
    return out, at


def _check_chords(chords, requests, allowed, vocab, n=None):
    """Validated `chords=` of a call: per request None or its `_Chords`.  n None
    (the plugin call): one value; with n requests one value for all of them (None
    or a dict) or a list or tuple of n.  requests: (events, tracks_to_generate,
    bars_to_generate) per request; allowed: `_check_pitches`' value per request.
    One request's value is a dict: a key is a bar number of bars_to_generate
    (every track of tracks_to_generate) or a (bar, track) tuple (that track only,
    replacing the bar's entry for it); a value is a sequence of segments (start,
    pitches): start an int in sixteenths from the bar line, the first 0, strictly
    ascending, below L = bar_units(events) <= 64; pitches a collection of MIDI
    numbers in [21, 108].  The effective set of a segment is its set intersected
    with the track's `pitches=` set, if it has one; it must not be empty, and a
    request has at most CHORD_SETS distinct ones.  Raises ValueError; touches
    neither the model nor np.random."""
    def is_int(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))

    def one_request(x, req, alw):
        if x is None:
            return None
        if not isinstance(x, dict):
            raise ValueError("chords: a dict {bar or (bar, track): [(start, pitches), ...]} (got %r)" % (x,))
        events, trk, brs = req
        trk, brs = [int(t) for t in trk], [int(b) for b in brs]
        per = {}  # (bar, track) -> segments; the (bar, track) keys replace the bar keys
        for both in (False, True):
            for key, segs in x.items():
                if isinstance(key, tuple) != both:
                    continue
                if both:
                    if len(key) != 2 or not is_int(key[0]) or not is_int(key[1]):
                        raise ValueError("chords: a key is a bar number or a (bar, track) tuple (got %r)" % (key,))
                    b, ts = int(key[0]), [int(key[1])]
                    if ts[0] not in trk:
                        raise ValueError("chords: track %r is not in tracks_to_generate %r" % (key[1], trk))
                elif not is_int(key):
                    raise ValueError("chords: a key is a bar number or a (bar, track) tuple (got %r)" % (key,))
                else:
                    b, ts = int(key), trk
                if b not in brs:
                    raise ValueError("chords: bar %r is not in bars_to_generate %r" % (b, brs))
                for t in ts:
                    per[b, t] = segs
        if not per:
            return None
        L = bar_units(events)
        if L > CHORD_POS:
            raise ValueError("chords: a bar of %d sixteenths (at most %d under chords=)" % (L, CHORD_POS))
        layout, n_masks = _mask_layout(events, trk, brs)
        midi = _table(vocab, "midi", lambda v: {int(v.index2char(i)[2:]): i for i in v.pitch_indices})
        at, sets = np.full((n_masks, CHORD_POS), -1, dtype=np.int8), []
        for b, t, m in layout:
            segs = per.get((b, t))
            if segs is None:
                continue
            if isinstance(segs, (str, bytes, dict)) or not hasattr(segs, "__len__") or len(segs) == 0:
                raise ValueError("chords: bar %d, track %d: a non-empty sequence of (start, pitches) segments" % (b, t))
            starts = []
            for seg in segs:
                if isinstance(seg, (str, bytes)) or not hasattr(seg, "__len__") or len(seg) != 2:
                    raise ValueError("chords: a segment is (start, pitches) (got %r)" % (seg,))
                start, ps = seg
                if not is_int(start):
                    raise ValueError("chords: a start is an int in sixteenths (got %r)" % (start,))
                if not _is_collection(ps):
                    raise ValueError("chords: a segment's pitches are a collection of MIDI note numbers (got %r)"
                                     % (ps,))
                if int(start) != 0 if not starts else int(start) <= starts[-1]:
                    raise ValueError("chords: bar %d, track %d: starts begin at 0 and ascend strictly" % (b, t))
                if int(start) >= L:
                    raise ValueError("chords: start %d is outside a bar of %d sixteenths" % (start, L))
                eff = _midi_set(ps, "chords")
                if alw and t in alw:
                    eff = tuple(p for p in eff if p in alw[t])
                    if not eff:
                        raise ValueError("chords: bar %d, track %d, start %d: no pitch is left under pitches="
                                         % (b, t, start))
                if eff not in sets:
                    if len(sets) == CHORD_SETS:
                        raise ValueError("chords: more than %d distinct pitch sets in one request" % CHORD_SETS)
                    sets.append(eff)
                at[m, int(start):] = sets.index(eff)  # the last segment with start <= position governs
                starts.append(int(start))
        rows = np.zeros((len(sets), vocab.vocab_size), dtype=bool)
        for k, s in enumerate(sets):
            rows[k, vocab.pitch_indices] = True
            rows[k, [midi[p] for p in s]] = False
        return _Chords(L, _frozen(at), _frozen(rows), tuple(sets))

    if n is None:
        if isinstance(chords, (list, tuple)):
            raise ValueError("chords is one dict here")
        return one_request(chords, requests[0], allowed[0])
    if isinstance(chords, (list, tuple)):
        if len(chords) != n:
            raise ValueError("chords: one value, or one per request (%d)" % n)
        return [one_request(x, rq, a) for x, rq, a in zip(chords, requests, allowed)]
    return [one_request(chords, rq, a) for rq, a in zip(requests, allowed)]


class _Span:
    """Decoding state of one request: mask index, span tokens, grammar flags."""

    def __init__(self, vocab, src, mask_target, all_controls, no_whole, greedy, logger, t=1.0,
                 p=None, rng=np.random, bans=None, score=False, template=None, bar_len=0, chords=None):
        self.v = vocab
        self.t = t
        self.p = p
        self.rng = rng  # the stream of this request's draws (np.random: the global one)
        # pitch constraints (_request_bans): the ban row of each mask (-1:
        # none) and the boolean rows; None: an unconstrained request
        self.ban_of_mask, self.ban_rows = bans if bans is not None else (None, None)
        self._keeps = {}  # (state code, ban row) -> the keep of governs()
        # take scores: with `score`, logp receives token_logprobs(..)[id] of
        # every emitted id, in draw order (the host draws append it, a device
        # path assigns its own); without, nothing is computed
        self.score = bool(score)
        self.logp = []
        # infill template (_check_template's rows): per mask None or the items
        # of the span's opening, token ids or TPL_PITCH; None: no template
        self.tpl = template
        # the bar clock (fill_bar=): bar_len is the bar's length in sixteenths
        # (0: off); the clock follows the tokens of the note span being drawn,
        # and `fill` receives (cursor, bar_len) of every note span that ends
        self.bar_len = int(bar_len)
        # chord-following infill (chords=): the request's `_Chords`, or None.  The
        # clock runs whenever the span has chords or a bar length; it bans by the
        # bar line only when bar_len > 0.  chord_spans receives, per constrained
        # note span, (onset, midi, allowed set) of every pitch pushed
        self.chords = chords
        self.clock = _BarClock(bar_len, grammar_tables(vocab, all_controls)[1], unit_table(vocab)) \
            if self.bar_len or chords is not None else None
        self.fill = []
        self.chord_spans = []
        self._chord_cur = None
        self.src = src
        self.mask_target = mask_target
        self.all_controls = set(int(c) for c in all_controls)
        self.no_whole = no_whole
        self.greedy = greedy
        self.logger = logger
        self.m0 = vocab.char2index('m_0')
        self.eos = vocab.char2index('<eos>')
        self._pitch = frozenset(vocab.pitch_indices)
        self._dur = frozenset(vocab.duration_only_indices)
        self.n_masks = int(np.sum(np.asarray(src) == self.m0))
        self.mask_idx = 0
        self.tgt_inp = []
        self.total = []
        self.done = self.n_masks == 0
        self._start_span()

    def _start_span(self):
        self.this_in = [self.m0]
        self.this_ev = ['m_0']
        self.in_pitch = self.in_rest = self.in_sep = self.in_continue = False
        if self.clock is not None:
            self.clock.reset()
        self._chord_cur = None
        if self.chords is not None and not self.done and self._note_span() and \
                self.chords.row_at(self.mask_idx, 0) >= 0:
            self._chord_cur = []
            self.chord_spans.append(self._chord_cur)

    def _note_span(self):
        return self.mask_idx < len(self.mask_target) and _target_code(self.mask_target[self.mask_idx]) == 0

    def clock_ban(self):
        """Boolean [V]: what the bar clock and the chord at the clock's `end` (the
        onset of a pitch drawn next) ban for the next draw (note spans only), or
        None."""
        if self.clock is None or self.done or not self._note_span():
            return None
        ban = self.clock.banned(self.v) if self.bar_len else None
        k = -1 if self.chords is None else self.chords.row_at(self.mask_idx, self.clock.end)
        if k >= 0:
            ban = self.chords.rows[k] if ban is None else ban | self.chords.rows[k]
        return ban

    def _span_ends(self):
        """A span ended (this_in still holds it, the dropped last token
        included): under the bar clock a note span reports its cursor."""
        if self.bar_len and self._note_span():
            self.fill.append((bar_fill(self.v, self.this_in[1:-1])[0], self.bar_len))

    def prefix(self):
        return self.tgt_inp + self.this_in

    def _ban_index(self):
        """The ban row of the mask being drawn, or -1."""
        if self.ban_of_mask is None or self.mask_idx >= len(self.ban_of_mask):
            return -1
        return self.ban_of_mask[self.mask_idx]

    def ban(self):
        """Boolean [V] ban of the mask being drawn, or None."""
        k = self._ban_index()
        return None if k < 0 else self.ban_rows[k]

    def forced(self):
        """The template item that governs the draw about to be made (a token
        id, or TPL_PITCH), or None: item len(this_in) - 1 of the mask's row."""
        if self.tpl is None or self.mask_idx >= len(self.tpl):
            return None
        row, i = self.tpl[self.mask_idx], len(self.this_in) - 1
        return None if row is None or i >= len(row) else row[i]

    def governs(self):
        """What governs the draw about to be made, `masked_row`'s arguments:
        (keep, clock_ban, force).  keep: the grammar keep of spec() less the
        mask's pitch ban -- what the score reads; the other two may be None."""
        return self._governs(self.state_code(), self._ban_index())

    def _governs(self, code, k):
        """governs() for state `code` and ban row k (-1: none), which the
        caller has read; the keep of a (state, ban row) pair is built once."""
        keep = self._keeps.get((code, k))
        if keep is None:
            keep = self._keeps[code, k] = _state_keep(self.v, code, None if k < 0 else self.ban_rows[k])
        return keep, self.clock_ban(), self.forced()

    def scored(self, logit, keep, idx):
        """With `score`: the emitted id's log-probability (t = 1, the redraws not
        counted) under the `keep` of the governs() tuple its draw was made from."""
        if self.score:
            if isinstance(logit, torch.Tensor):
                logit = logit.squeeze().detach().cpu().numpy()
            self.logp.append(token_logprobs(logit, keep)[int(idx)])

    def _draw_id(self, logit, check, failmsg, flags, gov, pb):
        """The draw of `gov` through sampling(), whose own keep is that of
        `flags`: the pitch-ban row pb that gov's keep was built from, and the
        clock ban, go in as `ban` (an unconstrained draw is the call it always
        was).  The reference's loop: the draw, then up to 11 redraws while
        `check` rejects; the 12th id stands unchecked and the failure is logged."""
        _, cb, force = gov
        if cb is not None or pb is not None:
            flags = dict(flags, ban=pb if cb is None else cb if pb is None else pb | cb)
        if force is not None:
            flags = dict(flags, force=force)
        for n in range(12):
            idx = sampling(logit, self.v, p=self.p, t=self.t, greedy=self.greedy, rng=self.rng, **flags)
            if n < 11 and (check is None or not check(idx)):
                return idx
        if self.logger is not None:
            self.logger.info(failmsg)
        return idx

    def state_code(self):
        """Grammar state of the current prefix (generation.py:549-630), the
        code csrc/decode_ops.hip grammar_state() computes on device."""
        nw = int(bool(self.no_whole))
        if self.in_sep:
            return 0
        if self.in_continue:
            return 1
        if self.in_pitch:
            return 2 + nw
        if self.in_rest:
            return 4 + nw
        if len(self.this_in) == 1:
            tc = _target_code(self.mask_target[self.mask_idx])
            return 10 if tc == 0 else 5 + tc
        return 11 + nw

    def spec(self):
        """(sampling flags, redraw check, failure message) of the current
        grammar state (generation.py:549-630)."""
        return grammar_spec(self.v, self.state_code())

    def advance(self, logit):
        """Consume the logits of the current prefix's last position."""
        code, k = self.state_code(), self._ban_index()  # (read once: spec and tuple come from the same pair)
        flags, check, failmsg = grammar_spec(self.v, code)
        gov = self._governs(code, k)
        idx = self._draw_id(logit, check, failmsg, flags, gov, None if k < 0 else self.ban_rows[k])
        self.scored(logit, gov[0], idx)
        return self.commit(idx)

    def commit_greedy(self, idx, check, failmsg):
        """Greedy draw already taken (argmax over the masked logits): the
        reference's redraw loop would re-draw the same id 11 times."""
        if self.logger is not None and check is not None and check(int(idx)):
            self.logger.info(failmsg)
        return self.commit(idx)

    def commit_all(self, seq):
        """commit() over a whole emitted id sequence when nothing reads the
        grammar flags between its ids (the device greedy grammar with no
        redraw logger): the same tgt_inp / total / mask_idx / done, without
        the per-token flag updates (only spec() reads them, and a finished
        request never calls it again)."""
        i2c, push = self.v.index2char, self._push
        for idx in seq:
            push(idx, i2c(idx))

    def commit(self, idx):
        v = self.v
        idx = int(idx)
        ev = v.index2char(idx)
        if idx == v.continue_index:
            self.in_continue, self.in_sep = True, False
        if idx in self._pitch:
            self.in_pitch, self.in_sep, self.in_continue = True, False, False
        if idx in self._dur:
            self.in_rest, self.in_pitch = False, False
        if ev == 'sep':
            self.in_sep = True
        if ev == 'rest':
            self.in_rest = True
        self._push(idx, ev)
        return idx

    def _push(self, idx, ev):
        """Push one emitted id (ev: its token), and end the span where it ends:
        a control token brings its <eos>; at <eos> or the 100-token cap the span
        goes to tgt_inp / total without its last token and the next mask starts."""
        if self.clock is not None:
            if self._chord_cur is not None and idx in self._pitch:
                end = self.clock.end
                k = self.chords.row_at(self.mask_idx, end)
                self._chord_cur.append((end, int(ev[2:]), self.chords.sets[k] if k >= 0 else None))
            self.clock.advance_id(idx)
        this_in, this_ev = self.this_in, self.this_ev
        if idx in self.all_controls:
            this_in += [idx, self.eos]
            this_ev += [ev, '<eos>']
        else:
            this_in.append(idx)
            this_ev.append(ev)
        if this_in[-1] == self.eos or len(this_in) >= 100:
            self._span_ends()
            self.tgt_inp.extend(this_in[:-1])
            self.total.extend(this_ev[:-1])
            self.mask_idx += 1
            if self.mask_idx >= self.n_masks:
                self.done = True
            else:
                self._start_span()


def _src_tokens(vocab, src):
    """[vocab.index2char(int(t)) for t in src] (generation.py:685) through
    one dict lookup per id instead of a method call and an int() each."""
    table = getattr(vocab, "_idx2char", None)
    get = table.get if isinstance(table, dict) else vocab.index2char
    return list(map(get, src.tolist() if hasattr(src, "tolist") else list(src)))


def _prepare(events, vocab, tracks_to_generate, bars_to_generate):
    """generation.py:470-516: duration tables, mask targets, masked src."""
    name_to_time, time_to_name, times, bar_duration = durations_for_events(events)
    n_bars = events.count('bar') if isinstance(events, list) else sum(1 for e in events if e == 'bar')
    target, tracks = mask_targets(events, tracks_to_generate, bars_to_generate)
    if bars_to_generate[-1] >= n_bars:
        events = fill_empty_bars(events, bars_to_generate[-1] - n_bars + 1, bar_duration,
                                 time_to_name, times)
    src, mtn, mbn = mask_bar_and_track(events, vocab, tracks, bars_to_generate)
    no_whole = not (int(events[0][0]) >= 4 and int(events[0][2]) == 4)
    return src, mtn, mbn, target, no_whole


class _Slot(namedtuple("_Slot", "src mask_track_names mask_bar_names target no_whole t p seed bans tpl bar_len "
                                "chords")):
    """One decode slot (a request, or one take of it), immutable: `_prepare`'s
    five values and the request's validated keywords -- t, p, the effective
    seed (None: the global stream), `_request_bans`' pair, `_check_template`'s
    rows, the bar length in sixteenths (0: no clock) and `_check_chords`'
    record (None: no chords)."""
    __slots__ = ()

    def span(self, vocab, all_controls, greedy, logger, score):
        """A fresh `_Span` of the slot; a seeded one starts its stream anew."""
        rng = np.random if self.seed is None else np.random.RandomState(self.seed)
        return _Span(vocab, self.src, self.target, all_controls, self.no_whole, greedy, logger, self.t,
                     self.p, rng, self.bans, score, self.tpl, self.bar_len, self.chords)


# A call's requests, resolved: the slots in decode order (request i takes[i] times in a row; takes None:
# no variations), and what `stats` reports: the seed per slot (or None), the pitches per request
_Resolved = namedtuple("_Resolved", "slots takes seeds allowed score rank")


class _Unprepared(Exception):
    """`_prepare` / `_request_bans` failed on the plugin call's request: the
    call prints the cause and returns None (generation.py:695-696)."""


def _masked_request(vocab, events, tracks_to_generate, bars_to_generate, allowed=None):
    """(`_prepare`'s five values, the ban rows) of one request; `events` is
    the masked song afterwards (fill_empty_bars appends to its argument)."""
    bans = _request_bans(vocab, events, tracks_to_generate, bars_to_generate, allowed)
    return _prepare(events, vocab, tracks_to_generate, bars_to_generate), bans


def _resolve(requests, vocab, all_controls, n, *, t, p, variations, seed, pitches, logprobs, rank,
             template, fill_bar, chords=None, checked=None):
    """Validate a call's keywords and build its slots.  n: the number of
    `requests` for generation_batch (a keyword is one value, or one per
    request), None for the plugin call (one request, one value each).  Raises
    ValueError in the order t/p, variations, seed, pitches, logprobs/rank,
    fill_bar, chords, template; touches neither the model nor np.random.
    checked(seeds, allowed): the plugin call's own step between the keyword
    checks and the decode (its stats, its use_kv_cache check); it has always
    come before the request is prepared, and with a template after that."""
    one = n is None

    def each(x):
        return [x] if one else x
    tps = each(_check_tp(t, p, n))
    takes = None if variations is None else each(_check_variations(variations, n))
    seeds = _check_seed(seed, n, takes if takes is None or not one else takes[0])
    allowed = each(_check_pitches(pitches, requests[0][1] if one else [tr for _, tr, _ in requests], n))
    score = _check_score(logprobs, rank, variations)
    bar_lens = [bar_units(ev) if fb else 0 for (ev, _, _), fb in zip(requests, each(_check_fill_bar(fill_bar, n)))]
    chord_recs = each(_check_chords(chords, requests, allowed, vocab, n))
    if checked is not None and template is None:
        checked(seeds, allowed)
    try:
        preps = [_masked_request(vocab, ev, tr, br, a) for (ev, tr, br), a in zip(requests, allowed)]
    except Exception as e:
        if one:
            raise _Unprepared(e) from None
        raise
    if one:
        template, had_template = [template], template is not None
    elif template is None:
        template = [None] * n
    elif not isinstance(template, (list, tuple)) or len(template) != n:
        raise ValueError("template: None, or one value per request (%d)" % n)
    slots = [_Slot(*q, a, b, None, bn, _check_template(x, vocab, q[0], q[3], all_controls, q[4], bn, bl, ch), bl, ch)
             for (q, bn), (a, b), x, bl, ch in zip(preps, tps, template, bar_lens, chord_recs)]
    if checked is not None and had_template:
        checked(seeds, allowed)
    if takes is not None:  # the expanded list: take k of request i is a slot of its own
        slots = [s for s, k in zip(slots, takes) for _ in range(k)]
    if seeds is not None:
        slots = [s._replace(seed=x) for s, x in zip(slots, seeds)]
    return _Resolved(slots, takes, seeds, allowed, score, bool(rank))


class _Precision:
    """Run a block at another arithmetic precision of the model, restoring
    the model's own afterwards (the plugin call decodes in fp32 whatever
    precision the model trains in)."""

    def __init__(self, model, precision):
        self.model, self.want = model, precision
        self.prev = None

    def __enter__(self):
        if self.want is not None and self.want != self.model.precision:
            self.prev = self.model.precision
            self.model.set_precision(self.want)
        return self

    def __exit__(self, *exc):
        if self.prev is not None:
            self.model.set_precision(self.prev)
        return False


def generation_all(model, events, device, vocab, logger, all_controls, tracks_to_generate,
                   bars_to_generate, *, greedy=False, use_kv_cache=True, stats=None,
                   precision="fp32", warm=True, device_grammar=True, t=1.0, p=None, variations=None,
                   seed=None, pitches=None, logprobs=False, rank=False, template=None, fill_bar=False,
                   chords=None):
    """`generation.py:468-696`.  Returns (restored '<U9' tokens,
    mask_track_names, mask_bar_names) or None (nothing masked / on error,
    after printing it, as the reference does).  `stats` (a dict, opt-in)
    receives the number of decode steps (= tokens drawn).
    warm: decode on this model's cached batch-1 session (KV caches and the
    captured step graph kept across calls, as in generation_batch); False
    builds a private session freed after the call.  A warm session is not
    re-entrant: concurrent calls on one model (threads) would share its
    caches and graph, so serialise them or pass warm=False.
    precision: arithmetic of this call's decode.  "fp32" (default) gives
    the reference's token ids bit for bit (north_star: bit-exact greedy ids;
    sampled ids are the same draws of the same numpy stream) whatever
    precision the model trains in; None decodes at the model's own precision
    (bf16 for a default-constructed model: faster, ids may differ at
    near-ties); the batched serving API `generation_batch` keeps None.
    device_grammar: (KV-cached path) run the grammar and the draws on the
    device inside the captured decode step -- greedy argmax, or sampling
    on numpy's MT19937 stream handed to the device and back
    (csrc/decode_ops.hip grammar_sample_kernel) -- with no host round trip
    per token; False keeps the per-token host loop.
    t, p: the temperature and the nucleus threshold of the reference's
    `sampling()` (softmax of masked logits / t; with p, the draw is among the
    most probable tokens whose cumulative probability first exceeds p).  The
    defaults are the reference's own call (the whole distribution at t = 1).
    Every path -- device, host loop, use_kv_cache=False -- draws from the same
    distribution on the same stream.  A t that is not finite and > 0, or a p
    that is neither None nor finite and >= 0, raises ValueError before
    anything is drawn.
    variations: an int n >= 1 returns a LIST of n results, n takes of the
    request decoded in lockstep on one session whose n request slots share
    ONE encoded source (one prefill, one cross-attention memory): exactly
    generation_batch([request] * n, greedy=greedy, precision=precision) on
    the same np.random stream.  None (default) is the single result.  The
    print-and-return-None on error holds for the call as a whole (KV-cached
    path only; anything else than an int >= 1 raises ValueError).
    seed: None (default) draws from the global np.random stream, as the
    reference does.  An int s in [0, 2**32 - 1] draws from a stream of the
    call's own, np.random.RandomState(s): the tokens are those of
    `np.random.seed(s); generation_all(...)` without the seed, on every path,
    and the global np.random state is neither read nor written.  With
    variations=n, take k (0-based) uses seed s + k (s + n - 1 <= 2**32 - 1),
    so a take can be regenerated alone with seed=s + k.  greedy=True
    validates the seed and draws nothing.  Anything else raises ValueError
    before the model or np.random is touched.  `stats` receives 'seeds', the
    effective seed of every take (None unseeded).
    pitches: None (default): any of the pitch tokens p_21 .. p_108 may be
    drawn, today's behaviour bit for bit.  A collection of ints (see
    pitch_set): the MIDI note numbers every masked track of the request may
    use; a dict {track number: collection}, keys among tracks_to_generate: the
    listed tracks only, the others unconstrained.  For every draw of a span
    of a constrained track the logits of the pitch tokens outside the set
    become -100.0 -- after the float32 -> float64 widening, before the division
    by t, exactly as a masked class's do (`keep &= ~ban` in sampling()); the
    redraw checks do not change.  A banned pitch therefore has probability
    about e^-100 relative to the best kept token: not a mathematical zero,
    but never drawn in practice.  Since at least one pitch is kept, every
    grammar state that demands a pitch can still be satisfied.  Every path --
    device (greedy, shared stream, seeded), host loop, use_kv_cache=False --
    draws the same tokens on the same stream; with variations all takes share
    the constraint.  An empty set, an entry that is not an int in [21, 108]
    (bool and float included) or an unknown track raises ValueError before
    the model or np.random is touched.  `stats` receives 'pitches': None, or
    the effective {track number: sorted tuple}.
    logprobs: False (default): today's call, and today's `stats`.  True: the
    call also scores what it draws.  `stats` receives 'logprobs', a list with
    one float64 array per take (one take without variations): entry j is the
    log-probability of the take's j-th drawn token, token_logprobs(logit,
    keep)[id] -- the log of the distribution sampling() builds from that
    step's masked (and, under `pitches`, banned) logits at t = 1, over the
    whole distribution -- so len(stats['logprobs'][k]) is take k's step count;
    and 'scores', float(np.sum(..)) of each array.  Both are in take order,
    as 'seeds' is.  The score never depends on the call's t and p and takes no
    account of the redraw loop, so takes drawn with different settings
    compare: it is the log-likelihood of the tokens under the model and the
    grammar mask.  Tokens, redraw log lines, steps and the np.random state
    afterwards are those of the call without logprobs, on every path; on the
    device the step graphs named '+score' take the numbers between the
    vocabulary projection and the next replay (smer_logprob_stage /
    smer_logprob_commit), and a call without logprobs replays the graphs it
    always did.
    rank: True (implies scoring; needs variations) returns the takes in
    descending mean log-probability per drawn token, scores[k] /
    len(logprobs[k]) -- the mean, so that a short take is not favoured for
    being short -- ties to the lower take index; `stats` receives 'order', the
    take indices in returned order, while 'seeds', 'logprobs' and 'scores'
    stay in take order.  Anything but a bool for either, or rank without
    variations, raises ValueError before the model or np.random is touched.
    template: None (default): every draw is free, today's behaviour bit for
    bit.  Otherwise one row per mask, in mask_targets order; a row is None
    (free) or a sequence of items: a token (string or id) -- that token is
    emitted at that position; ANY_PITCH -- any pitch token, and only a pitch
    token; '<eos>', as the last item of a note span's row only -- the span ends
    there.  Item i governs the draw made when the span holds i body tokens;
    the positions past the row are free, so a row is a determined opening
    followed by free decoding (rhythm_template and opening_template build the
    two common ones).  A constrained draw is a masked draw, as `pitches` is:
    after the float32 -> float64 widening, the grammar mask and the pitch ban,
    and before the division by t, a token item v sets x[v] = 0.0 and every
    other entry to -100.0, and ANY_PITCH sets every entry that is no pitch to
    -100.0.  The draw, the redraw loop and what they take from the stream are
    those of any other step, so the stream afterwards is defined by them, and
    every path -- device, host loop, use_kv_cache=False -- agrees on it.  Any
    other token keeps probability about e^(-100/t) each: not zero (DESIGN
    section 8).  logprobs=True reports the emitted token's log-probability
    under the model, the grammar mask and the pitch ban BEFORE the template
    is applied -- the number score_infill gives for the same token.  With
    variations all takes carry the template.  On the device the step graphs
    named '+tpl' force the items from a tape (smer_logits_template); a call
    without a template replays the graphs it always did.  _check_template
    lists what raises ValueError, before the model or np.random is touched.
    fill_bar: False (default): today's behaviour bit for bit.  True: every note
    span (mask target 'r') fills its bar exactly -- it never passes the bar
    line and can end only on it; control spans are untouched.  The bar's length
    L is bar_units(events) sixteenths, and a clock (_BarClock: the cursor rule
    of codec._Writer in integers) follows the tokens drawn.  It is a masked
    draw, as `pitches` is: after the widening, the grammar mask and the pitch
    ban, and before the template and the division by t, the logits of the
    candidates the clock bans become -100.0 -- a duration that would cross the
    bar line; a pitch, 'continue' or 'rest' at a full bar; a 'sep' that would
    rewind to the bar line; <eos> and the control tokens while the bar is not
    full.  The draw, the redraw loop and what they take from the stream are
    those of any other step, and every path -- device, host loop,
    use_kv_cache=False -- agrees.  logprobs=True reports what it reports
    without the keyword (the model, the grammar mask and the pitch ban: the
    number score_infill gives).  Under fill_bar a template is validated
    against the clock as well.  A span cut by the 100-token cap cannot be
    forced full: it is reported as it is.  `stats` receives
    'bar_fill': per take, one (cursor, L) per note span.  On the device the
    step graphs named '+bar' run the clock (smer_bar_clock); a call without
    the keyword replays the graphs it always did.  Anything but a bool, or a
    bar whose length is no integer in 1..255 sixteenths, raises ValueError
    before the model or np.random is touched.
    chords: None (default): today's behaviour, graphs and stats keys.  A dict
    gives the harmony of the infilled bars: a key is a bar number of
    bars_to_generate (every track of tracks_to_generate) or a (bar, track) tuple
    (that track only; it replaces the bar's entry for that track); a value is a
    sequence of segments (start, pitches) -- start an int in sixteenths from the
    bar line, the first 0, strictly ascending; pitches a collection of MIDI
    numbers as `pitches=` takes (pitch_set(classes=chord_tones(5, 'maj'))).
    The segment that governs a position is the last one that starts at or
    before it.  It is a masked draw, like the bar clock's: in a note span whose
    (bar, track) has segments, with `end` the clock's value before the draw --
    exactly the onset of a pitch drawn next: a pitch closes an open duration
    group and sounds where the next one starts, after 'sep' at the rewound
    position, as the second note of a chord at the first one's -- the logit of
    every pitch token outside the set of the segment that governs min(end, L -
    1) becomes -100.0, at the place in the row where the bar clock bans (after
    the score has read the row, before the template).  No other token and no
    other span is touched, and the clock runs whether or not fill_bar is set.
    A segment's set is intersected with the track's `pitches=` set, if any.
    logprobs=True and score_infill report what they report without the keyword.
    Under `template=` a pitch token item that its onset's chord bans is
    rejected; with rhythm_template one call reharmonises a bar and keeps its
    rhythm.  With variations all takes carry the chords.  `stats` receives
    'chords': per take, per constrained note span, the list of (onset, midi,
    allowed set) of its pitches.  On the device the step graphs named
    '+bar+chord' run smer_chord_ban after the clock; a call without the keyword
    replays the graphs it always did.  `_check_chords` lists what raises
    ValueError, before the model or np.random is touched."""
    t0 = time.perf_counter()

    def checked(seeds, allowed):
        if stats is not None:
            stats["seeds"] = seeds
            stats["pitches"] = allowed[0]
        if variations is not None and not use_kv_cache:
            raise ValueError("variations needs the KV-cached path (use_kv_cache=True)")
    try:
        rq = _resolve([(events if variations is None else list(events), tracks_to_generate, bars_to_generate)],
                      vocab, all_controls, None, t=t, p=p, variations=variations, seed=seed, pitches=pitches,
                      logprobs=logprobs, rank=rank, template=template, fill_bar=fill_bar, chords=chords,
                      checked=checked)
    except _Unprepared as e:  # reference behaviour (generation.py:695-696)
        print(e.args[0])
        return None
    if variations is not None:
        with _Precision(model, precision):
            try:
                out, st = _decode_batch(model, rq, vocab, all_controls, greedy=greedy, logger=logger,
                                        device_grammar=device_grammar, warm=warm, t0=t0)
                if stats is not None:
                    stats["steps"] = st["steps"]
                    if rq.slots[0].bar_len:
                        stats["bar_fill"] = st["bar_fill"]
                    if rq.slots[0].chords is not None:
                        stats["chords"] = st["chords"]
                    if rq.score:
                        stats["logprobs"], stats["scores"] = st["logprobs"], st["scores"]
                    if rank:
                        stats["order"] = st["order"][0]
                return out[0]
            except Exception as e:  # reference behaviour (generation.py:695-696)
                print(e)
                return None
    with _Precision(model, precision):
        return _generation_all(model, device, vocab, logger, all_controls, rq.slots[0], greedy, use_kv_cache,
                               stats, warm, device_grammar, rq.score)


def _reject_rows(vocab):
    rej = np.zeros((N_GRAMMAR_STATES, vocab.vocab_size), dtype=np.uint8)
    for c in range(N_GRAMMAR_STATES):
        chk = grammar_spec(vocab, c)[1]
        if chk is not None:
            rej[c] = [bool(chk(i)) for i in range(vocab.vocab_size)]
    return rej


def reject_table(vocab):
    """uint8 [13, V]: the redraw checks of the grammar states
    (generation.py:556-615; grammar_spec's check), 1 = redraw."""
    return _table(vocab, "reject", _reject_rows)


def _device_rows(rows):
    """`bans=` (per span None or (ban_of_mask row, bit rows uint32 [k, 16])) or
    `templates=` (per span None or its rows) of the device decodes: the list,
    or None when every entry is None (the graphs without that kernel replay)."""
    rows = list(rows)
    return rows if any(x is not None for x in rows) else None


def _device_bars(spans):
    """`bars=` of the device decodes: per span its bar length in sixteenths (0:
    no clock); None when no span has one and none has chords (the graphs
    without the clock replay; the chord node reads the clock's words)."""
    bars = [sp.bar_len for sp in spans]
    return bars if any(bars) or any(sp.chords is not None for sp in spans) else None


def _device_chords(spans):
    """`chords=` of the device decodes: per span None or (L, the positions' row
    table int8 [masks, CHORD_POS], the bit rows uint32 [k, 16]); None when no
    span has chords (the graphs without the chord node replay)."""
    return _device_rows(None if sp.chords is None else (sp.chords.L, sp.chords.at, ban_bits(sp.chords.rows))
                        for sp in spans)


def _replay(spans, res, logger, sampled=True):
    """Replay the ids a device loop emitted (a DecodeResult) through the host
    spans, which rebuild exactly the reference's event lists.  sampled: step
    by step, the requests in order -- the host loop's order, so the
    redraw-failure lines come out in its order too.  Greedy: commit_all
    without a logger (no redraw report to log), commit_greedy with one.
    With score the spans take the device's own log-probabilities, entry for
    entry with the ids.  Returns the number of tokens."""
    if sampled:
        for k in range(max([len(q) for q in res.ids] + [0])):
            for sp, seq, fl in zip(spans, res.ids, res.fails):
                if k < len(seq):
                    if fl[k] and logger is not None:
                        logger.info(sp.spec()[2])
                    sp.commit(seq[k])
    else:
        for sp, seq in zip(spans, res.ids):
            if logger is None:
                sp.commit_all(seq)
            else:
                for idx in seq:
                    _, chk, msg = sp.spec()
                    sp.commit_greedy(idx, chk, msg)
    if not all(sp.done for sp in spans):
        raise RuntimeError("device grammar and host replay disagree")
    if res.logp is not None:
        for sp, lp in zip(spans, res.logp):
            sp.logp = list(lp)
    return sum(len(seq) for seq in res.ids)


def _decode_on_device(sess, spans, vocab, all_controls, logger, greedy, seeds, score):
    """The span loop of `spans` on the device, then its ids replayed through
    the host spans (event lists, redraw-failure log lines).  Returns (tokens,
    DecodeResult, start, end of the device call), or None -- redo on the host
    with fresh spans -- when a row's probabilities missed 1 by more than 1e-9
    (np.random.choice territory); np.random is then rewound (a seeded call
    touches no global state: fresh spans start fresh RandomStates)."""
    keep, cls = grammar_tables(vocab, all_controls)
    kw = dict(eos=vocab.eos_index, m0=vocab.char2index('m_0'), score=score, bars=_device_bars(spans),
              chords=_device_chords(spans),
              templates=_device_rows(sp.tpl for sp in spans),
              bans=_device_rows(None if sp.ban_of_mask is None else (sp.ban_of_mask, ban_bits(sp.ban_rows))
                                for sp in spans))
    rng0 = np.random.get_state() if seeds is None and not greedy else None
    ts = time.perf_counter()
    if greedy:
        res = sess.greedy_decode(spans, keep, cls, **kw)
    else:
        res = sess.sampled_decode(spans, keep, reject_table(vocab), cls, t=[sp.t for sp in spans],
                                  p=[sp.p for sp in spans], seeds=seeds, **kw)
    te = time.perf_counter()
    if not greedy and np.any(res.err & 2):
        if seeds is None:
            np.random.set_state(rng0)
        return None
    if np.any(res.err if greedy else res.err & 1):
        raise ValueError("decoder prefix exceeds session max_tgt %d" % (sess.Tmax - 1))
    return _replay(spans, res, logger, sampled=not greedy), res, ts, te


def _generation_all(model, device, vocab, logger, all_controls, slot, greedy, use_kv_cache, stats,
                    warm=True, device_grammar=True, score=False):
    try:
        src = slot.src
        st = slot.span(vocab, all_controls, greedy, logger, score)
        if st.n_masks == 0:
            return None
        model.eval()
        with torch.no_grad():
            steps = 0
            if use_kv_cache:
                # the warm batch-1 session of this model and precision: KV
                # caches, step buffers and the captured step graph persist
                # across plugin calls (same rules as generation_batch's)
                sess = _batch_session(model, 1, len(src), max(128, 100 * st.n_masks + 8), None,
                                      warm=warm)
                sess.prefill([0], [src])
                if device_grammar and not greedy and vocab.vocab_size <= 512:
                    done = _decode_on_device(sess, [st], vocab, all_controls, logger, False,
                                             None if slot.seed is None else [slot.seed], score)
                    if done is not None:
                        steps = done[0]
                    else:  # fresh span, same RNG start: the host loop below
                        st = slot.span(vocab, all_controls, greedy, logger, score)
                        sess.prefill([0], [src])
                fed = 0
                while not st.done:
                    pre = st.prefix()
                    logit = sess.step([(0, pre[fed:], fed)])[0]
                    fed = len(pre)
                    st.advance(logit)
                    steps += 1
            else:
                src_t = torch.tensor(src)
                while not st.done:
                    out = model_generate(model, src_t, st.prefix(), device)
                    st.advance(out[-1].numpy())
                    steps += 1
            if stats is not None:
                stats["steps"] = steps
                if score:
                    stats["logprobs"] = [np.asarray(st.logp, dtype=np.float64)]
                    stats["scores"] = [float(np.sum(stats["logprobs"][0]))]
                if slot.bar_len:
                    stats["bar_fill"] = [list(st.fill)]
                if slot.chords is not None:
                    stats["chords"] = [list(st.chord_spans)]
        return restore_marked_input(_src_tokens(vocab, src), st.total), slot.mask_track_names, slot.mask_bar_names
    except Exception as e:  # reference behaviour (generation.py:695-696)
        print(e)


infill = generation_all


# Warm decode sessions of generation_batch, one per (model, precision, R,
# source count), at most two kept: the KV caches, step buffers and the captured step +
# grammar graph persist across calls (a serving process keeps them; capturing
# costs ~10 ms at C2).  A cached session is reused when the call's sources and
# prefix fit AND its cache capacities fall in the same decode-attention
# variant class as a fresh session's would (>= 512 key rows: 8-wave blocks;
# the kernels pick by capacity, and the variants sum in different orders), so
# reuse never changes a token.
_BATCH_SESSIONS = {}


def clear_decode_sessions(model=None):
    """Drop the warm decode sessions of `model` (all models when None),
    releasing their KV caches and captured graphs; the next
    generation_batch call builds a fresh session."""
    for key in [k for k, s in _BATCH_SESSIONS.items() if model is None or s.model is model]:
        del _BATCH_SESSIONS[key]


def _plugin_capacity(Smax, Tmax):
    """Capacities of a warm batch-1 (plugin) session: rounded up to powers of
    two (>= 128), so consecutive calls on sources / mask counts of similar
    size reuse one session and its captured graphs instead of rebuilding
    them (a rebuild + capture costs ~6 ms, 1/4 of a typical call); a fresh
    session for the same request rounds the same way.  The rounding never
    carries a capacity across 512 rows, where the decode attention switches
    to its 8-wave variant (another summation order), so warm and cold
    sessions give the same logits.  Tmax excludes the trash slot (the cache
    holds Tmax + 1 rows)."""
    S0, T0 = int(Smax), int(Tmax)
    S = 1 << max(7, (S0 - 1).bit_length())
    if S0 < 512:
        S = min(S, 511)
    T = (1 << max(7, T0.bit_length())) - 1
    if T0 + 1 < 512:
        T = min(T, 510)
    return S, T


def _batch_session(model, R, Smax, Tmax, precision, exact_tmax=False, warm=True, sources=None):
    """A decode session for this call.  A cached one is reused only when it
    still addresses the model's current weight buffers (moving the model
    re-flattens them) and, for an explicit max_tgt, has exactly that
    capacity (so the 'prefix exceeds max_tgt' error depends on this call's
    arguments alone; the auto-sized capacity 100 * n_masks + 8 can never be
    exceeded).  Before reuse the working weights are re-synchronised with the
    fp32 master in place (a load_state_dict or an optimizer step since the
    last call), so prefill and the captured step read current weights."""
    if precision is not None:
        model.set_precision(precision)
    NS = R if sources is None else int(sources)
    if not warm:
        return DecodeSession(model, R, Smax, Tmax, max_sources=NS)
    if R == 1 and not exact_tmax:
        Smax, Tmax = _plugin_capacity(Smax, Tmax)
    key = (id(model), model.precision, R, NS)
    s = _BATCH_SESSIONS.get(key)
    fits = (s is not None and s.model is model and s.Smax >= Smax and s.Tmax >= Tmax + 1
            and (s.Tmax == Tmax + 1 or not exact_tmax)
            and (s.Smax >= 512) == (Smax >= 512) and (s.Tmax >= 512) == (Tmax + 1 >= 512))
    if fits:
        W = s.eng.weights(s.dt)  # re-casts in place when the master moved
        if W.fc_w.data_ptr() == s.W.fc_w.data_ptr() and W.emb.data_ptr() == s.W.emb.data_ptr():
            s.W = W
            s.src_len[:] = 0
            return s
    s = DecodeSession(model, R, Smax, Tmax, max_sources=NS)
    _BATCH_SESSIONS.pop(key, None)
    while len(_BATCH_SESSIONS) >= 2:
        _BATCH_SESSIONS.pop(next(iter(_BATCH_SESSIONS)))
    _BATCH_SESSIONS[key] = s
    return s


def generation_batch(model, requests, vocab, all_controls, *, greedy=True, logger=None,
                     max_tgt=None, precision=None, return_stats=False, device_grammar=True,
                     warm=True, t=1.0, p=None, variations=None, seed=None, pitches=None,
                     logprobs=False, rank=False, template=None, fill_bar=False, chords=None):
    """Decode many infill requests in lockstep on one KV-cached session.

    requests: list of (events, tracks_to_generate, bars_to_generate).
    Decoding runs the grammar on device (`device_grammar`, the
    default): the step graph ends in the grammar kernel that picks every
    request's token and writes the next step's feed, so steps replay back
    to back; the emitted ids are then replayed through the host `_Span`s,
    which rebuild exactly the reference's event lists (and log the
    reference's redraw failures).  With greedy=False the kernel is the
    sampler (vocabularies up to 512 tokens): it draws for the requests in
    order on numpy's MT19937 stream, as the host loop does, so the tokens and
    the np.random state afterwards are the host loop's.
    `device_grammar=False` keeps the per-step host loop.
    t, p: temperature and nucleus threshold (see generation_all), one value
    or one per request; validated before anything is drawn (ValueError).
    warm: reuse (and keep) this model's cached decode session, as a serving
    process would; False builds a private session freed after the call
    (see also clear_decode_sessions).
    variations: None, or the number of takes per request (an int, or one
    int per request; t and p apply to all takes of a request).  The call
    then behaves exactly like this call on the list in which request i
    appears variations[i] times in a row -- same session sizes, tokens, redraw
    log lines, np.random state, 'tokens' and 'steps' -- but every request is
    encoded ONCE and its takes share one cross-attention memory
    (DecodeSession.prefill_takes), and entry i of the result is the list of
    its takes' results (None where nothing was masked).
    seed: None (default): every draw comes from the global np.random stream,
    the requests in turn, so a request's tokens depend on the batch around
    it.  An int in [0, 2**32 - 1] for all requests, or one per request (no
    None among them): request i draws from its own stream
    np.random.RandomState(seed[i]), so its tokens depend on its seed and its
    logits alone -- the same in any batch, at any position, and (in fp32) as
    generation_all(..., seed=seed[i]) -- and np.random is neither read nor
    written.  With variations, take k (0-based) of request i uses seed[i] + k
    (which must stay <= 2**32 - 1), so a take is regenerated alone with that
    seed; derived seeds of different requests may coincide, which is the
    caller's business.  On device the seeded sampler runs one block per
    request (smer_grammar_sample_step_rows).  greedy=True validates the seed
    and draws nothing.  Bad seeds raise ValueError before anything else.
    pitches: the allowed MIDI note numbers (see generation_all), one value
    for all requests or one per request.  A bare collection of ints or a
    dict applies to every request; a list or tuple with len(requests) entries
    that are each None, a collection or a dict is per request (None: that
    request is unconstrained).  The two are told apart by the entries, never
    by the length: a list of ints is always ONE pitch set for all requests,
    and a list whose entries are None / collections / dicts must have one
    entry per request (ValueError otherwise).  With variations all takes of
    a request share its constraint.  A call in which no request is
    constrained replays the step graphs it always did; a constrained call
    replays the '+ban' graph of its mode, whose extra kernel
    (smer_logits_ban) rewrites the banned logits ahead of the grammar
    kernel.  Validated before anything else is touched (ValueError).
    logprobs, rank: take scores (see generation_all).  logprobs=True: the
    stats dict receives 'logprobs' (one float64 array per entry of
    'generated': the log-probability of each of its drawn tokens, in draw
    order) and 'scores' (their sums); absent otherwise.  A scored call replays
    the '+score' graph of its mode ('greedy+score', 'stream+ban+score', ..)
    and emits the tokens of the unscored call; its host loops compute the same
    numbers from their own logits.  rank=True (needs variations; implies
    scoring) returns every request's takes in descending mean log-probability
    per drawn token, ties to the lower take index, and 'order' holds one list
    of take indices per request; 'generated', 'seeds', 'logprobs' and 'scores'
    stay in take order.  Both are validated as bools before anything else is
    touched (ValueError).
    template: None, or one value per request (see generation_all): None for a
    request without a template, else its rows, one per mask.  With variations
    all takes of a request carry its template.  A call in which no request
    has one replays the step graphs it always did; otherwise the '+tpl' graph
    of its mode ('greedy+tpl', 'rows+ban+tpl+score', ..), in which the
    requests without a template read an all-free tape.  Validated before
    anything else is touched (ValueError).
    fill_bar: the bar clock (see generation_all), one bool for all requests or
    one per request; with variations all takes of a request carry it.  A call
    in which no request sets it replays the step graphs it always did;
    otherwise the '+bar' graph of its mode ('greedy+bar', 'rows+ban+bar+tpl',
    ..), in which the requests without it have bar length 0 and are left
    alone.  The stats dict then receives 'bar_fill': per entry of 'generated'
    None, or one (cursor, L) per note span.  Validated before anything else is
    touched (ValueError).
    chords: chord-following infill (see generation_all): None, one dict for all
    requests, or a list or tuple with one value (None or a dict) per request;
    with variations all takes of a request carry it.  A call in which no
    request has chords replays the step graphs it always did; otherwise the
    '+bar+chord' graph of its mode ('greedy+bar+chord', 'rows+ban+bar+chord+tpl',
    ..), in which the clock node is always present (requests without fill_bar
    have bar length 0) and the requests without chords read an all-free table.
    The stats dict then receives 'chords': per entry of 'generated' None, or per
    constrained note span the list of (onset, midi, allowed set).  Validated
    before anything else is touched (ValueError).
    Returns a list of (restored, mask_track_names, mask_bar_names) (None
    where nothing was masked), and optionally {'tokens', 'steps', 'sources',
    'prefill_rows', 'seeds' (the effective seed of every entry of 'generated',
    None unseeded), 'pitches' (per request, None or the effective {track
    number: sorted tuple}), ..}."""
    t0 = time.perf_counter()
    rq = _resolve([(list(ev), tr, br) for ev, tr, br in requests], vocab, all_controls, len(requests), t=t,
                  p=p, variations=variations, seed=seed, pitches=pitches, logprobs=logprobs, rank=rank,
                  template=template, fill_bar=fill_bar, chords=chords)
    out, stats = _decode_batch(model, rq, vocab, all_controls, greedy=greedy, logger=logger, max_tgt=max_tgt,
                               precision=precision, device_grammar=device_grammar, warm=warm, t0=t0)
    return (out, stats) if return_stats else out


def _decode_batch(model, rq, vocab, all_controls, *, greedy, logger, device_grammar, warm, t0, max_tgt=None,
                  precision=None):
    """generation_batch on resolved requests (`_resolve`): (results, stats)."""
    slots, takes, seeds, score = rq.slots, rq.takes, rq.seeds, rq.score

    def fresh_spans():  # seeded: every request's stream starts (again) at its seed
        return [s.span(vocab, all_controls, greedy, logger, score) for s in slots]
    spans = fresh_spans()
    R = len(slots)
    # one source per request: its takes sit in a row and share it
    srcs = [slots[k].src for k in (range(R) if takes is None else np.cumsum([0] + takes[:-1]))]
    Smax = max(len(s.src) for s in slots)
    Tmax = max_tgt or max(128, 100 * max(s.n_masks for s in spans) + 8)
    model.eval()
    tokens = steps = 0
    with torch.no_grad():
        sess = _batch_session(model, R, Smax, Tmax, precision, exact_tmax=max_tgt is not None,
                              warm=warm, sources=len(srcs))

        def prefill():
            if takes is None:
                sess.prefill(list(range(R)), srcs)
            else:
                sess.prefill_takes(srcs, takes)
        t1 = time.perf_counter()
        prefill()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_dev = 0.0
        fed = [0] * R
        latency = None
        kv_reads = None
        # (the template and clock kernels serve vocabularies up to 512 tokens, as the sampler
        # does: a templated or clocked greedy call above that runs the host loop below)
        if device_grammar and (vocab.vocab_size <= 512 or (
                greedy and all(sp.tpl is None for sp in spans) and _device_bars(spans) is None)):
            done = _decode_on_device(sess, spans, vocab, all_controls, logger, greedy, seeds, score)
            if done is None:  # same RNG start, fresh spans: the whole batch goes through the host loop below
                spans = fresh_spans()
                prefill()
            else:
                n, res, ts, te = done
                tokens, steps, t_dev = tokens + n, res.steps, te - ts
            if done is not None and greedy:
                seqs = res.ids
                # completion time of each request from the call's start: host
                # preparation + prefill, then the GPU end time of its last step
                latency = [(ts - t0) + (res.step_ms[len(q) - 1] / 1000.0 if q else 0.0) for q in seqs]
                # key rows the decode steps attended to (SURVEY §8d infill bytes):
                # request r's i-th step reads its S_r memory rows and i+1 prefix rows
                # (a memory shared by several takes is read once per step in
                # which one of them is live)
                kv_reads = int(sum(len(q) * (len(q) + 1) // 2 for q in seqs))
                k0 = 0
                for src, n in zip(srcs, takes or [1] * R):
                    kv_reads += max(len(q) for q in seqs[k0:k0 + n]) * len(src)
                    k0 += n
        while True:
            live = [i for i in range(R) if not spans[i].done]
            if not live:
                break
            feeds = []
            for i in live:
                pre = spans[i].prefix()
                feeds.append((i, pre[fed[i]:], fed[i]))
                fed[i] = len(pre)
            ts = time.perf_counter()
            lg = sess.step(feeds)
            t_dev += time.perf_counter() - ts
            if greedy:
                # one masked argmax over all live rows, in float32 (same ids as
                # the per-row float64 softmax argmax: exp/normalise is monotone)
                codes = [spans[i].state_code() for i in live]
                specs = [grammar_spec(vocab, c) for c in codes]
                govs = [spans[i]._governs(c, spans[i]._ban_index()) for i, c in zip(live, codes)]
                x = masked_row(lg, np.stack([g[0] for g in govs]), dtype=np.float32)  # steps 1-2, all rows at once
                for k, (_, cb, force) in enumerate(govs):
                    if cb is not None or force is not None:  # steps 3-4 of the rows that have them
                        x[k] = masked_row(x[k], True, cb, force, vocab, np.float32)
                ids = np.argmax(x, axis=1)
                for k, i in enumerate(live):
                    spans[i].scored(lg[k], govs[k][0], ids[k])  # (the argmax is taken outside advance())
                    spans[i].commit_greedy(ids[k], specs[k][1], specs[k][2])
            else:
                for k, i in enumerate(live):
                    spans[i].advance(lg[k])
            tokens += len(live)
            steps += 1
    out = []
    for s, st in zip(slots, spans):
        if st.n_masks == 0:
            out.append(None)
            continue
        out.append((restore_marked_input(_src_tokens(vocab, s.src), st.total), s.mask_track_names,
                    s.mask_bar_names))
    lp_all = [np.asarray(st.logp, dtype=np.float64) for st in spans] if score else None
    order = None
    if takes is not None:  # entry i: the list of request i's takes
        nested, order, k0 = [], [], 0
        for n in takes:
            ks = _rank_order(lp_all[k0:k0 + n]) if rq.rank else list(range(n))
            order.append(ks)
            nested.append(None if out[k0] is None else [out[k0 + k] for k in ks])
            k0 += n
        out = nested
    t3 = time.perf_counter()
    extra = {}
    if score:
        extra = {"logprobs": lp_all, "scores": [float(np.sum(a)) for a in lp_all]}
    if rq.rank:
        extra["order"] = order
    if any(s.bar_len for s in slots):
        extra["bar_fill"] = [list(st.fill) if st.bar_len else None for st in spans]
    if any(s.chords is not None for s in slots):
        extra["chords"] = [list(st.chord_spans) if st.chords is not None else None for st in spans]
    return out, {**extra, "tokens": tokens, "steps": steps, "prepare_s": t1 - t0,
                 "prefill_s": t2 - t1, "decode_s": t3 - t2, "step_call_s": t_dev,
                 "request_latency_s": latency, "kv_row_reads": kv_reads,
                 "generated": [list(st.total) for st in spans],
                 "seeds": seeds, "pitches": rq.allowed, "sources": len(srcs), "prefill_rows": int(sess.prefill_rows),
                 "decode_phases_s": dict(sess.phase_s)}


# --------------------------------------------------------------------------
# scores of given content: teacher-forced infill log-probabilities
# --------------------------------------------------------------------------
MAX_BODY = 98  # tokens of a note span the 100-token cap keeps: m_0 + 98, the 99th draw is dropped


class InfillScore(NamedTuple):
    """What score_infill / score_batch return for one request, entry for
    entry in the order the decode would have drawn the tokens."""
    logprobs: np.ndarray    # float64 [n]: token_logprobs(logit row, keep)[token]
    score: float            # their sum
    tokens: np.ndarray      # int64 [n]: the scored ids, <eos> included where it is scored
    mask_index: np.ndarray  # int32 [n]: the mask (in mask_targets order) of each entry
    greedy: np.ndarray      # int64 [n]: the masked argmax at each position (first index on ties)


class _ForcedPlan(NamedTuple):
    """The scoring plan of one request (host only): the decoder input and,
    per scored entry, the decoder row whose logits predict it, the grammar
    state code of that draw, the ban row (-1: none), the token and its mask."""
    src: np.ndarray
    tgt: list
    row: np.ndarray
    code: np.ndarray
    ban_idx: np.ndarray
    ids: np.ndarray
    mask_index: np.ndarray
    ban_rows: object  # boolean [k, V], or None


def _content_ids(vocab, bodies):
    """Given content as id lists: token strings through the vocabulary, ints
    as they are.  m_0, <eos>, an unknown string or an id outside the
    vocabulary raises ValueError."""
    V, table = vocab.vocab_size, vocab._char2idx
    m0, eos = vocab.char2index('m_0'), vocab.eos_index
    out = []
    for k, body in enumerate(bodies):
        if isinstance(body, (str, bytes)) or not hasattr(body, "__iter__"):
            raise ValueError("content: span %d is not a sequence of tokens (got %r)" % (k, body))
        seq = []
        for x in (body.tolist() if isinstance(body, np.ndarray) else body):
            if isinstance(x, str):
                x = table.get(x)
            elif isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                x = None
            if x is None or not 0 <= x < V:
                raise ValueError("content: span %d holds a token that is not in the vocabulary" % k)
            if x == m0 or x == eos:
                raise ValueError("content: span %d holds m_0 or <eos> (the bodies carry neither)" % k)
            seq.append(int(x))
        out.append(seq)
    return out


def _split_targets(vocab, stream):
    """The bodies of `decoder_targets`' stream [m_0, tokens..., <eos>] per
    span."""
    m0, eos = vocab.mask_indices[0], vocab.eos_index
    bodies = []
    for x in stream:
        if x == m0:
            bodies.append([])
        elif not bodies:
            raise ValueError("content: the target stream does not start with m_0")
        else:
            bodies[-1].append(x)
    for b in bodies:
        if b and b[-1] == eos:
            del b[-1]
    return bodies


def _forced_plan(vocab, src, target, all_controls, no_whole, bodies, bans=None):
    """Replay given content through a `_Span` without drawing: before every
    commit(id) the decoder row that predicts the token (the row of the input
    token before it), the span's state_code(), the ban row of the mask and
    the id are recorded.  The decoder input is the span's final tgt_inp,
    [m_0, body...] per mask.  Scored is exactly what the decode would have
    drawn: a control span its one token (the <eos> commit() appends is not
    drawn); a note span of n <= 97 tokens those and the <eos> that ends it; a
    note span of MAX_BODY tokens those alone (the cap ended it: the decode's
    99th draw is dropped whatever it is).  A note span whose last token is a
    control token was ended by that token (commit() appends the <eos>
    undrawn), so no <eos> is scored for it, and such a span may hold 99
    tokens -- the take the decode itself returns when its 99th draw is a
    control.  Raises ValueError for a wrong number of spans, a control span
    that does not hold one token, a longer note body, or tokens after the one
    that ends a span; touches neither the model nor np.random."""
    sp = _Span(vocab, src, target, all_controls, no_whole, True, None, bans=bans)
    if sp.n_masks == 0:
        raise ValueError("nothing is masked: there is nothing to score")
    if len(bodies) != sp.n_masks or len(target) < sp.n_masks:
        raise ValueError("content: %d spans for %d masks" % (len(bodies), sp.n_masks))
    ctrl = sp.all_controls
    for k, body in enumerate(bodies):
        if _target_code(target[k]) != 0:
            if len(body) != 1:
                raise ValueError("content: span %d is a control span and holds one token (got %d)"
                                 % (k, len(body)))
        elif len(body) > MAX_BODY and not (len(body) == MAX_BODY + 1 and body[-1] in ctrl):
            raise ValueError("content: span %d holds %d tokens, a note span at most %d"
                             % (k, len(body), MAX_BODY))
    row, code, bidx, ids, midx = [], [], [], [], []

    def record(k, tok):
        row.append(len(sp.tgt_inp) + len(sp.this_in) - 1)
        code.append(sp.state_code())
        bidx.append(-1 if sp.ban_of_mask is None else int(sp.ban_of_mask[k]))
        ids.append(tok)
        midx.append(k)
    for k, body in enumerate(bodies):
        for tok in body:
            if sp.mask_idx != k:
                raise ValueError("content: span %d goes on after the token that ends it" % k)
            record(k, tok)
            sp.commit(tok)
        if sp.mask_idx == k:  # still open: ended by <eos> (drawn, unless the cap or a control span ends it)
            if _target_code(target[k]) == 0 and len(sp.this_in) < MAX_BODY + 1:
                record(k, sp.eos)
            sp.commit(sp.eos)
    return _ForcedPlan(np.asarray(src, dtype=np.int64), list(sp.tgt_inp), np.asarray(row, dtype=np.int32),
                       np.asarray(code, dtype=np.uint8), np.asarray(bidx, dtype=np.int8),
                       np.asarray(ids, dtype=np.int64), np.asarray(midx, dtype=np.int32),
                       None if sp.ban_rows is None else np.asarray(sp.ban_rows, dtype=bool))


def _request_bodies(vocab, events, tracks_to_generate, bars_to_generate, content, allowed, what):
    """(src, target, no_whole, ban rows, bodies) of one request: its masked
    form, and `content` as a list of bodies -- with None the events' own content
    at the masked positions (`decoder_targets` of the events `_prepare` masked,
    empty bars filled in where it fills them).  Host only."""
    events = list(events)
    if len(bars_to_generate) == 0 or len(tracks_to_generate) == 0:
        raise ValueError("nothing is masked: there is nothing to %s" % what)
    (src, _, _, target, no_whole), bans = _masked_request(vocab, events, tracks_to_generate, bars_to_generate,
                                                          allowed)
    if content is None:
        _, tracks = mask_targets(events, tracks_to_generate, bars_to_generate)
        bodies = _split_targets(vocab, decoder_targets(events, vocab, tracks, bars_to_generate))
    else:
        if isinstance(content, (str, bytes)) or not hasattr(content, "__len__"):
            raise ValueError("content: one token sequence per mask (got %r)" % (content,))
        bodies = list(content)
    return src, target, no_whole, bans, bodies


def _score_plan(vocab, events, tracks_to_generate, bars_to_generate, all_controls, content, allowed):
    """The plan of one request from its events."""
    src, target, no_whole, bans, bodies = _request_bodies(vocab, events, tracks_to_generate, bars_to_generate,
                                                          content, allowed, "score")
    return _forced_plan(vocab, src, target, all_controls, no_whole, _content_ids(vocab, bodies), bans)


def _host_scores(vocab, plan, logits):
    """The definition, entry by entry: token_logprobs of logits[plan.row[n]]
    under the entry's keep at its id, and the masked argmax.  logits: a
    float32 array (or a dict) of rows indexed by decoder row."""
    lp = np.empty(len(plan.ids), dtype=np.float64)
    arg = np.empty(len(plan.ids), dtype=np.int64)
    for n in range(len(plan.ids)):
        k = int(plan.ban_idx[n])
        keep = _state_keep(vocab, int(plan.code[n]), None if k < 0 else plan.ban_rows[k])
        r = logits[int(plan.row[n])]
        lp[n] = token_logprobs(r, keep)[plan.ids[n]]
        arg[n] = np.argmax(masked_row(r, keep))
    return lp, arg


def _score_forward(model, plans):
    """One full forward (no_grad, eval) over all plans, sources and targets
    padded to the longest under the three key padding masks; the
    cross-attention weights are not computed.  Returns logits [B, T, V]."""
    dev = model.embedding.weight.device
    B = len(plans)
    S, T = max(len(q.src) for q in plans), max(len(q.tgt) for q in plans)
    src, tgt = np.zeros((B, S), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    spad, tpad = np.ones((B, S), dtype=bool), np.ones((B, T), dtype=bool)
    for b, q in enumerate(plans):
        src[b, :len(q.src)], spad[b, :len(q.src)] = q.src, False
        tgt[b, :len(q.tgt)], tpad[b, :len(q.tgt)] = q.tgt, False
    spad_t = torch.from_numpy(spad).to(dev)
    model.eval()
    need = model.need_weights
    model.need_weights = False
    try:
        with torch.no_grad():
            out, _ = model.forward(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev),
                                   src_key_padding_mask=spad_t,
                                   tgt_key_padding_mask=torch.from_numpy(tpad).to(dev),
                                   memory_key_padding_mask=spad_t.clone(),
                                   tgt_mask=gen_nopeek_mask(T).unsqueeze(0).to(dev))
    finally:
        model.need_weights = need
    return out


def _device_scores(vocab, all_controls, plans, logits):
    """smer_logprob_rows over every scored entry of every plan: one launch
    (one per group of requests whose ban rows together exceed the kernel's
    127) and one device-to-host copy of both outputs.  logits [B, T, V]
    float32 on the device."""
    from . import ops
    B, T, V = logits.shape
    dev = logits.device
    flat = logits.reshape(B * T, V)
    keep = torch.from_numpy(grammar_tables(vocab, all_controls)[0]).to(dev)
    groups, cur, k_cur = [], [], 0
    for b, q in enumerate(plans):
        k = 0 if q.ban_rows is None else len(q.ban_rows)
        if cur and k_cur + k > 127:
            groups.append(cur)
            cur, k_cur = [], 0
        cur.append(b)
        k_cur += k
    groups.append(cur)
    lps, args = {}, {}
    for grp in groups:
        rows, bidx, bits, k0 = [], [], [], 0
        for b in grp:
            q = plans[b]
            rows.append(q.row.astype(np.int64) + b * T)
            bidx.append(np.where(q.ban_idx >= 0, q.ban_idx.astype(np.int64) + k0, -1))
            if q.ban_rows is not None:
                bits.append(ban_bits(q.ban_rows))
                k0 += len(q.ban_rows)
        N = sum(len(r) for r in rows)
        put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(a).astype(dt))).to(dev)  # noqa: E731
        out = torch.empty(12 * N, dtype=torch.uint8, device=dev)  # float64 [N] | int32 [N]: one copy back
        ops.logprob_rows(flat, put(rows, np.int32), put([plans[b].code for b in grp], np.uint8), keep,
                         put(bidx, np.int8), put([x.view(np.int32) for x in bits], np.int32) if bits else None,
                         put([plans[b].ids for b in grp], np.int32), out[:8 * N].view(torch.float64),
                         out[8 * N:].view(torch.int32))
        host = out.cpu().numpy()
        lp, arg, at = host[:8 * N].view(np.float64), host[8 * N:].view(np.int32), 0
        for b in grp:
            n = len(plans[b].ids)
            lps[b], args[b] = lp[at:at + n].copy(), arg[at:at + n].astype(np.int64)
            at += n
    return [lps[b] for b in range(B)], [args[b] for b in range(B)]


def score_batch(model, requests, vocab, all_controls, *, contents=None, pitches=None, precision=None,
                device_score=True):
    """Teacher-forced log-probabilities of given infill content: what
    `logprobs=True` reports for the tokens a decode draws, for tokens it did
    not draw -- the bar that was there before masking, a take edited by hand,
    a take of another checkpoint or precision.  All tokens are known, so
    there is no step loop: ONE full forward over all requests (no_grad, eval,
    causal mask, sources and targets padded to the longest under the key
    padding masks, no cross-attention weights), then one launch of
    smer_logprob_rows over every scored entry and one copy back.

    requests: list of (events, tracks_to_generate, bars_to_generate), as
    generation_batch takes them.
    contents: None, or one value per request: None scores the events' own
    content at the masked positions (what wire.decoder_targets extracts, after
    the empty bars _prepare fills in) -- so the default call scores the
    original bar, and a take is scored by passing its restored tokens as
    `events`; otherwise a list with one sequence of token strings or ids per
    mask, in mask_targets order, without m_0 and without <eos>.
    What is scored is exactly what the decode would have drawn (see
    _forced_plan): a control span (d / o / p / t) its one token; a note span
    of n <= 97 tokens those and the <eos> after them, n + 1 entries; a note
    span of exactly 98 tokens was ended by the 100-token cap, so its 98
    tokens are scored and no end token is -- the decode's 99th draw is dropped
    whatever it is, so summed over it the probability is 1.  A note span
    whose last token is a control token was ended by that token and scores no
    <eos> either.  Every number is token_logprobs(logit row, keep)[id] with
    keep = allowed_ids(grammar state) & ~ban: the same float32 -> float64
    widening, -100.0 and maximum subtraction.  A token outside the state's
    keep set, or banned under `pitches`, is not an error: it scores from x =
    -100 like any other entry.
    pitches: as generation_batch (one value, or one per request).
    precision: arithmetic of the forward (None: the model's own).
    device_score: False, or a vocabulary above 512 tokens, copies the needed
    logits rows to the host and applies token_logprobs per entry (the
    definition).
    Raises ValueError -- before the model or np.random is touched -- for a
    request with nothing masked, a wrong number of spans, a control span whose
    length is not 1, a note body longer than 98 tokens, m_0, <eos> or an
    unknown token in a body, tokens after the one that ends a span, or a bad
    pitches.  np.random is neither read nor written, and the warm decode
    sessions are left alone.  Returns one InfillScore per request."""
    n = len(requests)
    if n == 0:
        raise ValueError("no request to score")
    if not isinstance(device_score, (bool, np.bool_)):
        raise ValueError("device_score must be True or False (got %r)" % (device_score,))
    if precision not in (None, "fp32", "bf16", "fp8"):
        raise ValueError("precision must be None, 'fp32', 'bf16' or 'fp8' (got %r)" % (precision,))
    if contents is None:
        contents = [None] * n
    elif not isinstance(contents, (list, tuple)) or len(contents) != n:
        raise ValueError("contents: None, or one value per request (%d)" % n)
    allowed = _check_pitches(pitches, [tr for _, tr, _ in requests], n)
    plans = [_score_plan(vocab, ev, tr, br, all_controls, c, a)
             for (ev, tr, br), c, a in zip(requests, contents, allowed)]
    with _Precision(model, precision):
        logits = _score_forward(model, plans)
        if device_score and vocab.vocab_size <= 512 and logits.is_cuda:
            lps, args = _device_scores(vocab, all_controls, plans, logits.float().contiguous())
        else:
            lps, args = [], []
            for b, q in enumerate(plans):
                need = np.unique(q.row)
                got = logits[b].index_select(0, torch.from_numpy(need.astype(np.int64)).to(logits.device))
                lp, arg = _host_scores(vocab, q, dict(zip(need.tolist(), got.float().cpu().numpy())))
                lps.append(lp)
                args.append(arg)
    return [InfillScore(lp, float(np.sum(lp)), q.ids.copy(), q.mask_index.copy(), arg)
            for q, lp, arg in zip(plans, lps, args)]


def score_infill(model, events, device, vocab, all_controls, tracks_to_generate, bars_to_generate, *,
                 content=None, pitches=None, precision="fp32", device_score=True):
    """score_batch for one request, with the plugin call's defaults: the
    forward runs in fp32 whatever precision the model trains in (None: the
    model's own).  content: None (the events' own content at the masked
    positions), or one token sequence per mask.  `device` is accepted for
    symmetry with generation_all; the forward runs where the model is.
    Returns an InfillScore; raises ValueError as score_batch does."""
    return score_batch(model, [(events, tracks_to_generate, bars_to_generate)], vocab, all_controls,
                       contents=[content], pitches=None if pitches is None else [
                           _check_pitches(pitches, tracks_to_generate)],
                       precision=precision, device_score=device_score)[0]


# --------------------------------------------------------------------------
# infill templates: the opening of a span is given, the model writes the rest
# --------------------------------------------------------------------------
def _check_template(template, vocab, src, target, all_controls, no_whole, bans=None, bar_len=0, chords=None):
    """Validated template of one request: None stays None; otherwise one row
    per mask, in mask_targets order, each None (free) or a sequence of items
    -- a token (string or id), ANY_PITCH, or '<eos>' as the last item of a
    note span's row.  Item i governs the draw made when the span holds i body
    tokens.  Returns the rows as tuples of token ids and TPL_PITCH (None for a
    free row), the form `_Span` and the device tape take.
    Every row is replayed through a `_Span` without drawing (the grammar flags
    follow token classes alone, so an ANY_PITCH item moves them as any pitch
    does).  Raises ValueError for a wrong number of rows; a control span's row
    that is not exactly one token of that span's class; a token outside the
    keep set of its state (the pitch ban of `bans` applied) or one its redraw
    check would reject; ANY_PITCH in a state, or on a track, that keeps no
    pitch; m_0 or an unknown token; '<eos>' anywhere but last; items after the
    token that ends the span; a note row of more than MAX_BODY body items.
    bar_len (fill_bar=: the bar's length in sixteenths, 0: none): the rows are
    replayed with the bar clock, and an item the clock bans is rejected too -- a
    row that overruns the bar, ANY_PITCH at a full bar, a closing '<eos>' on a
    bar that is not full.  chords (chords=: the request's `_Chords`): the
    clock runs as well, and a pitch token item that the chord at its onset bans
    is rejected; ANY_PITCH stays satisfiable, every effective set being non-empty.
    Touches neither the model nor np.random."""
    if template is None:
        return None
    if isinstance(template, (str, bytes)) or not hasattr(template, "__len__"):
        raise ValueError("template: one row per mask (got %r)" % (template,))
    sp = _Span(vocab, src, target, all_controls, no_whole, True, None, bans=bans, bar_len=bar_len, chords=chords)
    if len(template) != sp.n_masks or len(target) < sp.n_masks:
        raise ValueError("template: %d rows for %d masks" % (len(template), sp.n_masks))
    V, table, pitch = vocab.vocab_size, vocab._char2idx, _pitch_mask(vocab)
    rows = []
    for k, row in enumerate(template):
        if row is None:
            rows.append(None)
            continue
        if isinstance(row, (str, bytes)) or not hasattr(row, "__iter__"):
            raise ValueError("template: row %d is not a sequence of items (got %r)" % (k, row))
        items = row.tolist() if isinstance(row, np.ndarray) else list(row)
        note = _target_code(target[k]) == 0
        if not note and len(items) != 1:
            raise ValueError("template: row %d belongs to a control span and holds one token (got %d)"
                             % (k, len(items)))
        sp.mask_idx, sp.done = k, False  # every span starts from cleared flags: the rows replay apart
        sp._start_span()
        out = []
        for i, x in enumerate(items):
            if sp.done or sp.mask_idx != k:
                raise ValueError("template: row %d goes on after the token that ends its span" % k)
            if x is not ANY_PITCH:
                if isinstance(x, str):
                    x = table.get(x)
                elif isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                    x = None
                if x is None or not 0 <= x < V:
                    raise ValueError("template: row %d holds an item that is not in the vocabulary" % k)
                x = int(x)
                if x == sp.m0:
                    raise ValueError("template: row %d holds m_0" % k)
                if x == sp.eos and not (note and i == len(items) - 1):
                    raise ValueError("template: '<eos>' only as the last item of a note span's row (row %d)" % k)
            if i >= MAX_BODY and x != sp.eos:
                raise ValueError("template: row %d holds more than %d body items" % (k, MAX_BODY))
            check, ban = sp.spec()[1], sp.ban()
            keep, cb, _ = sp.governs()
            if cb is not None:
                if cb[pitch].all() if x is ANY_PITCH else cb[x]:
                    raise ValueError("template: row %d, item %d: %s not allow %s there (the bar holds %d of %d "
                                     "sixteenths)" % (k, i, "fill_bar does" if chords is None else "fill_bar and "
                                                      "chords do", "a pitch" if x is ANY_PITCH else
                                                      repr(vocab.index2char(x)), sp.clock.end,
                                                      bar_len or chords.L))
            if x is ANY_PITCH:
                ok = np.flatnonzero(keep & pitch if cb is None else keep & pitch & ~cb)
                if check is not None:
                    ok = [j for j in ok if not check(int(j))]
                if len(ok) == 0:
                    raise ValueError("template: row %d asks for a pitch where the grammar%s allows none (item %d)"
                                     % (k, " and pitches=" if ban is not None else "", i))
                x, tok = TPL_PITCH, int(ok[0])
            else:
                if not keep[x]:
                    raise ValueError("template: row %d, item %d: %r is not allowed there (grammar state %d%s)"
                                     % (k, i, vocab.index2char(x), sp.state_code(),
                                        ", pitches=" if ban is not None else ""))
                if check is not None and check(x):
                    raise ValueError("template: row %d, item %d: %r would be redrawn there (grammar state %d)"
                                     % (k, i, vocab.index2char(x), sp.state_code()))
                tok = x
            out.append(x)
            sp.commit(tok)
        rows.append(tuple(out))
    return rows


def _template_bodies(events, vocab, tracks_to_generate, bars_to_generate, content):
    """(bodies as id lists, target codes) of a request for the template
    builders: `content` in score_infill's format, or with None the events' own
    content at the masked positions."""
    src, target, _, _, bodies = _request_bodies(vocab, events, tracks_to_generate, bars_to_generate, content,
                                                None, "build a template from")
    n = int(np.sum(np.asarray(src) == vocab.char2index('m_0')))
    if len(bodies) != n or len(target) < n:
        raise ValueError("content: %d spans for %d masks" % (len(bodies), n))
    return _content_ids(vocab, bodies), [_target_code(t) for t in target[:n]]


def rhythm_template(events, vocab, tracks_to_generate, bars_to_generate, *, content=None):
    """The template that keeps a bar's rhythm and lets the model choose new
    notes: every note span's row is its content with each pitch token replaced
    by ANY_PITCH, closed by '<eos>' where the content's span ended on one (a
    body shorter than the 98-token cap whose last token is no control token);
    control spans are free (None).  content: score_infill's format (one
    sequence of tokens or ids per mask, without m_0 and <eos>); None: the
    events' own content at the masked positions.  Pass the result as
    `template=`; the call validates it against its grammar."""
    bodies, codes = _template_bodies(events, vocab, tracks_to_generate, bars_to_generate, content)
    pitch, eos = _pitch_mask(vocab), vocab.eos_index
    ctrl = {i for idxs in vocab.control_indices.values() for i in idxs}
    rows = []
    for body, code in zip(bodies, codes):
        if code != 0:
            rows.append(None)
            continue
        row = [ANY_PITCH if pitch[x] else x for x in body[:MAX_BODY]]
        if len(body) < MAX_BODY and not (body and body[-1] in ctrl):
            row.append(eos)
        rows.append(row)
    return rows


def opening_template(events, vocab, tracks_to_generate, bars_to_generate, *, content=None, keep=1):
    """The template that keeps the opening of every note span and lets the
    model finish it: each note span's row is the first `keep` body tokens of
    its content (all of them when it holds fewer); control spans are free.
    keep: one int in 0..98, or one per note span in mask order.  content: as
    rhythm_template's."""
    bodies, codes = _template_bodies(events, vocab, tracks_to_generate, bars_to_generate, content)
    n_note = sum(1 for c in codes if c == 0)
    ks = list(keep) if isinstance(keep, (list, tuple, np.ndarray)) else [keep] * n_note
    if len(ks) != n_note:
        raise ValueError("keep: one int, or one per note span (%d)" % n_note)
    for x in ks:
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not 0 <= x <= MAX_BODY:
            raise ValueError("keep must be an int in 0..%d (got %r)" % (MAX_BODY, x))
    rows, it = [], iter(ks)
    for body, code in zip(bodies, codes):
        rows.append(list(body[:int(next(it))]) if code == 0 else None)
    return rows

"""Generate tests/golden/nucleus_draws.npz: draws of the reference's own
`generation.sampling` with a temperature and a nucleus threshold.

RUN ONLY WHERE A CHECKOUT OF THE REFERENCE IS PRESENT (it is imported at run
time from the directory given on the command line; nothing of it is stored).  Writes data only: the
float32 logit rows, the grammar flags of every row, its (t, p), the seed,
the drawn ids and the MT19937 state after the last draw.

    python tests/golden/make_golden_nucleus.py <reference checkout>
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "generation.py")):
    sys.exit("usage: make_golden_nucleus.py <reference checkout>")
REF = sys.argv[1]
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(OUT, "..", ".."))
sys.path.insert(0, REF)
for _m in ("pretty_midi", "music21", "coloredlogs"):
    sys.modules.setdefault(_m, types.ModuleType(_m))

import vocab as ref_vocab          # noqa: E402  (reference)
import generation as ref_gen       # noqa: E402  (reference)

from smer_music_generation_amd.generation import _FLAG_NAMES, N_GRAMMAR_STATES, grammar_spec  # noqa: E402
from smer_music_generation_amd.vocab import WordVocab  # noqa: E402

CTRL = ['key', 'tensile', 'density', 'polyphony', 'occupation']
TS = (0.5, 0.8, 1.0, 1.3)
PS = (None, 0.0, 0.5, 0.9, 0.999)
SEED = 20
PER_COMBO = 3  # 4 * 5 * 3 = 60 rows (<= 64)


def main():
    rv = ref_vocab.WordVocab(0, CTRL)
    v = WordVocab(0, CTRL)
    assert rv.vocab_size == v.vocab_size
    V = rv.vocab_size
    rng = np.random.default_rng(SEED)
    combos = [(t, p) for t in TS for p in PS] * PER_COMBO
    n = len(combos)
    rows = (rng.standard_normal((n, V)) * rng.uniform(0.5, 6.0, (n, 1))).astype(np.float32)
    codes = rng.integers(0, N_GRAMMAR_STATES, n)
    flags = np.zeros((n, len(_FLAG_NAMES)), dtype=np.uint8)
    ids = np.zeros(n, dtype=np.int64)
    np.random.seed(SEED)
    for i, (t, p) in enumerate(combos):
        fl = grammar_spec(v, int(codes[i]))[0]  # flag names only: the reference applies them
        for k, name in enumerate(_FLAG_NAMES):
            flags[i, k] = bool(fl.get(name))
        ids[i] = ref_gen.sampling(torch.from_numpy(rows[i]), rv, p=p, t=t, **fl)
    st = np.random.get_state()
    np.savez_compressed(
        os.path.join(OUT, "nucleus_draws.npz"), rows=rows, flags=flags,
        flag_names=np.array(_FLAG_NAMES), t=np.array([c[0] for c in combos], dtype=np.float64),
        p=np.array([-1.0 if c[1] is None else c[1] for c in combos], dtype=np.float64),  # -1: None
        seed=np.int64(SEED), ids=ids, mt_key=np.asarray(st[1], dtype=np.uint32), mt_pos=np.int64(st[2]))
    print("wrote nucleus_draws.npz: %d rows, V = %d" % (n, V))


if __name__ == "__main__":
    main()

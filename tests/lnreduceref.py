"""The summation order of the LayerNorm dgamma / dbeta reductions, in numpy
float32, written down once and independently of the kernels
(csrc/train_ops.hip: smer_col_reduce_launch per call, and
smer_ln_param_reduce_batch for all of a step's sites in one launch).

One pass over rows [0, n) of a column: four row groups, group g taking rows
g, g + 4, ...; a group adds its rows round-robin into four accumulators
(a0: g, g + 16, ...; a1: g + 4, g + 20, ...; a2; a3) while four of them are
left, the remaining rows into a0; the group's sum is (a0 + a1) + (a2 + a3)
and the pass gives (r0 + r1) + (r2 + r3).  More than 64 rows: one pass per
64-row chunk, then one pass over the chunk sums."""
import numpy as np

NBLKS = (1, 3, 4, 5, 16, 17, 63, 64, 65, 127, 128, 129, 512, 1000)
NS = (8, 32, 33, 64, 96, 512)
MODES = ("both", "dgamma", "dbeta")


def one_pass(rows):
    """rows float32 [n, C] -> float32 [C]."""
    rows = np.asarray(rows, dtype=np.float32)
    n, C = rows.shape
    r = []
    for g in range(4):
        a = [np.zeros(C, np.float32) for _ in range(4)]
        b = g
        while b + 12 < n:
            for j in range(4):
                a[j] = a[j] + rows[b + 4 * j]
            b += 16
        while b < n:
            a[0] = a[0] + rows[b]
            b += 4
        r.append((a[0] + a[1]) + (a[2] + a[3]))
    return (r[0] + r[1]) + (r[2] + r[3])


def col_reduce(rows):
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    if n <= 64:
        return one_pass(rows)
    return one_pass(np.stack([one_pass(rows[c:c + 64]) for c in range(0, n, 64)]))


def ln_param_reduce(part, N, prior_gamma=None, prior_beta=None, accumulate=False, mode="both"):
    """part float32 [nblk, 2N] (dgamma | dbeta partials).  Returns (dgamma,
    dbeta) float32 [N], None for the one `mode` leaves out."""
    s = col_reduce(part)
    out = []
    for which, sl, prior in (("dgamma", s[:N], prior_gamma), ("dbeta", s[N:], prior_beta)):
        if mode not in ("both", which):
            out.append(None)
        elif accumulate:
            out.append(np.asarray(prior, np.float32) + sl)
        else:
            out.append(sl.copy())
    return tuple(out)


def any_order_bound(part, prior=None):
    """|fp32 column sum in any order - exact sum| <= (nblk + 2) 2^-24 sum|x|:
    each of the nblk - 1 adds (and the first add to a zero accumulator)
    rounds a partial sum of magnitude <= sum|x| by at most 2^-24 of it.
    With a prior (accumulate) the final add prior + sum rounds once more, by
    at most 2^-24 (|prior| + sum|x|)."""
    part = np.asarray(part, np.float64)
    s = np.abs(part).sum(axis=0)
    b = (part.shape[0] + 2) * 2.0 ** -24 * s
    if prior is not None:
        b = b + 2.0 ** -24 * (np.abs(np.asarray(prior, np.float64)) + s)
    return b


def make_partials(rng, nblk, N):
    """randn scaled over seven decades, element by element."""
    x = rng.standard_normal((nblk, 2 * N)) * 10.0 ** rng.integers(-3, 4, size=(nblk, 2 * N))
    return x.astype(np.float32)

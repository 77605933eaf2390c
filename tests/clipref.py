"""Float64 / numpy reference of the gradient-clipping kernels
(csrc/train_ops.hip: grad_sqnorm_kernel, clip_scale_kernel) and the error
bound of the device norm, derived from the kernel's summation tree."""
import numpy as np

# --- the summation tree of grad_sqnorm_kernel, one partial ------------------
# Each lane accumulator takes 16 squares in sequence (4 iterations x 4
# elements of a 16-B load), each add one rounding (the square is fused into
# the fma, so it adds none; the "+ 1" below pays for it anyway).  Then
# (a0 + a1) + (a2 + a3): 2 levels, the 64-lane butterfly: 6 levels, the four
# waves (w0 + w1) + (w2 + w3): 2 levels.
SEQ_ADDS = 16
TREE_DEPTH = 2 + 6 + 2
U = 2.0 ** -24  # fp32 unit roundoff
# All terms are >= 0, so a term passes through at most SEQ_ADDS + TREE_DEPTH
# roundings plus its own square: |partial - exact| <= (k u + O(u^2)) exact
# with k = SEQ_ADDS + TREE_DEPTH + 1.
PARTIAL_RTOL = (SEQ_ADDS + TREE_DEPTH + 1) * U
# The partials are combined in double (2^-53 per add: nothing visible), so
# the total carries PARTIAL_RTOL; sqrt halves a relative error; the double
# root is rounded to fp32 once (u).  1.01 covers the O(u^2) terms.
NORM_RTOL = 1.01 * (PARTIAL_RTOL / 2 + U)


def chunk(lib):
    """CH, read from smer_grad_sqnorm_nparts itself: the largest n with one partial."""
    lo, hi = 1, 1 << 30
    assert lib.smer_grad_sqnorm_nparts(lo) == 1 and lib.smer_grad_sqnorm_nparts(hi) > 1
    while lo < hi:  # largest n with nparts(n) == 1
        mid = (lo + hi + 1) // 2
        if lib.smer_grad_sqnorm_nparts(mid) == 1:
            lo = mid
        else:
            hi = mid - 1
    return lo


def partition(n, ch):
    """[(start, end)] of the chunks of a range of n floats."""
    return [(a, min(n, a + ch)) for a in range(0, n, ch)]


def sqnorm(g):
    """Sum of squares in float64."""
    g = np.asarray(g, dtype=np.float64)
    return float(np.dot(g, g))


def part_sqnorms(g, ch):
    """Float64 sum of squares of every chunk."""
    g = np.asarray(g, dtype=np.float64)
    return np.array([np.dot(g[a:b], g[a:b]) for a, b in partition(g.size, ch)], dtype=np.float64)


def clip_scale32(norm32, max_norm):
    """min(1, max_norm / (norm + 1e-6)) with every operation in float32, in
    torch.nn.utils.clip_grad_norm_'s order: clip_coef = max_norm /
    (total_norm + 1e-6) is Tensor.__rtruediv__, reciprocal() * max_norm (two
    roundings), clamped to 1.0; 0 when the norm is not finite (the step is
    skipped)."""
    n = np.float32(norm32)
    if not np.isfinite(n):
        return np.float32(0.0)
    with np.errstate(over="ignore", divide="ignore"):
        coef = (np.float32(1.0) / (n + np.float32(1e-6))) * np.float32(max_norm)
    return np.float32(min(np.float32(1.0), coef))


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)

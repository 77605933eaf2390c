"""The numpy-fp32 mirror of the LayerNorm dgamma / dbeta reduction order
(tests/lnreduceref.py) against float64 column sums, over the (nblk, N) table
the GPU test holds the kernels to (tests/test_ln_param_reduce_gpu.py)."""
import numpy as np
import pytest

from tests import lnreduceref as R


@pytest.mark.parametrize("N", R.NS)
def test_mirror_within_any_order_bound_of_float64(N):
    rng = np.random.default_rng(1000 + N)
    for nblk in R.NBLKS:
        part = R.make_partials(rng, nblk, N)
        got = R.col_reduce(part)
        assert got.dtype == np.float32 and got.shape == (2 * N,)
        ref = part.astype(np.float64).sum(axis=0)
        err = np.abs(got.astype(np.float64) - ref)
        bound = R.any_order_bound(part)
        assert (err <= bound).all(), (nblk, N, float((err / np.maximum(bound, 1e-300)).max()))


def test_mirror_is_the_two_level_order():
    """Written out by hand for a size with a ragged last chunk: 65 rows are
    the 64-row pass, the 1-row pass, and a pass over those two sums."""
    rng = np.random.default_rng(7)
    part = R.make_partials(rng, 65, 8)
    a, b = R.one_pass(part[:64]), R.one_pass(part[64:])
    z = np.zeros_like(a)
    # a pass over two rows: group 0 has row 0, group 1 row 1, groups 2, 3 nothing
    want = (((a + z) + (z + z)) + ((b + z) + (z + z))) + ((z + z) + (z + z))
    assert np.array_equal(R.col_reduce(part), want)
    # 12 rows: no group has four rows left, so group g chains g, g + 4, g + 8 in a0
    p12 = part[:12]
    groups = [(((p12[g] + p12[g + 4]) + p12[g + 8]) + z) + (z + z) for g in range(4)]
    assert np.array_equal(R.one_pass(p12), (groups[0] + groups[1]) + (groups[2] + groups[3]))
    # 17 rows: every group's first four rows go round-robin, row 16 joins group 0's a0
    p17 = part[:17]
    groups = [(p17[g] + p17[g + 4]) + (p17[g + 8] + p17[g + 12]) for g in range(1, 4)]
    g0 = ((p17[0] + p17[16]) + p17[4]) + (p17[8] + p17[12])
    assert np.array_equal(R.one_pass(p17), (g0 + groups[0]) + (groups[1] + groups[2]))


def test_modes_and_accumulate():
    rng = np.random.default_rng(9)
    part = R.make_partials(rng, 5, 33)
    pg, pb = rng.standard_normal(33).astype(np.float32), rng.standard_normal(33).astype(np.float32)
    s = R.col_reduce(part)
    g, b = R.ln_param_reduce(part, 33, pg, pb, accumulate=True)
    assert np.array_equal(g, pg + s[:33]) and np.array_equal(b, pb + s[33:])
    g, b = R.ln_param_reduce(part, 33, mode="dgamma")
    assert b is None and np.array_equal(g, s[:33])
    g, b = R.ln_param_reduce(part, 33, mode="dbeta")
    assert g is None and np.array_equal(b, s[33:])

"""smer_ln_param_reduce_batch (all LayerNorm dgamma / dbeta reductions of a
step in one launch) against the per-call reductions it replaces, bit for
bit, at the edges of the two-level rule (64-row chunks, then the chunk sums)
and of the 64-column tiling; against the numpy-fp32 mirror of that order
(tests/lnreduceref.py), bit for bit; and against float64 column sums within
the any-order bound, which would catch both paths being wrong together.

Each N is one table of 14 nblk x {overwrite, accumulate} x {both, dgamma,
dbeta} = 84 sites in one launch, nblk = 1 next to nblk = 1000; one more
table mixes every N.  Outputs sit in NaN frames, partial rows past nblk are
NaN."""
import numpy as np
import pytest
import torch

from tests import lnreduceref as R

pytestmark = pytest.mark.gpu
FRAME = 8    # NaN floats on either side of an output
EXTRA = 3    # NaN partial rows past nblk


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rows_for(nblk):
    """A LayerNorm row count whose backward writes nblk partial rows (16 rows
    per workgroup up to 16384 rows)."""
    M = 16 * nblk
    assert M <= 16384
    return M


class _Site:
    def __init__(self, rng, nblk, N, accumulate, mode):
        self.nblk, self.N, self.accumulate, self.mode = nblk, N, accumulate, mode
        self.M = _rows_for(nblk)
        self.part = R.make_partials(rng, nblk, N)
        self.prior = rng.standard_normal((2, N)).astype(np.float32) * 3.0

    def outputs(self):
        """Framed dgamma / dbeta buffers with the prior inside, the views into them."""
        bufs, views = [], []
        for k, which in enumerate(("dgamma", "dbeta")):
            buf = torch.full((self.N + 2 * FRAME,), float("nan"), device="cuda")
            buf[FRAME:FRAME + self.N] = torch.from_numpy(self.prior[k]).cuda()
            bufs.append(buf)
            views.append(buf[FRAME:FRAME + self.N] if self.mode in ("both", which) else None)
        return bufs, views

    def check_frames(self, bufs, views):
        for k, (buf, v) in enumerate(zip(bufs, views)):
            assert torch.isnan(buf[:FRAME]).all() and torch.isnan(buf[FRAME + self.N:]).all(), self.tag()
            if v is None:  # an output the site leaves out is not touched
                assert np.array_equal(buf[FRAME:FRAME + self.N].cpu().numpy(), self.prior[k]), self.tag()

    def tag(self):
        return (self.nblk, self.N, self.accumulate, self.mode)


def _run_per_call(site):
    from smer_music_generation_amd import _lib, ops
    lib = _lib.load()
    assert lib.smer_layernorm_bwd_nblk(site.M, site.N) == site.nblk
    nbytes = lib.smer_layernorm_bwd_workspace(site.M, site.N)
    ws = torch.full((nbytes // 4,), float("nan"), device="cuda")
    ws[:site.part.size] = torch.from_numpy(site.part.reshape(-1)).cuda()
    bufs, views = site.outputs()
    _lib.call("smer_layernorm_param_reduce", site.M, site.N, ws.data_ptr(), nbytes,
              ops._p(views[0]), ops._p(views[1]), int(site.accumulate), ops._stream())
    return bufs, views


def _run_batch(sites):
    from smer_music_generation_amd import ops
    slots, outs, rows = [], [], []
    for s in sites:
        slot = torch.full(((s.nblk + EXTRA) * 2 * s.N,), float("nan"), device="cuda")
        slot[:s.part.size] = torch.from_numpy(s.part.reshape(-1)).cuda()
        slots.append(slot)
        bufs, views = s.outputs()
        outs.append((bufs, views))
        rows.append((slot.view(torch.uint8), s.M, s.N, views[0], views[1], s.accumulate))
    table = ops.LnReduceTable(rows, torch.device("cuda"))
    ops.ln_param_reduce_batch(table)
    torch.cuda.synchronize()
    return outs


def _check(sites):
    batch = _run_batch(sites)
    for s, (bufs_b, views_b) in zip(sites, batch):
        bufs_p, views_p = _run_per_call(s)
        torch.cuda.synchronize()
        s.check_frames(bufs_b, views_b)
        s.check_frames(bufs_p, views_p)
        mirror = R.ln_param_reduce(s.part, s.N, s.prior[0], s.prior[1], s.accumulate, s.mode)
        ref64 = s.part.astype(np.float64).sum(axis=0)
        for k in range(2):
            if views_b[k] is None:
                assert mirror[k] is None
                continue
            got = views_b[k].cpu().numpy()
            assert torch.equal(views_b[k], views_p[k]), ("batch != per call", s.tag(), k)
            assert np.array_equal(got, mirror[k]), ("batch != mirror", s.tag(), k)
            sl = slice(k * s.N, (k + 1) * s.N)
            want = ref64[sl] + (s.prior[k].astype(np.float64) if s.accumulate else 0.0)
            bound = R.any_order_bound(s.part[:, sl], s.prior[k] if s.accumulate else None)
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), ("float64", s.tag(), k, float((err / np.maximum(bound, 1e-300)).max()))


def _sites_for(rng, N):
    return [_Site(rng, nblk, N, acc, mode) for nblk in R.NBLKS for acc in (False, True) for mode in R.MODES]


@pytest.mark.parametrize("N", R.NS)
def test_batch_equals_per_call_mirror_and_float64(N):
    _check(_sites_for(np.random.default_rng(N), N))


def test_one_table_mixing_every_shape():
    """Sites of different nblk and N in one launch (the grid's x is sized by
    the widest; narrower sites' surplus workgroups leave at once), nblk = 1
    next to nblk = 1000, every mode."""
    rng = np.random.default_rng(99)
    sites = []
    for i, N in enumerate(R.NS):
        for j, nblk in enumerate((1, 1000, 64, 65, 5, 129)):
            sites.append(_Site(rng, nblk, N, (i + j) % 2 == 1, R.MODES[(i + 2 * j) % 3]))
    _check(sites)


def test_entry_rejects_what_the_kernel_cannot_hold():
    from smer_music_generation_amd import _lib, ops
    t = ops.LnReduceTable([(torch.zeros(4 * 2 * 8 * 4, dtype=torch.uint8, device="cuda"), 64, 8,
                            torch.zeros(8, device="cuda"), None, False)], torch.device("cuda"))
    t.host["nblk"][0] = 4097
    with pytest.raises(_lib.SmerError):
        ops.ln_param_reduce_batch(t)
    t.host["nblk"][0] = 4
    t.host["dgamma"][0] = 0
    with pytest.raises(_lib.SmerError):
        ops.ln_param_reduce_batch(t)

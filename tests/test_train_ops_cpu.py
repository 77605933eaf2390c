"""Host-side contract of the training-tail entry points (csrc/train_ops.hip,
csrc/norm_embed.hip): the workspace sizes the wrappers allocate from, and the
argument checks that must refuse a call before anything is launched (so these
run without a GPU; the pointers are dummies that are never dereferenced)."""
import ctypes

import pytest

F32, BF16, BAD_DTYPE = 0, 1, 7
_HOST_BUF = (ctypes.c_uint8 * (1 << 16))()


@pytest.fixture(scope="module")
def lib():
    from smer_music_generation_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ptr():
    """A 16-byte aligned dummy address inside a live host buffer."""
    return (ctypes.addressof(_HOST_BUF) + 15) & ~15


def _refused(lib, status, *words):
    msg = lib.smer_last_error()
    assert status < 0, status
    assert msg, "refused without a message"
    for w in words:
        assert w.encode() in msg, (w, msg)


# the shapes of tests/test_train_ops_gpu.py's colsum cases
@pytest.mark.parametrize("M,N", [(1, 8), (77, 309), (4096, 520), (4100, 520), (200, 64), (64, 1),
                                 (65, 1), (64 * 64 + 1, 3), (64 * 128 + 1, 3)])
def test_colsum_workspace_formula(lib, M, N):
    nblk = -(-M // 64)
    want = nblk * N * 4
    if nblk > 64:  # second stage: one partial row per 64 row blocks
        want += -(-nblk // 64) * N * 4
    assert lib.smer_colsum_workspace(M, N) == want


@pytest.mark.parametrize("d", [64, 768, 1024])
@pytest.mark.parametrize("n", [0, 1, 512, 513, 1091])
def test_embed_bwd_workspace_formula(lib, n, d):
    V = 309
    assert lib.smer_embed_bwd_workspace(V, d, n) == max(1, -(-n // 512)) * V * d * 4


def _embed_bwd(lib, p, *, d=64, ld0=None, ws_bytes=None, dtype=F32):
    V, n0 = 4, 4
    need = lib.smer_embed_bwd_workspace(V, d, n0)
    return lib.smer_embed_bwd(dtype, V, d, 1.0, p, p, d if ld0 is None else ld0, n0, 0.0, 0,
                              None, None, 0, 0, 0.0, 0, p, p, need if ws_bytes is None else ws_bytes,
                              None)


def test_embed_bwd_refuses_bad_arguments_before_launch(lib, ptr):
    _refused(lib, _embed_bwd(lib, ptr, d=72), "smer_embed_bwd", "d % 64")
    _refused(lib, _embed_bwd(lib, ptr, d=1088), "smer_embed_bwd", "1024")
    _refused(lib, _embed_bwd(lib, ptr, ld0=12), "smer_embed_bwd", "16-B aligned")
    need = lib.smer_embed_bwd_workspace(4, 64, 4)
    _refused(lib, _embed_bwd(lib, ptr, ws_bytes=need - 1), "smer_embed_bwd", "workspace")
    _refused(lib, _embed_bwd(lib, ptr, ws_bytes=0), "smer_embed_bwd", "workspace")


def _ln_fp8(lib, p, *, N=64, ldq=64):
    return lib.smer_layernorm_fwd_fp8(4, N, p, 64, p, p, 1e-5, p, 64, p, p, p, ldq, p, p, None)


def test_layernorm_fwd_fp8_refuses_bad_shapes_before_launch(lib, ptr):
    _refused(lib, _ln_fp8(lib, ptr, N=12), "smer_layernorm_fwd_fp8", "N % 8")
    _refused(lib, _ln_fp8(lib, ptr, ldq=12), "smer_layernorm_fwd_fp8", "strides")


@pytest.mark.parametrize("src,dst", [(BAD_DTYPE, F32), (F32, BAD_DTYPE), (BAD_DTYPE, BAD_DTYPE), (-1, BF16)])
def test_cast_refuses_unknown_dtype_before_launch(lib, ptr, src, dst):
    _refused(lib, lib.smer_cast(src, dst, 16, ptr, ptr, None), "smer_cast", "dtype")
    _refused(lib, lib.smer_cast2d(src, dst, 4, 4, ptr, 4, ptr, 4, None), "smer_cast2d", "dtype")


def test_colsum_refuses_unknown_dtype_and_short_workspace_before_launch(lib, ptr):
    M, N = 77, 309
    need = lib.smer_colsum_workspace(M, N)
    _refused(lib, lib.smer_colsum(BAD_DTYPE, M, N, ptr, 312, ptr, 0, ptr, need, None), "smer_colsum", "dtype")
    _refused(lib, lib.smer_colsum(F32, M, N, ptr, 312, ptr, 0, ptr, need - 1, None), "smer_colsum", "workspace")
    _refused(lib, lib.smer_colsum(F32, M, N, ptr, 312, ptr, 0, None, need, None), "smer_colsum", "workspace")
    # the two-stage shape needs its second-stage scratch too
    M2, N2 = 4100, 520
    first = -(-M2 // 64) * N2 * 4
    assert lib.smer_colsum_workspace(M2, N2) > first
    _refused(lib, lib.smer_colsum(F32, M2, N2, ptr, 528, ptr, 0, ptr, first, None), "smer_colsum", "workspace")

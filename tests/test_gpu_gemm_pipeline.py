"""The seams of the big tile's pipelined K loop (gpp_gemm.hip, ``gemm_tile``: the clean loop of the 128 x 128 row-contiguous tile)
against the CPU reference of tests/gemm_reference.py.

The clean loop runs the iterations whose PREFETCHED chunk of 16 k's is in range and untouched by a mask for both operands; the
iterations before and after it take the general path.  Full tiles are its precondition, so M = N is a multiple of 128 here, and K
makes the clean range empty (16: one chunk; 17: the only prefetched chunk is ragged), one iteration long (32), start at chunk 0 and
end at the last chunk (48, 64, 80, 144, 272), or stop before a ragged last chunk (47, 130).  With the LAUUM form (both masks 2,
klo_mode 3, lower output) the range of a tile starts at its own first row or column and its first chunks are cut by the mask, so
general iterations flank the clean ones on both sides, by a tile-dependent count.  Operands are windows of NaN-filled buffers and C
a window of a sentinel-filled one: a chunk stored to the wrong LDS buffer, stored twice, or read before its store poisons or
changes the small-integer result, which is compared for equality.  (``ctx.gemm`` has no k_reverse argument: the reversed sweep is
reached through the internal drivers only, and is not covered here.)
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_reference as gr  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 3  # GPP_OPT_GEMM_TILE value of the 128 x 128 tile
VARIANT = "TN"  # both operands stored [k][row]: the big tile's lean path
KS = (16, 32, 48, 64, 80, 144, 272, 17, 47, 130)
SCALARS = ((1.0, 0.0), (-1.0, 1.0), (-0.5, 2.0))
#: the mask / hint combinations the package itself launches, after the plain product
PACKAGE_PAIRS = ((0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 0, 2), (0, 2, 2, 0), (2, 2, 3, 0))  # (a_mask, b_mask, klo_mode, khi_mode)
#: (M = N, c_tri, the pairs valid for the case): four full tiles, every pair; the LAUUM form on the lower triangle of 3 x 3 tiles
CASES = ((256, 0, PACKAGE_PAIRS), (384, 1, ((2, 2, 3, 0),)))

_cache = {}


def _inputs(n, K):
    assert gr.TILES[TILE] == (128, 128) and gr.VARIANTS[VARIANT] == (1, 0) and n % 128 == 0
    if (n, K) not in _cache:
        A, B, C0 = gr.exact_inputs(n, n, K, seed=31000 + 10 * n + K)
        sa, sb = gr.store_operands(A, B, VARIANT)
        _cache[n, K] = (A, B, C0, sa.window(torch.from_numpy(sa.buf).cuda()), sb.window(torch.from_numpy(sb.buf).cuda()))
    return _cache[n, K]


def _run(ctx, dA, dB, n, K, C_init, alpha, beta, am, bm, klo, khi, c_tri):
    """One gpp_gemm on the forced tile; the n x n window of C afterwards, after checking that nothing around it changed."""
    from gpplus_amd.backend import OPT_GEMM_TILE

    sc = gr.store_output(C_init)
    dC = torch.from_numpy(sc.buf).cuda()
    ctx.set_option(OPT_GEMM_TILE, TILE)
    try:
        ctx.gemm(1, 0, n, n, K, alpha, dA, dB, beta, sc.window(dC), a_mask=am, b_mask=bm, klo_mode=klo, khi_mode=khi, c_tri=c_tri)
    finally:
        ctx.set_option(OPT_GEMM_TILE, 0)
    out = dC.cpu().numpy()
    g = sc.guard_mask()
    assert gr.same_bits(out[g], sc.buf[g]), "gpp_gemm wrote outside the window of C"
    return sc.window(out)[:n, :n]


def _c_init(C0, beta, c_tri):
    """What C holds before the call: C0, with NaN on the written entries when beta = 0 (they must not be read into the result)."""
    C = np.asarray(C0, dtype=np.float64).copy()
    if beta == 0.0:
        C[gr.selected(c_tri, *C.shape)] = np.nan
    return C


def _assert_same(got, ref, label):
    bad = ~(got == ref)
    if bad.any():
        m, n = (int(x) for x in np.argwhere(bad)[0])
        pytest.fail(f"{label}: {int(bad.sum())} wrong entries, the first C[{m}][{n}] = {got[m, n]!r} (reference {ref[m, n]!r}) in tile "
                    f"({m // 128}, {n // 128})")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n,c_tri,pairs", CASES, ids=["full4", "lauum9"])
def test_clean_loop_seams(gpu_ctx, n, c_tri, pairs, K):
    A, B, C0, dA, dB = _inputs(n, K)
    for am, bm, klo, khi in pairs:
        P = gr.masked_matmul(A, B, am, bm)
        for alpha, beta in SCALARS:
            ref = gr.masked_product(A, B, am, bm, c_tri, alpha, beta, C0, P=P)
            Ci = _c_init(C0, beta, c_tri)
            label = f"{n}x{n}x{K} masks ({am}, {bm}) c_tri {c_tri} alpha {alpha} beta {beta}"
            base = _run(gpu_ctx, dA, dB, n, K, Ci, alpha, beta, am, bm, 0, 0, c_tri)
            _assert_same(base, ref, label)
            if (klo, khi) != (0, 0):
                got = _run(gpu_ctx, dA, dB, n, K, Ci, alpha, beta, am, bm, klo, khi, c_tri)
                _assert_same(got, ref, f"{label} klo_mode {klo} khi_mode {khi}")
                assert gr.same_bits(got, base), f"{label}: hint ({klo}, {khi}) changed bits of the result"


@pytest.mark.parametrize("n,c_tri,am,bm,klo", [(256, 0, 0, 0, 0), (384, 1, 2, 2, 3)], ids=["full4", "lauum9"])
def test_consecutive_calls_agree_bitwise(gpu_ctx, n, c_tri, am, bm, klo):
    """Standard normals, K = 272 (clean iterations with general ones around them): two calls on the same operands give the same bits."""
    K = 272
    A, B, C0 = gr.real_inputs(n, n, K, seed=4242 + n)
    sa, sb = gr.store_operands(A, B, VARIANT)
    dA, dB = sa.window(torch.from_numpy(sa.buf).cuda()), sb.window(torch.from_numpy(sb.buf).cuda())
    first = _run(gpu_ctx, dA, dB, n, K, C0, -0.5, 2.0, am, bm, klo, 0, c_tri)
    second = _run(gpu_ctx, dA, dB, n, K, C0, -0.5, 2.0, am, bm, klo, 0, c_tri)
    sel = gr.selected(c_tri, n, n)
    assert not np.isnan(first[sel]).any()
    assert gr.same_bits(first, second)

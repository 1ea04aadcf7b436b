"""Every work-group tile, operand layout, mask pair and K-range mode of gpp_gemm / gpp_gemm_batched (gpp_gemm.hip, ``gemm_tile``)
against the CPU reference of tests/gemm_reference.py.

The tile is forced through GPP_OPT_GEMM_TILE (left to itself the launcher picks 32 x 32 for every shape small enough to test).
Operands are windows of NaN-filled buffers and C a window of a sentinel-filled one, so an element kept past M, N or K poisons the
result and a store outside M x N is seen.  The exact cases use small integers: every partial sum is an integer far below 2^53,
any summation order gives the same fp64 value, and the comparison is for equality — one index or predicate off by one fails them,
and the first wrong entry names its tile.  The real-valued cases are held to the derived bound of ``gemm_reference.error_bound``.
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_reference as gr  # noqa: E402

pytestmark = pytest.mark.gpu

#: (tile option, layout): the square tiles in all three layouts; 128 x 32 (the tall tile of the internal drivers) likewise
TILE_VARIANTS = [(t, v) for t in sorted(gr.TILES) for v in gr.VARIANTS]
SQUARE_TILE_VARIANTS = [(t, v) for t, v in TILE_VARIANTS if gr.TILES[t][0] == gr.TILES[t][1]]
SCALARS = ((1.0, 0.0), (-0.5, 2.0))
#: the mask / hint combinations the package itself launches, after the plain product
PACKAGE_PAIRS = ((0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 0, 2), (0, 2, 2, 0), (2, 2, 3, 0))  # (a_mask, b_mask, klo_mode, khi_mode)

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _exact(M, N, K):
    return _cached(("exact", M, N, K), lambda: gr.exact_inputs(M, N, K, seed=1000 * M + 10 * N + K))


def _exact_ref(M, N, K, am, bm, c_tri, alpha, beta):
    """Reference of the seeded exact inputs of this shape; the int64 product is computed once per (shape, mask pair)."""
    A, B, C0 = _exact(M, N, K)
    P = _cached(("P", M, N, K, am, bm), lambda: gr.masked_matmul(A, B, am, bm))
    return gr.masked_product(A, B, am, bm, c_tri, alpha, beta, C0, P=P)


@contextlib.contextmanager
def _forced_tile(ctx, tile):
    from gpplus_amd.backend import OPT_GEMM_TILE

    ctx.set_option(OPT_GEMM_TILE, tile)
    try:
        yield
    finally:
        ctx.set_option(OPT_GEMM_TILE, 0)


def _c_init(C0, beta, c_tri):
    """What C holds before the call: C0, with NaN on the written entries when beta = 0 (they must not be read into the result)."""
    C = np.asarray(C0, dtype=np.float64).copy()
    if beta == 0.0:
        C[gr.selected(c_tri, *C.shape)] = np.nan
    return C


class _Operands:
    """op(A), op(B) of one case on the device, in the variant's layout, inside their NaN guards; uploaded once, used by every
    launch of the case (the masks are the kernel's business)."""

    def __init__(self, variant, A_op, B_op, same=False):
        self.tA, self.tB = gr.VARIANTS[variant]
        self.M, self.K = A_op.shape
        self.N = B_op.shape[1]
        sa, sb = gr.store_operands(A_op, B_op, variant)
        self.A = sa.window(torch.from_numpy(sa.buf).cuda())
        if same:  # one tensor for both operands
            assert sa.buf.shape == sb.buf.shape and gr.same_bits(sa.buf, sb.buf)
            self.B = self.A
        else:
            self.B = sb.window(torch.from_numpy(sb.buf).cuda())

    def run(self, ctx, C_init, alpha, beta, a_mask=0, b_mask=0, klo_mode=0, khi_mode=0, c_tri=0):
        """One gpp_gemm; returns the M x N window of C afterwards, after checking that nothing around it changed."""
        sc = gr.store_output(C_init)
        dC = torch.from_numpy(sc.buf).cuda()
        ctx.gemm(self.tA, self.tB, self.M, self.N, self.K, alpha, self.A, self.B, beta, sc.window(dC), a_mask=a_mask, b_mask=b_mask,
                 klo_mode=klo_mode, khi_mode=khi_mode, c_tri=c_tri)
        out = dC.cpu().numpy()
        g = sc.guard_mask()
        assert gr.same_bits(out[g], sc.buf[g]), "gpp_gemm wrote outside the M x N window of C"
        return sc.window(out)[: self.M, : self.N]


def _assert_same(got, ref, tile, label):
    """Equality with the exact reference (no NaN anywhere); names the first wrong entry and its tile."""
    bad = ~(got == ref)
    if bad.any():
        tm, tn = gr.TILES[tile]
        m, n = (int(x) for x in np.argwhere(bad)[0])
        pytest.fail(f"{label}: {int(bad.sum())} wrong entries, the first C[{m}][{n}] = {got[m, n]!r} (reference {ref[m, n]!r}) in tile "
                    f"({m // tm}, {n // tn}) of {tm} x {tn}, wrong tile rows {sorted(set((np.argwhere(bad)[:, 0] // tm).tolist()))} "
                    f"columns {sorted(set((np.argwhere(bad)[:, 1] // tn).tolist()))}")


def _check_exact(ctx, ops, tile, C0, am, bm, hints, c_tri, alpha, beta, ref, label):
    """The unhinted product equals the reference; every hinted one equals the reference and, bit for bit, the unhinted one."""
    Ci = _c_init(C0, beta, c_tri)
    base = ops.run(ctx, Ci, alpha, beta, a_mask=am, b_mask=bm, c_tri=c_tri)
    _assert_same(base, ref, tile, f"{label} masks ({am}, {bm}) c_tri {c_tri} alpha {alpha} beta {beta}")
    for klo, khi in hints:
        got = ops.run(ctx, Ci, alpha, beta, a_mask=am, b_mask=bm, klo_mode=klo, khi_mode=khi, c_tri=c_tri)
        _assert_same(got, ref, tile, f"{label} masks ({am}, {bm}) klo_mode {klo} khi_mode {khi} c_tri {c_tri} alpha {alpha} beta {beta}")
        assert gr.same_bits(got, base), f"{label} masks ({am}, {bm}): hint ({klo}, {khi}) changed bits of the result"
    return base


@pytest.mark.parametrize("tile,variant", TILE_VARIANTS)
def test_mask_matrix(gpu_ctx, tile, variant):
    """All 9 mask pairs, unhinted and with every legal hint, at (3 Tm + 1, 2 Tn + 3, 3 Tm + 5): interior tiles whose K range passes
    through predicated, clean and mask-cut chunks, a ragged last tile row of ONE row, odd M, N and K."""
    tm, tn = gr.TILES[tile]
    M, N, K = 3 * tm + 1, 2 * tn + 3, 3 * tm + 5
    A, B, C0 = _exact(M, N, K)
    ops = _Operands(variant, A, B)
    with _forced_tile(gpu_ctx, tile):
        for am, bm in gr.MASK_PAIRS:
            for alpha, beta in SCALARS:
                ref = _exact_ref(M, N, K, am, bm, 0, alpha, beta)
                _check_exact(gpu_ctx, ops, tile, C0, am, bm, gr.legal_hints(am, bm), 0, alpha, beta, ref, f"{variant} {M}x{N}x{K}")


@pytest.mark.parametrize("tile,variant", TILE_VARIANTS)
def test_ragged_edges(gpu_ctx, tile, variant):
    """Extents of 1, one short of and one past the tile, K below one MFMA step, K = 0, K one past a 64-wide chunk, N = 2."""
    tm, tn = gr.TILES[tile]
    with _forced_tile(gpu_ctx, tile):
        for M, N, K in [(1, 1, 1), (tm + 1, tn - 1, 3), (2 * tm + 1, tn + 2, 65), (tm, tn, 0), (tm + 1, 2, 17)]:
            A, B, C0 = _exact(M, N, K)
            ops = _Operands(variant, A, B)
            for am, bm, klo, khi in PACKAGE_PAIRS:
                for alpha, beta in SCALARS:
                    ref = _exact_ref(M, N, K, am, bm, 0, alpha, beta)
                    if K == 0:  # nothing to add: beta*C0, exact zeros with beta = 0
                        np.testing.assert_array_equal(ref, beta * C0.astype(np.float64))
                    hints = [(klo, khi)] if (klo, khi) != (0, 0) else []
                    _check_exact(gpu_ctx, ops, tile, C0, am, bm, hints, 0, alpha, beta, ref, f"{variant} {M}x{N}x{K}")


@pytest.mark.parametrize("tile,variant", SQUARE_TILE_VARIANTS)
def test_triangular_output(gpu_ctx, tile, variant):
    """c_tri 1 and 2: the selected triangle equals the reference, the other one keeps its bits (C0 is what _check_exact's
    reference holds there), with the LAUUM masks and with one tensor as both operands."""
    T = gr.TILES[tile][0]
    with _forced_tile(gpu_ctx, tile):
        for n in (1, T + 1, 3 * T + 1):
            for K in (7, 3 * T + 5):
                A, B, C0 = _exact(n, n, K)
                ops = _Operands(variant, A, B)
                for alpha, beta in SCALARS:
                    _check_exact(gpu_ctx, ops, tile, C0, 0, 0, [], 1, alpha, beta, _exact_ref(n, n, K, 0, 0, 1, alpha, beta),
                                 f"{variant} {n}x{n}x{K}")
                    _check_exact(gpu_ctx, ops, tile, C0, 2, 2, [(3, 0)], 1, alpha, beta, _exact_ref(n, n, K, 2, 2, 1, alpha, beta),
                                 f"{variant} {n}x{n}x{K}")
                _check_exact(gpu_ctx, ops, tile, C0, 0, 0, [], 2, -1.0, 1.0, _exact_ref(n, n, K, 0, 0, 2, -1.0, 1.0),
                             f"{variant} {n}x{n}x{K}")
                if variant == "NN":
                    continue  # (one tensor as A [m][k] and B [k][n] would need M = K = N)
                # X X^T (NT) / X^T X (TN) with ONE tensor as A and B: the SYRK update of the upper triangle, and LAUUM's product
                X = A if variant == "NT" else A.T  # as stored
                A2, B2 = (X, X.T) if variant == "NT" else (X.T, X)
                twin = _Operands(variant, A2, B2, same=True)
                for am, bm, hints, c_tri, alpha, beta in [(0, 0, [], 2, -1.0, 1.0), (2, 2, [(3, 0)], 1, 1.0, 0.0)]:
                    ref = gr.masked_product(A2, B2, am, bm, c_tri, alpha, beta, C0)
                    _check_exact(gpu_ctx, twin, tile, C0, am, bm, hints, c_tri, alpha, beta, ref, f"{variant} one tensor {n}x{n}x{K}")


@pytest.mark.parametrize("tile,variant", TILE_VARIANTS)
def test_empty_k_ranges(gpu_ctx, tile, variant):
    """a_mask 1 with b_mask 2 (only n <= k <= m survives): with khi_mode 1 and klo_mode 2 together every tile wholly above the
    diagonal runs over an EMPTY range, and must hold exactly beta*C0 — as it must when only one of the hints, or none, is given."""
    tm, tn = gr.TILES[tile]
    n = 3 * tm + 1
    A, B, C0 = _exact(n, n, n)
    ops = _Operands(variant, A, B)
    empty = gr.empty_range_tiles(2, 1, n, n, n, tm, tn)
    assert empty.any()
    with _forced_tile(gpu_ctx, tile):
        for alpha, beta in SCALARS:
            ref = _exact_ref(n, n, n, 1, 2, 0, alpha, beta)
            np.testing.assert_array_equal(ref[empty], (beta * C0.astype(np.float64))[empty])
            base = _check_exact(gpu_ctx, ops, tile, C0, 1, 2, [(0, 1), (2, 0), (2, 1)], 0, alpha, beta, ref, f"{variant} {n}x{n}x{n}")
            np.testing.assert_array_equal(base[empty], (beta * C0.astype(np.float64))[empty])


def _real_case(M, N, K, am, bm, c_tri, alpha, beta):
    def make():
        A, B, C0 = gr.real_inputs(M, N, K, seed=7000 + 1000 * M + 10 * N + K)
        return A, B, C0, gr.masked_product(A, B, am, bm, c_tri, alpha, beta, C0), gr.error_bound(A, B, am, bm, alpha, beta, C0)

    return _cached(("real", M, N, K, am, bm, c_tri, alpha, beta), make)


@pytest.mark.parametrize("tile,variant", TILE_VARIANTS)
def test_real_inputs_within_derived_bound(gpu_ctx, tile, variant):
    """Standard normals against np.longdouble: |got - ref| <= (K + 4) 2^-53 (|alpha| |Am| @ |Bm| + |beta| |C0|), elementwise — the
    dot-product bound of any accumulation order plus the roundings of alpha and beta; derived, no margin on top."""
    if not np.finfo(np.longdouble).eps < 2e-19:
        pytest.skip("np.longdouble is no wider than float64 here: no higher-precision reference")
    tm, tn = gr.TILES[tile]
    square = tm == tn
    alpha, beta = 0.7, -1.3
    with _forced_tile(gpu_ctx, tile):
        for M, N, K in [(2 * tm + 1, tn + 2, 65), (3 * tm + 1, 2 * tn + 3, 3 * tm + 5)]:
            # the plain product, and LAUUM's: both masks 2 with klo_mode 3, lower output of a square product (full output of the
            # rectangular one on the tall tile, which has no triangular enumeration)
            for am, bm, klo, c_tri, Nc in [(0, 0, 0, 0, N), (2, 2, 3, 1 if square else 0, M if square else N)]:
                A, B, C0, ref, bound = _real_case(M, Nc, K, am, bm, c_tri, alpha, beta)
                got = _Operands(variant, A, B).run(gpu_ctx, C0, alpha, beta, a_mask=am, b_mask=bm, klo_mode=klo, c_tri=c_tri)
                assert not np.isnan(got).any()
                sel = gr.selected(c_tri, M, Nc)
                err = np.abs(got.astype(np.longdouble) - ref)
                ratio = float((err[sel] / np.maximum(bound[sel], np.finfo(np.float64).tiny)).max())
                print(f"tile {tm}x{tn} {variant} {M}x{Nc}x{K} masks ({am}, {bm}): max |got - ref| / bound = {ratio:.3f}")
                assert (err[sel] <= bound[sel]).all(), (variant, M, Nc, K, am, bm, ratio)
                assert gr.same_bits(got[~sel], C0[~sel])


def _flat(stored, gap, fill):
    """The buffers of the batch elements one after the other, ``gap`` doubles of fill between them: (flat array, element stride)."""
    stride = stored[0].buf.size + gap
    flat = np.full(len(stored) * stride, fill, dtype=np.float64)
    for b, s in enumerate(stored):
        assert s.buf.shape == stored[0].buf.shape
        flat[b * stride: b * stride + s.buf.size] = s.buf.ravel()
    return flat, stride


def _first_window(stored, dflat):
    s = stored[0]
    return s.window(dflat[: s.buf.size].view(*s.buf.shape))


@pytest.mark.parametrize("tile,variant", TILE_VARIANTS)
def test_batched(gpu_ctx, tile, variant):
    """gpp_gemm_batched, batch 3, A shared (sA = 0) or per element, B and C0 per element, even strides with a gap between the
    elements: every element equals its reference, and nothing between or around the windows changes."""
    tm, tn = gr.TILES[tile]
    M, N, K = tm + 1, tn + 2, 65
    batch, gap = 3, 6
    tA, tB = gr.VARIANTS[variant]
    elems = [gr.exact_inputs(M, N, K, seed=77 + b) for b in range(batch)]  # (A, B, C0) of each element
    with _forced_tile(gpu_ctx, tile):
        for shared_a in (True, False):
            As = [elems[0 if shared_a else b][0] for b in range(batch)]
            sa = [gr.Stored(a.T if tA else a, np.nan) for a in (As[:1] if shared_a else As)]
            sb = [gr.Stored(e[1].T if tB else e[1], np.nan) for e in elems]
            fa, stride_a = _flat(sa, gap, np.nan)
            fb, stride_b = _flat(sb, gap, np.nan)
            dA, dB = torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda()
            for am, bm, klo, khi in [(0, 0, 0, 0), (0, 2, 2, 0)]:
                for alpha, beta in SCALARS:
                    sc = [gr.store_output(_c_init(e[2], beta, 0)) for e in elems]
                    fc, stride_c = _flat(sc, gap, gr.SENTINEL)
                    dC = torch.from_numpy(fc).cuda()
                    assert stride_a % 2 == 0 and stride_b % 2 == 0 and stride_c % 2 == 0
                    gpu_ctx.gemm_batched(tA, tB, M, N, K, alpha, _first_window(sa, dA), 0 if shared_a else stride_a, _first_window(sb, dB),
                                         stride_b, beta, _first_window(sc, dC), stride_c, batch, a_mask=am, b_mask=bm, klo_mode=klo,
                                         khi_mode=khi)
                    out = dC.cpu().numpy()
                    outside = np.ones(fc.size, dtype=bool)
                    for b in range(batch):
                        lo = b * stride_c
                        outside[lo: lo + sc[b].buf.size] = sc[b].guard_mask().ravel()
                        got = sc[b].window(out[lo: lo + sc[b].buf.size].reshape(sc[b].buf.shape))
                        ref = gr.masked_product(As[b], elems[b][1], am, bm, 0, alpha, beta, elems[b][2])
                        _assert_same(got, ref, tile, f"{variant} element {b} shared A {shared_a} masks ({am}, {bm}) alpha {alpha} beta {beta}")
                    assert gr.same_bits(out[outside], fc[outside]), "gpp_gemm_batched wrote outside the windows of C"


def test_zero_extents_write_nothing(gpu_ctx):
    A, B, C0 = _exact(5, 6, 3)
    sc = gr.store_output(C0)
    for tile in (0,) + tuple(sorted(gr.TILES)):
        with _forced_tile(gpu_ctx, tile):
            for variant in gr.VARIANTS:
                tA, tB = gr.VARIANTS[variant]
                ops = _Operands(variant, A, B)
                for M, N in [(0, 6), (5, 0), (0, 0)]:
                    dC = torch.from_numpy(sc.buf).cuda()
                    gpu_ctx.gemm(tA, tB, M, N, 3, 1.0, ops.A, ops.B, 0.0, sc.window(dC))
                    gpu_ctx.gemm_batched(tA, tB, M, N, 3, 1.0, ops.A, 0, ops.B, 0, 0.0, sc.window(dC), 0, 2)
                    assert gr.same_bits(dC.cpu().numpy(), sc.buf)
                dC = torch.from_numpy(sc.buf).cuda()
                gpu_ctx.gemm_batched(tA, tB, 5, 6, 3, 1.0, ops.A, 0, ops.B, 0, 0.0, sc.window(dC), 0, 0)  # an empty batch
                assert gr.same_bits(dC.cpu().numpy(), sc.buf)


def test_bad_arguments_are_refused(gpu_ctx):
    """The documented negative codes, as GppError names them (the number of the offending argument)."""
    from gpplus_amd.backend import OPT_GEMM_TILE, GppError

    n = 6
    A, B, C0 = _exact(n, n, n)
    ops = _Operands("TN", A, B)
    sc = gr.store_output(C0)
    dC = torch.from_numpy(sc.buf).cuda()
    C = sc.window(dC)
    odd = torch.zeros(8, 7, dtype=torch.float64, device="cuda")[:n, :n]  # leading dimension 7
    assert odd.stride(0) % 2 == 1 and odd.data_ptr() % 16 == 0

    def gemm(code, tA=1, tB=0, M=n, N=n, a=ops.A, b=ops.B, c=C, **kw):
        with pytest.raises(GppError, match=rf"gpp_gemm: bad argument #{code}$"):
            gpu_ctx.gemm(tA, tB, M, N, n, 1.0, a, b, 0.0, c, **kw)

    def batched(code, tA=1, tB=0, M=n, N=n, a=ops.A, b=ops.B, c=C, sA=0, sB=0, sC=0, **kw):
        with pytest.raises(GppError, match=rf"gpp_gemm_batched: bad argument #{code}$"):
            gpu_ctx.gemm_batched(tA, tB, M, N, n, 1.0, a, sA, b, sB, 0.0, c, sC, 2, **kw)

    for code_gemm, code_batched, kw in [
            (2, 2, dict(tA=1, tB=1)),                                      # TT is not implemented
            (8, 8, dict(a=odd)), (10, 11, dict(b=odd)), (13, 15, dict(c=odd)),  # odd leading dimensions
            (15, 19, dict(a_mask=3)), (15, 19, dict(b_mask=-1)), (17, 21, dict(klo_mode=4)), (17, 21, dict(khi_mode=3)),
            (19, 23, dict(c_tri=3)),
            (19, 23, dict(N=n - 1, c_tri=1)), (19, 23, dict(M=n - 1, c_tri=2))]:  # a triangle of a rectangle
        gemm(code_gemm, **kw)
        batched(code_batched, **kw)
    for code, kw in [(8, dict(sA=3)), (11, dict(sB=3)), (15, dict(sC=3))]:  # odd element strides
        batched(code, **kw)
    with _forced_tile(gpu_ctx, 4):  # the tall tile has no triangular enumeration
        for c_tri in (1, 2):
            gemm(19, c_tri=c_tri)
            batched(23, c_tri=c_tri)
    for value in (-1, 5):
        with pytest.raises(GppError, match=r"gpp_set_option: bad argument #3$"):
            gpu_ctx.set_option(OPT_GEMM_TILE, value)
    # a refused value leaves the option as it was (0): the triangle the tall tile refuses goes through again
    assert gr.same_bits(dC.cpu().numpy(), sc.buf)  # nothing above was launched
    gpu_ctx.gemm(1, 0, n, n, n, 1.0, ops.A, ops.B, 0.0, C, c_tri=1)
    torch.cuda.synchronize()

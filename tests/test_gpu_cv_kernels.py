"""The two gathered, ragged products of grouped cross-validation (gpp_cv_blocks, gpp_cv_rows; gpp_cv.hip) against numpy in long
double.  The elementwise tolerance is ``gemm_reference.error_bound``: the dot-product bound of n terms in any order, derived, not
measured.  Every case prints observed / bound (pytest -s shows it).  Poisoned buffers (NaN) show what is read and what is written:
the Linv buffer strictly below its diagonal, the padding of G, every output before the call.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_reference import error_bound  # noqa: E402

pytestmark = pytest.mark.gpu


def _sized(N, sizes, seed):
    """Labels of a random assignment of the rows to folds of the given sizes (gathers are non-contiguous)."""
    assert sum(sizes) == N
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(len(sizes)), sizes))


# (name, N, labels, mp): folds of 1, 2, 63 and 65 rows fill N = 131 (below, at and past the 64-row tile with 64 in the second case);
# i mod 3 interleaves three folds of 101 / 100 / 100; 129 / 130 / 42 cross the 128 edge; mp both a multiple of the tile and not
CASES = [
    ("131:1,2,63,65", 131, _sized(131, [1, 2, 63, 65], 1), 128),
    ("131:1,2,63,65/mp66", 131, _sized(131, [1, 2, 63, 65], 1), 66),
    ("131:64,67", 131, _sized(131, [64, 67], 2), 128),
    ("301:mod3", 301, np.arange(301) % 3, 128),
    ("301:129,130,42", 301, _sized(301, [129, 130, 42], 3), 512),
    ("301:129,130,42/mp130", 301, _sized(301, [129, 130, 42], 3), 130),
]
IDS = [c[0] for c in CASES]


def _csr(labels):
    folds = [np.flatnonzero(labels == v) for v in np.unique(labels)]
    return folds, np.concatenate(folds).astype(np.int32), np.r_[0, np.cumsum([len(F) for F in folds])].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _linv(N):
    """An inverse-factor buffer as the library leaves it, for the reference: entries on and above the diagonal (row i from the
    diagonal on = column i of L^-1), zeros below."""
    rng = np.random.default_rng(100 + N)
    M = np.triu(rng.standard_normal((N, N)))
    M.setflags(write=False)
    return M


def _blocks_buffer(nf, mp):
    from gpplus_amd.backend import row_stride
    return torch.full((nf, mp, row_stride(mp)), float("nan"), dtype=torch.float64, device="cuda")[:, :, :mp]


def _run_blocks(gpu_ctx, Li, idx, off, mp):
    out = _blocks_buffer(off.shape[0] - 1, mp)
    gpu_ctx.cv_blocks(Li, torch.from_numpy(idx).cuda(), torch.from_numpy(off).cuda(), out)
    return out.cpu().numpy()


@pytest.mark.parametrize("name,N,labels,mp", CASES, ids=IDS)
def test_cv_blocks(gpu_ctx, name, N, labels, mp):
    from gpplus_amd.backend import square_buffer

    folds, idx, off = _csr(labels)
    Lup = _linv(N)
    Li = square_buffer(N, "cuda")
    Li.copy_(torch.from_numpy(np.where(np.triu(np.ones((N, N), dtype=bool)), Lup, np.nan)))  # nothing below the diagonal is read
    got = _run_blocks(gpu_ctx, Li, idx, off, mp)
    worst = 0.0
    upper = np.triu(np.ones((mp, mp), dtype=bool))
    for f, F in enumerate(folds):
        m = len(F)
        blk = got[f]
        assert np.isfinite(blk[upper]).all(), (name, f)                   # the whole upper triangle is written
        assert np.isnan(blk[~upper]).all(), (name, f)                     # the strict lower triangle never
        want_pad = np.eye(mp)
        pad = upper.copy()
        pad[:m, :m] = False
        assert np.array_equal(blk[pad], want_pad[pad]), (name, f)         # the padding is exactly identity
        A = Lup[F, :]                                                     # masked rows: zeros left of each row's diagonal
        ref = A.astype(np.longdouble) @ A.T.astype(np.longdouble)
        bound = error_bound(A, A.T, 0, 0, 1.0, 0.0, np.zeros((m, m)))
        sel = np.triu(np.ones((m, m), dtype=bool))
        err = np.abs(blk[:m, :m].astype(np.longdouble) - ref)[sel]
        assert (err <= bound[sel]).all(), (name, f, float((err / bound[sel]).max()))
        worst = max(worst, float((err / bound[sel]).max()))
    print(f"cv_blocks {name}: max observed / bound = {worst:.3f}")
    # a second launch agrees bit for bit; a fold alone gives the bits it has in the full call
    again = _run_blocks(gpu_ctx, Li, idx, off, mp)
    assert np.array_equal(got, again, equal_nan=True)
    for f, F in enumerate(folds):
        alone = _run_blocks(gpu_ctx, Li, F.astype(np.int32), np.array([0, len(F)], dtype=np.int32), mp)
        assert np.array_equal(alone[0], got[f], equal_nan=True), (name, f)


@pytest.mark.parametrize("name,N,labels,mp", CASES, ids=IDS)
def test_cv_rows(gpu_ctx, name, N, labels, mp):
    from gpplus_amd.backend import row_stride

    folds, idx, off = _csr(labels)
    nf = len(folds)
    rng = np.random.default_rng(7 + N)
    R = rng.standard_normal((N, N))
    Psq_h = R + R.T
    ldp = row_stride(N) + 16  # ldp > N, and the columns past N hold NaN
    Psq = torch.full((N, ldp), float("nan"), dtype=torch.float64, device="cuda")[:, :N]
    Psq.copy_(torch.from_numpy(Psq_h))
    G_h = np.full((nf, mp, mp), np.nan)  # the padding of G is never read
    for f, F in enumerate(folds):
        G_h[f, :len(F), :len(F)] = rng.standard_normal((len(F), len(F)))
    G = _blocks_buffer(nf, mp)
    G.copy_(torch.from_numpy(G_h))
    lds = row_stride(N)

    def run(Gt, idx_, off_, rows):
        S = torch.full((rows, lds), float("nan"), dtype=torch.float64, device="cuda")
        gpu_ctx.cv_rows(Gt, torch.from_numpy(idx_).cuda(), torch.from_numpy(off_).cuda(), Psq, S[:, :N])
        return S.cpu().numpy()

    got = run(G, idx, off, N)
    assert np.isfinite(got[:, :N]).all(), name      # all N rows are written
    assert np.isnan(got[:, N:]).all(), name         # columns [N, lds) never
    worst = 0.0
    for f, F in enumerate(folds):
        m = len(F)
        A, B = G_h[f, :m, :m], Psq_h[F, :]
        ref = A.astype(np.longdouble) @ B.astype(np.longdouble)
        bound = error_bound(A, B, 0, 0, 1.0, 0.0, np.zeros((m, N)))
        err = np.abs(got[off[f]:off[f + 1], :N].astype(np.longdouble) - ref)
        assert (err <= bound).all(), (name, f, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print(f"cv_rows {name}: max observed / bound = {worst:.3f}")
    assert np.array_equal(got, run(G, idx, off, N), equal_nan=True)
    for f, F in enumerate(folds):
        alone = run(G[f:f + 1], F.astype(np.int32), np.array([0, len(F)], dtype=np.int32), len(F))
        assert np.array_equal(alone, got[off[f]:off[f + 1]], equal_nan=True), (name, f)


def test_bindings_refuse_lists_the_kernels_would_trust(gpu_ctx):
    """The kernels gather rows idx[.] and write rows off[f] + a unchecked: the bindings verify the list against the buffers on the
    host and raise before anything is launched."""
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import row_stride, square_buffer

    N, mp = 40, 32
    Li, Psq = square_buffer(N, "cuda"), square_buffer(N, "cuda")
    Li.zero_(), Psq.zero_()
    dev = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")  # noqa: E731
    idx, off = dev([1, 5, 7, 0, 2]), dev([0, 3, 5])
    blocks = _blocks_buffer(2, mp)
    S = torch.zeros((5, row_stride(N)), dtype=torch.float64, device="cuda")[:, :N]
    gpu_ctx.cv_blocks(Li, idx, off, blocks)
    gpu_ctx.cv_rows(blocks, idx, off, Psq, S)
    for bad_idx, bad_off, what in ((dev([1, 5, 7, 0, 40]), off, "out of range"), (dev([1, 5, 7, 0, -1]), off, "out of range"),
                                   (dev([5, 1, 7, 0, 2]), off, "ascending"), (idx, dev([0, 3, 6]), "offsets"),
                                   (idx, dev([0, 4, 3]), "offsets"), (dev(list(range(34))), dev([0, 33, 34]), "does not fit")):
        with pytest.raises(GppError, match=what):
            gpu_ctx.cv_blocks(Li, bad_idx, bad_off, blocks)
        with pytest.raises(GppError, match=what):
            gpu_ctx.cv_rows(blocks, bad_idx, bad_off, Psq, torch.zeros((34, row_stride(N)), dtype=torch.float64, device="cuda")[:, :N])
    with pytest.raises(GppError, match="rows"):  # S too short for the rows the folds write
        gpu_ctx.cv_rows(blocks, idx, off, Psq, S[:4])
    with pytest.raises(GppError, match="batched matrix"):  # G not square
        gpu_ctx.cv_rows(blocks[:, :, :30], idx, off, Psq, S)
    with pytest.raises(GppError, match="batched matrix"):
        gpu_ctx.cv_blocks(Li, idx, off, blocks[:, :30, :])
    with pytest.raises(GppError, match="blocks for"):  # one block per fold
        gpu_ctx.cv_blocks(Li, idx, off, blocks[:1])

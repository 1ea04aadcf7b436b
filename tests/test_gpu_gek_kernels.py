"""gpp_kernel_dxdx on the GPU against the long-double closed form of tests/gek_reference.py within that file's per-entry bound
(operation count of the two terms plus the propagated multiplier errors), for the three kinds on shapes that cover one pair, several
tiles on either axis, differentiated dims on both sides of the split and a single direction; extents (sentinels in the padding columns
and in a guard band), finiteness and exact zeros, bitwise repeatability, bitwise symmetry with Ua = Ub, and every argument code."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_reference as G  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
SENTINEL = -7.25
GUARD = 64  # doubles in front of and behind the buffer (512 bytes: the window stays 16-byte aligned)

HX_CASES = [(1, 1, 1, 0, 1, 0), (5, 70, 5, 2, 3, 2), (17, 33, 6, 0, 6, 3), (3, 130, 4, 3, 1, 3)]  # Ma, Mb, D, d0, nd, d_split


def _inputs(Ma, Mb, D, d0, nd, kind):
    rng = np.random.default_rng(1000 * Ma + 10 * Mb + D + 7 * kind)
    Ua = rng.uniform(-1.0, 1.0, (Ma, D))
    Ub = rng.uniform(-1.0, 1.0, (Mb, D))
    w = rng.uniform(0.2, 2.0, D) / D
    zero = d0 + 1 if nd >= 2 else None
    if zero is not None:
        w[zero] = 0.0  # a differentiated feature without weight
    copy = None
    if Ma > 1:
        copy = (Ma - 1, min(3, Mb - 1))
        Ua[copy[0]] = Ub[copy[1]]  # the coincident pair
    return Ua, Ub, w, 1.3, zero, copy


def _guarded(rows, cols, dev):
    """A rows x cols window (leading dimension: cols padded to even, plus 2) of a sentinel-filled buffer with a guard band."""
    ld = (cols + 1) // 2 * 2 + 2
    flat = torch.full((2 * GUARD + rows * ld,), SENTINEL, dtype=torch.float64, device=dev)
    return flat, flat[GUARD:GUARD + rows * ld].view(rows, ld), ld


def _dev(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("Ma,Mb,D,d0,nd,d_split", HX_CASES)
def test_kernel_dxdx(gpu_ctx, Ma, Mb, D, d0, nd, d_split, kind):
    """Per-entry bound: ``gek_reference.d2k_bound`` (its module docstring derives it): 4 u of the diagonal term, 8 u of the product
    term, and the multiplier errors dm_f of the staged arithmetic propagated through g_j and |p_j p_l|; for Matern 3/2 the h''
    multiplier's own error, and an exact 0 of it where r = 0."""
    dev = gpu_ctx.device
    Ua, Ub, w, sf2, zero, copy = _inputs(Ma, Mb, D, d0, nd, kind)
    dUa, dUb, dw, ds = _dev(Ua, dev), _dev(Ub, dev), _dev(w, dev), _dev([sf2], dev)
    R_, C_ = Ma * nd, Mb * nd

    def run():
        flat, buf, ld = _guarded(R_, C_, dev)
        gpu_ctx.kernel_dxdx(dUa, dUb, dw, ds, d0, nd, buf[:, :C_], kind=kind, d_split=d_split)
        torch.cuda.synchronize()
        return flat.cpu(), buf.cpu(), ld

    flat, buf, ld = run()
    assert bool((buf[:, C_:] == SENTINEL).all()), "padding columns were written"
    assert bool((flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all()), "guard band was written"
    got = buf[:, :C_].numpy()
    assert np.isfinite(got).all()
    ref, bound = G.d2k_bound(Ua, Ub, w, sf2, kind, d_split, d0, nd)
    err = np.abs(got.astype(LD) - ref)
    worst = float((err / np.maximum(np.abs(ref), 1e-300))[np.abs(ref) > 0].max())
    print(f"kernel_dxdx Ma={Ma} Mb={Mb} D={D} d0={d0} nd={nd} d_split={d_split} kind={kind}: worst relative error {worst:.3e}, "
          f"worst error / bound {float((err / np.maximum(bound, 1e-300))[bound > 0].max()):.3e}")
    assert (err <= bound).all(), float((err - bound).max())
    g4 = got.reshape(Ma, nd, Mb, nd)
    if zero is not None:
        z = zero - d0
        assert (g4[:, z, :, :] == 0.0).all() and (g4[:, :, :, z] == 0.0).all(), "a feature with w_d == 0: exact zeros in its row and column"
    if copy is not None:
        blk = g4[copy[0], :, copy[1], :]
        assert (blk - np.diag(np.diag(blk)) == 0.0).all(), "the coincident pair: exact zeros off the diagonal"
        s = D if kind == 0 else d_split
        for j in range(nd):
            c = 2.0 if d0 + j < s else (6.0 if kind == 1 else 10.0 / 3.0)
            # (two exponentials at EXP_REL_ERR = 4 u each and at most five roundings: 13 u, taken as 16 u)
            assert abs(blk[j, j] - c * w[d0 + j] * sf2) <= 16 * 2.0 ** -53 * c * w[d0 + j] * sf2, "the coincident pair: the prior curvature"
    flat2, _, _ = run()
    assert torch.equal(flat.view(torch.int64), flat2.view(torch.int64)), "two launches differ"


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_kernel_dxdx_is_bitwise_symmetric_on_equal_rows(gpu_ctx, kind):
    dev = gpu_ctx.device
    M, D, d0, nd, d_split = 37, 6, 1, 5, 3
    Ua, _, w, sf2, _, _ = _inputs(M, M, D, d0, nd, kind)
    Ua[5] = Ua[20]  # a coincident pair off the diagonal too
    dU, dw, ds = _dev(Ua, dev), _dev(w, dev), _dev([sf2], dev)
    flat, buf, ld = _guarded(M * nd, M * nd, dev)
    gpu_ctx.kernel_dxdx(dU, dU.clone(), dw, ds, d0, nd, buf[:, :M * nd], kind=kind, d_split=d_split)
    torch.cuda.synchronize()
    H = buf[:, :M * nd].contiguous()
    assert bool(torch.isfinite(H).all())
    assert torch.equal(H.view(torch.int64), H.T.contiguous().view(torch.int64)), "H is not bitwise symmetric"
    ref, bound = G.d2k_bound(Ua, Ua, w, sf2, kind, d_split, d0, nd)
    assert (np.abs(H.cpu().numpy().astype(LD) - ref) <= bound).all()


def test_kernel_dxdx_argument_codes(gpu_ctx):
    from gpplus_amd._lib import GppError

    dev = gpu_ctx.device
    Ma, Mb, D, d0, nd = 3, 9, 4, 1, 3
    Ua = torch.rand(Ma, D, dtype=torch.float64, device=dev)
    Ub = torch.rand(Mb, D, dtype=torch.float64, device=dev)
    w = torch.rand(D, dtype=torch.float64, device=dev)
    sf2 = torch.ones(1, dtype=torch.float64, device=dev)
    flat, buf, ld = _guarded(Ma * nd, Mb * nd, dev)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    gpu_ctx._stream()

    def raw(h_=h, ua=Ua.data_ptr(), ub=Ub.data_ptr(), w_=w.data_ptr(), s_=sf2.data_ptr(), D_=D, kind=1, d_split=1, d0_=d0, nd_=nd,
            ptr=buf.data_ptr(), ld_=ld, Ma_=Ma, Mb_=Mb):
        return lib.gpp_kernel_dxdx(h_, ua, Ma_, ub, Mb_, D_, w_, s_, kind, d_split, d0_, nd_, ptr, ld_)

    assert raw(h_=None) == -1 and raw(ua=None) == -2 and raw(Ma_=0) == -3 and raw(ub=None) == -4 and raw(Mb_=0) == -5
    assert raw(D_=65) == -6 and raw(D_=0) == -6 and raw(w_=None) == -7 and raw(s_=None) == -8
    assert raw(kind=3) == -9 and raw(kind=-1) == -9 and raw(d_split=5) == -10 and raw(d_split=-1) == -10
    assert raw(d0_=-1) == -11 and raw(d0_=4) == -11
    assert raw(nd_=0) == -12 and raw(d0_=2, nd_=3) == -12
    assert raw(ptr=buf.data_ptr() + 8) == -13 and raw(ptr=None) == -13
    assert raw(ld_=ld + 1) == -14 and raw(ld_=Mb * nd - 1) == -14
    torch.cuda.synchronize()
    assert bool((flat == SENTINEL).all()), "a refused call wrote something"
    assert raw() == 0
    torch.cuda.synchronize()
    assert bool((buf[:, :Mb * nd] != SENTINEL).all()) and bool((buf[:, Mb * nd:] == SENTINEL).all())
    # the binding refuses the same things in words
    with pytest.raises(GppError, match="leading dimension"):
        gpu_ctx.kernel_dxdx(Ua, Ub, w, sf2, d0, nd, torch.zeros((Ma * nd, Mb * nd + 2), dtype=torch.float64, device=dev)[:, :Mb * nd])
    with pytest.raises(GppError, match="differentiated columns"):
        gpu_ctx.kernel_dxdx(Ua, Ub, w, sf2, 2, 3, buf[:, :Mb * nd])
    with pytest.raises(GppError, match="must be"):
        gpu_ctx.kernel_dxdx(Ua, Ub, w, sf2, d0, nd, buf[:, :Mb * nd - 1])

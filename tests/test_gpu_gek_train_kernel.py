"""gpp_gek_grad_reduce on the GPU against the block-level autograd reference of tests/gek_train_reference.py (``block_sums``) with
random symmetric weights: all three kinds on shapes that cover one pair, exact tiles, partial tiles, several tiles per side, more
directions than one pass of the kernel's column loop takes (nd = 12 > 8) and feature gradients; gradient points that are copies of
function rows and of each other; a NaN-filled upper triangle of Kinv (never read); bitwise repeatability, exact accumulation into
pre-filled outputs, argument codes.

The bar is 1e-6 of the largest reference magnitude per output, the project's bar for these kernels (tests/test_gpu_gek.py).  The
host floor — the same reference with its points in another order, i.e. another summation order — is printed beside every error:
it sits near 1e-15, nine orders below the bar."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_train_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-6
#: N, Mg, D, d0, nd, dU, coincident points
SHAPES = [(1, 1, 1, 0, 1, 0, False), (16, 16, 3, 2, 1, 0, False), (37, 19, 5, 2, 3, 2, True), (130, 33, 9, 1, 8, 1, True),
          (40, 17, 20, 8, 12, 4, False)]
_refs = {}


def _d_split(d0, nd):
    """The Matern factor starts inside the differentiated range where that has three or more features (both factors then carry
    directions and the mixed terms are exercised), at its first feature otherwise (the layout GP_Plus produces)."""
    return d0 + (1 if nd >= 3 else 0)


def _inputs(N, Mg, D, d0, nd, dU, coincide, kind):
    rng = np.random.default_rng(100 * N + 10 * Mg + D + 7 * kind)
    U, Ug = rng.uniform(-1.0, 1.0, (N, D)), rng.uniform(-1.0, 1.0, (Mg, D))
    if coincide:
        Ug[0] = U[3]
        Ug[1] = U[3]           # a copy of a function row and of another gradient point
        Ug[Mg - 1] = Ug[5]
        Ug[7] = U[N - 1]
    w = rng.uniform(0.2, 2.0, D) / D
    n = N + Mg * nd
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    Kinv = A + A.T
    alpha = rng.standard_normal(n)
    return tuple(torch.tensor(np.ascontiguousarray(a)) for a in (U, Ug, w, Kinv, alpha)) + (1.3,)


def _reference(shape, kind):
    """(inputs, reference sums, floor): computed once per (shape, kind) and left unchanged."""
    key = (shape, kind)
    if key not in _refs:
        N, Mg, D, d0, nd, dU, coincide = shape
        U, Ug, w, Kinv, alpha, sf2 = inp = _inputs(*shape, kind)
        W = 0.5 * (torch.outer(alpha, alpha) - Kinv)
        ds = _d_split(d0, nd)
        ref = T.block_sums(U, Ug, w, sf2, kind, ds, d0, nd, W, dU)
        # the floor: the same sums with the points of both sets reversed (W permuted to match)
        pi, pa = torch.arange(N - 1, -1, -1), torch.arange(Mg - 1, -1, -1)
        perm = torch.cat([pi, N + (pa[:, None] * nd + torch.arange(nd)[None, :]).reshape(-1)])
        alt = T.block_sums(U[pi], Ug[pa], w, sf2, kind, ds, d0, nd, W[perm][:, perm], dU)
        floor = max(((alt[0] - ref[0]).abs().max() / ref[0].abs().max()).item(), (abs(alt[1] - ref[1]) / abs(ref[1])).item())
        if dU:
            floor = max(floor, ((alt[2][pi] - ref[2]).abs().max() / ref[2].abs().max()).item(),
                        ((alt[3][pa] - ref[3]).abs().max() / ref[3].abs().max()).item())
        _refs[key] = (inp, ref, floor)
    return _refs[key]


def _run(ctx, shape, kind, inp, prefill=None):
    from gpplus_amd.backend import square_buffer

    N, Mg, D, d0, nd, dU, _ = shape
    U, Ug, w, Kinv, alpha, sf2 = inp
    dev = ctx.device
    n = N + Mg * nd
    buf = square_buffer(n, dev)
    buf.copy_(Kinv.to(dev))
    buf += torch.full((n, n), float("nan"), dtype=torch.float64, device=dev).triu(1)  # only the lower triangle may be read
    c = lambda t: t.to(dev).contiguous()  # noqa: E731
    if prefill is None:
        g_w, g_s = torch.zeros(D, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        g_U = torch.zeros(N, dU, dtype=torch.float64, device=dev) if dU else None
    else:
        g_w, g_s = c(prefill[0]).clone(), c(prefill[1]).clone()
        g_U = c(prefill[2]).clone() if dU else None
    g_Ug = torch.full((Mg, dU), float("nan"), dtype=torch.float64, device=dev) if dU else None  # written, not added to
    ctx.gek_grad_reduce(c(U), c(Ug), c(w), torch.tensor([sf2], dtype=torch.float64, device=dev), d0, nd, c(alpha), buf, dU, g_w, g_s,
                        g_U, g_Ug, kind=kind, d_split=_d_split(d0, nd))
    torch.cuda.synchronize()
    return g_w.cpu(), g_s.cpu(), (g_U.cpu() if dU else None), (g_Ug.cpu() if dU else None)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-Mg%d-D%d-d0%d-nd%d-dU%d" % s[:6])
def test_against_the_block_reference(gpu_ctx, shape, kind):
    N, Mg, D, d0, nd, dU, coincide = shape
    inp, ref, floor = _reference(shape, kind)
    got = _run(gpu_ctx, shape, kind, inp)
    names = ("g_w", "g_sf2", "g_U", "g_Ug")
    for name, g, r in zip(names, got, (ref[0], ref[1].reshape(1), ref[2], ref[3])):
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), name
        scale = r.abs().max().item()
        err = (g - r).abs().max().item()
        print(f"{shape[:6]} kind={kind} {name}: max error {err:.3e} = {err / scale:.3e} of max|reference| {scale:.3e}; host floor {floor:.1e}")
        assert err <= BAR * scale, (name, err, scale)
    assert floor <= 1e-2 * BAR, floor  # the reference's own summation-order noise stays two orders below the bar
    # two calls give the same bits
    again = _run(gpu_ctx, shape, kind, inp)
    for g, h in zip(got, again):
        assert g is None or torch.equal(g.view(torch.int64), h.view(torch.int64))
    # accumulation: pre-filled g_w / g_sf2 / g_U receive exactly the sums of the zero-filled call
    rng = np.random.default_rng(3)
    pre = (torch.tensor(rng.standard_normal(D)), torch.tensor(rng.standard_normal(1)), torch.tensor(rng.standard_normal((N, dU))))
    acc = _run(gpu_ctx, shape, kind, inp, prefill=pre)
    assert torch.equal(acc[0], pre[0] + got[0]) and torch.equal(acc[1], pre[1] + got[1])
    if dU:
        assert torch.equal(acc[2], pre[2] + got[2]) and torch.equal(acc[3].view(torch.int64), got[3].view(torch.int64))


def test_argument_codes(gpu_ctx):
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import OP_GEK_GRAD, square_buffer

    N, Mg, D, d0, nd = 6, 3, 5, 2, 3
    n = N + Mg * nd
    dev = gpu_ctx.device
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)  # noqa: E731
    U, Ug, w, sf2, alpha = z(N, D), z(Mg, D), torch.ones(D, dtype=torch.float64, device=dev), torch.ones(1, dtype=torch.float64, device=dev), z(n)
    Kinv = square_buffer(n + 2, dev)
    Kinv.zero_()
    g_w, g_s, g_U, g_Ug = z(D), z(1), z(N, 2), z(Mg, 2)
    gpu_ctx.ensure_workspace(OP_GEK_GRAD, N, Mg, D, 2)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(kind=0, d_split=2, dU=2, ptr=None, ld=None):
        return lib.gpp_gek_grad_reduce(h, P(U), N, P(Ug), Mg, D, P(w), P(sf2), kind, d_split, d0, nd, P(alpha),
                                       ctypes.c_void_p(Kinv.data_ptr() if ptr is None else ptr), Kinv.stride(0) if ld is None else ld,
                                       dU, P(g_w), P(g_s), P(g_U), P(g_Ug))

    assert call() == 0
    assert call(dU=3) == -16                      # a feature with a gradient among the differentiated ones
    assert call(kind=1, d_split=1, dU=2) == -16   # outside the RBF factor on a Matern kind
    assert call(kind=2, d_split=2, dU=2) == 0
    assert Kinv.stride(0) % 2 == 0 and n == 15
    assert call(ld=Kinv.stride(0) + 1) == -15     # an odd leading dimension
    assert call(ld=n - 1) == -15                  # even, but shorter than n
    assert call(ptr=Kinv.data_ptr() + 8) == -14   # not 16-byte aligned
    torch.cuda.synchronize()
    for bad in (dict(dU=3, g_U=z(N, 3), g_Ug=z(Mg, 3)), dict(kind=1, d_split=1)):
        kw = dict(kind=0, d_split=2, dU=2, g_U=g_U, g_Ug=g_Ug)
        kw.update(bad)
        with pytest.raises(GppError):
            gpu_ctx.gek_grad_reduce(U, Ug, w, sf2, d0, nd, alpha, Kinv[:n, :n], kw["dU"], g_w, g_s, kw["g_U"], kw["g_Ug"],
                                    kind=kw["kind"], d_split=kw["d_split"])
    with pytest.raises(GppError):
        gpu_ctx.gek_grad_reduce(U, Ug, w, sf2, d0, nd, alpha[:-1], Kinv[:n, :n], 0, g_w, g_s)
    with pytest.raises(GppError):
        gpu_ctx.gek_grad_reduce(U, Ug, w, sf2, d0, nd, alpha, Kinv[:n - 1, :n - 1], 0, g_w, g_s)

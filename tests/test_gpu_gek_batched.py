"""The batched gradient-enhanced objective on the GPU: the three batched entry points (gpp_cross_kernel_dx_batched,
gpp_kernel_dxdx_batched, gpp_gek_grad_reduce_batched) against their single-problem twins bit for bit and against the closed-form /
autograd block reference of tests/gek_train_reference.py; ``batched.batched_gek_mll`` through ``optim.BatchedObjective`` against the
fp64 autograd reference (tests/gek_train_reference.py, tests/gek_partial_reference.py for masks) and against the eager
``linalg.exact_gek_mll`` element by element; repeatability; one element that is not positive definite; the drivers
(``fit_model_torch_batched`` against ``fit_model_torch``, ``GP_Plus.fit``) and the refusals.

Bars: 1e-6 of the largest reference magnitude for the kernels (tests/test_gpu_gek_train_kernel.py), value 1e-5 relative and every
gradient tensor 1e-6 of its largest reference magnitude for the objective (tests/test_gpu_gek_train.py), 1e-5 relative for the
recorded losses of a fit (tests/test_gpu_loo_batched.py).  Every comparison prints its figures before it asserts."""
import copy
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_partial_reference as P  # noqa: E402
import gek_reference as G  # noqa: E402
import gek_train_reference as T  # noqa: E402
import pathwise_reference as R  # noqa: E402
from oracle.gp_oracle import NotPSDError, psd_safe_cholesky  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 5
BAR = 1e-6                          # the kernels against the block reference
VALUE_BAR, GRAD_BAR = 1e-5, 1e-6    # the objective against the autograd reference and against the eager objective
RTOL = 1e-5                         # recorded losses of the batched fit against the sequential one
DT = torch.float64

#: N, Mg, D, d0, nd, kind, d_split, dU, selection, shared U
SHAPES = [
    (30, 3, 4, 1, 3, R.KIND_RBF, 0, 1, None, False),            # partial 16-point tiles on both sides
    (77, 5, 6, 2, 4, R.KIND_MATERN52, 2, 2, "pattern", False),  # odd N; a feature gradient through the RBF factor
    (130, 17, 5, 0, 5, R.KIND_MATERN32, 1, 0, None, True),      # a second tile of gradient points; both factors; nd > 4
    (64, 2, 12, 2, 10, R.KIND_RBF, 0, 0, "alternating", True),  # nd > 8
]
#: the shape of the test with one bad element: six gradient points, so that five copies of one point leave fifteen dependent rows
BAD_SHAPE = (30, 6, 4, 1, 3, R.KIND_RBF, 0, 1, None, False)
_IDS = ["N%d-Mg%d-D%d-nd%d" % (s[0], s[1], s[2], s[4]) for s in SHAPES]
_inputs_cache = {}


def _bits(t):
    return t.contiguous().view(torch.int64)


def _mask(selection, Mg, nd):
    if selection is None:
        return None
    return P.pattern_mask(Mg, nd) if selection == "pattern" else P.alternating_row(nd).expand(Mg, nd).clone()


def _inputs(shape):
    """The B parameter sets of a shape as CPU tensors, made once and left unchanged: w and sf2 scaled per element as
    ``test_gpu_loo_batched._element`` scales them, the feature rows moved per element unless shared, and for the reduction a
    symmetric ``Kinv`` and a vector ``alpha`` per element that come from no factorisation."""
    if shape not in _inputs_cache:
        N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
        rng = np.random.default_rng(1000 * N + 10 * Mg + D)
        U0, Ug0 = torch.tensor(rng.uniform(-1.0, 1.0, (N, D))), torch.tensor(rng.uniform(-1.0, 1.0, (Mg, D)))
        Ug0[0] = U0[3]  # a gradient point that is a function row
        w0 = torch.tensor(rng.uniform(0.2, 2.0, D) / D)
        mask = _mask(selection, Mg, nd)
        q = Mg * nd if mask is None else int(mask.sum())
        n = N + q
        scale = lambda b: 1.0 + 0.02 * b  # noqa: E731
        U = U0.clone() if shared else torch.stack([U0 * scale(b) for b in range(B)])
        Ug = torch.stack([Ug0 * scale(b) for b in range(B)])
        A = torch.tensor(rng.standard_normal((B, n, n)) / np.sqrt(n))
        _inputs_cache[shape] = dict(U=U, Ug=Ug, w=torch.stack([w0 * (0.6 + 0.2 * b) for b in range(B)]),
                                    sf2=torch.tensor([1.3 * (0.5 + 0.25 * b) for b in range(B)], dtype=DT),
                                    Kinv=A + A.transpose(1, 2), alpha=torch.tensor(rng.standard_normal((B, n))), mask=mask, q=q, n=n)
    return _inputs_cache[shape]


def _element_rows(t, b):
    return t if t.dim() == 2 else t[b]


def _selection(mask, dev):
    from gpplus_amd.backend import GradientSelection

    return None if mask is None else GradientSelection(mask, dev)


def _padded(ctx, t, n):
    """(B, n, n) on the device in a ``batched_buffer``, the upper triangle NaN: only the lower one may be read."""
    buf = ctx.batched_buffer(t.shape[0], n)
    buf.copy_(t.to(ctx.device))
    buf += torch.full((n, n), float("nan"), dtype=DT, device=ctx.device).triu(1)
    return buf


def _even(t):
    """Per-element feature rows with an even batch stride (an odd M D is padded by one double per element), as the objective
    passes them: the batched entry points refuse an odd stride."""
    from gpplus_amd.batched import _even_elements

    out = _even_elements(t)
    assert out.dim() == 2 or out.shape[0] == 1 or out.stride(0) % 2 == 0
    return out


def _vector(ctx, t):
    v = ctx.batched_vector(t.shape[0], t.shape[1])
    v.copy_(t.to(ctx.device))
    return v


def _build_batched(ctx, shape, inp, sel, nb=B, Ug=None):
    """The two block builds for the first ``nb`` elements: straight into the windows A[b, :N, N:n] and A[b, N:n, N:n] of a
    ``batched_buffer`` when N is even; with an odd N those windows start at an odd column, which the builders refuse (16-byte
    stores), and the blocks are built aside as the objective builds them."""
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import row_stride

    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    dev, q, n = ctx.device, inp["q"], inp["n"]
    c = lambda t: t.to(dev).contiguous()  # noqa: E731
    U = _even(c(inp["U"] if shared else inp["U"][:nb]))
    Ug = _even(c(inp["Ug"][:nb])) if Ug is None else Ug
    w, sf2 = c(inp["w"][:nb]), c(inp["sf2"][:nb])
    A = ctx.batched_buffer(nb, n)
    A.fill_(float("nan"))
    fg, gg = A[:, :N, N:n], A[:, N:n, N:n]
    if N % 2:
        with pytest.raises(GppError, match="16-byte"):
            ctx.cross_kernel_dx_batched(Ug, U, w, sf2, d0, nd, fg, kind=kind, d_split=d_split, sel=sel)
        with pytest.raises(GppError, match="16-byte"):
            ctx.kernel_dxdx_batched(Ug, Ug, w, sf2, d0, nd, gg, kind=kind, d_split=d_split, sel_a=sel, sel_b=sel)
        fg = torch.full((nb, N, row_stride(q)), float("nan"), dtype=DT, device=dev)[:, :, :q]
        gg = torch.full((nb, q, row_stride(q)), float("nan"), dtype=DT, device=dev)[:, :, :q]
    ctx.cross_kernel_dx_batched(Ug, U, w, sf2, d0, nd, fg, kind=kind, d_split=d_split, sel=sel)
    ctx.kernel_dxdx_batched(Ug, Ug, w, sf2, d0, nd, gg, kind=kind, d_split=d_split, sel_a=sel, sel_b=sel)
    torch.cuda.synchronize()
    if N % 2 == 0:  # nothing but the two windows was written
        assert bool(torch.isnan(A[:, :N, :N]).all()) and bool(torch.isnan(A[:, N:n, :N]).all())
    return fg.cpu(), gg.cpu()


def _prefill(shape, nb):
    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    rng = np.random.default_rng(3)
    return (torch.tensor(rng.standard_normal((nb, D))), torch.tensor(rng.standard_normal(nb)),
            torch.tensor(rng.standard_normal((nb, N, dU))))


def _reduce_batched(ctx, shape, inp, sel, nb=B, Ug=None):
    """The batched reduction for the first ``nb`` elements on pre-filled g_w / g_sf2 / g_U (it ADDS) and a NaN-filled g_Ug (it WRITES)."""
    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    dev, n = ctx.device, inp["n"]
    c = lambda t: t.to(dev).contiguous()  # noqa: E731
    U = _even(c(inp["U"] if shared else inp["U"][:nb]))
    Ug = _even(c(inp["Ug"][:nb])) if Ug is None else Ug
    pre = _prefill(shape, nb)
    g_w, g_s = c(pre[0]), c(pre[1])
    g_U = c(pre[2]) if dU else None
    g_Ug = torch.full((nb, Mg, dU), float("nan"), dtype=DT, device=dev) if dU else None
    ctx.gek_grad_reduce_batched(U, Ug, c(inp["w"][:nb]), c(inp["sf2"][:nb]), d0, nd, _vector(ctx, inp["alpha"][:nb]),
                                _padded(ctx, inp["Kinv"][:nb], n), dU, g_w, g_s, g_U, g_Ug, kind=kind, d_split=d_split, sel=sel)
    torch.cuda.synchronize()
    return g_w.cpu(), g_s.cpu(), (g_U.cpu() if dU else None), (g_Ug.cpu() if dU else None)


def _single(ctx, shape, inp, sel, b, nb=B):
    """The three single-problem calls on element b's operands: (Kfg, Kgg, (g_w, g_sf2, g_U, g_Ug))."""
    from gpplus_amd.backend import rows_buffer, square_buffer

    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    dev, q, n = ctx.device, inp["q"], inp["n"]
    c = lambda t: t.to(dev).contiguous()  # noqa: E731
    U, Ug, w, sf2 = c(_element_rows(inp["U"], b)), c(inp["Ug"][b]), c(inp["w"][b]), c(inp["sf2"][b:b + 1])
    fg = ctx.cross_kernel_dx(Ug, U, w, sf2, d0, nd, rows_buffer(N, q, dev), kind=kind, d_split=d_split, sel=sel)
    gg = ctx.kernel_dxdx(Ug, Ug, w, sf2, d0, nd, square_buffer(q, dev), kind=kind, d_split=d_split, sel_a=sel, sel_b=sel)
    pre = _prefill(shape, nb)
    g_w, g_s = c(pre[0][b]), c(pre[1][b:b + 1])
    g_U = c(pre[2][b]) if dU else None
    g_Ug = torch.full((Mg, dU), float("nan"), dtype=DT, device=dev) if dU else None
    Kinv = square_buffer(n, dev)
    Kinv.copy_(inp["Kinv"][b].to(dev))
    Kinv += torch.full((n, n), float("nan"), dtype=DT, device=dev).triu(1)
    ctx.gek_grad_reduce(U, Ug, w, sf2, d0, nd, c(inp["alpha"][b]), Kinv, dU, g_w, g_s, g_U, g_Ug, kind=kind, d_split=d_split, sel=sel)
    torch.cuda.synchronize()
    return fg.cpu(), gg.cpu(), (g_w.cpu(), g_s.cpu(), (g_U.cpu() if dU else None), (g_Ug.cpu() if dU else None))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the entry points
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_batched_entry_points_equal_the_single_problem_ones_bitwise(gpu_ctx, shape):
    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    inp = _inputs(shape)
    sel = _selection(inp["mask"], gpu_ctx.device)
    fg, gg = _build_batched(gpu_ctx, shape, inp, sel)
    red = _reduce_batched(gpu_ctx, shape, inp, sel)
    assert bool(torch.isfinite(fg).all()) and bool(torch.isfinite(gg).all())
    for b in range(B):
        fg1, gg1, red1 = _single(gpu_ctx, shape, inp, sel, b)
        assert torch.equal(_bits(fg[b]), _bits(fg1)), ("Kfg", b)
        assert torch.equal(_bits(gg[b]), _bits(gg1)), ("Kgg", b)
        for name, got, one in zip(("g_w", "g_sf2", "g_U", "g_Ug"), red, red1):
            if got is not None:
                assert bool(torch.isfinite(got[b]).all()), (name, b)
                assert torch.equal(_bits(got[b].reshape(-1)), _bits(one.reshape(-1))), (name, b)
    # B = 1: the batched calls on element 0 alone
    fg0, gg0 = _build_batched(gpu_ctx, shape, inp, sel, nb=1)
    fg1, gg1, red1 = _single(gpu_ctx, shape, inp, sel, 0, nb=1)
    red0 = _reduce_batched(gpu_ctx, shape, inp, sel, nb=1)
    assert torch.equal(_bits(fg0[0]), _bits(fg1)) and torch.equal(_bits(gg0[0]), _bits(gg1))
    for got, one in zip(red0, red1):
        assert got is None or torch.equal(_bits(got[0].reshape(-1)), _bits(one.reshape(-1)))


def test_a_shared_block_of_gradient_points_equals_per_element_copies(gpu_ctx):
    shape = SHAPES[2]
    inp = dict(_inputs(shape))
    Ug0 = inp["Ug"][0].to(gpu_ctx.device).contiguous()
    inp["Ug"] = inp["Ug"][0].repeat(B, 1, 1)
    fg_c, gg_c = _build_batched(gpu_ctx, shape, inp, None)
    red_c = _reduce_batched(gpu_ctx, shape, inp, None)
    fg_s, gg_s = _build_batched(gpu_ctx, shape, inp, None, Ug=Ug0)
    red_s = _reduce_batched(gpu_ctx, shape, inp, None, Ug=Ug0)
    assert torch.equal(_bits(fg_c), _bits(fg_s)) and torch.equal(_bits(gg_c), _bits(gg_s))
    for a, s in zip(red_c, red_s):
        assert a is None or torch.equal(_bits(a), _bits(s))


@pytest.mark.parametrize("shape", SHAPES[:2], ids=_IDS[:2])
def test_batched_entry_points_against_the_block_reference(gpu_ctx, shape):
    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    inp = _inputs(shape)
    sel = _selection(inp["mask"], gpu_ctx.device)
    fg, gg = _build_batched(gpu_ctx, shape, inp, sel)
    red = _reduce_batched(gpu_ctx, shape, inp, sel)
    pre = _prefill(shape, B)
    keep = torch.arange(Mg * nd) if inp["mask"] is None else inp["mask"].reshape(-1).nonzero().reshape(-1)
    idx = torch.cat([torch.arange(N), N + keep])
    for b in range(B):
        U, Ug, w, sf2 = _element_rows(inp["U"], b), inp["Ug"][b], inp["w"][b], inp["sf2"][b]
        Kfg, Kgg = T.blocks(U, Ug, w, sf2, kind, d_split, d0, nd)
        for name, got, ref in (("Kfg", fg[b], Kfg[:, keep]), ("Kgg", gg[b], Kgg[keep][:, keep])):
            err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
            print(f"{shape[:5]}[{b}] {name}: max error {err:.3e} = {err / scale:.3e} of max|reference| {scale:.3e}")
            assert err <= BAR * scale, (name, b, err, scale)
        # the weights of the observed rows in the dense layout, zeros elsewhere: the sums then run over the observed entries alone
        Wc = 0.5 * (torch.outer(inp["alpha"][b], inp["alpha"][b]) - inp["Kinv"][b])
        W = torch.zeros(N + Mg * nd, N + Mg * nd, dtype=DT)
        W[idx[:, None], idx[None, :]] = Wc
        ref = T.block_sums(U, Ug, w, sf2, kind, d_split, d0, nd, W, dU)
        got = (red[0][b] - pre[0][b], red[1][b] - pre[1][b], red[2][b] - pre[2][b], red[3][b])
        for name, g, r in zip(("g_w", "g_sf2", "g_U", "g_Ug"), got, (ref[0], ref[1].reshape(()), ref[2], ref[3])):
            err, scale = (g - r).abs().max().item(), r.abs().max().item()
            print(f"{shape[:5]}[{b}] {name}: max error {err:.3e} = {err / scale:.3e} of max|reference| {scale:.3e}")
            assert err <= BAR * scale, (name, b, err, scale)


# ---------------------------------------------------------------------------------------------------------------------------
# batched_gek_mll on plain tensors: repeatability, one bad element, the refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _leaves(shape, nb=B, noise=0.05, tau=0.05):
    """The arguments of ``batched_gek_mll`` for the first ``nb`` parameter sets of a shape, on the GPU, the differentiable ones as
    leaves: tau scaled and the mean shifted per element, y and r_g fixed patterns, a shared noise."""
    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    inp = _inputs(shape)
    q = inp["q"]
    t = dict(U=inp["U"].clone() if shared else inp["U"][:nb].clone(), Ug=inp["Ug"][:nb].clone(), w=inp["w"][:nb].clone(),
             sf2=inp["sf2"][:nb].clone(), tau=torch.tensor([[tau * (1.0 + 0.5 * b)] for b in range(nb)], dtype=DT),
             mean=torch.stack([torch.full((N,), 0.05 * b, dtype=DT) for b in range(nb)]),
             y=torch.sin(1.7 * torch.arange(N, dtype=DT)))
    fixed = dict(r_g=0.3 * torch.cos(0.9 * torch.arange(q, dtype=DT)), noise=torch.full((q,), noise, dtype=DT),
                 grp=torch.zeros(N, dtype=torch.int32))
    return t, fixed


def _call(shape, t, fixed, need_grad=True):
    from gpplus_amd.batched import batched_gek_mll

    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    lv = {k: v.to("cuda").requires_grad_(need_grad) for k, v in t.items()}
    fx = {k: v.to("cuda") for k, v in fixed.items()}
    val = batched_gek_mll(lv["U"], lv["Ug"], lv["w"], lv["sf2"], lv["tau"], lv["mean"], lv["y"], fx["r_g"], fx["noise"], fx["grp"],
                          kind, d_split, d0, nd, dU, sel=_selection(_inputs(shape)["mask"], "cuda"))
    if not need_grad:
        return val.detach().cpu(), None
    torch.nansum(val).backward()
    return val.detach().cpu(), {k: v.grad.detach().cpu() for k, v in lv.items()}


def test_two_calls_agree_bitwise(gpu_ctx):
    """Odd N (the blocks built aside), a selection, a Matern kind and feature gradients."""
    shape = SHAPES[1]
    t, fixed = _leaves(shape)
    v1, g1 = _call(shape, t, fixed)
    v2, g2 = _call(shape, t, fixed)
    assert bool(torch.isfinite(v1).all())
    assert torch.equal(_bits(v1), _bits(v2))
    assert set(g1) == {"U", "Ug", "w", "sf2", "tau", "mean", "y"}
    for k in g1:
        assert bool(torch.isfinite(g1[k]).all()) and float(g1[k].abs().max()) > 0.0, k
        assert torch.equal(_bits(g1[k]), _bits(g2[k])), k


def _joint_matrix(shape, t, fixed, b):
    """Kj of element b on the CPU from the closed-form blocks."""
    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    U, Ug, w, sf2 = _element_rows(t["U"], b), t["Ug"][b], t["w"][b], t["sf2"][b]
    Kff = T._pair_parts(U, U, w, sf2, kind, d_split)[1] + torch.diag(t["tau"][b][fixed["grp"].long()])
    Kfg, Kgg = T.blocks(U, Ug, w, sf2, kind, d_split, d0, nd)
    return torch.cat([torch.cat([Kff, Kfg], 1), torch.cat([Kfg.T, Kgg + torch.diag(fixed["noise"])], 1)], 0)


def test_one_bad_element_returns_nan_and_leaves_the_others_alone(gpu_ctx):
    """Element 2: every gradient point a copy of the first one, an explicit noise of 0 and tau at its lower bound (1e-8, GP_Plus's
    ``lb_noise``), so its joint matrix is exactly singular; its sf2 is 1e14, so the spacing of the doubles on its diagonal (~1e-2)
    exceeds the largest jitter of the schedule (1e-6): the jitter is absorbed and every attempt factors the same singular bits, in
    which the fifteen rows of the five copies have pivots of rounding size.  The CPU reference confirms that this element alone fails
    and that the others need no jitter."""
    shape = BAD_SHAPE
    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    bad = 2
    t, fixed = _leaves(shape, noise=0.0)
    t["Ug"][bad] = t["Ug"][bad][0].clone().expand(Mg, D)
    t["sf2"][bad] = 1e14
    t["tau"][bad] = 1e-8
    for b in range(B):
        S = _joint_matrix(shape, t, fixed, b)
        if b == bad:
            with pytest.raises(NotPSDError), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                psd_safe_cholesky(S)
        else:
            assert psd_safe_cholesky(S)[1] == 0.0, b
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        val, grads = _call(shape, t, fixed)
    print("values with element 2 singular:", val.tolist())
    good = [b for b in range(B) if b != bad]
    assert bool(torch.isnan(val[bad])) and bool(torch.isfinite(val[good]).all())
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()), name
        if name != "y":  # (y is shared: its gradient is the sum over the elements, to which the bad one adds nothing — below)
            assert float(g[bad].abs().max()) == 0.0, name
    # the others: the bits of a call without the bad element
    val4, grads4 = _call(shape, {k: (v if k == "y" else v[good]) for k, v in t.items()}, fixed)
    assert torch.equal(_bits(val[good]), _bits(val4))
    for name in grads:
        if name != "y":
            assert torch.equal(_bits(grads[name][good]), _bits(grads4[name])), name
    # y is shared: its gradient is the sum over the elements, to which the bad one adds an exact zero (another order of addition)
    assert torch.allclose(grads["y"], grads4["y"], rtol=1e-13, atol=1e-13 * float(grads4["y"].abs().max()))


def test_refusals(gpu_ctx, monkeypatch):
    from gpplus_amd._lib import GppError

    shape = SHAPES[0]
    N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
    t, fixed = _leaves(shape)
    with monkeypatch.context() as mp:  # (a capture is not started for this: the check is the host-side query)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(NotImplementedError, match="capture"):
            _call(shape, t, fixed)
    # an odd batch stride is refused by the backend, before the launch: of the feature rows, of the output, of alpha
    inp = _inputs(shape)
    dev, q, n = gpu_ctx.device, inp["q"], inp["n"]
    c = lambda x: x.to(dev).contiguous()  # noqa: E731
    U, Ug, w, sf2 = c(inp["U"]), c(inp["Ug"]), c(inp["w"]), c(inp["sf2"])
    assert (N * D) % 2 == 0 and (Mg * D) % 2 == 0
    U_odd = torch.zeros(B, N * D + 1, dtype=DT, device=dev)[:, :N * D].view(B, N, D)
    U_odd.copy_(U)
    assert U_odd.stride(0) % 2 == 1
    out = gpu_ctx.batched_buffer(B, n)
    out.fill_(7.0)
    fg = out[:, :N, N:n]
    with pytest.raises(GppError, match="odd"):
        gpu_ctx.cross_kernel_dx_batched(Ug, U_odd, w, sf2, d0, nd, fg, kind=kind, d_split=d_split)
    odd_out = torch.full((B, N * 48 + 1), 7.0, dtype=DT, device=dev)[:, :N * 48].view(B, N, 48)[:, :, :q]
    with pytest.raises(GppError, match="odd"):
        gpu_ctx.cross_kernel_dx_batched(Ug, U, w, sf2, d0, nd, odd_out, kind=kind, d_split=d_split)
    g_w, g_s = torch.zeros(B, D, dtype=DT, device=dev), torch.zeros(B, dtype=DT, device=dev)
    alpha_odd = torch.zeros(B, n + 1 - (n & 1), dtype=DT, device=dev)[:, :n] if n % 2 == 0 else torch.zeros(B, n, dtype=DT, device=dev)
    assert alpha_odd.stride(0) % 2 == 1
    Kinv = gpu_ctx.batched_buffer(B, n)
    Kinv.zero_()
    with pytest.raises(GppError, match="odd"):
        gpu_ctx.gek_grad_reduce_batched(U, Ug, w, sf2, d0, nd, alpha_odd, Kinv, 0, g_w, g_s, kind=kind, d_split=d_split)
    # ... and by the library itself, with a code of its own and nothing enqueued
    P_ = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = gpu_ctx.lib.gpp_cross_kernel_dx_batched(gpu_ctx.h, P_(Ug), Mg * D, Mg, P_(U_odd), U_odd.stride(0), N, D, P_(w), P_(sf2), kind,
                                                 d_split, d0, nd, None, None, q, P_(fg), fg.stride(1), fg.stride(0), B)
    assert rc == -30
    rc = gpu_ctx.lib.gpp_kernel_dxdx_batched(gpu_ctx.h, P_(Ug), Mg * D, Mg, P_(Ug), Mg * D, Mg, D, P_(w), P_(sf2), kind, d_split, d0, nd,
                                             None, None, q, None, None, q, P_(out[:, N:n, N:n]), out.stride(1), out.stride(0) + 1, B)
    assert rc == -30
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(odd_out.min()) == 7.0 and float(g_w.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the objective against the reference
# ---------------------------------------------------------------------------------------------------------------------------
_cases = {}
_refs = {}


def _model_from_oracle(o, X, y, **kw):
    from gpplus_amd.models import GP_Plus

    m = GP_Plus(torch.tensor(X), torch.tensor(y), dtype=DT, device="cuda", **kw)
    sd = m.state_dict()
    for k, v in o.params.items():
        sd[k] = v.reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    return m


def _case(name):
    """(model, the B oracles, xg, dY, noise): B parameter sets around the oracle parameters — every trainable tensor moved by
    0.05 (b - 2) times a fixed pattern, which scales w, sf2 and tau per element, shifts the means and, with qualitative columns,
    moves the latent map and with it the features of every element; element 2 is the oracle's own."""
    if name not in _cases:
        o, X, y, kw, xg, dY, noise, _ = G.gek_case(name)
        oracles = []
        for b in range(B):
            ob = copy.deepcopy(o)
            for i, k in enumerate(o.trainable):
                v = o.params[k]
                ob.params[k] = v + 0.05 * (b - 2) * torch.cos(torch.arange(v.numel(), dtype=DT) + i).reshape(v.shape)
            oracles.append(ob)
        _cases[name] = (_model_from_oracle(o, X, y, **kw), oracles, xg, dY, noise)
    return _cases[name]


def _reference(name, noise_given, masked):
    """The CPU reference (loss, gradients) of every element, evaluated once and left unchanged."""
    key = (name, noise_given, masked)
    if key not in _refs:
        from gpplus_amd.gradient_enhanced import GRADIENT_NUGGET_REL

        m, oracles, xg, dY, noise = _case(name)
        nz, rel = (noise, None) if noise_given else (None, GRADIENT_NUGGET_REL)
        if masked:
            mask = P.pattern_mask(xg.shape[0], dY.shape[1])
            _refs[key] = [P.gek_loss_and_grad_partial(ob, xg, dY, nz, mask, rel) for ob in oracles]
        else:
            _refs[key] = [T.gek_loss_and_grad(ob, xg, dY, nz, rel) for ob in oracles]
    return _refs[key]


def _compare(what, loss, grads, ref_loss, ref_grads, names):
    bad = []
    rel = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    print(f"{what}: loss {loss.item():.12e} against {ref_loss.item():.12e}: rel {rel:.2e}")
    if not rel <= VALUE_BAR:
        bad.append((what, "loss", rel))
    for n in names:
        ref = ref_grads[n].reshape(grads[n].shape)
        scale = ref.abs().max().item()
        err = (grads[n] - ref).abs().max().item()
        print(f"{what} {n}: max error {err:.3e} = {err / scale:.3e} of max|reference| {scale:.3e}")
        if not err <= GRAD_BAR * scale:
            bad.append((what, n, err, scale))
    return bad


def _eager(m, params, xg, dY, nz, mask):
    """The eager objective (linalg.exact_gek_mll through GradientEnhancedMarginalLogLikelihood) at one parameter set."""
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood

    sd = m.state_dict()
    for k, v in params.items():
        sd[k] = v.reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    m.train()
    m.zero_grad()
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, nz, mask)
    loss = -mll(m(*m.train_inputs), m.train_targets)
    loss.backward()
    return loss.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name,noise_given,masked", [("c3", True, False), ("c3", False, False), ("c3", True, True), ("c3", False, True),
                                                     ("c4", True, False), ("c4", False, False),
                                                     ("c1-matern52", True, False), ("c1-matern52", False, False)])
def test_the_objective_against_the_reference_and_the_eager_objective(gpu_ctx, name, noise_given, masked):
    from gpplus_amd.optim import BatchedObjective

    m, oracles, xg, dY, noise = _case(name)
    refs = _reference(name, noise_given, masked)
    nz = noise if noise_given else None
    mask = P.pattern_mask(xg.shape[0], dY.shape[1]) if masked else None
    obj = BatchedObjective(m, B, "gek", gradients=(xg, dY, nz) if mask is None else (xg, dY, nz, mask))
    trainable = list(oracles[0].trainable)
    assert set(obj.names) == set(trainable)
    for b, ob in enumerate(oracles):
        obj.set_row(b, {n: ob.params[n].reshape(obj.theta[n][b].shape) for n in obj.names})
    loss = obj.loss()
    loss.sum().backward()
    assert loss.shape == (B,) and bool(torch.isfinite(loss).all())
    lossc = loss.detach().cpu()
    bad = []
    what = f"{name} noise_given={noise_given} masked={masked}"
    try:
        for b, ob in enumerate(oracles):
            grads = {n: obj.theta[n].grad[b].detach().cpu() for n in obj.names}
            bad += _compare(f"{what} [{b}] reference", lossc[b], grads, *refs[b], trainable)
            e_loss, e_grads = _eager(m, ob.params, xg, dY, nz, mask)
            assert set(e_grads) == set(trainable)
            bad += _compare(f"{what} [{b}] eager", lossc[b], grads, e_loss, e_grads, trainable)
    finally:  # the model is shared by the cases of this test: back to the oracle's own parameters
        sd = m.state_dict()
        for k, v in oracles[2].params.items():
            sd[k] = v.reshape(sd[k].shape).to(sd[k])
        m.load_state_dict(sd)
    assert not bad, bad


def test_the_cases_cover_feature_gradients_and_noise_groups():
    m, oracles, xg, dY, noise = _case("c3")
    assert oracles[0].dz > 0  # qualitative columns: U and Ug differ per element and carry gradients
    assert G.GEK_CASES["c4"][2].get("multiple_noise") and G.GEK_CASES["c4"][2].get("m_gp") == "multiple_constant"
    assert G.GEK_CASES["c1-matern52"][2].get("quant_correlation_class") == "Matern52Kernel"


# ---------------------------------------------------------------------------------------------------------------------------
# 5. / 6. the drivers
# ---------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Counts the calls of the eager and of the batched objective while both stay what they are."""

    def __init__(self, monkeypatch):
        import gpplus_amd.linalg as LA
        import gpplus_amd.optim.mll_batched as MB

        self.eager = self.batched = 0
        eager, batched = LA.exact_gek_mll, MB.batched_gek_mll

        def eager_spy(*a, **k):
            self.eager += 1
            return eager(*a, **k)

        def batched_spy(*a, **k):
            self.batched += 1
            return batched(*a, **k)

        monkeypatch.setattr(LA, "exact_gek_mll", eager_spy)
        monkeypatch.setattr(MB, "batched_gek_mll", batched_spy)


def test_fit_model_torch_batched_gek_follows_the_sequential_driver(gpu_ctx, monkeypatch):
    from gpplus_amd.optim import fit_model_torch, fit_model_torch_batched
    from gpplus_amd.utils import set_seed

    o, X, y, xg, dY, _ = T.fit_case()
    noise = G.prior_curvature_noise(o, 1e-4)
    ma, mb = _model_from_oracle(o, X, y), _model_from_oracle(o, X, y)
    spy = _Spy(monkeypatch)
    fit_model_torch_batched.last_graph = "untouched"
    set_seed(9)
    fb, hb = fit_model_torch_batched(mb, num_restarts=3, num_iter=30, objective="gek", gradients=(xg, dY, noise))
    assert spy.eager == 0 and spy.batched == 30
    assert fit_model_torch_batched.last_graph is None  # the step is not captured
    set_seed(9)
    fa, ha = fit_model_torch(ma, num_restarts=3, num_iter=30, verbose=False, objective="gek", gradients=(xg, dY, noise))
    assert spy.eager > 0 and spy.batched == 30
    assert len(ha) == len(hb) == 4 and [len(h) for h in ha] == [len(h) for h in hb]
    dev = max(abs(x - y_) / abs(x) for a, b in zip(ha, hb) for x, y_ in zip(a, b))
    wa, wb = int(np.argmin([h[-1] for h in ha])), int(np.argmin([h[-1] for h in hb]))
    print(f"batched against sequential gek fit: largest relative deviation of a loss {dev:.2e}; winners {wa} / {wb}; "
          f"final loss {fa:.12f} / {fb:.12f} (rel {abs(fa - fb) / abs(fa):.2e})")
    assert dev <= RTOL
    assert wa == wb and abs(fa - fb) <= RTOL * abs(fa)


def test_gp_plus_fit_with_the_gek_objective_takes_the_batched_route(gpu_ctx, monkeypatch):
    from gpplus_amd import settings
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.utils import set_seed

    fx = dict(np.load(os.path.join(GOLD, "c3_borehole_mixed_n100.npz")))
    _, _, xg, dY, noise = _case("c3")

    def model():
        set_seed(2)
        return GP_Plus(torch.tensor(fx["Xtrain" if "Xtrain" in fx else "Utrain"]), torch.tensor(fx["ytrain"]), qual_dict={0: 5, 5: 5}, dtype=DT, device="cuda")

    spy = _Spy(monkeypatch)
    m = model()
    best, histories = m.fit(optim_type="adam_torch", objective="gek", gradients=(xg, dY, noise))
    lens = [len(h) for h in histories]
    print(f"GP_Plus.fit(objective='gek'): {len(histories)} runs of {min(lens)}..{max(lens)} losses; start {histories[0][0]:.6f}, "
          f"best {best:.6f}; {spy.batched} batched and {spy.eager} eager evaluations")
    assert len(histories) == 65 and all(0 < n <= 100 for n in lens)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert np.isfinite(best) and best < histories[0][0]
    assert spy.eager == 0 and spy.batched == max(lens)  # the batched route: one batched evaluation per Adam step

    # the sequential route (any other optim_type: a warning and 4 restarts, as for the other objectives)
    m = model()
    calls = spy.batched
    with settings.batched_restarts(False), pytest.warns(UserWarning, match="adam_torch"):
        best_s, hist_s = m.fit(objective="gek", gradients=(xg, dY, noise))
    print(f"sequential: {len(hist_s)} runs, best {best_s:.6f}; {spy.eager} eager evaluations")
    assert len(hist_s) == 5 and np.isfinite(best_s)
    assert spy.batched == calls and spy.eager == sum(len(h) for h in hist_s)

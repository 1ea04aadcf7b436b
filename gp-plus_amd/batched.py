"""Batched evaluation: B independent exact-GP log-likelihoods of the SAME data size in every kernel launch.

The reference fits a model by running its restarts one after the other (optim/mll_torch.py:99-141: ``num_restarts + 1``
Adam runs of 100 evaluations each; optim/mll_scipy.py:281-295 farms L-BFGS starts out to joblib workers).  For the sizes
its examples use (N = 100 ... 500) one evaluation is a chain of a few dozen latency-bound launches that leave the GPU
almost empty, so the MI355X-native form of "restart parallelism" is to evaluate ALL restarts in the same launches: every
kernel of ``csrc/`` takes a batch dimension (``gpp_*_batched``), and 64 restarts cost the latency chain of one.

``BatchedMLLFunction`` is ``linalg.ExactMLLFunction`` with a leading batch dimension on every argument:
    U (N, D) shared or (B, N, D);  w (B, D);  sf2 (B,);  tau (B, S);  mean (B, N);  y (N,) or (B, N)  ->  mll (B,)
``BatchedLOOFunction`` is ``linalg.ExactLOOFunction`` (the leave-one-out pseudo-likelihood) in the same form; the two share the
forward's scaffold and the backward, as the eager pair shares ``linalg._exact_forward`` / ``_eval_backward``.
``BatchedGEKFunction`` is ``linalg.ExactGEKFunction`` (the joint density of function values and gradient observations) in the same
form; its matrix has three blocks and its jitter goes on the gradient rows as well, so it hands ``_factor_batched`` a build of its
own and shares the attempt, the jitter policy (``psd_safe.psd_safe_batched``) and the backward with the other two.
Elements whose covariance is not positive definite after the jitter schedule (gpytorch's 1e-8 * 10^i) return NaN and
zero gradients instead of raising: one bad restart must not stop the others (the drivers score it +inf).
"""
from __future__ import annotations

import threading
from typing import Dict, Optional, Tuple

import torch

from .backend import KIND_RBF, UPLO_UPPER, GppContext, get_context, row_stride
from .linalg import _as_f64, _grad_buffers
from .psd_safe import psd_safe_batched

__all__ = ["BatchedWorkspace", "BatchedMLLFunction", "batched_mll", "BatchedLOOFunction", "batched_loo", "BatchedGEKFunction",
           "batched_gek_mll"]


class BatchedWorkspace:
    def __init__(self, ctx: GppContext, B: int, N: int):
        dev = ctx.device
        self.B, self.N = B, N
        self.A, self.Li, self.Ki = (ctx.batched_buffer(B, N) for _ in range(3))
        self.r, self.z, self.alpha = (ctx.batched_vector(B, N) for _ in range(3))
        self.out3 = torch.empty(B, 3, dtype=torch.float64, device=dev)
        self.info = torch.zeros(B, dtype=torch.int32, device=dev)
        self.info_host = torch.zeros(B, dtype=torch.int32).pin_memory()
        self.info_event = torch.cuda.Event()
        self.epoch = 0
        self._ctx, self._loo = ctx, None

    def loo_vectors(self):
        """The O(B N) vectors of a batched leave-one-out evaluation (BatchedLOOFunction), allocated on first use and kept: d, a,
        sqrt(b), beta, the scratch z / out3 of beta's solve (the evaluation's own z and out3 stay what the value was computed
        from) and the values.  A graph capture finds them allocated by the passes that warm it up."""
        if self._loo is None:
            from types import SimpleNamespace
            vec = lambda: self._ctx.batched_vector(self.B, self.N)  # noqa: E731
            dev = self.A.device
            self._loo = SimpleNamespace(d=vec(), a=vec(), sb=vec(), beta=vec(), z=vec(),
                                        out3=torch.empty(self.B, 3, dtype=torch.float64, device=dev),
                                        val=torch.empty(self.B, dtype=torch.float64, device=dev))
        return self._loo


_workspaces: Dict[Tuple[int, int, int], BatchedWorkspace] = {}
_lock = threading.Lock()


def get_batched_workspace(ctx: GppContext, B: int, N: int) -> BatchedWorkspace:
    key = (ctx.index, B, N)
    ws = _workspaces.get(key)
    if ws is None:
        with _lock:
            for k in [k for k in _workspaces if k[0] == ctx.index]:
                del _workspaces[k]
            ws = BatchedWorkspace(ctx, B, N)
            _workspaces[key] = ws
    return ws


def _factor_batched(gctx: GppContext, ws: BatchedWorkspace, build, after=None) -> torch.Tensor:
    """Build + factor all elements; failing ones are retried with gpytorch's jitter schedule added to THEIR diagonal
    (``psd_safe.psd_safe_batched``).  ``build(extra)`` writes every element's matrix into the upper triangle of ``ws.A`` with the
    (B, 1) jitters ``extra`` on its diagonal, or as it is for ``extra`` None.  Returns the boolean mask (B,) of elements that are
    positive definite in the end.  ``after()`` enqueues the rest of the evaluation before the host waits for the status words (one
    wait per attempt, covering the factorisation only)."""
    if torch.cuda.is_current_stream_capturing():
        # inside a HIP-graph capture (optim/mll_batched.py) nothing may wait for the host: ONE attempt without jitter (and without
        # the launch that would add a zero one); the status words stay on the device and the owner of the graph re-runs the step
        # eagerly when any of them is not zero
        build(None)
        gctx.potrf_batched(ws.A, ws.Li, ws.info)
        if after is not None:
            after()
        return ws.info == 0

    def attempt(extra):
        build(extra)
        gctx.potrf_batched(ws.A, ws.Li, ws.info)
        ok = ws.info == 0
        ws.info_host.copy_(ws.info, non_blocking=True)
        ws.info_event.record()
        if after is not None:
            after()
        ws.info_event.synchronize()
        return ok, ws.info_host

    return psd_safe_batched(ws.B, ws.A.device, attempt)[0]


def _batched_operands(w, sf2, tau, grp):
    """w (B, D), sf2 (B,) and tau (B, S) detached, fp64 and contiguous on w's device, ``grp`` as int32, and S."""
    dev, B = w.device, w.shape[0]
    td = _as_f64(tau.detach().reshape(B, -1), dev)
    if grp is not None and grp.dtype != torch.int32:
        grp = grp.to(torch.int32)
    return _as_f64(w.detach(), dev), _as_f64(sf2.detach().reshape(B), dev), td, grp, td.shape[1]


# ---------------------------------------------------------------------------------------------------
# what the two batched Functions share
# ---------------------------------------------------------------------------------------------------
def _batched_forward(fn, ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU):
    """The forward of the batched objectives.  ``fn`` (BatchedMLLFunction / BatchedLOOFunction) supplies what differs: whether the
    value alone needs alpha, the ``tail`` of the enqueued sequence behind trtri, z and alpha, and its ``result``.  The gradients
    are produced here (when any input needs one), ahead of the host's wait for the factorisation status."""
    dev = w.device
    gctx = get_context(dev)
    B, D = w.shape
    N = U.shape[-2]
    Ud = _as_f64(U.detach(), dev)
    wd, sd, td, grp, S = _batched_operands(w, sf2, tau, grp)
    ws = get_batched_workspace(gctx, B, N)
    ws.epoch += 1
    torch.sub(_as_f64(y.detach(), dev).expand(B, N), _as_f64(mean.detach(), dev).expand(B, N), out=ws.r)
    need = ctx.needs_input_grad
    need_grad = any(need[:6])
    dUk = dU if need[0] and dU > 0 else 0
    g_w, g_s, g_t, g_Ud = _grad_buffers(need_grad, dev, (B,), D, S, (N, dUk))
    ops, grads = (Ud, wd, sd, grp, S), (dUk, g_w, g_s, g_t, g_Ud)

    def build(extra):
        gctx.kernel_build_batched(Ud, wd, sd, td if extra is None else td + extra, grp, ws.A, kind=kind, d_split=d_split,
                                  uplo=UPLO_UPPER)

    def rest():
        gctx.trtri_batched(ws.A, ws.Li, ws.Ki)
        gctx.mll_reduce_batched(ws.A, ws.Li, ws.r, ws.z, ws.out3)
        if need_grad or fn.value_needs_alpha:
            gctx.alpha_batched(ws.Li, ws.z, ws.alpha)
        fn.tail(gctx, ws, need_grad, ops, grads, kind, d_split)

    ok = _factor_batched(gctx, ws, build, after=rest)
    value, g_mean = fn.result(ws, need_grad)
    return _batched_result(ctx, ok, value, (g_w, g_s, g_t, (g_Ud,), g_mean), (U,), w, sf2, tau, mean, y)


def _batched_result(ctx, ok, value, grads, blocks, w, sf2, tau, mean, y):
    """Notes on ``ctx`` what ``_batched_backward`` needs — ``grads`` = (g_w, g_s, g_t, one g_U per block of feature rows in
    ``blocks``, g_mean), the mask, every input's dtype and shape — and returns the values, NaN where ``ok`` is false."""
    ctx.saved = grads + (ok,)
    ctx.in_dtypes = tuple(t.dtype for t in blocks + (w, sf2, tau, mean, y))
    ctx.shapes = (tuple(t.shape for t in blocks), sf2.shape, tau.shape, mean.shape, y.shape)
    return torch.where(ok, value, torch.full_like(value, float("nan")))


def _batched_backward(ctx, grad_out):
    """The gradients of (the leading blocks of feature rows: U, or U and Ug; w, sf2, tau, mean, y) from the fp64 ones the forward
    produced, scaled by ``grad_out`` (zero for an element that is not positive definite), each in its input's dtype and shape; None
    for the arguments behind them.  A block's ``g_U`` (B, M, dU; or None) fills the leading columns of its gradient, summed over the
    batch when the block is shared.  The saved ``g_mean`` is the objective's derivative by the mean (alpha for the MLL and GEK,
    -beta for LOO); y receives its negative."""
    g_w, g_s, g_t, g_rows, gm_all, ok = ctx.saved
    need, dt = ctx.needs_input_grad, ctx.in_dtypes
    row_shapes, sf2_shape, tau_shape, mean_shape, y_shape = ctx.shapes
    k = len(row_shapes)
    (B, D), dev = g_w.shape, g_w.device
    go = torch.where(ok, grad_out.to(torch.float64), torch.zeros_like(grad_out, dtype=torch.float64))  # failed: no gradient
    gm = go.unsqueeze(1) * torch.where(ok.unsqueeze(1), gm_all, torch.zeros_like(gm_all))

    def rows(g_d, shape):
        full = torch.zeros(B, shape[-2], D, dtype=torch.float64, device=dev)
        if g_d is not None:
            full[:, :, :g_d.shape[2]] = torch.where(ok.view(B, 1, 1), g_d, torch.zeros_like(g_d)) * go.view(B, 1, 1)
        return full if len(shape) == 3 else full.sum(0)

    def red(t, shape):  # gradient of a broadcast argument: sum over the batch
        return t.reshape(shape) if len(shape) == t.dim() else t.sum(0).reshape(shape)

    nanfree = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))  # noqa: E731
    return tuple(rows(g_d, shape).to(dt[i]) if need[i] else None for i, (g_d, shape) in enumerate(zip(g_rows, row_shapes))) + (
        nanfree(go.unsqueeze(1) * g_w).to(dt[k]) if need[k] else None,
        nanfree(go * g_s).reshape(sf2_shape).to(dt[k + 1]) if need[k + 1] else None,
        nanfree(go.unsqueeze(1) * g_t).reshape(tau_shape).to(dt[k + 2]) if need[k + 2] else None,
        red(gm, mean_shape).to(dt[k + 3]) if need[k + 3] else None,
        red(-gm, y_shape).to(dt[k + 4]) if need[k + 4] else None) + (None,) * (len(need) - k - 5)


class BatchedMLLFunction(torch.autograd.Function):
    """B independent evaluations per launch.  As in linalg.ExactMLLFunction the gradients are produced in ``forward``
    (when any input needs one), ahead of the host's wait for the factorisation status; ``backward`` only scales them."""

    value_needs_alpha = False

    @staticmethod
    def forward(ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU):
        return _batched_forward(BatchedMLLFunction, ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU)

    @staticmethod
    def tail(gctx, ws, need_grad, ops, grads, kind, d_split):
        if not need_grad:
            return
        gctx.lauum_batched(ws.Li, ws.Ki)
        gctx.grad_reduce_batched(*ops, ws.alpha, ws.Ki, *grads, kind=kind, d_split=d_split)

    @staticmethod
    def result(ws, need_grad):
        return ws.out3[:, 2].clone(), (ws.alpha.clone() if need_grad else None)

    @staticmethod
    def backward(ctx, grad_out):
        return _batched_backward(ctx, grad_out)


def batched_mll(U: torch.Tensor, w: torch.Tensor, sf2: torch.Tensor, tau: torch.Tensor, mean: torch.Tensor, y: torch.Tensor,
                grp: Optional[torch.Tensor] = None, kind: int = KIND_RBF, d_split: int = 0, n_grad_dims: int = 0) -> torch.Tensor:
    """(B,) log N(y | mean_b, sf2_b k(U_b, U_b; w_b) + diag(tau_b[grp])) for B parameter sets in one pass."""
    return BatchedMLLFunction.apply(U, w, sf2, tau, mean, y, grp, kind, d_split, int(n_grad_dims))


class BatchedLOOFunction(torch.autograd.Function):
    """B leave-one-out log pseudo-likelihoods per launch: ``linalg.ExactLOOFunction`` with the arguments, the broadcasting, the
    NaN-for-not-positive-definite contract and the backward scaling of :class:`BatchedMLLFunction`; dloo/dmean = -beta and
    dloo/dy = +beta.  The batched twin of ``ExactLOOFunction.tail``, all of it enqueued ahead of the host's wait: d, a, sqrt(b) and
    the value from the rows of Linv (gpp_loo_scalars_batched); with a gradient beta = P a by the two triangular products into
    scratch, the LAUUM into Ki, S = diag(sqrt b) P into A (dead since trtri), the lower triangle of S^T S into Li (dead since
    beta), gpp_loo_grad_reduce_batched.  Three B x N x N buffers, as for the MLL.  No host wait of its own: inside a graph capture
    it makes ``_factor_batched``'s single attempt and leaves the status words on the device."""

    value_needs_alpha = True

    @staticmethod
    def forward(ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU):
        return _batched_forward(BatchedLOOFunction, ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU)

    @staticmethod
    def tail(gctx, ws, need_grad, ops, grads, kind, d_split):
        B, N, lv = ws.B, ws.N, ws.loo_vectors()
        gctx.loo_scalars_batched(ws.Li, ws.alpha, None, lv.d, a=lv.a, sqrtb=lv.sb, loo=lv.val)
        if not need_grad:
            return
        gctx.mll_reduce_batched(ws.A, ws.Li, lv.a, lv.z, lv.out3)  # beta = Linv^T (Linv a): ws.z / ws.out3 stay the evaluation's
        gctx.alpha_batched(ws.Li, lv.z, lv.beta)
        gctx.lauum_batched(ws.Li, ws.Ki)
        gctx.sym_rowscale_batched(ws.Ki, lv.sb, ws.A)
        gctx.gemm_batched(1, 0, N, N, N, 1.0, ws.A[0], ws.A.stride(0), ws.A[0], ws.A.stride(0), 0.0, ws.Li[0], ws.Li.stride(0), B,
                          c_tri=1)  # C(lower) = S^T S = P diag(b) P
        gctx.loo_grad_reduce_batched(*ops, ws.alpha, lv.beta, ws.Li, *grads, kind=kind, d_split=d_split)

    @staticmethod
    def result(ws, need_grad):
        lv = ws.loo_vectors()
        return lv.val.clone(), (lv.beta.neg() if need_grad else None)  # dloo/dmean = -beta

    @staticmethod
    def backward(ctx, grad_out):
        return _batched_backward(ctx, grad_out)


def _even_elements(t: torch.Tensor) -> torch.Tensor:
    """``t`` (B, M, D) contiguous with every element 16-byte aligned: an odd M D is padded by one double per element (the batched
    derivative kernels take even batch strides only).  A shared (M, D) block is returned as it is."""
    if t.dim() == 2 or not (t.shape[1] * t.shape[2]) & 1:
        return t
    B, M, D = t.shape
    buf = torch.empty(B, M * D + 1, dtype=t.dtype, device=t.device)
    out = buf[:, :M * D].view(B, M, D)
    out.copy_(t)
    return out


class BatchedGEKFunction(torch.autograd.Function):
    """``linalg.ExactGEKFunction`` with a leading batch dimension: (B,) joint log-densities log N([y - mean_b; r_g] | 0, Kj_b) of N
    function rows and q gradient observations, Kj_b built from w_b, sf2_b, tau_b (and U_b, Ug_b when the features differ per element).
        U (N, D) shared or (B, N, D);  Ug (Mg, D) shared or (B, Mg, D);  w (B, D);  sf2 (B,);  tau (B, S);  mean (B, N) or (N,);
        y (N,) or (B, N);  r_g (q,) shared;  nu (q,) shared or None
    ``nu=None``: ``nugget_rel`` times the prior curvature at EACH element's w and sf2, whose derivative by w and sf2 is added on the
    host as (B, nd) sums, as the eager function does.  The sequence is the eager one, every launch serving all elements: the three
    blocks into the upper triangle of ``ws.A`` (the two derivative blocks by gpp_cross_kernel_dx_batched / gpp_kernel_dxdx_batched,
    built aside and copied when N is odd: their 16-byte stores need an even first column), nu and the jitter on the gradient rows'
    diagonal, potrf, trtri, z, alpha, LAUUM, gpp_grad_reduce_batched on the leading N x N views, gpp_gek_grad_reduce_batched.
    The attempts are ``_factor_batched``'s: an element that fails is retried with the schedule's next jitter on ITS whole diagonal
    (function and gradient rows, as the eager function adds ``jit`` to both) while the others keep theirs; one that is still not
    positive definite returns NaN and zero gradients.  The gradients are produced in ``forward``; ``backward`` is
    ``_batched_backward`` with two blocks of feature rows.  Not available inside a graph capture (as the eager objective)."""

    @staticmethod
    def forward(ctx, U, Ug, w, sf2, tau, mean, y, r_g, nu, grp, kind, d_split, d0, nd, dU, nugget_rel, sel=None):
        from .linalg import KernelSpec, _curvature_coefficients

        dev = w.device
        gctx = get_context(dev)  # raises GppError for anything but a GPU: there is no CPU path
        with torch.cuda.device(dev):
            if torch.cuda.is_current_stream_capturing():
                raise NotImplementedError("the gradient-enhanced objective is not available inside a graph capture")
            B, D = w.shape
            N, Mg = U.shape[-2], Ug.shape[-2]
            q = Mg * nd if sel is None else sel.q
            n = N + q
            Ud, Ugd = _even_elements(_as_f64(U.detach(), dev)), _even_elements(_as_f64(Ug.detach(), dev))
            wd, sd, td, grp, S = _batched_operands(w, sf2, tau, grp)
            need = ctx.needs_input_grad
            need_grad = any(need[:7])
            dUk = dU if (need[0] or need[1]) and dU > 0 else 0
            # c_j of the prior curvature c_j w_j sf2 (linalg.gradient_prior_curvature): the kind and the split are shared
            coef = float(nugget_rel) * _curvature_coefficients(KernelSpec(wd[0], sd[0], kind, d_split))[d0:d0 + nd]
            if nu is None:
                nu_d = coef * wd[:, d0:d0 + nd] * sd.unsqueeze(1)  # (B, nd)
                nu_d = nu_d.repeat(1, Mg) if sel is None else nu_d[:, sel.flat % nd]
            else:
                nu_d = _as_f64(nu.detach().reshape(1, -1), dev)
            ws = get_batched_workspace(gctx, B, n)
            ws.epoch += 1
            torch.sub(_as_f64(y.detach(), dev).expand(B, N), _as_f64(mean.detach(), dev).expand(B, N), out=ws.r[:, :N])
            ws.r[:, N:].copy_(_as_f64(r_g.detach().reshape(1, -1), dev).expand(B, q))
            g_w, g_s, g_t, g_Ud, g_Ugd = _grad_buffers(need_grad, dev, (B,), D, S, (N, dUk), (Mg, dUk))
            aligned = N % 2 == 0
            Kfg_w, Kgg_w = ws.A[:, :N, N:n], ws.A[:, N:n, N:n]
            Kfg_out = Kfg_w if aligned else torch.empty(B, N, row_stride(q), dtype=torch.float64, device=dev)[:, :, :q]
            Kgg_out = Kgg_w if aligned else torch.empty(B, q, row_stride(q), dtype=torch.float64, device=dev)[:, :, :q]
            gdiag = Kgg_w.diagonal(dim1=1, dim2=2)

            def rest():
                gctx.trtri_batched(ws.A, ws.Li, ws.Ki)
                gctx.mll_reduce_batched(ws.A, ws.Li, ws.r, ws.z, ws.out3)
                if not need_grad:
                    return
                gctx.alpha_batched(ws.Li, ws.z, ws.alpha)
                gctx.lauum_batched(ws.Li, ws.Ki)
                gctx.grad_reduce_batched(Ud, wd, sd, grp, S, ws.alpha[:, :N], ws.Ki[:, :N, :N], dUk, g_w, g_s, g_t, g_Ud, kind=kind,
                                         d_split=d_split)
                gctx.gek_grad_reduce_batched(Ud, Ugd, wd, sd, d0, nd, ws.alpha, ws.Ki, dUk, g_w, g_s, g_Ud, g_Ugd, kind=kind,
                                             d_split=d_split, sel=sel)
                if nu is None:
                    # d nu_k / dw_j = rel c_j sf2, d nu_k / dsf2 = rel c_j w_j on the rows k = (a, j), times W_kk
                    a_g = ws.alpha[:, N:]
                    Wd = 0.5 * (a_g * a_g - ws.Ki[:, N:n, N:n].diagonal(dim1=1, dim2=2))
                    if sel is not None:  # (scattered into the dense layout, zeros elsewhere: the same ordered sum, no atomics)
                        dense = torch.zeros(B, Mg * nd, dtype=torch.float64, device=dev)
                        dense[:, sel.flat] = Wd
                        Wd = dense
                    Wd = Wd.reshape(B, Mg, nd).sum(1)
                    g_w[:, d0:d0 + nd].add_(coef * sd.unsqueeze(1) * Wd)
                    g_s.add_((coef * wd[:, d0:d0 + nd] * Wd).sum(1))

            def build(extra):  # (never None: this objective refuses a capture)
                gctx.kernel_build_batched(Ud, wd, sd, td + extra, grp, ws.A[:, :N, :N], kind=kind, d_split=d_split, uplo=UPLO_UPPER)
                gctx.cross_kernel_dx_batched(Ugd, Ud, wd, sd, d0, nd, Kfg_out, kind=kind, d_split=d_split, sel=sel)
                gctx.kernel_dxdx_batched(Ugd, Ugd, wd, sd, d0, nd, Kgg_out, kind=kind, d_split=d_split, sel_a=sel, sel_b=sel)
                if not aligned:
                    Kfg_w.copy_(Kfg_out)
                    Kgg_w.copy_(Kgg_out)
                gdiag.add_(nu_d + extra)

            ok = _factor_batched(gctx, ws, build, after=rest)
            grads = (g_w, g_s, g_t, (g_Ud, g_Ugd), ws.alpha[:, :N].clone() if need_grad else None)
            return _batched_result(ctx, ok, ws.out3[:, 2].clone(), grads, (U, Ug), w, sf2, tau, mean, y)

    @staticmethod
    def backward(ctx, grad_out):
        return _batched_backward(ctx, grad_out)


def batched_gek_mll(U: torch.Tensor, Ug: torch.Tensor, w: torch.Tensor, sf2: torch.Tensor, tau: torch.Tensor, mean: torch.Tensor,
                    y: torch.Tensor, r_g: torch.Tensor, noise: Optional[torch.Tensor], grp: Optional[torch.Tensor], kind: int,
                    d_split: int, d0: int, nd: int, n_grad_dims: int = 0, sel=None) -> torch.Tensor:
    """(B,) joint log-densities log N([y - mean_b; r_g] | 0, Kj_b) of the N function rows and the q observed gradients with respect
    to the features d0 .. d0 + nd - 1 at the rows ``Ug``, for B parameter sets in one pass: ``linalg.exact_gek_mll`` with a leading
    batch dimension (:class:`BatchedGEKFunction` for the shapes).  ``noise``: the q variances of the gradient observations, shared,
    or None for ``gradient_enhanced.GRADIENT_NUGGET_REL`` times the prior curvature at each element's own hyperparameters; ``sel``: a
    ``backend.GradientSelection`` of the observed (point, direction) entries, one for every element.  Differentiable with respect to
    U[..., :n_grad_dims], Ug[..., :n_grad_dims], w, sf2, tau, mean and y; an element that is not positive definite after the jitter
    schedule gives NaN and zero gradients.  Refused under ``settings.sharded_evaluation`` and inside a graph capture."""
    from .gradient_enhanced import GRADIENT_NUGGET_REL
    from .linalg import _gradient_cache_refusals

    _gradient_cache_refusals("the gradient-enhanced objective")
    d0, nd, dU = int(d0), int(nd), int(n_grad_dims)
    if w.dim() != 2:
        raise ValueError(f"w must be (B, D) (got {tuple(w.shape)})")
    B, D = w.shape
    for t, name in ((U, "U"), (Ug, "Ug")):
        if t.dim() not in (2, 3) or t.shape[-1] != D or t.shape[-2] < 1 or (t.dim() == 3 and t.shape[0] != B):
            raise ValueError(f"{name} must be (rows, {D}) or ({B}, rows, {D}) with at least one row (got {tuple(t.shape)})")
    if nd < 1 or d0 < 0 or d0 + nd > D:
        raise ValueError(f"the differentiated features [{d0}, {d0 + nd}) must be a non-empty range of the {D} features")
    Mg = Ug.shape[-2]
    if sel is not None and (sel.num_points, sel.nd) != (Mg, nd):
        raise ValueError(f"a selection of {sel.num_points} points x {sel.nd} directions for {Mg} x {nd}")
    q = Mg * nd if sel is None else sel.q
    if r_g.numel() != q or (noise is not None and noise.numel() != q):
        raise ValueError(f"{r_g.numel()} gradients / {None if noise is None else noise.numel()} noise variances for {q} gradient "
                         "observations")
    if dU > d0:
        raise ValueError(f"the {dU} feature columns with a gradient must lie in front of the differentiated ones (d0 = {d0})")
    return BatchedGEKFunction.apply(U, Ug, w, sf2, tau, mean, y, r_g, noise, grp, int(kind), int(d_split), d0, nd, dU,
                                    GRADIENT_NUGGET_REL, sel)


def batched_loo(U: torch.Tensor, w: torch.Tensor, sf2: torch.Tensor, tau: torch.Tensor, mean: torch.Tensor, y: torch.Tensor,
                grp: Optional[torch.Tensor] = None, kind: int = KIND_RBF, d_split: int = 0, n_grad_dims: int = 0) -> torch.Tensor:
    """(B,) leave-one-out log pseudo-likelihoods sum_i log p(y_i | y_-i; theta_b) for B parameter sets in one pass; the signature
    and the autograd contract of :func:`batched_mll`."""
    return BatchedLOOFunction.apply(U, w, sf2, tau, mean, y, grp, kind, d_split, int(n_grad_dims))

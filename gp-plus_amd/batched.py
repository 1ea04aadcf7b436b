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
Elements whose covariance is not positive definite after the jitter schedule (gpytorch's 1e-8 * 10^i) return NaN and
zero gradients instead of raising: one bad restart must not stop the others (the drivers score it +inf).
"""
from __future__ import annotations

import threading
from typing import Dict, Optional, Tuple

import torch

from .backend import KIND_RBF, UPLO_UPPER, GppContext, get_context
from .linalg import _as_f64
from .psd_safe import jitter_schedule

__all__ = ["BatchedWorkspace", "BatchedMLLFunction", "batched_mll", "BatchedLOOFunction", "batched_loo"]


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


def _factor_batched(gctx: GppContext, ws: BatchedWorkspace, U, w, sf2, tau, grp, kind, d_split, after=None) -> torch.Tensor:
    """Build + factor all elements; failing ones are retried with gpytorch's jitter schedule added to THEIR noise.
    Returns the boolean mask (B,) of elements that are positive definite in the end.  ``after()`` enqueues the rest of
    the evaluation before the host waits for the status words (one wait per attempt, covering the factorisation only)."""
    if torch.cuda.is_current_stream_capturing():
        # inside a HIP-graph capture (optim/mll_batched.py) nothing may wait for the host: ONE attempt without jitter; the status
        # words stay on the device and the owner of the graph re-runs the step eagerly when any of them is not zero
        gctx.kernel_build_batched(U, w, sf2, tau, grp, ws.A, kind=kind, d_split=d_split, uplo=UPLO_UPPER)
        gctx.potrf_batched(ws.A, ws.Li, ws.info)
        if after is not None:
            after()
        return ws.info == 0
    jitters = jitter_schedule()[1:]  # (the first attempt is the unjittered one)
    extra = torch.zeros(ws.B, 1, dtype=torch.float64, device=U.device)
    ok = None
    for attempt in range(len(jitters) + 1):
        gctx.kernel_build_batched(U, w, sf2, tau + extra, grp, ws.A, kind=kind, d_split=d_split, uplo=UPLO_UPPER)
        gctx.potrf_batched(ws.A, ws.Li, ws.info)
        ok = ws.info == 0
        ws.info_host.copy_(ws.info, non_blocking=True)
        ws.info_event.record()
        if after is not None:
            after()
        ws.info_event.synchronize()
        if bool((ws.info_host == 0).all()) or attempt == len(jitters):
            break
        extra = torch.where(ok.unsqueeze(1), extra, torch.full_like(extra, jitters[attempt]))
    return ok


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
    Ud, wd, sd, td = _as_f64(U.detach(), dev), _as_f64(w.detach(), dev), _as_f64(sf2.detach().reshape(B), dev), \
        _as_f64(tau.detach().reshape(B, -1), dev)
    S = td.shape[1]
    if grp is not None and grp.dtype != torch.int32:
        grp = grp.to(torch.int32)
    ws = get_batched_workspace(gctx, B, N)
    ws.epoch += 1
    torch.sub(_as_f64(y.detach(), dev).expand(B, N), _as_f64(mean.detach(), dev).expand(B, N), out=ws.r)
    need = ctx.needs_input_grad
    need_grad = any(need[:6])
    need_U = need[0] and dU > 0
    g_w = g_s = g_t = g_Ud = None
    if need_grad:
        g_w = torch.empty(B, D, dtype=torch.float64, device=dev)
        g_s = torch.empty(B, dtype=torch.float64, device=dev)
        g_t = torch.empty(B, S, dtype=torch.float64, device=dev)
        g_Ud = torch.empty(B, N, dU, dtype=torch.float64, device=dev) if need_U else None
    ops, grads = (Ud, wd, sd, grp, S), (dU if need_U else 0, g_w, g_s, g_t, g_Ud)

    def rest():
        gctx.trtri_batched(ws.A, ws.Li, ws.Ki)
        gctx.mll_reduce_batched(ws.A, ws.Li, ws.r, ws.z, ws.out3)
        if need_grad or fn.value_needs_alpha:
            gctx.alpha_batched(ws.Li, ws.z, ws.alpha)
        fn.tail(gctx, ws, need_grad, ops, grads, kind, d_split)

    ok = _factor_batched(gctx, ws, Ud, wd, sd, td, grp, kind, d_split, after=rest)
    value, g_mean = fn.result(ws, need_grad)
    ctx.saved = (g_w, g_s, g_t, g_Ud, g_mean, ok, (B, N, Ud.shape[-1], dU))
    ctx.in_dtypes = (U.dtype, w.dtype, sf2.dtype, tau.dtype, mean.dtype, y.dtype)
    ctx.shapes = (U.shape, sf2.shape, tau.shape, mean.shape, y.shape)
    return torch.where(ok, value, torch.full_like(value, float("nan")))


def _batched_backward(ctx, grad_out):
    """The gradients of (U, w, sf2, tau, mean, y) from the fp64 ones the forward produced, scaled by ``grad_out`` (zero for an
    element that is not positive definite), each in its input's dtype and shape.  The saved ``g_mean`` is the objective's derivative
    by the mean (alpha for the MLL, -beta for LOO); y receives its negative."""
    g_w, g_s, g_t, g_Ud, gm_all, ok, (B, N, Dfull, dU) = ctx.saved
    dev = gm_all.device
    U_shape, sf2_shape, tau_shape, mean_shape, y_shape = ctx.shapes
    need_U = g_Ud is not None
    go = torch.where(ok, grad_out.to(torch.float64), torch.zeros_like(grad_out, dtype=torch.float64))  # failed: no gradient
    dt = ctx.in_dtypes
    gm = torch.where(ok.unsqueeze(1), gm_all, torch.zeros_like(gm_all))
    g_U = None
    if ctx.needs_input_grad[0]:
        full = torch.zeros(B, N, Dfull, dtype=torch.float64, device=dev)
        if need_U:
            full[:, :, :dU] = torch.where(ok.view(B, 1, 1), g_Ud, torch.zeros_like(g_Ud)) * go.view(B, 1, 1)
        g_U = (full if len(U_shape) == 3 else full.sum(0)).to(dt[0])

    def red(t, shape):  # gradient of a broadcast argument: sum over the batch
        return t.reshape(shape) if len(shape) == t.dim() else t.sum(0).reshape(shape)

    g_mean = go.unsqueeze(1) * gm
    nanfree = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    return (g_U,
            nanfree(go.unsqueeze(1) * g_w).to(dt[1]) if ctx.needs_input_grad[1] else None,
            nanfree(go * g_s).reshape(sf2_shape).to(dt[2]) if ctx.needs_input_grad[2] else None,
            nanfree(go.unsqueeze(1) * g_t).reshape(tau_shape).to(dt[3]) if ctx.needs_input_grad[3] else None,
            red(g_mean, mean_shape).to(dt[4]) if ctx.needs_input_grad[4] else None,
            red(-g_mean, y_shape).to(dt[5]) if ctx.needs_input_grad[5] else None,
            None, None, None, None)


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


def batched_loo(U: torch.Tensor, w: torch.Tensor, sf2: torch.Tensor, tau: torch.Tensor, mean: torch.Tensor, y: torch.Tensor,
                grp: Optional[torch.Tensor] = None, kind: int = KIND_RBF, d_split: int = 0, n_grad_dims: int = 0) -> torch.Tensor:
    """(B,) leave-one-out log pseudo-likelihoods sum_i log p(y_i | y_-i; theta_b) for B parameter sets in one pass; the signature
    and the autograd contract of :func:`batched_mll`."""
    return BatchedLOOFunction.apply(U, w, sf2, tau, mean, y, grp, kind, d_split, int(n_grad_dims))

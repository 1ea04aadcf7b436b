"""Exact-GP linear algebra on the MI355X: one ``torch.autograd.Function`` whose forward and backward are sequences
of libgpp_hip calls (no ATen linear algebra, no CPU fallback).

Replaces, for the path ``optim/mll_torch.py:114-117``:
  forward  = gpytorch ``MultivariateNormal.log_prob`` -> ``inv_quad_logdet`` -> ``psd_safe_cholesky``
             (kernel build K1-K4, Cholesky K5, solve + logdet + quadratic form K6)
  backward = ATen ``cholesky_backward`` + the backward of every N^2 kernel op (K7): Ky^-1 by trtri + lauum, then ONE
             tiled reduction of W = (alpha alpha^T - Ky^-1)/2 against dKy/dtheta.
Both halves are ENQUEUED together in the Function's forward when a gradient is wanted (see ExactMLLFunction), so that
the single host sync of an evaluation — reading the factorisation status — comes after all of its device work.
Jitter policy (``psd_safe.py``, one driver for every factorisation of the package) restates
gpytorch.utils.cholesky.psd_safe_cholesky [3P]: 1e-8 * 10^i, i = 0..2 (fp64), warn, then ``NotPSDError``; NaN inputs raise ``NanError``.
"""
from __future__ import annotations

import math
import threading
from contextlib import contextmanager, nullcontext
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from .backend import (KIND_MATERN32, KIND_RBF, UPLO_FULL, UPLO_UPPER, GppContext, get_context, row_stride, rows_buffer,
                      square_buffer)
from .psd_safe import inputs_nan_probe, psd_safe
from . import settings

__all__ = ["KernelSpec", "exact_mll", "ExactMLLFunction", "CalibratedMLLFunction", "Calibration", "exact_loo", "ExactLOOFunction",
           "loo_moments", "exact_cv", "ExactCVFunction", "exact_gek_mll", "ExactGEKFunction",
           "cv_moments", "EvalWorkspace", "dense_kernel", "cross_kernel",
           "FactorCache", "factorize", "append_to_cache", "GradientFactorCache", "append_gradients_to_cache",
           "predict_from_gradient_cache", "dense_log_prob", "predict_mean", "predict_var", "predictive_cov_upper",
           "train_post_cov_upper", "mvn_root", "mvn_draw"]


@dataclass
class KernelSpec:
    """What the fused tile kernel needs: K_ij = sf2 * k(sum_d w_d (u_id-u_jd)^2).  All tensors live on the GPU."""
    w: torch.Tensor            # (D,) weights, autograd-connected to the raw lengthscales
    sf2: torch.Tensor          # () outputscale, autograd-connected
    kind: int = KIND_RBF
    d_split: int = 0


class EvalWorkspace:
    """Device buffers of one N-point evaluation, reused across evaluations (3 N x N fp64 matrices: Ky -> U (upper),
    Linv (lower) + its mirror (upper), scratch / Kinv (lower)).  ``epoch`` increments on every forward so a stale backward can tell its factors were overwritten."""

    def __init__(self, ctx: GppContext, N: int):
        dev = ctx.device
        self.N = N
        self.A = square_buffer(N, dev)
        self.Li = square_buffer(N, dev)
        self.Ki = square_buffer(N, dev)
        self.z = torch.empty(N, dtype=torch.float64, device=dev)
        self.alpha = torch.empty(N, dtype=torch.float64, device=dev)
        self.r = torch.empty(N, dtype=torch.float64, device=dev)
        self.out3 = torch.empty(3, dtype=torch.float64, device=dev)
        self.info = torch.zeros(1, dtype=torch.int32, device=dev)
        self.info_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.info_event = torch.cuda.Event()
        self.epoch = 0
        self._loo = None

    def loo_vectors(self):
        """The O(N) vectors of a leave-one-out evaluation (ExactLOOFunction), allocated on first use: d, a, sqrt(b), beta, the
        scratch z / out3 of beta's solve (the evaluation's own z and out3 stay what the value was computed from) and the value."""
        if self._loo is None:
            from types import SimpleNamespace
            v = lambda n: torch.empty(n, dtype=torch.float64, device=self.A.device)  # noqa: E731
            self._loo = SimpleNamespace(d=v(self.N), a=v(self.N), sb=v(self.N), beta=v(self.N), z=v(self.N), out3=v(3), val=v(1))
        return self._loo


_workspaces: Dict[Tuple[int, int, int], EvalWorkspace] = {}
_workspaces_lock = threading.Lock()
_tls = threading.local()


@contextmanager
def eval_slot(slot: int):
    """Evaluations issued inside this block (by this host thread) use workspace ``slot``.  Independent evaluations
    that run concurrently — e.g. two restarts of a fit driven from two threads on two HIP streams — take distinct
    slots so their N x N buffers do not alias (each slot holds 3 x 8 N^2 bytes)."""
    old = getattr(_tls, "slot", 0)
    _tls.slot = slot
    try:
        yield
    finally:
        _tls.slot = old


def current_slot() -> int:
    return getattr(_tls, "slot", 0)

#: smallest N for which gpp_potrf_ws (with scratch) runs its look-ahead driver on the internal streams (gpp_api.hip)
LOOKAHEAD_MIN_N = 3840

#: largest N at which gpp_lauum still runs its small tiles: the fused LAUUM + gradient reduction (128-wide tiles only) serves N above it
FUSED_GRAD_MIN_N = 5120

#: optional stage timing (bench.py): when this is a list, every stage appends (name, start_event, end_event) recorded
#: on the stream the kernels are launched on (PyTorch's current stream).
STAGE_EVENTS = None


class _stage:
    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        if STAGE_EVENTS is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if STAGE_EVENTS is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            STAGE_EVENTS.append((self.name, self.e0, e1))
        return False


def get_workspace(ctx: GppContext, N: int, slot: int = 0) -> EvalWorkspace:
    key = (ctx.index, N, slot)
    ws = _workspaces.get(key)
    if ws is None:
        with _workspaces_lock:
            # keep at most one size per (device, slot): drop others so 3 x 8 N^2 bytes are not held per historical N
            for k in [k for k in _workspaces if k[0] == ctx.index and k[2] == slot]:
                del _workspaces[k]
            ws = EvalWorkspace(ctx, N)
            _workspaces[key] = ws
    return ws


def _as_f64(t: torch.Tensor, device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float64).contiguous()


def _factor(ctx: GppContext, ws: EvalWorkspace, U, w, sf2, tau, grp, kind, d_split, after=None) -> float:
    """Build Ky (upper) and factor it, with gpytorch's jitter-retry policy.  Returns the jitter that was needed.
    ``after()`` enqueues whatever follows the factorisation BEFORE ``info`` is read back, so the GPU keeps working while
    the host waits (and afterwards runs the Python between forward and backward); a failed attempt just repeats it."""
    if torch.cuda.is_current_stream_capturing():
        # Inside a HIP-graph capture (gp-plus_amd/graphed.py) nothing may wait for the host: ONE attempt without jitter, the
        # status stays on the device in ``ws.info`` — the owner of the graph reads it with the result of every replay and
        # falls back to this eager path (jitter retries, exceptions) when it is not zero.
        if ws.N >= LOOKAHEAD_MIN_N:
            raise RuntimeError("graph capture of the evaluation is limited to the single-stream factorisation (N < 3840)")
        ctx.kernel_build(U, w, sf2, tau, grp, ws.A, jitter=0.0, kind=kind, d_split=d_split, uplo=UPLO_UPPER)
        ctx.potrf(ws.A, ws.Li, ws.info, ws.Ki)
        if after is not None:
            after()
        return 0.0

    def build_factor(jit):
        # Build and factorisation are ONE call: where the ticket list runs (N >= 6912) only the first diagonal block's columns of
        # Ky are built on this stream; the rest is written on the library's CU-masked update stream in front of the executor,
        # beside the first panel on its own 32 CUs.  (As an UNMASKED launch beside the panel the same build had flooded every CU,
        # the panel's included, and the first leaf waited for it anyway: 53.6 ms against 0.64 + 52.4, not adopted then.)
        # The "kernel_build" stage stays as the mark of an evaluation's first launch (tools/c3_stages.py and config_stages.py
        # measure the gap in front of it); the build's time is part of "potrf".
        with _stage("kernel_build"):
            pass
        with _stage("potrf"):
            ctx.build_potrf(U, w, sf2, tau, grp, ws.A, ws.Li, ws.info, ws.Ki, jitter=jit, kind=kind, d_split=d_split)

    return _attempts(ctx, ws, build_factor, inputs_nan_probe(U, w, sf2, tau), after)


def _attempts(ctx: GppContext, ws: EvalWorkspace, build_factor, nan_probe, after=None) -> float:
    """The attempt every single-GPU factorisation of an evaluation makes, under ``psd_safe``: ``build_factor(jit)`` enqueues the
    matrix with ``jit`` on its diagonal and its factorisation into ``ws`` (status in ``ws.info``), ``after()`` the rest of the
    evaluation, and only then the host waits for the status word.  Returns the jitter that was needed."""
    def attempt(jit):
        # The factorisation's launches (a DAG over the library's internal streams, ~1000 launches at N = 20000) run fastest
        # when they are enqueued while the device executes them, and measurably slower when they were parked in the
        # queues beforehand — N = 20000: potrf 55.7 ms when enqueued on an idle device, 58.0 when enqueued ~1 ms ahead
        # (behind the previous evaluation's gradient reduction), 58.7-59.3 when enqueued a whole evaluation ahead, and
        # the stages of the evaluation that is still running slow down as well (GPU_MAX_HW_QUEUES 4 / 8 / 16 alike; an
        # idle pause alone changes nothing).  So the host waits HERE for whatever is still running on this stream: the
        # Python between two evaluations has overlapped the previous one's inverse stages by now and nothing is exposed.
        # bench.py at N = 20000 on one box: 151-153 ms per evaluation without this wait, 143-144 with it; C3 (N = 10000)
        # 25.4-26.0 -> 24.3-24.8 ms.
        if ws.N >= LOOKAHEAD_MIN_N:  # (below, the factorisation is a single-stream chain and the host is the bottleneck)
            torch.cuda.current_stream(ctx.index).synchronize()
        build_factor(jit)
        # the second host wait of an evaluation (the reference syncs on loss.item() too) covers the factorisation only: the
        # status goes to pinned host memory behind an event, the rest of the evaluation is enqueued, THEN the host waits
        ws.info_host.copy_(ws.info, non_blocking=True)
        ws.info_event.record(torch.cuda.current_stream(ctx.index))
        if after is not None:
            after()
        ws.info_event.synchronize()
        return int(ws.info_host[0])

    return psd_safe(ctx, attempt, nan_probe)


# ---------------------------------------------------------------------------------------------------
# what the evaluation Functions share (ExactMLLFunction, ExactLOOFunction, sharded.ShardedMLLFunction)
# ---------------------------------------------------------------------------------------------------
def _operands(U, w, sf2, tau, grp):
    """The operands of an evaluation as the kernels take them: U, w, sf2 (1,) and tau (S,) detached, fp64 and contiguous on U's
    device, and ``grp`` as int32."""
    dev = U.device
    Ud, wd, sd, td = _as_f64(U.detach(), dev), _as_f64(w.detach(), dev), _as_f64(sf2.detach().reshape(1), dev), \
        _as_f64(tau.detach().reshape(-1), dev)
    if grp is not None and grp.dtype != torch.int32:
        grp = grp.to(torch.int32)
    return Ud, wd, sd, td, grp


def _eval_operands(ctx, U, w, sf2, tau, mean, y, grp, dU, Ug=None):
    """``_operands``, the number of noise groups S, and (need_grad, need_U) from ``ctx.needs_input_grad``, whose leading entries
    are the blocks of feature rows: U, or U and ``Ug``.  Notes on ``ctx`` what ``_eval_backward`` needs to hand every gradient back
    in its input's dtype and shape."""
    Ud, wd, sd, td, grp = _operands(U, w, sf2, tau, grp)
    blocks = (U,) if Ug is None else (U, Ug)
    k, need = len(blocks), ctx.needs_input_grad
    ctx.in_dtypes = tuple(t.dtype for t in blocks + (w, sf2, tau, mean, y))
    ctx.shapes = (tuple(t.shape[0] for t in blocks), sf2.shape, tau.shape)
    return Ud, wd, sd, td, grp, td.numel(), any(need[:k + 5]), any(need[:k]) and dU > 0


def _grad_buffers(need_grad, dev, lead, D, S, *rows):
    """The fp64 buffers the gradient reductions fill, of one problem (``lead`` = ()) or of B (``lead`` = (B,)): g_w (D), g_s (one
    value), g_t (S) and, for each block of feature rows ``(M, dU)``, g_U (M x dU) or None for dU = 0; all None without
    ``need_grad``."""
    def new(*shape):
        return torch.empty(lead + shape, dtype=torch.float64, device=dev) if need_grad else None

    return (new(D), new() if lead else new(1), new(S)) + tuple(new(M, dU) if dU > 0 else None for M, dU in rows)


def _eval_backward(ctx, grad_out, g_w, g_s, g_t, g_rows, g_mean):
    """The gradients of (the leading blocks of feature rows: U, or U and Ug; w, sf2, tau, mean, y) from the fp64 ones an evaluation
    produced, scaled by ``grad_out``, each in its input's dtype (and shape): a block's entry of ``g_rows`` (M x dU, or None) fills
    the leading columns of its gradient, the others are zero; ``g_mean`` is the objective's derivative by the mean (alpha for the
    MLL and GEK, -beta for LOO) and y receives its negative."""
    need, dt = ctx.needs_input_grad, ctx.in_dtypes
    row_counts, sf2_shape, tau_shape = ctx.shapes
    k = len(row_counts)
    go = grad_out.to(torch.float64)

    def rows(g_d, M):
        g = torch.zeros(M, g_w.shape[0], dtype=torch.float64, device=g_w.device)
        if g_d is not None:
            g[:, :g_d.shape[1]] = g_d
        return go * g

    return tuple(rows(g_d, M).to(dt[i]) if need[i] else None for i, (g_d, M) in enumerate(zip(g_rows, row_counts))) + (
        (go * g_w).to(dt[k]) if need[k] else None,
        (go * g_s).reshape(sf2_shape).to(dt[k + 1]) if need[k + 1] else None,
        (go * g_t).reshape(tau_shape).to(dt[k + 2]) if need[k + 2] else None,
        (go * g_mean).to(dt[k + 3]) if need[k + 3] else None,
        (-go * g_mean).to(dt[k + 4]) if need[k + 4] else None)


def _exact_forward(fn, ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot):
    """The forward of the single-GPU objectives.  ``fn`` (ExactMLLFunction / ExactLOOFunction) supplies what differs: whether the
    value alone needs alpha, the ``tail`` of the enqueued sequence behind trtri, z and alpha, and its ``result``."""
    gctx = get_context(U.device)  # raises GppError for anything but a GPU: there is no CPU path
    with torch.cuda.device(U.device):  # streams, events and the library's launches all refer to the model's GPU
        if not fn.capturable and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError(f"{getattr(fn, 'what', 'the leave-one-out objective')} is not available inside a graph capture")
        dev = U.device
        N, D = U.shape
        Ud, wd, sd, td, grp, S, need_grad, need_U = _eval_operands(ctx, U, w, sf2, tau, mean, y, grp, dU)
        need_grad = need_grad or getattr(fn, "wants_grad", False)  # (an input of the objective's own: the calibration parameters)
        ws = get_workspace(gctx, N, slot)
        ws.epoch += 1
        torch.sub(_as_f64(y.detach(), dev), _as_f64(mean.detach(), dev), out=ws.r)
        dUk = dU if need_U else 0
        g_w, g_s, g_t, g_Ud = _grad_buffers(need_grad, dev, (), D, S, (N, dUk))
        ops, grads = (Ud, wd, sd, grp, S), (dUk, g_w, g_s, g_t, g_Ud)

        def rest():
            with _stage("trtri"):
                gctx.trtri(ws.A, ws.Li, ws.Ki)
            with _stage("mll_reduce"):
                gctx.mll_reduce(ws.A, ws.Li, ws.r, ws.z, ws.out3)
            # (Measured and NOT adopted: z, the MLL scalars and alpha on a side stream beside the LAUUM launch — the extra
            #  stream perturbs the hardware-queue mapping of the NEXT evaluation's factorisation DAG: potrf 53.3 -> 58-60 ms,
            #  137 -> 142-144 ms per evaluation at N = 20000, tools/attic/side_ab.py.)
            if need_grad or fn.value_needs_alpha:
                with _stage("alpha"):
                    gctx.alpha(ws.Li, ws.z, ws.alpha)
            fn.tail(gctx, ws, need_grad, ops, grads, kind, d_split)

        _factor(gctx, ws, Ud, wd, sd, td, grp, kind, d_split, after=rest)
        value, g_mean = fn.result(ws, need_grad)
        ctx.saved = (g_w, g_s, g_t, (g_Ud,), g_mean)
        return value


class ExactMLLFunction(torch.autograd.Function):
    """mll = log N(y | mean, sf2*k(U,U;w) + diag(tau[grp]))  with gradients for U[:, :dU], w, sf2, tau, mean, y.

    The whole evaluation — value AND the parameter gradients (K7: Ky^-1 by trtri + lauum, one fused reduction) — is
    enqueued in ``forward`` ahead of the single host sync on the factorisation status whenever an input needs a gradient:
    the device then works through the Python that lies between the reference's ``-mll(...)`` and ``loss.backward()``
    (optim/mll_torch.py:116-117), and ``backward`` only scales the stored gradients by the incoming one."""

    capturable, value_needs_alpha = True, False

    @staticmethod
    def forward(ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot):
        return _exact_forward(ExactMLLFunction, ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot)

    @staticmethod
    def tail(gctx, ws, need_grad, ops, grads, kind, d_split):
        if not need_grad:
            return
        # Above FUSED_GRAD_MIN_N the gradient reduction is the EPILOGUE of the LAUUM's tiles where the library supports it (RBF,
        # D <= 16, no feature gradients): Ky^-1 is then neither written nor read, and ws.Ki holds the inverse's scratch, not
        # Ky^-1 (nothing reads it after a training evaluation: the prediction and sampling paths form their own).
        fused = False
        with _stage("lauum"):
            if ws.N > FUSED_GRAD_MIN_N:
                fused = gctx.lauum_grad(ws.Li, *ops, ws.alpha, *grads[:4], kind=kind)
            if not fused:
                gctx.lauum(ws.Li, ws.Ki)
        with _stage("grad_reduce"):
            if not fused:
                gctx.grad_reduce(*ops, ws.alpha, ws.Ki, *grads, kind=kind, d_split=d_split)

    @staticmethod
    def result(ws, need_grad):
        return ws.out3[2].clone(), (ws.alpha.clone() if need_grad else None)

    @staticmethod
    def backward(ctx, grad_out):
        return _eval_backward(ctx, grad_out, *ctx.saved) + (None,) * 5


def exact_mll(U: torch.Tensor, spec: KernelSpec, tau: torch.Tensor, mean: torch.Tensor, y: torch.Tensor,
              grp: Optional[torch.Tensor] = None, n_grad_dims: Optional[int] = None, slot: Optional[int] = None,
              calib: Optional["Calibration"] = None) -> torch.Tensor:
    """log N(y | mean, Ky) on the GPU; differentiable w.r.t. U[:, :n_grad_dims], spec.w, spec.sf2, tau, mean, y — and, with
    ``calib``, w.r.t. the calibration parameters ``calib.theta`` whose values ``U`` holds (CalibratedMLLFunction)."""
    if slot is None:
        slot = current_slot()
    if n_grad_dims is None:
        n_grad_dims = U.shape[1] if U.requires_grad else 0
    shard = settings.sharded_evaluation.value()
    if calib is not None:
        if shard is not None:
            raise NotImplementedError("calibration parameters are not available under settings.sharded_evaluation")
        return CalibratedMLLFunction.apply(U, spec.w, spec.sf2, tau, mean, y, grp, spec.kind, spec.d_split, int(n_grad_dims), slot,
                                           calib.theta, calib.member, calib.cols)
    if shard is not None:
        from .sharded import sharded_mll
        return sharded_mll(U, spec.w, spec.sf2, tau, mean, y, grp, spec.kind, spec.d_split, int(n_grad_dims),
                           group=shard.get("group"), nb=int(shard.get("nb", 1024)))
    return ExactMLLFunction.apply(U, spec.w, spec.sf2, tau, mean, y, grp, spec.kind, spec.d_split, int(n_grad_dims), slot)


class _CalibratedEvaluation:
    """What ``_exact_forward`` asks of an objective, for ONE evaluation of the marginal likelihood of a model with calibration
    parameters: ExactMLLFunction's sequence on the dense route (plain LAUUM, Ky^-1 in memory: the LAUUM-fused reduction has no
    feature gradients) followed by gpp_calib_grad_reduce on the same alpha and Ky^-1."""

    capturable, value_needs_alpha, what = False, False, "the marginal likelihood of a model with calibration parameters"

    def __init__(self, member, cols, wants_grad):
        self.member, self.cols, self.wants_grad, self.g_theta = member, cols, wants_grad, None

    def tail(self, gctx, ws, need_grad, ops, grads, kind, d_split):
        if not need_grad:
            return
        with _stage("lauum"):
            gctx.lauum(ws.Li, ws.Ki)
        with _stage("grad_reduce"):
            gctx.grad_reduce(*ops, ws.alpha, ws.Ki, *grads, kind=kind, d_split=d_split)
        if self.wants_grad:
            with _stage("calib_grad_reduce"):
                self.g_theta = torch.empty(self.cols.numel(), dtype=torch.float64, device=ws.A.device)
                gctx.calib_grad_reduce(*ops[:3], ws.alpha, ws.Ki, self.member, self.cols, self.g_theta, kind=kind, d_split=d_split)

    @staticmethod
    def result(ws, need_grad):
        return ExactMLLFunction.result(ws, need_grad)


class CalibratedMLLFunction(torch.autograd.Function):
    """:class:`ExactMLLFunction` with one more differentiable input, the calibration parameters ``theta`` (C,): theta[k] stands in
    feature column ``cols[k]`` of the rows with ``member[i] != 0`` (reference models/gp_plus.py:439-461).  ``U`` already holds the
    values — as constants: those columns are past ``dU`` — and
        d mll / d theta_k = sum_ij W_ij (m_i - m_j) dK_ij/du_{i,cols[k]},   W = (alpha alpha^T - Ky^-1) / 2
    comes from gpp_calib_grad_reduce, a scalar reduction per parameter: no N x D feature gradient exists on this route.  A sibling
    of ExactMLLFunction, so a model without calibration parameters enqueues exactly what it did before."""

    @staticmethod
    def forward(ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot, theta, member, cols):
        ev = _CalibratedEvaluation(member, cols, ctx.needs_input_grad[11])
        ctx.theta_dtype = theta.dtype
        value = _exact_forward(ev, ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot)
        ctx.g_theta = ev.g_theta
        return value

    @staticmethod
    def backward(ctx, grad_out):
        g_theta = None
        if ctx.needs_input_grad[11]:
            g_theta = (grad_out.to(torch.float64) * ctx.g_theta).to(ctx.theta_dtype)
        return _eval_backward(ctx, grad_out, *ctx.saved) + (None,) * 5 + (g_theta, None, None)


@dataclass
class Calibration:
    """The calibration parameters of a lazy covariance: ``theta`` (C,) autograd-connected to the model's ``Theta_<n>.constant``,
    ``member`` (N,) int32 (1 on the rows of the calibrated source) and ``cols`` (C,) int32 (feature column of each parameter)."""
    theta: torch.Tensor
    member: torch.Tensor
    cols: torch.Tensor


class ExactLOOFunction(torch.autograd.Function):
    """Leave-one-out log pseudo-likelihood (Rasmussen & Williams 5.4.2; gpytorch LeaveOneOutPseudoLikelihood without its 1/N)
        loo = sum_i log N(y_i | mu_i, s2_i),   s2_i = 1 / P_ii,   mu_i = y_i - alpha_i / P_ii,   P = Ky^-1, alpha = P (y - mean)
    with the inputs, gradients and autograd contract of :class:`ExactMLLFunction`.  With a = dloo/dalpha = -alpha / d,
    b = dloo/dd = 1 / (2 d) + alpha^2 / (2 d^2), beta = P a:
        dloo = sum_ij W_ij dKy_ij,   W = -(alpha beta^T + beta alpha^T) / 2 - P diag(b) P,   dloo/dmean = -beta,   dloo/dy = beta.
    Sequence (all enqueued ahead of the host's wait for the factorisation status, as in ExactMLLFunction): build + potrf, trtri,
    z, alpha, gpp_loo_scalars (d from the rows of Linv: no LAUUM for the value); with a gradient: beta by the same two
    triangular products, plain LAUUM into Ki, S = diag(sqrt b) P as a full square into A (dead since trtri), the lower triangle
    of S^T S by the TN GEMM into Li (dead since beta), gpp_loo_grad_reduce.  No fourth N x N buffer; the value is produced by the
    same kernels on the same inputs with and without a gradient.  Reference: optim/mll_noise_continuation.py:54 names the
    criterion and never evaluates it."""

    capturable, value_needs_alpha = False, True

    @staticmethod
    def forward(ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot):
        return _exact_forward(ExactLOOFunction, ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot)

    @staticmethod
    def tail(gctx, ws, need_grad, ops, grads, kind, d_split):
        N, lv = ws.N, ws.loo_vectors()
        with _stage("loo_scalars"):
            gctx.loo_scalars(ws.Li, ws.alpha, None, lv.d, a=lv.a, sqrtb=lv.sb, loo=lv.val)
        if not need_grad:
            return
        with _stage("loo_beta"):  # beta = Ky^-1 a = Linv^T (Linv a), into scratch: ws.z / ws.out3 stay the evaluation's
            gctx.mll_reduce(ws.A, ws.Li, lv.a, lv.z, lv.out3)
            gctx.alpha(ws.Li, lv.z, lv.beta)
        with _stage("lauum"):
            gctx.lauum(ws.Li, ws.Ki)
        with _stage("sym_rowscale"):
            gctx.sym_rowscale(ws.Ki, lv.sb, ws.A)
        with _stage("loo_gemm"):  # C(lower) = S^T S = P diag(b) P: M = N = K, row-contiguous TN
            gctx.gemm(1, 0, N, N, N, 1.0, ws.A, ws.A, 0.0, ws.Li, c_tri=1)
        with _stage("loo_grad_reduce"):
            gctx.loo_grad_reduce(*ops, ws.alpha, lv.beta, ws.Li, *grads, kind=kind, d_split=d_split)

    @staticmethod
    def result(ws, need_grad):
        lv = ws.loo_vectors()
        return lv.val[0].clone(), (lv.beta.neg() if need_grad else None)  # dloo/dmean = -beta

    @staticmethod
    def backward(ctx, grad_out):
        return _eval_backward(ctx, grad_out, *ctx.saved) + (None,) * 5


def exact_loo(U: torch.Tensor, spec: KernelSpec, tau: torch.Tensor, mean: torch.Tensor, y: torch.Tensor,
              grp: Optional[torch.Tensor] = None, n_grad_dims: Optional[int] = None, slot: Optional[int] = None) -> torch.Tensor:
    """Leave-one-out log pseudo-likelihood sum_i log p(y_i | y_-i) on the GPU; the signature and the autograd contract of
    :func:`exact_mll` (differentiable w.r.t. U[:, :n_grad_dims], spec.w, spec.sf2, tau, mean, y)."""
    if slot is None:
        slot = current_slot()
    if n_grad_dims is None:
        n_grad_dims = U.shape[1] if U.requires_grad else 0
    if settings.sharded_evaluation.value() is not None:
        raise NotImplementedError("the leave-one-out objective is not available under settings.sharded_evaluation")
    return ExactLOOFunction.apply(U, spec.w, spec.sf2, tau, mean, y, grp, spec.kind, spec.d_split, int(n_grad_dims), slot)


class _CVEvaluation:
    """What ``_exact_forward`` asks of an objective (``capturable``, ``value_needs_alpha``, ``tail``, ``result``) for ONE evaluation
    of the cross-validation objective: unlike the marginal likelihood and leave-one-out it carries an argument of its own, the folds."""

    capturable, value_needs_alpha, what = False, True, "the cross-validation objective"

    def __init__(self, folds):
        self.folds, self.terms, self.infos = folds, None, None

    def tail(self, gctx, ws, need_grad, ops, grads, kind, d_split):
        from .cv import fold_gradient_factors, fold_solves
        N, lv = ws.N, ws.loo_vectors()
        with _stage("cv_folds"):  # one batched sequence per bucket: P_FF, its factor and inverse factor, z, a, diag P_FF^-1, the terms
            a, _, self.terms, self.infos, kept = fold_solves(gctx, ws.Li, ws.alpha, self.folds, keep_factors=need_grad)
        if not need_grad:
            return
        lv.a.copy_(a)
        with _stage("cv_beta"):  # beta = Ky^-1 a by the two triangular products, as ExactLOOFunction
            gctx.mll_reduce(ws.A, ws.Li, lv.a, lv.z, lv.out3)
            gctx.alpha(ws.Li, lv.z, lv.beta)
        with _stage("lauum"):
            gctx.lauum(ws.Li, ws.Ki)
        with _stage("sym_rowscale"):  # Psq: the full symmetric square of Ky^-1 into A (dead since trtri)
            gctx.sym_rowscale(ws.Ki, torch.ones(N, dtype=torch.float64, device=ws.A.device), ws.A)
        with _stage("cv_rows"):  # S = the row blocks G_F P[F, :] stacked bucket after bucket into Li (dead after the LAUUM)
            for b, Li_b, z, na, out3 in kept:
                G = fold_gradient_factors(b, Li_b, z, na, out3)
                gctx.cv_rows(G, b.idx, b.off, ws.A, ws.Li[b.base:b.base + b.rows])
                del G
        del kept
        with _stage("cv_gemm"):  # C(lower) = S^T S = sum_F P[:, F] (dcv/dP_FF) P[F, :] into A (Psq is dead)
            gctx.gemm(1, 0, N, N, N, 1.0, ws.Li, ws.Li, 0.0, ws.A, c_tri=1)
        with _stage("loo_grad_reduce"):
            gctx.loo_grad_reduce(*ops, ws.alpha, lv.beta, ws.A, *grads, kind=kind, d_split=d_split)

    def result(self, ws, need_grad):
        from .cv import check_infos
        check_infos(self.infos, self.folds)  # (no jitter retry on a fold block: a jittered P_FF has no meaning)
        value = self.terms.sum() - 0.5 * ws.N * math.log(2.0 * math.pi)
        return value, (ws.loo_vectors().beta.neg() if need_grad else None)  # dcv/dmean = -beta


class ExactCVFunction(torch.autograd.Function):
    """Grouped (k-fold) cross-validation log pseudo-likelihood from one factorisation (gp-plus_amd/cv.py, gpp.h gpp_cv_blocks):
        cv = sum_F log p(y_F | y_-F) = sum_F [ -1/2 alpha_F' P_FF^-1 alpha_F + 1/2 log|P_FF| ] - (N / 2) log 2 pi,   P = Ky^-1
    with the inputs, gradients and autograd contract of :class:`ExactLOOFunction` plus the folds (a ``cv.FoldIndex``).  With
    a_F = -P_FF^-1 alpha_F = dcv/dalpha on F, dcv/dP_FF = (a_F a_F' + P_FF^-1) / 2 = G_F' G_F and beta = P a:
        dcv = sum_ij W_ij dKy_ij,   W = -(alpha beta^T + beta alpha^T) / 2 - S^T S,   dcv/dmean = -beta,   dcv/dy = beta,
    S the row blocks G_F P[F, :] stacked — leave-one-out's shape with a block-diagonal matrix in place of diag(b), so
    gpp_loo_grad_reduce takes it unchanged.  Sequence: build + potrf, trtri, z, alpha, the per-bucket batched fold solves
    (``cv.fold_solves``); with a gradient: beta, plain LAUUM into Ki, the full square Psq into A, G by element-wise torch ops on the
    small batches, gpp_cv_rows into Li, the TN GEMM into A's lower triangle, gpp_loo_grad_reduce.  No fourth N x N buffer; the value
    comes from the same kernels with and without a gradient.  Not capturable (the fold blocks' status is read on the host)."""

    @staticmethod
    def forward(ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot, folds):
        return _exact_forward(_CVEvaluation(folds), ctx, U, w, sf2, tau, mean, y, grp, kind, d_split, dU, slot)

    @staticmethod
    def backward(ctx, grad_out):
        return _eval_backward(ctx, grad_out, *ctx.saved) + (None,) * 6


def exact_cv(U: torch.Tensor, spec: KernelSpec, tau: torch.Tensor, mean: torch.Tensor, y: torch.Tensor, folds,
             grp: Optional[torch.Tensor] = None, n_grad_dims: Optional[int] = None, slot: Optional[int] = None) -> torch.Tensor:
    """Grouped cross-validation log pseudo-likelihood sum_F log p(y_F | y_-F) on the GPU for ``folds`` (an int k, one integer label
    per row, or a ``cv.FoldIndex``); the autograd contract of :func:`exact_loo`."""
    from .cv import FoldIndex
    folds = FoldIndex.make(folds, U.shape[0])  # host work: its errors come before a device is touched
    if slot is None:
        slot = current_slot()
    if n_grad_dims is None:
        n_grad_dims = U.shape[1] if U.requires_grad else 0
    if settings.sharded_evaluation.value() is not None:
        raise NotImplementedError("the cross-validation objective is not available under settings.sharded_evaluation")
    return ExactCVFunction.apply(U, spec.w, spec.sf2, tau, mean, y, grp, spec.kind, spec.d_split, int(n_grad_dims), slot, folds)


# ---------------------------------------------------------------------------------------------------
# dense evaluations (no autograd): .evaluate(), cross covariances, prediction
# ---------------------------------------------------------------------------------------------------
@torch.no_grad()
def dense_kernel(U: torch.Tensor, spec: KernelSpec, tau: Optional[torch.Tensor] = None,
                 grp: Optional[torch.Tensor] = None, jitter: float = 0.0) -> torch.Tensor:
    """Dense N x N covariance (full symmetric) — what ``lazy.evaluate()`` returns (models/gp_plus.py:474)."""
    dev = U.device
    gctx = get_context(dev)
    N = U.shape[0]
    out = square_buffer(N, dev)
    gctx.kernel_build(_as_f64(U, dev), _as_f64(spec.w, dev), _as_f64(spec.sf2.reshape(1), dev),
                      None if tau is None else _as_f64(tau.reshape(-1), dev),
                      None if grp is None else grp.to(torch.int32), out, jitter=jitter, kind=spec.kind,
                      d_split=spec.d_split, uplo=UPLO_FULL)
    return out


@torch.no_grad()
def cross_kernel(Ua: torch.Tensor, Ub: torch.Tensor, spec: KernelSpec) -> torch.Tensor:
    dev = Ua.device
    gctx = get_context(dev)
    M, N = Ua.shape[0], Ub.shape[0]
    out = rows_buffer(M, N, dev)
    gctx.cross_kernel(_as_f64(Ua, dev), _as_f64(Ub, dev), _as_f64(spec.w, dev), _as_f64(spec.sf2.reshape(1), dev), out,
                      kind=spec.kind, d_split=spec.d_split)
    return out


class FactorCache:
    """Cholesky factor, its inverse and alpha = Ky^-1 (y - m) of the training covariance: the analogue of gpytorch's
    prediction strategy caches (mean_cache / covar_cache) used by models/gpregression.py:122-149."""

    def __init__(self, gctx, L, Linv, alpha, U, spec, jitter, ws=None, z=None, refactor=None):
        self.gctx, self.L, self.Linv, self.alpha, self.U, self.spec, self.jitter = gctx, L, Linv, alpha, U, spec, jitter
        self.z = z  # Linv (y - m): the mean of a prediction that also wants the variance is V z
        # L and Linv live in the shared prediction workspace: another model's factorisation of the same size overwrites
        # them.  ``stale()`` tells the owner to factor again instead of predicting from someone else's matrices.
        self._ws, self._epoch = ws, (ws.epoch if ws is not None else 0)
        self._refactor = refactor  # (tau, grp, r = y - m): what ``refresh`` needs besides U and spec (O(N) copies)
        # ``append_to_cache``: the pair of matrices this cache's L / Linv are leading windows of when it owns them (never stale), and
        # how it was made: None (factorised), "in_place", "copy" or "refactor"
        self._own, self.route = None, None

    def stale(self) -> bool:
        return self._ws is not None and self._ws.epoch != self._epoch

    def refresh(self) -> None:
        """Factor again when another model of the same size has taken the shared workspace since (two GPs fitted on one X
        whose predictions are read alternately): the lazily evaluated variance of an EARLIER prediction stays valid, as it
        is in gpytorch, whose prediction strategy owns its caches.  Same inputs, same jitter schedule: the same factor."""
        if not self.stale():
            return
        if self._refactor is None:
            raise RuntimeError("the prediction workspace was reused by another model and this cache cannot be rebuilt")
        tau, grp, r = self._refactor
        with torch.cuda.device(self.U.device):
            fresh = _factorize(self.U, self.spec, tau, grp, torch.zeros_like(r), r)
        self.L, self.Linv, self.alpha, self.z, self.jitter = fresh.L, fresh.Linv, fresh.alpha, fresh.z, fresh.jitter
        self._ws, self._epoch = fresh._ws, fresh._epoch


@torch.no_grad()
def factorize(U, spec: KernelSpec, tau, grp, mean, y) -> FactorCache:
    get_context(U.device)
    with torch.cuda.device(U.device):
        return _factorize(U, spec, tau, grp, mean, y)


def _factorize(U, spec: KernelSpec, tau, grp, mean, y) -> FactorCache:
    dev = U.device
    gctx = get_context(dev)
    N = U.shape[0]
    Ud, wd, sd, td, grp = _operands(U, spec.w, spec.sf2, tau, grp)
    ws = get_workspace(gctx, N, slot=-1)
    ws.epoch += 1
    jit = _factor(gctx, ws, Ud, wd, sd, td, grp, spec.kind, spec.d_split)
    gctx.trtri(ws.A, ws.Li, ws.Ki)
    torch.sub(_as_f64(y, dev), _as_f64(mean, dev), out=ws.r)
    gctx.mll_reduce(ws.A, ws.Li, ws.r, ws.z, ws.out3)
    gctx.alpha(ws.Li, ws.z, ws.alpha)
    return FactorCache(gctx, ws.A, ws.Li, ws.alpha.clone(), Ud, KernelSpec(wd, sd.reshape(()), spec.kind, spec.d_split), jit, ws,
                       z=ws.z.clone(), refactor=(td.clone(), None if grp is None else grp.clone(), ws.r.clone()))


#: ``append_to_cache`` borders the factor for q <= min(N, APPEND_MAX_Q) new rows and factors all N + q rows from scratch above.
#: 2048 is the largest q the append was MEASURED at (tools/bench_condition.py, N = 20 000: 50.9 ms in place / 52.9 by copy against
#: 117.9 for the factorisation of 22 048 rows; the margin shrinks with q: 8.3x at 256, 2.3x at 2048): nothing above it is claimed.
APPEND_MAX_Q = 2048


class _OwnedFactors:
    """The two square matrices a conditioned cache owns: capacity x capacity buffers whose leading ``filled`` x ``filled`` windows hold
    the factor and the inverse factor.  Several caches may hold windows of one pair (a chain of in-place appends): a cache may
    append in place only while its own extent is the filled extent, i.e. while nobody has appended behind it."""

    def __init__(self, capacity: int, device):
        self.capacity, self.filled = capacity, 0
        self.A = square_buffer(capacity, device)
        self.Linv = square_buffer(capacity, device)


def _owned_copy(src: FactorCache, n: int, capacity: int) -> _OwnedFactors:
    own = _OwnedFactors(capacity, src.U.device)
    own.A[:n, :n].copy_(src.L[:n, :n])
    own.Linv[:n, :n].copy_(src.Linv[:n, :n])
    own.filled = n
    return own


def _owned_cache(gctx, own, n, alpha, U, spec, jitter, z, refactor, route) -> FactorCache:
    out = FactorCache(gctx, own.A[:n, :n], own.Linv[:n, :n], alpha, U, spec, jitter, ws=None, z=z, refactor=refactor)
    out._own, out.route = own, route
    return out


@torch.no_grad()
def append_to_cache(cache: FactorCache, Uq, tau, grp_q, mean_q, y_q, reserve: int = 256) -> FactorCache:
    """A new ``FactorCache`` of the N cached rows plus the q rows with features ``Uq``, noise groups ``grp_q`` (into ``tau``), prior
    means ``mean_q`` and targets ``y_q``, in O(N^2 q) by bordering the cached factor (gpp_chol_append) instead of O((N + q)^3).
    The result owns its matrices (capacity N + q + reserve; never stale, ``refresh`` does nothing); ``cache`` stays valid and
    bitwise unchanged.  ``route`` on the result tells what was done:
      "in_place"  ``cache`` owns its matrices, nobody has appended behind it and the capacity suffices: the new rows and columns
                  go into the same pair (the leading windows are not touched, so ``cache`` and its other holders go on reading them);
      "copy"      otherwise — the first append to a cache of the shared prediction workspace (refreshed first), a second child
                  of one parent, a full pair: the windows are copied into a new pair;
      "refactor"  the Schur complement was not positive definite, or q > min(N, APPEND_MAX_Q = 2048, the largest measured q): all N + q rows are factorised
                  from scratch under the jitter-retry policy of ``factorize``, and the factor is copied into an owned pair."""
    if settings.sharded_evaluation.value() is not None:
        raise NotImplementedError("appending to a factor cache is not available under settings.sharded_evaluation")
    dev = cache.U.device
    gctx = cache.gctx
    on_gpu = dev.type == "cuda"  # (anything else only under a stand-in context: the library itself has no CPU path)
    with torch.cuda.device(dev) if on_gpu else nullcontext():
        if on_gpu and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("appending to a factor cache is not available inside a graph capture")
        n, reserve = cache.U.shape[0], max(int(reserve), 0)
        Uq = _as_f64(Uq.detach(), dev)
        q = Uq.shape[0]
        if q < 1 or Uq.dim() != 2 or Uq.shape[1] != cache.U.shape[1]:
            raise ValueError(f"the new rows must be q >= 1 rows of {cache.U.shape[1]} features (got {tuple(Uq.shape)})")
        tau0, grp0, r0 = cache._refactor
        # One vector of noise levels serves the old and the new rows.  The two may differ in length by the zero-noise group that
        # Multifidelity_noise appends for rows of an unlisted source (present on one side only): the longer one is used, and the
        # levels both sides know must be the same numbers — the cached factor was built from the cache's.
        tau = _as_f64(tau.detach().reshape(-1), dev)
        both = min(tau.numel(), tau0.numel())
        if not torch.equal(tau[:both], tau0[:both]):
            raise ValueError("the noise levels of the new rows differ from those the cache was factorised with "
                             "(parameters changed since? factorise again instead of appending)")
        if tau.numel() < tau0.numel():
            tau = tau0
        if (grp0 is None) != (grp_q is None):
            raise ValueError("the new rows must carry noise groups exactly when the cached rows do")
        if grp_q is not None:
            grp_q = grp_q.to(device=dev, dtype=torch.int32).reshape(-1)
            if grp_q.numel() != q:
                raise ValueError(f"noise-group index has {grp_q.numel()} entries for {q} new rows")
        r_q = _as_f64(y_q.detach().reshape(-1), dev) - _as_f64(mean_q.detach().reshape(-1), dev)
        if r_q.numel() != q:
            raise ValueError(f"{r_q.numel()} targets / means for {q} new rows")
        U2 = torch.cat([cache.U, Uq])
        refactor = (tau.clone(), None if grp0 is None else torch.cat([grp0, grp_q]), torch.cat([r0, r_q]))
        spec = cache.spec

        def from_scratch():
            fresh = _factorize(U2, spec, refactor[0], refactor[1], torch.zeros_like(refactor[2]), refactor[2])
            own = _owned_copy(fresh, n + q, n + q + reserve)
            return _owned_cache(gctx, own, n + q, fresh.alpha, U2, fresh.spec, fresh.jitter, fresh.z, refactor, "refactor")

        if q > min(n, APPEND_MAX_Q):
            return from_scratch()
        cache.refresh()  # (a cache of the shared workspace that another model has factored into since)
        own = cache._own
        if own is not None and own.filled == n and n + q <= own.capacity:
            route = "in_place"
        else:
            own, route = _owned_copy(cache, n, n + q + reserve), "copy"
        with _stage("append_operands"):
            k = gctx.cross_kernel(cache.U, Uq, spec.w, spec.sf2.reshape(1), rows_buffer(n, q, dev), kind=spec.kind,
                                  d_split=spec.d_split)  # N x q
            C = square_buffer(q, dev)
            gctx.kernel_build(Uq, spec.w, spec.sf2.reshape(1), tau, grp_q, C, jitter=cache.jitter, kind=spec.kind,
                              d_split=spec.d_split, uplo=UPLO_UPPER)
        z = torch.empty(n + q, dtype=torch.float64, device=dev)
        alpha = torch.empty(n + q, dtype=torch.float64, device=dev)
        z[:n].copy_(cache.z)
        alpha[:n].copy_(cache.alpha)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        with _stage("chol_append"):
            gctx.chol_append(own.A, own.Linv, n, q, k, C, r_q, z, alpha, info)
        if int(info.item()) != 0:  # (the windows are untouched and ``filled`` stays: the pair serves the next attempt)
            return from_scratch()
        own.filled = n + q
        return _owned_cache(gctx, own, n + q, alpha, U2, spec, cache.jitter, z, refactor, route)


@torch.no_grad()
def loo_moments(cache: FactorCache, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Leave-one-out predictive mean and variance of every training target from a factor cache, O(N^2): mu_i = y_i - alpha_i / d_i,
    s2_i = 1 / d_i with d = diag(Ky^-1) read off the rows of ``cache.Linv`` (gpp_loo_scalars) — no LAUUM, no N x N scratch."""
    cache.refresh()  # another model of the same size may have factored into the shared workspace since
    dev = cache.U.device
    N = cache.U.shape[0]
    with torch.cuda.device(dev):
        d, mu, s2 = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3))
        cache.gctx.loo_scalars(cache.Linv, cache.alpha, _as_f64(y.reshape(-1), dev), d, mu=mu, s2=s2)
    return mu, s2


@torch.no_grad()
def cv_moments(cache: FactorCache, y: torch.Tensor, folds) -> Tuple[torch.Tensor, torch.Tensor]:
    """Held-out predictive mean and variance of every training target under the folds (an int k, labels or a ``cv.FoldIndex``) from a
    factor cache: mu_F = y_F - P_FF^-1 alpha_F, s2_F = diag(P_FF^-1), in the original row order.  The per-bucket batched fold solves
    of ``cv.fold_solves`` on the cached inverse factor: no LAUUM, no N x N scratch, O(N sum m_F^2)."""
    from .cv import FoldIndex, check_infos, fold_solves
    folds = FoldIndex.make(folds, cache.U.shape[0])
    cache.refresh()
    dev = cache.U.device
    with torch.cuda.device(dev):
        a, d, _, infos, _ = fold_solves(cache.gctx, cache.Linv, cache.alpha, folds)
        check_infos(infos, folds)
        mu = _as_f64(y.reshape(-1), dev) + a
    return mu, d


@torch.no_grad()
def predict_from_cache(cache: FactorCache, Us: torch.Tensor, need_var: bool = True, need_V: bool = False, V=None):
    """K8: mean contribution K_*N alpha and prior-minus-explained variance; optionally V = K_*N Linv^T.
    Mean only: the [test][train] cross block and one row reduction, O(M N).  With the variance: the TRANSPOSED cross block, so that
    V = Kns^T Linv^T is the row-contiguous TN product (gpp_predict_tn), and both outputs come from one pass over V.
    ``V``: an M x N window of the caller's own buffer to receive V (``variance_reduction`` keeps spare columns behind it)."""
    dev = Us.device
    gctx = cache.gctx
    M, N = Us.shape[0], cache.U.shape[0]
    mean = torch.empty(M, dtype=torch.float64, device=dev)
    if not (need_var or need_V):
        Ksn = cross_kernel(Us, cache.U, cache.spec)
        gctx.predict(cache.Linv, cache.alpha, Ksn, None, None, mean, None)
        return mean, None, None
    Kns = cross_kernel(cache.U, Us, cache.spec)  # N x M
    if V is None:
        V = rows_buffer(M, N, dev)
    kss = cache.spec.sf2.reshape(1).expand(M).contiguous()
    var = torch.empty(M, dtype=torch.float64, device=dev)
    gctx.predict_tn(cache.Linv, cache.z, Kns, kss, V, mean, var)
    return mean, var, V


#: Operand form ``variance_reduction`` hands gpp_post_cross_sq: False = V as ``predict_from_cache`` leaves it (points x K, the NT
#: tile body), True = V^T (K x points, the row-contiguous TN body; one extra transposition of each V, O(M N)).  MEASURED
#: (tools/bench_alc.py, N = 20 000, M_c = M_r = 4096 / 16384): the fused launch takes 16.7 / 267.6 ms on V and 9.3 / 148.9 ms on V^T,
#: and a q = 16 greedy run with everything included 358 ms against 232 ms at 4096: V^T, as gpp_predict_tn found for the prediction.
ALC_TRANSPOSED = True


def _operand_V(cache, Us, transposed: bool, Kmax: Optional[int] = None):
    """(V or V^T, latent variance) of the latent f at the feature rows ``Us``: the operand of gpp_post_cross_sq / _lin_sq / _min, in
    a buffer with room for ``Kmax`` coordinates per point (``transposed``: Kmax x points, else points x Kmax; None: the K it holds).
    ``cache``: a ``FactorCache`` (K = N, V = K_*N Linv^T of ``predict_from_cache``) or a ``GradientFactorCache`` (K = N + q,
    gpp_predict_tn on ``_gek_function_operand``)."""
    dev, gctx, M = Us.device, cache.gctx, Us.shape[0]
    is_g = isinstance(cache, GradientFactorCache)
    K = cache.U.shape[0] + (cache.q if is_g else 0)
    Kmax = K if Kmax is None else Kmax
    V = rows_buffer(M, K if transposed else Kmax, dev)
    if is_g:
        mean = torch.empty(M, dtype=torch.float64, device=dev)
        var = torch.empty(M, dtype=torch.float64, device=dev)
        gctx.predict_tn(cache.Linv, cache.z, _gek_function_operand(cache, Us), cache.spec.sf2.reshape(1).expand(M).contiguous(),
                        V[:, :K], mean, var)
    else:
        _, var, _ = predict_from_cache(cache, Us, need_V=True, V=V[:, :K])
    if not transposed:
        return V, var
    Vt = rows_buffer(Kmax, M, dev)
    gctx.transpose(V, Vt[:K])
    return Vt, var


def _per_row(what: str, t, n: int, noun: str, rows: str, dev) -> torch.Tensor:
    """``t`` as a contiguous fp64 vector on ``dev`` with one of ``noun`` for each of the ``n`` ``rows``."""
    t = _as_f64(t.detach().reshape(-1), dev)
    if t.numel() != n:
        raise ValueError(f"{what}: {t.numel()} {noun} for {n} {rows}")
    return t


def _score_points(what: str, cache, Uc, Ur, q: int = 1):
    """The first input checks of the four score functions: (Uc, Ur) on the cache's device, fp64 and contiguous, each at least one
    row of the cache's D features, and 1 <= q <= M_c."""
    dev, D = cache.U.device, cache.U.shape[1]
    Uc, Ur = _as_f64(Uc.detach(), dev).contiguous(), _as_f64(Ur.detach(), dev).contiguous()
    for U, name in ((Uc, "candidates"), (Ur, "reference points")):
        if U.dim() != 2 or U.shape[0] < 1 or U.shape[1] != D:
            raise ValueError(f"{what}: the {name} must be at least one row of {D} features (got {tuple(U.shape)})")
    if q < 1 or q > Uc.shape[0]:
        raise ValueError(f"{what}: q must be between 1 and the number of candidates ({Uc.shape[0]}); got {q}")
    return Uc, Ur


def _alc_common(what: str, cache, Uc, tau_c, Ur, omega, q: int = 1):
    """The input checks of the three variance-reduction scores: ``_score_points``, then (tau_c, omega) as fp64 vectors of M_c and M_r
    on the cache's device.  ``omega`` None: 1 / M_r each."""
    Uc, Ur = _score_points(what, cache, Uc, Ur, q)
    dev, Mr = Uc.device, Ur.shape[0]
    tau_c = _per_row(what, tau_c, Uc.shape[0], "noise levels", "candidates", dev)
    if omega is None:
        omega = torch.full((Mr,), 1.0 / Mr, dtype=torch.float64, device=dev)
    else:
        omega = _per_row(what, omega, Mr, "weights", "reference points", dev)
    return Uc, tau_c, Ur, omega


@contextmanager
def _score_call(what: str, cache):
    """What every score function runs under: refused under ``settings.sharded_evaluation``, the cache's GPU current, refused inside a
    graph capture."""
    _gradient_cache_refusals(what)
    dev = cache.U.device  # (anything but a GPU only under a stand-in context: the library itself has no CPU path)
    with torch.cuda.device(dev) if dev.type == "cuda" else nullcontext():
        _gradient_cache_refusals(what, dev)
        yield


def _greedy_picks(stage: str, cache: FactorCache, Uc, tau_c, Ur, q: int, cost, transposed: bool, score):
    """The greedy rounds of ``variance_reduction`` (``stage`` "alc") and ``knowledge_gradient`` ("kg"): both operands with q - 1 spare
    coordinates, then per round the candidates' M_c scores ``score(K, s, Vc, Vr)`` — K = N + t coordinates, s the variance of an
    observation at each candidate, Vc / Vr the K-coordinate windows of the operands —, the pick by score (by score / ``cost``) among
    the rows not yet taken, and the coordinate the pick appends to every point.  Returns (the first round's scores, the picked rows
    in pick order, their undivided scores)."""
    dev, N, Mc = cache.U.device, cache.U.shape[0], Uc.shape[0]
    with _stage(stage + "_operands"):
        (Vc, var_c), (Vr, _) = (_operand_V(cache, U, transposed, N + q - 1) for U in (Uc, Ur))
    Ucr = torch.cat([Uc, Ur]) if q > 1 else None
    taken = torch.zeros(Mc, dtype=torch.bool, device=dev)
    picks, gains, first = [], [], None
    for t in range(q):
        K = N + t
        s = var_c.clamp_min(0.0) + tau_c + cache.jitter
        dv = score(K, s, Vc[:K] if transposed else Vc[:, :K], Vr[:K] if transposed else Vr[:, :K])
        if t == 0:
            first = dv.clone()
        rank = (dv if cost is None else dv / cost).masked_fill(taken, float("-inf"))
        j = int(torch.argmax(rank))
        picks.append(j)
        gains.append(dv[j])
        taken[j] = True
        if t + 1 == q:
            break
        # the new coordinate of every point: c(x, x_j) / sqrt(s_j), c by the current (N + t)-long vectors
        with _stage(stage + "_append"):
            var_c = _append_pick_coordinate(cache, Ucr, Uc, j, s[j], Vc, Vr, K, var_c, transposed)
    return first, torch.tensor(picks, dtype=torch.int64, device=dev), torch.stack(gains)


def _append_pick_coordinate(cache: FactorCache, Ucr, Uc, j: int, s_j, Vc, Vr, K: int, var_c, transposed: bool):
    """Coordinate K of every candidate and reference point after candidate j has been picked: c(x, x_j) / sqrt(s_j), c by the current
    K-long vectors, written in place behind them.  Returns the candidates' reduced latent variance."""
    dev, gctx, spec = cache.U.device, cache.gctx, cache.spec
    Mc = Uc.shape[0]
    Mr = Ucr.shape[0] - Mc
    col = gctx.cross_kernel(Ucr, Uc[j:j + 1], spec.w, spec.sf2.reshape(1), rows_buffer(Mc + Mr, 1, dev), kind=spec.kind,
                            d_split=spec.d_split)
    if transposed:
        vj = rows_buffer(K, 1, dev)
        vj.copy_(Vc[:K, j:j + 1])
        gctx.gemm(1, 0, Mc, 1, K, -1.0, Vc[:K], vj, 1.0, col[:Mc])
        gctx.gemm(1, 0, Mr, 1, K, -1.0, Vr[:K], vj, 1.0, col[Mc:])
    else:
        vj = Vc[j:j + 1, :K]
        gctx.gemm(0, 1, Mc, 1, K, -1.0, Vc[:, :K], vj, 1.0, col[:Mc])
        gctx.gemm(0, 1, Mr, 1, K, -1.0, Vr[:, :K], vj, 1.0, col[Mc:])
    col.div_(s_j.sqrt())
    if transposed:
        Vc[K].copy_(col[:Mc, 0])
        Vr[K].copy_(col[Mc:, 0])
    else:
        Vc[:, K].copy_(col[:Mc, 0])
        Vr[:, K].copy_(col[Mc:, 0])
    return var_c - col[:Mc, 0] ** 2


@torch.no_grad()
def variance_reduction(cache: FactorCache, Uc, tau_c, Ur, omega=None, q: int = 1, cost=None, transposed: Optional[bool] = None):
    """Expected reduction of the omega-weighted posterior variance of the latent f over the reference features ``Ur`` (M_r x D) from
    ONE noisy observation at each candidate ``Uc`` (M_c x D; ``tau_c``: the candidates' own noise levels, M_c), and a greedy batch of
    ``q`` of them.  With v(x) = Linv k(X, x) and c(x, x') = sf2 k(x, x') - v(x)^T v(x'):
        dV(c) = sum_r omega_r c(x_r, x_c)^2 / s_c,    s_c = max(c(x_c, x_c), 0) + tau_c + jitter  (the diagonal ``append_to_cache`` uses)
    whatever the observed value.  The M_c x M_r block of c never exists: the sums come from gpp_post_cross_sq on the V of
    ``predict_from_cache``.  After a pick j every point gains the coordinate c(x, x_j) / sqrt(s_j) (one ``cross_kernel`` column and two
    matrix-vector products, O((M_c + M_r)(N + t))), appended in place to buffers with q - 1 spare columns; the kernel then runs with
    K = N + t.  The q gains add up to the reduction from conditioning on all q picks at once.  A picked candidate is excluded from
    later rounds; with ``cost`` (M_c positive numbers) the pick maximises gain / cost and the reported gains stay undivided.
    ``omega`` None: 1 / M_r each.  Returns (the M_c first-round scores, the q picked rows of ``Uc`` in pick order, their gains), in
    the cache's (scaled-target) units.  The cache is only read.  Refused under ``settings.sharded_evaluation`` and inside a graph
    capture, like ``append_to_cache``."""
    what = "variance_reduction"
    q, transposed = int(q), ALC_TRANSPOSED if transposed is None else bool(transposed)
    with _score_call(what, cache):
        gctx, spec = cache.gctx, cache.spec
        Uc, tau_c, Ur, omega = _alc_common(what, cache, Uc, tau_c, Ur, omega, q)
        Mc, dev = Uc.shape[0], Uc.device
        if cost is not None:
            cost = _per_row(what, cost, Mc, "costs", "candidates", dev)
        cache.refresh()  # (a cache of the shared workspace that another model has factored into since)
        num = torch.empty(Mc, dtype=torch.float64, device=dev)

        def score(K, s, Vc, Vr):
            with _stage("post_cross_sq"):
                gctx.post_cross_sq(Uc, Ur, spec.w, spec.sf2.reshape(1), Vc, Vr, K, num, omega=omega, kind=spec.kind,
                                   d_split=spec.d_split, transposed=transposed)
            return num / s

        return _greedy_picks("alc", cache, Uc, tau_c, Ur, q, cost, transposed, score)


#: Most bytes the derivative cross block Dk and the product Q = Dk^T Linv^T of ONE chunk of ``gradient_from_cache`` may take, each:
#: the test points go in chunks of as many points as fit (at least one).  At N = 20 000 and nd = 8 that is 209 points per chunk.
GRAD_CHUNK_BYTES = 256 << 20


def _curvature_coefficients(spec: KernelSpec) -> torch.Tensor:
    """c_d of ``gradient_prior_curvature`` for all D features: 2 on the RBF factor, 6 (Matern 3/2) or 10 / 3 (Matern 5/2) behind."""
    D = spec.w.numel()
    split = D if spec.kind == KIND_RBF else int(spec.d_split)
    c = torch.full((D,), 2.0, dtype=torch.float64, device=spec.w.device)
    if spec.kind != KIND_RBF:
        c[split:] = 6.0 if spec.kind == KIND_MATERN32 else 10.0 / 3.0
    return c


def gradient_prior_curvature(spec: KernelSpec, d0: int, nd: int) -> torch.Tensor:
    """kappa_j = d^2 (sf2 k) / du_j du'_j at u' = u for the features d0 .. d0 + nd - 1: c_j w_j sf2 with c_j = 2 on a feature of
    the RBF factor, 6 on a Matern-3/2 and 10 / 3 on a Matern-5/2 feature (h'(0) = -3 and -5 / 3 of the Matern factor h(r),
    r^2 = 2 nu 2 sum_d w_d delta_d^2): the prior variance of the gradient's components, which are uncorrelated a priori."""
    return (_curvature_coefficients(spec) * spec.w.reshape(-1) * spec.sf2.reshape(()))[d0:d0 + nd]


def _gradient_chunk_points(N: int, nd: int) -> int:
    per_point = 8 * nd * row_stride(N)
    mc = max(1, GRAD_CHUNK_BYTES // per_point)
    while mc > 1 and 8 * N * row_stride(mc * nd) > GRAD_CHUNK_BYTES:
        mc -= 1
    return mc


@torch.no_grad()
def gradient_from_cache(cache: FactorCache, Us, d0: int, nd: int, want: str, omega=None):
    """Posterior of the gradient of the latent f with respect to the features d0 .. d0 + nd - 1 at the feature rows ``Us`` (M x D):
    grad f(x_a) | data ~ N(g_a, S_a) with, for Dk[n, (a, j)] = d/du_{d0+j} sf2 k(u_a, U_n) and Q = Dk^T Linv^T,
        g_a = Q_a z = Dk_a^T alpha,        S_a = diag(kappa) - Q_a Q_a^T        (kappa: ``gradient_prior_curvature``).
    No observation noise enters: noise has no derivative.  ``want``:
      "mean"  g (M x nd) alone, by ONE gpp_kernel_apply_grad call (C = alpha, Gbar = 1), O(M N): no block is formed;
      "std"   (g, var): the diagonal of S (M x nd), unclamped;
      "cov"   (g, S): M x nd x nd, bitwise symmetric;
      "sum"   (sum_a omega_a g_a g_a^T, sum_a omega_a S_a), nd x nd each: the two parts of the active-subspace matrix, without
              storing per-point matrices; ``omega``: M weights, None for 1 / M each.
    For the last three the points go in chunks whose Dk and Q stay within ``GRAD_CHUNK_BYTES`` each; per chunk gpp_cross_kernel_dx
    writes Dk, gpp_predict_tn (kss = kappa tiled per point) gives Q, g and the variance diagonal from the product every prediction
    uses, and gpp_point_gram reduces Q to the per-point Gram matrices or their weighted sum; the sums of "sum" add up in chunk
    order.  For nd > 16 (beyond gpp_point_gram) the Gram matrices come from ``torch.bmm`` on the chunk's Q.  Everything is in the
    cache's (scaled-target) units.  The cache is only read (and refreshed when another model has taken the shared workspace).
    Refused under ``settings.sharded_evaluation`` and inside a graph capture, like ``variance_reduction``."""
    if want not in ("mean", "std", "cov", "sum"):
        raise ValueError(f"want must be 'mean', 'std', 'cov' or 'sum' (got {want!r})")
    if settings.sharded_evaluation.value() is not None:
        raise NotImplementedError("gradient_from_cache is not available under settings.sharded_evaluation")
    dev = cache.U.device
    gctx = cache.gctx
    on_gpu = dev.type == "cuda"  # (anything else only under a stand-in context: the library itself has no CPU path)
    with torch.cuda.device(dev) if on_gpu else nullcontext():
        if on_gpu and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("gradient_from_cache is not available inside a graph capture")
        Us = _as_f64(Us.detach(), dev).contiguous()
        N, D = cache.U.shape
        d0, nd = int(d0), int(nd)
        if Us.dim() != 2 or Us.shape[0] < 1 or Us.shape[1] != D:
            raise ValueError(f"the test points must be at least one row of {D} features (got {tuple(Us.shape)})")
        if nd < 1 or d0 < 0 or d0 + nd > D:
            raise ValueError(f"the differentiated features [{d0}, {d0 + nd}) must be a non-empty range of the {D} features")
        M = Us.shape[0]
        if want == "sum":
            if omega is None:
                omega = torch.full((M,), 1.0 / M, dtype=torch.float64, device=dev)
            else:
                omega = _as_f64(omega.detach().reshape(-1), dev).contiguous()
                if omega.numel() != M:
                    raise ValueError(f"{omega.numel()} weights for {M} test points")
        cache.refresh()  # (a cache of the shared workspace that another model has factored into since)
        spec = cache.spec
        w, sf2 = spec.w, spec.sf2.reshape(1)
        if want == "mean":
            g = torch.empty((M, D), dtype=torch.float64, device=dev)
            with _stage("grad_mean"):
                gctx.kernel_apply_grad(Us, cache.U, w, sf2, cache.alpha.reshape(-1, 1), torch.ones((M, 1), dtype=torch.float64, device=dev),
                                       g, kind=spec.kind, d_split=spec.d_split)
            return g[:, d0:d0 + nd].contiguous()
        kappa = gradient_prior_curvature(spec, d0, nd)
        mean = torch.empty((M, nd), dtype=torch.float64, device=dev)
        var = torch.empty((M, nd), dtype=torch.float64, device=dev) if want == "std" else None
        cov = torch.empty((M, nd, nd), dtype=torch.float64, device=dev) if want == "cov" else None
        if want == "sum":
            mean_part = torch.zeros((nd, nd), dtype=torch.float64, device=dev)
            cov_part = torch.zeros((nd, nd), dtype=torch.float64, device=dev)
        step = _gradient_chunk_points(N, nd)
        for a0 in range(0, M, step):
            mc = min(step, M - a0)
            Dk = rows_buffer(N, mc * nd, dev)
            Q = rows_buffer(mc * nd, N, dev)
            g_c = torch.empty(mc * nd, dtype=torch.float64, device=dev)
            v_c = torch.empty(mc * nd, dtype=torch.float64, device=dev)
            with _stage("cross_kernel_dx"):
                gctx.cross_kernel_dx(Us[a0:a0 + mc], cache.U, w, sf2, d0, nd, Dk, kind=spec.kind, d_split=spec.d_split)
            with _stage("grad_predict_tn"):
                gctx.predict_tn(cache.Linv, cache.z, Dk, kappa.repeat(mc), Q, g_c, v_c)
            del Dk
            g_c = g_c.view(mc, nd)
            mean[a0:a0 + mc] = g_c
            if want == "std":
                var[a0:a0 + mc] = v_c.view(mc, nd)
                continue
            with _stage("point_gram"):
                if nd <= 16:
                    if want == "cov":
                        G = torch.empty((mc, nd, nd), dtype=torch.float64, device=dev)
                        gctx.point_gram(Q, nd, G=G)
                    else:
                        Gsum = torch.empty((nd, nd), dtype=torch.float64, device=dev)
                        gctx.point_gram(Q, nd, Gsum=Gsum, omega=omega[a0:a0 + mc])
                else:
                    Q3 = Q.unflatten(0, (mc, nd))
                    G = torch.bmm(Q3, Q3.transpose(1, 2))
                    G = 0.5 * (G + G.transpose(1, 2))
                    if want == "sum":
                        Gsum = (omega[a0:a0 + mc, None, None] * G).sum(0)
            if want == "cov":
                cov[a0:a0 + mc] = torch.diag(kappa) - G
            else:
                om = omega[a0:a0 + mc]
                mean_part += (g_c * om[:, None]).T @ g_c
                cov_part += om.sum() * torch.diag(kappa) - Gsum
        if want == "std":
            return mean, var
        if want == "cov":
            return mean, cov
        return 0.5 * (mean_part + mean_part.T), cov_part


class GradientFactorCache:
    """Factor, inverse factor, z and alpha of the N function rows of a ``FactorCache`` bordered with q = Mg nd gradient observations
    (``append_gradients_to_cache``): row N + a nd + j is d f / du_{d0+j} at the feature row ``Ug[a]``.  With a selection ``sel``
    (``backend.GradientSelection``: partial gradients) q = sel.q and row N + k is its observation k, the direction sel.dir[k] at the
    point that owns k.  It owns its matrices (never stale) and is deliberately NOT a ``FactorCache``: its last q rows are not
    function values, so nothing that reads a ``FactorCache`` (prediction, appends, scores, sampling) may take it.  Its consumers
    are ``predict_from_gradient_cache``, ``variance_reduction_from_gradient_cache`` (plain ALC from the gradient-enhanced posterior)
    and ``variance_reduction_block`` (the score of a run that returns y and gradient components), which build their (N + q)-row
    operands with the same helpers (``_gek_function_operand``, ``_gek_gradient_tail``)."""

    def __init__(self, gctx, own, n, q, z, alpha, U, Ug, d0, nd, spec, jitter, sel=None):
        self.gctx, self._own = gctx, own
        self.L, self.Linv = own.A[:n + q, :n + q], own.Linv[:n + q, :n + q]
        self.z, self.alpha, self.U, self.Ug, self.d0, self.nd, self.spec, self.jitter = z, alpha, U, Ug, d0, nd, spec, jitter
        self.q, self.sel = q, sel


def _gradient_cache_refusals(what: str, dev=None):
    if settings.sharded_evaluation.value() is not None:
        raise NotImplementedError(f"{what} is not available under settings.sharded_evaluation")
    if dev is not None and dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise NotImplementedError(f"{what} is not available inside a graph capture")


@torch.no_grad()
def append_gradients_to_cache(cache: FactorCache, Ug, d0: int, nd: int, r_g, noise_diag, sel=None) -> GradientFactorCache:
    """A ``GradientFactorCache`` of the N cached rows plus q = Mg nd observations of the gradient of the latent f with respect to
    the features d0 .. d0 + nd - 1 at the feature rows ``Ug`` (Mg x D), in O(N^2 q) by bordering the cached factor (gpp_chol_append):
    the cross block is cov(f(x_n), d_j f(ug_a)) = gpp_cross_kernel_dx(Ua = Ug, Ub = U) (N x q), the corner
    cov(d_j f(ug_a), d_l f(ug_b)) = gpp_kernel_dxdx(Ug, Ug) plus diag(noise_diag + the cache's jitter).  ``r_g``: the q observed
    gradients, point-major (a nd + j), in the cache's scaled units — every supported mean is constant, so their prior mean is 0;
    ``noise_diag``: their q noise variances, same units squared.  The windows are always copied into a new pair of capacity
    N + q: ``cache`` stays valid and bitwise unchanged (it is refreshed first when another model has taken the shared workspace).
    ``sel``: a ``backend.GradientSelection`` of the (point, direction) entries that were observed; q = sel.q, ``r_g`` and
    ``noise_diag`` hold those q entries in its order, and both blocks are built at their compact size by the ``_sel`` kernels.

    ``ValueError`` for q > min(N, APPEND_MAX_Q): there is no from-scratch route, since no build kernel forms the mixed matrix.
    ``errors.NotPSDError`` when the Schur complement is not positive definite (duplicate gradient points without noise).
    Refused under ``settings.sharded_evaluation`` and inside a graph capture, like ``append_to_cache``."""
    from .errors import NotPSDError

    _gradient_cache_refusals("appending gradients to a factor cache")
    dev = cache.U.device
    gctx = cache.gctx
    on_gpu = dev.type == "cuda"  # (anything else only under a stand-in context: the library itself has no CPU path)
    with torch.cuda.device(dev) if on_gpu else nullcontext():
        _gradient_cache_refusals("appending gradients to a factor cache", dev)
        n, D = cache.U.shape
        d0, nd = int(d0), int(nd)
        Ug = _as_f64(Ug.detach(), dev).contiguous()
        if Ug.dim() != 2 or Ug.shape[0] < 1 or Ug.shape[1] != D:
            raise ValueError(f"the gradient points must be at least one row of {D} features (got {tuple(Ug.shape)})")
        if nd < 1 or d0 < 0 or d0 + nd > D:
            raise ValueError(f"the differentiated features [{d0}, {d0 + nd}) must be a non-empty range of the {D} features")
        if sel is not None and (sel.num_points, sel.nd) != (Ug.shape[0], nd):
            raise ValueError(f"a selection of {sel.num_points} points x {sel.nd} directions for {Ug.shape[0]} x {nd}")
        q = Ug.shape[0] * nd if sel is None else sel.q
        r_g = _as_f64(r_g.detach().reshape(-1), dev).contiguous()
        noise_diag = _as_f64(noise_diag.detach().reshape(-1), dev)
        if r_g.numel() != q or noise_diag.numel() != q:
            raise ValueError(f"{r_g.numel()} gradients / {noise_diag.numel()} noise variances for {q} gradient observations")
        if q > min(n, APPEND_MAX_Q):
            raise ValueError(f"{q} gradient observations exceed min(N = {n}, {APPEND_MAX_Q}): the factor can only be bordered, "
                             "no build kernel forms the mixed function / gradient matrix from scratch")
        cache.refresh()  # (a cache of the shared workspace that another model has factored into since)
        own = _owned_copy(cache, n, n + q)
        spec = cache.spec
        w, sf2 = spec.w, spec.sf2.reshape(1)
        with _stage("append_gradient_operands"):
            k = gctx.cross_kernel_dx(Ug, cache.U, w, sf2, d0, nd, rows_buffer(n, q, dev), kind=spec.kind, d_split=spec.d_split,
                                     sel=sel)
            C = gctx.kernel_dxdx(Ug, Ug, w, sf2, d0, nd, square_buffer(q, dev), kind=spec.kind, d_split=spec.d_split, sel_a=sel,
                                 sel_b=sel)
            C.diagonal().add_(noise_diag + cache.jitter)
        z = torch.empty(n + q, dtype=torch.float64, device=dev)
        alpha = torch.empty(n + q, dtype=torch.float64, device=dev)
        z[:n].copy_(cache.z)
        alpha[:n].copy_(cache.alpha)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        with _stage("chol_append"):
            gctx.chol_append(own.A, own.Linv, n, q, k, C, r_g, z, alpha, info)
        minor = int(info.item())
        if minor == 0:
            # A Schur complement that is singular in exact arithmetic (the same gradient observed twice without noise) may still
            # factor, on a pivot that is rounding noise of either sign.  S_kk = C_kk - |V_k|^2 is formed from N + q products of size
            # up to C_kk: a squared pivot within 4 (N + q) u of C_kk has no digit left and counts as not positive.  (The default
            # nugget keeps S_kk >= 1e-6 C_kk / (1 + 1e-6), five orders above this at N + q = 22 048.)
            piv = own.A[n:n + q, n:n + q].diagonal()
            lost = piv * piv <= (4.0 * (n + q) * 2.0 ** -53) * C.diagonal()
            if bool(lost.any()):
                minor = int(lost.to(torch.int32).argmax().item()) + 1
        if minor != 0:
            entry = minor - 1 if sel is None else int(sel.flat[minor - 1])  # a nd + j of the failing observation
            raise NotPSDError(f"conditioning on gradients: leading minor {minor} of the Schur complement of the {q} gradient "
                              f"observations is not positive definite (gradient point {entry // nd}, direction "
                              f"{entry % nd}); pass a larger noise")
        own.filled = n + q
        return GradientFactorCache(gctx, own, n, q, z, alpha, cache.U, Ug, d0, nd, spec, cache.jitter, sel)


def _gek_function_tail(gcache: "GradientFactorCache", Us) -> torch.Tensor:
    """cov(f(Us_a), gradient observation k) as an M x q matrix: gpp_cross_kernel_dx(Ua = Ug, Ub = Us), the observations of the cache's
    selection as columns (what ``predict_from_gradient_cache`` and ``variance_reduction_block`` transpose into a function column)."""
    spec = gcache.spec
    return gcache.gctx.cross_kernel_dx(gcache.Ug, Us, spec.w, spec.sf2.reshape(1), gcache.d0, gcache.nd,
                                       rows_buffer(Us.shape[0], gcache.q, Us.device), kind=spec.kind, d_split=spec.d_split,
                                       sel=gcache.sel)


def _gek_function_operand(gcache: "GradientFactorCache", Us) -> torch.Tensor:
    """The (N + q) x M operand of gpp_predict_tn for the latent f at ``Us``: rows [0, N) = gpp_cross_kernel(U, Us), rows [N, N + q) =
    ``_gek_function_tail`` transposed."""
    spec, N = gcache.spec, gcache.U.shape[0]
    op = rows_buffer(N + gcache.q, Us.shape[0], Us.device)
    gcache.gctx.cross_kernel(gcache.U, Us, spec.w, spec.sf2.reshape(1), op[:N], kind=spec.kind, d_split=spec.d_split)
    gcache.gctx.transpose(_gek_function_tail(gcache, Us), op[N:])
    return op


def _gek_gradient_tail(gcache: "GradientFactorCache", Us, out, sel_b=None) -> torch.Tensor:
    """cov(gradient observation k, d f / du_{d0+l}(Us_a)) into ``out`` (q x (M nd), or with the selection ``sel_b`` of the test
    side's (point, direction) entries q x sel_b.q): gpp_kernel_dxdx(Ug, Us) on the cache's selection of its own side."""
    spec = gcache.spec
    return gcache.gctx.kernel_dxdx(gcache.Ug, Us, spec.w, spec.sf2.reshape(1), gcache.d0, gcache.nd, out, kind=spec.kind,
                                   d_split=spec.d_split, sel_a=gcache.sel, sel_b=sel_b)


@torch.no_grad()
def predict_from_gradient_cache(gcache: GradientFactorCache, Us, want: str = "function"):
    """Posterior at the feature rows ``Us`` (M x D) from a ``GradientFactorCache``, in the cache's scaled units, by gpp_predict_tn on
    an (N + q)-row operand whose first N rows are what a ``FactorCache`` prediction uses and whose last q rows are the covariances
    with the gradient observations.  ``want``:
      "function"  (mean contribution, variance) of the latent f, M each: rows [0, N) = gpp_cross_kernel(U, Us), rows [N, N + q) =
                  gpp_cross_kernel_dx(Ua = Ug, Ub = Us) (M x q) transposed; the prior mean is not added and the variance is unclamped;
      "gradient"  (mean, variance diagonal) of the gradient with respect to the cache's differentiated features, M x nd each, in
                  chunks of ``GRAD_CHUNK_BYTES`` like ``gradient_from_cache``: rows [0, N) = gpp_cross_kernel_dx(Ua = Us, Ub = U), rows
                  [N, N + q) = gpp_kernel_dxdx(Ug, Us); the prior diagonal is ``gradient_prior_curvature``.
    Refused under ``settings.sharded_evaluation`` and inside a graph capture."""
    if want not in ("function", "gradient"):
        raise ValueError(f"want must be 'function' or 'gradient' (got {want!r})")
    _gradient_cache_refusals("predicting from a gradient cache")
    dev = gcache.U.device
    gctx = gcache.gctx
    on_gpu = dev.type == "cuda"
    with torch.cuda.device(dev) if on_gpu else nullcontext():
        _gradient_cache_refusals("predicting from a gradient cache", dev)
        Us = _as_f64(Us.detach(), dev).contiguous()
        N, D = gcache.U.shape
        if Us.dim() != 2 or Us.shape[0] < 1 or Us.shape[1] != D:
            raise ValueError(f"the test points must be at least one row of {D} features (got {tuple(Us.shape)})")
        M, d0, nd = Us.shape[0], gcache.d0, gcache.nd
        q = gcache.q  # (the test side stays dense: all nd directions at every test point)
        spec = gcache.spec
        w, sf2 = spec.w, spec.sf2.reshape(1)
        if want == "function":
            with _stage("gek_operands"):
                op = _gek_function_operand(gcache, Us)
            mean = torch.empty(M, dtype=torch.float64, device=dev)
            var = torch.empty(M, dtype=torch.float64, device=dev)
            with _stage("gek_predict_tn"):
                gctx.predict_tn(gcache.Linv, gcache.z, op, sf2.expand(M).contiguous(), rows_buffer(M, N + q, dev), mean, var)
            return mean, var
        kappa = gradient_prior_curvature(spec, d0, nd)
        mean = torch.empty((M, nd), dtype=torch.float64, device=dev)
        var = torch.empty((M, nd), dtype=torch.float64, device=dev)
        step = _gradient_chunk_points(N + q, nd)
        for a0 in range(0, M, step):
            mc = min(step, M - a0)
            op = rows_buffer(N + q, mc * nd, dev)
            g_c = torch.empty(mc * nd, dtype=torch.float64, device=dev)
            v_c = torch.empty(mc * nd, dtype=torch.float64, device=dev)
            with _stage("gek_operands"):
                gctx.cross_kernel_dx(Us[a0:a0 + mc], gcache.U, w, sf2, d0, nd, op[:N], kind=spec.kind, d_split=spec.d_split)
                _gek_gradient_tail(gcache, Us[a0:a0 + mc], op[N:])
            with _stage("gek_predict_tn"):
                gctx.predict_tn(gcache.Linv, gcache.z, op, kappa.repeat(mc), rows_buffer(mc * nd, N + q, dev), g_c, v_c)
            del op
            mean[a0:a0 + mc] = g_c.view(mc, nd)
            var[a0:a0 + mc] = v_c.view(mc, nd)
        return mean, var


#: Most bytes each of the chunk-sized buffers of ``variance_reduction_block`` may take (the operand block, V, the whitened V and its
#: transpose; ``GRAD_CHUNK_BYTES`` idiom): the candidates go in chunks of as many as fit, at least one.  MEASURED (tools/
#: bench_alc_gradient.py, N = 20 000, M_c x M_r = 4096 x 4096, all 8 gradient components: b = 9): the whole score takes 1088 / 537 / 415 ms
#: at 64 / 256 / 1024 MiB (46 / 184 / 744 candidates per chunk) — gpp_predict_tn on a chunk's columns 672 / 336 / 257 ms and the fused
#: launch 341 / 144 / 103 ms: both want some thousands of rows per call.  At 1 GiB a call holds about 5 GiB of temporaries.
ALC_GRADIENT_CHUNK_BYTES = 1024 << 20


def _alc_gradient_chunk_points(K: int, b: int) -> int:
    mc = max(1, ALC_GRADIENT_CHUNK_BYTES // (8 * b * row_stride(K)))
    while mc > 1 and 8 * K * row_stride(mc * b) > ALC_GRADIENT_CHUNK_BYTES:
        mc -= 1
    return mc


@torch.no_grad()
def variance_reduction_from_gradient_cache(gcache: GradientFactorCache, Uc, tau_c, Ur, omega=None, transposed: Optional[bool] = None):
    """First-round scores of ``variance_reduction`` (one noisy function value per candidate) from a gradient-enhanced posterior:
    gpp_post_cross_sq on operands of K = N + q coordinates, dV(c) = sum_r omega_r c(x_r, x_c)^2 / (c(x_c, x_c) + tau_c + jitter).
    M_c scores in the cache's scaled units; the cache is only read.  Refused under ``settings.sharded_evaluation`` and inside a graph
    capture."""
    what = "variance_reduction_from_gradient_cache"
    transposed = ALC_TRANSPOSED if transposed is None else bool(transposed)
    with _score_call(what, gcache):
        Uc, tau_c, Ur, omega = _alc_common(what, gcache, Uc, tau_c, Ur, omega)
        spec, K = gcache.spec, gcache.U.shape[0] + gcache.q
        with _stage("alc_operands"):
            (Vc, var_c), (Vr, _) = _operand_V(gcache, Uc, transposed), _operand_V(gcache, Ur, transposed)
        num = torch.empty(Uc.shape[0], dtype=torch.float64, device=Uc.device)
        with _stage("post_cross_sq"):
            gcache.gctx.post_cross_sq(Uc, Ur, spec.w, spec.sf2.reshape(1), Vc, Vr, K, num, omega=omega, kind=spec.kind,
                                      d_split=spec.d_split, transposed=transposed)
        return num / (var_c.clamp_min(0.0) + tau_c + gcache.jitter)


@torch.no_grad()
def variance_reduction_block(cache, Uc, tau_c, gnoise, dirs, Ur, omega=None, transposed: Optional[bool] = None):
    """Expected reduction of the omega-weighted posterior variance of the latent f over ``Ur`` (M_r x D) from ONE run at each candidate
    ``Uc`` (M_c x D) that returns a noisy function value AND noisy gradient components: the b = 1 + p' linear functionals
    l_0 = f(x_c), l_j = d f / du_{dirs[j-1]}(x_c).  With c_r (b) the posterior cross-covariance of f(x_r) with the functionals and S_c
    (b x b) their posterior covariance plus the observation diagonal,
        dV(c) = sum_r omega_r c_r^T S_c^-1 c_r = sum_{i < b} sum_r omega_r (W_c c_r)_i^2,      S_c = L_c L_c^T,  W_c = L_c^-1,
    whatever the observed values.  Row i of W_c is itself a linear functional at x_c, so the b sums of a candidate are b rows of ONE
    gpp_post_cross_lin_sq launch on the whitened explained part W_c V_c: the M_c b x M_r block never exists.

    ``cache``: a ``FactorCache``, or a ``GradientFactorCache`` (the score from a gradient-enhanced posterior, K = N + q coordinates).
    ``dirs``: the observed directions, a strictly increasing list of feature columns (inside the cache's differentiated range
    [d0, d0 + nd) for a ``GradientFactorCache``); one set serves every candidate of a call.  ``tau_c`` (M_c) and ``gnoise`` (M_c x p'):
    the noise variances of the value and of the gradient components;
        S_c = blockdiag(sf2, diag kappa_dirs) - G_c + diag(tau_c + jitter, gnoise + jitter),        G_c = V_c V_c^T,
    the diagonal ``append_to_cache`` and ``append_gradients_to_cache`` add: the score equals what conditioning would do.  Per chunk of
    candidates (``ALC_GRADIENT_CHUNK_BYTES``): the raw operand block ((N or N + q) x (m_c b) columns, candidate-major: the function
    column by ``cross_kernel``, the gradient columns by gpp_cross_kernel_dx on a selection of ``dirs``, the last q rows of a gradient
    cache by the helpers of ``predict_from_gradient_cache``), gpp_predict_tn for V, gpp_point_gram with group size b for G_c (b <= 16;
    ``torch.bmm`` above), a batched Cholesky and triangular inverse on the host side (N m_c b^2 flops for W_c V_c against
    N^2 m_c b for V), the transposition under ``ALC_TRANSPOSED``, one fused launch, and the sum of each candidate's b rows.  The
    reference operand V_r is computed once.

    Returns (the M_c scores of the run with gradients, the M_c scores of the value alone: row 0 of each block, the first-round score
    of ``variance_reduction``), in the cache's scaled units.  ``errors.NotPSDError`` when a candidate's S_c is not positive definite
    (it names the candidate): pass more noise.  The cache is only read.  Refused under ``settings.sharded_evaluation`` and inside a
    graph capture, like ``variance_reduction``."""
    from .backend import GradientSelection
    from .errors import NotPSDError

    what = "variance_reduction_block"
    transposed = ALC_TRANSPOSED if transposed is None else bool(transposed)
    with _score_call(what, cache):
        is_g = isinstance(cache, GradientFactorCache)
        dev, gctx = cache.U.device, cache.gctx
        Uc, tau_c, Ur, omega = _alc_common(what, cache, Uc, tau_c, Ur, omega)
        (N, D), Mc = cache.U.shape, Uc.shape[0]
        dirs = [int(d) for d in dirs]
        lo, hi = (cache.d0, cache.d0 + cache.nd) if is_g else (0, D)
        if len(dirs) < 1 or any(b <= a for a, b in zip(dirs, dirs[1:])) or dirs[0] < lo or dirs[-1] >= hi:
            raise ValueError(f"{what}: dirs must be a strictly increasing, non-empty list of feature columns in [{lo}, {hi}) "
                             f"(got {dirs})")
        pn = len(dirs)
        b = 1 + pn
        gnoise = _as_f64(gnoise.detach(), dev)
        if gnoise.shape != (Mc, pn):
            raise ValueError(f"{what}: gnoise must be ({Mc}, {pn}): one variance per candidate and observed direction "
                             f"(got {tuple(gnoise.shape)})")
        if not is_g:
            cache.refresh()  # (a cache of the shared workspace that another model has factored into since)
        spec = cache.spec
        w, sf2 = spec.w, spec.sf2.reshape(1)
        K = N + (cache.q if is_g else 0)
        # the derivative kernels' range and the selection of dirs inside it; the fused launch's range is the span of dirs
        dd0, dnd = (cache.d0, cache.nd) if is_g else (dirs[0], dirs[-1] - dirs[0] + 1)
        k0, kn = dirs[0], dirs[-1] - dirs[0] + 1
        row_mask = torch.zeros(dnd, dtype=torch.bool)
        row_mask[[d - dd0 for d in dirs]] = True
        acol = torch.tensor([1 + d - k0 for d in dirs], dtype=torch.int64, device=dev)
        prior = torch.cat([sf2, gradient_prior_curvature(spec, 0, D)[torch.tensor(dirs, dtype=torch.int64, device=dev)]])
        noise = torch.cat([tau_c.reshape(-1, 1), gnoise], 1) + cache.jitter
        with _stage("alc_operands"):
            Vr, _ = _operand_V(cache, Ur, transposed)
        with_g = torch.empty(Mc, dtype=torch.float64, device=dev)
        value = torch.empty(Mc, dtype=torch.float64, device=dev)
        step = _alc_gradient_chunk_points(K, b)
        for a0 in range(0, Mc, step):
            mc = min(step, Mc - a0)
            Ux = Uc[a0:a0 + mc]
            selc = None if pn == dnd else GradientSelection(row_mask.expand(mc, dnd).contiguous(), dev)
            with _stage("alc_gradient_operands"):
                op = rows_buffer(K, mc * b, dev)
                o3 = op.unflatten(1, (mc, b))  # candidate-major columns: (value, dirs) of each candidate side by side
                o3[:N, :, 0] = cross_kernel(cache.U, Ux, spec)
                Dk = gctx.cross_kernel_dx(Ux, cache.U, w, sf2, dd0, dnd, rows_buffer(N, mc * pn, dev), kind=spec.kind,
                                          d_split=spec.d_split, sel=selc)
                o3[:N, :, 1:] = Dk.unflatten(1, (mc, pn))
                del Dk
                if is_g:
                    o3[N:, :, 0] = _gek_function_tail(cache, Ux).T
                    o3[N:, :, 1:] = _gek_gradient_tail(cache, Ux, rows_buffer(cache.q, mc * pn, dev), selc).unflatten(1, (mc, pn))
            V = rows_buffer(mc * b, K, dev)
            mean = torch.empty(mc * b, dtype=torch.float64, device=dev)
            var = torch.empty(mc * b, dtype=torch.float64, device=dev)
            with _stage("alc_gradient_predict_tn"):
                gctx.predict_tn(cache.Linv, cache.z, op, prior.repeat(mc), V, mean, var)
            del op
            V3 = V.unflatten(0, (mc, b))
            with _stage("alc_gradient_whiten"):
                if b <= 16:
                    G = torch.empty((mc, b, b), dtype=torch.float64, device=dev)
                    gctx.point_gram(V, b, G=G)
                else:
                    G = torch.bmm(V3, V3.transpose(1, 2))
                    G = 0.5 * (G + G.transpose(1, 2))
                S = torch.diag_embed(prior + noise[a0:a0 + mc]) - G
                Lc, info = torch.linalg.cholesky_ex(S)
                if bool((info != 0).any()):
                    j = int((info != 0).to(torch.int32).argmax())
                    raise NotPSDError(f"{what}: the covariance of the value and the {pn} gradient components at candidate {a0 + j} is "
                                      f"not positive definite (leading minor {int(info[j])}); pass a larger gradient noise")
                W = torch.linalg.solve_triangular(Lc, torch.eye(b, dtype=torch.float64, device=dev).expand(mc, b, b), upper=False)
                Vw = rows_buffer(mc * b, K, dev)
                Vw.unflatten(0, (mc, b)).copy_(torch.bmm(W, V3))
                del V, V3
                if transposed:
                    Vf = rows_buffer(K, mc * b, dev)
                    gctx.transpose(Vw, Vf)
                    del Vw
                else:
                    Vf = Vw
                A = torch.zeros((mc, b, 1 + kn), dtype=torch.float64, device=dev)
                A[:, :, 0] = W[:, :, 0]
                A[:, :, acol] = W[:, :, 1:]
            num = torch.empty(mc * b, dtype=torch.float64, device=dev)
            with _stage("post_cross_lin_sq"):
                gctx.post_cross_lin_sq(Ux.repeat_interleave(b, 0), Ur, w, sf2, A.view(mc * b, 1 + kn), k0, kn, Vf, Vr, K, num, omega=omega,
                                       kind=spec.kind, d_split=spec.d_split, transposed=transposed)
            num = num.view(mc, b)
            with_g[a0:a0 + mc] = num.sum(1)
            value[a0:a0 + mc] = num[:, 0]
        return with_g, value


# ---------------------------------------------------------------------------------------------------
# training on gradient observations: the joint log-likelihood of [y; grad y], factored from scratch
# ---------------------------------------------------------------------------------------------------
class ExactGEKFunction(torch.autograd.Function):
    """log N([y - mean; r_g] | 0, Kj) of N function rows U and q = Mg nd gradient observations at the rows Ug,
        Kj = [[sf2 k(U, U) + diag(tau[grp]), Kfg], [Kfg^T, Kgg + diag(nu)]],
    Kfg = gpp_cross_kernel_dx(Ua = Ug, Ub = U) (N x q), Kgg = gpp_kernel_dxdx(Ug, Ug), rows point-major as in
    ``append_gradients_to_cache``; with gradients for U[:, :dU], Ug[:, :dU], w, sf2, tau, mean and y.  ``nu``: the q noise variances
    of the gradient observations (constant), or None for ``nugget_rel`` times ``gradient_prior_curvature`` at the CURRENT w and sf2,
    whose derivative by w and sf2 is added on the host from the diagonal of the gradient rows' block of Kj^-1 - alpha alpha^T.

    As in ExactMLLFunction the whole evaluation is enqueued in ``forward``: the three blocks into the triangle gpp_potrf reads
    (nu and the jitter on the diagonal, the attempts of ``_attempts`` as for ``_factor``), potrf, trtri, z, alpha, the dense LAUUM,
    gpp_grad_reduce on the leading N x N view and gpp_gek_grad_reduce on the other two blocks; ``backward`` is ``_eval_backward``
    with two blocks of feature rows."""

    @staticmethod
    def forward(ctx, U, Ug, w, sf2, tau, mean, y, r_g, nu, grp, kind, d_split, d0, nd, dU, nugget_rel, slot, sel=None):
        gctx = get_context(U.device)  # raises GppError for anything but a GPU: there is no CPU path
        with torch.cuda.device(U.device):
            if torch.cuda.is_current_stream_capturing():
                raise NotImplementedError("the gradient-enhanced objective is not available inside a graph capture")
            dev = U.device
            (N, D), Mg = U.shape, Ug.shape[0]
            q = Mg * nd if sel is None else sel.q
            n = N + q
            Ud, wd, sd, td, grp, S, need_grad, need_U = _eval_operands(ctx, U, w, sf2, tau, mean, y, grp, dU, Ug)
            Ugd = _as_f64(Ug.detach(), dev)
            dUk = dU if need_U else 0
            spec = KernelSpec(wd, sd, kind, d_split)
            if nu is None:
                nu_d = float(nugget_rel) * gradient_prior_curvature(spec, d0, nd)
                nu_d = nu_d.repeat(Mg) if sel is None else nu_d[sel.flat % nd]
            else:
                nu_d = _as_f64(nu.detach().reshape(-1), dev)
            ws = get_workspace(gctx, n, slot)
            ws.epoch += 1
            torch.sub(_as_f64(y.detach(), dev), _as_f64(mean.detach(), dev), out=ws.r[:N])
            ws.r[N:].copy_(_as_f64(r_g.detach().reshape(-1), dev))
            g_w, g_s, g_t, g_Ud, g_Ugd = _grad_buffers(need_grad, dev, (), D, S, (N, dUk), (Mg, dUk))
            # gpp_cross_kernel_dx / gpp_kernel_dxdx write 16-byte pairs: a window that starts at an odd column N is built aside
            aligned = N % 2 == 0
            Kfg_out = ws.A[:N, N:n] if aligned else rows_buffer(N, q, dev)
            Kgg_out = ws.A[N:n, N:n] if aligned else square_buffer(q, dev)

            def rest():
                with _stage("trtri"):
                    gctx.trtri(ws.A, ws.Li, ws.Ki)
                with _stage("mll_reduce"):
                    gctx.mll_reduce(ws.A, ws.Li, ws.r, ws.z, ws.out3)
                if not need_grad:
                    return
                with _stage("alpha"):
                    gctx.alpha(ws.Li, ws.z, ws.alpha)
                with _stage("lauum"):
                    gctx.lauum(ws.Li, ws.Ki)
                with _stage("grad_reduce"):
                    gctx.grad_reduce(Ud, wd, sd, grp, S, ws.alpha[:N], ws.Ki[:N, :N], dUk, g_w, g_s, g_t, g_Ud, kind=kind,
                                     d_split=d_split)
                with _stage("gek_grad_reduce"):
                    gctx.gek_grad_reduce(Ud, Ugd, wd, sd, d0, nd, ws.alpha, ws.Ki, dUk, g_w, g_s, g_Ud, g_Ugd, kind=kind,
                                         d_split=d_split, sel=sel)
                    if nu is None:
                        # d nu_k / dw_j = rel c_j sf2, d nu_k / dsf2 = rel c_j w_j on the rows k = (a, j), times W_kk
                        a_g = ws.alpha[N:]
                        Wd = 0.5 * (a_g * a_g - ws.Ki[N:n, N:n].diagonal())
                        if sel is not None:  # (scattered into the dense layout, zeros elsewhere: the same ordered sum, no atomics)
                            Wd = torch.zeros(Mg * nd, dtype=torch.float64, device=dev).index_put_((sel.flat,), Wd)
                        Wd = Wd.view(Mg, nd).sum(0)
                        c = float(nugget_rel) * _curvature_coefficients(spec)[d0:d0 + nd]
                        g_w[d0:d0 + nd].add_(c * sd * Wd)
                        g_s.add_((c * wd[d0:d0 + nd] * Wd).sum())

            def build_factor(jit):
                with _stage("gek_build"):
                    gctx.kernel_build(Ud, wd, sd, td, grp, ws.A[:N, :N], jitter=jit, kind=kind, d_split=d_split, uplo=UPLO_UPPER)
                    gctx.cross_kernel_dx(Ugd, Ud, wd, sd, d0, nd, Kfg_out, kind=kind, d_split=d_split, sel=sel)
                    gctx.kernel_dxdx(Ugd, Ugd, wd, sd, d0, nd, Kgg_out, kind=kind, d_split=d_split, sel_a=sel, sel_b=sel)
                    if not aligned:
                        ws.A[:N, N:n].copy_(Kfg_out)
                        ws.A[N:n, N:n].copy_(Kgg_out)
                    ws.A[N:n, N:n].diagonal().add_(nu_d + jit)
                with _stage("potrf"):
                    gctx.potrf(ws.A, ws.Li, ws.info, ws.Ki)

            _attempts(gctx, ws, build_factor, inputs_nan_probe(torch.cat([Ud.reshape(-1), Ugd.reshape(-1), ws.r]), wd, sd,
                                                               torch.cat([td, nu_d])), after=rest)
            ctx.saved = (g_w, g_s, g_t, (g_Ud, g_Ugd), ws.alpha[:N].clone() if need_grad else None)
            return ws.out3[2].clone()

    @staticmethod
    def backward(ctx, grad_out):
        return _eval_backward(ctx, grad_out, *ctx.saved) + (None,) * 11


def exact_gek_mll(U: torch.Tensor, Ug: torch.Tensor, spec: KernelSpec, tau: torch.Tensor, mean: torch.Tensor, y: torch.Tensor,
                  r_g: torch.Tensor, noise: Optional[torch.Tensor], grp: Optional[torch.Tensor], d0: int, nd: int,
                  n_grad_dims: Optional[int] = None, slot: Optional[int] = None, sel=None) -> torch.Tensor:
    """log N([y - mean; r_g] | 0, Kj) on the GPU (``ExactGEKFunction``): the joint density of the N function rows ``U`` and the
    q = Mg nd observed gradients ``r_g`` (point-major, scaled units; prior mean 0) with respect to the features d0 .. d0 + nd - 1 at
    the rows ``Ug``.  ``noise``: their q variances (scaled units squared, constant during a fit), or None for
    ``gradient_enhanced.GRADIENT_NUGGET_REL`` times the prior curvature at the current hyperparameters.  Differentiable with respect
    to U[:, :n_grad_dims], Ug[:, :n_grad_dims], spec.w, spec.sf2, tau, mean and y; n_grad_dims <= d0.  The matrix is factored from
    scratch in a workspace of N + q rows: q is limited by memory alone.  ``sel``: a ``backend.GradientSelection`` of the observed
    (point, direction) entries (partial gradients): q = sel.q, ``r_g`` and ``noise`` hold those entries in its order, and the
    density is that of the selected rows alone.  Refused under ``settings.sharded_evaluation`` and inside a graph capture."""
    from .gradient_enhanced import GRADIENT_NUGGET_REL

    _gradient_cache_refusals("the gradient-enhanced objective")
    if slot is None:
        slot = current_slot()
    if n_grad_dims is None:
        n_grad_dims = min(U.shape[1], int(d0)) if (U.requires_grad or Ug.requires_grad) else 0
    d0, nd, dU = int(d0), int(nd), int(n_grad_dims)
    D = U.shape[1]
    if Ug.dim() != 2 or Ug.shape[0] < 1 or Ug.shape[1] != D:
        raise ValueError(f"the gradient points must be at least one row of {D} features (got {tuple(Ug.shape)})")
    if nd < 1 or d0 < 0 or d0 + nd > D:
        raise ValueError(f"the differentiated features [{d0}, {d0 + nd}) must be a non-empty range of the {D} features")
    if sel is not None and (sel.num_points, sel.nd) != (Ug.shape[0], nd):
        raise ValueError(f"a selection of {sel.num_points} points x {sel.nd} directions for {Ug.shape[0]} x {nd}")
    q = Ug.shape[0] * nd if sel is None else sel.q
    if r_g.numel() != q or (noise is not None and noise.numel() != q):
        raise ValueError(f"{r_g.numel()} gradients / {None if noise is None else noise.numel()} noise variances for {q} gradient "
                         "observations")
    if dU > d0:
        raise ValueError(f"the {dU} feature columns with a gradient must lie in front of the differentiated ones (d0 = {d0})")
    return ExactGEKFunction.apply(U, Ug, spec.w, spec.sf2, tau, mean, y, r_g, noise, grp, spec.kind, spec.d_split, d0, nd, dU,
                                  GRADIENT_NUGGET_REL, slot, sel)


#: Scratch one gpp_post_cross_min launch of ``knowledge_gradient`` may ask for: above it the reference rows go in column chunks
#: (a multiple of 128 columns each), whose minima compose exactly.  16384 x 16384 at Q = 32 would take 1 GiB in one launch.
KG_WORKSPACE_CAP = 256 << 20


def gauss_hermite_rule(num_nodes: int):
    """Nodes and weights of the ``num_nodes``-point Gauss-Hermite rule for a standard normal variable (probabilists' form), as
    numpy float64: weights normalised to sum 1, the nodes made exactly antisymmetric and the weights exactly symmetric."""
    import numpy as np

    z, W = np.polynomial.hermite_e.hermegauss(int(num_nodes))
    z = (z - z[::-1]) / 2
    W = (W + W[::-1]) / 2
    return z, W / W.sum()


@torch.no_grad()
def knowledge_gradient(cache: FactorCache, Uc, tau_c, Ur, mean_r, q: int = 1, cost=None, maximize: bool = False, num_nodes: int = 32,
                       transposed: Optional[bool] = None):
    """Knowledge gradient of ONE noisy observation at each candidate ``Uc`` (M_c x D; ``tau_c``: the candidates' own noise levels)
    for the minimum (``maximize``: the maximum) of the posterior mean over the reference features ``Ur`` (M_r x D; ``mean_r``: the
    posterior mean of f there, prior mean included, in the cache's scaled units), and a greedy batch of ``q`` candidates.  With
    v(x) = Linv k(X, x), c(x, x') = sf2 k(x, x') - v(x)^T v(x') and s_c = max(c(x_c, x_c), 0) + tau_c + jitter, an observation at x_c
    moves the mean at x_r to mu_r + c(x_r, x_c) / sqrt(s_c) Z with Z ~ N(0, 1), so
        KG(c) = min_r mu_r - E_Z[ min_r (mu_r + c_cr Z / sqrt(s_c)) ].
    The expectation is APPROXIMATED by a Gauss-Hermite rule with ``num_nodes`` (1..64) nodes — deterministic, not the exact
    expectation through the lower envelope of the M_r lines: with 32 nodes the error measured on small problems is a few per cent
    of the largest score and one node gives exactly 0.  Per node the minimum over r comes from gpp_post_cross_min
    on the V of ``predict_from_cache``; the M_c x M_r block of c never exists.  The means are shifted by their minimum, m_r >= 0, so
    the score is -sum_k W_k min_r(...) >= 0 (the minimum is concave, W >= 0 and sum_k W_k z_k = 0); rounding noise is clamped at 0.
    Reference rows beyond ``KG_WORKSPACE_CAP`` bytes of scratch go in column chunks combined by ``torch.minimum``, bit for bit the
    result of one launch.

    q > 1 is the "Kriging believer" heuristic (Ginsbourger et al. 2010): after a pick j its observation is believed to equal its
    mean, so mu stays, every point gains the coordinate c(x, x_j) / sqrt(s_j) as in ``variance_reduction`` and the variances shrink;
    picked rows are excluded.  Unlike ALC's, the gains of this heuristic do NOT add up to a joint quantity.  With ``cost`` the pick
    maximises score / cost and the reported gains stay undivided.  Returns (the M_c first-round scores, the picked rows of ``Uc`` in
    pick order, their gains), in the cache's (scaled-target) units.  The cache is only read.  Refused under
    ``settings.sharded_evaluation`` and inside a graph capture, like ``variance_reduction``."""
    from .backend import MAX_NODES, post_cross_min_workspace_bytes

    what = "knowledge_gradient"
    q, Q, transposed = int(q), int(num_nodes), ALC_TRANSPOSED if transposed is None else bool(transposed)
    with _score_call(what, cache):
        gctx, spec = cache.gctx, cache.spec
        Uc, Ur = _score_points(what, cache, Uc, Ur, q)
        (Mc, dev), Mr = (Uc.shape[0], Uc.device), Ur.shape[0]
        if Q < 1 or Q > MAX_NODES:
            raise ValueError(f"{what}: num_nodes must be between 1 and {MAX_NODES}; got {Q}")
        tau_c = _per_row(what, tau_c, Mc, "noise levels", "candidates", dev)
        mean_r = _per_row(what, mean_r, Mr, "means", "reference points", dev)
        if cost is not None:
            cost = _per_row(what, cost, Mc, "costs", "candidates", dev)
        cache.refresh()  # (a cache of the shared workspace that another model has factored into since)
        w, sf2 = spec.w, spec.sf2.reshape(1)
        z, W = gauss_hermite_rule(Q)
        nodes = torch.tensor(z, dtype=torch.float64, device=dev)
        W = torch.tensor(W, dtype=torch.float64, device=dev)
        m = ((mean_r.max() - mean_r) if maximize else (mean_r - mean_r.min())).contiguous()
        # reference rows per launch: all of them, or the multiple of 128 columns whose records fit under the cap
        step = Mr
        if post_cross_min_workspace_bytes(Mc, Mr, Q) > KG_WORKSPACE_CAP:
            step = 128 * max(1, int(KG_WORKSPACE_CAP // post_cross_min_workspace_bytes(Mc, 128, Q)))
        out = torch.empty(Mc, Q, dtype=torch.float64, device=dev)
        part = torch.empty(Mc, Q, dtype=torch.float64, device=dev) if step < Mr else None

        def score(K, s, Vc, Vr):
            scale = 1.0 / s.sqrt()
            with _stage("post_cross_min"):
                for c0 in range(0, Mr, step):
                    c1 = min(Mr, c0 + step)
                    gctx.post_cross_min(Uc, Ur[c0:c1], w, sf2, Vc, Vr[:, c0:c1] if transposed else Vr[c0:c1], K, m[c0:c1], scale,
                                        nodes, out if c0 == 0 else part, kind=spec.kind, d_split=spec.d_split,
                                        transposed=transposed)
                    if c0 > 0:
                        torch.minimum(out, part, out=out)
            return (-(out * W).sum(dim=1)).clamp_min(0.0)

        return _greedy_picks("kg", cache, Uc, tau_c, Ur, q, cost, transposed, score)


# ---------------------------------------------------------------------------------------------------
# differentiable prediction (settings.differentiable_predictions): gpytorch's exact prediction strategy under autograd with its
# default detach_test_caches — alpha = Ky^-1 (y - m) and Ky are constants; the test-train covariance, the prior variance sf2 and
# (through Utr) the training features stay differentiable.  Both backwards end in gpp_cross_grad, which recomputes K_*N in
# registers: G = gmean alpha^T (mean) or -2 diag(gvar) B with B = K_*N Ky^-1 = V Linv (variance).
# ---------------------------------------------------------------------------------------------------
def _cross_backward(ctx, gmean, alpha, gvar, B):
    """Gradients (Us, Utr, w, sf2) of sum_aj G_aj K_aj from one gpp_cross_grad call, each in the dtype of its input."""
    cache, dB = ctx.cache, ctx.dB
    Us, Utr, w, sf2 = ctx.saved_tensors
    need = ctx.needs_input_grad
    dev = cache.U.device
    Ua = _as_f64(Us.detach(), dev)
    Ub = cache.U if Utr is None else _as_f64(Utr.detach(), dev)
    M, D = Ua.shape
    N = Ub.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    g_Ua = torch.empty(M, D, **f64) if need[0] else None
    g_Ub = torch.empty(N, dB, **f64) if need[1] and dB > 0 else None
    g_w = torch.empty(D, **f64) if need[2] else None
    g_s = torch.empty(1, **f64) if need[3] else None
    if g_Ua is not None or g_Ub is not None or g_w is not None or g_s is not None:
        cache.gctx.cross_grad(Ua, Ub, _as_f64(w.detach(), dev), _as_f64(sf2.detach().reshape(1), dev), gmean, alpha, gvar, B,
                              g_Ua, g_Ub, g_w, g_s, kind=cache.spec.kind, d_split=cache.spec.d_split)
    g_U = None
    if need[1]:
        g_U = torch.zeros(N, D, **f64)
        if g_Ub is not None:
            g_U[:, :dB] = g_Ub
    return (None if g_Ua is None else g_Ua.to(Us.dtype), None if g_U is None else g_U.to(Utr.dtype),
            None if g_w is None else g_w.to(w.dtype), None if g_s is None else g_s.reshape(sf2.shape).to(sf2.dtype))


class PredictMeanFunction(torch.autograd.Function):
    """mean_a = sum_j K(Us_a, Utr_j) alpha_j: the forward is ``predict_from_cache``'s mean-only path (the same numbers as a
    no-grad prediction); the backward is ONE gpp_cross_grad with G = gmean alpha^T — O(M N D), no N x N operand."""

    @staticmethod
    def forward(ctx, Us, Utr, w, sf2, cache, dB):
        dev = cache.U.device
        with torch.cuda.device(dev):
            mean, _, _ = predict_from_cache(cache, _as_f64(Us.detach(), dev), need_var=False)
        ctx.cache, ctx.dB = cache, dB
        ctx.save_for_backward(Us, Utr, w, sf2)
        return mean

    @staticmethod
    def backward(ctx, gmean):
        with torch.cuda.device(ctx.cache.U.device):
            grads = _cross_backward(ctx, gmean.to(torch.float64).contiguous(), ctx.cache.alpha, None, None)
        return grads + (None, None)


class PredictVarFunction(torch.autograd.Function):
    """var_a = sf2 - k_a^T Ky^-1 k_a: the forward is ``predict_from_cache``'s variance path (V = K_*N Linv^T, kept for the
    backward); the backward forms B = V Linv (one M N^2 GEMM) and runs gpp_cross_grad with gvar = -2 dL/dvar."""

    @staticmethod
    def forward(ctx, Us, Utr, w, sf2, cache, dB):
        dev = cache.U.device
        with torch.cuda.device(dev):
            # another model of the same size may have factored into the shared workspace since the cache was made
            cache.refresh()
            _, var, V = predict_from_cache(cache, _as_f64(Us.detach(), dev), need_var=True, need_V=True)
        ctx.cache, ctx.dB, ctx.V = cache, dB, V
        ctx.save_for_backward(Us, Utr, w, sf2)
        return var

    @staticmethod
    def backward(ctx, gvar):
        cache, V = ctx.cache, ctx.V
        with torch.cuda.device(cache.U.device):
            cache.refresh()  # Linv of this cache's own factor (the same bits: same inputs, same jitter schedule)
            M, N = V.shape
            B = torch.empty((M, V.stride(0)), dtype=torch.float64, device=V.device)[:, :N]
            # B = V Linv against the lower triangle of the Linv buffer (its upper triangle holds the mirror; keep k >= n), as the
            # row-contiguous TN product from V^T: the NN form of the same product measured 95 ms against 55 for the forward's TN
            # product at M = 8192, N = 20000 (the k-contiguous variant, gpp_predict_tn); the transpose costs 2 M N doubles of traffic
            Vt = rows_buffer(N, M, V.device)
            cache.gctx.transpose(V, Vt)
            cache.gctx.gemm(1, 0, M, N, N, 1.0, Vt, cache.Linv, 0.0, B, b_mask=2, klo_mode=2)
            del Vt
            gv = gvar.to(torch.float64).contiguous()
            g_Us, g_Utr, g_w, g_s = _cross_backward(ctx, None, None, -2.0 * gv, B)
            if g_s is not None:
                g_s = g_s + gv.sum().reshape(g_s.shape).to(g_s.dtype)  # k(u, u) = sf2 for every stationary kind
        return g_Us, g_Utr, g_w, g_s, None, None


def predict_mean(cache: FactorCache, Us, Utr, w, sf2, dB: int = 0) -> torch.Tensor:
    """K_*N alpha, differentiable w.r.t. the test features Us, the training features Utr[:, :dB] (None: the cache's, constant),
    the kernel weights w and the outputscale sf2."""
    return PredictMeanFunction.apply(Us, Utr, w, sf2, cache, int(dB))


def predict_var(cache: FactorCache, Us, Utr, w, sf2, dB: int = 0) -> torch.Tensor:
    """sf2 - diag(K_*N Ky^-1 K_N*), differentiable like :func:`predict_mean`."""
    return PredictVarFunction.apply(Us, Utr, w, sf2, cache, int(dB))


@torch.no_grad()
def dense_log_prob(cov: torch.Tensor, diff: torch.Tensor) -> torch.Tensor:
    """log N(diff | 0, cov) for a dense covariance (used by ``evaluation``'s joint NLPD, models/gp_plus.py:900-903)."""
    dev = cov.device
    gctx = get_context(dev)
    N = cov.shape[0]
    A = square_buffer(N, dev)
    A.copy_(cov)
    Li, T = square_buffer(N, dev), square_buffer(N, dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    fresh = True

    def attempt(jit):
        nonlocal fresh
        if not fresh:
            A.copy_(cov)
            A.diagonal().add_(jit)
        fresh = False
        gctx.potrf(A, Li, info)
        return int(info.item())

    psd_safe(gctx, attempt)
    gctx.trtri(A, Li, T)
    z = torch.empty(N, dtype=torch.float64, device=dev)
    out3 = torch.empty(3, dtype=torch.float64, device=dev)
    gctx.mll_reduce(A, Li, _as_f64(diff, dev), z, out3)
    return out3[2].clone()


# ---------------------------------------------------------------------------------------------------
# sampling (MultivariateNormal.rsample, GP_Plus.sample_y — models/gp_plus.py:985-998): a covariance built straight into the upper
# triangle of a square buffer, its Cholesky factor U (Sigma = U^T U) with the jitter schedule of ``dense_log_prob``, and draws
# loc + Z U.  No autograd: gradients through draws are not offered.
# ---------------------------------------------------------------------------------------------------
@torch.no_grad()
def predictive_cov_upper(Us: torch.Tensor, spec: KernelSpec, V: torch.Tensor, d: Optional[torch.Tensor] = None,
                         jitter: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K(Us, Us) + diag(d) + jitter I - V V^T (V = K_*N L^-T from ``predict_from_cache``) in the UPPER triangle of ``out``: the
    kernel build writes the upper tiles only and the MFMA GEMM subtracts V V^T on the upper triangle only (c_tri = 2), half the
    flops of the full square that ``covariance_matrix`` forms."""
    dev = Us.device
    gctx = get_context(dev)
    M = Us.shape[0]
    A = square_buffer(M, dev) if out is None else out
    tau = grp = None
    if d is not None:  # the added diagonal as M noise groups of one point each
        tau = _as_f64(d.reshape(-1), dev)
        grp = torch.arange(M, dtype=torch.int32, device=dev)
    with _stage("pred_cov_build"):
        gctx.kernel_build(_as_f64(Us, dev), _as_f64(spec.w, dev), _as_f64(spec.sf2.reshape(1), dev), tau, grp, A, jitter=jitter,
                          kind=spec.kind, d_split=spec.d_split, uplo=UPLO_UPPER)
    with _stage("pred_cov_vvt"):
        gctx.gemm(0, 1, M, M, V.shape[1], -1.0, V, V, 1.0, A, c_tri=2)
    return A


@torch.no_grad()
def train_post_cov_upper(cache: FactorCache, d: Optional[torch.Tensor] = None, jitter: float = 0.0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same covariance when the test points ARE the training points: Sigma = T - T Ky^-1 T (+ diag(d) + jitter I), T the
    training noise (plus the cache's own jitter, so that it equals the general route's K - K (Ky + jI)^-1 K).  Ky^-1 is one LAUUM of
    the cached inverse factor into ``out``, which gpp_post_cov_train then overwrites in place; cache.L / cache.Linv stay as they are."""
    cache.refresh()
    gctx = cache.gctx
    dev = cache.U.device
    N = cache.U.shape[0]
    A = square_buffer(N, dev) if out is None else out
    tau, grp, _ = cache._refactor
    if cache.jitter:
        tau = tau + cache.jitter
    with _stage("sample_lauum"):
        gctx.lauum(cache.Linv, A)
    with _stage("post_cov_train"):
        gctx.post_cov_train(A, tau, grp, None if d is None else _as_f64(d.reshape(-1), dev), A, jitter=jitter)
    return A


@torch.no_grad()
def mvn_root(build_upper, n: int, device) -> Tuple[torch.Tensor, float]:
    """Upper Cholesky factor U of a covariance that ``build_upper(A, jitter)`` writes into the upper triangle of the n x n buffer A
    (with ``jitter`` added to its diagonal), under the jitter schedule of ``dense_log_prob``: 0, then cholesky_jitter * 10^i, then
    ``NotPSDError``; a panel time-out repeats the attempt.  Returns (U, jitter); U's strict lower triangle is not part of it."""
    dev = torch.device(device)
    gctx = get_context(dev)
    A, Li, T = square_buffer(n, dev), square_buffer(n, dev), square_buffer(n, dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)

    def attempt(jit):
        build_upper(A, jit)
        with _stage("sample_potrf"):
            gctx.potrf(A, Li, info, T)
        return int(info.item())

    return A, psd_safe(gctx, attempt)


@torch.no_grad()
def mvn_draw(U: torch.Tensor, loc: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
    """loc + Z U for Z (S x M, fp64) and the upper factor U of ``mvn_root``: S draws of N(loc, U^T U), one NN GEMM against U's upper
    triangle (b_mask = 1, K range cut at each column tile's end)."""
    dev = U.device
    gctx = get_context(dev)
    S, M = Z.shape
    Zp = rows_buffer(S, M, dev)
    Zp.copy_(Z)
    out = rows_buffer(S, M, dev)
    out.copy_(_as_f64(loc, dev).expand(S, M))
    if S > 0 and M > 0:
        gctx.gemm(0, 0, S, M, M, 1.0, Zp, U, 1.0, out, b_mask=1, khi_mode=2)
    return out

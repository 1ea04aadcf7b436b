"""Torch-tensor front of the C ABI: one :class:`GppContext` per GPU owns the library handle, follows PyTorch's
current HIP stream and keeps the scratch workspace.  PyTorch is used for device memory and streams only; every
number is produced by the kernels in ``csrc/``.

Reference boundary this replaces: the gpytorch/ATen operators reached from ``optim/mll_torch.py:112-117`` and
``models/gpregression.py:122-149``.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading
import weakref
from typing import Dict, Optional, Tuple

import torch

from . import _lib, settings
from ._lib import NO_WORKSPACE, GppError, check  # noqa: F401 (NO_WORKSPACE: re-exported, the tests read it here)

KIND_RBF, KIND_MATERN32, KIND_MATERN52 = 0, 1, 2
UPLO_FULL, UPLO_LOWER, UPLO_UPPER = 0, 1, 2
OPT_COOP_PANEL, OPT_PANEL_FAULT, OPT_PANEL_TIMEOUT_MS, OPT_EXEC_SCHED, OPT_DAG_SCHED = 1, 2, 3, 4, 5  # gpp_set_option (include/gpp.h)
OPT_GEMM_TILE = 6  # tile of gemm / gemm_batched: 0 by grid size, 1 = 32x32, 2 = 64x64, 3 = 128x128, 4 = 128x32 (tests)
OP_MLL_EVAL, OP_PREDICT, OP_PREDICT_GRAD = 0, 1, 2
OP_APPLY = 3  # gpp_kernel_apply / gpp_rff_apply: N carries the contracted length
OP_APPLY_GRAD = 4  # gpp_kernel_apply_grad / gpp_rff_apply_grad: N carries the contracted length
OP_APPEND = 5  # gpp_chol_append: N cached points, M carries the appended count q
OP_POST_CROSS = 6  # gpp_post_cross_sq: N carries the reference count M_r, M the candidate count M_c
OP_POST_CROSS_MIN = 7  # gpp_post_cross_min: N carries M_r, M carries M_c, S the node count Q
OP_POINT_GRAM = 8  # gpp_point_gram with a weighted sum: M points, D carries the rows per point
OP_GEK_GRAD = 9  # gpp_gek_grad_reduce: N function points, M carries the gradient points Mg, S the feature columns with a gradient
OP_POST_CROSS_LIN = 10  # gpp_post_cross_lin_sq: N carries the reference count M_r, M the functional count M_f
#: most quadrature nodes gpp_post_cross_min takes (gpp_gemm.hip PostCrossMinEpilogue::QMAX)
MAX_NODES = 64
#: longest contraction gpp_kernel_apply / gpp_rff_apply run without scratch (gpp_apply.hip AP_SPLIT)
APPLY_SPLIT = 2048
NOT_SUPPORTED = 2001  # GPP_NOT_SUPPORTED: gpp_lauum_grad does not take these arguments, nothing was enqueued
#: the tile kernels stage at most this many feature columns (manifold + quantitative) per point in LDS (gpp_build.hip DMAX)
MAX_FEATURES = 64


def _check_features(D: int) -> None:
    if D < 1 or D > MAX_FEATURES:
        raise GppError(f"the covariance kernels take 1..{MAX_FEATURES} feature columns per point (got {D})")

#: one context (library handle + stream binding + scratch) per (device, host thread): concurrent evaluations driven
#: from different threads on different HIP streams never share a handle
_contexts: Dict[Tuple[int, int], "GppContext"] = {}
_contexts_lock = threading.Lock()


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need(t: torch.Tensor, dtype, name: str) -> None:
    if not t.is_cuda:
        raise GppError(f"{name} must live on the GPU (got {t.device}); libgpp_hip has no CPU path")
    if t.dtype != dtype:
        raise GppError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous() and t.dim() == 1:
        raise GppError(f"{name} must be contiguous")


#: status word of a factorisation whose cooperative panel kernel gave up waiting for one of its own work-groups (gpp_leaf.hip:
#: a wait is abandoned after ~1 s instead of hanging the GPU).  NOT "matrix not positive definite": adding jitter cannot help.
INFO_PANEL_TIMEOUT = 1 << 30
#: the same for a wait of one of the DAG executor's work-groups (gpp_dag_f64 and its gate kernels): bit 29 on top
INFO_EXEC_TIMEOUT = (1 << 30) | (1 << 29)


def check_status(info: int) -> None:
    """Raise for the status words that are not LAPACK's "leading minor k is not positive definite"."""
    if info >= INFO_PANEL_TIMEOUT:
        what = "an executor launch" if info & (1 << 29) else "the cooperative panel kernel"
        raise GppError(f"gpp_potrf: {what} timed out waiting for one of its work-groups (another kernel holding the stream's CUs "
                       "for seconds, or a caller-supplied CU-masked stream with fewer CUs than the launch assumed); "
                       "GPP_COOP_PANEL=0 selects the leaf-step factorisation, GPP_DAG_SCHED=0 the launch-per-product one")


def panel_timed_out(ctx: "GppContext", info: int) -> bool:
    """True when ``info`` is a time-out status the context can answer by switching a cooperative path off; the caller then factors
    again.  The DAG EXECUTOR's time-out (bit 29: its work-groups wait for the panel stream's launches — under co-tenancy or serialised
    dispatch they give up first) switches only the executor off: the factorisation falls back to launch-per-product with the
    cooperative panel, which needs 32 resident work-groups.  The PANEL's own
    time-out switches the panel off (and with it everything built on it): leaf-step launches need no co-residency at all."""
    if info < INFO_PANEL_TIMEOUT:
        return False
    import warnings

    ms = info & 0xFFFFF
    if info & (1 << 29):
        if not ctx.dag_sched:
            check_status(info)  # cannot happen without the executor: report it
        warnings.warn(f"libgpp_hip: an executor launch timed out after {ms} ms (another tenant of this GPU held part of its CUs, or "
                      "dispatches are serialised); this context now factors with one launch per product", RuntimeWarning)
        ctx.set_option(OPT_DAG_SCHED, 0)
        return True
    if not ctx.coop_panel:
        check_status(info)  # cannot happen without a panel: report it
    warnings.warn(f"libgpp_hip: a cooperative panel launch timed out after {ms} ms (another tenant of this GPU held part "
                  "of its CUs); this context now factors with leaf-step launches", RuntimeWarning)
    ctx.set_option(OPT_COOP_PANEL, 0)
    return True


def row_stride(n: int) -> int:
    """Row stride of an n-column fp64 matrix: n padded to a multiple of 16 doubles (128-byte lines)."""
    return max(16, (n + 15) // 16 * 16)


def rows_buffer(m: int, n: int, device) -> torch.Tensor:
    """Uninitialised m x n fp64 matrix with padded rows (``row_stride``)."""
    return torch.empty((m, row_stride(n)), dtype=torch.float64, device=device)[:, :n]


def square_buffer(n: int, device) -> torch.Tensor:
    return rows_buffer(n, n, device)


def _ld(m: torch.Tensor) -> int:
    if m.dim() != 2 or m.stride(1) != 1:
        raise GppError("matrix must be 2-D with unit column stride")
    return m.stride(0) if m.shape[0] > 1 else max(m.shape[1], m.stride(0))


def _post_cross_checks(fn, a, named, K, kind, d_split, transposed, omega=None, own=None):
    """What ``post_cross_sq``, ``post_cross_lin_sq`` and ``post_cross_min`` (``fn``) check alike, in the order they always did:
    every tensor of ``named`` (name -> tensor, in the wrapper's order) is fp64 on the GPU; the feature rows ``U{a}`` (a = "c" or "f")
    and ``Ur``, ``w``, ``sf2``, K >= 1 and kind / d_split; then the wrapper's ``own(M_a, D)`` checks, if any; the windows ``V{a}`` and
    ``Vr`` under ``transposed``; ``omega``.  Returns (M_a, M_r, D)."""
    for n, t in named.items():
        _need(t, torch.float64, n)
    Ua, Ur, w, sf2 = named["U" + a], named["Ur"], named["w"], named["sf2"]
    if Ua.dim() != 2 or Ur.dim() != 2 or Ua.shape[1] != Ur.shape[1]:
        raise GppError(f"U{a} and Ur must be matrices with the same feature count (got {tuple(Ua.shape)}, {tuple(Ur.shape)})")
    (Ma, D), Mr = Ua.shape, Ur.shape[0]
    _check_features(D)
    if min(Ma, Mr, K) < 1:
        raise GppError(f"{fn} takes M_{a}, M_r, K >= 1 (got {Ma}, {Mr}, {K})")
    if not (Ua.is_contiguous() and Ur.is_contiguous()):
        raise GppError(f"U{a} and Ur must be contiguous")
    if w.numel() != D or not w.is_contiguous():
        raise GppError(f"w must be a contiguous vector of {D} weights (got {w.numel()})")
    if sf2.numel() < 1:
        raise GppError("sf2 must hold one value")
    if not (0 <= int(d_split) <= D) or kind not in (KIND_RBF, KIND_MATERN32, KIND_MATERN52):
        raise GppError(f"bad kernel kind / d_split ({kind}, {d_split}) for {D} features")
    if own is not None:
        own(Ma, D)
    for n, pts in (("V" + a, Ma), ("Vr", Mr)):
        t = named[n]
        if t.dim() != 2 or t.stride(1) != 1:
            raise GppError(f"{n} must be 2-D with unit column stride")
        rows, cols = (K, pts) if transposed else (pts, K)
        if t.shape[0] < rows or t.shape[1] < cols or (t.shape[1 if transposed else 0] != pts):
            raise GppError(f"{n} is {tuple(t.shape)}: {fn} with {pts} points and K = {K} needs "
                           f"{'at least ' + str(K) + ' x ' + str(pts) if transposed else str(pts) + ' x at least ' + str(K)}")
        ld = _ld(t)
        if ld & 1 or ld < cols:
            raise GppError(f"{n}: the leading dimension ({ld}) must be even and at least {cols}")
        if t.data_ptr() & 15:
            raise GppError(f"{n} must be 16-byte aligned")
    if omega is not None:
        _need(omega, torch.float64, "omega")
        if omega.dim() != 1 or omega.numel() != Mr or not omega.is_contiguous():
            raise GppError(f"omega must be a contiguous vector of {Mr} weights (got {tuple(omega.shape)})")
    return Ma, Mr, D


class GradientSelection:
    """Which (point, direction) entries of ``Mg`` gradient points with ``nd`` directions each are observed, in the form the
    ``_sel`` entry points of gpp.h take.  Built once per call from a bool mask (Mg, nd) — the ONLY producer of these arrays, whose
    contents the C layer does not check:
      ``first``  device int32 (Mg + 1): first[a] = the number of observed entries of the points before a;
      ``dir``    device int32 (q): the direction of observation k, strictly increasing within a point;
      ``q``      the number of observations, a Python int (the mask is read on the host once: one sync for a device mask);
      ``flat``   device int64 (q): a nd + j of observation k, the gather of a dense point-major (Mg nd) vector;
      ``mask``   a bool copy of the mask on the device.
    Observation k is row (or column) k of every compact block, point-major."""

    def __init__(self, mask, device=None):
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.dim() != 2 or mask.shape[1] < 1:
            raise GppError("a gradient selection is built from a bool mask (points, directions)")
        dev = mask.device if device is None else torch.device(device)
        host = mask.detach().cpu().contiguous()
        self.num_points, self.nd = int(host.shape[0]), int(host.shape[1])
        first = torch.zeros(self.num_points + 1, dtype=torch.int64)
        torch.cumsum(host.sum(1), 0, out=first[1:])
        flat = host.reshape(-1).nonzero().reshape(-1)  # (row-major: point-major, directions increasing within a point)
        self.q = int(flat.numel())
        if self.q < 1 or self.num_points * self.nd > 0x7ffffff0:
            raise GppError(f"a gradient selection needs at least one observed entry (mask {tuple(host.shape)}, {self.q} observed)")
        self.first = first.to(torch.int32).to(dev)
        self.dir = (flat % self.nd).to(torch.int32).to(dev)
        self.flat = flat.to(dev)
        self.mask = host.to(dev)

    def _check(self, name, M, nd, device):
        if self.num_points != M or self.nd != nd or self.first.device != device:
            raise GppError(f"{name}: the selection is for {self.num_points} points x {self.nd} directions on {self.first.device}, the "
                           f"call has {M} x {nd} on {device}")


def _on_own_device(fn):
    """Run a GppContext operator with the context's GPU as the CURRENT device.  The library enqueues on the stream it is
    handed; PyTorch's default stream is the null handle, which HIP resolves against the calling thread's current device —
    so a model on cuda:1 driven while cuda:0 is current would launch on the wrong GPU with cuda:1 pointers."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if torch.cuda.current_device() == self.index:
            return fn(self, *args, **kwargs)
        with torch.cuda.device(self.index):
            return fn(self, *args, **kwargs)

    return wrapper


class GppContext:
    def __init__(self, device: torch.device):
        if device.type != "cuda":
            raise GppError("GppContext needs a cuda (HIP) device; there is no CPU fallback")
        if not torch.cuda.is_available():
            raise GppError("no GPU visible to PyTorch: the HIP path cannot run")
        self.lib = _lib.load()
        self.device = device
        self.index = device.index if device.index is not None else torch.cuda.current_device()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.index):
            check(self.lib.gpp_create(ctypes.byref(h), self.index), "gpp_create")
        self.h = h
        self.coop_panel = settings.ENV_COOP_PANEL  # mirrors the handle's GPP_OPT_COOP_PANEL
        self.dag_sched = settings.ENV_DAG_SCHED
        # kernels that wait for each other across launches cannot run when dispatches are serialised: they would only time out
        if any(os.environ.get(v, "0") not in ("", "0") for v in ("HIP_LAUNCH_BLOCKING", "AMD_SERIALIZE_KERNEL", "CUDA_LAUNCH_BLOCKING")):
            self.set_option(OPT_DAG_SCHED, 0)
        self._ws: Optional[torch.Tensor] = None

    # -- plumbing --------------------------------------------------------------------------------
    def _stream(self) -> None:
        s = torch.cuda.current_stream(self.index).cuda_stream
        check(self.lib.gpp_set_stream(self.h, ctypes.c_void_p(s)), "gpp_set_stream")

    def set_option(self, option: int, value: int) -> None:
        check(self.lib.gpp_set_option(self.h, int(option), int(value)), "gpp_set_option")
        if option == OPT_COOP_PANEL:
            self.coop_panel = bool(value)
        elif option in (OPT_DAG_SCHED, OPT_EXEC_SCHED):
            self.dag_sched = bool(value)

    @_on_own_device
    def internal_streams(self):
        """(latency stream, throughput stream, unmasked stream): the handle's internal streams as torch streams — 32 CUs,
        the other 224, and one without a CU mask."""
        if getattr(self, "_istreams", None) is None:
            out = []
            for which in (0, 1, 2):
                p = ctypes.c_void_p()
                check(self.lib.gpp_internal_stream(self.h, which, ctypes.byref(p)), "gpp_internal_stream")
                out.append(torch.cuda.ExternalStream(p.value, device=self.device))
            self._istreams = tuple(out)
        return self._istreams

    @_on_own_device
    def ensure_workspace(self, op: int, N: int, M: int, D: int, S: int) -> None:
        need = int(self.lib.gpp_workspace_bytes(self.h, op, N, M, D, S))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            check(self.lib.gpp_set_workspace(self.h, self._ws.data_ptr(), self._ws.numel()), "gpp_set_workspace")

    def _check_groups(self, grp: torch.Tensor, N: int, S: int) -> None:
        """The kernels index tau[grp[i]] / g_tau[grp[i]] unchecked: the length is verified on every call, the value range
        once per index tensor (it costs a device read, i.e. a host sync)."""
        _need(grp, torch.int32, "grp")
        if grp.numel() != N:
            raise GppError(f"noise-group index has {grp.numel()} entries for {N} points (stale fidel_indices?)")
        # keyed on the tensor OBJECT (weak reference) and its version counter, not on its address: the caching allocator
        # hands a new index tensor of the same size the address of a freed one
        seen = getattr(self, "_grp_ok", None)
        if seen is None or seen[0]() is not grp or seen[1:] != (grp._version, N, S):
            lo, hi = int(grp.min()), int(grp.max())
            if lo < 0 or hi >= max(S, 1):
                raise GppError(f"noise-group index out of range: values in [{lo}, {hi}] for {S} noise levels")
            self._grp_ok = (weakref.ref(grp), grp._version, N, S)

    # -- operators -------------------------------------------------------------------------------
    @_on_own_device
    def kernel_build(self, U, w, sf2, tau, grp, out, *, jitter=0.0, kind=KIND_RBF, d_split=0, uplo=UPLO_FULL,
                     row0=0, nrows=None):
        N, D = U.shape
        _check_features(D)
        for t, n in ((U, "U"), (w, "w"), (sf2, "sf2"), (out, "Ky")):
            _need(t, torch.float64, n)
        if tau is not None:
            _need(tau, torch.float64, "tau")
        S = 0 if tau is None else tau.numel()
        if grp is not None:
            self._check_groups(grp, N, S)
        if not U.is_contiguous():
            raise GppError("U must be contiguous")
        self._stream()
        check(self.lib.gpp_kernel_build(self.h, U.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), _ptr(tau), _ptr(grp), S,
                                        float(jitter), kind, d_split, uplo, out.data_ptr(), _ld(out), row0,
                                        N - row0 if nrows is None else nrows), "gpp_kernel_build")
        return out

    @_on_own_device
    def cross_kernel(self, Ua, Ub, w, sf2, out, *, kind=KIND_RBF, d_split=0):
        _check_features(Ua.shape[1])
        for t, n in ((Ua, "Ua"), (Ub, "Ub"), (w, "w"), (sf2, "sf2"), (out, "Kab")):
            _need(t, torch.float64, n)
        if not (Ua.is_contiguous() and Ub.is_contiguous()):
            raise GppError("Ua/Ub must be contiguous")
        self._stream()
        check(self.lib.gpp_cross_kernel(self.h, Ua.data_ptr(), Ua.shape[0], Ub.data_ptr(), Ub.shape[0], Ua.shape[1],
                                        w.data_ptr(), sf2.data_ptr(), kind, d_split, out.data_ptr(), _ld(out)),
              "gpp_cross_kernel")
        return out

    def _apply_checks(self, Ua, second, C, out, sf2, g_Ua=None):
        """Shared by the two products and their gradients; ``out`` is the M x S operand (Out, or Gbar with ``g_Ua`` given)."""
        M, D = Ua.shape
        L, S = C.shape
        _check_features(D)
        for t, n in ((Ua, "Ua"), (second, "Ub / Omega"), (C, "C / Theta"), (out, "Out")):
            _need(t, torch.float64, n)
        if not (Ua.is_contiguous() and second.is_contiguous()):
            raise GppError("Ua and Ub / Omega must be contiguous")
        if second.shape != (L, D):
            raise GppError(f"the second operand must be {L} x {D} (got {tuple(second.shape)})")
        if out.shape != (M, S):
            raise GppError(f"Out must be {M} x {S} (got {tuple(out.shape)})")
        if min(M, L, S) < 1:
            raise GppError("gpp_kernel_apply / gpp_rff_apply take M, N (F), S >= 1")
        _need(sf2, torch.float64, "sf2")
        if sf2.numel() < 1:
            raise GppError("sf2 must hold one value")
        if g_Ua is not None:
            _need(g_Ua, torch.float64, "g_Ua")
            if g_Ua.shape != (M, D):
                raise GppError(f"g_Ua must be {M} x {D} (got {tuple(g_Ua.shape)})")
        self.ensure_workspace(OP_APPLY if g_Ua is None else OP_APPLY_GRAD, L, M, D, S)
        return M, D, L, S

    @_on_own_device
    def kernel_apply(self, Ua, Ub, w, sf2, C, out, *, beta=0.0, kind=KIND_RBF, d_split=0):
        """out = beta out + sf2 k(Ua, Ub; w) C without forming the M x N kernel block (gpp_kernel_apply)."""
        M, D, N, S = self._apply_checks(Ua, Ub, C, out, sf2)
        _need(w, torch.float64, "w")
        if w.numel() != D:
            raise GppError(f"w has {w.numel()} entries for {D} features")
        self._stream()
        check(self.lib.gpp_kernel_apply(self.h, Ua.data_ptr(), M, Ub.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), kind, d_split,
                                        C.data_ptr(), _ld(C), S, float(beta), out.data_ptr(), _ld(out)), "gpp_kernel_apply")
        return out

    @_on_own_device
    def rff_apply(self, Ua, omega, phase, sf2, theta, out, *, beta=0.0):
        """out = beta out + Phi(Ua) theta with Phi[a,f] = sqrt(2 sf2 / F) cos(omega_f . Ua_a + phase_f) (gpp_rff_apply)."""
        M, D, F, S = self._apply_checks(Ua, omega, theta, out, sf2)
        _need(phase, torch.float64, "phase")
        if phase.numel() != F:
            raise GppError(f"phase has {phase.numel()} entries for {F} features")
        self._stream()
        check(self.lib.gpp_rff_apply(self.h, Ua.data_ptr(), M, D, omega.data_ptr(), phase.data_ptr(), F, sf2.data_ptr(),
                                     theta.data_ptr(), _ld(theta), S, float(beta), out.data_ptr(), _ld(out)), "gpp_rff_apply")
        return out

    @_on_own_device
    def kernel_apply_grad(self, Ua, Ub, w, sf2, C, gbar, g_Ua, *, beta=0.0, kind=KIND_RBF, d_split=0):
        """g_Ua = beta g_Ua + d sum(gbar o (sf2 k(Ua, Ub; w) C)) / d Ua, without forming an M x N block (gpp_kernel_apply_grad)."""
        M, D, N, S = self._apply_checks(Ua, Ub, C, gbar, sf2, g_Ua)
        _need(w, torch.float64, "w")
        if w.numel() != D:
            raise GppError(f"w has {w.numel()} entries for {D} features")
        self._stream()
        check(self.lib.gpp_kernel_apply_grad(self.h, Ua.data_ptr(), M, Ub.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), kind, d_split,
                                             C.data_ptr(), _ld(C), S, gbar.data_ptr(), _ld(gbar), float(beta), g_Ua.data_ptr(),
                                             _ld(g_Ua)), "gpp_kernel_apply_grad")
        return g_Ua

    @_on_own_device
    def rff_apply_grad(self, Ua, omega, phase, sf2, theta, gbar, g_Ua, *, beta=0.0):
        """g_Ua = beta g_Ua + d sum(gbar o (Phi(Ua) theta)) / d Ua, Phi as in ``rff_apply`` (gpp_rff_apply_grad)."""
        M, D, F, S = self._apply_checks(Ua, omega, theta, gbar, sf2, g_Ua)
        _need(phase, torch.float64, "phase")
        if phase.numel() != F:
            raise GppError(f"phase has {phase.numel()} entries for {F} features")
        self._stream()
        check(self.lib.gpp_rff_apply_grad(self.h, Ua.data_ptr(), M, D, omega.data_ptr(), phase.data_ptr(), F, sf2.data_ptr(),
                                          theta.data_ptr(), _ld(theta), S, gbar.data_ptr(), _ld(gbar), float(beta), g_Ua.data_ptr(),
                                          _ld(g_Ua)), "gpp_rff_apply_grad")
        return g_Ua

    @_on_own_device
    def potrf(self, A, Linv, info, T=None):
        _need(A, torch.float64, "A"); _need(Linv, torch.float64, "Linv"); _need(info, torch.int32, "info")
        self._stream()
        if T is None:
            check(self.lib.gpp_potrf(self.h, A.data_ptr(), A.shape[0], _ld(A), Linv.data_ptr(), _ld(Linv), info.data_ptr()),
                  "gpp_potrf")
        else:
            check(self.lib.gpp_potrf_ws(self.h, A.data_ptr(), A.shape[0], _ld(A), Linv.data_ptr(), _ld(Linv), T.data_ptr(),
                                        _ld(T), info.data_ptr()), "gpp_potrf_ws")

    @_on_own_device
    def build_potrf(self, U, w, sf2, tau, grp, A, Linv, info, T, *, jitter=0.0, kind=KIND_RBF, d_split=0):
        """``kernel_build(..., uplo=UPLO_UPPER)`` into ``A`` followed by ``potrf(A, Linv, info, T)`` as ONE call
        (gpp_build_potrf_ws): the same bits; where the ticket list runs, most of Ky is built beside the first panel."""
        N, D = U.shape
        _check_features(D)
        for t, n in ((U, "U"), (w, "w"), (sf2, "sf2"), (A, "A"), (Linv, "Linv"), (T, "T")):
            _need(t, torch.float64, n)
        _need(info, torch.int32, "info")
        if tau is not None:
            _need(tau, torch.float64, "tau")
        S = 0 if tau is None else tau.numel()
        if grp is not None:
            self._check_groups(grp, N, S)
        if not U.is_contiguous():
            raise GppError("U must be contiguous")
        self._stream()
        check(self.lib.gpp_build_potrf_ws(self.h, U.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), _ptr(tau), _ptr(grp), S,
                                          float(jitter), kind, d_split, A.data_ptr(), _ld(A), Linv.data_ptr(), _ld(Linv),
                                          T.data_ptr(), _ld(T), info.data_ptr()), "gpp_build_potrf_ws")

    @_on_own_device
    def trtri(self, U, Linv, T):
        self._stream()
        check(self.lib.gpp_trtri(self.h, U.data_ptr(), U.shape[0], _ld(U), Linv.data_ptr(), _ld(Linv), T.data_ptr(), _ld(T)),
              "gpp_trtri")

    @_on_own_device
    def lauum(self, Linv, Kinv):
        self._stream()
        check(self.lib.gpp_lauum(self.h, Linv.data_ptr(), Linv.shape[0], _ld(Linv), Kinv.data_ptr(), _ld(Kinv)), "gpp_lauum")

    @_on_own_device
    def lauum_grad(self, Linv, U, w, sf2, grp, S, alpha, dU, g_w, g_sf2, g_tau, *, kind=KIND_RBF) -> bool:
        """LAUUM with the gradient reduction as its epilogue (gpp_lauum_grad): g_w, g_sf2, g_tau as ``lauum`` + ``grad_reduce``
        define them, without Ky^-1 in memory.  False: not supported for these arguments (kind, D > 16, dU > 0) — nothing was
        enqueued and the caller runs the pair."""
        N, D = U.shape
        for t, n in ((Linv, "Linv"), (U, "U"), (w, "w"), (sf2, "sf2"), (alpha, "alpha"), (g_w, "g_w"), (g_sf2, "g_sf2"),
                     (g_tau, "g_tau")):
            _need(t, torch.float64, n)
        if grp is not None:
            self._check_groups(grp, N, S)
        if not U.is_contiguous():
            raise GppError("U must be contiguous")
        self.ensure_workspace(OP_MLL_EVAL, N, 0, D, S)
        self._stream()
        status = self.lib.gpp_lauum_grad(self.h, Linv.data_ptr(), N, _ld(Linv), U.data_ptr(), D, w.data_ptr(), sf2.data_ptr(),
                                         _ptr(grp), S, kind, dU, alpha.data_ptr(), g_w.data_ptr(), g_sf2.data_ptr(),
                                         g_tau.data_ptr())
        if status == NOT_SUPPORTED:
            return False
        check(status, "gpp_lauum_grad")
        return True

    @_on_own_device
    def post_cov_train(self, Kinv, tau, grp, d, out, *, jitter=0.0):
        """out(upper) = diag(tau[grp] + d + jitter) - T Kinv T with T = diag(tau[grp]), from the lower triangle of Kinv
        (gpp_post_cov_train): the posterior covariance at the training inputs.  ``out`` may be ``Kinv`` itself."""
        N = Kinv.shape[0]
        for t, n in ((Kinv, "Kinv"), (tau, "tau"), (out, "A")):
            _need(t, torch.float64, n)
        if d is not None:
            _need(d, torch.float64, "d")
            if d.numel() != N or not d.is_contiguous():
                raise GppError(f"d must be a contiguous vector of {N} doubles")
        if grp is not None:
            self._check_groups(grp, N, tau.numel())
        if out.shape[0] != N or out.shape[1] != N:
            raise GppError("post_cov_train: shapes do not match")
        self._stream()
        check(self.lib.gpp_post_cov_train(self.h, Kinv.data_ptr(), N, _ld(Kinv), tau.data_ptr(), _ptr(grp), tau.numel(), _ptr(d),
                                          float(jitter), out.data_ptr(), _ld(out)), "gpp_post_cov_train")
        return out

    @_on_own_device
    def syrk_rows(self, Urow, C, nb, first_block, rank, nranks):
        """C(upper) -= Urow^T Urow on the block rows (height nb) of C this rank owns (block-cyclic), one launch."""
        self._stream()
        check(self.lib.gpp_syrk_rows(self.h, Urow.data_ptr(), _ld(Urow), C.data_ptr(), _ld(C), C.shape[0], Urow.shape[0], nb,
                                     first_block, rank, nranks), "gpp_syrk_rows")

    @_on_own_device
    def shard_list_begin(self, N, nb, rank, nranks, A, Kc, Lc, D, W, info, workers=0) -> bool:
        """Enqueue this rank's ticket list of the sharded factorisation + forward sweep (gpp_shard_list_begin in gpp.h).  False:
        not applicable here, nothing was enqueued."""
        self._stream()
        used = ctypes.c_int(0)
        check(self.lib.gpp_shard_list_begin(self.h, N, nb, rank, nranks, A.data_ptr(), _ld(A), Kc.data_ptr(), Lc.data_ptr(), _ld(Kc),
                                            D.data_ptr(), W[0].data_ptr(), W[1].data_ptr(), W[2].data_ptr(), _ld(W[0]),
                                            info.data_ptr(), int(workers), ctypes.byref(used)), "gpp_shard_list_begin")
        return bool(used.value)

    def shard_messages(self, N: int, nb: int, k: int):
        """Column ranges [(c0, c1), ...] of block row k's messages in the order they travel (gpp.h): the head — diagonal block and
        the next block's columns —, then the tail in pieces of ``gpp_shard_piece_cols()`` columns.  The index in the list is the
        ``tail`` argument of ``shard_list_gate`` / ``shard_list_signal``."""
        o, o2 = k * nb, min((k + 2) * nb, N)
        W = int(self.lib.gpp_shard_piece_cols()) or N
        return [(o, o2)] + [(c, min(c + W, N)) for c in range(o2, N, W)]

    @_on_own_device
    def shard_list_gate(self, stream, tail: int, k: int) -> None:
        check(self.lib.gpp_shard_list_gate(self.h, ctypes.c_void_p(stream.cuda_stream), int(tail), k), "gpp_shard_list_gate")

    @_on_own_device
    def shard_list_signal(self, stream, tail: int, k: int) -> None:
        check(self.lib.gpp_shard_list_signal(self.h, ctypes.c_void_p(stream.cuda_stream), int(tail), k), "gpp_shard_list_signal")

    @_on_own_device
    def shard_list_end(self) -> None:
        self._stream()
        check(self.lib.gpp_shard_list_end(self.h), "gpp_shard_list_end")

    @_on_own_device
    def shard_back_list(self, N, nb, rank, nranks, A, Kc, Lc, D, info, workers=0) -> bool:
        """The sharded back-substitution of this rank as one ticket list on the current stream (gpp_shard_back_list in gpp.h).
        False: not applicable here, nothing was enqueued."""
        self._stream()
        used = ctypes.c_int(0)
        check(self.lib.gpp_shard_back_list(self.h, N, nb, rank, nranks, A.data_ptr(), _ld(A), Kc.data_ptr(), Lc.data_ptr(), _ld(Kc),
                                           D.data_ptr(), info.data_ptr(), int(workers), ctypes.byref(used)), "gpp_shard_back_list")
        return bool(used.value)

    @_on_own_device
    def gemm_lower_cols(self, A, B, C, alpha, beta, nb, first_block, rank, nranks, row0=0, row1=None, compact=False):
        """C(lower, owned column blocks of width nb) = beta C + alpha A^T B;  A, B: K x M row-contiguous, C: M x M; rows
        [row0, row1) of C only.  ``compact``: B (K rows) and C (M rows) hold only the owned column blocks, side by side."""
        M, K = A.shape[1], A.shape[0]
        if compact:
            if B.shape[0] != K or C.shape[0] != M:
                raise GppError("gemm_lower_cols: shapes do not match")
        elif A.shape != B.shape or C.shape[0] != C.shape[1] or C.shape[0] != M:
            raise GppError("gemm_lower_cols: shapes do not match")
        self._stream()
        check(self.lib.gpp_gemm_lower_cols(self.h, A.data_ptr(), _ld(A), B.data_ptr(), _ld(B), C.data_ptr(), _ld(C), M,
                                           K, float(alpha), float(beta), nb, first_block, rank, nranks, row0,
                                           M if row1 is None else row1, 1 if compact else 0),
              "gpp_gemm_lower_cols")

    @_on_own_device
    def trmv_lower_cols(self, T, x, y, nb, rank, nranks, trans=False, compact=False):
        """y = (owned column blocks of lower T) x, or their transpose times x on the owned entries (0 elsewhere).
        ``compact``: T (N rows) holds only the owned column blocks, side by side."""
        for t, n in ((x, "x"), (y, "y")):
            _need(t, torch.float64, n)
        if trans:
            self.ensure_workspace(OP_MLL_EVAL, T.shape[0], 0, 1, 1)
        self._stream()
        check(self.lib.gpp_trmv_lower_cols(self.h, T.data_ptr(), _ld(T), T.shape[0], x.data_ptr(), y.data_ptr(), nb, rank, nranks,
                                           1 if trans else 0, 1 if compact else 0), "gpp_trmv_lower_cols")

    @_on_own_device
    def mll_scalars(self, U, z, out3):
        self._stream()
        check(self.lib.gpp_mll_scalars(self.h, U.data_ptr(), _ld(U), U.shape[0], z.data_ptr(), out3.data_ptr()), "gpp_mll_scalars")

    @_on_own_device
    def lauum_rows(self, Linv, Kinv, rank, nranks):
        """This rank's cyclic share (128-row tile rows) of Kinv = Linv^T Linv, one launch."""
        self._stream()
        check(self.lib.gpp_lauum_rows(self.h, Linv.data_ptr(), Linv.shape[0], _ld(Linv), Kinv.data_ptr(), _ld(Kinv), rank, nranks),
              "gpp_lauum_rows")

    @_on_own_device
    def lauum_rows_range(self, Linv, Kinv, rank, nranks, row0, row1):
        """The part of this rank's cyclic share of Kinv = Linv^T Linv inside rows [row0, row1) (needs the column blocks of
        Linv up to row1 only)."""
        self._stream()
        check(self.lib.gpp_lauum_rows_range(self.h, Linv.data_ptr(), Linv.shape[0], _ld(Linv), Kinv.data_ptr(), _ld(Kinv), rank,
                                            nranks, row0, row1), "gpp_lauum_rows_range")

    @_on_own_device
    def transpose(self, src, dst):
        """dst = src^T, out of place (2-D views with unit column stride)."""
        if src.shape[0] != dst.shape[1] or src.shape[1] != dst.shape[0]:
            raise GppError("transpose: shapes do not match")
        self._stream()
        check(self.lib.gpp_transpose(self.h, src.data_ptr(), src.stride(0), src.shape[0], src.shape[1], dst.data_ptr(), dst.stride(0)),
              "gpp_transpose")

    @_on_own_device
    def mll_reduce(self, L, Linv, r, z, out3):
        for t, n in ((r, "r"), (z, "z"), (out3, "out3")):
            _need(t, torch.float64, n)
        self._stream()
        check(self.lib.gpp_mll_reduce(self.h, L.data_ptr(), _ld(L), Linv.data_ptr(), _ld(Linv), L.shape[0], r.data_ptr(),
                                      z.data_ptr(), out3.data_ptr()), "gpp_mll_reduce")

    @_on_own_device
    def alpha(self, Linv, z, alpha):
        N = Linv.shape[0]
        self._stream()
        check(self.lib.gpp_alpha(self.h, Linv.data_ptr(), _ld(Linv), N, z.data_ptr(), alpha.data_ptr()), "gpp_alpha")

    @_on_own_device
    def grad_reduce(self, U, w, sf2, grp, S, alpha, Kinv, dU, g_w, g_sf2, g_tau, g_U, *, kind=KIND_RBF, d_split=0):
        N, D = U.shape
        if grp is not None:
            self._check_groups(grp, N, S)
        self.ensure_workspace(OP_MLL_EVAL, N, 0, D, S)
        self._stream()
        check(self.lib.gpp_grad_reduce(self.h, U.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), _ptr(grp), S, kind,
                                       d_split, alpha.data_ptr(), Kinv.data_ptr(), _ld(Kinv), dU, g_w.data_ptr(),
                                       g_sf2.data_ptr(), g_tau.data_ptr(), _ptr(g_U)), "gpp_grad_reduce")

    @_on_own_device
    def loo_scalars(self, Linv, alpha, y, d, mu=None, s2=None, a=None, sqrtb=None, loo=None):
        """Leave-one-out quantities from the inverse factor (gpp_loo_scalars): d = diag(Ky^-1) by row reductions of ``Linv``,
        and whichever of mu = y - alpha / d, s2 = 1 / d, a = -alpha / d, sqrtb and the pseudo-likelihood ``loo`` were passed."""
        N = Linv.shape[0]
        _need(Linv, torch.float64, "Linv")
        for t, n, size in ((alpha, "alpha", N), (y, "y", N), (d, "d", N), (mu, "mu", N), (s2, "s2", N), (a, "a", N),
                           (sqrtb, "sqrtb", N), (loo, "loo", 1)):
            if t is None:
                continue
            _need(t, torch.float64, n)
            if t.numel() < size or not t.is_contiguous():
                raise GppError(f"{n} must be a contiguous vector of {size} doubles")
        if mu is not None and y is None:
            raise GppError("loo_scalars: mu needs y")
        self._stream()
        check(self.lib.gpp_loo_scalars(self.h, Linv.data_ptr(), _ld(Linv), N, alpha.data_ptr(), _ptr(y), d.data_ptr(), _ptr(mu),
                                       _ptr(s2), _ptr(a), _ptr(sqrtb), _ptr(loo)), "gpp_loo_scalars")

    @_on_own_device
    def sym_rowscale(self, Kinv, s, out):
        """out[i, j] = s[i] * Kinv[max(i, j), min(i, j)]: the full row-scaled square from Kinv's lower triangle, out of place
        (gpp_sym_rowscale)."""
        N = Kinv.shape[0]
        for t, n in ((Kinv, "Kinv"), (s, "s"), (out, "S")):
            _need(t, torch.float64, n)
        if out.shape[0] != N or out.shape[1] != N or s.numel() != N or not s.is_contiguous():
            raise GppError("sym_rowscale: shapes do not match")
        if out.data_ptr() == Kinv.data_ptr():
            raise GppError("sym_rowscale works out of place")
        self._stream()
        check(self.lib.gpp_sym_rowscale(self.h, Kinv.data_ptr(), N, _ld(Kinv), s.data_ptr(), out.data_ptr(), _ld(out)),
              "gpp_sym_rowscale")
        return out

    @_on_own_device
    def loo_grad_reduce(self, U, w, sf2, grp, S, alpha, beta, C, dU, g_w, g_sf2, g_tau, g_U, *, kind=KIND_RBF, d_split=0):
        """``grad_reduce`` with the leave-one-out weights W = -(alpha beta^T + beta alpha^T) / 2 - C (gpp_loo_grad_reduce)."""
        N, D = U.shape
        _check_features(D)
        for t, n in ((alpha, "alpha"), (beta, "beta")):
            _need(t, torch.float64, n)
            if t.numel() != N or not t.is_contiguous():
                raise GppError(f"{n} must be a contiguous vector of {N} doubles")
        if grp is not None:
            self._check_groups(grp, N, S)
        self.ensure_workspace(OP_MLL_EVAL, N, 0, D, S)
        self._stream()
        check(self.lib.gpp_loo_grad_reduce(self.h, U.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), _ptr(grp), S, kind, d_split,
                                           alpha.data_ptr(), beta.data_ptr(), C.data_ptr(), _ld(C), dU, g_w.data_ptr(),
                                           g_sf2.data_ptr(), g_tau.data_ptr(), _ptr(g_U)), "gpp_loo_grad_reduce")

    @_on_own_device
    def calib_grad_reduce(self, U, w, sf2, alpha, Kinv, member, cols, g_theta, *, kind=KIND_RBF, d_split=0):
        """g_theta[k] = d MLL / d theta_k for calibration parameters written into feature column ``cols[k]`` of the rows with
        ``member[i] != 0``: the sum of ``grad_reduce``'s g_U[i, cols[k]] over those rows without the N x D block
        (gpp_calib_grad_reduce).  ``member`` (N,) and ``cols`` (C,) int32 on the GPU, ``Kinv`` as the LAUUM leaves it."""
        N, D = U.shape
        _check_features(D)
        C = int(cols.numel())
        for t, n, size in ((U, "U", N * D), (w, "w", D), (sf2, "sf2", 1), (alpha, "alpha", N), (g_theta, "g_theta", C)):
            _need(t, torch.float64, n)
            if t.numel() != size or not t.is_contiguous():
                raise GppError(f"{n} must be contiguous with {size} doubles")
        _need(Kinv, torch.float64, "Kinv")
        if Kinv.dim() != 2 or Kinv.shape[0] != N or Kinv.shape[1] != N:
            raise GppError(f"Kinv must be {N} x {N}")
        for t, n, size in ((member, "member", N), (cols, "cols", C)):
            _need(t, torch.int32, n)
            if t.dim() != 1 or t.numel() != size:
                raise GppError(f"{n} must be a vector of {size} int32")
        if C < 1 or C > D:
            raise GppError(f"1 <= C <= D calibrated columns (got C = {C}, D = {D})")
        # the value range costs a device read: once per index tensor, as for the noise groups
        seen = getattr(self, "_cols_ok", None)
        if seen is None or seen[0]() is not cols or seen[1:] != (cols._version, D):
            lo, hi = int(cols.min()), int(cols.max())
            if lo < 0 or hi >= D:
                raise GppError(f"calibrated feature column out of range: values in [{lo}, {hi}] for {D} feature columns")
            self._cols_ok = (weakref.ref(cols), cols._version, D)
        self.ensure_workspace(OP_MLL_EVAL, N, 0, D, 1)
        self._stream()
        check(self.lib.gpp_calib_grad_reduce(self.h, U.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), kind, d_split,
                                             alpha.data_ptr(), Kinv.data_ptr(), _ld(Kinv), member.data_ptr(), cols.data_ptr(), C,
                                             g_theta.data_ptr()), "gpp_calib_grad_reduce")

    @_on_own_device
    def grad_reduce_rows(self, U, w, sf2, grp, S, alpha, Kinv, dU, nb, rank, nranks, g_w, g_sf2, g_tau, g_U, *,
                         kind=KIND_RBF, d_split=0):
        """Partial sums over the block rows of Kinv owned by ``rank`` (block-cyclic, block height ``nb``)."""
        N, D = U.shape
        if grp is not None:
            self._check_groups(grp, N, S)
        self.ensure_workspace(OP_MLL_EVAL, N, 0, D, S)
        self._stream()
        check(self.lib.gpp_grad_reduce_rows(self.h, U.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), _ptr(grp), S, kind,
                                            d_split, alpha.data_ptr(), Kinv.data_ptr(), _ld(Kinv), dU, nb, rank, nranks,
                                            g_w.data_ptr(), g_sf2.data_ptr(), g_tau.data_ptr(), _ptr(g_U)),
              "gpp_grad_reduce_rows")

    @_on_own_device
    def grad_reduce_cols(self, U, w, sf2, grp, S, alpha, Kinv, dU, nb, rank, nranks, g_w, g_sf2, g_tau, g_U, *,
                         kind=KIND_RBF, d_split=0, compact=False):
        """Partial sums over the COLUMN blocks of Kinv's lower triangle owned by ``rank`` (block-cyclic, width ``nb``).
        ``compact``: Kinv (N rows) holds only the owned column blocks, side by side."""
        N, D = U.shape
        if grp is not None:
            self._check_groups(grp, N, S)
        self.ensure_workspace(OP_MLL_EVAL, N, 0, D, S)
        self._stream()
        check(self.lib.gpp_grad_reduce_cols(self.h, U.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), _ptr(grp), S, kind,
                                            d_split, alpha.data_ptr(), Kinv.data_ptr(), _ld(Kinv), dU, nb, rank, nranks,
                                            g_w.data_ptr(), g_sf2.data_ptr(), g_tau.data_ptr(), _ptr(g_U), 1 if compact else 0),
              "gpp_grad_reduce_cols")

    @_on_own_device
    def predict(self, Linv, alpha, Ksn, kss, V, mean_out, var_out):
        self._stream()
        check(self.lib.gpp_predict(self.h, Linv.data_ptr(), _ld(Linv), Linv.shape[0], alpha.data_ptr(), Ksn.data_ptr(),
                                   _ld(Ksn), Ksn.shape[0], _ptr(kss), _ptr(V), 0 if V is None else _ld(V),
                                   mean_out.data_ptr(), _ptr(var_out)), "gpp_predict")

    @_on_own_device
    def predict_tn(self, Linv, z, Kns, kss, V, mean_out, var_out):
        """Prediction from the transposed cross block Kns (N x M) and z = Linv r: mean, variance and V = Kns^T Linv^T."""
        self._stream()
        check(self.lib.gpp_predict_tn(self.h, Linv.data_ptr(), _ld(Linv), Linv.shape[0], z.data_ptr(), Kns.data_ptr(), _ld(Kns),
                                      Kns.shape[1], kss.data_ptr(), V.data_ptr(), _ld(V), mean_out.data_ptr(), var_out.data_ptr()),
              "gpp_predict_tn")

    @_on_own_device
    def cross_grad(self, Ua, Ub, w, sf2, gmean, alpha, gvar, B, g_Ua, g_Ub, g_w, g_sf2, *, kind=KIND_RBF, d_split=0):
        """Backward of a prediction from the test / training features Ua (M x D) and Ub (N x D): with G = gmean alpha^T +
        diag(gvar) B and K = sf2 k(Ua, Ub; w), g_Ua = G dK/dUa (M x dA), g_Ub = G^T dK/dUb (N x dB), g_w, g_sf2 (gpp_cross_grad).
        Either input pair may be None, and so may every output (dA / dB are the outputs' widths)."""
        M, D = Ua.shape
        N = Ub.shape[0]
        _check_features(D)
        for t, n in ((Ua, "Ua"), (Ub, "Ub"), (w, "w"), (sf2, "sf2")):
            _need(t, torch.float64, n)
        if not (Ua.is_contiguous() and Ub.is_contiguous()):
            raise GppError("Ua/Ub must be contiguous")
        for t, n in ((gmean, "gmean"), (alpha, "alpha"), (gvar, "gvar"), (g_w, "g_w"), (g_sf2, "g_sf2")):
            if t is not None:
                _need(t, torch.float64, n)
        dA = 0 if g_Ua is None else g_Ua.shape[1]
        dB = 0 if g_Ub is None else g_Ub.shape[1]
        for t, rows, n in ((g_Ua, M, "g_Ua"), (g_Ub, N, "g_Ub")):
            if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.shape[0] != rows):
                raise GppError(f"{n} must be a contiguous float64 ({rows} x d) matrix")
        self.ensure_workspace(OP_PREDICT_GRAD, N, M, D, dB)
        self._stream()
        check(self.lib.gpp_cross_grad(self.h, Ua.data_ptr(), M, Ub.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), kind, d_split,
                                      _ptr(gmean), _ptr(alpha), _ptr(gvar), _ptr(B), 0 if B is None else _ld(B), _ptr(g_Ua), dA,
                                      _ptr(g_Ub), dB, _ptr(g_w), _ptr(g_sf2)), "gpp_cross_grad")

    @_on_own_device
    def gemm(self, transA, transB, M, N, K, alpha, A, B, beta, C, *, a_mask=0, b_mask=0, klo_mode=0, khi_mode=0,
             c_tri=0):
        self._stream()
        check(self.lib.gpp_gemm(self.h, transA, transB, M, N, K, float(alpha), A.data_ptr(), _ld(A), B.data_ptr(), _ld(B),
                                float(beta), C.data_ptr(), _ld(C), a_mask, b_mask, klo_mode, khi_mode, c_tri), "gpp_gemm")

    @_on_own_device
    def gemm_batched(self, transA, transB, M, N, K, alpha, A, sA, B, sB, beta, C, sC, batch, *, a_mask=0, b_mask=0,
                     klo_mode=0, khi_mode=0, c_tri=0):
        """``batch`` products of one shape; A/B/C are the first elements' views, sA/sB/sC element strides between them."""
        self._stream()
        check(self.lib.gpp_gemm_batched(self.h, transA, transB, M, N, K, float(alpha), A.data_ptr(), _ld(A), sA, B.data_ptr(),
                                        _ld(B), sB, float(beta), C.data_ptr(), _ld(C), sC, batch, a_mask, b_mask, klo_mode,
                                        khi_mode, c_tri), "gpp_gemm_batched")

    # -- batched evaluation: tensors carry a leading batch dimension -------------------------------------------
    # matrices: (B, N, ld) views of a (B, N, ld) allocation ([:, :, :N]); vectors: (B, N) views of a (B, sv) allocation
    # with sv even (``batched_vector``); parameters (B, D), (B,), (B, S)
    def batched_buffer(self, B: int, n: int) -> torch.Tensor:
        return torch.empty((B, n, row_stride(n)), dtype=torch.float64, device=self.device)[:, :, :n]

    def batched_vector(self, B: int, n: int) -> torch.Tensor:
        return torch.empty((B, n + (n & 1)), dtype=torch.float64, device=self.device)[:, :n]

    @_on_own_device
    def ensure_workspace_batched(self, B, N, D, S):
        need = B * int(self.lib.gpp_workspace_bytes(self.h, OP_MLL_EVAL, N, 0, D, S))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            check(self.lib.gpp_set_workspace(self.h, self._ws.data_ptr(), self._ws.numel()), "gpp_set_workspace")

    @_on_own_device
    def kernel_build_batched(self, U, w, sf2, tau, grp, out, *, jitter=0.0, kind=KIND_RBF, d_split=0, uplo=UPLO_FULL):
        """U: (N, D) shared or (B, N, D); w: (B, D); sf2: (B,); tau: (B, S) or None; out: (B, N, ld) view."""
        B, N = out.shape[0], out.shape[1]
        D = w.shape[1]
        sU = 0 if U.dim() == 2 else U.stride(0)
        S = 0 if tau is None else tau.shape[1]
        if grp is not None and grp.numel() != N:  # (the kernels index grp[i] unchecked; the value range is _check_groups' matter)
            raise GppError(f"noise-group index has {grp.numel()} entries for {N} points (stale fidel_indices?)")
        self._stream()
        check(self.lib.gpp_kernel_build_batched(self.h, U.data_ptr(), sU, N, D, w.data_ptr(), sf2.data_ptr(), _ptr(tau),
                                                _ptr(grp), S, float(jitter), kind, d_split, uplo, out.data_ptr(), out.stride(1),
                                                out.stride(0), B), "gpp_kernel_build_batched")

    @_on_own_device
    def potrf_batched(self, A, Linv, info):
        self._stream()
        check(self.lib.gpp_potrf_batched(self.h, A.data_ptr(), A.shape[1], A.stride(1), A.stride(0), Linv.data_ptr(),
                                         Linv.stride(1), Linv.stride(0), info.data_ptr(), A.shape[0]), "gpp_potrf_batched")

    @_on_own_device
    def trtri_batched(self, U, Linv, T):
        self._stream()
        check(self.lib.gpp_trtri_batched(self.h, U.data_ptr(), U.shape[1], U.stride(1), U.stride(0), Linv.data_ptr(),
                                         Linv.stride(1), Linv.stride(0), T.data_ptr(), T.stride(1), T.stride(0), U.shape[0]),
              "gpp_trtri_batched")

    @_on_own_device
    def lauum_batched(self, Linv, Kinv):
        self._stream()
        check(self.lib.gpp_lauum_batched(self.h, Linv.data_ptr(), Linv.shape[1], Linv.stride(1), Linv.stride(0), Kinv.data_ptr(),
                                         Kinv.stride(1), Kinv.stride(0), Linv.shape[0]), "gpp_lauum_batched")

    @_on_own_device
    def mll_reduce_batched(self, L, Linv, r, z, out3):
        self._stream()
        check(self.lib.gpp_mll_reduce_batched(self.h, L.data_ptr(), L.stride(1), L.stride(0), Linv.data_ptr(), Linv.stride(1),
                                              Linv.stride(0), L.shape[1], r.data_ptr(), z.data_ptr(), self._sv(r, z), out3.data_ptr(),
                                              L.shape[0]), "gpp_mll_reduce_batched")

    @staticmethod
    def _sv(*vecs):
        sv = vecs[0].stride(0)
        if any(v.stride(0) != sv or v.stride(1) != 1 for v in vecs) or (sv & 1):
            raise GppError("batched vectors must share one even row stride (use GppContext.batched_vector)")
        return sv

    @_on_own_device
    def alpha_batched(self, Linv, z, alpha):
        self._stream()
        check(self.lib.gpp_alpha_batched(self.h, Linv.data_ptr(), Linv.stride(1), Linv.stride(0), Linv.shape[1], z.data_ptr(),
                                         alpha.data_ptr(), self._sv(z, alpha), Linv.shape[0]), "gpp_alpha_batched")

    def _ensemble_lib(self):
        """``libgpp_ensemble_hip.so`` (include/gpp_ensemble.h): gpp_predict_gen and gpp_predict_gen_batched, on this context's handle."""
        if getattr(self, "elib", None) is None:
            self.elib = _lib.load_ensemble()
        return self.elib

    def _ensure_predict_gen_workspace(self, N: int, M: int, batch: int) -> None:
        need = int(self._ensemble_lib().gpp_predict_gen_workspace_bytes(N, M, batch)) + 256
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            check(self.lib.gpp_set_workspace(self.h, self._ws.data_ptr(), self._ws.numel()), "gpp_set_workspace")

    @_on_own_device
    def predict_gen(self, Ua, Ub, w, sf2, Linv, z, mean_out, var_out, *, kind=KIND_RBF, d_split=0):
        """mean = V z and var = sf2 - rowsum(V o V), V = sf2 k(Ua, Ub; w) L^-T, from the mirror in the upper triangle of ``Linv``
        (N x N view of an even-stride buffer) and z = Linv r, without forming the cross block or V (gpp_predict_gen)."""
        (M, D), N = Ua.shape, Ub.shape[0]
        _check_features(D)
        for t, n in ((Ua, "Ua"), (Ub, "Ub"), (w, "w"), (sf2, "sf2"), (Linv, "Linv"), (z, "z"), (mean_out, "mean_out"), (var_out, "var_out")):
            _need(t, torch.float64, n)
        if not (Ua.is_contiguous() and Ub.is_contiguous()):
            raise GppError("Ua/Ub must be contiguous")
        if Ub.shape[1] != D or w.numel() != D or sf2.numel() < 1 or min(M, N) < 1:
            raise GppError(f"gpp_predict_gen takes Ua (M, D), Ub (N, D), w (D), sf2 (1) with M, N >= 1 (got {tuple(Ua.shape)}, "
                           f"{tuple(Ub.shape)}, {w.numel()}, {sf2.numel()})")
        if Linv.shape != (N, N) or z.numel() != N or mean_out.numel() != M or var_out.numel() != M:
            raise GppError(f"gpp_predict_gen: Linv must be {N} x {N}, z ({N}), mean_out / var_out ({M})")
        if not (z.is_contiguous() and mean_out.is_contiguous() and var_out.is_contiguous()):
            raise GppError("z, mean_out and var_out must be contiguous")
        self._ensure_predict_gen_workspace(N, M, 1)
        self._stream()
        check(self._ensemble_lib().gpp_predict_gen(self.h, Ua.data_ptr(), M, Ub.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), kind, d_split,
                                       Linv.data_ptr(), _ld(Linv), z.data_ptr(), mean_out.data_ptr(), var_out.data_ptr()),
              "gpp_predict_gen")

    @_on_own_device
    def predict_gen_batched(self, Ua, Ub, w, sf2, Linv, z, mean_out, var_out, *, kind=KIND_RBF, d_split=0):
        """``predict_gen`` for B parameter sets in one launch (gpp_predict_gen_batched).  Ua: (M, D) shared or (B, M, D); Ub: (N, D)
        shared or (B, N, D); w: (B, D); sf2: (B,); Linv: (B, N, ld) view; z: (B, N) and mean_out / var_out: (B, M) views of
        even-stride allocations (``batched_vector``)."""
        B, D = w.shape
        M, N = Ua.shape[-2], Ub.shape[-2]
        _check_features(D)
        for t, n in ((Ua, "Ua"), (Ub, "Ub"), (w, "w"), (sf2, "sf2"), (Linv, "Linv"), (z, "z"), (mean_out, "mean_out"), (var_out, "var_out")):
            _need(t, torch.float64, n)
        for t, rows, n in ((Ua, M, "Ua"), (Ub, N, "Ub")):
            if t.dim() not in (2, 3) or t.shape[-1] != D or rows < 1 or (t.dim() == 3 and t.shape[0] != B):
                raise GppError(f"{n} must be (rows, {D}) or ({B}, rows, {D}) with at least one row (got {tuple(t.shape)})")
            if t.stride(-1) != 1 or t.stride(-2) != D:
                raise GppError(f"the rows of {n} must be contiguous")
        if not w.is_contiguous() or sf2.numel() != B or not sf2.is_contiguous():
            raise GppError(f"w must be a contiguous ({B}, {D}) tensor and sf2 a contiguous ({B},) one")
        if Linv.shape != (B, N, N) or Linv.stride(2) != 1:
            raise GppError(f"Linv must be a ({B}, {N}, {N}) view with contiguous rows (got {tuple(Linv.shape)})")
        if z.shape != (B, N) or mean_out.shape != (B, M) or var_out.shape != (B, M):
            raise GppError(f"z must be ({B}, {N}), mean_out / var_out ({B}, {M})")
        sUa = 0 if Ua.dim() == 2 else Ua.stride(0)
        sUb = 0 if Ub.dim() == 2 else Ub.stride(0)
        sv, so = self._sv(z), self._sv(mean_out, var_out)
        self._ensure_predict_gen_workspace(N, M, B)
        self._stream()
        check(self._ensemble_lib().gpp_predict_gen_batched(self.h, Ua.data_ptr(), sUa, M, Ub.data_ptr(), sUb, N, D, w.data_ptr(), sf2.data_ptr(),
                                               kind, d_split, Linv.data_ptr(), Linv.stride(1), Linv.stride(0), z.data_ptr(), sv,
                                               mean_out.data_ptr(), var_out.data_ptr(), so, B), "gpp_predict_gen_batched")

    @_on_own_device
    def grad_reduce_batched(self, U, w, sf2, grp, S, alpha, Kinv, dU, g_w, g_sf2, g_tau, g_U, *, kind=KIND_RBF, d_split=0):
        B, N = Kinv.shape[0], Kinv.shape[1]
        D = w.shape[1]
        sU = 0 if U.dim() == 2 else U.stride(0)
        self.ensure_workspace_batched(B, N, D, S)
        self._stream()
        check(self.lib.gpp_grad_reduce_batched(self.h, U.data_ptr(), sU, N, D, w.data_ptr(), sf2.data_ptr(), _ptr(grp), S, kind,
                                               d_split, alpha.data_ptr(), self._sv(alpha), Kinv.data_ptr(), Kinv.stride(1),
                                               Kinv.stride(0), dU,
                                               g_w.data_ptr(), g_sf2.data_ptr(), g_tau.data_ptr(), _ptr(g_U), B),
              "gpp_grad_reduce_batched")

    @_on_own_device
    def loo_scalars_batched(self, Linv, alpha, y, d, mu=None, s2=None, a=None, sqrtb=None, loo=None):
        """``loo_scalars`` for B problems in one launch: Linv (B, N, ld) view; alpha, y, d, mu, s2, a, sqrtb (B, N) views that share
        one even row stride (``batched_vector``); loo (B,) contiguous.  y, mu, s2, a, sqrtb and loo may each be None."""
        B, N = Linv.shape[0], Linv.shape[1]
        _need(Linv, torch.float64, "Linv")
        vecs = [(t, n) for t, n in ((alpha, "alpha"), (y, "y"), (d, "d"), (mu, "mu"), (s2, "s2"), (a, "a"), (sqrtb, "sqrtb"))
                if t is not None]
        for t, n in vecs:
            _need(t, torch.float64, n)
            if t.dim() != 2 or t.shape[0] != B or t.shape[1] != N:
                raise GppError(f"{n} must be a ({B}, {N}) batched vector")
        if mu is not None and y is None:
            raise GppError("loo_scalars_batched: mu needs y")
        if loo is not None:
            _need(loo, torch.float64, "loo")
            if loo.numel() < B or not loo.is_contiguous():
                raise GppError(f"loo must be a contiguous vector of {B} doubles")
        self._stream()
        check(self.lib.gpp_loo_scalars_batched(self.h, Linv.data_ptr(), Linv.stride(1), Linv.stride(0), N, alpha.data_ptr(), _ptr(y),
                                               d.data_ptr(), _ptr(mu), _ptr(s2), _ptr(a), _ptr(sqrtb), self._sv(*(t for t, _ in vecs)),
                                               _ptr(loo), B), "gpp_loo_scalars_batched")

    @_on_own_device
    def sym_rowscale_batched(self, Kinv, s, out):
        """``sym_rowscale`` for B problems in one launch: Kinv and out (B, N, ld) views, s a (B, N) batched vector."""
        B, N = Kinv.shape[0], Kinv.shape[1]
        for t, n in ((Kinv, "Kinv"), (s, "s"), (out, "S")):
            _need(t, torch.float64, n)
        if tuple(out.shape) != (B, N, N) or tuple(s.shape) != (B, N):
            raise GppError("sym_rowscale_batched: shapes do not match")
        if out.data_ptr() == Kinv.data_ptr():
            raise GppError("sym_rowscale works out of place")
        self._stream()
        check(self.lib.gpp_sym_rowscale_batched(self.h, Kinv.data_ptr(), N, Kinv.stride(1), Kinv.stride(0), s.data_ptr(), self._sv(s),
                                                out.data_ptr(), out.stride(1), out.stride(0), B), "gpp_sym_rowscale_batched")
        return out

    @_on_own_device
    def loo_grad_reduce_batched(self, U, w, sf2, grp, S, alpha, beta, C, dU, g_w, g_sf2, g_tau, g_U, *, kind=KIND_RBF, d_split=0):
        """``grad_reduce_batched`` with the leave-one-out weights of ``loo_grad_reduce``: beta (B, N) beside alpha, C (B, N, ld)."""
        B, N = C.shape[0], C.shape[1]
        D = w.shape[1]
        _check_features(D)
        sU = 0 if U.dim() == 2 else U.stride(0)
        self.ensure_workspace_batched(B, N, D, S)
        self._stream()
        check(self.lib.gpp_loo_grad_reduce_batched(self.h, U.data_ptr(), sU, N, D, w.data_ptr(), sf2.data_ptr(), _ptr(grp), S, kind,
                                                   d_split, alpha.data_ptr(), beta.data_ptr(), self._sv(alpha, beta), C.data_ptr(),
                                                   C.stride(1), C.stride(0), dU, g_w.data_ptr(), g_sf2.data_ptr(), g_tau.data_ptr(),
                                                   _ptr(g_U), B), "gpp_loo_grad_reduce_batched")


    # -- grouped cross-validation: ragged lists of folds as CSR (idx ascending inside a fold, off with nfolds + 1 entries) ------
    def _check_csr(self, idx, off, N: int, mp: int) -> Tuple[int, int]:
        """The kernels trust the CSR list: they gather rows idx[.] unchecked, walk m_f = off[f + 1] - off[f] entries of a fold and
        (gpp_cv_rows) write the rows off[f] + a.  Shapes are verified on every call, the CONTENTS once per pair of index tensors
        (a device read, i.e. a host sync; remembered per index tensor OBJECT, as ``_check_groups`` does): offsets ascending inside idx, every fold at most ``mp``
        rows, every index in [0, N) and ascending inside its fold.  Returns (nfolds, the largest offset)."""
        for t, n in ((idx, "idx"), (off, "off")):
            _need(t, torch.int32, n)
            if t.dim() != 1 or not t.is_contiguous():
                raise GppError(f"{n} must be a contiguous int32 vector")
        if off.numel() < 1:
            raise GppError("off must hold nfolds + 1 entries")
        nfolds = off.numel() - 1
        cache = self.__dict__.setdefault("_csr_ok", {})  # id(off) -> (idx, off as weak references, what was checked, largest offset)
        key = (idx._version, off._version, N, mp)
        seen = cache.get(id(off))
        if seen is not None and seen[0]() is idx and seen[1]() is off and seen[2] == key:
            return nfolds, seen[3]
        for k in [k for k, v in cache.items() if v[0]() is None or v[1]() is None]:
            del cache[k]  # (lists whose tensors are gone: an evaluation keeps one entry per bucket of its folds alive)
        o, i = off.cpu().numpy().astype("int64"), idx.cpu().numpy().astype("int64")
        sizes = o[1:] - o[:-1]
        if o[0] < 0 or (sizes < 0).any() or o[-1] > i.shape[0]:
            raise GppError(f"fold offsets must ascend from >= 0 to at most the {i.shape[0]} entries of idx")
        if nfolds and int(sizes.max()) > mp:
            raise GppError(f"a fold of {int(sizes.max())} rows does not fit the {mp} x {mp} blocks of this call")
        used = i[o[0]:o[-1]]
        if used.shape[0] and (int(used.min()) < 0 or int(used.max()) >= N):
            raise GppError(f"fold index out of range: values in [{int(used.min())}, {int(used.max())}] for {N} rows")
        if used.shape[0] > 1:
            inner = used[1:] > used[:-1]
            inner[(o[1:-1] - o[0] - 1)[(o[1:-1] > o[0]) & (o[1:-1] < o[-1])]] = True  # (a fold's first entry follows another fold's last)
            if not inner.all():
                raise GppError("fold indices must be strictly ascending inside every fold")
        cache[id(off)] = (weakref.ref(idx), weakref.ref(off), key, int(o[-1]))
        return nfolds, int(o[-1])

    @_on_own_device
    def cv_blocks(self, Linv, idx, off, out):
        """The upper triangles of P_FF = (Ky^-1)[F, F] for every fold of the CSR list, identity-padded to out's (nfolds, mp, mp)
        blocks, from the rows of the inverse factor with its mirror (gpp_cv_blocks).  ``out``: a ``batched_buffer`` view."""
        _need(Linv, torch.float64, "Linv"); _need(out, torch.float64, "B")
        if Linv.dim() != 2 or Linv.shape[0] != Linv.shape[1]:
            raise GppError("cv_blocks: Linv must be square")
        if out.dim() != 3 or out.shape[1] != out.shape[2] or out.stride(2) != 1:
            raise GppError("cv_blocks: B must be a (nfolds, mp, mp) batched matrix")
        nfolds, _ = self._check_csr(idx, off, Linv.shape[0], out.shape[1])
        if out.shape[0] != nfolds:
            raise GppError(f"cv_blocks: B holds {out.shape[0]} blocks for {nfolds} folds")
        self._stream()
        check(self.lib.gpp_cv_blocks(self.h, Linv.data_ptr(), _ld(Linv), Linv.shape[0], idx.data_ptr(), off.data_ptr(), nfolds,
                                     out.shape[1], out.data_ptr(), out.stride(1), out.stride(0)), "gpp_cv_blocks")
        return out

    @_on_own_device
    def cv_rows(self, G, idx, off, Psq, S):
        """S[off[f] + a, :] = sum_b G[f, a, b] Psq[idx[off[f] + b], :] for every fold of the CSR list (gpp_cv_rows).  G: (nfolds,
        mp, mp) batched matrix whose padding is not read (no fold longer than mp); Psq: the full symmetric N x N square; S: at least
        off[-1] rows of N."""
        for t, n in ((G, "G"), (Psq, "Psq"), (S, "S")):
            _need(t, torch.float64, n)
        if G.dim() != 3 or G.shape[1] != G.shape[2] or G.stride(2) != 1 or G.stride(1) < G.shape[2] \
                or (G.shape[0] > 1 and G.stride(0) < G.shape[1] * G.stride(1)):
            raise GppError("cv_rows: G must be a (nfolds, mp, mp) batched matrix")
        N = Psq.shape[0]
        if Psq.dim() != 2 or S.dim() != 2 or Psq.shape[1] != N or S.shape[1] != N:
            raise GppError("cv_rows: Psq must be N x N and S must have N columns")
        nfolds, rows = self._check_csr(idx, off, N, G.shape[1])
        if G.shape[0] != nfolds:
            raise GppError(f"cv_rows: G holds {G.shape[0]} blocks for {nfolds} folds")
        if S.shape[0] < rows:
            raise GppError(f"cv_rows: S has {S.shape[0]} rows, the folds write up to row {rows}")
        self._stream()
        check(self.lib.gpp_cv_rows(self.h, G.data_ptr(), G.stride(1), G.stride(0), idx.data_ptr(), off.data_ptr(), nfolds,
                                   Psq.data_ptr(), _ld(Psq), N, S.data_ptr(), _ld(S)), "gpp_cv_rows")
        return S

    # -- bordering a cached factorisation --------------------------------------------------------------------------------------
    @_on_own_device
    def chol_append(self, A, Linv, N, q, k, C, rq, z, alpha, info):
        """Border the N x N factorisation held in the leading windows of the buffers ``A`` (upper factor) and ``Linv`` (inverse
        factor with its mirror) with q new points (gpp_chol_append): k the N x q cross block, C the q x q corner (upper), rq the new
        residuals; z and alpha hold N entries and have room for N + q.  Everything is checked before any launch."""
        N, q = int(N), int(q)
        if N < 1 or q < 1:
            raise GppError(f"chol_append needs N >= 1 cached and q >= 1 new points (got {N}, {q})")
        for t, n in ((A, "A"), (Linv, "Linv"), (k, "k"), (C, "C"), (rq, "rq"), (z, "z"), (alpha, "alpha")):
            _need(t, torch.float64, n)
        _need(info, torch.int32, "info")
        for t, n, rows, cols in ((A, "A", N + q, N + q), (Linv, "Linv", N + q, N + q), (k, "k", N, q), (C, "C", q, q)):
            if t.dim() != 2 or t.stride(1) != 1:
                raise GppError(f"{n} must be 2-D with unit column stride")
            if (n in ("A", "Linv") and (t.shape[0] < rows or t.shape[1] < cols)) or (n in ("k", "C") and tuple(t.shape) != (rows, cols)):
                raise GppError(f"{n} is {tuple(t.shape)}: chol_append with N = {N}, q = {q} needs "
                               f"{'at least ' if n in ('A', 'Linv') else ''}{rows} x {cols}")
            ld = _ld(t)
            if ld & 1 or ld < cols:
                raise GppError(f"{n}: the leading dimension ({ld}) must be even and at least {cols}")
            if t.data_ptr() & 15:
                raise GppError(f"{n} must be 16-byte aligned")
        if rq.dim() != 1 or rq.numel() != q or not rq.is_contiguous():
            raise GppError(f"rq must be a contiguous vector of {q} doubles")
        for t, n in ((z, "z"), (alpha, "alpha")):
            if t.dim() != 1 or t.numel() < N + q or not t.is_contiguous():
                raise GppError(f"{n} must be a contiguous vector with room for {N + q} doubles (got {t.numel()})")
        if info.numel() < 1:
            raise GppError("info must hold one int32")
        self.ensure_workspace(OP_APPEND, N, q, 0, 0)
        self._stream()
        status = self.lib.gpp_chol_append(self.h, A.data_ptr(), _ld(A), Linv.data_ptr(), _ld(Linv), N, q, k.data_ptr(), _ld(k),
                                          C.data_ptr(), _ld(C), rq.data_ptr(), z.data_ptr(), alpha.data_ptr(), info.data_ptr())
        check(status, "gpp_chol_append")

    # -- expected variance reduction ---------------------------------------------------------------------------------------------
    @_on_own_device
    def post_cross_sq(self, Uc, Ur, w, sf2, Vc, Vr, K, out, *, omega=None, kind=KIND_RBF, d_split=0, transposed=False):
        """out[c] = sum_r omega_r (sf2 k(Uc_c, Ur_r; w) - sum_{n < K} Vc[c, n] Vr[r, n])^2 without forming the M_c x M_r block
        (gpp_post_cross_sq).  ``Vc`` / ``Vr``: M_c x (>= K) and M_r x (>= K) windows of row-major buffers, or with ``transposed`` the
        (>= K) x M_c and (>= K) x M_r windows of the transposed operands; what lies beyond K is not read.  ``omega``: M_r weights or
        None for all ones.  Everything is checked before any launch."""
        K = int(K)
        Mc, Mr, D = _post_cross_checks("post_cross_sq", "c", dict(Uc=Uc, Ur=Ur, w=w, sf2=sf2, Vc=Vc, Vr=Vr, out=out), K, kind, d_split,
                                       transposed, omega)
        if out.dim() != 1 or out.numel() < Mc or not out.is_contiguous():
            raise GppError(f"out must be a contiguous vector with room for {Mc} doubles (got {out.numel()})")
        self.ensure_workspace(OP_POST_CROSS, Mr, Mc, 0, 0)
        self._stream()
        status = self.lib.gpp_post_cross_sq(self.h, Uc.data_ptr(), Mc, Ur.data_ptr(), Mr, D, w.data_ptr(), sf2.data_ptr(), int(kind),
                                            int(d_split), Vc.data_ptr(), _ld(Vc), Vr.data_ptr(), _ld(Vr), K, 1 if transposed else 0,
                                            _ptr(omega), out.data_ptr())
        check(status, "gpp_post_cross_sq")
        return out

    @_on_own_device
    def post_cross_lin_sq(self, Uf, Ur, w, sf2, A, d0, nd, Vf, Vr, K, out, *, omega=None, kind=KIND_RBF, d_split=0, transposed=False):
        """``post_cross_sq`` for rows that observe a linear functional of f at their point (gpp_post_cross_lin_sq): row i is
        A[i, 0] f + sum_{j < nd} A[i, 1 + j] df/du_{d0 + j} at Uf_i, and out[i] = sum_r omega_r (its prior covariance with f(Ur_r)
        - sum_{n < K} Vf[i, n] Vr[r, n])^2.  ``A``: M_f x (>= 1 + nd) window of a row-major buffer; what lies beyond 1 + nd is not
        read.  ``Vf`` / ``Vr``, ``transposed`` and ``omega`` as in ``post_cross_sq``.  Everything is checked before any launch."""
        K, d0, nd = int(K), int(d0), int(nd)

        def functionals(Mf, D):
            if d0 < 0 or nd < 1 or d0 + nd > D:
                raise GppError(f"the observed directions [{d0}, {d0 + nd}) must be a non-empty range inside the {D} features")
            if A.dim() != 2 or A.stride(1) != 1 or A.shape[0] != Mf or A.shape[1] < 1 + nd or (Mf > 1 and _ld(A) < 1 + nd):
                raise GppError(f"A is {tuple(A.shape)}: {Mf} functionals of {nd} directions need {Mf} x at least {1 + nd}, "
                               "unit column stride")

        Mf, Mr, D = _post_cross_checks("post_cross_lin_sq", "f", dict(Uf=Uf, Ur=Ur, w=w, sf2=sf2, A=A, Vf=Vf, Vr=Vr, out=out), K, kind,
                                       d_split, transposed, omega, own=functionals)
        if out.dim() != 1 or out.numel() < Mf or not out.is_contiguous():
            raise GppError(f"out must be a contiguous vector with room for {Mf} doubles (got {out.numel()})")
        self.ensure_workspace(OP_POST_CROSS_LIN, Mr, Mf, 0, 0)
        self._stream()
        status = self.lib.gpp_post_cross_lin_sq(self.h, Uf.data_ptr(), Mf, Ur.data_ptr(), Mr, D, w.data_ptr(), sf2.data_ptr(),
                                                int(kind), int(d_split), d0, nd, A.data_ptr(), max(_ld(A), 1 + nd), Vf.data_ptr(),
                                                _ld(Vf), Vr.data_ptr(), _ld(Vr), K, 1 if transposed else 0, _ptr(omega),
                                                out.data_ptr())
        check(status, "gpp_post_cross_lin_sq")
        return out

    # -- knowledge gradient ------------------------------------------------------------------------------------------------------
    @_on_own_device
    def post_cross_min(self, Uc, Ur, w, sf2, Vc, Vr, K, m, scale, nodes, out, *, kind=KIND_RBF, d_split=0, transposed=False):
        """out[c, k] = min_r (m_r + nodes_k scale_c (sf2 k(Uc_c, Ur_r; w) - sum_{n < K} Vc[c, n] Vr[r, n])) without forming the
        M_c x M_r block (gpp_post_cross_min).  ``Vc`` / ``Vr`` and ``transposed`` as in ``post_cross_sq``; ``m``: M_r offsets,
        ``scale``: M_c factors, ``nodes``: 1..64 values, ``out``: a contiguous M_c x Q matrix.  Everything is checked before any
        launch."""
        K = int(K)
        Mc, Mr, D = _post_cross_checks("post_cross_min", "c", dict(Uc=Uc, Ur=Ur, w=w, sf2=sf2, Vc=Vc, Vr=Vr, m=m, scale=scale, nodes=nodes,
                                                                   out=out), K, kind, d_split, transposed)
        if nodes.dim() != 1 or not (1 <= nodes.numel() <= MAX_NODES) or not nodes.is_contiguous():
            raise GppError(f"nodes must be a contiguous vector of 1..{MAX_NODES} values (got {tuple(nodes.shape)})")
        Q = nodes.numel()
        for t, n, pts in ((m, "m", Mr), (scale, "scale", Mc)):
            if t.dim() != 1 or t.numel() != pts or not t.is_contiguous():
                raise GppError(f"{n} must be a contiguous vector of {pts} values (got {tuple(t.shape)})")
        if out.dim() != 2 or out.shape[0] < Mc or out.shape[1] != Q or not out.is_contiguous():
            raise GppError(f"out must be a contiguous matrix of (at least) {Mc} x {Q} doubles (got {tuple(out.shape)})")
        self.ensure_workspace(OP_POST_CROSS_MIN, Mr, Mc, 0, Q)
        self._stream()
        status = self.lib.gpp_post_cross_min(self.h, Uc.data_ptr(), Mc, Ur.data_ptr(), Mr, D, w.data_ptr(), sf2.data_ptr(), int(kind),
                                             int(d_split), Vc.data_ptr(), _ld(Vc), Vr.data_ptr(), _ld(Vr), K, 1 if transposed else 0,
                                             m.data_ptr(), scale.data_ptr(), nodes.data_ptr(), Q, out.data_ptr())
        check(status, "gpp_post_cross_min")
        return out

    # -- the derivative blocks: posterior of the gradient, conditioning and training on gradient observations ---------------------
    # (one problem per call, or B in one launch each for batched.BatchedGEKFunction: the checks below serve both)
    @staticmethod
    def _dx_rows(name, t, B, D):
        """One side's feature rows: a contiguous (M, D) matrix or, in a batched call (``B`` not None), (B, M, D) with each element's
        block contiguous; returns (M, batch stride), the stride 0 for a matrix (which every element of a batch then shares)."""
        _need(t, torch.float64, name)
        if t.dim() == 2:
            if t.shape[1] != D or not t.is_contiguous():
                raise GppError(f"{name} must be a contiguous (M, {D}) matrix{'' if B is None else f' or ({B}, M, {D})'} "
                               f"(got {tuple(t.shape)})")
            M, s = t.shape[0], 0
        else:
            if B is None or t.dim() != 3 or t.shape[0] != B or t.shape[2] != D or t.stride(2) != 1 or t.stride(1) != D:
                raise GppError(f"{name} must be {'an (M' if B is None else f'({B}, M'}, {D}) matrix with contiguous rows "
                               f"(got {tuple(t.shape)}, strides {t.stride()})")
            M, s = t.shape[1], (t.stride(0) if B > 1 else t.shape[1] * D + (t.shape[1] * D & 1))
            if s & 1:
                raise GppError(f"{name}: the batch stride ({s}) is odd: every element must stay 16-byte aligned (pad the elements)")
            if s < M * D:
                raise GppError(f"{name}: the batch stride ({s}) is shorter than an element ({M * D})")
        if M < 1:
            raise GppError(f"{name} needs at least one row")
        return M, s

    def _dx_checks(self, what, Ua, Ub, w, sf2, d0, nd, kind, d_split, batched=False):
        """The operand checks of the derivative-block calls; returns (B, D, Ma, sUa, Mb, sUb), B None and the strides 0 for one
        problem.  One problem: w holds D weights and sf2 one value; batched: w is (B, D) and sf2 (B,)."""
        for t, n in ((w, "w"), (sf2, "sf2")):
            _need(t, torch.float64, n)
        if not w.is_contiguous() or (batched and w.dim() != 2):
            raise GppError(f"{what}: w must be a contiguous {'(B, D) matrix' if batched else 'vector of weights'} (got {tuple(w.shape)})")
        B, D = w.shape if batched else (None, w.numel())
        _check_features(D)
        if batched and (B < 1 or B > 65535):
            raise GppError(f"{what} takes 1..65535 elements (got {B})")
        if sf2.numel() < 1 or (batched and (sf2.dim() != 1 or sf2.numel() != B or not sf2.is_contiguous())):
            raise GppError(f"{what}: sf2 must {f'be a contiguous vector of {B} values' if batched else 'hold one value'} "
                           f"(got {tuple(sf2.shape)})")
        Ma, sa = self._dx_rows("Ua", Ua, B, D)
        Mb, sb = self._dx_rows("Ub", Ub, B, D)
        if not (0 <= int(d_split) <= D) or kind not in (KIND_RBF, KIND_MATERN32, KIND_MATERN52):
            raise GppError(f"bad kernel kind / d_split ({kind}, {d_split}) for {D} features")
        if nd < 1 or d0 < 0 or d0 + nd > D:
            raise GppError(f"the differentiated columns [{d0}, {d0 + nd}) must be a non-empty range of the {D} features")
        return B, D, Ma, sa, Mb, sb

    @staticmethod
    def _dx_window(name, out, rows, cols, B=None):
        """The checks of a window the same calls write or read: rows x cols, or (B, rows, cols) in a batched call (e.g. a block of
        ``batched_buffer``), with unit column stride, an even leading dimension and batch stride, 16-byte aligned; returns
        (leading dimension, batch stride), the stride 0 for one problem."""
        _need(out, torch.float64, name)
        shape = (rows, cols) if B is None else (B, rows, cols)
        if out.dim() != len(shape) or out.stride(-1) != 1 or tuple(out.shape) != shape:
            raise GppError(f"{name} must be {' x '.join(map(str, shape))} with unit column stride (got {tuple(out.shape)})")
        # (a single row has no stride to speak of: a batch takes the padded width, one problem the width itself)
        ld = out.stride(-2) if rows > 1 else max(cols + (0 if B is None else cols & 1), out.stride(-2))
        if ld & 1 or ld < cols:
            raise GppError(f"{name}: the leading dimension ({ld}) must be even and at least {cols}")
        s = 0
        if B is not None:
            s = out.stride(0) if B > 1 else rows * ld
            if s & 1:
                raise GppError(f"{name}: the batch stride ({s}) is odd: every element must stay 16-byte aligned")
            if B > 1 and s < (rows - 1) * ld + cols:
                raise GppError(f"{name}: the batch stride ({s}) is shorter than an element")
        if out.data_ptr() & 15:
            raise GppError(f"{name} must be 16-byte aligned")
        return ld, s

    @staticmethod
    def _sel_q(what, sel, M, nd, device):
        """The number of gradient entries of M points: all M nd, or those of the ``GradientSelection`` ``sel`` (checked)."""
        if sel is None:
            return M * nd
        sel._check(what, M, nd, device)
        return sel.q

    @staticmethod
    def _sel_args(sel, q):
        """A side's selection as the ``_sel`` and ``_batched`` entry points take it: first, dir (NULL for every entry) and q."""
        return (None, None, q) if sel is None else (sel.first.data_ptr(), sel.dir.data_ptr(), q)

    def _dx_entry(self, name, sides):
        """(entry point, its name, selection arguments) of a single-problem call: the plain one, which takes no selection
        arguments, unless a side of ``sides`` = ((sel, q), ...) has a selection."""
        if all(sel is None for sel, _ in sides):
            return getattr(self.lib, name), name, ()
        return getattr(self.lib, name + "_sel"), name + "_sel", tuple(a for side in sides for a in self._sel_args(*side))

    @_on_own_device
    def cross_kernel_dx(self, Ua, Ub, w, sf2, d0, nd, out, *, kind=KIND_RBF, d_split=0, sel=None):
        """out[n, a nd + j] = d/du_{d0+j} sf2 k(u, Ub_n; w) at u = Ua_a: the derivative cross block with the training points as rows,
        the operand ``predict_tn`` takes (gpp_cross_kernel_dx).  ``out``: an N x (M nd) window of a row-major buffer with an even
        leading dimension, 16-byte aligned; what lies beyond column M nd is not written.  Everything is checked before the launch.
        ``sel``: a ``GradientSelection`` of the points ``Ua``: ``out`` is then N x sel.q, column k the selected entry k
        (gpp_cross_kernel_dx_sel)."""
        d0, nd = int(d0), int(nd)
        _, D, M, _, N, _ = self._dx_checks("cross_kernel_dx", Ua, Ub, w, sf2, d0, nd, kind, d_split)
        q = self._sel_q("cross_kernel_dx", sel, M, nd, Ua.device)
        ld, _ = self._dx_window("Dk", out, N, q)
        fn, name, sel_args = self._dx_entry("gpp_cross_kernel_dx", ((sel, q),))
        self._stream()
        check(fn(self.h, Ua.data_ptr(), M, Ub.data_ptr(), N, D, w.data_ptr(), sf2.data_ptr(), int(kind), int(d_split), d0, nd,
                 *sel_args, out.data_ptr(), ld), name)
        return out

    @_on_own_device
    def point_gram(self, Q, nd, G=None, Gsum=None, *, omega=None):
        """G[a] = Q_a Q_a^T of the ``nd`` consecutive rows of each point in ``Q`` ((M nd) x N, a window of a row-major buffer with an
        even leading dimension, 16-byte aligned; nd <= 16) and / or Gsum = sum_a omega_a G[a] (gpp_point_gram).  ``G``: a contiguous
        M x nd x nd tensor or None; ``Gsum``: a contiguous nd x nd matrix or None; ``omega``: M weights or None for all ones.
        Everything is checked before any launch."""
        nd = int(nd)
        _need(Q, torch.float64, "Q")
        if Q.dim() != 2 or Q.stride(1) != 1:
            raise GppError("Q must be 2-D with unit column stride")
        if nd < 1 or nd > 16:
            raise GppError(f"point_gram takes 1..16 rows per point (got {nd})")
        rows, N = Q.shape
        if rows < nd or rows % nd or N < 1:
            raise GppError(f"Q is {tuple(Q.shape)}: its rows must be a positive multiple of nd = {nd} and it needs a column")
        M = rows // nd
        ld = _ld(Q)
        if ld & 1 or ld < N:
            raise GppError(f"Q: the leading dimension ({ld}) must be even and at least {N}")
        if Q.data_ptr() & 15:
            raise GppError("Q must be 16-byte aligned")
        if G is None and Gsum is None:
            raise GppError("point_gram needs G or Gsum")
        for t, n, shape in ((G, "G", (M, nd, nd)), (Gsum, "Gsum", (nd, nd))):
            if t is not None:
                _need(t, torch.float64, n)
                if tuple(t.shape) != shape or not t.is_contiguous():
                    raise GppError(f"{n} must be a contiguous {shape} tensor (got {tuple(t.shape)})")
        if omega is not None:
            _need(omega, torch.float64, "omega")
            if omega.dim() != 1 or omega.numel() != M or not omega.is_contiguous():
                raise GppError(f"omega must be a contiguous vector of {M} weights (got {tuple(omega.shape)})")
        if Gsum is not None:
            self.ensure_workspace(OP_POINT_GRAM, 0, M, nd, 0)
        self._stream()
        status = self.lib.gpp_point_gram(self.h, Q.data_ptr(), ld, M, nd, N, _ptr(omega), _ptr(G), _ptr(Gsum))
        check(status, "gpp_point_gram")
        return G, Gsum

    # -- conditioning on gradient observations -----------------------------------------------------------------------------------
    @_on_own_device
    def kernel_dxdx(self, Ua, Ub, w, sf2, d0, nd, out, *, kind=KIND_RBF, d_split=0, sel_a=None, sel_b=None):
        """out[a nd + j, b nd + l] = d^2/du_{d0+j} dv_{d0+l} sf2 k(u, v; w) at u = Ua_a, v = Ub_b: the covariance of two gradient
        observations (gpp_kernel_dxdx).  ``out``: an (Ma nd) x (Mb nd) window of a row-major buffer with an even leading dimension,
        16-byte aligned; what lies beyond column Mb nd is not written.  Everything is checked before the launch.
        ``sel_a`` / ``sel_b``: a ``GradientSelection`` of the points ``Ua`` / ``Ub``: the rows / columns of ``out`` are then its
        selected entries (gpp_kernel_dxdx_sel)."""
        d0, nd = int(d0), int(nd)
        _, D, Ma, _, Mb, _ = self._dx_checks("kernel_dxdx", Ua, Ub, w, sf2, d0, nd, kind, d_split)
        qa = self._sel_q("kernel_dxdx (rows)", sel_a, Ma, nd, Ua.device)
        qb = self._sel_q("kernel_dxdx (columns)", sel_b, Mb, nd, Ua.device)
        ld, _ = self._dx_window("H", out, qa, qb)
        fn, name, sel_args = self._dx_entry("gpp_kernel_dxdx", ((sel_a, qa), (sel_b, qb)))
        self._stream()
        check(fn(self.h, Ua.data_ptr(), Ma, Ub.data_ptr(), Mb, D, w.data_ptr(), sf2.data_ptr(), int(kind), int(d_split), d0, nd,
                 *sel_args, out.data_ptr(), ld), name)
        return out

    # -- training on gradient observations ---------------------------------------------------------------------------------------
    def _gek_grad_checks(self, what, U, Ug, w, sf2, d0, nd, alpha, Kinv, dU, g_w, g_sf2, g_U, g_Ug, kind, d_split, sel, batched):
        """The checks ``gek_grad_reduce`` and its batched form share: the operands, dU, alpha ((n,), or a (B, n) batched vector), the
        window Kinv and the four outputs.  Returns (B, D, Mg, sUg, N, sU, q, alpha's batch stride, Kinv's leading dimension and batch
        stride), B None and the strides 0 for one problem."""
        B, D, Mg, sug, N, su = self._dx_checks(what, Ug, U, w, sf2, d0, nd, kind, d_split, batched)
        q = self._sel_q(what, sel, Mg, nd, Ug.device)
        n, lead = N + q, ((B,) if batched else ())
        if dU < 0 or dU > d0 or (kind != KIND_RBF and dU > int(d_split)):
            raise GppError(f"{what}: the {dU} feature columns with a gradient must lie in front of the differentiated ones "
                           f"(d0 = {d0}) and, on a Matern kind, inside the RBF factor (d_split = {d_split})")
        _need(alpha, torch.float64, "alpha")
        if tuple(alpha.shape) != lead + (n,) or alpha.stride(-1) != 1:
            raise GppError(f"alpha must be a {'(%d, %d) batched vector' % (B, n) if batched else 'contiguous vector of %d doubles' % n} "
                           f"(got {tuple(alpha.shape)})")
        sv = 0
        if batched:
            sv = alpha.stride(0) if B > 1 else n + (n & 1)
            if sv & 1:
                raise GppError(f"alpha: the batch stride ({sv}) is odd: every element must stay 16-byte aligned (use batched_vector)")
            if sv < n:
                raise GppError(f"alpha: the batch stride ({sv}) is shorter than an element ({n})")
        ld, sk = self._dx_window("Kinv", Kinv, n, n, B)
        for t, name, shape in ((g_w, "g_w", (D,)), (g_sf2, "g_sf2", () if batched else (1,)), (g_U, "g_U", (N, dU)),
                               (g_Ug, "g_Ug", (Mg, dU))):
            if t is None:
                if dU > 0 or name in ("g_w", "g_sf2"):
                    raise GppError(f"{what}: {name} is missing")
                continue
            _need(t, torch.float64, name)
            if tuple(t.shape) != lead + shape or not t.is_contiguous():
                raise GppError(f"{name} must be a contiguous {lead + shape} tensor (got {tuple(t.shape)})")
        return B, D, Mg, sug, N, su, q, sv, ld, sk

    @_on_own_device
    def gek_grad_reduce(self, U, Ug, w, sf2, d0, nd, alpha, Kinv, dU, g_w, g_sf2, g_U=None, g_Ug=None, *, kind=KIND_RBF, d_split=0,
                        sel=None):
        """The gradient of the joint log-likelihood of [y; grad y] through the function / gradient and gradient / gradient blocks
        (gpp_gek_grad_reduce): ADDS to ``g_w`` (D), ``g_sf2`` (1) and ``g_U`` (N x dU), WRITES ``g_Ug`` (Mg x dU).  ``alpha``: the
        n = N + Mg nd solved residuals; ``Kinv``: n x n as the LAUUM leaves it (lower triangle), an even leading dimension, 16-byte
        aligned.  ``dU`` <= d0, and <= d_split on the Matern kinds.  Everything is checked before the launch.
        ``sel``: a ``GradientSelection`` of the points ``Ug``: n = N + sel.q, row N + k the selected entry k
        (gpp_gek_grad_reduce_sel)."""
        d0, nd, dU = int(d0), int(nd), int(dU)
        _, D, Mg, _, N, _, q, _, ld, _ = self._gek_grad_checks("gek_grad_reduce", U, Ug, w, sf2, d0, nd, alpha, Kinv, dU, g_w, g_sf2,
                                                               g_U, g_Ug, kind, d_split, sel, False)
        fn, name, sel_args = self._dx_entry("gpp_gek_grad_reduce", ((sel, q),))
        self.ensure_workspace(OP_GEK_GRAD, N, Mg, D, dU)
        self._stream()
        status = fn(self.h, U.data_ptr(), N, Ug.data_ptr(), Mg, D, w.data_ptr(), sf2.data_ptr(), int(kind), int(d_split), d0, nd,
                    *sel_args, alpha.data_ptr(), Kinv.data_ptr(), ld, dU, g_w.data_ptr(), g_sf2.data_ptr(),
                    _ptr(g_U) if dU else None, _ptr(g_Ug) if dU else None)
        check(status, name)

    # -- the three above for B problems in one launch each (batched.BatchedGEKFunction) -------------------------------------------
    @_on_own_device
    def cross_kernel_dx_batched(self, Ua, Ub, w, sf2, d0, nd, out, *, kind=KIND_RBF, d_split=0, sel=None):
        """``cross_kernel_dx`` for B problems in one launch (gpp_cross_kernel_dx_batched).  Ua: (M, D) shared or (B, M, D); Ub: (N, D)
        shared or (B, N, D); w: (B, D); sf2: (B,); out: a (B, N, q) window with unit column stride, an even leading dimension and an
        even batch stride, 16-byte aligned, q = M nd or ``sel.q`` (ONE selection serves every element).  Element b is bitwise
        ``cross_kernel_dx`` on element b's operands.  Everything is checked before the launch."""
        d0, nd = int(d0), int(nd)
        B, D, M, sa, N, sb = self._dx_checks("cross_kernel_dx_batched", Ua, Ub, w, sf2, d0, nd, kind, d_split, True)
        q = self._sel_q("cross_kernel_dx_batched", sel, M, nd, Ua.device)
        ld, so = self._dx_window("Dk", out, N, q, B)
        self._stream()
        check(self.lib.gpp_cross_kernel_dx_batched(self.h, Ua.data_ptr(), sa, M, Ub.data_ptr(), sb, N, D, w.data_ptr(), sf2.data_ptr(),
                                                   int(kind), int(d_split), d0, nd, *self._sel_args(sel, q), out.data_ptr(), ld, so, B),
              "gpp_cross_kernel_dx_batched")
        return out

    @_on_own_device
    def kernel_dxdx_batched(self, Ua, Ub, w, sf2, d0, nd, out, *, kind=KIND_RBF, d_split=0, sel_a=None, sel_b=None):
        """``kernel_dxdx`` for B problems in one launch (gpp_kernel_dxdx_batched): the operands of ``cross_kernel_dx_batched``, out a
        (B, qa, qb) window.  Element b is bitwise ``kernel_dxdx`` on element b's operands.  Everything is checked before the launch."""
        d0, nd = int(d0), int(nd)
        B, D, Ma, sa, Mb, sb = self._dx_checks("kernel_dxdx_batched", Ua, Ub, w, sf2, d0, nd, kind, d_split, True)
        qa = self._sel_q("kernel_dxdx_batched (rows)", sel_a, Ma, nd, Ua.device)
        qb = self._sel_q("kernel_dxdx_batched (columns)", sel_b, Mb, nd, Ua.device)
        ld, so = self._dx_window("H", out, qa, qb, B)
        self._stream()
        check(self.lib.gpp_kernel_dxdx_batched(self.h, Ua.data_ptr(), sa, Ma, Ub.data_ptr(), sb, Mb, D, w.data_ptr(), sf2.data_ptr(),
                                               int(kind), int(d_split), d0, nd, *self._sel_args(sel_a, qa), *self._sel_args(sel_b, qb),
                                               out.data_ptr(), ld, so, B), "gpp_kernel_dxdx_batched")
        return out

    @_on_own_device
    def gek_grad_reduce_batched(self, U, Ug, w, sf2, d0, nd, alpha, Kinv, dU, g_w, g_sf2, g_U=None, g_Ug=None, *, kind=KIND_RBF,
                                d_split=0, sel=None):
        """``gek_grad_reduce`` for B problems in one launch (gpp_gek_grad_reduce_batched): ADDS to ``g_w`` (B, D), ``g_sf2`` (B) and
        ``g_U`` (B, N, dU), WRITES ``g_Ug`` (B, Mg, dU), all contiguous.  U: (N, D) shared or (B, N, D); Ug: (Mg, D) shared or
        (B, Mg, D); w: (B, D); sf2: (B,); alpha: a (B, n) batched vector (even row stride); Kinv: a (B, n, n) window as
        ``lauum_batched`` leaves it.  Element b is bitwise ``gek_grad_reduce`` on element b's operands.  Everything is checked before
        the launch."""
        d0, nd, dU = int(d0), int(nd), int(dU)
        B, D, Mg, sug, N, su, q, sv, ld, sk = self._gek_grad_checks("gek_grad_reduce_batched", U, Ug, w, sf2, d0, nd, alpha, Kinv, dU,
                                                                    g_w, g_sf2, g_U, g_Ug, kind, d_split, sel, True)
        need = B * int(self.lib.gpp_workspace_bytes(self.h, OP_GEK_GRAD, N, Mg, D, dU))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            check(self.lib.gpp_set_workspace(self.h, self._ws.data_ptr(), self._ws.numel()), "gpp_set_workspace")
        self._stream()
        status = self.lib.gpp_gek_grad_reduce_batched(self.h, U.data_ptr(), su, N, Ug.data_ptr(), sug, Mg, D, w.data_ptr(),
                                                      sf2.data_ptr(), int(kind), int(d_split), d0, nd, *self._sel_args(sel, q),
                                                      alpha.data_ptr(), sv, Kinv.data_ptr(), ld, sk, dU, g_w.data_ptr(),
                                                      g_sf2.data_ptr(), _ptr(g_U) if dU else None, _ptr(g_Ug) if dU else None, B)
        check(status, "gpp_gek_grad_reduce_batched")


def post_cross_min_workspace_bytes(Mc: int, Mr: int, Q: int) -> int:
    """Scratch bytes of one ``post_cross_min`` launch (a host-side query: no handle, no device)."""
    from ._lib import load

    return int(load().gpp_workspace_bytes(None, OP_POST_CROSS_MIN, int(Mr), int(Mc), 0, int(Q)))


def get_context(device) -> GppContext:
    device = torch.device(device)
    if device.type != "cuda":
        raise GppError(
            f"the exact-GP hot path runs only on an MI355X through libgpp_hip (device={device}); no CPU fallback exists")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, threading.get_ident())
    ctx = _contexts.get(key)
    if ctx is None:
        with _contexts_lock:
            ctx = GppContext(torch.device("cuda", idx))
            _contexts[key] = ctx
    return ctx


@atexit.register
def _destroy_contexts() -> None:
    """Release the library handles (and their internal CU-masked streams / events) while the HIP runtime is still
    alive; leaving them to process teardown crashes under rocprofv3."""
    if not _contexts:
        return
    try:
        torch.cuda.synchronize()
    except Exception:
        pass
    for key, ctx in list(_contexts.items()):
        try:
            ctx.lib.gpp_destroy(ctx.h)
        except Exception:
            pass
        _contexts.pop(key, None)

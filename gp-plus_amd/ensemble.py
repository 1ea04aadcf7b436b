"""Hyperparameter ensembles: predictions from K parameter sets of one model — the restarts a fit would discard, or any other sample of
hyperparameters — mixed by their moments.  The reference does this with multi-pass ensembles that are moment-matched across passes
(models/gp_plus.py:387-396, 474-482; ``num_pass_pred = 30``); here the K members are factored in one batched pass
(``gpp_*_batched``) and predicted in ONE launch, ``gpp_predict_gen_batched``, which generates each member's cross block in registers
and never writes it or V = K_*N L^-T to memory.
"""
from __future__ import annotations

from collections import OrderedDict
from copy import deepcopy
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from . import settings

__all__ = ["HyperparameterEnsemble", "mixture_weights", "mixture_moments", "ENSEMBLE_CHUNK_BYTES", "ENSEMBLE_FUSED_MAX_N"]

#: the records of one fused launch (K x ceil(N / 64) x rows x 2 doubles), and the cross block and V of one composed step, stay
#: within this: the test points go in chunks (the size of ``linalg.GRAD_CHUNK_BYTES``)
ENSEMBLE_CHUNK_BYTES = 256 << 20

#: ``predict(route=None)`` takes the fused launch up to this N and the composed route (gpp_cross_kernel + gpp_predict_tn per member)
#: above it: the largest measured N at which the fused launch was not slower for any K measured there.  MEASURED
#: (tools/bench_ensemble.py, profiles/r21_ensemble_bench.txt; p = 8, RBF, M = 4096, device events, medians of 5, the two routes
#: alternating), fused / composed in ms at (N, K): (100, 65) 0.315 / 2.459, (500, 8) 0.451 / 0.727, (500, 65) 2.755 / 5.550,
#: (2000, 16) 9.265 / 9.864, (6144, 8) 39.99 / 32.86 — 7.8x, 1.6x, 2.0x and 1.06x for the fused launch, then 0.82x: between 2000 and
#: 6144 the GEMM-backed route overtakes it (31 against 38 TFLOP/s on K M N^2 at 6144); nothing in between was timed.
ENSEMBLE_FUSED_MAX_N = 2000


def _host_f64(values) -> torch.Tensor:
    """A flat fp64 host tensor of ``values`` (a tensor, or numbers that are read as doubles, not rounded through fp32)."""
    t = values.detach() if torch.is_tensor(values) else torch.as_tensor(np.asarray(values, dtype=np.float64))
    return t.to(device="cpu", dtype=torch.float64).reshape(-1)


def mixture_weights(weights, losses, num_data: Optional[int], K: int) -> torch.Tensor:
    """The K mixture weights (fp64, on the host, summing to 1).  ``"posterior"``: pi_b proportional to exp(-n (loss_b - min loss))
    with n = ``num_data``, since a loss is -(log density + log priors) / n; ``"uniform"``: 1 / K; a length-K tensor: non-negative
    with a positive sum, normalised here."""
    if isinstance(weights, str):
        if weights == "uniform":
            return torch.full((K,), 1.0 / K, dtype=torch.float64)
        if weights != "posterior":
            raise ValueError(f'weights must be "posterior", "uniform" or a tensor of {K} weights (got {weights!r})')
        if losses is None:
            raise ValueError('weights="posterior" needs the losses of the members')
        if num_data is None or int(num_data) < 1:
            raise ValueError(f'weights="posterior" needs num_data >= 1, the observations the losses are normalised by (got {num_data})')
        e = torch.exp(-float(int(num_data)) * (losses - losses.min()))
        return e / e.sum()
    w = _host_f64(weights)
    if w.numel() != K:
        raise ValueError(f"{w.numel()} weights for {K} members")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not float(w.sum()) > 0.0:
        raise ValueError("the weights must be finite and non-negative with a positive sum")
    return w / w.sum()


def mixture_moments(pi: torch.Tensor, mu: torch.Tensor, var: torch.Tensor):
    """Mean and variance (M,) of the mixture sum_b pi_b N(mu_b, var_b) from the (K, M) member moments, by the law of total variance:
    mu = sum_b pi_b mu_b, var = sum_b pi_b var_b + sum_b pi_b (mu_b - mu)^2 (the reference's moment matching across passes)."""
    p = pi.to(mu).reshape(-1, 1)
    mean = (p * mu).sum(0)
    return mean, (p * var).sum(0) + (p * (mu - mean) ** 2).sum(0)


class HyperparameterEnsemble:
    """K hyperparameter sets of ``model`` and the mixture of their posteriors.

    ``states``: a dict mapping each trainable parameter name of the model to a stacked ``(K, *shape)`` tensor (the layout of
    ``optim.BatchedObjective.theta``), or a list of K dicts name -> tensor.  ``losses``: the K objective values the members ended
    with (``-(log density + log priors) / n``).  ``weights``: ``"posterior"`` — pi_b proportional to exp(-n (loss_b - min loss)),
    n = ``num_data`` (default: the number of training targets; N + q after an ``objective="gek"`` fit) — ``"uniform"``, or K
    non-negative weights.  ``"posterior"`` weighs the modes BY THEIR HEIGHT ONLY: there is no curvature (Laplace) term, so a narrow
    mode counts as much as a wide one of the same height; and restarts that converged to the same optimum are counted as often as
    they occur — nothing de-duplicates them.

    The ensemble keeps a detached copy of the model (parameters, data, no N x N factors): refitting or conditioning the model
    afterwards does not change it.  On first use all members are factored in one batched pass (gpp_kernel_build_batched,
    gpp_potrf_batched under ``psd_safe.psd_safe_batched``'s per-member jitter schedule, gpp_trtri_batched, gpp_mll_reduce_batched) and
    Linv (K x N x stride) and z are copied into tensors the ensemble owns, so the shared ``BatchedWorkspace`` stays free for anyone;
    ``jitter`` then holds what each member needed.  A member that stays indefinite raises ``errors.NotPSDError`` naming it.  Each
    member's features, weights, outputscale, noise, noise groups and prior mean come from the model's own forward under
    ``functional_call`` + ``vmap`` (``optim.mll_batched.member_operands``).

    Everything is validated on the host before a device is touched.  ``NotImplementedError`` for a model with calibration parameters
    and for N above ``optim.BATCHED_MAX_N``; at ``predict``: under ``settings.sharded_evaluation`` and inside a graph capture;
    ``RuntimeError`` for a model that is not on a GPU; ``MemoryError`` when the owned cache and the batched workspace together
    exceed a third of the device's free memory (the rule of ``GP_Plus._restarts_fit_one_batch``).

    Out of scope: gradients through the predictions, sampling, scores, conditioning and LOO / CV from an ensemble."""

    def __init__(self, model, states: Union[Dict[str, torch.Tensor], List[Dict[str, torch.Tensor]]], losses=None,
                 weights="posterior", num_data: Optional[int] = None):
        from .optim.mll_batched import BATCHED_MAX_N

        expect = OrderedDict((n, tuple(p.shape)) for n, p in model.named_parameters() if p.requires_grad)
        if isinstance(states, (list, tuple)):
            if len(states) < 1:
                raise ValueError("an ensemble needs at least one member (K >= 1)")
            for b, st in enumerate(states):
                if not isinstance(st, dict) or set(st) != set(expect):
                    raise ValueError(f"member {b}: the names must be the model's trainable parameters {sorted(expect)}")
                for n in expect:
                    if tuple(torch.as_tensor(st[n]).shape) != expect[n]:
                        raise ValueError(f"member {b}: {n} must have shape {expect[n]} (got {tuple(torch.as_tensor(st[n]).shape)})")
            states = {n: torch.stack([torch.as_tensor(st[n]).detach() for st in states]) for n in expect}
        if not isinstance(states, dict) or set(states) != set(expect):
            got = sorted(states) if isinstance(states, dict) else type(states).__name__
            raise ValueError(f"states must map the model's trainable parameters {sorted(expect)} to stacked tensors (got {got})")
        K = None
        for n, shape in expect.items():
            t = states[n]
            if not torch.is_tensor(t) or t.dim() != len(shape) + 1 or tuple(t.shape[1:]) != shape:
                raise ValueError(f"{n} must be stacked as (K, {', '.join(map(str, shape))}) "
                                 f"(got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__})")
            K = t.shape[0] if K is None else K
            if t.shape[0] != K:
                raise ValueError(f"{n} holds {t.shape[0]} members where the others hold {K}")
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"{n} holds a NaN or an inf")
        if K is None or K < 1:
            raise ValueError("an ensemble needs at least one member (K >= 1)")
        if losses is not None:
            losses = _host_f64(losses)
            if losses.numel() != K:
                raise ValueError(f"{losses.numel()} losses for {K} members")
            if not bool(torch.isfinite(losses).all()):
                raise ValueError("the losses must be finite")
        N = int(model.train_targets.shape[0])
        if num_data is None:
            num_data = N
        self._weights = mixture_weights(weights, losses, num_data, K)
        if len(getattr(model, "calibration_id", None) or []) > 0:
            raise NotImplementedError("HyperparameterEnsemble is not available for a model with calibration parameters: the batched "
                                      "evaluation has no calibrated form")
        if N > BATCHED_MAX_N:
            raise NotImplementedError(f"HyperparameterEnsemble: {N} training rows are beyond the batched kernels' range "
                                      f"({BATCHED_MAX_N})")
        self._losses, self.num_data = losses, int(num_data)
        held = model.__dict__.pop("restart_ensemble", None)  # (the receiver's own ensemble is not part of the copy)
        try:
            with torch.no_grad():
                child = model._copy_without_factors()
        finally:
            if held is not None:
                model.restart_ensemble = held
        child.eval()
        self._model = child
        params = dict(child.named_parameters())
        self._states = OrderedDict((n, states[n].detach().to(params[n]).clone()) for n in expect)
        self._fixed = {n: p.detach() for n, p in child.named_parameters() if not p.requires_grad}
        self._buffers = dict(child.named_buffers())
        self._K, self._N = int(K), N
        self._cache = None
        #: the jitter each member's factorisation needed (K,), on the host; None until the members are factored
        self.jitter = None

    # -- the members ------------------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return self._K

    def __repr__(self):
        return f"HyperparameterEnsemble(members={self._K}, training rows={self._N})"

    @property
    def states(self) -> "OrderedDict[str, torch.Tensor]":
        """name -> (K, *shape) stacked parameters (copies)."""
        return OrderedDict((n, t.clone()) for n, t in self._states.items())

    @property
    def losses(self) -> Optional[torch.Tensor]:
        return None if self._losses is None else self._losses.clone()

    @property
    def weights(self) -> torch.Tensor:
        return self._weights.clone()

    def state(self, b: int) -> Dict[str, torch.Tensor]:
        """Member ``b`` as a complete state dict of the model (for ``load_state_dict``)."""
        b = int(b)
        if not 0 <= b < self._K:
            raise IndexError(f"member {b} of {self._K}")
        sd = deepcopy(self._model.state_dict())
        sd.update({n: t[b].clone() for n, t in self._states.items()})
        return sd

    # -- operands through the model's own forward ---------------------------------------------------------------------------------
    def _operands(self, rows):
        """(U, w, sf2, tau, prior mean) of every member at the input rows ``rows`` with a leading K, and (grp, kind, d_split)."""
        from .optim.mll_batched import member_operands

        static = []

        def one(params):
            full = dict(self._fixed)
            full.update(params)
            full.update(self._buffers)
            return member_operands(self._model, full, rows, static.append, priors=False)

        with torch.no_grad():
            U, w, sf2, tau, mean, _ = torch.vmap(one, in_dims=(0,), randomness="error")(dict(self._states))
        return (U, w, sf2, tau, mean), static[-1]

    def _shared_features(self) -> bool:
        """True when the model has no learned latent map: every member then sees the same features."""
        m = self._model
        return not (hasattr(m, "_features") and int(m._features(m.train_inputs[0])[1]) > 0)

    def _refusals(self, what: str, dev) -> None:
        if settings.sharded_evaluation.value() is not None:
            raise NotImplementedError(f"{what} is not available under settings.sharded_evaluation")
        if dev.type != "cuda":
            raise RuntimeError("this build evaluates a Gaussian process only on an MI355X (device='cuda'); there is no CPU path")
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError(f"{what} is not available inside a graph capture")

    def cache_bytes(self) -> int:
        """Bytes of the owned factor cache: Linv (K x N x stride) and z."""
        from .backend import row_stride

        return 8 * self._K * (self._N * row_stride(self._N) + self._N + (self._N & 1))

    def _ensure_cache(self, gctx):
        """Factor all members in one batched pass and keep Linv, z and the operands of the training rows."""
        if self._cache is not None:
            return self._cache
        from types import SimpleNamespace

        from .backend import UPLO_UPPER, row_stride
        from .batched import _batched_operands, _even_elements, get_batched_workspace
        from .errors import NotPSDError
        from .linalg import _as_f64
        from .psd_safe import psd_safe_batched

        K, N, dev = self._K, self._N, gctx.device
        own, work = self.cache_bytes(), 3 * 8 * K * N * row_stride(N)
        free, _ = torch.cuda.mem_get_info(dev)
        if own + work > free // 3:
            raise MemoryError(f"HyperparameterEnsemble: the owned cache ({own} bytes) and the batched workspace ({work} bytes) of "
                              f"{K} members with {N} rows exceed a third of the device's free memory ({free} bytes free)")
        m = self._model
        (U, w, sf2, tau, mean), (grp, kind, d_split) = self._operands(m.train_inputs[0])
        Ud = _as_f64(U[0], dev) if self._shared_features() else _even_elements(_as_f64(U, dev))
        wd, sd, td, grp, S = _batched_operands(w, sf2, tau, grp)
        ws = get_batched_workspace(gctx, K, N)
        ws.epoch += 1
        torch.sub(_as_f64(m.train_targets.detach(), dev).expand(K, N), _as_f64(mean, dev).expand(K, N), out=ws.r)
        used = []

        def attempt(extra):
            used.append(extra)
            gctx.kernel_build_batched(Ud, wd, sd, td + extra, grp, ws.A, kind=kind, d_split=d_split, uplo=UPLO_UPPER)
            gctx.potrf_batched(ws.A, ws.Li, ws.info)
            ok = ws.info == 0
            ws.info_host.copy_(ws.info, non_blocking=True)
            ws.info_event.record()
            gctx.trtri_batched(ws.A, ws.Li, ws.Ki)
            gctx.mll_reduce_batched(ws.A, ws.Li, ws.r, ws.z, ws.out3)
            ws.info_event.synchronize()
            return ok, ws.info_host

        ok, _ = psd_safe_batched(K, dev, attempt)
        bad = [int(b) for b in (~ok).nonzero().reshape(-1).tolist()]
        if bad:
            raise NotPSDError(f"HyperparameterEnsemble: member{'s' if len(bad) > 1 else ''} {', '.join(map(str, bad))} "
                              f"not positive definite after the jitter schedule")
        Li, z = gctx.batched_buffer(K, N), gctx.batched_vector(K, N)
        Li.copy_(ws.Li)
        z.copy_(ws.z)
        self.jitter = used[-1].reshape(-1).cpu()
        self._cache = SimpleNamespace(U=Ud, w=wd, sf2=sd, tau=td, Li=Li, z=z, kind=int(kind), d_split=int(d_split))
        return self._cache

    # -- prediction -------------------------------------------------------------------------------------------------------------
    def predict(self, Xtest, return_std: bool = True, include_noise: bool = True, return_members: bool = False, route=None):
        """Mean (and std) of the mixture at the rows of ``Xtest``, in the units of the training targets with the conventions of
        ``GP_Plus.predict``.  Per member mu_b = y_min + y_std (m_b(x) + mean_b) and sigma_b^2 = y_std^2 clamp(var_b [+ the noise of
        the row's own source under member b], ``settings.min_variance``); the mixture is mu = sum_b pi_b mu_b and
        sigma^2 = sum_b pi_b sigma_b^2 + sum_b pi_b (mu_b - mu)^2.  ``return_members=True`` appends the (K, M) member means and stds.
        ``route``: "fused" (one gpp_predict_gen_batched launch per chunk of test rows), "composed" (per member gpp_cross_kernel and
        gpp_predict_tn on its slices of the owned cache) or None: fused up to N = ``ENSEMBLE_FUSED_MAX_N``.  The test rows go in
        chunks that keep the records within ``ENSEMBLE_CHUNK_BYTES``; on the fused route the chunking does not change a bit of the
        result (a row's result does not depend on the other rows of a launch)."""
        from .backend import get_context
        from .batched import _even_elements
        from .linalg import _as_f64

        what = "HyperparameterEnsemble.predict"
        if route not in (None, "fused", "composed"):
            raise ValueError(f'route must be None, "fused" or "composed" (got {route!r})')
        m = self._model
        X = m._alc_rows(Xtest, "Xtest", what)
        dev = m.train_inputs[0].device
        self._refusals(what, dev)
        gctx = get_context(dev)
        fused = route == "fused" or (route is None and self._N <= ENSEMBLE_FUSED_MAX_N)
        with torch.cuda.device(dev), torch.no_grad():
            c = self._ensure_cache(gctx)
            X = X.to(m.train_inputs[0])
            (Us, _, _, tau, prior), (grp_t, _, _) = self._operands(X)
            K, N, M = self._K, self._N, X.shape[0]
            shared = c.U.dim() == 2
            Us = _as_f64(Us[0] if shared else Us, dev)
            mean = torch.empty(K, M, dtype=torch.float64, device=dev)
            var = torch.empty(K, M, dtype=torch.float64, device=dev)
            step = self._chunk_rows(fused)
            for a0 in range(0, M, step):
                mc = min(step, M - a0)
                (self._fused_chunk if fused else self._composed_chunk)(gctx, c, Us[..., a0:a0 + mc, :], mean[:, a0:a0 + mc],
                                                                       var[:, a0:a0 + mc], _even_elements)
            y_min, y_std = m.y_min.detach().to(torch.float64), m.y_std.detach().to(torch.float64)
            mu = y_min + y_std * (_as_f64(prior, dev).expand(K, M) + mean)
            if not return_std:
                mix_mu = (self._weights.to(dev).reshape(-1, 1) * mu).sum(0)
                return (mix_mu, mu) if return_members else mix_mu
            if include_noise:
                td = _as_f64(tau.reshape(K, -1), dev)
                var = var + (td[:, grp_t.long()] if grp_t is not None else td[:, :1])
            s2 = y_std * y_std * var.clamp_min(settings.min_variance.value())
            mix_mu, mix_var = mixture_moments(self._weights.to(dev), mu, s2)
            out = (mix_mu, mix_var.sqrt())
            return out + (mu, s2.sqrt()) if return_members else out

    def _chunk_rows(self, fused: bool) -> int:
        """Test rows per chunk: the fused launch's records, or one member's cross block and V on the composed route, within
        ``ENSEMBLE_CHUNK_BYTES`` (whole 64-row tiles where more than one fits)."""
        from .backend import row_stride

        per_row = 16 * self._K * ((self._N + 63) // 64) if fused else 16 * row_stride(self._N)
        rows = max(1, ENSEMBLE_CHUNK_BYTES // per_row)
        return rows if rows < 64 else rows // 64 * 64

    def _fused_chunk(self, gctx, c, Us, mean, var, even):
        K, mc = self._K, Us.shape[-2]
        Ua = Us.contiguous() if Us.dim() == 2 else even(Us.contiguous())
        mo, vo = gctx.batched_vector(K, mc), gctx.batched_vector(K, mc)
        gctx.predict_gen_batched(Ua, c.U, c.w, c.sf2, c.Li, c.z, mo, vo, kind=c.kind, d_split=c.d_split)
        mean.copy_(mo)
        var.copy_(vo)

    def _composed_chunk(self, gctx, c, Us, mean, var, even):
        from .backend import rows_buffer

        N, mc, dev = self._N, Us.shape[-2], mean.device
        Kns, V = rows_buffer(N, mc, dev), rows_buffer(mc, N, dev)
        mo, vo = (torch.empty(mc, dtype=torch.float64, device=dev) for _ in range(2))
        for b in range(self._K):
            Ub = c.U if c.U.dim() == 2 else c.U[b]
            Ua = (Us if Us.dim() == 2 else Us[b]).contiguous()
            gctx.cross_kernel(Ub, Ua, c.w[b], c.sf2[b:b + 1], Kns, kind=c.kind, d_split=c.d_split)
            gctx.predict_tn(c.Li[b], c.z[b], Kns, c.sf2[b:b + 1].expand(mc).contiguous(), V, mo, vo)
            mean[b].copy_(mo)
            var[b].copy_(vo)

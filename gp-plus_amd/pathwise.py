"""Pathwise posterior draws (Matheron's rule; Wilson et al. 2020, "Efficiently sampling functions from Gaussian process
posteriors"): a draw of the posterior FUNCTION, built once from the cached factor in O(N^2 S) and evaluated afterwards at any
number of points in O(N + F) per point and path, without ever forming an M x N matrix.

No reference counterpart: the reference draws vectors only (models/gp_plus.py:985-998, ``likelihood(self(X)).sample``), as
``GP_Plus.sample_y`` does here through the dense M x M predictive covariance.

In the scaled target space, with u(x) the model's features, m its mean, k the product kernel of ``KernelSpec``,
T = diag(tau[grp] + jitter) and Ky = K + T:

    prior draw     g_s(x) = phi(x)^T theta_s,   phi_f(x) = sqrt(2 sf2 / F) cos(omega_f . u(x) + b_f),   theta_s ~ N(0, I_F)
    path           f_s(x) = m(x) + g_s(x) + k(x, X) c_s,      c_s = Ky^-1 (y - m(X) - g_s(X) - eps_s),   eps_s ~ N(0, T)

E_s[f_s(x)] is the exact posterior mean whatever F is; the covariance of the paths is the posterior covariance with the prior
kernel replaced by its F-feature estimate in the terms that do not pass through Ky^-1.  The two sums over F and N are the HIP
kernels gpp_rff_apply and gpp_kernel_apply (csrc/gpp_apply.hip); their gradients with respect to u(x), gpp_rff_apply_grad and
gpp_kernel_apply_grad, make a path differentiable in x (``paths_with_grad``), which is what lets ``minimize`` search every draw for
its minimiser (Thompson sampling, ``bayesian_optimizations.thompson_sample``).

Every random number (omega, b, theta, eps) is drawn in float64 on the CPU from one ``torch.Generator`` and then moved to the
device: a seed gives the same paths on every machine.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

__all__ = ["draw_spectral", "PosteriorPaths", "PathMinimum"]

#: scratch the chunked evaluation lets gpp_kernel_apply ask for (partial products of a contraction cut in pieces)
WORKSPACE_BYTES = 256 << 20
#: rows per chunk when the contraction needs no scratch
MAX_CHUNK = 1 << 18


def _cpu_generator(generator: Optional[torch.Generator]) -> Optional[torch.Generator]:
    if generator is not None:
        if not isinstance(generator, torch.Generator):
            raise TypeError(f"generator must be a torch.Generator (got {type(generator).__name__})")
        if generator.device.type != "cpu":
            raise ValueError("the random numbers of a path are drawn on the CPU: pass a CPU torch.Generator")
    return generator


def draw_spectral(spec, D: int, F: int, generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(omega, phase)``: F frequencies (F x D) from the spectral measure of the kernel ``spec`` describes and F phases from
    U[0, 2 pi), float64 on the CPU.

    RBF dims (d < d_split, or all of them for the RBF kind): exp(-w_d delta^2) has the measure N(0, 2 w_d), so
    omega_fd = sqrt(2 w_d) z_fd.  Matern dims: the multivariate Student-t measure with 2 nu degrees of freedom,
    omega_fd = sqrt(2 w_d) z_fd sqrt(2 nu / g_f) with ONE g_f ~ chi^2_{2 nu} per feature shared by all Matern dims (the sum of
    2 nu squared normals).  The product of kernels on disjoint dims has the product measure; a dim with w_d = 0 gets omega = 0.
    Draw order: z (F x D), g's normals (F x 2 nu, Matern kinds only), phases (F)."""
    D, F = int(D), int(F)
    if D < 1 or F < 1:
        raise ValueError(f"draw_spectral needs D >= 1 and F >= 1 (got D = {D}, F = {F})")
    generator = _cpu_generator(generator)
    w = spec.w.detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    if w.numel() != D:
        raise ValueError(f"the kernel has {w.numel()} feature weights, D = {D}")
    if bool((w < 0).any()):
        raise ValueError("feature weights must be non-negative")
    kind, d_split = int(spec.kind), int(spec.d_split)
    if kind not in (0, 1, 2):
        raise ValueError(f"unknown kernel kind {kind}")
    omega = torch.randn(F, D, dtype=torch.float64, generator=generator) * (2.0 * w).sqrt()
    if kind != 0:
        two_nu = 3 if kind == 1 else 5
        g = torch.randn(F, two_nu, dtype=torch.float64, generator=generator).pow(2).sum(dim=1)
        omega[:, d_split:] *= (two_nu / g).sqrt().unsqueeze(1)
    phase = torch.rand(F, dtype=torch.float64, generator=generator) * (2.0 * math.pi)
    return omega, phase


class _PathChunk(torch.autograd.Function):
    """g_s(x) + k(x, X) c_s at one chunk of feature rows (M_c x S): the two applies of ``paths`` forward, their fused gradients
    backward.  Everything but the features is a constant of the drawn paths."""

    @staticmethod
    def forward(ctx, Us, paths):
        buf = torch.empty(Us.shape[0], paths.size, dtype=torch.float64, device=Us.device)
        paths.gctx.rff_apply(Us, paths.omega, paths.phase, paths._sf2, paths.theta, buf)
        paths.gctx.kernel_apply(Us, paths.U, paths.spec.w, paths._sf2, paths.coef, buf, beta=1.0, kind=paths.spec.kind,
                                d_split=paths.spec.d_split)
        ctx.paths = paths
        ctx.save_for_backward(Us)
        return buf

    @staticmethod
    @once_differentiable
    def backward(ctx, gbar):
        (Us,), paths = ctx.saved_tensors, ctx.paths
        gbar = gbar.to(torch.float64).contiguous()
        g = torch.empty_like(Us)
        with torch.cuda.device(Us.device):
            paths.gctx.rff_apply_grad(Us, paths.omega, paths.phase, paths._sf2, paths.theta, gbar, g)
            paths.gctx.kernel_apply_grad(Us, paths.U, paths.spec.w, paths._sf2, paths.coef, gbar, g, beta=1.0, kind=paths.spec.kind,
                                         d_split=paths.spec.d_split)
        return g, None


@dataclass
class PathMinimum:
    """What :meth:`PosteriorPaths.minimize` returns: ``x`` (S x p) the best point found for every draw and ``f`` (S) its value
    f_s(x_s); ``f_candidates`` (S) the best value among the random candidates; ``x_starts`` (S x num_starts x p) the candidates the
    descent started from."""
    x: torch.Tensor
    f: torch.Tensor
    f_candidates: torch.Tensor
    x_starts: torch.Tensor


class PosteriorPaths:
    """``size`` posterior function draws of a fitted model, fixed at construction.

    Holds ``omega`` (F x D), ``phase`` (F), ``theta`` (F x S), ``eps`` (N x S), ``coef`` (N x S; the c_s above), its own reference to
    the cache's training features and ``KernelSpec``, and the model (for features and prior mean).  After construction it does
    not depend on the shared prediction workspace: another model may factor into it.

    The object is valid only while the model's parameters stay what they were at construction: ``coef`` is frozen, while features
    and prior mean come from the model's forward at every :meth:`paths` call.  After a refit, an optimiser step or a
    ``load_state_dict`` :meth:`paths` raises ``RuntimeError`` (the parameters' version counters are compared): draw new paths.

    :meth:`paths` evaluates all draws at any inputs.  The draws are of the LATENT function f (no observation noise is added) in
    the scaled target space ``sample_y`` uses, and carry no autograd graph."""

    def __init__(self, model, cache, size: int = 1, num_features: int = 2048, generator: Optional[torch.Generator] = None):
        from .backend import rows_buffer

        S, F = int(size), int(num_features)
        if S < 1:
            raise ValueError(f"size must be at least 1 (got {size})")
        if F < 1:
            raise ValueError(f"num_features must be at least 1 (got {num_features})")
        generator = _cpu_generator(generator)
        cache.refresh()  # another model of the same size may have factored into the shared workspace since
        if cache._refactor is None:
            raise RuntimeError("this factor cache does not know its noise levels: paths need one made by linalg.factorize")
        self.model, self.gctx = model, cache.gctx
        self._versions = self._parameter_versions()
        self.U, self.spec = cache.U, cache.spec
        dev = self.U.device
        N, D = self.U.shape
        tau, grp, r = cache._refactor
        t = tau.reshape(-1)
        noise = (t[0].expand(N) if grp is None else t[grp.long()]) + float(cache.jitter)
        self.noise = noise.contiguous()  # diag(T), the factor's own jitter included

        omega, phase = draw_spectral(self.spec, D, F, generator)
        theta = torch.randn(F, S, dtype=torch.float64, generator=generator)
        eps = torch.randn(N, S, dtype=torch.float64, generator=generator) * noise.detach().cpu().sqrt().unsqueeze(1)
        self.omega, self.phase, self.theta, self.eps = (x.to(dev).contiguous() for x in (omega, phase, theta, eps))
        self._sf2 = self.spec.sf2.reshape(1).contiguous()

        with torch.no_grad(), torch.cuda.device(dev):
            gctx = self.gctx
            R = rows_buffer(N, S, dev)
            gctx.rff_apply(self.U, self.omega, self.phase, self._sf2, self.theta, R)  # g_s(X)
            torch.sub(r.unsqueeze(1) - self.eps, R, out=R)                           # y - m(X) - eps_s - g_s(X)
            # c = L^-T (L^-1 R): both as row-contiguous TN products against the Linv buffer (L^-1 in its lower triangle, the mirror
            # L^-T in its strict upper one) — A[k][m] with k <= m reads the mirror, i.e. L^-1[m][k]; with k >= m it reads L^-1[k][m]
            Z, Cb = rows_buffer(N, S, dev), rows_buffer(N, S, dev)
            gctx.gemm(1, 0, N, S, N, 1.0, cache.Linv, R, 0.0, Z, a_mask=1, khi_mode=1)
            gctx.gemm(1, 0, N, S, N, 1.0, cache.Linv, Z, 0.0, Cb, a_mask=2, klo_mode=1)
            self.coef = Cb.contiguous()

    def _parameter_versions(self):
        return tuple((id(p), p._version) for p in self.model.parameters())

    @property
    def size(self) -> int:
        return self.theta.shape[1]

    @property
    def num_features(self) -> int:
        return self.theta.shape[0]

    def _chunk_rows(self) -> int:
        from .backend import APPLY_SPLIT

        N, S = self.coef.shape
        pieces = max(-(-N // APPLY_SPLIT), -(-self.num_features // APPLY_SPLIT))
        if pieces <= 1:
            return MAX_CHUNK
        return max(64, min(MAX_CHUNK, WORKSPACE_BYTES // (pieces * S * 8) // 64 * 64))

    @torch.no_grad()
    def paths(self, X, chunk: Optional[int] = None) -> torch.Tensor:
        """The draws at the rows of ``X``: ``(size, len(X))``, float64, in the scaled target space of ``sample_y``, latent f without
        observation noise, no autograd graph.  ``X`` has the columns of the training inputs (categorical and source columns
        included): features and prior mean come from the model's own eval-mode forward.  Rows are processed in chunks (``chunk``
        rows, by default as many as the scratch workspace allows); a row's values do not depend on the chunking, bit for bit.
        Puts the model into eval mode (as ``predict`` and ``sample_y`` do) and raises ``RuntimeError`` when the model's parameters
        were modified since the paths were drawn."""
        from .gpcore.kernels import LazyKernelMatrix
        from .gpcore.module import Module

        model = self.model
        if self._parameter_versions() != self._versions:
            raise RuntimeError("the model's parameters changed since these paths were drawn (their coefficients belong to the old "
                               "parameters): call sample_paths again")
        ref = model.train_inputs[0]
        X = torch.as_tensor(X)
        if X.dim() == 1:
            X = X.unsqueeze(0) if ref.shape[1] > 1 else X.unsqueeze(1)
        if X.dim() != 2 or X.shape[1] != ref.shape[1]:
            raise ValueError(f"X must have the {ref.shape[1]} columns of the training inputs (got shape {tuple(X.shape)})")
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"chunk must be at least 1 (got {chunk})")
        X = X.to(device=ref.device, dtype=ref.dtype)
        M, S = X.shape[0], self.size
        dev = self.U.device
        out = torch.empty(S, M, dtype=torch.float64, device=dev)
        rows = self._chunk_rows() if chunk is None else int(chunk)
        model.eval()
        with torch.cuda.device(dev):
            for i0 in range(0, M, rows):
                prior = Module.__call__(model, X[i0:i0 + rows])
                cov = prior.lazy_covariance_matrix
                if not isinstance(cov, LazyKernelMatrix):
                    raise RuntimeError("pathwise draws need the model's forward to return a lazy kernel covariance")
                Us = cov.U1.to(torch.float64).contiguous()
                buf = torch.empty(Us.shape[0], S, dtype=torch.float64, device=dev)
                self.gctx.rff_apply(Us, self.omega, self.phase, self._sf2, self.theta, buf)
                self.gctx.kernel_apply(Us, self.U, self.spec.w, self._sf2, self.coef, buf, beta=1.0, kind=self.spec.kind,
                                       d_split=self.spec.d_split)
                out[:, i0:i0 + rows] = (buf + prior.mean.to(torch.float64).unsqueeze(1)).T
        return out

    __call__ = paths

    def paths_with_grad(self, X, chunk: Optional[int] = None) -> torch.Tensor:
        """:meth:`paths` with an autograd graph: the same values, bit for bit (the same launches under the same chunking rule),
        connected to ``X``'s quantitative columns through the model's own forward for features and prior mean; categorical and
        source columns get zero gradient, as in ``predict_with_grad``.  The frequencies, phases, weights, coefficients, kernel
        parameters and training features are constants of the drawn paths.  One autograd node per row chunk; its backward is
        gpp_rff_apply_grad followed by gpp_kernel_apply_grad into one buffer, O(N + F) per point and path like the forward, and
        cannot itself be differentiated again."""
        from .gpcore.kernels import LazyKernelMatrix
        from .gpcore.module import Module

        model = self.model
        if self._parameter_versions() != self._versions:
            raise RuntimeError("the model's parameters changed since these paths were drawn (their coefficients belong to the old "
                               "parameters): call sample_paths again")
        ref = model.train_inputs[0]
        X = torch.as_tensor(X)
        if X.dim() == 1:
            X = X.unsqueeze(0) if ref.shape[1] > 1 else X.unsqueeze(1)
        if X.dim() != 2 or X.shape[1] != ref.shape[1]:
            raise ValueError(f"X must have the {ref.shape[1]} columns of the training inputs (got shape {tuple(X.shape)})")
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"chunk must be at least 1 (got {chunk})")
        X = X.to(device=ref.device, dtype=ref.dtype)
        dev = self.U.device
        rows = self._chunk_rows() if chunk is None else int(chunk)
        model.eval()
        out = []
        with torch.cuda.device(dev):
            for i0 in range(0, X.shape[0], rows):
                prior = Module.__call__(model, X[i0:i0 + rows])
                cov = prior.lazy_covariance_matrix
                if not isinstance(cov, LazyKernelMatrix):
                    raise RuntimeError("pathwise draws need the model's forward to return a lazy kernel covariance")
                buf = _PathChunk.apply(cov.U1.to(torch.float64).contiguous(), self)
                out.append((buf + prior.mean.to(torch.float64).unsqueeze(1)).T)
        if not out:
            return torch.empty(self.size, 0, dtype=torch.float64, device=dev)
        return out[0] if len(out) == 1 else torch.cat(out, dim=1)

    def minimize(self, lower, upper, fixed: Optional[Dict[int, float]] = None, num_candidates: int = 1024, num_starts: int = 4,
                 steps: int = 50, maximize: bool = False, generator: Optional[torch.Generator] = None, lr: float = 0.05) -> PathMinimum:
        """arg min_x f_s(x) over the box [lower, upper] for every draw s (arg max with ``maximize``): a Thompson-sampling step.

        ``lower`` / ``upper`` have one entry per input column; ``fixed`` maps a column to the value it keeps (every categorical and
        source column must be fixed; a quantitative one may be).  ``num_candidates`` points are drawn uniformly in the box from the
        CPU ``generator`` and all draws are scored on them with :meth:`paths`; each draw's best ``num_starts`` candidates are then
        advanced together, S * num_starts points per :meth:`paths_with_grad` call, by ``steps`` steps of Adam on the free
        quantitative columns in box units (step ``lr`` of the box width), projected back into the box after every step.  The loss
        is the sum of each point's own draw, so a point only ever sees its own gradient.  The best value seen along each
        trajectory is kept — the start included, so ``f <= f_candidates`` (``>=`` with ``maximize``).  Nothing inside the loop
        waits for the GPU.  Evaluating every draw at every point costs a factor S more than needed in the contraction, which is
        immaterial at these sizes."""
        model = self.model
        ref = model.train_inputs[0]
        p, S = ref.shape[1], self.size
        num_candidates, num_starts, steps = int(num_candidates), int(num_starts), int(steps)
        if num_starts < 1 or num_candidates < num_starts or steps < 0:
            raise ValueError(f"minimize needs num_candidates >= num_starts >= 1 and steps >= 0 (got {num_candidates}, {num_starts}, {steps})")
        generator = _cpu_generator(generator)
        lo = torch.as_tensor(lower, dtype=torch.float64).reshape(-1).clone()
        hi = torch.as_tensor(upper, dtype=torch.float64).reshape(-1).clone()
        if lo.numel() != p or hi.numel() != p:
            raise ValueError(f"lower and upper need one entry for each of the {p} input columns")
        fixed = {int(c): float(v) for c, v in (fixed or {}).items()}
        if any(c < 0 or c >= p for c in fixed):
            raise ValueError(f"fixed names a column outside 0..{p - 1}")
        for c, v in fixed.items():
            lo[c] = hi[c] = v
        if bool((lo > hi).any()):
            raise ValueError("lower must not exceed upper")
        quant = set(int(c) for c in model.quant_index.tolist())
        loose = [c for c in range(p) if c not in quant and c not in fixed]
        if loose:
            raise ValueError(f"columns {loose} are categorical or source columns: give their values in fixed")
        free = torch.zeros(p, dtype=torch.float64)
        free[[c for c in sorted(quant) if c not in fixed]] = 1.0

        dev = self.U.device
        cand = lo + torch.rand(num_candidates, p, dtype=torch.float64, generator=generator) * (hi - lo)
        cand = torch.minimum(torch.maximum(cand, lo), hi).to(dev)
        lo, hi, free = lo.to(dev), hi.to(dev), free.to(dev)
        sign = -1.0 if maximize else 1.0
        scores = sign * self.paths(cand)                                   # S x candidates
        start_f, start_i = torch.topk(scores, num_starts, dim=1, largest=False)
        x_starts = cand[start_i]                                           # S x starts x p
        x = x_starts.reshape(S * num_starts, p).to(ref.dtype)
        own = torch.arange(S, device=dev).repeat_interleave(num_starts).unsqueeze(0)
        width = (hi - lo) * free                                           # 0 on the columns that stay
        best_f = torch.full((S * num_starts,), float("inf"), dtype=torch.float64, device=dev)
        best_x = x.clone()
        m1, m2 = torch.zeros_like(x, dtype=torch.float64), torch.zeros_like(x, dtype=torch.float64)
        b1, b2, eps = 0.9, 0.999, 1e-8
        for t in range(1, steps + 1):
            xg = x.detach().requires_grad_(True)
            f = sign * self.paths_with_grad(xg).gather(0, own).squeeze(0)  # each point's own draw
            (g,) = torch.autograd.grad(f.sum(), xg)
            better = f.detach() < best_f
            best_f = torch.where(better, f.detach(), best_f)
            best_x = torch.where(better.unsqueeze(1), x, best_x)
            gz = g.to(torch.float64) * width                               # the gradient in box units
            m1.mul_(b1).add_(gz, alpha=1.0 - b1)
            m2.mul_(b2).addcmul_(gz, gz, value=1.0 - b2)
            step = (lr / (1.0 - b1 ** t)) * m1 / ((m2 / (1.0 - b2 ** t)).sqrt() + eps)
            x = torch.minimum(torch.maximum(x.to(torch.float64) - step * width, lo), hi).to(ref.dtype)
        f = sign * self.paths(x).gather(0, own).squeeze(0)
        better = f < best_f
        best_f = torch.where(better, f, best_f)
        best_x = torch.where(better.unsqueeze(1), x, best_x)
        win = best_f.reshape(S, num_starts).argmin(dim=1)
        rows = torch.arange(S, device=dev)
        return PathMinimum(x=best_x.reshape(S, num_starts, p)[rows, win], f=sign * best_f.reshape(S, num_starts)[rows, win],
                           f_candidates=sign * start_f[:, 0], x_starts=x_starts)

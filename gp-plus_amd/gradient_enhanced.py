"""Gradient-enhanced Kriging on a fitted model: ``GP_Plus.condition_on_gradients`` borders the cached factorisation with observed
gradients (``linalg.append_gradients_to_cache``: gpp_cross_kernel_dx for the function / gradient block, gpp_kernel_dxdx for the
gradient / gradient block, gpp_chol_append for the border) and returns a ``GradientEnhancedPosterior``.  No reference counterpart."""
from __future__ import annotations

import numpy as np
import torch

from .gpcore.distributions import DenseCovariance, MultivariateNormal
from .gpcore.module import Module
from .utils import data_type_check

__all__ = ["GRADIENT_NUGGET_REL", "GradientEnhancedPosterior", "condition_on_gradients", "check_gradient_observations",
           "check_gradient_run", "variance_reduction_of_runs"]

#: ``noise=None``: the variance given to a gradient observation, as a fraction of the prior curvature of its direction (the prior
#: variance of that component of the gradient, ``linalg.gradient_prior_curvature``).
GRADIENT_NUGGET_REL = 1e-6


class GradientEnhancedPosterior:
    """The posterior of a fitted model conditioned on its own training data AND on gradient observations, as returned by
    ``GP_Plus.condition_on_gradients``.  It offers ``predict`` and ``predict_gradient`` with the conventions of the model's own, and
    ``variance_reduction`` (where to run next, with or without gradients), the attributes ``num_function_rows`` (N),
    ``num_gradient_points`` (Mg), ``num_gradient_observations`` (q: Mg p, or the number of observed components when an ``observed=``
    mask was given) and ``observed`` (the (Mg, p) bool mask).  Nothing else: no further conditioning, no sampling, no leave-one-out or
    cross-validation, no knowledge gradient, no joint covariance, no hyperparameter training on the gradient data.  It holds a detached copy of the model (parameters, training inputs, no N x N factors) for the features, prior means and
    noise of test rows: refitting or modifying the model it came from does not change it."""

    def __init__(self, model, gcache):
        self._model, self._cache = model, gcache

    @property
    def num_function_rows(self) -> int:
        return int(self._cache.U.shape[0])

    @property
    def num_gradient_points(self) -> int:
        return int(self._cache.Ug.shape[0])

    @property
    def num_gradient_observations(self) -> int:
        return int(self._cache.q)

    @property
    def observed(self) -> torch.Tensor:
        """A copy of the (Mg, p) bool mask of the observed gradient components (all True without ``observed=``)."""
        sel = self._cache.sel
        if sel is None:
            return torch.ones(self.num_gradient_points, self._cache.nd, dtype=torch.bool, device=self._cache.Ug.device)
        return sel.mask.clone()

    def __repr__(self):
        return (f"GradientEnhancedPosterior(function rows={self.num_function_rows}, gradient points={self.num_gradient_points}, "
                f"directions={self._cache.nd}, gradient observations={self.num_gradient_observations})")

    def _prior(self, Xtest, what: str):
        m = self._model
        X = m._alc_rows(Xtest, "Xtest", what).to(m.train_inputs[0])
        out = Module.__call__(m, X)
        return X, out, out.lazy_covariance_matrix.U1

    def predict(self, Xtest, return_std=True, include_noise=True):
        """Mean (and std) at the rows of ``Xtest`` in the units of the training targets, with the return convention of
        ``GP_Plus.predict``: the std includes the noise of each test row's own source unless ``include_noise=False``."""
        from .linalg import predict_from_gradient_cache

        m = self._model
        with torch.no_grad():
            X, out, Us = self._prior(Xtest, "GradientEnhancedPosterior.predict")
            mean_c, var = predict_from_gradient_cache(self._cache, Us, "function")
            post = MultivariateNormal(out.mean.to(torch.float64) + mean_c, DenseCovariance(var, n=var.shape[0]))
            if return_std and include_noise:
                m.likelihood.fidel_indices = X[:, -1]  # noise of the test points' own sources
                post = m.likelihood(post)
            mean = m.y_min + m.y_std * post.mean
            if return_std:
                return mean, post.variance.sqrt() * m.y_std
            return mean

    def predict_gradient(self, Xtest, return_std=True):
        """Posterior mean (M, p) — and with ``return_std`` the std (M, p) — of the gradient of the latent f with respect to the
        quantitative input columns, in y per input unit, ``quant_index`` order, as ``GP_Plus.predict_gradient`` returns them."""
        from .linalg import predict_from_gradient_cache

        m = self._model
        with torch.no_grad():
            _, _, Us = self._prior(Xtest, "GradientEnhancedPosterior.predict_gradient")
            mean, var = predict_from_gradient_cache(self._cache, Us, "gradient")
            scale = m.y_std.detach().to(torch.float64)
            if return_std:
                return mean * scale, var.clamp_min(0.0).sqrt() * scale.abs()
            return mean * scale


    def variance_reduction(self, Xcand, Xref, weights=None, gradient=None, gradient_noise=None):
        """``GP_Plus.variance_reduction`` from this posterior, with the same arguments, units and refusals.  ``gradient=None``: the
        expected reduction of the weighted posterior variance over ``Xref`` from ONE noisy function value at each row of ``Xcand``
        (M_c scores; gpp_post_cross_sq on operands of N + q coordinates).  ``gradient=True`` or a length-p bool mask: the pair
        (scores of a run that returns y and those gradient components, scores of the value alone), by
        ``linalg.variance_reduction_block``.  Nothing is conditioned: the posterior stays as it is."""
        return variance_reduction_of_runs(self._model, self._cache, Xcand, Xref, weights, gradient, gradient_noise)


def _check_observed_mask(observed, Mg: int, p: int, what: str):
    """``observed`` as a host bool (Mg, p) tensor: a bool (or 0 / 1 valued) mask that broadcasts to (Mg, p), every row with at
    least one True.  ``ValueError`` otherwise."""
    m = observed.detach().cpu() if torch.is_tensor(observed) else torch.as_tensor(np.asarray(observed))
    if m.dtype != torch.bool:
        if m.is_complex() or not bool(((m == 0) | (m == 1)).all()):
            raise ValueError(f"{what}: observed must be a bool mask (or hold only 0 and 1)")
        m = m != 0
    if m.dim() > 2:
        raise ValueError(f"{what}: observed must broadcast to ({Mg}, {p}) (got {tuple(m.shape)})")
    try:
        m = torch.broadcast_to(m, (Mg, p)).contiguous()
    except RuntimeError:
        raise ValueError(f"{what}: observed must broadcast to ({Mg}, {p}) (got {tuple(m.shape)})") from None
    empty = ~m.any(1)
    if bool(empty.any()):
        raise ValueError(f"{what}: gradient point {int(empty.to(torch.int32).argmax())} has no observed component under the "
                         "observed= mask: drop the row")
    return m


def check_gradient_observations(model, X, dY, noise, what: str, observed=None):
    """The host-side validation ``condition_on_gradients`` and the ``"gek"`` training objective share: returns (X, dY, noise,
    observed) with dY as (Mg, p), ``noise`` as an fp64 (Mg, p) tensor or None and ``observed`` as a host bool (Mg, p) tensor or None.
    ``ValueError`` for wrong shapes, NaN / inf, Mg = 0, rows the model cannot take, negative noise, a model without a quantitative
    column, or a mask that is not one (``_check_observed_mask``).  With a mask the entries of ``dY`` and ``noise`` under its False
    entries are not read: they may be NaN or inf, and come back as zeros.  Without one NaN is refused: it never means "missing"."""
    X, dY = data_type_check(X), data_type_check(dY)
    train_x = model.train_inputs[0]
    p = int(model.quant_index.numel())
    if X.dim() != 2 or X.shape[1] != train_x.shape[1]:
        raise ValueError(f"{what}: X must be (q, {train_x.shape[1]}) like the training inputs (got {tuple(X.shape)})")
    if p == 0:
        raise ValueError(f"{what}: the model has no quantitative input column to differentiate")
    if dY.dim() == 1 and p == 1:
        dY = dY.reshape(-1, 1)
    if dY.dim() != 2 or dY.shape[1] != p:
        raise ValueError(f"{what}: dY must be (q, {p}): one column per quantitative input column (got {tuple(dY.shape)})")
    if dY.shape[0] != X.shape[0]:
        raise ValueError(f"{what}: {X.shape[0]} rows of X for {dY.shape[0]} gradients")
    if X.shape[0] == 0:
        raise ValueError(f"{what}: no observation given (q = 0)")
    Mg = X.shape[0]
    if observed is not None:
        observed = _check_observed_mask(observed, Mg, p, what)
        dY = torch.where(observed.to(dY.device), dY, torch.zeros((), dtype=dY.dtype, device=dY.device))
    if not (bool(torch.isfinite(X).all()) and bool(torch.isfinite(dY).all())):
        raise ValueError(f"{what}: X and dY must be finite (NaN or inf found)")
    model._check_new_rows(X)
    if noise is not None:
        # (a Python or numpy number straight to fp64: ``data_type_check`` would round a float to the default dtype first)
        noise = noise.detach().to(torch.float64) if torch.is_tensor(noise) else torch.as_tensor(np.asarray(noise, dtype=np.float64))
        try:
            noise = torch.broadcast_to(noise, (Mg, p))
        except RuntimeError:
            raise ValueError(f"{what}: noise must be a scalar or broadcast to ({Mg}, {p}) (got {tuple(noise.shape)})") from None
        if observed is not None:
            noise = torch.where(observed.to(noise.device), noise, torch.zeros((), dtype=noise.dtype, device=noise.device))
        if not bool(torch.isfinite(noise).all()) or bool((noise < 0).any()):
            raise ValueError(f"{what}: the noise variances must be finite and not negative")
    return X, dY, noise, observed


def condition_on_gradients(model, X, dY, noise=None, observed=None) -> GradientEnhancedPosterior:
    """The work behind ``GP_Plus.condition_on_gradients`` (documented there)."""
    from . import settings as gpp_settings
    from .backend import GradientSelection, get_context
    from .linalg import APPEND_MAX_Q, append_gradients_to_cache, gradient_prior_curvature

    what = "condition_on_gradients"
    X, dY, noise, observed = check_gradient_observations(model, X, dY, noise, what, observed)
    train_x = model.train_inputs[0]
    p = int(model.quant_index.numel())
    Mg = X.shape[0]
    N = int(train_x.shape[0])
    if observed is None:
        if Mg * p > min(N, APPEND_MAX_Q):
            raise ValueError(f"{what}: {Mg} points x {p} directions = {Mg * p} gradient observations exceed "
                             f"min(N = {N}, {APPEND_MAX_Q})")
    else:
        q = int(observed.sum())
        if q > min(N, APPEND_MAX_Q):
            raise ValueError(f"{what}: {q} gradient observations (the True entries of observed, at {Mg} points x {p} directions) "
                             f"exceed min(N = {N}, {APPEND_MAX_Q})")
    if gpp_settings.sharded_evaluation.value() is not None:
        raise NotImplementedError(f"{what} is not available under settings.sharded_evaluation")
    get_context(train_x.device)  # (raises for anything but a GPU: there is no CPU path)

    model.eval()
    with torch.no_grad():
        cache = model._ensure_prediction_cache()
        Ug = Module.__call__(model, X.to(train_x)).lazy_covariance_matrix.U1
        d0 = Ug.shape[1] - p
        y_std = model.y_std.detach().to(torch.float64)
        r_g = dY.to(device=Ug.device, dtype=torch.float64) / y_std
        if noise is None:
            noise_diag = (GRADIENT_NUGGET_REL * gradient_prior_curvature(cache.spec, d0, p)).expand(Mg, p)
        else:
            noise_diag = noise.to(Ug.device) / y_std ** 2
        if observed is None:
            gcache = append_gradients_to_cache(cache, Ug, d0, p, r_g, noise_diag.contiguous())
        else:
            sel = GradientSelection(observed, Ug.device)
            gcache = append_gradients_to_cache(cache, Ug, d0, p, r_g.reshape(-1)[sel.flat], noise_diag.reshape(-1)[sel.flat], sel)
        child = model._copy_without_factors()
        child.eval()
    return GradientEnhancedPosterior(child, gcache)


def check_gradient_run(model, gradient, gradient_noise, Mc: int, what: str):
    """The host-side validation of ``variance_reduction(..., gradient=, gradient_noise=)``: returns (mask, noise) with ``mask`` a host
    bool (p) tensor of the gradient components a run returns (``gradient=True``: all p quantitative columns) and ``noise`` an fp64
    (Mc, p) tensor in (y per input unit)^2, or None for ``GRADIENT_NUGGET_REL`` times the prior curvature.  ``ValueError`` for a model
    without a quantitative column, ``gradient=False``, a mask that is not one, of another length or without a True, and noise that
    does not broadcast to (Mc, p), is not finite or is negative under the mask (what lies under a False is not read)."""
    p = int(model.quant_index.numel())
    if p == 0:
        raise ValueError(f"{what}: the model has no quantitative input column to differentiate")
    if gradient is True:
        mask = torch.ones(p, dtype=torch.bool)
    elif gradient is False:
        raise ValueError(f"{what}: gradient must be None (a run returns y alone), True or a bool mask of the {p} quantitative columns")
    else:
        g = gradient.detach().cpu() if torch.is_tensor(gradient) else torch.as_tensor(np.asarray(gradient))
        if g.dim() != 1 or g.shape[0] != p:
            raise ValueError(f"{what}: gradient must be True or a bool mask of length {p}, one entry per quantitative column: the same "
                             f"directions at every candidate (got shape {tuple(g.shape)})")
        mask = _check_observed_mask(g.reshape(1, p), 1, p, what)[0]
    noise = gradient_noise
    if noise is not None:
        noise = noise.detach().cpu().to(torch.float64) if torch.is_tensor(noise) else torch.as_tensor(np.asarray(noise, dtype=np.float64))
        try:
            noise = torch.broadcast_to(noise, (Mc, p))
        except RuntimeError:
            raise ValueError(f"{what}: gradient_noise must be a scalar, a row of {p} or ({Mc}, {p}) (got {tuple(noise.shape)})") from None
        noise = torch.where(mask, noise, torch.zeros((), dtype=noise.dtype))
        if not bool(torch.isfinite(noise).all()) or bool((noise < 0).any()):
            raise ValueError(f"{what}: the gradient noise variances must be finite and not negative")
    return mask, noise


def variance_reduction_of_runs(model, cache, Xcand, Xref, weights=None, gradient=None, gradient_noise=None):
    """The work behind ``GP_Plus.variance_reduction(..., gradient=)`` (``cache`` None: the model's own prediction cache) and
    ``GradientEnhancedPosterior.variance_reduction`` (``cache``: its ``GradientFactorCache``; ``model``: its copy of the model).
    Everything is validated on the host before any device work; results in y^2 units."""
    from .linalg import gradient_prior_curvature, variance_reduction_block, variance_reduction_from_gradient_cache
    from .models.gpregression import _check_weights

    what = "variance_reduction"
    Xc, Xr = model._alc_rows(Xcand, "Xcand"), model._alc_rows(Xref, "Xref")
    Mc = Xc.shape[0]
    weights = _check_weights(what, weights, Xr.shape[0], "reference rows")
    if gradient is None:
        if gradient_noise is not None:
            raise ValueError(f"{what}: gradient_noise without gradient= (a run that returns y alone has no gradient noise)")
        mask = noise = None
    else:
        mask, noise = check_gradient_run(model, gradient, gradient_noise, Mc, what)
    cache, (Xc, Xr), (out_c, out_r) = model._score_preamble(what, (Xc, Xr), cache)
    with torch.no_grad():
        Uc, Ur = out_c.lazy_covariance_matrix.U1, out_r.lazy_covariance_matrix.U1
        tau_c = model._noise_of_rows(out_c, Xc)
        dev = Xc.device
        omega = None if weights is None else weights.to(dev)
        scale = model.y_std.detach().to(torch.float64) ** 2
        if mask is None:
            return variance_reduction_from_gradient_cache(cache, Uc, tau_c, Ur, omega=omega) * scale
        p = int(mask.numel())
        d0 = Uc.shape[1] - p
        dirs = [d0 + int(j) for j in mask.nonzero().reshape(-1)]
        if noise is None:
            gnoise = (GRADIENT_NUGGET_REL * gradient_prior_curvature(cache.spec, d0, p))[mask.to(dev)].expand(Mc, len(dirs))
        else:
            gnoise = noise[:, mask].to(dev) / scale
        with_g, value = variance_reduction_block(cache, Uc, tau_c, gnoise.contiguous(), dirs, Ur, omega=omega)
        return with_g * scale, value * scale

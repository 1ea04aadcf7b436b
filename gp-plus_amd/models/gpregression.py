"""``GPR``: standard GP regression model of GP+ (reference: models/gpregression.py:38-221), on the own gpcore protocol
and the HIP back end.  Same constructor, attributes, buffers and state_dict keys; ``posterior``/``fantasize`` (botorch
glue for Bayesian optimisation) are outside the exact-GP hot path and raise.
"""
import math
from typing import List, Tuple, Union

import torch

from .. import kernels
from ..gpcore import (ExactGP, GaussianLikelihood, GreaterThan, Kernel, LogNormalPrior, MultivariateNormal, Positive,
                      settings as gptsettings)
from ..likelihoods_noise.multifidelity import Multifidelity_likelihood
from ..priors import LogHalfHorseshoePrior, MollifiedUniformPrior
from ..utils.transforms import inv_softplus, softplus


def _require(cond: bool, message: str) -> None:
    if not cond:
        raise RuntimeError(message)


def _named_correlation(name: str, n_features: int) -> Kernel:
    """A kernel of ``kernels`` chosen by name: ARD over every input column, ``l = exp(raw)``, mollified-uniform prior on
    ``raw`` over [log 0.1, log 10] (models/gpregression.py:89-102; any failure is reported as the reference reports it)."""
    try:
        k = getattr(kernels, name)(ard_num_dims=n_features,
                                   lengthscale_constraint=Positive(transform=torch.exp, inv_transform=torch.log))
        k.register_prior('lengthscale_prior', MollifiedUniformPrior(math.log(0.1), math.log(10)), 'raw_lengthscale')
    except Exception:
        raise RuntimeError("%s not an allowed kernel" % name)
    return k


def _check_weights(what: str, weights, n: int, noun: str):
    """``weights`` (None stays None) as fp64, one for each of the ``n`` ``noun``: finite, non-negative, not all zero."""
    from ..utils import data_type_check

    if weights is None:
        return None
    weights = data_type_check(weights).reshape(-1).to(torch.float64)
    if weights.shape[0] != n:
        raise ValueError(f"{what}: {weights.shape[0]} weights for {n} {noun}")
    if not bool(torch.isfinite(weights).all()) or bool((weights < 0).any()):
        raise ValueError(f"{what}: the weights must be finite and non-negative")
    if not bool((weights > 0).any()):
        raise ValueError(f"{what}: the weights are all zero")
    return weights


def _check_cost(what: str, cost, Mc: int):
    """``cost`` (None stays None) as fp64, one for each of the ``Mc`` candidates: finite and positive."""
    from ..utils import data_type_check

    if cost is None:
        return None
    cost = data_type_check(cost).reshape(-1).to(torch.float64)
    if cost.shape[0] != Mc:
        raise ValueError(f"{what}: {cost.shape[0]} costs for {Mc} candidates")
    if not bool(torch.isfinite(cost).all()) or bool((cost <= 0).any()):
        raise ValueError(f"{what}: the costs must be finite and positive")
    return cost


def _check_q(what: str, q, Mc: int) -> int:
    q = int(q)
    if q < 1 or q > Mc:
        raise ValueError(f"{what}: q must be between 1 and the number of candidates ({Mc}); got {q}")
    return q


class GPR(ExactGP):
    #: registered on the model in this order (state_dict keys of the reference, models/gpregression.py:73-76)
    _TARGET_BUFFERS = ('y_min', 'y_std', 'y_scaled')

    def __init__(self, train_x: torch.Tensor, train_y: torch.Tensor, correlation_kernel, noise_indices: List[int],
                 fix_noise: bool = False, fix_noise_val: float = 1e-5, lb_noise: float = 1e-12) -> None:
        # models/gpregression.py:50-56
        _require(torch.is_tensor(train_x), "'train_x' must be a tensor")
        _require(torch.is_tensor(train_y), "'train_y' must be a tensor")
        _require(train_x.shape[0] == train_y.shape[0], "Inputs and output have different number of observations")

        # tau = exp(raw) + lb_noise; one level, or one per data source named in the last input column (:59-66)
        noise_args = dict(noise_constraint=GreaterThan(lb_noise, transform=torch.exp, inv_transform=torch.log))
        if noise_indices:
            likelihood = Multifidelity_likelihood(noise_indices=noise_indices, fidel_indices=train_x[:, -1], **noise_args)
        else:
            likelihood = GaussianLikelihood(**noise_args)

        # targets scaled to [0, 1] by their range (:67-69); the three quantities travel with the state_dict
        lo = train_y.min()
        span = train_y.max() - lo
        scaled = (train_y - lo) / span
        ExactGP.__init__(self, train_x, scaled, likelihood)
        for key, value in zip(self._TARGET_BUFFERS, (lo, span, scaled)):
            self.register_buffer(key, value)
        self._num_outputs = 1

        # priors in the reference's registration order: noise, lengthscale (named kernels only), outputscale — this is the
        # order reset_parameters() consumes random numbers in (:84, :97-99, :113-115)
        self.likelihood.register_prior('noise_prior', LogHalfHorseshoePrior(0.01, lb_noise), 'raw_noise')
        if fix_noise:
            self.likelihood.raw_noise.requires_grad_(False)
            self.likelihood.noise_covar.noise = torch.tensor(fix_noise_val)

        if isinstance(correlation_kernel, str):
            correlation_kernel = _named_correlation(correlation_kernel, self.train_inputs[0].size(1))
        _require(isinstance(correlation_kernel, Kernel),
                 "specified correlation kernel is not a `gpytorch.kernels.Kernel` instance")
        self.covar_module = kernels.ScaleKernel(
            base_kernel=correlation_kernel, outputscale_constraint=Positive(transform=softplus, inv_transform=inv_softplus))
        self.covar_module.register_prior('outputscale_prior', LogNormalPrior(1e-6, 1.), 'outputscale')

    # a plain GPR has no mean module in the reference either (forward uses self.mean_module set by subclasses)
    def forward(self, x: torch.Tensor) -> MultivariateNormal:
        mean_x = self.mean_module(x)
        covar_x = self.covar_module(x)
        return MultivariateNormal(mean_x, covar_x)

    def predict(self, x: torch.Tensor, return_std: bool = False, include_noise: bool = False
                ) -> Union[torch.Tensor, Tuple[torch.Tensor]]:
        """models/gpregression.py:122-149."""
        self.eval()
        with gptsettings.fast_computations(log_prob=False):
            if self.train_targets.ndim != 1:
                raise NotImplementedError("batched GPs are outside the exact-GP hot path")
            output = self(x)
            self.fidel_indices = x[:, -1]
            if return_std and include_noise:
                self.likelihood.fidel_indices = x[:, -1]  # noise of the test points' own sources
                output = self.likelihood(output)
            out_mean = self.y_min + self.y_std * output.mean
            if return_std:
                out_std = output.variance.sqrt() * self.y_std
                return out_mean, out_std
            return out_mean

    def posterior(self, X, output_indices=None, observation_noise=True, posterior_transform=None, **kwargs):
        raise NotImplementedError("botorch posterior glue (models/gpregression.py:151-166) is out of scope of this build")

    def fantasize(self, X, sampler, observation_noise=True, **kwargs):
        raise NotImplementedError("botorch fantasize glue (models/gpregression.py:177-221) is out of scope of this build")

    def _check_new_rows(self, X: torch.Tensor) -> None:
        """Hook of ``condition_on``: raise ``ValueError`` for rows the model cannot take (GP_Plus: unseen levels or sources)."""

    def _after_copy(self, child) -> None:
        """Hook of ``condition_on``: mend whatever a deep copy of the model leaves pointing at the original."""

    def _copy_without_factors(self):
        """A deep copy of this model without its prediction cache (the N x N factors are not part of the copy): the copy route of
        ``condition_on`` and ``condition_on_gradients``."""
        import copy

        held, self.prediction_strategy = self.prediction_strategy, None
        # (predict_with_grad leaves ``fidel_indices`` — a slice of its differentiable input — on the model and the likelihood:
        #  such non-leaf attributes are copied detached)
        memo = {id(v): v.detach().clone() for mod in self.modules() for v in vars(mod).values()
                if torch.is_tensor(v) and not v.is_leaf}
        try:
            child = copy.deepcopy(self, memo)
        finally:
            self.prediction_strategy = held
        self._after_copy(child)
        return child

    def condition_on(self, X, y, reserve: int = 256):
        """A NEW model, in eval mode, that has the q observations (X, y) beside this model's training data, made by bordering
        the cached factorisation in O(N^2 q) (``linalg.append_to_cache``, gpp_chol_append) instead of factorising N + q rows in
        O((N + q)^3).  No reference counterpart: the reference's BO loop builds and refits a new model at every iteration
        (bayesian_optimizations/BO_GP_plus.py); its ``fantasize`` is botorch glue and stays out of scope.

        The receiver's data, parameters and cache are not modified (it is put in eval mode, as by ``predict``; without a cache it
        is factorised first, O(N^3) once).  The hyperparameters are COPIED, neither shared nor refitted: fitting either model
        later leaves the other alone.  The new targets are scaled with THIS model's ``y_min`` / ``y_std`` — the hyperparameters
        were fitted in that scaling — and both buffers are kept; a model constructed on all N + q rows would rescale by the joint
        range, so its ``y_scaled`` (and, after a fit, its parameters) differ from the conditioned model's.  The new rows go
        through the model's own ``forward`` and likelihood as the training rows do: latent map, per-source means, per-source
        noise of the rows' own source column.  ``reserve``: rows of spare capacity in the new model's matrices; appends within
        it run in place (``prediction_strategy.route`` is "in_place", "copy" or "refactor").  ``train()`` on the new model drops
        the cache like on any model, and ``fit()`` then trains on N + q points.

        ``ValueError`` before any kernel runs: wrong column count, length mismatch, NaN / inf, q = 0, a categorical level or a
        source the model has not seen.  ``NotImplementedError`` under ``settings.sharded_evaluation`` or a graph capture."""
        from .. import settings as gpp_settings
        from ..backend import get_context
        from ..gpcore.module import Module
        from ..linalg import append_to_cache
        from ..utils import data_type_check

        X, y = data_type_check(X), data_type_check(y)
        train_x = self.train_inputs[0]
        if X.dim() != 2 or X.shape[1] != train_x.shape[1]:
            raise ValueError(f"condition_on: X must be (q, {train_x.shape[1]}) like the training inputs (got {tuple(X.shape)})")
        y = y.reshape(-1)
        if y.shape[0] != X.shape[0]:
            raise ValueError(f"condition_on: {X.shape[0]} rows of X for {y.shape[0]} targets")
        if X.shape[0] == 0:
            raise ValueError("condition_on: no observation given (q = 0)")
        if not (bool(torch.isfinite(X).all()) and bool(torch.isfinite(y).all())):
            raise ValueError("condition_on: X and y must be finite (NaN or inf found)")
        self._check_new_rows(X)
        if gpp_settings.sharded_evaluation.value() is not None:
            raise NotImplementedError("condition_on is not available under settings.sharded_evaluation")
        get_context(train_x.device)  # (raises for anything but a GPU: there is no CPU path)

        Xq = X.to(train_x)
        yq = (y.to(self.train_targets) - self.y_min) / self.y_std
        self.eval()
        with torch.no_grad():
            cache = self._ensure_prediction_cache()
            out_q = Module.__call__(self, Xq)
            cov_q = out_q.lazy_covariance_matrix
            noisy = self._likelihood_of_rows(out_q, Xq).lazy_covariance_matrix
            new_cache = append_to_cache(cache, cov_q.U1, noisy.tau, noisy.grp, out_q.mean, yq, reserve)

            child = self._copy_without_factors()
            child.train_inputs = (torch.cat([train_x, Xq]),)
            targets = torch.cat([self.train_targets, yq])
            child.train_targets = targets
            child.y_scaled = targets
            if hasattr(child.likelihood, "fidel_indices"):
                child.likelihood.fidel_indices = child.train_inputs[0][:, -1]
            if hasattr(child, "count"):
                child.count = targets.shape[0]
            child.eval()
            child.prediction_strategy = new_cache
        return child

    def _alc_rows(self, X, name: str, what: str = "variance_reduction") -> torch.Tensor:
        """A candidate or reference set of ``variance_reduction`` / ``knowledge_gradient``, checked on the host like
        ``condition_on``'s new rows."""
        from ..utils import data_type_check

        X = data_type_check(X)
        train_x = self.train_inputs[0]
        if X.dim() != 2 or X.shape[1] != train_x.shape[1]:
            raise ValueError(f"{what}: {name} must be (m, {train_x.shape[1]}) like the training inputs "
                             f"(got {tuple(X.shape)})")
        if X.shape[0] == 0:
            raise ValueError(f"{what}: {name} is empty")
        if not bool(torch.isfinite(X).all()):
            raise ValueError(f"{what}: {name} must be finite (NaN or inf found)")
        self._check_new_rows(X)
        return X

    def _noise_of_rows(self, out, X) -> torch.Tensor:
        """The noise level of each row's own source (fp64, one per row of ``X``; ``out``: the model's prior at ``X``), as
        ``condition_on`` gives a new row."""
        noisy = self._likelihood_of_rows(out, X).lazy_covariance_matrix
        tau = noisy.tau.detach().reshape(-1).to(torch.float64)
        return tau[noisy.grp.long()] if noisy.grp is not None else tau[:1].expand(X.shape[0])

    def _score_preamble(self, what: str, row_sets, cache=None):
        """What every score does once its arguments are validated: refused under ``settings.sharded_evaluation``, a GPU context or
        none (there is no CPU path), eval mode, the prediction cache (``cache`` None) and the model's prior at each validated row
        set.  Returns (cache, the row sets on the model's device and dtype, their priors)."""
        from .. import settings as gpp_settings
        from ..backend import get_context
        from ..gpcore.module import Module

        if gpp_settings.sharded_evaluation.value() is not None:
            raise NotImplementedError(f"{what} is not available under settings.sharded_evaluation")
        train_x = self.train_inputs[0]
        get_context(train_x.device)  # (raises for anything but a GPU: there is no CPU path)
        row_sets = [X.to(train_x) for X in row_sets]
        self.eval()
        with torch.no_grad():
            if cache is None:
                cache = self._ensure_prediction_cache()
            return cache, row_sets, [Module.__call__(self, X) for X in row_sets]

    def _variance_reduction(self, Xcand, Xref, weights=None, q: int = 1, cost=None):
        """(first-round scores, picked rows of ``Xcand``, their gains) of ``linalg.variance_reduction``, in y^2 units: the work behind
        ``variance_reduction`` and ``bayesian_optimizations.select_by_variance_reduction``.  Everything is validated on the host
        before any device work."""
        from ..linalg import variance_reduction

        what = "variance_reduction"
        Xc, Xr = self._alc_rows(Xcand, "Xcand"), self._alc_rows(Xref, "Xref")
        weights = _check_weights(what, weights, Xr.shape[0], "reference rows")
        cost = _check_cost(what, cost, Xc.shape[0])
        q = _check_q(what, q, Xc.shape[0])
        cache, (Xc, Xr), (out_c, out_r) = self._score_preamble(what, (Xc, Xr))
        with torch.no_grad():
            dev = Xc.device
            first, picks, gains = variance_reduction(cache, out_c.lazy_covariance_matrix.U1, self._noise_of_rows(out_c, Xc),
                                                     out_r.lazy_covariance_matrix.U1,
                                                     omega=None if weights is None else weights.to(dev), q=q,
                                                     cost=None if cost is None else cost.to(dev))
            scale = self.y_std.to(torch.float64) ** 2
            return first * scale, picks, gains * scale

    def variance_reduction(self, Xcand, Xref, weights=None) -> torch.Tensor:
        """Active learning (Cohn's ALC; IMSE over a reference set): for every row of ``Xcand`` the expected reduction of the
        weighted posterior variance of the latent f over the rows of ``Xref`` from ONE noisy observation at that row,
            sum_r w_r var_before(x_r) - sum_r w_r var_after(x_r),        w_r = ``weights`` (default 1 / M_r each),
        in the units of y^2 (``predict``'s std squared).  The posterior variance after an observation does not depend on the
        observed value, so nothing is conditioned and nothing is factorised: the scores come from the cached factor through
        gpp_post_cross_sq, which never forms the M_c x M_r cross-covariance.  No reference counterpart.

        Rows go through the model's ``forward`` and likelihood as ``condition_on`` sends new rows: latent map, per-source noise of
        each candidate's own source column.  A multi-fidelity user passes candidates of several sources and reference rows of the
        high-fidelity source.  The model is put in eval mode and is otherwise untouched; a warm cache is reused.

        ``ValueError`` before any device work: wrong column count, an empty set, NaN / inf, negative or all-zero weights, a wrong
        weights length, a categorical level or source the model has not seen.  ``NotImplementedError`` under
        ``settings.sharded_evaluation`` or a graph capture."""
        return self._variance_reduction(Xcand, Xref, weights)[0]

    def _knowledge_gradient(self, Xcand, Xref, q: int = 1, cost=None, maximize: bool = False, num_nodes: int = 32):
        """(first-round scores, picked rows of ``Xcand``, their gains) of ``linalg.knowledge_gradient``, in the units of y: the work
        behind ``knowledge_gradient`` and ``bayesian_optimizations.select_by_knowledge_gradient``.  Everything is validated on the
        host before any device work."""
        from ..backend import MAX_NODES
        from ..linalg import knowledge_gradient, predict_from_cache

        what = "knowledge_gradient"
        Xc, Xr = self._alc_rows(Xcand, "Xcand", what), self._alc_rows(Xref, "Xref", what)
        cost = _check_cost(what, cost, Xc.shape[0])
        q, num_nodes = _check_q(what, q, Xc.shape[0]), int(num_nodes)
        if num_nodes < 1 or num_nodes > MAX_NODES:
            raise ValueError(f"{what}: num_nodes must be between 1 and {MAX_NODES}; got {num_nodes}")
        cache, (Xc, Xr), (out_c, out_r) = self._score_preamble(what, (Xc, Xr))
        with torch.no_grad():
            Ur = out_r.lazy_covariance_matrix.U1
            tau_c = self._noise_of_rows(out_c, Xc)
            cache.refresh()
            mean_r = out_r.mean.to(torch.float64) + predict_from_cache(cache, Ur, need_var=False)[0]
            first, picks, gains = knowledge_gradient(cache, out_c.lazy_covariance_matrix.U1, tau_c, Ur, mean_r, q=q,
                                                     cost=None if cost is None else cost.to(Xc.device), maximize=bool(maximize),
                                                     num_nodes=num_nodes)
            scale = self.y_std.to(torch.float64).abs()
            return first * scale, picks, gains * scale

    def knowledge_gradient(self, Xcand, Xref, maximize: bool = False, num_nodes: int = 32) -> torch.Tensor:
        """Optimisation by the knowledge gradient (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011): for every row of
        ``Xcand`` the expected drop of the minimum (``maximize``: the expected rise of the maximum) of the posterior mean over the
        rows of ``Xref`` from ONE noisy observation at that row,
            min_r mu(x_r) - E[ min_r mu_after(x_r) ],
        in the units of y.  A cheap low-fidelity run scores by what it does to the high-fidelity optimum elsewhere: a
        multi-fidelity user passes candidates of several sources and reference rows of the high-fidelity source, and divides by
        each source's cost (``select_by_knowledge_gradient``).  The candidate's own location takes part in the minimum only if the
        caller puts it in ``Xref``.

        The expectation over the observed value is APPROXIMATED by a deterministic Gauss-Hermite rule with ``num_nodes`` nodes
        (1..64), not computed exactly through the lower envelope of the M_r lines: at 32 nodes the error measured on the
        multi-fidelity fixture is about 2 % of the largest score, with the same best candidate; more nodes, less
        error.  Nothing is conditioned and nothing is factorised: per node the minimum comes from the cached factor through
        gpp_post_cross_min, which never forms the M_c x M_r cross-covariance.  No reference counterpart (the reference's AFs.py
        scores a point by the prediction at that point only).

        Rows go through the model's ``forward`` and likelihood as in ``variance_reduction``: latent map, per-source noise of each
        candidate's own source column.  The model is put in eval mode and is otherwise untouched; a warm cache is reused.

        ``ValueError`` before any device work: wrong column count, an empty set, NaN / inf, a categorical level or source the model
        has not seen, ``num_nodes`` outside 1..64.  ``NotImplementedError`` under ``settings.sharded_evaluation`` or a graph
        capture."""
        return self._knowledge_gradient(Xcand, Xref, maximize=maximize, num_nodes=num_nodes)[0]

    def reset_parameters(self) -> None:
        """Reset parameters by sampling from their priors (models/gpregression.py:168-174)."""
        # The reference builds its priors from Python numbers (torch's default dtype, float32) and never casts them on its
        # CPU path, so every draw is made in that dtype and converted afterwards — whatever ``dtype`` the model was given.
        # Here a model is created in its dtype, buffers of the priors included; the expanded copy is put back first so
        # that one seed gives the start points the reference would draw (tests/test_restart_sampling.py).
        draw_dtype = torch.get_default_dtype()
        for _, module, prior, closure, setting_closure in self.named_priors():
            current = closure(module)
            if not current.requires_grad:
                continue  # (consumes no random numbers)
            sampler = prior.expand(current.shape).to(dtype=draw_dtype)
            setting_closure(module, sampler.sample().to(**self.tkwargs))

"""``ExactMarginalLogLikelihood`` (gpytorch.mlls subset; reference use: optim/mll_torch.py:17,96,116):
    (log p(y | X) + sum of prior log-densities) / N
and ``LeaveOneOutPseudoLikelihood`` (gpytorch.mlls.LeaveOneOutPseudoLikelihood; Rasmussen & Williams 5.4.2):
    (sum_i log p(y_i | X, y_-i) + sum of prior log-densities) / N
and ``CrossValidationPseudoLikelihood``, its grouped (k-fold, leave-one-group-out) form (no gpytorch counterpart):
    (sum_F log p(y_F | X, y_-F) + sum of prior log-densities) / N
"""
import torch

from .distributions import MultivariateNormal
from .module import Module


class ExactMarginalLogLikelihood(Module):
    def __init__(self, likelihood, model):
        super().__init__()
        self.likelihood = likelihood
        self.model = model

    def forward(self, function_dist: MultivariateNormal, target: torch.Tensor, *params):
        if not isinstance(function_dist, MultivariateNormal):
            raise RuntimeError("ExactMarginalLogLikelihood can only operate on Gaussian random variables")
        num_data = function_dist.event_shape.numel()
        output = self.likelihood(function_dist, *params)
        res = output.log_prob(target)
        prior_sum = self._prior_sum(res.dtype)
        if prior_sum is not None:
            res = res + prior_sum
        return res / num_data

    def _prior_sum(self, dtype):
        """Sum of the prior log-densities ([3P] ExactMarginalLogLikelihood adds them to the likelihood term one by one; here they
        are summed first, in registration order, and added once).  None when the model has no priors."""
        total = None
        for _, module, prior, closure, _ in self.named_priors():
            term = prior.log_prob(closure(module)).sum().to(dtype)
            total = term if total is None else total + term
        return total

    def named_priors(self, memo=None, prefix=""):
        # priors of the model (which includes the likelihood's) — the MLL module itself has none
        yield from self.model.named_priors(memo, prefix)


class LeaveOneOutPseudoLikelihood(ExactMarginalLogLikelihood):
    """The leave-one-out log pseudo-likelihood as a training criterion, with gpytorch's scaling: the sum of the N leave-one-out
    predictive log-densities plus the prior log-densities, divided by N (``MultivariateNormal.loo_log_prob``)."""

    def forward(self, function_dist: MultivariateNormal, target: torch.Tensor, *params):
        if not isinstance(function_dist, MultivariateNormal):
            raise RuntimeError("LeaveOneOutPseudoLikelihood can only operate on Gaussian random variables")
        num_data = function_dist.event_shape.numel()
        output = self.likelihood(function_dist, *params)
        res = output.loo_log_prob(target)
        prior_sum = self._prior_sum(res.dtype)
        if prior_sum is not None:
            res = res + prior_sum
        return res / num_data


class CrossValidationPseudoLikelihood(ExactMarginalLogLikelihood):
    """The grouped cross-validation log pseudo-likelihood as a training criterion, in the scaling of
    :class:`LeaveOneOutPseudoLikelihood`: the sum over the folds of the held-out log-densities log p(y_F | X, y_-F) plus the prior
    log-densities, divided by N (``MultivariateNormal.cv_log_prob``).  ``folds``: an int k (a seeded random partition), one integer
    label per training row, or a ``cv.FoldIndex``; normalised once, here."""

    def __init__(self, likelihood, model, folds):
        super().__init__(likelihood, model)
        from ..cv import FoldIndex
        self.folds = FoldIndex.make(folds, int(model.train_targets.shape[0]))

    def forward(self, function_dist: MultivariateNormal, target: torch.Tensor, *params):
        if not isinstance(function_dist, MultivariateNormal):
            raise RuntimeError("CrossValidationPseudoLikelihood can only operate on Gaussian random variables")
        num_data = function_dist.event_shape.numel()
        output = self.likelihood(function_dist, *params)
        res = output.cv_log_prob(target, self.folds)
        prior_sum = self._prior_sum(res.dtype)
        if prior_sum is not None:
            res = res + prior_sum
        return res / num_data


class GradientEnhancedMarginalLogLikelihood(ExactMarginalLogLikelihood):
    """The joint marginal log-likelihood of the training targets AND of gradients observed at the rows ``Xg`` — gradient-enhanced
    Kriging as a training criterion — in the scaling of :class:`ExactMarginalLogLikelihood` with n = N + q observations, q = Mg p:
        (log N([y - mean; dY / y_std] | 0, Kj) + sum of prior log-densities) / n
    (``MultivariateNormal.gek_log_prob``, ``linalg.exact_gek_mll``).  ``Xg``: (Mg, columns of the training inputs); ``dY``: (Mg, p),
    d y / d x over the quantitative columns in ``quant_index`` order, y per input unit; ``noise``: their variances in (y per input
    unit)^2, a scalar or anything that broadcasts to (Mg, p), constant during the fit — None takes
    ``gradient_enhanced.GRADIENT_NUGGET_REL`` times the prior curvature at the current hyperparameters.  ``observed``: a bool mask
    that broadcasts to (Mg, p), for partial gradients: only its True entries of ``dY`` (and of ``noise``) are observations, the rest
    is not read, and q is their number.  The data are validated once, here, as ``GP_Plus.condition_on_gradients`` validates them
    (the number of observations is limited by memory alone)."""

    def __init__(self, likelihood, model, Xg, dY, noise=None, observed=None):
        super().__init__(likelihood, model)
        from ..gradient_enhanced import check_gradient_observations

        if len(getattr(model, "calibration_id", ())) > 0:
            raise NotImplementedError("the gradient-enhanced objective is not available for a model with calibration parameters: "
                                      "gradient observations by a calibrated column are not defined")
        Xg, dY, noise, observed = check_gradient_observations(model, Xg, dY, noise, "GradientEnhancedMarginalLogLikelihood", observed)
        train_x = model.train_inputs[0]
        y_std = model.y_std.detach().to(device=train_x.device, dtype=torch.float64)
        self.Xg = Xg.to(train_x)
        self.r_g = (dY.to(device=train_x.device, dtype=torch.float64) / y_std).contiguous()
        self.noise = None if noise is None else (noise.to(train_x.device) / y_std ** 2).contiguous()
        self.num_directions = int(model.quant_index.numel())
        self.selection = None
        if observed is not None:  # the q observed entries alone, in the selection's order
            from ..backend import GradientSelection

            self.selection = sel = GradientSelection(observed, train_x.device)
            self.r_g = self.r_g.reshape(-1)[sel.flat].contiguous()
            self.noise = None if self.noise is None else self.noise.reshape(-1)[sel.flat].contiguous()

    def joint_log_prob(self, output: MultivariateNormal, target: torch.Tensor) -> torch.Tensor:
        """log N([target - mean; dY / y_std] | 0, Kj) for the noisy training distribution ``output``: neither normalised nor with
        the priors (what the scipy driver adds its own terms to).  The gradient points go through the model's ``forward`` here,
        at the current parameters: their latent columns carry the categorical map's graph."""
        p = self.num_directions
        Ug = Module.__call__(self.model, self.Xg).lazy_covariance_matrix.U1
        return output.gek_log_prob(target, (Ug, self.r_g, self.noise, Ug.shape[1] - p, p, self.selection))

    def forward(self, function_dist: MultivariateNormal, target: torch.Tensor, *params):
        if not isinstance(function_dist, MultivariateNormal):
            raise RuntimeError("GradientEnhancedMarginalLogLikelihood can only operate on Gaussian random variables")
        num_data = function_dist.event_shape.numel() + self.r_g.numel()
        res = self.joint_log_prob(self.likelihood(function_dist, *params), target)
        prior_sum = self._prior_sum(res.dtype)
        if prior_sum is not None:
            res = res + prior_sum
        return res / num_data

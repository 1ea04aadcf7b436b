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

"""``ExactGP`` (gpytorch.models.ExactGP subset): train-mode call returns the prior at the training inputs, eval-mode
call returns the exact predictive distribution through a cached factorisation (gpytorch's prediction strategy),
computed by the HIP back end (linalg.factorize / predict_from_cache)."""
from __future__ import annotations


import torch

from .. import settings
from .distributions import DenseCovariance, MultivariateNormal
from .kernels import LazyKernelMatrix
from .module import Module


class GP(Module):
    pass


def _same_inputs(inputs, train_inputs) -> bool:
    """True when the eval-mode inputs are the training inputs: the same tensors, or equal ones (``torch.equal`` waits for the
    GPU, so it is asked only when a draw needs the answer)."""
    if train_inputs is None or len(inputs) != len(train_inputs):
        return False
    for x, t in zip(inputs, train_inputs):
        if x is t:
            continue
        if not (torch.is_tensor(x) and x.shape == t.shape and x.dtype == t.dtype and x.device == t.device and torch.equal(x, t)):
            return False
    return True


class ExactGP(GP):
    def __init__(self, train_inputs, train_targets, likelihood):
        if train_inputs is not None and torch.is_tensor(train_inputs):
            train_inputs = (train_inputs,)
        super().__init__()
        self.train_inputs = None if train_inputs is None else tuple(
            (i.unsqueeze(-1) if i.ndimension() == 1 else i) for i in train_inputs)
        self.train_targets = train_targets
        self.likelihood = likelihood
        self.prediction_strategy = None

    def _apply(self, fn, *args, **kwargs):
        if self.train_inputs is not None:
            self.train_inputs = tuple(fn(t) for t in self.train_inputs)
            self.train_targets = fn(self.train_targets)
        return super()._apply(fn, *args, **kwargs)

    def train(self, mode: bool = True):
        if mode:
            self.prediction_strategy = None
        return super().train(mode)

    def _likelihood_of_rows(self, out, X):
        """``likelihood(out)`` with the noise of each row's own source: a likelihood with ``fidel_indices`` reads the source column of
        the rows ``X`` for the call — whatever a previous predict() / evaluation() left there (models/gpregression.py:136-139
        overwrites it with the test points' sources) — and gets the caller's value back."""
        lik = self.likelihood
        swap = hasattr(lik, "fidel_indices")
        if swap:
            saved, lik.fidel_indices = lik.fidel_indices, X[:, -1]
        try:
            return lik(out)
        finally:
            if swap:
                lik.fidel_indices = saved

    def _ensure_prediction_cache(self, **kwargs):
        """Factor the training covariance once per eval() phase (gpytorch's prediction strategy caches)."""
        from ..linalg import factorize

        if self.prediction_strategy is not None and self.prediction_strategy.stale():
            self.prediction_strategy = None  # another model reused the prediction workspace: factor again
        if self.prediction_strategy is None:
            with torch.no_grad():
                train_out = Module.__call__(self, *self.train_inputs, **kwargs)
                cov = train_out.lazy_covariance_matrix
                if not isinstance(cov, LazyKernelMatrix):
                    raise RuntimeError("exact prediction needs the model's forward to return a lazy kernel covariance")
                noisy = self._likelihood_of_rows(train_out, self.train_inputs[0]).lazy_covariance_matrix
                self.prediction_strategy = factorize(cov.U1, cov.spec, noisy.tau, noisy.grp, train_out.mean, self.train_targets)
        return self.prediction_strategy

    def __call__(self, *args, **kwargs):
        inputs = [a.unsqueeze(-1) if torch.is_tensor(a) and a.ndimension() == 1 else a for a in args]
        if self.training:
            if self.train_inputs is None:
                raise RuntimeError("train_inputs, train_targets cannot be None in training mode.")
            if not all(ti is x or torch.equal(ti, x) for ti, x in zip(self.train_inputs, inputs)):  # (equal() waits for the GPU)
                raise RuntimeError("You must train on the training inputs!")
            return Module.__call__(self, *inputs, **kwargs)
        # ---- posterior mode -----------------------------------------------------------------------
        if settings.differentiable_predictions.value() and torch.is_grad_enabled() and (
                any(torch.is_tensor(a) and a.requires_grad for a in inputs) or any(p.requires_grad for p in self.parameters())):
            return self._differentiable_posterior(inputs, kwargs)
        from ..linalg import factorize, predict_from_cache, cross_kernel

        with torch.no_grad():
            self._ensure_prediction_cache(**kwargs)
            cache = self.prediction_strategy
            test_out = Module.__call__(self, *inputs, **kwargs)
            tcov = test_out.lazy_covariance_matrix
            Us = tcov.U1.to(torch.float64).contiguous()
            # the mean is O(M N) and computed now; the variance needs V = K_*N L^-T (M N^2 flops) and is computed when — if —
            # somebody asks for it (predict(return_std=False), the acquisition means of a BO loop and Sobol's p + 2 batches do not)
            mean_c, _, _ = predict_from_cache(cache, Us, need_var=False)
            pred_mean = test_out.mean.to(torch.float64) + mean_c
            lazy = {}

            def var_and_v(cache=cache, Us=Us):
                if "V" not in lazy:
                    # another model of the same size may have factored into the shared workspace since this prediction was
                    # made (p1 = m1(x); p2 = m2(x); p1.stddev): the cache rebuilds its factor from its own inputs
                    cache.refresh()
                    with torch.no_grad():
                        _, lazy["var"], lazy["V"] = predict_from_cache(cache, Us, need_var=True, need_V=True)
                return lazy["var"], lazy["V"]

            def full_cov(Us=Us, spec=cache.spec, gctx=cache.gctx):
                M = Us.shape[0]
                V = var_and_v()[1]
                Kss = LazyKernelMatrix(Us, None, spec).evaluate()
                # Kss - V V^T through the MFMA GEMM (NT, lower + mirrored by symmetry)
                gctx.gemm(0, 1, M, M, V.shape[1], -1.0, V, V, 1.0, Kss)
                return Kss

            train_inputs = self.train_inputs

            def cov_upper(A, added, jitter, Us=Us, spec=cache.spec, cache=cache):
                # what rsample factors: at the training inputs Sigma = T - T Ky^-1 T (+ the likelihood's diagonal), which does
                # not lose the O(tau) result to a difference of O(sf2) terms and needs no V; elsewhere Kss - V V^T
                from ..linalg import predictive_cov_upper, train_post_cov_upper

                if not kwargs and _same_inputs(inputs, train_inputs):
                    return train_post_cov_upper(cache, added, jitter, out=A)
                return predictive_cov_upper(Us, spec, var_and_v()[1], added, jitter, out=A)

            return MultivariateNormal(pred_mean, DenseCovariance(lambda: var_and_v()[0], full_cov, n=Us.shape[0],
                                                                 upper_builder=cov_upper))

    def _differentiable_posterior(self, inputs, kwargs):
        """The eval-mode call under ``settings.differentiable_predictions``: the same factor cache and the same numbers as the
        no-grad path, with the test features and test mean (and, when a latent map makes them depend on parameters, the training
        features) built under autograd.  The mean and the variance diagonal are autograd-connected (linalg.predict_mean /
        predict_var); the joint covariance is not offered."""
        from ..linalg import predict_mean, predict_var

        with torch.no_grad():
            cache = self._ensure_prediction_cache(**kwargs)
        test_out = Module.__call__(self, *inputs, **kwargs)
        tcov = test_out.lazy_covariance_matrix
        if not isinstance(tcov, LazyKernelMatrix):
            raise RuntimeError("exact prediction needs the model's forward to return a lazy kernel covariance")
        Us, spec = tcov.U1.to(torch.float64), tcov.spec
        Utr, dB = None, 0
        # (n_grad_dims == 0: no feature column depends on a parameter — no latent map — and the training features are constants)
        if tcov.n_grad_dims != 0 and any(p.requires_grad for p in self.parameters()):
            trcov = Module.__call__(self, *self.train_inputs, **kwargs).lazy_covariance_matrix
            if trcov.U1.requires_grad:
                dB = trcov.n_grad_dims if trcov.n_grad_dims is not None else trcov.U1.shape[1]
                if dB > 0:
                    Utr = trcov.U1.to(torch.float64)
        pred_mean = test_out.mean.to(torch.float64) + predict_mean(cache, Us, Utr, spec.w, spec.sf2, dB)
        lazy = {}

        def var():
            if "var" not in lazy:
                lazy["var"] = predict_var(cache, Us, Utr, spec.w, spec.sf2, dB)
            return lazy["var"]

        def full_cov():
            raise NotImplementedError("the joint predictive covariance of a differentiable prediction is not available "
                                      "(only its mean and variance carry gradients); predict without "
                                      "settings.differentiable_predictions for covariance_matrix")

        def no_draws(A, added, jitter):
            raise NotImplementedError("sampling from a differentiable prediction is not available (only its mean and variance "
                                      "carry gradients); sample without settings.differentiable_predictions")

        return MultivariateNormal(pred_mean, DenseCovariance(var, full_cov, n=Us.shape[0], upper_builder=no_draws))

"""L-BFGS-B (and friends) multistart fit driver through scipy (reference: optim/mll_scipy.py:37-307).

Same objective and surface as the reference — ``obj = -(log_prob + sum of prior log-densities)`` (NOT divided by N,
optim/mll_scipy.py:37-43,120), parameter pack/unpack over ``named_parameters`` with ``requires_grad``, the bounds table
(:149-183), method defaults (:261-271), NotPSD/NaN starts scored ``inf`` (:232-240,295) — with every evaluation on the
HIP back end.  Differences, by design:
  * the starts run one after the other on the GPU instead of in joblib/loky worker processes (:287-293); with an
    initialised process group use ``fit_restarts_parallel(model, fit_fn=fit_model_scipy, ...)`` to spread them over GPUs;
  * restart points come from ``model.reset_parameters()`` (prior samples pushed through the parameters' own setting
    closures) — the reference concatenates prior samples in ``named_priors`` order and on the constrained scale for the
    outputscale (:130-137), which does not line up with its own packing order;
  * parameters keep the model's dtype; the reference round-trips theta through fp32 (:32-35,97), which
    ``settings.reference_fp32_theta(True)`` reproduces;
  * the interval-score term and the NN-weight regularisers (:44-59) belong to out-of-scope model variants.
"""
from collections import OrderedDict
from copy import deepcopy
from functools import reduce
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from scipy.optimize import Bounds, OptimizeResult, minimize

from ..errors import NanError, NotPSDError


def marginal_log_likelihood(model, add_prior: bool, regularization_parameter=[0, 0], objective: str = "mll", folds=None,
                            gradients=None):
    """optim/mll_scipy.py:37-60 (exact log-marginal + priors, un-normalised).  ``objective="loo"``: the leave-one-out log
    pseudo-likelihood in place of the log-marginal; ``objective="cv"``: the grouped cross-validation one over ``folds``;
    ``objective="gek"``: the joint log-marginal of the targets and of observed gradients, ``gradients`` a
    ``GradientEnhancedMarginalLogLikelihood`` that holds the validated data."""
    from .mll_torch import check_objective_folds

    folds = check_objective_folds(objective, folds, int(model.train_targets.shape[0]))
    if (objective == "gek") != (gradients is not None):
        raise ValueError('objective="gek" and gradients= go together')
    output = model(*model.train_inputs)
    noisy = model.likelihood(output)
    if objective == "gek":
        out = gradients.joint_log_prob(noisy, model.train_targets)
    elif objective == "cv":
        out = noisy.cv_log_prob(model.train_targets, folds)
    else:
        out = noisy.loo_log_prob(model.train_targets) if objective == "loo" else noisy.log_prob(model.train_targets)
    if add_prior:
        for _, module, prior, closure, _ in model.named_priors():
            out = out + prior.log_prob(closure(module)).sum().to(out)
    if getattr(model, "interval_score", False):
        raise NotImplementedError("the interval-score objective term (optim/mll_scipy.py:57-59) is outside this build's scope")
    return out


class MLLObjective:
    """optim/mll_scipy.py:63-127."""

    def __init__(self, model, add_prior, regularization_parameter, objective: str = "mll", folds=None, gradients=None):
        from .mll_torch import check_objective, check_objective_folds, check_objective_gradients

        self.model, self.add_prior, self.regularization_parameter = model, add_prior, regularization_parameter
        self.objective = check_objective(objective)
        self.folds = check_objective_folds(objective, folds, int(model.train_targets.shape[0]))  # normalised once per fit
        gradients = check_objective_gradients(objective, gradients)
        self.gradients = None
        if gradients is not None:  # validated and scaled once per fit
            from ..gpcore.mlls import GradientEnhancedMarginalLogLikelihood

            self.gradients = GradientEnhancedMarginalLogLikelihood(model.likelihood, model, *gradients)
        self.param_shapes = OrderedDict()
        for n, p in self.model.named_parameters():
            if p.requires_grad:
                self.param_shapes[n] = p.size() if len(p.size()) > 0 else torch.Size([1])

    def _params(self):
        return OrderedDict([(n, p) for n, p in self.model.named_parameters() if p.requires_grad])

    def pack_parameters(self) -> np.ndarray:
        return np.concatenate([p.detach().cpu().double().numpy().ravel() for p in self._params().values()])

    def unpack_parameters(self, x: np.ndarray) -> "OrderedDict[str, torch.Tensor]":
        i, named = 0, OrderedDict()
        params = self._params()
        x = self._theta(x)
        for n, shape in self.param_shapes.items():
            ln = reduce(lambda a, b: a * b, shape)
            named[n] = torch.from_numpy(np.asarray(x[i:i + ln], dtype=np.float64).reshape(*shape)).to(params[n]).reshape(params[n].shape)
            i += ln
        return named

    @staticmethod
    def _theta(x: np.ndarray) -> np.ndarray:
        """theta as the model will see it: float32-rounded under ``settings.reference_fp32_theta`` (optim/mll_scipy.py:32-35,97)."""
        from .. import settings

        x = np.asarray(x, dtype=np.float64)
        return x.astype(np.float32).astype(np.float64) if settings.reference_fp32_theta.value() else x

    def pack_grads(self) -> np.ndarray:
        return np.concatenate([p.grad.detach().cpu().double().numpy().ravel() for p in self._params().values()]).astype(np.float64)

    def _graphed(self):
        """The replayed form of ``fun`` (gp-plus_amd/graphed.py), built on first use; None when it does not apply."""
        if getattr(self, "_graph", None) is None and not getattr(self, "_graph_failed", False):
            from .. import settings
            from ..graphed import GraphedObjective
            from ..linalg import LOOKAHEAD_MIN_N

            params = list(self._params().values())
            dev = params[0].device if params else torch.device("cpu")
            n_points = self.model.train_inputs[0].shape[0]
            ok = (self.objective == "mll" and settings.graphed_objective.value() and dev.type == "cuda" and n_points < LOOKAHEAD_MIN_N
                  and settings.sharded_evaluation.value() is None and not getattr(self.model, "interval_score", False)
                  and not getattr(self.model, "calibration_id", None))  # (calibrated models: the eager evaluation)
            if not ok:
                self._graph_failed = True
                return None
            try:
                self._graph = GraphedObjective(
                    lambda: -marginal_log_likelihood(self.model, self.add_prior, self.regularization_parameter), params,
                    n_points, dev)
            except (NotPSDError, NanError):  # an indefinite warm-up point: the eager path has the jitter policy for it
                self._graph_failed = True
                return None
            except RuntimeError as exc:  # a capture the stack refuses — the eager evaluation is the same computation, but say so
                import warnings

                warnings.warn(f"fit_model_scipy: the objective could not be captured as a HIP graph ({exc}); evaluating eagerly",
                              RuntimeWarning)
                self._graph_failed = True
                return None
        return getattr(self, "_graph", None)

    def fun(self, x: np.ndarray, return_grad=True) -> Union[float, Tuple[float, np.ndarray]]:
        g = self._graphed() if return_grad else None
        if g is not None:
            res = g.evaluate(self._theta(x))
            if res is not None:
                return res
            # the factorisation failed without jitter (or the objective is not finite): this point goes the eager way
            from ..backend import INFO_PANEL_TIMEOUT
            if g.last_status >= INFO_PANEL_TIMEOUT:
                # a cooperative panel launch inside the graph timed out (another tenant of this GPU): the eager evaluation below
                # switches the panel off for this context, and the graph is captured again without it at the next call
                self._graph = None
        old = self.model.state_dict()
        old.update(self.unpack_parameters(x))
        self.model.load_state_dict(old)
        self.model.zero_grad()
        obj = -marginal_log_likelihood(self.model, self.add_prior, self.regularization_parameter, self.objective, self.folds,
                                       self.gradients)
        if return_grad:
            obj.backward()
            return obj.item(), self.pack_grads()
        return obj.item()


def get_bounds(likobj: MLLObjective, theta: np.ndarray):
    """optim/mll_scipy.py:149-183."""
    lo, hi = [], []
    for name, values in likobj.unpack_parameters(theta).items():
        n = values.numel()
        if name == 'likelihood.noise_covar.raw_noise' or name.startswith('[') or name.startswith('latent['):
            a, b = -np.inf, np.inf
        elif 'raw_lengthscale' in name or name.startswith('covar_module'):
            a, b = -10.0, 3.0
        elif name.startswith('mean'):
            a, b = -1.5, 1.5
        elif name.startswith('Theta_'):  # calibration parameters (optim/mll_scipy.py:173-175)
            a, b = -15.0, 15.0
        else:
            a, b = -np.inf, np.inf
        lo += [a] * n
        hi += [b] * n
    return np.array(lo), np.array(hi)


def _fit_model_from_state(likobj, theta0, jac, options, method='L-BFGS-B', constraint=False, bounds=False):
    if constraint:
        raise NotImplementedError("latent-position constraints (optim/mll_scipy.py:140-147,189) are outside this build's scope")
    bnds = Bounds(*get_bounds(likobj, theta0)) if bounds else None
    try:
        return minimize(fun=likobj.fun, x0=theta0, args=(True) if jac else (False), method=method, jac=jac, bounds=bnds,
                        options=options)
    except (NotPSDError, NanError) as e:  # unstable start: scored inf by the caller (optim/mll_scipy.py:232-236,295)
        # The exception is RETURNED and lives on in the caller's result list (as in the reference) — without its traceback: the
        # frames of the failed evaluation (the autograd Function's forward, its tensors, its context) would stay alive with it, and
        # with them alive the NEXT HIP-graph capture on this stack dies in hipStreamEndCapture (round 6: found by the continuation
        # driver, whose level below the noise bound fails by design and is followed by more fits; minimal reproducer
        # tools/attic/dev/capture_bisect.py — `fun_keep_exc` crashes, `keep_no_tb` does not).
        return e.with_traceback(None)


def fit_model_scipy(model, add_prior: bool = True, num_restarts: int = 1, theta0_list: Optional[List[np.ndarray]] = None,
                    jac: bool = True, options: Dict = {}, n_jobs: int = -1, method='L-BFGS-B', constraint=False,
                    bounds=False, regularization_parameter: List[int] = [0, 0],
                    objective: str = "mll", folds=None, gradients=None) -> Tuple[List[OptimizeResult], float]:
    from .mll_torch import check_objective_folds, check_objective_gradients

    # "loo" / "cv": the leave-one-out / grouped cross-validation log pseudo-likelihood (+ priors), evaluated eagerly;
    # "gek" with gradients=(Xg, dY[, noise]): the joint log-marginal of the targets and the observed gradients, eagerly too
    folds = check_objective_folds(objective, folds, int(model.train_targets.shape[0]))
    check_objective_gradients(objective, gradients)
    if method == 'L-BFGS-B':
        defaults = {'ftol': 1e-6, 'gtol': 1e-5, 'maxfun': 5000, 'maxiter': 2000}
    elif method == 'trust-constr':
        defaults = {'verbose': 1}
    elif method == 'BFGS':
        defaults = {'gtol': 1e-07, 'norm': np.inf, 'eps': 1.4901161193847656e-08, 'maxiter': None, 'disp': False,
                    'return_all': False, 'finite_diff_rel_step': None}
    elif method == 'SLSQP':
        defaults = {'maxiter': 100, 'ftol': 1e-06, 'iprint': 1, 'disp': False, 'eps': 1.4901161193847656e-08,
                    'finite_diff_rel_step': None}
    elif method == 'Newton-CG':
        defaults = {'xtol': 1e-05, 'eps': 1.4901161193847656e-08, 'maxiter': None, 'disp': False, 'return_all': False}
    else:
        raise ValueError('Wrong method')
    for key in options.keys():
        if key not in defaults.keys():
            raise RuntimeError('Unknown option %s!' % key)
        defaults[key] = options[key]

    model.train()
    likobj = MLLObjective(model, add_prior, regularization_parameter, objective, folds, gradients)
    if theta0_list is None:
        theta0_list = [likobj.pack_parameters()]
        if num_restarts > -1:
            start_state = deepcopy(model.state_dict())
            samples = []
            for _ in range(num_restarts + 1):
                model.reset_parameters()
                samples.append(likobj.pack_parameters())
            model.load_state_dict(start_state)
            theta0_list.extend(samples)
            theta0_list.pop(0)  # as the reference: the incumbent point itself is not among the starts
    out = [_fit_model_from_state(likobj, theta0, jac, defaults, method, constraint, bounds) for theta0 in theta0_list]
    # (a start that diverged to a non-finite objective is scored like a failed one; the reference's argmin would pick
    #  the NaN and load NaN parameters into the model)
    nlls_opt = [np.inf if isinstance(res, Exception) or not np.isfinite(res.fun) else res.fun for res in out]
    best_idx = int(np.argmin(nlls_opt))
    if not isinstance(out[best_idx], Exception) and np.isfinite(nlls_opt[best_idx]):
        old = deepcopy(model.state_dict())
        old.update(likobj.unpack_parameters(out[best_idx].x))
        model.load_state_dict(old)
    return out, nlls_opt[best_idx]

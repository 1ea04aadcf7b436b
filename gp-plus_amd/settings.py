"""The handful of gpytorch.settings the path touches.  ``fast_computations`` is accepted and ignored: this back end is
always the exact Cholesky path (the reference forces it with ``fast_computations(log_prob=False)`` at
models/gpregression.py:127,161 and optim/mll_scipy.py:217; optim/mll_torch.py does not, SURVEY.md hazard B-2)."""
import os as _os
from contextlib import contextmanager

# Every environment variable the Python package reads (INTEGRATION.md has the table; the library's own are in csrc/gpp_internal.h,
# GppEnv), parsed once, when the package is imported: set them before that.
ENV_COOP_PANEL = _os.environ.get("GPP_COOP_PANEL", "1") != "0"                          # backend.GppContext.coop_panel
ENV_DAG_SCHED = _os.environ.get("GPP_DAG_SCHED", "1") != "0"                            # backend.GppContext.dag_sched
ENV_SHARD_LIST = _os.environ.get("GPP_SHARD_LIST", "1") not in ("", "0")                # sharded: the per-rank ticket lists
ENV_SHARD_WORKERS = int(_os.environ.get("GPP_SHARD_WORKERS", "0"))                      # sharded: executor work-groups (0: by CU count)
ENV_SHARD_PUSH = _os.environ.get("GPP_SHARD_PUSH", "0") not in ("", "0")                # push.ENABLED: the one-to-all push transport
ENV_SHARDED_FORCE_COLLECTIVES = _os.environ.get("GPP_SHARDED_FORCE_COLLECTIVES", "0") not in ("", "0")  # sharded: one rank, every collective
ENV_SHARD_DEBUG = bool(_os.environ.get("GPP_SHARD_DEBUG"))                              # sharded: print a list's time-out status


class _Value:
    def __init__(self, default):
        self._v = default

    def value(self, *_):
        return self._v

    @contextmanager
    def __call__(self, v):
        old, self._v = self._v, v
        try:
            yield
        finally:
            self._v = old


cholesky_jitter = _Value(1e-8)      # gpytorch.settings.cholesky_jitter (double)
cholesky_max_tries = _Value(3)      # gpytorch.settings.cholesky_max_tries
min_variance = _Value(1e-10)        # gpytorch.settings.min_variance (double)


# Restart-parallel fits on ONE GPU: ``GP_Plus.fit()`` advances the reference's sequential restarts (optim/mll_torch.py:99-141)
# together, one batched evaluation per Adam iteration (optim/mll_batched.py: same start points, same per-run Adam and early
# stop, same winner), whenever the problem is small enough that one evaluation leaves the MI355X mostly idle.
# ``with settings.batched_restarts(False):`` runs the restarts one after the other, exactly as the reference does.
batched_restarts = _Value(True)


# Graph replay of the L-BFGS objective (optim/mll_scipy.py): for small problems, where one evaluation is a chain of ~100 short
# launches issued by ~2 ms of Python, ``fit_model_scipy`` captures objective + gradient once as a HIP graph and replays it per
# evaluation (gp-plus_amd/graphed.py).  ``with settings.graphed_objective(False):`` evaluates eagerly, as the reference does.
graphed_objective = _Value(True)


# The reference's scipy driver casts every slice of theta to float32 before loading it into the model (optim/mll_scipy.py:32-35
# ``tkwargs``, :97 ``torch.from_numpy(param).to(**tkwargs)``), whatever the model's dtype: an fp64 model's L-BFGS trajectory is
# evaluated at fp32-rounded points.  Off by default (this build keeps the model's dtype);
# ``with settings.reference_fp32_theta(True):`` reproduces the reference's round trip in ``MLLObjective`` — objective, gradient
# and the final ``load_state_dict`` then see float32(theta) — so that a trajectory can be compared with the reference's.
reference_fp32_theta = _Value(False)


# Sharded single evaluation (gp-plus_amd/sharded.py): ``with settings.sharded_evaluation({"group": None, "nb": 1024}):``
# makes every exact-GP log-likelihood inside the block a cooperative evaluation by all ranks of the process group
# (None = the default group).  Every rank must run the same model code with the same parameters.
sharded_evaluation = _Value(None)


# Differentiable predictions (GP_Plus.predict_with_grad, reference models/gp_plus.py:626-628): inside
# ``with settings.differentiable_predictions(True):``, with grad mode on and some input or parameter requiring grad, the eval-mode call
# of a model builds its test features, test mean and (for a latent map) training features under autograd, and the mean and the
# variance diagonal of the returned MultivariateNormal are autograd-connected (linalg.predict_mean / predict_var, backward by
# gpp_cross_grad).  Off by default: predictions then carry no graph, as they always have (callers call ``.numpy()`` on them).
differentiable_predictions = _Value(False)


@contextmanager
def fast_computations(covar_root_decomposition=True, log_prob=True, solves=True):
    yield


@contextmanager
def max_cholesky_size(_n):
    yield

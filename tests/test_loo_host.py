"""Leave-one-out pseudo-likelihood, the parts that need no GPU: the two dense fp64 references against each other (the closed form
W = -(alpha beta^T + beta alpha^T) / 2 - P diag(b) P that the HIP path implements, against autograd through the inverse), and the
host-side interface (the objective class, the ``objective`` switch of the fit drivers)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loo_reference import KIND_MATERN52, KIND_RBF, loo_autograd, loo_closed_form, make_inputs  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("D,kind,d_split,S", [(3, KIND_RBF, 0, 1), (8, KIND_MATERN52, 3, 3), (8, KIND_RBF, 0, 3)])
def test_closed_form_matches_autograd(D, kind, d_split, S):
    """N = 120: value and EVERY gradient (w, sf2, tau, mean, y and the features U) of the closed form against autograd, to 1e-10
    relative (of the largest entry, per gradient vector)."""
    inp = make_inputs(120, D, seed=11, S=S)
    v0, g0 = loo_autograd(**inp, kind=kind, d_split=d_split)
    v1, g1 = loo_closed_form(**inp, kind=kind, d_split=d_split)
    assert abs(v1 - v0) <= 1e-10 * abs(v0), (float(v0), float(v1))
    assert set(g0) == {"U", "w", "sf2", "tau", "mean", "y"}
    for name, ref in g0.items():
        got = g1[name].reshape(ref.shape)
        err = (got - ref).abs().max().item()
        assert err <= 1e-10 * ref.abs().max().item(), (name, err, ref.abs().max().item())


def _small_model():
    from gpplus_amd.models import GP_Plus

    fx = dict(np.load(os.path.join(GOLD, "c1_borehole_n500.npz")))
    return GP_Plus(torch.tensor(fx["Xtrain"][:40]), torch.tensor(fx["ytrain"][:40]), dtype=torch.float64, device="cpu")


def test_objective_class_is_exported_and_rejects_non_gaussian_input():
    from gpplus_amd import gpcore
    from gpplus_amd.gpcore import ExactMarginalLogLikelihood, LeaveOneOutPseudoLikelihood
    from gpplus_amd.gpcore.mlls import LeaveOneOutPseudoLikelihood as from_mlls

    assert LeaveOneOutPseudoLikelihood is from_mlls and hasattr(gpcore, "LeaveOneOutPseudoLikelihood")
    m = _small_model()
    loo = LeaveOneOutPseudoLikelihood(m.likelihood, m)
    assert isinstance(loo, ExactMarginalLogLikelihood)  # the same priors, the same 1 / N
    with pytest.raises(RuntimeError, match="Gaussian"):
        loo(torch.zeros(40, dtype=torch.float64), m.train_targets)


def test_objective_has_no_cpu_fallback():
    from gpplus_amd._lib import GppError
    from gpplus_amd.gpcore import LeaveOneOutPseudoLikelihood

    m = _small_model()
    m.train()
    with pytest.raises(GppError, match="no CPU fallback"):
        LeaveOneOutPseudoLikelihood(m.likelihood, m)(m(*m.train_inputs), m.train_targets)


def test_unknown_objective_raises_value_error():
    from gpplus_amd.optim import MLLObjective, fit_model_scipy, fit_model_torch

    m = _small_model()
    with pytest.raises(ValueError, match="objective"):
        fit_model_torch(m, num_iter=1, verbose=False, objective="loocv")
    with pytest.raises(ValueError, match="objective"):
        fit_model_scipy(m, num_restarts=0, objective="nll")
    with pytest.raises(ValueError, match="objective"):
        MLLObjective(m, True, [0, 0], objective="")
    with pytest.raises(ValueError, match="objective"):
        m.fit(objective="LOO")


def test_library_binds_the_leave_one_out_entry_points():
    from gpplus_amd import _lib

    lib = _lib.load()
    for name in ("gpp_loo_scalars", "gpp_sym_rowscale", "gpp_loo_grad_reduce"):
        assert name in _lib._SIGNATURES and hasattr(lib, name)


def test_sharded_evaluation_is_refused():
    from gpplus_amd import settings
    from gpplus_amd.linalg import KernelSpec, exact_loo

    inp = make_inputs(16, 3, seed=1, S=1)
    spec = KernelSpec(inp["w"], inp["sf2"], KIND_RBF, 0)
    with settings.sharded_evaluation({"nb": 1024}):
        with pytest.raises(NotImplementedError, match="sharded"):
            exact_loo(inp["U"], spec, inp["tau"], inp["mean"], inp["y"])

"""Deterministic calibration without a GPU: the dense reference (tests/calibration_reference.py) checks itself against central
differences, and the model's host side — constructor validation, parameter and prior names, bounds, the exported symbol, and the
refusals of what a calibrated model cannot do rightly."""
import os
import re

import numpy as np
import pytest
import torch

import calibration_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: central-difference step and bar of the reference's own gradient check.  With h = 1e-4 the truncation error is h^2 f''' / 6 ~ 1e-9
#: of these gradients and the rounding error eps |f| / h ~ 1e-12 / 6e-3 ~ 2e-10; measured on this fixture: 2.4e-10 ... 6.4e-10 of
#: the gradient at h = 1e-4 (2.6e-8 ... 4.7e-8 at 1e-3, 0.8e-9 ... 1.5e-9 at 1e-5).  The bar leaves two orders of magnitude.
FD_STEP, FD_BAR = 1e-4, 1e-7


def _oracle(ids):
    fx = cr.load_fixture()
    co = cr.CalibratedOracle(fx["Xtrain"], fx["ytrain"], ids, **cr.C4_KW)
    for k in list(co.params):
        if f"theta1::param::{k}" in fx:
            co.params[k] = torch.as_tensor(fx[f"theta1::param::{k}"], dtype=torch.float64).reshape(co.params[k].shape)
    for i, n in enumerate(ids):  # away from the prior mean and from any optimum
        co.params[f"Theta_{n}.constant"] = torch.tensor([0.7 - 1.1 * i], dtype=torch.float64)
    return co


def _model(ids=(2, 7), **kw):
    from gpplus_amd.models import GP_Plus

    fx = cr.load_fixture()
    args = dict(cr.C4_KW)
    args.update(kw)
    return GP_Plus(torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"]), dtype=torch.float64, device="cpu",
                   calibration_id=list(ids), **args)


@pytest.mark.parametrize("ids", [[2], [2, 7]])
def test_reference_theta_gradient_matches_central_differences(ids):
    co = _oracle(ids)
    _, grads = co.loss_and_grad()
    scale = max(abs(grads[f"Theta_{n}.constant"].item()) for n in ids)
    assert scale > 1e-4  # (theta is away from an optimum: the check is not of a zero)
    for n in ids:
        name = f"Theta_{n}.constant"
        fd = cr.central_differences(co, name, 0, FD_STEP)
        err = abs(fd - grads[name].item())
        print(f"ids={ids} {name}: autograd {grads[name].item():.12e} central {fd:.12e} rel {err / scale:.2e}")
        assert err <= FD_BAR * scale, (name, fd, grads[name].item())


def test_reference_pairs_of_one_source_contribute_nothing():
    co = _oracle([2, 7])
    src = co.o.train_x[:, -1]
    for rows in (torch.where(src == 0)[0], torch.where(src != 0)[0], torch.tensor([0])):
        assert torch.equal(cr.kernel_operands(co, rows)["g_theta"], torch.zeros(2, dtype=torch.float64))


def test_constructor_validation():
    with pytest.raises(ValueError, match="quantitative"):
        _model(ids=(10,))
    with pytest.raises(ValueError, match="quantitative"):
        _model(ids=(11,))
    with pytest.raises(ValueError, match="twice"):
        _model(ids=(2, 2))
    with pytest.raises(ValueError, match="one entry per"):
        _model(ids=(2, 7), mean_prior_cal=[0.0])
    with pytest.raises(NotImplementedError, match="probabilistic"):
        _model(ids=(2,), calibration_type="probabilistic")
    with pytest.raises(ValueError, match="source"):
        _model(ids=(2,), qual_dict={})


def test_parameters_priors_and_training_entries():
    from gpplus_amd.gpcore import NormalPrior

    fx = cr.load_fixture()
    X = torch.tensor(fx["Xtrain"]).clone()
    X[X[:, -1] == 0, 2] = float("nan")  # the expected way to say "unknown"
    from gpplus_amd.models import GP_Plus

    m = GP_Plus(X, torch.tensor(fx["ytrain"]), dtype=torch.float64, device="cpu", calibration_id=[2, 7],
                mean_prior_cal=[0.5, -0.5], std_prior_cal=[2.0, 3.0], **cr.C4_KW)
    sd = m.state_dict()
    assert "Theta_2.constant" in sd and "Theta_7.constant" in sd and sd["Theta_2.constant"].shape == (1,)
    priors = {name: prior for name, _, prior, _, _ in m.named_priors()}
    for n, mu, sdv in ((2, 0.5, 2.0), (7, -0.5, 3.0)):
        prior = priors[f"Theta_{n}.mean_prior"]
        assert isinstance(prior, NormalPrior) and float(prior.loc) == mu and float(prior.scale) == sdv
    tr = m.train_inputs[0]
    hf = tr[:, -1] == 0
    assert not torch.isnan(tr).any()
    assert torch.equal(tr[hf][:, [2, 7]], torch.zeros(int(hf.sum()), 2, dtype=torch.float64))
    assert torch.equal(tr[~hf][:, [2, 7]], torch.tensor(fx["Xtrain"])[~hf][:, [2, 7]])
    # the priors take part in restarts: a reset moves theta
    torch.manual_seed(0)
    m.reset_parameters()
    assert float(m.state_dict()["Theta_2.constant"]) != 0.0 and float(m.state_dict()["Theta_7.constant"]) != 0.0
    # calibration_result: the values, and the reference's conversion to the units of the data (gp_plus.py:956)
    sd = m.state_dict()
    sd["Theta_2.constant"], sd["Theta_7.constant"] = torch.tensor([0.25]), torch.tensor([-1.5])
    m.load_state_dict(sd)
    assert m.calibration_result() == {2: 0.25, 7: -1.5}
    mean_train, std_train = np.arange(11.0), 2.0 * np.ones(11)
    assert m.calibration_result(mean_train, std_train) == {2: 0.25 * 2.0 + 2.0, 7: -1.5 * 2.0 + 7.0}
    with pytest.raises(ValueError):
        m.calibration_result(mean_train)


def test_features_carry_theta_for_any_input():
    m = _model(ids=(2, 7))
    sd = m.state_dict()
    sd["Theta_2.constant"], sd["Theta_7.constant"] = torch.tensor([0.25]), torch.tensor([-1.5])
    m.load_state_dict(sd)
    fx = cr.load_fixture()
    xt = torch.tensor(fx["Xtest"])
    hf = xt[:, -1] == 0
    assert hf.any() and (~hf).any()
    for mode in (m.train, m.eval):
        mode()
        U, dz = m._features(xt)
        assert dz == 2 and U.shape == (xt.shape[0], 12)
        assert torch.equal(U[hf][:, [4, 9]], torch.tensor([0.25, -1.5], dtype=torch.float64).expand(int(hf.sum()), 2))
        assert torch.equal(U[~hf][:, 2:], xt[~hf][:, :10])
    m.train()
    cov = m(*m.train_inputs).lazy_covariance_matrix
    assert cov.calib is not None and cov.calib.cols.tolist() == [4, 9] and cov.calib.theta.requires_grad
    assert torch.equal(cov.calib.member.bool(), m.train_inputs[0][:, -1] == 0)
    assert m.likelihood(m(*m.train_inputs)).lazy_covariance_matrix.calib is not None  # (kept when the noise is added)
    assert _model(ids=()).train()(*_model(ids=()).train_inputs).lazy_covariance_matrix.calib is None


def test_bounds_for_theta():
    from gpplus_amd.optim.mll_scipy import MLLObjective, get_bounds

    m = _model(ids=(2, 7))
    obj = MLLObjective(m, True, [0, 0])
    lo, hi = get_bounds(obj, obj.pack_parameters())
    names = [n for n, p in m.named_parameters() if p.requires_grad for _ in range(p.numel())]
    picked = [(a, b) for n, a, b in zip(names, lo, hi) if n.startswith("Theta_")]
    assert picked == [(-15.0, 15.0), (-15.0, 15.0)]


def test_symbol_is_declared_exported_and_bound():
    from gpplus_amd import _lib, backend, linalg

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_calib_grad_reduce\s*\(", header)
    assert "gpp_calib_grad_reduce" in _lib.exported_symbols() and len(_lib._SIGNATURES["gpp_calib_grad_reduce"][1]) == 15
    lib = _lib.load()
    assert lib.gpp_calib_grad_reduce.argtypes == _lib._SIGNATURES["gpp_calib_grad_reduce"][1]
    assert callable(backend.GppContext.calib_grad_reduce) and callable(linalg.CalibratedMLLFunction.apply)
    # a NULL handle is argument 1, before anything else is looked at
    assert lib.gpp_calib_grad_reduce(None, None, 0, 0, None, None, 0, 0, None, None, 0, None, None, 0, None) == -1


def test_refusals():
    from gpplus_amd import settings
    from gpplus_amd.optim import fit_model_torch_batched

    m = _model(ids=(2,))
    x = m.train_inputs[0][:3]
    for call in (lambda: m.predict_gradient(x), lambda: m.active_subspace(x),
                 lambda: m.condition_on_gradients(x, torch.zeros(3, 10, dtype=torch.float64)),
                 lambda: m.fit(objective="loo"), lambda: m.fit(objective="cv", folds=3),
                 lambda: m.fit(optim_type="adam_torch_batched"), lambda: fit_model_torch_batched(m, num_restarts=1)):
        with pytest.raises(NotImplementedError, match="calibration"):
            call()
    assert m._restarts_fit_one_batch(5) is False
    m.train()
    noisy = m.likelihood(m(*m.train_inputs))
    with pytest.raises(NotImplementedError, match="calibration"):
        noisy.loo_log_prob(m.train_targets)
    with pytest.raises(NotImplementedError, match="calibration"):
        noisy.cv_log_prob(m.train_targets, 3)
    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError, match="sharded_evaluation"):
            noisy.log_prob(m.train_targets)


def test_reference_recovers_theta_on_the_analytic_problem():
    """What tests/test_gpu_calibration.py asks of ``fit_model_scipy`` holds for the reference alone: its own L-BFGS-B run from the
    same start (every raw parameter at its initial value, theta at its prior mean 0) lowers the objective and ends nearer
    THETA_STAR than it began.  Sizes and seed are the GPU test's."""
    from gpplus_amd.test_functions.calibration import THETA_STAR, calibration_problem

    X, y = calibration_problem(16, 64, seed=0)
    assert np.isnan(X[:16, 1]).all() and not np.isnan(X[16:]).any()
    co = cr.CalibratedOracle(X, y, [1], qual_dict={2: 2}, m_gp="multiple_constant")
    assert float(co.params["Theta_1.constant"]) == 0.0
    start, res = co.fit_lbfgs()
    theta_hat = float(co.params["Theta_1.constant"])
    print(f"reference: objective {start:.6f} -> {res.fun:.6f} in {res.nit} iterations; theta {theta_hat:.6f}")
    assert res.fun < start
    assert abs(theta_hat - THETA_STAR) < abs(0.0 - THETA_STAR)

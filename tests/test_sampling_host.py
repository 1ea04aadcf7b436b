"""Posterior sampling on the host side (no GPU): the public surface of GP_Plus.sample_y (gp_plus.py:985-998) and of
MultivariateNormal.sample / rsample, the C ABI entry point behind them, and the laziness that lets a draw at the training
inputs skip the O(M N^2) predictive variance."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_sample_y_signature_matches_reference():
    from gpplus_amd.models import GP_Plus

    sig = inspect.signature(GP_Plus.sample_y)
    assert list(sig.parameters) == ["self", "size", "X", "plot"]
    assert [sig.parameters[k].default for k in ("size", "X", "plot")] == [1, None, False]


def test_multivariate_normal_has_sample_and_rsample():
    from gpplus_amd.gpcore import MultivariateNormal

    for name in ("sample", "rsample"):
        sig = inspect.signature(getattr(MultivariateNormal, name))
        assert list(sig.parameters)[:3] == ["self", "sample_shape", "base_samples"], name
        assert sig.parameters["sample_shape"].default == torch.Size()
        assert sig.parameters["base_samples"].default is None


def test_post_cov_train_is_declared_exported_and_bound():
    from gpplus_amd import _lib, linalg
    from gpplus_amd.backend import GppContext

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_post_cov_train\s*\(", header)
    assert "gpp_post_cov_train" in _lib.exported_symbols()
    assert getattr(_lib.load(), "gpp_post_cov_train") is not None
    assert callable(GppContext.post_cov_train)
    for name in ("predictive_cov_upper", "train_post_cov_upper", "mvn_root", "mvn_draw"):
        assert name in linalg.__all__ and callable(getattr(linalg, name)), name


def test_sample_y_plot_raises_before_any_work():
    from gpplus_amd.models import GP_Plus

    fx = dict(np.load(os.path.join(GOLD, "c1_borehole_n500.npz")))
    m = GP_Plus(torch.tensor(fx["Xtrain"][:50]), torch.tensor(fx["ytrain"][:50]), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="plotting"):
        m.sample_y(size=3, plot=True)


def test_likelihood_keeps_the_predictive_variance_lazy():
    """likelihood(pred) must not evaluate the variance: a draw at the training inputs never needs V = K_*N L^-T."""
    from gpplus_amd.gpcore.distributions import DenseCovariance
    from gpplus_amd.gpcore.kernels import DiagNoise

    calls = []

    def diag():
        calls.append(1)
        return torch.full((4,), 2.0, dtype=torch.float64)

    seen = []
    cov = DenseCovariance(diag, None, n=4, upper_builder=lambda A, added, jit: seen.append(added))
    noisy = cov + DiagNoise(torch.tensor([0.5], dtype=torch.float64), None, 4)
    assert calls == [] and noisy.shape == torch.Size([4, 4])
    assert noisy._upper is cov._upper
    torch.testing.assert_close(noisy.diag(), torch.full((4,), 2.5, dtype=torch.float64))
    assert calls == [1]
    noisy._upper(None, noisy._added, 0.0)
    torch.testing.assert_close(seen[0], torch.full((4,), 0.5, dtype=torch.float64))


def test_post_cov_train_identity_in_float64():
    """The identity the kernel rests on: K - K Ky^-1 K = T - T Ky^-1 T for Ky = K + T, and the numpy statement of the kernel."""
    rng = np.random.default_rng(3)
    n = 60
    X = rng.standard_normal((n, 3))
    K = 0.8 * np.exp(-0.5 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    tau = np.array([1e-3, 4e-3, 2e-2])
    grp = rng.integers(0, 3, n)
    t = tau[grp]
    Ky = K + np.diag(t)
    Kinv = np.linalg.inv(Ky)
    general = K - K @ Kinv @ K
    kernel_form = -t[:, None] * Kinv.T * t[None, :] + np.diag(t)
    assert np.abs(general - kernel_form).max() < 1e-10
    # with the likelihood's own noise on top: 2T - T Ky^-1 T, eigenvalues in [min tau, 2 max tau)
    ev = np.linalg.eigvalsh(kernel_form + np.diag(t))
    assert ev.min() >= tau.min() * (1 - 1e-9) and ev.max() < 2 * tau.max()

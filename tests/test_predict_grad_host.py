"""Host-side contract of differentiable predictions (GP_Plus.predict_with_grad, settings.differentiable_predictions):
no GPU needed."""
import pytest
import torch


def test_differentiable_predictions_default_off():
    from gpplus_amd import settings

    assert settings.differentiable_predictions.value() is False
    with settings.differentiable_predictions(True):
        assert settings.differentiable_predictions.value() is True
    assert settings.differentiable_predictions.value() is False


def test_predict_with_grad_on_cpu_model_has_no_fallback():
    """Like every other compute path, a CPU model reaches the library's no-CPU-fallback error (not NotImplementedError)."""
    from gpplus_amd._lib import GppError
    from gpplus_amd import settings
    from gpplus_amd.models import GP_Plus

    g = torch.Generator().manual_seed(0)
    X = torch.rand(24, 3, generator=g, dtype=torch.float64)
    y = X.sum(1)
    m = GP_Plus(X, y, dtype=torch.float64, device="cpu")
    Xt = torch.rand(5, 3, generator=g, dtype=torch.float64, requires_grad=True)
    with pytest.raises(GppError):
        m.predict_with_grad(Xt)
    assert settings.differentiable_predictions.value() is False  # the switch is restored on the way out

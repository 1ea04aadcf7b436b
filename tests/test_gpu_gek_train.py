"""Training on gradient observations on the GPU: ``GradientEnhancedMarginalLogLikelihood`` against the fp64 autograd reference of
tests/gek_train_reference.py on the five fixture cases of tests/gek_reference.py at their oracle parameters (value at a relative
1e-5, the suite's loss bar; every named parameter's gradient at 1e-6 of the largest reference magnitude in its tensor; with an
explicit noise and with the default nugget, whose derivative the latter exercises), bitwise repeatability, the value against the
log-density recomputed from the bordered factor of ``condition_on_gradients``, a fit through ``fit_model_scipy`` and the refusals.
The reference's floor is printed by tests/test_gek_train_host.py."""
import math
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_reference as G  # noqa: E402
import gek_train_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

VALUE_BAR, GRAD_BAR = 1e-5, 1e-6
_cache = {}


def _model_from_oracle(o, X, y, **kw):
    from gpplus_amd.models import GP_Plus

    m = GP_Plus(torch.tensor(X), torch.tensor(y), dtype=torch.float64, device="cuda", **kw)
    sd = m.state_dict()
    for k, v in o.params.items():
        sd[k] = v.reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    return m


def _case(name):
    """(model, oracle, xg, dY, noise, {noise_given: reference loss and gradients}): built once per case and left unchanged."""
    if name not in _cache:
        from gpplus_amd.gradient_enhanced import GRADIENT_NUGGET_REL

        o, X, y, kw, xg, dY, noise, _ = G.gek_case(name)
        refs = {True: T.gek_loss_and_grad(o, xg, dY, noise), False: T.gek_loss_and_grad(o, xg, dY, None, GRADIENT_NUGGET_REL)}
        _cache[name] = (_model_from_oracle(o, X, y, **kw), o, xg, dY, noise, refs)
    return _cache[name]


def _evaluate(m, xg, dY, noise):
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood

    m.train()
    m.zero_grad()
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, noise)
    loss = -mll(m(*m.train_inputs), m.train_targets)
    loss.backward()
    return loss.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}


def _compare(what, loss, grads, ref_loss, ref_grads, trainable):
    rel = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    print(f"{what}: loss {loss.item():.12e} against {ref_loss.item():.12e}: rel {rel:.2e}")
    assert rel <= VALUE_BAR
    assert set(grads) == set(trainable), (sorted(grads), sorted(trainable))
    for n in trainable:
        ref = ref_grads[n].reshape(grads[n].shape)
        scale = ref.abs().max().item()
        err = (grads[n] - ref).abs().max().item()
        print(f"{what} {n}: max error {err:.3e} = {err / scale:.3e} of max|reference| {scale:.3e}")
        assert err <= GRAD_BAR * scale, (n, err, scale)


@pytest.mark.parametrize("noise_given", [True, False])
@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_against_the_reference(gpu_ctx, name, noise_given):
    m, o, xg, dY, noise, refs = _case(name)
    nz = noise if noise_given else None
    loss, grads = _evaluate(m, xg, dY, nz)
    _compare(f"{name} noise_given={noise_given}", loss, grads, *refs[noise_given], o.trainable)
    # two evaluations are bitwise equal
    loss2, grads2 = _evaluate(m, xg, dY, nz)
    assert torch.equal(loss.view(torch.int64), loss2.view(torch.int64))
    for n in grads:
        assert torch.equal(grads[n].view(torch.int64), grads2[n].view(torch.int64)), n


def test_an_odd_number_of_function_rows(gpu_ctx):
    """Every fixture case has an even N.  With an odd N the two derivative windows of the joint matrix start at an odd column, where
    the block builders' 16-byte stores are not aligned: the blocks are then built aside and copied.  c3 cut to 77 rows, both noises."""
    import gradpost_reference as gr
    from gpplus_amd.gradient_enhanced import GRADIENT_NUGGET_REL

    fixture, _, kw, Mg = G.GEK_CASES["c3"]
    fx = gr.load_fixture(fixture)
    o = gr.load_oracle(fx, 77, **kw)
    X, y = gr.fixture_xy(fx, 77)
    xg = gr.fixture_test_rows(fx, Mg + 1).clone()
    p = len(o.quant_index)
    dY = 0.1 * float(o.y_std) * torch.sin(torch.arange((Mg + 1) * p, dtype=torch.float64)).reshape(Mg + 1, p)
    noise = G.prior_curvature_noise(o, 1e-4)
    m = _model_from_oracle(o, X, y, **kw)
    for nz, rel in ((noise, None), (None, GRADIENT_NUGGET_REL)):
        loss, grads = _evaluate(m, xg, dY, nz)
        _compare(f"c3 cut to 77 rows, noise_given={nz is not None}", loss, grads, *T.gek_loss_and_grad(o, xg, dY, nz, rel), o.trainable)


def test_the_cases_cover_feature_gradients_noise_groups_and_both_matern_kinds():
    assert G.GEK_CASES["c3"][2].get("qual_dict") and G.GEK_CASES["c4"][2].get("multiple_noise")
    assert {G.GEK_CASES[n][2].get("quant_correlation_class") for n in ("c1-matern52", "c1-matern32")} == {"Matern52Kernel", "Matern32Kernel"}


@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_value_equals_the_log_density_of_the_bordered_factor(gpu_ctx, name):
    """Both routes factor the same matrix: the from-scratch value against -(z'z + 2 sum log diag + n log 2 pi) / 2 from the
    ``GradientFactorCache`` of ``condition_on_gradients`` at the same parameters, to 1e-9 relative, with the jitter of both at 0."""
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood

    m, o, xg, dY, noise, _ = _case(name)
    gc = m.condition_on_gradients(xg, dY, noise=noise)._cache
    assert gc.jitter == 0.0
    n = gc.z.numel()
    bordered = (-0.5 * ((gc.z * gc.z).sum() + 2 * torch.log(gc.L.diagonal()).sum() + n * math.log(2 * math.pi))).item()
    m.train()
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, noise)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")  # (jitter would be announced by a warning)
        value = mll.joint_log_prob(m.likelihood(m(*m.train_inputs)), m.train_targets).item()
    rel = abs(value - bordered) / abs(bordered)
    print(f"{name}: from scratch {value:.12e}, bordered {bordered:.12e}: rel {rel:.2e}")
    assert rel <= 1e-9


def test_a_fit_raises_the_objective_and_ends_where_the_reference_agrees(gpu_ctx):
    from gpplus_amd.optim import fit_model_scipy
    from gpplus_amd.optim.mll_scipy import MLLObjective

    o, X, y, xg, dY, noise = T.fit_case()
    m = _model_from_oracle(o, X, y)
    m.train()
    probe = MLLObjective(m, True, [0, 0], "gek", None, (xg, dY, noise))
    start = probe.fun(probe.pack_parameters(), False)
    ref_start = T.gek_loss(o, xg, dY, noise, normalize=False).item()
    assert abs(start - ref_start) <= VALUE_BAR * abs(ref_start)
    out, best = fit_model_scipy(m, num_restarts=-1, objective="gek", gradients=(xg, dY, noise))
    print(f"fit: objective {start:.6f} -> {best:.6f} in {out[0].nit} iterations")
    assert best < start - 1e-3 * abs(start)
    # the reference at the final parameters
    sd = m.state_dict()
    for k in o.params:
        o.params[k] = sd[k].detach().cpu().to(torch.float64).reshape(o.params[k].shape)
    ref_loss, ref_grads = T.gek_loss_and_grad(o, xg, dY, noise, normalize=False)
    value, _ = probe.fun(probe.pack_parameters(), True)
    assert value == best or abs(value - best) <= 1e-12 * abs(best)
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    _compare("fit end", torch.tensor(value, dtype=torch.float64), grads, ref_loss, ref_grads, o.trainable)


def test_refusals(gpu_ctx, monkeypatch):
    import calibration_reference as cr
    from gpplus_amd import settings
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim import fit_model_scipy, fit_model_torch

    m, o, xg, dY, noise, _ = _case("c3")
    m.train()
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, noise)
    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError, match="sharded_evaluation"):
            mll(m(*m.train_inputs), m.train_targets)
    with monkeypatch.context() as mp:  # (a capture is not started for this: the check is the host-side query)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(NotImplementedError, match="capture"):
            mll(m(*m.train_inputs), m.train_targets)
    with pytest.raises(ValueError, match="gek"):
        fit_model_torch(m, objective="mll", gradients=(xg, dY))
    with pytest.raises(ValueError, match="gradients"):
        fit_model_scipy(m, objective="gek")
    with pytest.raises(ValueError, match="gradients"):
        m.fit(objective="gek")
    nan = dY.clone()
    nan[0, 0] = float("nan")
    for args in ((xg[:, :-1], dY), (xg, dY[:, :-1]), (xg, dY[:1]), (xg[:0], dY[:0]), (xg, nan), (xg, dY, -1.0),
                 (xg, dY, torch.ones(3, 7, dtype=torch.float64))):
        with pytest.raises(ValueError):
            fit_model_scipy(m, objective="gek", gradients=args)
    # a calibrated model
    fx = cr.load_fixture()
    cm = GP_Plus(torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"]), dtype=torch.float64, device="cuda", calibration_id=[2],
                 **cr.C4_KW)
    xc = torch.tensor(fx["Xtest"])[:2]
    gc = torch.ones(2, int(cm.quant_index.numel()), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="calibration"):
        cm.fit(objective="gek", gradients=(xc, gc))
    with pytest.raises(NotImplementedError, match="calibration"):
        GradientEnhancedMarginalLogLikelihood(cm.likelihood, cm, xc, gc)

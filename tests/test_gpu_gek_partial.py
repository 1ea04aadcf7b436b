"""Partial gradients on the GPU: ``GP_Plus.condition_on_gradients(..., observed=mask)`` and the ``"gek"`` objective with
``gradients=(Xg, dY, noise, observed)`` against the dense fp64 references of tests/gek_partial_reference.py (the joint Gaussian with
the unobserved rows and columns dropped), on the cases of tests/gek_reference.py with the mask pattern
((3 a + 5 j) mod 7) < 3 — 2 to 4 components per point and an odd q — and with one row of alternating directions.

The bars are those of tests/test_gpu_gek.py (1e-6 of the largest reference magnitude) and tests/test_gpu_gek_train.py (value 1e-5
relative, gradients 1e-6 of the largest reference magnitude per tensor, the bordered factor 1e-9)."""
import math
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_partial_reference as P  # noqa: E402
import gek_reference as G  # noqa: E402
import gek_train_reference as T  # noqa: E402
import gradpost_reference as gr  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-6
VALUE_BAR, GRAD_BAR = 1e-5, 1e-6
MASKS = ("pattern", "alternating row")
_cache, _refs, _train = {}, {}, {}


def _model_from_oracle(o, X, y, **kw):
    from gpplus_amd.models import GP_Plus

    m = GP_Plus(torch.tensor(X), torch.tensor(y), dtype=torch.float64, device="cuda", **kw)
    sd = m.state_dict()
    for k, v in o.params.items():
        sd[k] = v.reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    return m


def _case(name):
    """(model, oracle, xg, dY, noise, xt): built once per case and left unchanged."""
    if name not in _cache:
        o, X, y, kw, xg, dY, noise, xt = G.gek_case(name)
        _cache[name] = (_model_from_oracle(o, X, y, **kw), o, xg, dY, noise, xt)
    return _cache[name]


def _mask(which, Mg, p):
    return P.pattern_mask(Mg, p) if which == "pattern" else P.alternating_row(p)


def _reference(name, which):
    if (name, which) not in _refs:
        m, o, xg, dY, noise, xt = _case(name)
        _refs[name, which] = P.gek_posterior_partial(o, xg, dY, noise, xt, _mask(which, *dY.shape))
    return _refs[name, which]


def _close(got, ref, what, bar=BAR):
    scale = ref.abs().max().item()
    err = (got.detach().cpu() - ref).abs().max().item()
    print(f"{what}: max error {err:.3e} = {err / scale:.3e} of max|reference| {scale:.3e}")
    assert err <= bar * scale, (what, err, scale)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _compare_posterior(post, xt, ref, what):
    mean, std = post.predict(xt)
    _, std_latent = post.predict(xt, include_noise=False)
    gmean, gstd = post.predict_gradient(xt)
    _close(mean, ref["mean"], f"{what} mean")
    _close(std, ref["std"], f"{what} std")
    _close(std_latent, ref["var"].clamp_min(0).sqrt(), f"{what} std without noise", bar=BAR * ref["std"].abs().max().item()
           / ref["var"].clamp_min(0).sqrt().abs().max().item())
    _close(gmean, ref["gmean"], f"{what} gradient mean")
    _close(gstd, ref["gvar"].clamp_min(0).sqrt(), f"{what} gradient std")
    return mean, std, gmean, gstd


def _poison(t, mask, value=float("nan")):
    full = torch.broadcast_to(mask, t.shape)
    return torch.where(full, t, torch.full_like(t, value))


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_against_the_partial_reference(gpu_ctx, name, which):
    m, o, xg, dY, noise, xt = _case(name)
    Mg, p = dY.shape
    N = m.train_inputs[0].shape[0]
    mask = _mask(which, Mg, p)
    q = int(torch.broadcast_to(mask, (Mg, p)).sum())
    ref = _reference(name, which)
    post = m.condition_on_gradients(xg, dY, noise=noise, observed=mask)
    assert post.num_function_rows == N and post.num_gradient_points == Mg and post.num_gradient_observations == q
    assert post._cache.Linv.shape == (N + q,) * 2 and post._cache.z.shape == (N + q,)
    assert post.observed.dtype == torch.bool and torch.equal(post.observed.cpu(), torch.broadcast_to(mask, (Mg, p)))
    post.observed[:] = False  # a copy: the posterior's own mask is out of reach
    assert bool(post.observed.any())
    mean, _, gmean, _ = _compare_posterior(post, xt, ref, f"{name} [{which}]")
    assert gmean.shape == (G.M_TEST, p)  # all p directions at the test points
    dense = m.condition_on_gradients(xg, dY, noise=noise).predict(xt, return_std=False)
    assert not torch.allclose(mean, dense, rtol=1e-6, atol=0)  # fewer observations than the dense call: another posterior


@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_properties(gpu_ctx, name):
    m, o, xg, dY, noise, xt = _case(name)
    Mg, p = dY.shape
    base = m.predict(xt)
    cache = m.prediction_strategy
    held = (_bits(cache.L).clone(), _bits(cache.Linv).clone(), cache.alpha.clone(), cache.z.clone())
    params = {k: v.clone() for k, v in m.state_dict().items()}

    def outputs(post):
        return (*post.predict(xt), *post.predict_gradient(xt))

    # the all-True mask gives the bits of observed=None, with the noise given and with the default nugget
    for nz in (noise, None):
        plain = m.condition_on_gradients(xg, dY, noise=nz)
        assert plain.num_gradient_observations == Mg * p and bool(plain.observed.all())
        for mask in (torch.ones(Mg, p, dtype=torch.bool), torch.ones(p, dtype=torch.bool)):
            full = m.condition_on_gradients(xg, dY, noise=nz, observed=mask)
            # (the factor through its diagonal, z and alpha: one triangle of its buffer is scratch of the bordering)
            assert torch.equal(_bits(full._cache.L.diagonal()), _bits(plain._cache.L.diagonal()))
            assert torch.equal(_bits(full._cache.z), _bits(plain._cache.z)) and torch.equal(_bits(full._cache.alpha), _bits(plain._cache.alpha))
            for a, b in zip(outputs(plain), outputs(full)):
                assert torch.equal(_bits(a), _bits(b))
    # NaN / inf in the unobserved entries of dY and of the noise give the bits of finite values there; two calls agree
    mask = P.pattern_mask(Mg, p)
    nz = noise.expand(Mg, p)
    clean = outputs(m.condition_on_gradients(xg, dY, noise=nz, observed=mask))
    dirty = outputs(m.condition_on_gradients(xg, _poison(dY, mask), noise=_poison(nz, mask, float("inf")), observed=mask))
    again = outputs(m.condition_on_gradients(xg, dY, noise=nz, observed=mask))
    for a, b, c in zip(clean, dirty, again):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))
    # the receiver: the same cache object with the same bits, the same parameters, the same predictions
    assert m.prediction_strategy is cache
    assert torch.equal(_bits(cache.L), held[0]) and torch.equal(_bits(cache.Linv), held[1])
    assert torch.equal(cache.alpha, held[2]) and torch.equal(cache.z, held[3])
    assert all(torch.equal(v, params[k]) for k, v in m.state_dict().items())
    after = m.predict(xt)
    assert torch.equal(_bits(base[0]), _bits(after[0])) and torch.equal(_bits(base[1]), _bits(after[1]))


def test_the_limit_counts_the_observed_entries(gpu_ctx):
    """c1 (N = 500, p = 8) with 100 gradient points: Mg p = 800 > min(N, 2048), but 3 of 8 directions are q = 300."""
    m, o, _, _, noise, xt = _case("c1")
    fx = gr.load_fixture(G.GEK_CASES["c1"][0])
    xg = gr.fixture_test_rows(fx, 100).clone()
    assert xg.shape == (100, 8) and m.train_inputs[0].shape[0] == 500
    g0, _ = gr.gradient_posterior(o, xg)
    dY = 1.25 * g0 + 0.05 * g0.abs().max() * torch.sin(torch.arange(g0.numel(), dtype=torch.float64)).reshape(g0.shape)
    mask = torch.tensor([True, False, False, True, False, False, True, False])
    with pytest.raises(ValueError, match="800 gradient observations exceed"):
        m.condition_on_gradients(xg, dY, noise=noise)
    post = m.condition_on_gradients(xg, _poison(dY, mask), noise=noise, observed=mask)
    assert post.num_gradient_observations == 300 and post._cache.Linv.shape == (800, 800)
    _compare_posterior(post, xt, P.gek_posterior_partial(o, xg, dY, noise, xt, mask), "c1 with 300 of 800 components")


def test_the_failing_observation_is_named_through_the_selection(gpu_ctx):
    """The same point twice without noise: the first observed component of the second copy repeats one of the first copy's, so
    the leading minor that fails is named as gradient point 1 and that DIRECTION (5), not as entry // nd and entry % nd of the
    compact index."""
    from gpplus_amd.errors import NotPSDError

    m, o, xg, dY, noise, xt = _case("c1-matern52")
    twice, dY2 = torch.cat([xg[:1], xg[:1]]), torch.cat([dY[:1], dY[:1]])
    mask = torch.zeros(2, dY.shape[1], dtype=torch.bool)
    mask[0, [2, 5]] = True
    mask[1, [5, 6]] = True
    with pytest.raises(NotPSDError, match=r"leading minor 3 .* 4 gradient observations .*gradient point 1, direction 5\)"):
        m.condition_on_gradients(twice, dY2, noise=0.0, observed=mask)
    post = m.condition_on_gradients(twice, dY2, noise=noise, observed=mask)  # with noise the duplicates are two readings
    assert post.num_gradient_observations == 4 and bool(torch.isfinite(post.predict(xt)[0]).all())


# ---- training ------------------------------------------------------------------------------------------------------------------------
def _train_case(name):
    """(a model of its own — the prediction tests leave their test rows' sources in the shared one's likelihood —, the mask, the
    reference loss and gradients with the noise given and with the default nugget): built once per case."""
    if name not in _train:
        from gpplus_amd.gradient_enhanced import GRADIENT_NUGGET_REL

        o, X, y, kw, xg, dY, noise, _ = G.gek_case(name)
        mask = P.pattern_mask(*dY.shape)
        _train[name] = (_model_from_oracle(o, X, y, **kw), mask, {True: P.gek_loss_and_grad_partial(o, xg, dY, noise, mask),
                               False: P.gek_loss_and_grad_partial(o, xg, dY, None, mask, GRADIENT_NUGGET_REL)})
    return _train[name]


def _evaluate(m, xg, dY, noise, mask):
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood

    m.train()
    m.zero_grad()
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, noise, mask)
    loss = -mll(m(*m.train_inputs), m.train_targets)
    loss.backward()
    m.eval()
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
def test_the_objective_against_the_partial_reference(gpu_ctx, name, noise_given):
    _, o, xg, dY, noise, _ = _case(name)
    m, mask, refs = _train_case(name)
    nz = noise if noise_given else None
    loss, grads = _evaluate(m, xg, _poison(dY, mask), nz, mask)
    _compare(f"{name} noise_given={noise_given}", loss, grads, *refs[noise_given], o.trainable)
    loss2, grads2 = _evaluate(m, xg, dY, nz, mask)  # two evaluations are bitwise equal, whatever lies under the mask
    assert torch.equal(_bits(loss), _bits(loss2))
    for n in grads:
        assert torch.equal(_bits(grads[n]), _bits(grads2[n])), n


@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_value_equals_the_log_density_of_the_bordered_factor(gpu_ctx, name):
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood

    _, o, xg, dY, noise, _ = _case(name)
    m, mask, _ = _train_case(name)
    gc = m.condition_on_gradients(xg, dY, noise=noise, observed=mask)._cache
    assert gc.jitter == 0.0
    n = gc.z.numel()
    assert n == m.train_inputs[0].shape[0] + int(mask.sum())
    bordered = (-0.5 * ((gc.z * gc.z).sum() + 2 * torch.log(gc.L.diagonal()).sum() + n * math.log(2 * math.pi))).item()
    m.train()
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, noise, mask)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")  # (jitter would be announced by a warning)
        value = mll.joint_log_prob(m.likelihood(m(*m.train_inputs)), m.train_targets).item()
    m.eval()
    rel = abs(value - bordered) / abs(bordered)
    print(f"{name}: from scratch {value:.12e}, bordered {bordered:.12e}: rel {rel:.2e}")
    assert rel <= 1e-9


def test_a_short_fit_lowers_the_loss_and_the_fitted_model_conditions(gpu_ctx):
    from gpplus_amd.optim import fit_model_torch

    o, X, y, xg, dY, noise = T.fit_case()
    mask = P.pattern_mask(*dY.shape)
    m = _model_from_oracle(o, X, y)
    start, _ = _evaluate(m, xg, dY, None, mask)
    best, histories = fit_model_torch(m, num_iter=60, num_restarts=0, verbose=False, objective="gek",
                                      gradients=(xg, _poison(dY, mask), None, mask))
    end, _ = _evaluate(m, xg, dY, None, mask)
    print(f"fit: loss {start.item():.6f} -> {end.item():.6f} in {len(histories[0])} Adam steps (best recorded {best:.6f})")
    assert math.isfinite(best) and end.item() < start.item() - 1e-3 * abs(start.item())
    post = m.condition_on_gradients(xg, dY, observed=mask)
    assert post.num_gradient_observations == int(mask.sum())
    assert bool(torch.isfinite(post.predict(xg)[0]).all()) and bool(torch.isfinite(post.predict_gradient(xg)[1]).all())


def test_refusals(gpu_ctx, monkeypatch):
    import calibration_reference as cr
    from gpplus_amd import linalg, settings
    from gpplus_amd.backend import GradientSelection
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood
    from gpplus_amd.models import GP_Plus

    m, o, xg, dY, noise, xt = _case("c3")
    Mg, p = dY.shape
    mask = P.pattern_mask(Mg, p)
    post = m.condition_on_gradients(xg, dY, noise=noise, observed=mask)
    cache = m.prediction_strategy
    m.train()
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, noise, mask)
    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            m.condition_on_gradients(xg, dY, noise=noise, observed=mask)
        with pytest.raises(NotImplementedError):
            post.predict(xt)
        with pytest.raises(NotImplementedError):
            post.predict_gradient(xt)
        with pytest.raises(NotImplementedError, match="sharded_evaluation"):
            mll(m(*m.train_inputs), m.train_targets)
    with monkeypatch.context() as mp:  # (a capture is not started for this: the check is the host-side query)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        sel = GradientSelection(mask, "cuda")
        with pytest.raises(NotImplementedError, match="capture"):
            linalg.append_gradients_to_cache(cache, post._cache.Ug, post._cache.d0, p, torch.ones(sel.q, device="cuda"),
                                             torch.ones(sel.q, dtype=torch.float64, device="cuda"), sel)
        with pytest.raises(NotImplementedError, match="capture"):
            linalg.predict_from_gradient_cache(post._cache, post._cache.Ug)
        with pytest.raises(NotImplementedError, match="capture"):
            mll(m(*m.train_inputs), m.train_targets)
    m.eval()
    empty = mask.clone()
    empty[1] = False
    nan = dY.clone()
    nan[tuple(mask.nonzero()[0])] = float("nan")
    for kw in (dict(observed=empty), dict(observed=mask[:, :-1]), dict(observed=mask.to(torch.float64) * 0.5), dict(dY=nan, observed=mask)):
        with pytest.raises(ValueError):
            m.condition_on_gradients(xg, kw.pop("dY", dY), noise=noise, **kw)
    # a calibrated model
    fx = cr.load_fixture()
    cm = GP_Plus(torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"]), dtype=torch.float64, device="cuda", calibration_id=[2],
                 **cr.C4_KW)
    xc = torch.tensor(fx["Xtest"])[:2]
    pc = int(cm.quant_index.numel())
    gc, mc = torch.ones(2, pc, dtype=torch.float64), P.alternating_row(pc)
    with pytest.raises(NotImplementedError, match="calibrat"):
        cm.condition_on_gradients(xc, gc, observed=mc)
    with pytest.raises(NotImplementedError, match="calibration"):
        cm.fit(objective="gek", gradients=(xc, gc, None, mc))
    with pytest.raises(NotImplementedError, match="calibration"):
        GradientEnhancedMarginalLogLikelihood(cm.likelihood, cm, xc, gc, None, mc)

"""``variance_reduction(..., gradient=)`` of GP_Plus and of GradientEnhancedPosterior and ``select_run_by_variance_reduction`` on the GPU,
on the cases of tests/alc_gradient_cases.py (c1 / c3 / c4 as tests/test_gpu_alc.py builds them, c1-matern52 / c1-matern32 from
``gek_reference.GEK_CASES``), with all gradient components and with about half of them, weighted and unweighted, against

  (a) tests/alc_gradient_reference.py — the long-double joint refit of [the model's observations; the candidate's value; its gradient
      components] — and
  (b) the package's independent route, for every candidate: sum_r w_r (std^2 of predict(Xref, include_noise=False) before - after
      ``condition_on(x_c, 0)`` followed by ``condition_on_gradients(x_c, 0, noise, observed=mask)``); from a gradient-enhanced posterior
      ``condition_on(x_c)`` followed by ``condition_on_gradients([Xg; x_c], ..., observed=[all; mask])``.

Both are held to 1e-10 of sf2 y_std^2, the bar of tests/test_gpu_alc.py; tests/test_alc_gradient_host.py shows the fp64 floor of every
case at or below 1e-16 of sf2 with cond(S_c) < 10 at the gradient noise of ``alc_gradient_cases.NOISE_REL`` (1e-4 of the prior
curvature for every case: none had to be raised).  Every test prints its observed errors before asserting (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alc_gradient_cases as C  # noqa: E402
import alc_gradient_reference as AG  # noqa: E402
import gek_reference as G  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-10
_models, _memo = {}, {}


def _case(name):
    """(model, candidates, reference rows, host inputs): built once per case; the model is only read afterwards."""
    if name not in _models:
        m, Xc, Xr = C.build(name, "cuda")
        m.predict(Xr[:3], return_std=True)  # a warm cache: the calls below reuse it
        _models[name] = (m, Xc, Xr, C.host_inputs(name, m, Xc, Xr, jitter=float(m.prediction_strategy.jitter)))
    return _models[name]


def _mask(p, which):
    return torch.ones(p, dtype=torch.bool) if which == "all" else C.half_mask(p)


def _weighted_variance(who, Xr, omega):
    _, std = who.predict(Xr, return_std=True, include_noise=False)
    return float((omega * std.double() ** 2).sum())


def _omega(Mr, weighted):
    omega = np.random.default_rng(11).uniform(0.0, 2.0, size=Mr) if weighted else None
    om = torch.full((Mr,), 1.0 / Mr, dtype=torch.float64, device="cuda") if omega is None else torch.tensor(omega, device="cuda")
    return omega, om


def _snapshot(m):
    c = m.prediction_strategy
    return [v.clone() for v in m.state_dict().values()] + [m.train_inputs[0].clone(), m.train_targets.clone(), c.L.clone(), c.Linv.clone(),
                                                           c.alpha.clone(), c.z.clone(), c.U.clone()]


@pytest.mark.parametrize("name", C.NAMES)
@pytest.mark.parametrize("which", ["all", "half"])
@pytest.mark.parametrize("weighted", [False, True])
def test_scores_against_the_joint_refit_and_against_conditioning(gpu_ctx, name, which, weighted):
    m, Xc, Xr, (ops, scale, p, d0, kappa) = _case(name)
    Mc, Mr = Xc.shape[0], Xr.shape[0]
    mask = _mask(p, which)
    omega, om = _omega(Mr, weighted)
    wts = None if omega is None else torch.tensor(omega)
    noise_row = torch.tensor(C.NOISE_REL[name] * kappa * scale)  # (y per input unit)^2
    m.predict(Xr[:3], return_std=True)  # (warm again: the cases share one workspace, another model may have factored into it since)
    cache, snap = m.prediction_strategy, _snapshot(m)
    gradient = True if which == "all" else mask
    got, value = m.variance_reduction(Xc, Xr, weights=wts, gradient=gradient, gradient_noise=noise_row)
    assert got.shape == (Mc,) and value.shape == (Mc,) and got.dtype == torch.float64 and m.prediction_strategy is cache and not m.training
    again, _ = m.variance_reduction(Xc, Xr, weights=wts, gradient=gradient, gradient_noise=noise_row)
    assert torch.equal(got, again)
    jitter = float(cache.jitter)
    key = (name, which, weighted)
    if key not in _memo:
        rel, gn = C.run_noise(name, kappa, mask.numpy(), Mc, jitter)
        _memo[key] = AG.score_by_refit(C.reference_model(ops), ops["Uc"], ops["noise_c"], gn, d0 + rel, ops["Ur"], omega) * scale
    ref = _memo[key]
    bar = TOL * ops["sf2"] * scale
    e_ref = float(np.abs(got.cpu().numpy().astype(np.longdouble) - ref).max())
    before = _weighted_variance(m, Xr, om)
    zero = torch.zeros(1, dtype=torch.float64)
    own = np.array([before - _weighted_variance(m.condition_on(Xc[c:c + 1], zero).condition_on_gradients(
        Xc[c:c + 1], torch.zeros(1, p, dtype=torch.float64), noise=noise_row, observed=mask), Xr, om) for c in range(Mc)])
    e_own = float(np.abs(got.cpu().numpy() - own).max())
    plain = m.variance_reduction(Xc, Xr, weights=wts)
    e_val = float((value - plain).abs().max())
    print(f"{name} {which} weighted {weighted}: scores in [{float(got.min()):.3e}, {float(got.max()):.3e}] (the value alone: "
          f"[{float(value.min()):.3e}, {float(value.max()):.3e}]), bar {bar:.3e}: against the joint refit {e_ref:.2e}, against conditioning "
          f"{e_own:.2e}, the value alone against variance_reduction {e_val:.2e}")
    assert bool((value > 0).all()) and bool((got >= value).all())
    assert e_ref <= bar and e_own <= bar and e_val <= bar, (e_ref, e_own, e_val, bar)
    for a, b in zip(snap, _snapshot(m)):
        assert torch.equal(a, b), "the receiver changed"


def test_default_noise_and_noise_forms(gpu_ctx):
    from gpplus_amd.gradient_enhanced import GRADIENT_NUGGET_REL

    m, Xc, Xr, (ops, scale, p, d0, kappa) = _case("c3")
    Mc = Xc.shape[0]
    row = torch.tensor(GRADIENT_NUGGET_REL * kappa * scale)
    default = m.variance_reduction(Xc, Xr, gradient=True)[0]
    explicit = m.variance_reduction(Xc, Xr, gradient=True, gradient_noise=row)[0]
    assert float((default - explicit).abs().max()) <= TOL * ops["sf2"] * scale
    full = m.variance_reduction(Xc, Xr, gradient=True, gradient_noise=row.expand(Mc, p).clone())[0]
    assert torch.equal(explicit, full)
    scalar = m.variance_reduction(Xc, Xr, gradient=True, gradient_noise=float(row[0]))[0]
    same = m.variance_reduction(Xc, Xr, gradient=True, gradient_noise=torch.full((p,), float(row[0]), dtype=torch.float64))[0]
    assert torch.equal(scalar, same)
    # more gradient noise, less gain; what lies under a False of the mask is not read
    noisy = m.variance_reduction(Xc, Xr, gradient=True, gradient_noise=1e4 * row)[0]
    assert bool((noisy < explicit).all())
    mask = C.half_mask(p)
    holes = torch.where(mask, row, torch.tensor(float("nan"), dtype=torch.float64))
    assert torch.equal(m.variance_reduction(Xc, Xr, gradient=mask, gradient_noise=holes)[0],
                       m.variance_reduction(Xc, Xr, gradient=mask, gradient_noise=row)[0])


@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_scores_from_a_gradient_enhanced_posterior(gpu_ctx, name):
    o, X, y, kw, xg, dY, noise, xt = C.oracle_case(name)
    key = ("posterior", name)
    if key not in _models:
        m = C.model_from_oracle(name, "cuda")
        _models[key] = (m, m.condition_on_gradients(xg, dY, noise=noise))
    m, post = _models[key]
    p = int(m.quant_index.numel())
    Xc, Xr = xt[8:12].clone(), xt[12:].clone()
    Mc, Mr = Xc.shape[0], Xr.shape[0]
    ops, scale, _, d0, kappa = C.host_inputs("posterior", m, Xc, Xr, jitter=float(post._cache.jitter))
    mask = C.half_mask(p)
    omega, om = _omega(Mr, True)
    wts = torch.tensor(omega)
    noise_row = torch.tensor(C.NOISE_REL[name] * kappa * scale)
    bar = TOL * ops["sf2"] * scale
    bits = [t.clone() for t in (post._cache.Linv, post._cache.z, post._cache.alpha)]
    plain = post.variance_reduction(Xc, Xr, weights=wts)
    with_g, value = post.variance_reduction(Xc, Xr, weights=wts, gradient=mask, gradient_noise=noise_row)
    assert plain.shape == (Mc,) and with_g.shape == (Mc,) and torch.equal(plain, post.variance_reduction(Xc, Xr, weights=wts))
    # (a) the long-double joint refit with the posterior's gradient observations in the model
    Mg = xg.shape[0]
    with torch.no_grad():
        Ug = m._features(xg.to(m.train_inputs[0]))[0].detach().cpu().numpy().astype(np.float64)
    gdirs = np.tile(d0 + np.arange(p), Mg)
    gnoise_g = np.tile(noise.numpy() / scale + float(post._cache.jitter), Mg)
    ref_model = C.reference_model(ops, np.repeat(Ug, p, 0), gdirs, gnoise_g)
    rel, gn = C.run_noise(name, kappa, mask.numpy(), Mc, float(post._cache.jitter))
    ref_g = AG.score_by_refit(ref_model, ops["Uc"], ops["noise_c"], gn, d0 + rel, ops["Ur"], omega) * scale
    ref_v = AG.score_by_refit(ref_model, ops["Uc"], ops["noise_c"], np.zeros((Mc, 0)), (), ops["Ur"], omega) * scale
    e_ref = max(float(np.abs(with_g.cpu().numpy().astype(np.longdouble) - ref_g).max()),
                float(np.abs(plain.cpu().numpy().astype(np.longdouble) - ref_v).max()))
    # (b) conditioning, for every candidate
    before = _weighted_variance(post, Xr, om)
    zero = torch.zeros(1, dtype=torch.float64)
    own_v, own_g = [], []
    for c in range(Mc):
        child = m.condition_on(Xc[c:c + 1], zero)
        own_v.append(before - _weighted_variance(child.condition_on_gradients(xg, dY, noise=noise), Xr, om))
        both = child.condition_on_gradients(torch.cat([xg, Xc[c:c + 1]]), torch.cat([dY, torch.zeros(1, p, dtype=dY.dtype)]),
                                            noise=torch.cat([noise.expand(Mg, p), noise_row[None]]),
                                            observed=torch.cat([torch.ones(Mg, p, dtype=torch.bool), mask[None]]))
        own_g.append(before - _weighted_variance(both, Xr, om))
    e_v = float(np.abs(plain.cpu().numpy() - np.array(own_v)).max())
    e_g = float(np.abs(with_g.cpu().numpy() - np.array(own_g)).max())
    e_val = float((value - plain).abs().max())
    print(f"{name} posterior ({post.num_gradient_observations} gradient observations): bar {bar:.3e}: against the joint refit {e_ref:.2e}; "
          f"against conditioning: gradient=None {e_v:.2e}, gradient=mask {e_g:.2e}; the value alone against gradient=None {e_val:.2e}")
    assert bool((plain > 0).all()) and bool((with_g >= value).all())
    assert e_ref <= bar and e_v <= bar and e_g <= bar and e_val <= bar, (e_ref, e_v, e_g, e_val, bar)
    for a, b in zip(bits, (post._cache.Linv, post._cache.z, post._cache.alpha)):
        assert torch.equal(a, b), "the posterior changed"


def test_the_pick_is_the_best_gain_per_cost_of_both_run_types(gpu_ctx):
    from gpplus_amd.bayesian_optimizations import select_run_by_variance_reduction

    m, Xc, Xr, (ops, scale, p, d0, kappa) = _case("c1")
    Mc = Xc.shape[0]
    from gpplus_amd.gradient_enhanced import GRADIENT_NUGGET_REL
    rel, gn = C.run_noise("c1", kappa, np.ones(p, dtype=bool), Mc)
    gn = gn / C.NOISE_REL["c1"] * GRADIENT_NUGGET_REL + float(m.prediction_strategy.jitter)  # (the default noise of the public entry)
    ref_model = C.reference_model(ops)
    ref_g = AG.score_by_refit(ref_model, ops["Uc"], ops["noise_c"], gn, d0 + rel, ops["Ur"]) * scale
    ref_v = AG.score_by_refit(ref_model, ops["Uc"], ops["noise_c"], np.zeros((Mc, 0)), (), ops["Ur"]) * scale
    seen = set()
    vec = np.linspace(1.0, 2.0, Mc)
    for cv, cg in ((1.0, 2.0), (1.0, 1e6), (1.0, 1.0001), (vec, 3.0 * vec[::-1].copy())):
        rank = np.stack([ref_v / cv, ref_g / cg], 1).astype(np.float64)
        flat = np.sort(rank.reshape(-1))[::-1]
        margin = float((flat[0] - flat[1]) / flat[0])
        j, t = np.unravel_index(int(np.argmax(rank)), rank.shape)
        idx, with_gradient, gains = select_run_by_variance_reduction(m, Xc, Xr, cost_value=torch.as_tensor(cv), cost_gradient=torch.as_tensor(cg))
        print(f"costs {np.asarray(cv).reshape(-1)[0]:g} / {np.asarray(cg).reshape(-1)[0]:g}: reference pick {j} ({'gradient' if t else 'value'}), "
              f"margin {margin:.2e}; got {idx} ({'gradient' if with_gradient else 'value'})")
        assert margin > 1e-6 and (idx, bool(with_gradient)) == (int(j), bool(t))
        assert gains.shape == (Mc, 2) and float(np.abs(gains.cpu().numpy() - np.stack([ref_v, ref_g], 1).astype(np.float64)).max()) <= \
            TOL * ops["sf2"] * scale
        seen.add(bool(t))
    assert seen == {False, True}, "the costs never flip the run type"
    # the defaults: gradient=True, costs 1 and 2; a posterior takes the same call
    assert select_run_by_variance_reduction(m, Xc, Xr)[:2] == select_run_by_variance_reduction(m, Xc, Xr, cost_value=1.0, cost_gradient=2.0)[:2]


def test_without_the_new_keywords_nothing_changed(gpu_ctx):
    from gpplus_amd import settings

    m, Xc, Xr, (ops, scale, p, d0, kappa) = _case("c4")
    wts = torch.rand(Xr.shape[0], generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    old = m._variance_reduction(Xc, Xr, wts)[0]  # (what variance_reduction returned before the keywords existed)
    a, b = m.variance_reduction(Xc, Xr, weights=wts), m.variance_reduction(Xc, Xr, wts)
    bits = lambda t: t.contiguous().view(torch.int64)  # noqa: E731
    assert torch.equal(bits(a), bits(old)) and torch.equal(bits(b), bits(old)) and torch.is_tensor(a)
    assert torch.equal(bits(m.variance_reduction(Xc, Xr, None, None, None)), bits(m._variance_reduction(Xc, Xr)[0]))
    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            m.variance_reduction(Xc, Xr, gradient=True)

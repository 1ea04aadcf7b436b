"""Differentiable posterior paths on the GPU: ``PosteriorPaths.paths_with_grad`` against ``paths`` (bit for bit) and against the
dense autograd reference of tests/pathwise_grad_reference.py, ``minimize`` and ``thompson_sample``.

Tolerances: the project's gradient tolerance, 1e-5 of max |g|, and its prediction tolerance, 1e-4 of max |f|.
Observed on an MI355X: see DESIGN.md section 3.10.  Models, paths (S = 8, F = 256) and held-out points are those of
tests/test_gpu_pathwise.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import pathwise_grad_reference as G  # noqa: E402
import test_gpu_pathwise as T  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL_GRAD, RTOL_PRED = 1e-5, 1e-4


@pytest.fixture(scope="module")
def cases(gpu_ctx):
    """name -> (fixture, model, paths, held-out inputs): built once, never modified."""
    out = {}
    for name in T.MODELS:
        fx, m = T._model(name)
        paths = m.sample_paths(size=8, num_features=256, generator=torch.Generator().manual_seed(1234))
        out[name] = (fx, m, paths, T._held_out(fx, T.MODELS[name][1]))
    return out


def _dense_values(paths, Us):
    """g_s + k c_s at the feature rows Us (CPU), from the paths' own tensors."""
    spec = paths.spec
    c = lambda t: t.detach().cpu().to(torch.float64)  # noqa: E731
    return G.dense_path_values(Us, c(paths.U), c(spec.w).reshape(-1), float(spec.sf2), int(spec.kind), int(spec.d_split),
                               c(paths.omega), c(paths.phase), c(paths.theta), c(paths.coef))


@pytest.mark.parametrize("name", list(T.MODELS))
def test_values_are_those_of_paths_and_the_gradient_matches_the_dense_reference(cases, name):
    fx, m, paths, Xt = cases[name]
    want = paths.paths(Xt)
    assert not want.requires_grad and want.grad_fn is None  # paths() itself carries no graph
    X = Xt.clone().requires_grad_(True)
    got = paths.paths_with_grad(X)
    assert got.shape == want.shape and got.dtype == torch.float64 and got.requires_grad
    assert torch.equal(got.detach(), want)
    Gw = torch.randn(want.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    (grad,) = torch.autograd.grad((Gw.cuda() * got).sum(), X)
    # the dense reference: autograd on the CPU through the features; the model's features are [embedding | quantitative columns]
    Us, _ = T._features_and_mean(m, Xt)
    Us = Us.clone().requires_grad_(True)
    (gU,) = torch.autograd.grad((Gw.T * _dense_values(paths, Us)).sum(), Us)
    quant = m.quant_index.cpu().tolist()
    ref = torch.zeros(Xt.shape, dtype=torch.float64)
    ref[:, quant] = gU[:, Us.shape[1] - len(quant):]
    other = [c for c in range(Xt.shape[1]) if c not in quant]
    assert bool((grad[:, other] == 0).all()), "categorical and source columns get zero gradient"
    err = (grad.cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(f"{name}: max |g - ref| / max |g| = {err:.3e}")
    assert err <= RTOL_GRAD


@pytest.mark.parametrize("name", ["c1", "c4"])
def test_chunking_changes_no_bit(cases, name):
    fx, m, paths, Xt = cases[name]
    X0 = torch.cat([Xt, m.train_inputs[0][:70]])
    Gw = torch.randn(8, X0.shape[0], dtype=torch.float64, generator=torch.Generator().manual_seed(3)).cuda()
    res = []
    for chunk in (None, 37, 1000):
        X = X0.clone().requires_grad_(True)
        f = paths.paths_with_grad(X, chunk=chunk)
        res.append((f.detach(), torch.autograd.grad((Gw * f).sum(), X)[0]))
    assert torch.equal(res[0][0], paths.paths(X0))
    for f, g in res[1:]:
        assert torch.equal(f, res[0][0]) and torch.equal(g, res[0][1])
    with pytest.raises(ValueError):
        paths.paths_with_grad(X0, chunk=0)
    with pytest.raises(ValueError):
        paths.paths_with_grad(X0[:, :-1])


def test_paths_belong_to_their_parameters(gpu_ctx):
    fx, m = T._model("c3")
    Xt = T._held_out(fx, T.MODELS["c3"][1], 10)
    p = m.sample_paths(size=2, num_features=32, generator=torch.Generator().manual_seed(1))
    assert p.paths_with_grad(Xt).shape == (2, 10)
    with torch.no_grad():
        m.likelihood.noise_covar.raw_noise.add_(0.5)
    with pytest.raises(RuntimeError):
        p.paths_with_grad(Xt)
    with pytest.raises(RuntimeError):
        p.minimize(Xt.min(0).values.cpu(), Xt.max(0).values.cpu(), fixed={0: 0.0, 5: 0.0})


def _box(fx, name):
    Xtr = torch.tensor(fx["Xtrain"] if "Xtrain" in fx else fx["Utrain"])
    fixed = {c: float(Xtr[3, c]) for c in T.MODELS[name][1].get("qual_dict", {})}
    return Xtr.min(0).values, Xtr.max(0).values, fixed


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_minimize(cases, name):
    fx, m, _, _ = cases[name]
    lo, hi, fixed = _box(fx, name)
    kw = dict(fixed=fixed, num_candidates=256, num_starts=3, steps=20)
    paths = m.sample_paths(size=4, num_features=256, generator=torch.Generator().manual_seed(11))
    res = paths.minimize(lo, hi, generator=torch.Generator().manual_seed(5), **kw)
    p = lo.numel()
    assert res.x.shape == (4, p) and res.f.shape == (4,) and res.f_candidates.shape == (4,) and res.x_starts.shape == (4, 3, p)
    x = res.x.cpu()
    assert bool((x >= lo).all()) and bool((x <= hi).all())
    for c, v in fixed.items():
        assert bool((x[:, c] == v).all()) and bool((res.x_starts[..., c] == v).all())
    assert bool((res.f <= res.f_candidates).all())
    print(f"{name}: best candidate {res.f_candidates.tolist()}, after descent {res.f.tolist()}")
    assert torch.equal(res.f, paths.paths(res.x).diagonal())
    again = paths.minimize(lo, hi, generator=torch.Generator().manual_seed(5), **kw)
    for a in ("x", "f", "f_candidates", "x_starts"):
        assert torch.equal(getattr(again, a), getattr(res, a)), a
    # the dense reference's path at x
    ref = T._reference_of(paths)
    Us, mean = T._features_and_mean(m, res.x)
    want = ref.paths(Us, mean, paths.omega, paths.phase, paths.theta, paths.eps).diagonal()
    err = (res.f.cpu() - want).abs().max().item() / want.abs().max().item()
    print(f"{name}: max |f(x) - ref| / max |f| = {err:.3e}")
    assert err <= RTOL_PRED
    # the other direction: the maximiser is no worse than the best candidate either
    up = paths.minimize(lo, hi, maximize=True, generator=torch.Generator().manual_seed(5), **kw)
    assert bool((up.f >= up.f_candidates).all()) and bool((up.f >= res.f).all())
    if fixed:
        with pytest.raises(ValueError):
            paths.minimize(lo, hi, num_candidates=8, num_starts=2, steps=1)  # categorical columns left free


def test_thompson_sample(cases):
    from gpplus_amd.bayesian_optimizations import thompson_sample

    fx, m, _, _ = cases["c3"]
    lo, hi, fixed = _box(fx, "c3")
    x = thompson_sample(m, 3, lo, hi, fixed=fixed, num_features=128, generator=torch.Generator().manual_seed(2), num_candidates=64,
                        num_starts=2, steps=5)
    assert x.shape == (3, lo.numel()) and x.device.type == "cuda"
    assert bool((x.cpu() >= lo).all()) and bool((x.cpu() <= hi).all())
    for c, v in fixed.items():
        assert bool((x[:, c] == v).all())

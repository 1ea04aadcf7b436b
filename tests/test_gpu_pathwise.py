"""Pathwise posterior draws on the GPU (gpplus_amd.pathwise, GP_Plus.sample_paths) against the dense CPU reference of
tests/pathwise_reference.py fed the paths' own tensors; the training identity; chunking and seeding bit for bit; the model-level
statistics on c1; sample_paths end to end on the mixed and the multi-fidelity model.

Parity tolerance: the project's prediction tolerance, 1e-4 of max |f|.  Observed on an MI355X: see DESIGN.md
section 3.9."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import pathwise_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
RTOL_PRED = 1e-4
C3_KW = {"qual_dict": {0: 5, 5: 5}}
C4_KW = {"qual_dict": {10: 3}, "multiple_noise": True, "m_gp": "multiple_constant"}
MODELS = {
    "c1": ("c1_borehole_n500.npz", {}),
    "c3": ("c3_borehole_mixed_n100.npz", C3_KW),
    "c4": ("c4_wing_mf_n300.npz", C4_KW),
    "c1_matern52": ("c1_borehole_n500.npz", {"quant_correlation_class": "Matern52Kernel"}),
}


def _model(name):
    from gpplus_amd.models import GP_Plus

    fixture, kw = MODELS[name]
    fx = dict(np.load(os.path.join(GOLD, fixture)))
    xkey = "Xtrain" if "Xtrain" in fx else "Utrain"
    m = GP_Plus(torch.tensor(fx[xkey]), torch.tensor(fx["ytrain"]), dtype=torch.float64, device="cuda", **kw)
    sd = m.state_dict()
    for k in list(sd):
        fk = f"theta1::param::{k}"
        if fk in fx and np.size(fx[fk]) == sd[k].numel():
            sd[k] = torch.as_tensor(fx[fk]).reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    m.eval()
    return fx, m


def _held_out(fx, kw, n=64):
    """n held-out inputs: the fixture's test points; where it has fewer (c4: 60), further ones made from its first points by moving
    every quantitative column 3 % of its training range."""
    Xtr = fx["Xtrain"] if "Xtrain" in fx else fx["Utrain"]
    Xt = (fx["Xtest"] if "Xtest" in fx else fx["Utest"])[:n]
    if Xt.shape[0] < n:
        extra = Xt[:n - Xt.shape[0]].copy()
        quant = [c for c in range(Xtr.shape[1]) if c not in kw.get("qual_dict", {})]
        extra[:, quant] += 0.03 * (Xtr[:, quant].max(0) - Xtr[:, quant].min(0))
        Xt = np.concatenate([Xt, extra])
    return torch.tensor(Xt, device="cuda")


def _features_and_mean(m, X):
    """u(x) and m(x) of the model's own eval-mode forward, on the CPU."""
    from gpplus_amd.gpcore.module import Module

    with torch.no_grad():
        out = Module.__call__(m, X)
    return out.lazy_covariance_matrix.U1.to(torch.float64).cpu(), out.mean.to(torch.float64).cpu()


def _reference_of(paths):
    """The dense reference on the paths' own training features, residual, noise and kernel."""
    spec = paths.spec
    m = paths.model
    Xtr = m.train_inputs[0]
    _, mean_tr = _features_and_mean(m, Xtr)
    resid = m.train_targets.to(torch.float64).cpu() - mean_tr
    return R.PathReference(paths.U.cpu(), resid, paths.noise.cpu(), spec.w.cpu(), float(spec.sf2), spec.kind, spec.d_split)


@pytest.fixture(scope="module")
def cases(gpu_ctx):
    """name -> (fixture, model, paths, reference, held-out inputs): S = 8, F = 256, one seed; built once, never modified."""
    out = {}
    for name in MODELS:
        fx, m = _model(name)
        paths = m.sample_paths(size=8, num_features=256, generator=torch.Generator().manual_seed(1234))
        out[name] = (fx, m, paths, _reference_of(paths), _held_out(fx, MODELS[name][1]))
    return out


@pytest.mark.parametrize("name", list(MODELS))
def test_paths_match_the_dense_reference(cases, name):
    fx, m, paths, ref, Xt = cases[name]
    assert Xt.shape[0] == 64
    assert paths.omega.shape == (256, paths.U.shape[1]) and paths.theta.shape == (256, 8)
    assert paths.eps.shape == paths.coef.shape == (paths.U.shape[0], 8)
    args = (paths.omega, paths.phase, paths.theta, paths.eps)
    for what, X in (("held-out", Xt), ("training", m.train_inputs[0])):
        got = paths.paths(X)
        assert got.shape == (8, X.shape[0]) and got.dtype == torch.float64 and not got.requires_grad
        Us, mean = _features_and_mean(m, X)
        want = ref.paths(Us, mean, *args)
        err = (got.cpu() - want).abs().max().item() / want.abs().max().item()
        print(f"{name} {what}: max |f - ref| / max |f| = {err:.3e}")
        assert err <= RTOL_PRED
    # the coefficients themselves, through their effect: K c against the reference's K c_ref
    cref = ref.coef(*args)
    kc = ref.K @ paths.coef.cpu()
    assert (kc - ref.K @ cref).abs().max().item() <= RTOL_PRED * max(kc.abs().max().item(), 1.0)


@pytest.mark.parametrize("name", list(MODELS))
def test_training_identity(cases, name):
    """paths(X_train) = y - eps - T coef in the scaled target space (K = Ky - T)."""
    fx, m, paths, ref, _ = cases[name]
    got = paths.paths(m.train_inputs[0])
    y = m.train_targets.to(torch.float64)
    want = (y.unsqueeze(1) - paths.eps - paths.noise.unsqueeze(1) * paths.coef).T
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"{name}: training identity, max error / max |f| = {err:.3e}")
    assert err <= RTOL_PRED


@pytest.mark.parametrize("name", ["c1", "c4"])
def test_chunking_and_seeding_are_bitwise(cases, name):
    fx, m, paths, _, Xt = cases[name]
    X = torch.cat([Xt, m.train_inputs[0][:70]])
    whole = paths.paths(X)
    assert torch.equal(paths.paths(X, chunk=37), whole)
    assert torch.equal(paths(X, chunk=1000), whole)
    again = m.sample_paths(size=8, num_features=256, generator=torch.Generator().manual_seed(1234))
    for a in ("omega", "phase", "theta", "eps", "coef"):
        assert torch.equal(getattr(again, a), getattr(paths, a)), a
    assert torch.equal(again.paths(X), whole)
    other = m.sample_paths(size=8, num_features=256, generator=torch.Generator().manual_seed(4321))
    assert not torch.equal(other.paths(X), whole)


def test_model_level_statistics(cases):
    """c1, S = 4096, F = 2048, 64 held-out points: the mean over the paths is the predictive mean (unbiased for any F) within
    6 sd / sqrt(S) at every point, and the sample variance is the reference's RFF-exact variance within 6 sqrt(2 / (S - 1))
    relative at every point.  The distance of the RFF-exact variance from the true posterior variance is printed only."""
    fx, m, _, _, Xt = cases["c1"]
    S, F = 4096, 2048
    paths = m.sample_paths(size=S, num_features=F, generator=torch.Generator().manual_seed(99))
    f = paths.paths(Xt).cpu()
    with torch.no_grad():
        pred = m(Xt).mean.to(torch.float64).cpu()
    sd = f.std(0, unbiased=True)
    zmean = ((f.mean(0) - pred).abs() / (sd / math.sqrt(S)))
    ref = _reference_of(paths)
    Us, mean = _features_and_mean(m, Xt)
    rv = ref.rff_variance(Us, paths.omega, paths.phase)
    zvar = (f.var(0, unbiased=True) / rv - 1.0).abs() / math.sqrt(2.0 / (S - 1))
    _, pv = ref.posterior(Us, mean)
    print(f"c1 S={S} F={F}: mean z max {zmean.max().item():.2f}, variance z max {zvar.max().item():.2f}, "
          f"max |rff var / true var - 1| = {(rv / pv - 1).abs().max().item():.3f}")
    assert zmean.shape == (64,) and bool((zmean <= 6.0).all())
    assert zvar.shape == (64,) and bool((zvar <= 6.0).all())


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_sample_paths_end_to_end(gpu_ctx, name):
    """Shapes, dtype, reproducibility under a seed, and survival of another model of the same N taking the shared workspace."""
    from gpplus_amd.pathwise import PosteriorPaths

    fx, m = _model(name)
    Xt = _held_out(fx, MODELS[name][1], 40)
    p = m.sample_paths(size=3, num_features=100, generator=torch.Generator().manual_seed(7))
    assert isinstance(p, PosteriorPaths) and p.size == 3 and p.num_features == 100
    f = p.paths(Xt)
    assert f.shape == (3, 40) and f.dtype == torch.float64 and f.device.type == "cuda" and bool(torch.isfinite(f).all())
    one = p.paths(Xt[0])
    assert one.shape == (3, 1) and torch.equal(one, f[:, :1])
    draws = m.sample_y(size=2, X=Xt)
    assert draws.dtype == f.dtype  # the dtype (and scaling) sample_y returns
    # another model of the same N factors into the shared prediction workspace ...
    fx2, m2 = _model(name)
    with torch.no_grad():
        m2.likelihood.noise_covar.raw_noise.add_(1.0)
    m2.eval()
    m2.predict(Xt, return_std=True)
    assert m.prediction_strategy.stale()
    # ... the existing paths are unaffected, and new ones from the same seed are the same paths
    assert torch.equal(p.paths(Xt), f)
    q = m.sample_paths(size=3, num_features=100, generator=torch.Generator().manual_seed(7))
    assert torch.equal(q.coef, p.coef) and torch.equal(q.paths(Xt), f)
    with pytest.raises(ValueError):
        p.paths(Xt[:, :-1])
    with pytest.raises(ValueError):
        m.sample_paths(size=0)
    # paths belong to the parameters they were drawn under
    with torch.no_grad():
        m.likelihood.noise_covar.raw_noise.add_(0.5)
    with pytest.raises(RuntimeError):
        p.paths(Xt)
    m.sample_paths(size=1, num_features=8, generator=torch.Generator().manual_seed(1)).paths(Xt)
    with pytest.raises(ValueError):
        m.sample_paths(generator=torch.Generator(device="cuda"))

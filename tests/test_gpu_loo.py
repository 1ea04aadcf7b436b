"""Leave-one-out log pseudo-likelihood on the HIP path (linalg.exact_loo: gpp_loo_scalars, gpp_sym_rowscale, the TN GEMM,
gpp_loo_grad_reduce) against the dense fp64 CPU reference of tests/loo_reference.py, and the public interface on top of it.

Tolerances are the project's: 1e-5 relative for the value, 1e-5 of max|g| per gradient vector.  Every test
prints its observed errors before asserting (pytest -s shows them).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loo_reference import KIND_MATERN52, KIND_RBF, loo_autograd, loo_closed_form, loo_dense, make_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-5


# (N, D, kind, d_split, S, dU): every N of {63, 65, 333, 1537}; D = 3, 8, 20; RBF and Matern 5/2 with d_split; one noise level
# without a group index and three with one; with and without feature gradients
CASES = [
    (63, 3, KIND_RBF, 0, 1, 0),
    (65, 8, KIND_MATERN52, 3, 3, 2),
    (333, 20, KIND_RBF, 0, 3, 2),
    (333, 8, KIND_MATERN52, 2, 1, 0),
    (1537, 8, KIND_RBF, 0, 3, 0),
    (1537, 20, KIND_MATERN52, 5, 3, 2),
]


@functools.lru_cache(maxsize=None)
def _reference(N, D, kind, d_split, S):
    """Inputs and the autograd reference of one case, computed once and shared (read-only)."""
    inp = make_inputs(N, D, seed=1000 + N + D, S=S)
    val, grads = loo_autograd(**inp, kind=kind, d_split=d_split)
    return inp, val, grads


def _evaluate(inp, kind, d_split, dU, need_grad=True):
    """One exact_loo evaluation on the GPU: (value, gradients as CPU tensors)."""
    from gpplus_amd.linalg import KernelSpec, exact_loo

    leaves = {k: inp[k].to("cuda").requires_grad_(need_grad) for k in ("U", "w", "sf2", "tau", "mean", "y")}
    grp = None if inp["grp"] is None else inp["grp"].to("cuda")
    spec = KernelSpec(leaves["w"], leaves["sf2"], kind, d_split)
    val = exact_loo(leaves["U"], spec, leaves["tau"], leaves["mean"], leaves["y"], grp, n_grad_dims=dU)
    if not need_grad:
        return val.detach().cpu(), None
    val.backward()
    return val.detach().cpu(), {k: v.grad.detach().cpu() for k, v in leaves.items()}


def _check(val, grads, ref_val, ref_grads, dU, label):
    err = abs(val.item() - ref_val.item()) / abs(ref_val.item())
    print(f"{label}: value {val.item():.12f} ref {ref_val.item():.12f} rel err {err:.2e}")
    errs = {}
    for name, ref in ref_grads.items():
        got = grads[name].reshape(ref.shape)
        if name == "U":  # only the leading dU feature columns carry a gradient; the others are reported as zero
            assert torch.count_nonzero(got[:, dU:]) == 0
            got, ref = got[:, :dU], ref[:, :dU]
            if dU == 0:
                continue
        errs[name] = ((got - ref).abs().max().item(), ref.abs().max().item())
        print(f"{label}: d{name}: max err {errs[name][0]:.3e} of max|g| {errs[name][1]:.3e} ({errs[name][0] / errs[name][1]:.2e})")
    assert err <= RTOL, (label, err)
    for name, (e, scale) in errs.items():
        assert e <= RTOL * scale, (label, name, e, scale)


@pytest.mark.parametrize("N,D,kind,d_split,S,dU", CASES)
def test_exact_loo_matches_autograd(gpu_ctx, N, D, kind, d_split, S, dU):
    inp, ref_val, ref_grads = _reference(N, D, kind, d_split, S)
    val, grads = _evaluate(inp, kind, d_split, dU)
    _check(val, grads, ref_val, ref_grads, dU, f"N={N} D={D} kind={kind} S={S} dU={dU}")
    # bitwise repeatable, and the value does not depend on whether a gradient was asked for
    val2, grads2 = _evaluate(inp, kind, d_split, dU)
    assert torch.equal(val, val2)
    for name in grads:
        assert torch.equal(grads[name], grads2[name]), name
    val3, _ = _evaluate(inp, kind, d_split, dU, need_grad=False)
    assert torch.equal(val, val3)


def test_exact_loo_large_matches_closed_form(gpu_ctx):
    """N = 5200: 128-wide LAUUM tiles and the look-ahead factorisation; the reference is the closed form (no autograd graph of a
    5200 x 5200 inverse)."""
    N, D = 5200, 8
    inp = make_inputs(N, D, seed=5200, S=3)
    ref_val, ref_grads = loo_closed_form(**inp, kind=KIND_RBF, d_split=0, dU=0)
    val, grads = _evaluate(inp, KIND_RBF, 0, 0)
    _check(val, grads, ref_val, ref_grads, 0, f"N={N} D={D}")


@pytest.mark.parametrize("N", [1, 64, 65, 200])
def test_sym_rowscale_against_numpy(gpu_ctx, N):
    from gpplus_amd.backend import square_buffer

    rng = np.random.default_rng(N)
    A = rng.standard_normal((N, N))
    s = rng.uniform(0.5, 2.0, N)
    sym = np.tril(A) + np.tril(A, -1).T
    want = s[:, None] * sym
    Kinv = square_buffer(N, "cuda")
    poisoned = np.where(np.tril(np.ones((N, N), dtype=bool)), A, np.nan)  # nothing above the diagonal may be read
    Kinv.copy_(torch.from_numpy(poisoned))
    out = square_buffer(N, "cuda")
    out.fill_(np.nan)
    gpu_ctx.sym_rowscale(Kinv, torch.from_numpy(s).cuda(), out)
    got = out.cpu().numpy()
    assert np.array_equal(got, want)  # one multiplication per entry: exact
    assert np.array_equal(np.isnan(Kinv.cpu().numpy()), np.isnan(poisoned))  # out of place: the input is untouched


def test_loo_scalars_rows_do_not_depend_on_the_matrix_around_them(gpu_ctx):
    """d_i = sum_{j >= i} Linv[i, j]^2 reads row i from the diagonal on and nothing else: NaN below the diagonal changes nothing,
    and the values agree with numpy to round-off."""
    from gpplus_amd.backend import square_buffer

    N = 131
    rng = np.random.default_rng(3)
    M = rng.standard_normal((N, N))
    alpha, y = rng.standard_normal(N), rng.standard_normal(N)
    Li = square_buffer(N, "cuda")
    Li.copy_(torch.from_numpy(np.where(np.triu(np.ones((N, N), dtype=bool)), M, np.nan)))
    d, mu, s2, a, sb = (torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(5))
    val = torch.empty(1, dtype=torch.float64, device="cuda")
    gpu_ctx.loo_scalars(Li, torch.from_numpy(alpha).cuda(), torch.from_numpy(y).cuda(), d, mu=mu, s2=s2, a=a, sqrtb=sb, loo=val)
    dref = (np.triu(M) ** 2).sum(axis=1)
    np.testing.assert_allclose(d.cpu().numpy(), dref, rtol=1e-13)
    np.testing.assert_allclose(mu.cpu().numpy(), y - alpha / dref, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(s2.cpu().numpy(), 1.0 / dref, rtol=1e-13)
    np.testing.assert_allclose(a.cpu().numpy(), -alpha / dref, rtol=1e-13)
    np.testing.assert_allclose(sb.cpu().numpy(), np.sqrt(0.5 / dref + 0.5 * alpha ** 2 / dref ** 2), rtol=1e-13)
    want = (0.5 * np.log(dref) - 0.5 * alpha ** 2 / dref).sum() - 0.5 * N * np.log(2 * np.pi)
    np.testing.assert_allclose(val.item(), want, rtol=1e-12)


def _load(name):
    return dict(np.load(os.path.join(GOLD, name)))


def _build(fx, tag, **kw):
    from gpplus_amd.models import GP_Plus

    xkey = "Xtrain" if "Xtrain" in fx else "Utrain"
    m = GP_Plus(torch.tensor(fx[xkey]), torch.tensor(fx["ytrain"]), dtype=torch.float64, device="cuda", **kw)
    sd = m.state_dict()
    for k in list(sd):
        fk = f"{tag}::param::{k}"
        if fk in fx:
            sd[k] = torch.as_tensor(fx[fk]).reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    return m


def test_loo_predict_against_delete_one_solves(gpu_ctx):
    """N = 65: GP_Plus.loo_predict() against 65 explicit dense solves, each with one training point removed."""
    from gpplus_amd.models import GP_Plus

    fx = _load("c1_borehole_n500.npz")
    N = 65
    m = GP_Plus(torch.tensor(fx["Xtrain"][:N]), torch.tensor(fx["ytrain"][:N]), dtype=torch.float64, device="cuda")
    sd = m.state_dict()
    for k, v in {"covar_module.base_kernel.raw_lengthscale": -1.0, "covar_module.raw_outputscale": 0.3,
                 "likelihood.noise_covar.raw_noise": -6.0, "mean_module.constant": 0.4}.items():
        sd[k] = torch.full_like(sd[k], v)
    m.load_state_dict(sd)
    m.train()
    with torch.no_grad():
        out = m.likelihood(m(*m.train_inputs))
        Ky = out.covariance_matrix.cpu().to(torch.float64)
        mean = out.mean.cpu().to(torch.float64)
    y = m.train_targets.cpu().to(torch.float64)
    mu_ref, sd_ref = torch.empty(N, dtype=torch.float64), torch.empty(N, dtype=torch.float64)
    for i in range(N):
        keep = torch.arange(N) != i
        Kmm, k = Ky[keep][:, keep], Ky[keep, i]
        sol = torch.linalg.solve(Kmm, torch.stack([y[keep] - mean[keep], k], dim=1))
        mu_ref[i] = mean[i] + k @ sol[:, 0]
        sd_ref[i] = (Ky[i, i] - k @ sol[:, 1]).sqrt()
    y_min, y_std = m.y_min.cpu().to(torch.float64), m.y_std.cpu().to(torch.float64)
    mu_ref, sd_ref = y_min + y_std * mu_ref, sd_ref * y_std.abs()
    mu, sd_ = m.loo_predict()
    assert mu.shape == (N,) and sd_.shape == (N,)
    e_mu = (mu.cpu() - mu_ref).abs().max().item() / mu_ref.abs().max().item()
    e_sd = (sd_.cpu() - sd_ref).abs().max().item() / sd_ref.abs().max().item()
    print(f"loo_predict N={N}: mean rel err {e_mu:.2e}, std rel err {e_sd:.2e}")
    assert e_mu <= RTOL and e_sd <= RTOL
    # from the cache: asking again factors nothing and gives the same bits
    mu2, sd2 = m.loo_predict()
    assert torch.equal(mu, mu2) and torch.equal(sd_, sd2)


MODEL_CASES = [
    ("c3_borehole_mixed_n100.npz", {"qual_dict": {0: 5, 5: 5}}),
    ("c4_wing_mf_n300.npz", {"qual_dict": {10: 3}, "multiple_noise": True, "m_gp": "multiple_constant"}),
]


def _objective(m, loo):
    out = m(*m.train_inputs)
    return loo(out, m.train_targets)


@pytest.mark.parametrize("fixture,kw", MODEL_CASES)
def test_model_objective_value_and_directional_derivative(gpu_ctx, fixture, kw):
    """Manifold (categorical inputs through a latent map: feature gradients) and multiple noise levels: the objective's value
    against the reference on the model's own dense covariance, and a central difference along the gradient direction."""
    from gpplus_amd.gpcore import LeaveOneOutPseudoLikelihood

    fx = _load(fixture)
    m = _build(fx, "theta1", **kw)
    m.train()
    loo = LeaveOneOutPseudoLikelihood(m.likelihood, m)
    N = m.train_targets.shape[0]
    with torch.no_grad():
        noisy = m.likelihood(m(*m.train_inputs))
        Ky, mean = noisy.covariance_matrix.cpu().to(torch.float64), noisy.mean.cpu().to(torch.float64)
        prior = loo._prior_sum(torch.float64)
        prior = 0.0 if prior is None else prior.item()
    ref = (loo_dense(Ky, m.train_targets.cpu().to(torch.float64) - mean).item() + prior) / N
    params = [p for p in m.parameters() if p.requires_grad]
    for p in params:
        p.grad = None
    val = _objective(m, loo)
    val.backward()
    err = abs(val.item() - ref) / abs(ref)
    print(f"{fixture}: objective {val.item():.12f} ref {ref:.12f} rel err {err:.2e}")
    assert err <= RTOL
    params = [p for p in params if p.grad is not None]
    g = torch.cat([p.grad.reshape(-1) for p in params]).to(torch.float64)
    assert bool(torch.isfinite(g).all()) and g.abs().max().item() > 0
    gg = (g @ g).item()
    u = g / g.norm()
    theta0 = [p.detach().clone() for p in params]
    eps = 1e-5

    def at(step):
        with torch.no_grad():
            o = 0
            for p, p0 in zip(params, theta0):
                n = p.numel()
                p.copy_(p0 + step * u[o:o + n].reshape(p.shape).to(p0))
                o += n
            return _objective(m, loo).item()

    fd = (at(eps) - at(-eps)) / (2 * eps) * g.norm().item()
    at(0.0)
    e = abs(fd - gg) / gg
    print(f"{fixture}: central difference along g: {fd:.10e} against g.g {gg:.10e} (rel {e:.2e})")
    assert e <= RTOL


@pytest.mark.parametrize("fixture,kw", MODEL_CASES)
def test_fit_model_torch_with_the_loo_objective(gpu_ctx, fixture, kw):
    from gpplus_amd.optim import fit_model_torch

    fx = _load(fixture)
    m = _build(fx, "theta1", **kw)
    best, histories = fit_model_torch(m, num_iter=30, verbose=False, objective="loo")
    hist = histories[0]
    print(f"{fixture}: loss {hist[0]:.6f} -> {hist[-1]:.6f} in {len(hist)} iterations")
    assert len(hist) == 30 and hist[-1] < hist[0] and best == hist[-1]
    assert fit_model_torch.last_graph is None  # the eager evaluation, no replayed graph
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_scipy_driver_and_model_fit_accept_the_loo_objective(gpu_ctx):
    from gpplus_amd.optim import MLLObjective, fit_model_scipy

    fx = _load("c3_borehole_mixed_n100.npz")
    m = _build(fx, "theta1", qual_dict={0: 5, 5: 5})
    obj = MLLObjective(m, True, [0, 0], objective="loo")
    theta = obj.pack_parameters()
    f0, g0 = obj.fun(theta)
    assert obj._graphed() is None and np.isfinite(f0) and np.all(np.isfinite(g0))
    res, best = fit_model_scipy(m, num_restarts=-1, theta0_list=[theta], options={"maxiter": 5}, objective="loo")
    print(f"scipy, objective=loo: {f0:.6f} -> {best:.6f}")
    assert best < f0

"""Grouped cross-validation on the HIP path (linalg.exact_cv / cv_moments: gpp_cv_blocks, the batched fold solves, gpp_cv_rows, the
TN GEMM, gpp_loo_grad_reduce) against the dense fp64 CPU reference of tests/cv_reference.py — delete-fold conditioning, which shares
nothing with the identity the library uses — and the public interface on top of it.

Tolerances are the project's (as in test_gpu_loo.py): 1e-5 relative for the value, 1e-5 of max|g| per gradient
vector.  Every test prints its observed errors before asserting (pytest -s shows them).

The reference is ``cv_autograd`` (delete-fold conditioning) in every case and fold structure but one: singleton folds at N = 1537,
where autograd would keep 1537 factorisations of 1536 x 1536 matrices alive.  That one case uses ``loo_reference.loo_autograd``
instead — the leave-one-out formula through ``torch.linalg.inv``, i.e. the m = 1 form of the identity under test and NOT independent
of it; tests/test_cv_host.py holds its value and every gradient against ``cv_autograd`` with singleton folds at N = 60 (1e-10).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cv_reference import (closed_form_grads, cv_autograd, cv_closed_form, cv_dense, cv_moments_dense,  # noqa: E402
                          folds_from_labels)
from loo_reference import KIND_MATERN52, KIND_RBF, _kernel, _noise, loo_autograd, make_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-5

# (N, D, kind, d_split, S, dU)
CASES = [
    (63, 3, KIND_RBF, 0, 1, 0),
    (65, 8, KIND_MATERN52, 3, 3, 2),
    (333, 20, KIND_RBF, 0, 3, 2),
    (1537, 8, KIND_RBF, 0, 3, 0),
]
STRUCTURES = ("kfold5", "ragged", "singletons")


def _labels(N, structure):
    """The three fold structures of a case, as one integer label per row."""
    if structure == "singletons":
        return np.arange(N)
    if structure == "kfold5":
        from gpplus_amd.cv import FoldIndex
        fi = FoldIndex(5, N, seed=N)
        labels = np.empty(N, dtype=np.int64)
        for f in range(fi.nfolds):
            labels[fi.fold(f)] = f
        return labels
    # ragged: sizes from 1 to about N / 3 (a singleton, a pair, sizes on both sides of the 32 / 128 / 512 bucket edges as N allows)
    sizes = [s for s in (1, 2, 5, N // 10, N // 5, N // 3) if s > 0]
    rest = N - sum(sizes)
    sizes += [rest // 2, rest - rest // 2] if rest > N // 3 else [rest]
    sizes = [s for s in sizes if s > 0]
    assert sum(sizes) == N
    return np.random.default_rng(N).permutation(np.repeat(np.arange(len(sizes)), sizes))


@functools.lru_cache(maxsize=None)
def _reference(N, D, kind, d_split, S, structure):
    """Inputs, labels and the autograd reference of one case, computed once and shared (read-only)."""
    inp = make_inputs(N, D, seed=1000 + N + D, S=S)
    labels = _labels(N, structure)
    if structure == "singletons" and N > 333:  # (1537 only: see the module docstring)
        val, grads = loo_autograd(**inp, kind=kind, d_split=d_split)
    else:
        val, grads = cv_autograd(**inp, folds=folds_from_labels(labels), kind=kind, d_split=d_split)
    return inp, labels, val, grads


def _evaluate(inp, folds, kind, d_split, dU, need_grad=True, fn="cv"):
    """One evaluation on the GPU: (value, gradients as CPU tensors)."""
    from gpplus_amd.linalg import KernelSpec, exact_cv, exact_loo, exact_mll

    leaves = {k: inp[k].to("cuda").requires_grad_(need_grad) for k in ("U", "w", "sf2", "tau", "mean", "y")}
    grp = None if inp["grp"] is None else inp["grp"].to("cuda")
    spec = KernelSpec(leaves["w"], leaves["sf2"], kind, d_split)
    if fn == "cv":
        val = exact_cv(leaves["U"], spec, leaves["tau"], leaves["mean"], leaves["y"], folds, grp, n_grad_dims=dU)
    else:
        val = (exact_loo if fn == "loo" else exact_mll)(leaves["U"], spec, leaves["tau"], leaves["mean"], leaves["y"], grp,
                                                       n_grad_dims=dU)
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


@pytest.mark.parametrize("structure", STRUCTURES)
@pytest.mark.parametrize("N,D,kind,d_split,S,dU", CASES)
def test_exact_cv_matches_autograd(gpu_ctx, N, D, kind, d_split, S, dU, structure):
    inp, labels, ref_val, ref_grads = _reference(N, D, kind, d_split, S, structure)
    val, grads = _evaluate(inp, labels, kind, d_split, dU)
    _check(val, grads, ref_val, ref_grads, dU, f"N={N} D={D} kind={kind} S={S} dU={dU} {structure}")
    # bitwise repeatable, and the value does not depend on whether a gradient was asked for
    val2, grads2 = _evaluate(inp, labels, kind, d_split, dU)
    assert torch.equal(val, val2)
    for name in grads:
        assert torch.equal(grads[name], grads2[name]), name
    val3, _ = _evaluate(inp, labels, kind, d_split, dU, need_grad=False)
    assert torch.equal(val, val3)


@pytest.mark.parametrize("N,D,kind,d_split,S,dU", CASES)
def test_exact_cv_limits_are_loo_and_mll(gpu_ctx, N, D, kind, d_split, S, dU):
    """Folds of one point give the leave-one-out value, one fold of everything the marginal likelihood: 1e-10 relative."""
    inp = make_inputs(N, D, seed=1000 + N + D, S=S)
    single, _ = _evaluate(inp, np.arange(N), kind, d_split, dU, need_grad=False)
    loo, _ = _evaluate(inp, None, kind, d_split, dU, need_grad=False, fn="loo")
    e_loo = abs(single.item() - loo.item()) / abs(loo.item())
    whole, _ = _evaluate(inp, 1, kind, d_split, dU, need_grad=False)
    mll, _ = _evaluate(inp, None, kind, d_split, dU, need_grad=False, fn="mll")
    e_mll = abs(whole.item() - mll.item()) / abs(mll.item())
    print(f"N={N}: singletons against exact_loo {e_loo:.2e}, one fold against exact_mll {e_mll:.2e}")
    assert e_loo <= 1e-10 and e_mll <= 1e-10


def test_exact_cv_large_matches_closed_form(gpu_ctx):
    """N = 5200 with 4 folds of 1300: the 2048 bucket, the batched factorisation beyond one leaf, 128-wide LAUUM tiles and the
    look-ahead outer factorisation; the reference is the closed form through P (4 delete-fold solves of 3900 points under autograd are
    too slow), which tests/test_cv_host.py holds against delete-fold conditioning."""
    N, D = 5200, 8
    inp = make_inputs(N, D, seed=5200, S=3)
    labels = np.random.default_rng(5200).permutation(np.repeat(np.arange(4), 1300))
    K, _ = _kernel(inp["U"], inp["w"], inp["sf2"], KIND_RBF, 0)
    Ky = K + torch.diag(_noise(inp["tau"], inp["grp"], N))
    ref_val, W, beta = cv_closed_form(Ky.numpy(), (inp["y"] - inp["mean"]).numpy(), folds_from_labels(labels))
    ref_grads = closed_form_grads(inp["U"].numpy(), inp["w"].numpy(), inp["sf2"].item(), inp["tau"].numpy(), inp["grp"].numpy(), W, beta)
    val, grads = _evaluate(inp, labels, KIND_RBF, 0, 0)
    _check(val, grads, torch.tensor(ref_val), ref_grads, 0, f"N={N} D={D} 4x1300")


def test_not_positive_definite_fold_block_names_the_fold(gpu_ctx):
    """A fold block that does not factor raises NotPSDError naming the fold (no jitter retry on a fold block), through the real
    sequence: gpp_cv_blocks on an inverse-factor buffer whose rows 2, 3, 4 are zero gives fold 1 the block P_FF = 0, the batched
    factorisation reports its first pivot, and ``cv_moments`` raises.  The same folds on a sound buffer raise nothing."""
    from types import SimpleNamespace

    from gpplus_amd.backend import square_buffer
    from gpplus_amd.cv import FoldIndex, check_infos, fold_solves
    from gpplus_amd.errors import NotPSDError
    from gpplus_amd.linalg import cv_moments

    N = 6
    fi = FoldIndex(np.array([4, 4, 9, 9, 9, 4]), N)
    Li = square_buffer(N, "cuda")
    Li.copy_(torch.eye(N, dtype=torch.float64) * 2.0)
    alpha = torch.arange(1.0, N + 1.0, dtype=torch.float64, device="cuda")
    cache = SimpleNamespace(gctx=gpu_ctx, Linv=Li, alpha=alpha, U=torch.zeros(N, 1, device="cuda"), refresh=lambda: None)
    mu, s2 = cv_moments(cache, torch.zeros(N, dtype=torch.float64), fi)  # P = 4 I: mu = y - alpha / 4, s2 = 1 / 4
    assert torch.allclose(s2.cpu(), torch.full((N,), 0.25, dtype=torch.float64), rtol=1e-14)
    assert torch.allclose(mu.cpu(), -alpha.cpu() / 4.0, rtol=1e-14)
    Li[2:5].zero_()
    _, _, _, infos, _ = fold_solves(gpu_ctx, Li, alpha, fi)
    assert [int(v) for _, info in infos for v in info.cpu()] == [0, 1]  # fold 1: leading minor 1
    with pytest.raises(NotPSDError, match=r"fold 1 \(label 9, 3 rows\)"):
        check_infos(infos, fi)
    with pytest.raises(NotPSDError, match=r"fold 1 \(label 9, 3 rows\)"):
        cv_moments(cache, torch.zeros(N, dtype=torch.float64), fi)


# ---- the model-level interface ----------------------------------------------------------------------------------------------------
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


def _dense_of(m):
    m.train()
    with torch.no_grad():
        out = m.likelihood(m(*m.train_inputs))
        return out.covariance_matrix.cpu().to(torch.float64), out.mean.cpu().to(torch.float64)


def _check_cv_predict(m, folds_arg, label):
    from gpplus_amd.cv import FoldIndex

    N = m.train_targets.shape[0]
    Ky, mean = _dense_of(m)
    y = m.train_targets.cpu().to(torch.float64)
    fi = FoldIndex.make(folds_arg, N)
    mu_r, s2_r = cv_moments_dense(Ky, y - mean, [fi.fold(f) for f in range(fi.nfolds)])
    y_min, y_std = m.y_min.cpu().to(torch.float64), m.y_std.cpu().to(torch.float64)
    mu_ref, sd_ref = y_min + y_std * (mean + mu_r), s2_r.sqrt() * y_std.abs()
    mu, sd_ = m.cv_predict(fi)
    assert mu.shape == (N,) and sd_.shape == (N,)
    e_mu = (mu.cpu() - mu_ref).abs().max().item() / mu_ref.abs().max().item()
    e_sd = (sd_.cpu() - sd_ref).abs().max().item() / sd_ref.abs().max().item()
    print(f"cv_predict {label}: {fi.nfolds} folds, sizes {int(fi.sizes.min())}..{int(fi.sizes.max())}: mean rel err {e_mu:.2e}, "
          f"std rel err {e_sd:.2e}")
    assert e_mu <= RTOL and e_sd <= RTOL
    # from the cache: asking again factors nothing and gives the same bits
    cache = m._ensure_prediction_cache()
    epoch = cache._ws.epoch
    mu2, sd2 = m.cv_predict(fi)
    assert torch.equal(mu, mu2) and torch.equal(sd_, sd2) and cache._ws.epoch == epoch
    assert torch.equal(m.cv_predict(fi, return_std=False), mu)


def test_cv_predict_against_delete_fold_solves(gpu_ctx):
    """The borehole fixture's first 65 rows, 5 folds: GP_Plus.cv_predict() against explicit dense solves with each fold removed."""
    from gpplus_amd.models import GP_Plus

    fx = _load("c1_borehole_n500.npz")
    N = 65
    m = GP_Plus(torch.tensor(fx["Xtrain"][:N]), torch.tensor(fx["ytrain"][:N]), dtype=torch.float64, device="cuda")
    sd = m.state_dict()
    for k, v in {"covar_module.base_kernel.raw_lengthscale": -1.0, "covar_module.raw_outputscale": 0.3,
                 "likelihood.noise_covar.raw_noise": -6.0, "mean_module.constant": 0.4}.items():
        sd[k] = torch.full_like(sd[k], v)
    m.load_state_dict(sd)
    _check_cv_predict(m, 5, "c1[:65] 5-fold")
    # an int k draws its partition from the generator: the same seed, the same folds
    g1, g2 = torch.Generator(), torch.Generator()
    g1.manual_seed(11), g2.manual_seed(11)
    assert torch.equal(m.cv_predict(5, generator=g1)[0], m.cv_predict(5, generator=g2)[0])


def test_cv_predict_leave_one_level_combination_out(gpu_ctx):
    from gpplus_amd.cv import group_labels

    fx = _load("c3_borehole_mixed_n100.npz")
    m = _build(fx, "theta1", qual_dict={0: 5, 5: 5})
    _check_cv_predict(m, group_labels(fx["Utrain"], [0, 5]), "c3 level combinations")


def test_cv_predict_leave_one_source_out(gpu_ctx):
    from gpplus_amd.cv import group_labels

    fx = _load("c4_wing_mf_n300.npz")
    m = _build(fx, "theta1", qual_dict={10: 3}, multiple_noise=True, m_gp="multiple_constant")
    _check_cv_predict(m, group_labels(fx["Xtrain"], [10]), "c4 sources")


MODEL_CASES = [
    ("c3_borehole_mixed_n100.npz", {"qual_dict": {0: 5, 5: 5}}, [0, 5]),
    ("c4_wing_mf_n300.npz", {"qual_dict": {10: 3}, "multiple_noise": True, "m_gp": "multiple_constant"}, [10]),
]


def _objective(m, cv):
    return cv(m(*m.train_inputs), m.train_targets)


@pytest.mark.parametrize("fixture,kw,cols", MODEL_CASES)
def test_model_objective_value_and_directional_derivative(gpu_ctx, fixture, kw, cols):
    """Manifold (categorical inputs through a latent map: feature gradients) and multiple noise levels, folds = the level
    combinations / the sources: the objective's value against the reference on the model's own dense covariance, and a central
    difference along the gradient direction (the construction and tolerance of the leave-one-out test)."""
    from gpplus_amd.cv import FoldIndex, group_labels
    from gpplus_amd.gpcore import CrossValidationPseudoLikelihood

    fx = _load(fixture)
    m = _build(fx, "theta1", **kw)
    m.train()
    N = m.train_targets.shape[0]
    fi = FoldIndex(group_labels(fx["Xtrain" if "Xtrain" in fx else "Utrain"], cols), N)
    cv = CrossValidationPseudoLikelihood(m.likelihood, m, fi)
    Ky, mean = _dense_of(m)
    with torch.no_grad():
        prior = cv._prior_sum(torch.float64)
        prior = 0.0 if prior is None else prior.item()
    ref = (cv_dense(Ky, m.train_targets.cpu().to(torch.float64) - mean, [fi.fold(f) for f in range(fi.nfolds)]).item() + prior) / N
    params = [p for p in m.parameters() if p.requires_grad]
    for p in params:
        p.grad = None
    val = _objective(m, cv)
    val.backward()
    err = abs(val.item() - ref) / abs(ref)
    print(f"{fixture}: {fi.nfolds} folds: objective {val.item():.12f} ref {ref:.12f} rel err {err:.2e}")
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
            return _objective(m, cv).item()

    fd = (at(eps) - at(-eps)) / (2 * eps) * g.norm().item()
    at(0.0)
    e = abs(fd - gg) / gg
    print(f"{fixture}: central difference along g: {fd:.10e} against g.g {gg:.10e} (rel {e:.2e})")
    assert e <= RTOL


@pytest.mark.parametrize("fixture,kw,cols", MODEL_CASES)
def test_fit_model_torch_with_the_cv_objective(gpu_ctx, fixture, kw, cols):
    from gpplus_amd.cv import group_labels
    from gpplus_amd.optim import fit_model_torch

    fx = _load(fixture)
    m = _build(fx, "theta1", **kw)
    labels = group_labels(fx["Xtrain" if "Xtrain" in fx else "Utrain"], cols)
    best, histories = fit_model_torch(m, num_iter=12, verbose=False, objective="cv", folds=labels)
    hist = histories[0]
    print(f"{fixture}: loss {hist[0]:.6f} -> {hist[-1]:.6f} in {len(hist)} iterations")
    assert len(hist) == 12 and hist[-1] < hist[0] and best == hist[-1]
    assert fit_model_torch.last_graph is None  # the eager evaluation, no replayed graph
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_scipy_driver_and_model_fit_accept_the_cv_objective(gpu_ctx):
    from gpplus_amd.optim import MLLObjective, fit_model_scipy, fit_model_torch, fit_model_torch_batched

    fx = _load("c3_borehole_mixed_n100.npz")
    m = _build(fx, "theta1", qual_dict={0: 5, 5: 5})
    obj = MLLObjective(m, True, [0, 0], objective="cv", folds=5)
    theta = obj.pack_parameters()
    f0, g0 = obj.fun(theta)
    assert obj._graphed() is None and np.isfinite(f0) and np.all(np.isfinite(g0))
    res, best = fit_model_scipy(m, num_restarts=-1, theta0_list=[theta], options={"maxiter": 5}, objective="cv", folds=5)
    print(f"scipy, objective=cv: {f0:.6f} -> {best:.6f}")
    assert np.isfinite(best) and best < f0
    # GP_Plus.fit: always the sequential, eager route (here the 4 restarts of a non-Adam optim_type, 5 x 100 evaluations)
    m = _build(fx, "theta1", qual_dict={0: 5, 5: 5})
    fit_model_torch_batched.last_graph = "untouched"
    with pytest.warns(UserWarning, match="adam_torch"):
        best, histories = m.fit(objective="cv", folds=5)
    print(f"GP_Plus.fit, objective=cv: {len(histories)} runs, best {best:.6f}")
    assert len(histories) == 5 and np.isfinite(best) and all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert fit_model_torch.last_graph is None and fit_model_torch_batched.last_graph == "untouched"
    # the batched driver hands "cv" to the sequential one
    m = _build(fx, "theta1", qual_dict={0: 5, 5: 5})
    best_b, hist_b = fit_model_torch_batched(m, num_iter=3, num_restarts=1, objective="cv", folds=5)
    assert len(hist_b) == 2 and np.isfinite(best_b) and fit_model_torch_batched.last_graph == "untouched"


def test_default_fit_still_takes_the_batched_route(gpu_ctx):
    """GP_Plus.fit() with the default objective: 65 restarts advancing together, the step replayed as a graph — as before."""
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim import fit_model_torch, fit_model_torch_batched
    from gpplus_amd.utils import set_seed

    fx = _load("c3_borehole_mixed_n100.npz")
    set_seed(2)
    m = GP_Plus(torch.tensor(fx["Utrain"]), torch.tensor(fx["ytrain"]), qual_dict={0: 5, 5: 5}, dtype=torch.float64, device="cuda")
    fit_model_torch_batched.last_graph = fit_model_torch.last_graph = "untouched"
    best, histories = m.fit(optim_type="adam_torch")
    g = fit_model_torch_batched.last_graph
    assert len(histories) == 65 and np.isfinite(best)
    assert g is not None and g != "untouched" and g.replays > 0  # the batched driver ran, its step replayed as a graph
    assert fit_model_torch.last_graph == "untouched"             # ... and the sequential one did not

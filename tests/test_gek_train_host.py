"""Training on gradient observations without a GPU: the closed-form blocks of tests/gek_train_reference.py against the long-double
``gek_reference.d2k`` and the autograd Jacobian ``gek_reference._dk`` on every fixture case, its autograd gradient against central
differences of its own value (the floor of the GPU comparison, printed), its value against the joint matrix of
``gek_reference.gek_posterior``, the reference's own L-BFGS-B run on the fit of tests/test_gpu_gek_train.py, the drivers' argument
errors (raised before a device is touched) and the new symbol's declarations."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_reference as G  # noqa: E402
import gek_train_reference as T  # noqa: E402
import gradpost_reference as gr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = G.gek_case(name)
    return _cases[name]


@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_blocks_equal_the_long_double_closed_form_and_the_autograd_jacobian(name):
    """Three evaluations of smooth functions at O(1) separations, fp64 or better: held to 1e-11 of the largest entry."""
    o, X, y, kw, xg, dY, noise, xt = _case(name)
    w, sf2, kind, d_split, d0, nd = G.oracle_spec(o)
    with torch.no_grad():
        U, Ug = o.features(o.train_x), o.features(xg)
        wt, st, kind_t, ds_t, d0_t, nd_t = T.spec_tensors(o)
        assert (kind_t, ds_t, d0_t, nd_t) == (kind, d_split, d0, nd) and np.allclose(wt.numpy(), w, rtol=1e-15, atol=0)
        Kfg, Kgg = T.blocks(U, Ug, wt, st, kind, d_split, d0, nd)
    ref_gg = torch.tensor(G.d2k(Ug.numpy(), Ug.numpy(), w, sf2, kind, d_split, d0, nd).astype(np.float64))
    ref_fg = G._dk(o, xg, U)
    for what, got, ref in (("Kgg", Kgg, ref_gg), ("Kfg", Kfg, ref_fg)):
        err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
        print(f"{name} {what}: {err:.3e} of max {scale:.3e}")
        assert got.shape == ref.shape and err <= 1e-11 * scale


@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_value_equals_the_log_density_of_the_posteriors_joint_matrix(name):
    o, X, y, kw, xg, dY, noise, xt = _case(name)
    with torch.no_grad():
        got = T.gek_mll(o, xg, dY, noise).item()
        p, Mg = len(o.quant_index), xg.shape[0]
        m_tr, K_tr = o.forward(o.train_x)
        Kff = K_tr + torch.diag(o.noise_vector(o.train_x))
        Kfg = G._dk(o, xg, o.features(o.train_x))
        Kgg = G._d2k_t(o, xg, xg) + torch.diag((noise / float(o.y_std) ** 2).expand(Mg, p).reshape(-1))
        S = torch.cat([torch.cat([Kff, Kfg], 1), torch.cat([Kfg.T, Kgg], 1)], 0)
        r = torch.cat([o.y_sc - m_tr, (dY / float(o.y_std)).reshape(-1)])
        n = r.numel()
        ref = (-0.5 * r @ torch.linalg.solve(S, r) - 0.5 * torch.linalg.slogdet(S)[1] - 0.5 * n * math.log(2 * math.pi)).item()
    print(f"{name}: value {got:.12e} against {ref:.12e}: rel {abs(got - ref) / abs(ref):.2e}")
    assert abs(got - ref) <= 1e-9 * abs(ref)


@pytest.mark.parametrize("noise_given", [True, False])
@pytest.mark.parametrize("name", ["c3", "c1-matern52", "c1-matern32"])
def test_gradient_matches_central_differences_of_its_own_value(name, noise_given):
    """The floor of the GPU comparison: autograd against central differences (step 1e-5, truncation ~1e-10 relative) on the first
    entries of every parameter tensor, held to 1e-6 of the largest gradient entry — the bar the GPU test uses — and printed."""
    from gpplus_amd.gradient_enhanced import GRADIENT_NUGGET_REL

    o, X, y, kw, xg, dY, noise, xt = _case(name)
    nz, rel = (noise, None) if noise_given else (None, GRADIENT_NUGGET_REL)
    _, grads = T.gek_loss_and_grad(o, xg, dY, nz, rel)
    h, worst = 1e-5, 0.0
    for k, g in grads.items():
        scale = g.abs().max().item()
        flat = o.params[k].reshape(-1)
        for i in range(min(3, flat.numel())):
            vals = []
            for s in (+1, -1):
                p = {kk: v.clone() for kk, v in o.params.items()}
                p[k].reshape(-1)[i] += s * h
                with torch.no_grad():
                    vals.append(T.gek_loss(o, xg, dY, nz, p, rel).item())
            fd = (vals[0] - vals[1]) / (2 * h)
            err = abs(fd - g.reshape(-1)[i].item())
            worst = max(worst, err / max(scale, 1e-300))
            assert err <= 1e-6 * scale + 1e-9, (k, i, fd, g.reshape(-1)[i].item())
    print(f"{name} noise_given={noise_given}: largest |central - autograd| / max|grad| over the probed entries: {worst:.2e}")


def test_block_sums_are_the_gradient_of_the_weighted_sum():
    """``block_sums`` with W = the all-ones matrix differentiates 2 sum(Kfg) + sum(Kgg): checked by central differences in w."""
    rng = np.random.default_rng(5)
    for kind, d_split in ((0, 0), (1, 2), (2, 2)):
        U, Ug = torch.tensor(rng.standard_normal((7, 5))), torch.tensor(rng.standard_normal((3, 5)))
        Ug[1] = U[2]  # a coincident pair
        w, sf2 = torch.tensor(rng.uniform(0.2, 1.0, 5)), torch.tensor(0.8, dtype=torch.float64)
        n = 7 + 3 * 3
        W = torch.ones(n, n, dtype=torch.float64)
        g_w, g_s, g_U, g_Ug = T.block_sums(U, Ug, w, sf2, kind, d_split, 2, 3, W, 2)
        assert all(bool(torch.isfinite(t).all()) for t in (g_w, g_s, g_U, g_Ug)) and g_U.shape == (7, 2) and g_Ug.shape == (3, 2)

        def total(wv):
            a, b = T.blocks(U, Ug, wv, sf2, kind, d_split, 2, 3)
            return (2 * a.sum() + b.sum()).item()

        for d in range(5):
            e = torch.zeros(5, dtype=torch.float64)
            e[d] = 1e-6
            fd = (total(w + e) - total(w - e)) / 2e-6
            assert abs(fd - g_w[d].item()) <= 1e-6 * g_w.abs().max().item(), (kind, d, fd, g_w[d].item())


def test_the_references_own_fit_rises():
    """What tests/test_gpu_gek_train.py asks of ``fit_model_scipy(objective="gek")`` holds for the reference alone: its own L-BFGS-B
    run from the same start lowers the (negative) objective."""
    o, X, y, xg, dY, noise = T.fit_case()
    start, res = T.fit_lbfgs(o, xg, dY, noise)
    print(f"reference: objective {start:.6f} -> {res.fun:.6f} in {res.nit} iterations")
    assert res.fun < start - 1e-3 * abs(start)


def _cpu_model():
    from gpplus_amd.models import GP_Plus

    fx = gr.load_fixture("c3_borehole_mixed_n100.npz")
    X, y = gr.fixture_xy(fx, 30)
    return GP_Plus(torch.tensor(X), torch.tensor(y), dtype=torch.float64, device="cpu", qual_dict={0: 5, 5: 5}), \
        gr.fixture_test_rows(fx, 3)


def test_driver_argument_errors_need_no_gpu():
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood
    from gpplus_amd.optim import fit_model_scipy, fit_model_torch, fit_model_torch_batched
    from gpplus_amd.optim.mll_torch import GRADIENT_OBJECTIVES, check_objective, check_objective_gradients

    assert GRADIENT_OBJECTIVES == ("gek",) and check_objective("gek") == "gek"
    with pytest.raises(ValueError, match="gek"):
        check_objective("gke")
    m, xg = _cpu_model()
    p = int(m.quant_index.numel())
    dY = torch.ones(xg.shape[0], p, dtype=torch.float64)
    for fit in (fit_model_torch, fit_model_scipy, fit_model_torch_batched, m.fit):
        with pytest.raises(ValueError, match="gek"):
            fit(objective="mll", gradients=(xg, dY)) if fit == m.fit else fit(m, objective="mll", gradients=(xg, dY))
        with pytest.raises(ValueError, match="gradients"):
            fit(objective="gek") if fit == m.fit else fit(m, objective="gek")
    with pytest.raises(ValueError):
        check_objective_gradients("gek", (xg,))
    assert check_objective_gradients("gek", (xg, dY)) == (xg, dY, None) and check_objective_gradients("mll", None) is None
    nan = dY.clone()
    nan[0, 0] = float("nan")
    bad_level = xg.clone()
    bad_level[0, 5] = 9.0
    for what, args in {"columns": (xg[:, :-1], dY), "dY shape": (xg, dY[:, :-1]), "rows": (xg, dY[:1]), "empty": (xg[:0], dY[:0]),
                       "nan": (xg, nan), "level": (bad_level, dY), "negative noise": (xg, dY, -1.0)}.items():
        with pytest.raises(ValueError):
            GradientEnhancedMarginalLogLikelihood(m.likelihood, m, *args)
        with pytest.raises(ValueError):
            fit_model_scipy(m, objective="gek", gradients=args)
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, 0.5)
    assert mll.r_g.shape == (xg.shape[0], p) and mll.noise.shape == (xg.shape[0], p) and mll.num_directions == p
    assert torch.allclose(mll.noise, torch.full_like(mll.noise, 0.5) / m.y_std.double() ** 2)


def test_symbol_is_declared_exported_and_bound():
    from gpplus_amd import _lib, backend, linalg

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_gek_grad_reduce\s*\(", header) and "GPP_OP_GEK_GRAD 9" in header
    assert "gpp_gek_grad_reduce" in _lib.exported_symbols() and len(_lib._SIGNATURES["gpp_gek_grad_reduce"][1]) == 20
    lib = _lib.load()
    assert lib.gpp_gek_grad_reduce.argtypes == _lib._SIGNATURES["gpp_gek_grad_reduce"][1]
    assert callable(backend.GppContext.gek_grad_reduce) and callable(linalg.ExactGEKFunction.apply) and callable(linalg.exact_gek_mll)
    assert lib.gpp_gek_grad_reduce(*([None] * 2), 0, None, 0, 0, None, None, 0, 0, 0, 0, None, None, 0, 0, None, None, None, None) == -1
    # the workspace query grows with every extent and is 0 for an empty problem
    q = lambda *a: int(lib.gpp_workspace_bytes(None, backend.OP_GEK_GRAD, *a))  # noqa: E731
    assert q(100, 10, 5, 2) > q(100, 10, 5, 0) > 256 and q(200, 10, 5, 0) > q(100, 10, 5, 0) and q(0, 0, 5, 0) == 256

"""Conditioning on gradient observations without a GPU: the long-double closed form of d^2 k / du dv (tests/gek_reference.py) against
torch double-backward autograd of the oracle's kernel and against its stated limits at coincident points, the dense reference by
joint Cholesky against the same posterior by the Schur complement on every fixture case of tests/test_gpu_gek.py (the floor of the
GPU comparison, printed), the argument errors of ``condition_on_gradients`` on a CPU model (raised before a device is touched), the
refusals of the linalg entries and the new symbols' declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_reference as G  # noqa: E402
import gradpost_reference as gr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KCLASSES = ["Rough_RBF", "Matern32Kernel", "Matern52Kernel"]


def _small_oracle(kclass, mixed):
    """An oracle on random rows: three quantitative columns, behind one categorical column (a 2-d latent map: d_split = 2) if ``mixed``."""
    from oracle.gp_oracle import OracleGP

    rng = np.random.default_rng(3 + len(kclass) + mixed)
    Xq = rng.standard_normal((20, 3))
    if mixed:
        X = np.concatenate([rng.integers(0, 3, (20, 1)).astype(np.float64), Xq], 1)
        o = OracleGP(X, rng.standard_normal(20), qual_dict={0: 3}, quant_correlation_class=kclass)
    else:
        o = OracleGP(Xq, rng.standard_normal(20), quant_correlation_class=kclass)
    o.params[o.ls_key] = torch.tensor(rng.uniform(-1.0, 0.5, (1, 3)))
    o.params["covar_module.raw_outputscale"] = torch.tensor(0.7, dtype=torch.float64)
    return o, rng


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kclass", KCLASSES)
def test_closed_form_matches_double_backward_of_the_oracle_kernel(kclass, mixed):
    """Both sides are fp64-or-better evaluations of a smooth function at O(1) separations: held to 1e-11 of the largest entry."""
    o, rng = _small_oracle(kclass, mixed)
    w, sf2, kind, d_split, d0, nd = G.oracle_spec(o)
    assert (d0, nd, d_split) == ((2, 3, 2) if mixed else (0, 3, 0)) and kind == KCLASSES.index(kclass)
    D = d0 + nd
    Ua = torch.tensor(rng.standard_normal((3, D)), requires_grad=True)
    Ub = torch.tensor(rng.standard_normal((4, D)), requires_grad=True)
    K = o.prior_cov(Ua, Ub)
    H = np.zeros((3, nd, 4, nd))
    for a in range(3):
        for b in range(4):
            ga, = torch.autograd.grad(K[a, b], Ua, create_graph=True)
            for j in range(nd):
                gb, = torch.autograd.grad(ga[a, d0 + j], Ub, retain_graph=True)
                H[a, j, b, :] = gb[b, d0:].numpy()
    ref = G.d2k(Ua.detach().numpy(), Ub.detach().numpy(), w, sf2, kind, d_split, d0, nd).astype(np.float64)
    err = np.abs(ref - H.reshape(3 * nd, 4 * nd)).max()
    print(f"{kclass} mixed={mixed}: closed form against double backward: {err:.3e} of max {np.abs(ref).max():.3e}")
    assert err <= 1e-11 * np.abs(ref).max()
    # k(u, v) = k(v, u): the block of (Ub, Ua) is the transpose
    back = G.d2k(Ub.detach().numpy(), Ua.detach().numpy(), w, sf2, kind, d_split, d0, nd)
    assert np.abs(back.T - G.d2k(Ua.detach().numpy(), Ub.detach().numpy(), w, sf2, kind, d_split, d0, nd)).max() <= 1e-17


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kclass", KCLASSES)
def test_coincident_pairs_meet_the_stated_limits(kclass, mixed):
    from gpplus_amd.linalg import KernelSpec, gradient_prior_curvature

    o, rng = _small_oracle(kclass, mixed)
    w, sf2, kind, d_split, d0, nd = G.oracle_spec(o)
    u = rng.standard_normal((1, d0 + nd))
    H = G.d2k(u, u.copy(), w, sf2, kind, d_split, d0, nd).astype(np.float64)
    kap = gr.kappa(o).detach().numpy()
    assert np.allclose(np.diag(H), kap, rtol=1e-14, atol=0) and (H - np.diag(np.diag(H)) == 0).all()
    spec = KernelSpec(torch.tensor(w), torch.tensor(sf2, dtype=torch.float64), kind, d_split)
    assert np.allclose(gradient_prior_curvature(spec, d0, nd).numpy(), np.diag(H), rtol=1e-14, atol=0)
    # towards the limit: finite and continuous.  With rho^2 = 10 sum_d w_d delta_d^2 (>= r^2 of either Matern kind, >= q1) every
    # multiplier differs from its value at rho = 0 by at most 2 rho of it for rho <= 1/2 (|1 - e^-x| <= x; h' and h'' of the Matern
    # factors have slopes <= their own size), and the product term is at most 4 w_j w_l |D_j D_l| sf2 |h''| <= 6 sqrt(w_j w_l) sf2 rho
    # (Matern 3/2, |sqrt(w) D| <= r / sqrt(6)) or 4 (25 / 3) sf2 w rho^2 / 10 otherwise: both sides within 8 rho of the largest kappa.
    for eps in (1e-3, 1e-7, 1e-12, 1e-150):
        v = u + eps * np.linspace(1.0, 2.0, d0 + nd)[None, :]
        He = G.d2k(u, v, w, sf2, kind, d_split, d0, nd).astype(np.float64)
        assert np.isfinite(He).all()
        rho = np.sqrt(10 * (w * (u - v)[0] ** 2).sum())
        assert rho <= 0.5
        assert np.abs(He - np.diag(kap)).max() <= 8 * rho * kap.max() + 1e-15 * kap.max()


@pytest.mark.parametrize("name", list(G.GEK_CASES))
def test_joint_cholesky_and_schur_complement_agree(name):
    """The floor of tests/test_gpu_gek.py's comparison: the two dense routes to the same posterior must agree within 1e-8 of the
    largest reference magnitude at the noise the GPU test passes (``GEK_NOISE_REL``, 1e-4 of the prior curvature)."""
    o, X, y, kw, xg, dY, noise, xt = G.gek_case(name)
    a = G.gek_posterior(o, xg, dY, noise, xt, "joint")
    b = G.gek_posterior(o, xg, dY, noise, xt, "schur")
    base_mean = o.y_min + o.y_std * gr.posterior_mean(o, xt).detach()
    p = len(o.quant_index)
    assert a["gmean"].shape == (G.M_TEST, p) and xg.shape[0] * p <= min(X.shape[0], 2048)
    for key in a:
        rel = float((a[key] - b[key]).abs().max() / a[key].abs().max())
        print(f"{name} {key}: joint against Schur {rel:.3e} of max|reference| (noise = {G.GEK_NOISE_REL[name]:g} x curvature)")
        assert rel <= 1e-8, (name, key, rel)
    # the gradients carry information: the prediction moves, and no variance grows
    assert float((a["mean"] - base_mean).abs().max()) > 1e-6 * float(base_mean.abs().max())
    _, S0 = gr.gradient_posterior(o, xt)
    assert bool((a["gvar"] <= torch.diagonal(S0, dim1=1, dim2=2) * (1 + 1e-9) + 1e-12).all())
    # at the gradient points the gradient's posterior variance is at most the observation noise
    at = G.gek_posterior(o, xg, dY, noise, xg, "joint")
    assert bool((at["gvar"] <= noise[None, :] * (1 + 1e-9)).all())


def test_c4_low_fidelity_gradients_move_the_high_fidelity_prediction():
    o, X, y, kw, xg, dY, noise, xt = G.gek_case("c4")
    assert bool((xg[:, -1] != 0).all())
    hi = xt[xt[:, -1] == 0]
    assert hi.shape[0] >= 4
    got = G.gek_posterior(o, xg, dY, noise, hi, "joint")["mean"]
    base = o.y_min + o.y_std * gr.posterior_mean(o, hi).detach()
    assert float((got - base).abs().max()) > 1e-6 * float(base.abs().max())


def test_argument_errors_come_before_the_device_on_a_cpu_model():
    from gpplus_amd._lib import GppError
    from gpplus_amd.models import GP_Plus

    fx = gr.load_fixture("c3_borehole_mixed_n100.npz")
    X, y = torch.tensor(fx["Utrain"]), torch.tensor(fx["ytrain"])
    m = GP_Plus(X[:80], y[:80], qual_dict={0: 5, 5: 5}, dtype=torch.float64, device="cpu")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    good, dY = X[80:84], torch.ones(4, 6, dtype=torch.float64)
    bad_nan, bad_inf, bad_level, dy_nan = good.clone(), good.clone(), good.clone(), dY.clone()
    bad_nan[1, 2] = float("nan")
    bad_inf[0, 3] = float("inf")
    bad_level[2, 5] = 9.0
    dy_nan[3, 0] = float("nan")
    calls = {"columns": (good[:, :7], dY), "dY columns": (good, dY[:, :5]), "dY rows": (good, dY[:3]), "dY 1-d": (good, dY[:, 0]),
             "empty": (good[:0], dY[:0]), "nan": (bad_nan, dY), "inf": (bad_inf, dY), "dY nan": (good, dy_nan), "level": (bad_level, dY),
             "too many": (X[:14], torch.ones(14, 6, dtype=torch.float64))}  # 84 > N = 80
    for what, (rows, grads) in calls.items():
        with pytest.raises(ValueError, match="condition_on_gradients|not seen"):
            m.condition_on_gradients(rows, grads)
    for what, nz in {"negative": -1e-3, "negative entry": torch.tensor([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]), "nan": float("nan"),
                     "shape": torch.ones(3, 6)}.items():
        with pytest.raises(ValueError, match="noise"):
            m.condition_on_gradients(good, dY, noise=nz)
    # valid calls reach the device, and there is none
    for nz in (None, 0.0, 1e-3, torch.full((6,), 1e-3), torch.full((4, 1), 1e-3)):
        with pytest.raises(GppError, match="no CPU fallback"):
            m.condition_on_gradients(good, dY, noise=nz)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    # a source the model has not seen
    fx = gr.load_fixture("c4_wing_mf_n300.npz")
    X, y = torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"])
    keep = X[:, 10] != 2
    m = GP_Plus(X[keep], y[keep], qual_dict={10: 3}, multiple_noise=True, m_gp="multiple_constant", dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="not seen"):
        m.condition_on_gradients(X[~keep][:2], torch.ones(2, 10, dtype=torch.float64))
    # a model without a quantitative column
    rng = np.random.default_rng(2)
    Xc = torch.tensor(np.stack([rng.integers(0, 3, 40), rng.integers(0, 2, 40)], 1).astype(np.float64))
    mc = GP_Plus(Xc, torch.tensor(rng.standard_normal(40)), qual_dict={0: 3, 1: 2}, dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="no quantitative"):
        mc.condition_on_gradients(Xc[:5], torch.ones(5, 0, dtype=torch.float64))


def test_sharded_setting_is_refused_by_the_linalg_entries():
    from gpplus_amd import linalg, settings

    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            linalg.append_gradients_to_cache(None, None, 0, 1, None, None)
        with pytest.raises(NotImplementedError):
            linalg.predict_from_gradient_cache(None, None, "function")
    with pytest.raises(ValueError, match="want"):
        linalg.predict_from_gradient_cache(None, None, "cov")
    assert not issubclass(linalg.GradientFactorCache, linalg.FactorCache)


def test_symbols_are_declared_exported_and_bound():
    from gpplus_amd import _lib, backend, gradient_enhanced, linalg
    from gpplus_amd.models import GP_Plus

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_kernel_dxdx\s*\(", header)
    assert "gpp_kernel_dxdx" in _lib.exported_symbols() and len(_lib._SIGNATURES["gpp_kernel_dxdx"][1]) == 14
    lib = _lib.load()
    assert lib.gpp_kernel_dxdx.argtypes == _lib._SIGNATURES["gpp_kernel_dxdx"][1]
    assert callable(backend.GppContext.kernel_dxdx) and callable(GP_Plus.condition_on_gradients)
    assert callable(linalg.append_gradients_to_cache) and callable(linalg.predict_from_gradient_cache)
    assert gradient_enhanced.GRADIENT_NUGGET_REL == 1e-6 and "1e-6" in GP_Plus.condition_on_gradients.__doc__
    # a NULL handle is argument 1, before anything else is looked at
    assert lib.gpp_kernel_dxdx(None, None, 0, None, 0, 0, None, None, 0, 0, 0, 0, None, 0) == -1

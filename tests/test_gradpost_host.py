"""Posterior of the gradient without a GPU: the closed-form prior curvature kappa against second differences of the oracle's
kernel, the dense reference of tests/gradpost_reference.py against central differences of the oracle's posterior mean, the
reference covariance's symmetry and definiteness, the argument errors of ``predict_gradient`` / ``active_subspace`` on a CPU model
(raised before a device is touched), and the new symbols' declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradpost_reference as gr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"Rough_RBF": 0, "Matern32Kernel": 1, "Matern52Kernel": 2}


@pytest.mark.parametrize("kclass", list(KINDS))
def test_kappa_is_the_mixed_second_difference_of_the_kernel(kclass):
    """d^2 k / du_j du'_j at u' = u by the four-point central difference with step h in both arguments, which for a stationary
    kernel is (2 k(0) - 2 k(2 h e_j)) / (4 h^2).  With delta = 2 h and k = sf2 (1 - kappa delta^2 / (2 sf2) + ...) the next terms of the
    series give the difference's relative truncation error: w delta^2 / 2 = 2 w h^2 (RBF: exp(-w delta^2)), r^2 / 4 = 10 w h^2
    (Matern 5/2: h(r) = 1 - r^2 / 6 + r^4 / 24 + O(r^5), r^2 = 10 w delta^2) and (2 / 3) r = (4 / 3) sqrt(6 w) h (Matern 3/2:
    h(r) = 1 - r^2 / 2 + r^3 / 3 - ..., r = sqrt(6 w) delta, first order only).  h = 1e-3 with w <= 10^0.5 keeps them below 7e-6,
    7e-5 and 6e-3.  Rounding: the kernel values carry ~1e-15 sf2, divided by 4 h^2 = 4e-6 and by kappa >= 0.2 sf2: ~1e-9.  The
    tolerance is twice the truncation term plus 1e-7."""
    from oracle.gp_oracle import OracleGP
    from gpplus_amd.linalg import KernelSpec, gradient_prior_curvature

    rng = np.random.default_rng(5)
    d = 3
    o = OracleGP(rng.standard_normal((20, d)), rng.standard_normal(20), quant_correlation_class=kclass)
    o.params[o.ls_key] = torch.tensor(rng.uniform(-1.0, 0.5, (1, d)))  # w = 10^raw in [0.1, 3.2]
    o.params["covar_module.raw_outputscale"] = torch.tensor(0.7, dtype=torch.float64)
    w = 0.5 / o.lengthscale().reshape(-1) ** 2
    sf2 = torch.nn.functional.softplus(o.params["covar_module.raw_outputscale"])
    kap = gr.kappa(o)
    spec = KernelSpec(w, sf2, KINDS[kclass], 0)
    assert torch.allclose(gradient_prior_curvature(spec, 0, d), kap, rtol=1e-14, atol=0)
    # the library's split: a leading RBF dimension in front of the Matern ones
    mixed = gradient_prior_curvature(KernelSpec(w, sf2, KINDS[kclass], 1), 0, d)
    assert torch.allclose(mixed[0], 2.0 * w[0] * sf2, rtol=1e-14) and torch.allclose(mixed[1:], kap[1:], rtol=1e-14)
    assert torch.equal(gradient_prior_curvature(spec, 1, 2), gradient_prior_curvature(spec, 0, d)[1:])
    h = 1e-3
    u = torch.tensor(rng.standard_normal(d))
    for j in range(d):
        e = torch.zeros(d, dtype=torch.float64)
        e[j] = h
        pts = torch.stack([u + e, u - e])
        K = o.prior_cov(pts, pts.clone())
        second = (K[0, 0] - K[0, 1] - K[1, 0] + K[1, 1]) / (4 * h * h)
        wj = float(w[j])
        trunc = {0: 2 * wj * h * h, 2: 10 * wj * h * h, 1: (4.0 / 3.0) * np.sqrt(6 * wj) * h}[KINDS[kclass]]
        assert abs(float(second - kap[j])) <= (2 * trunc + 1e-7) * float(kap[j]), (kclass, j, float(second), float(kap[j]))


@pytest.fixture(scope="module")
def c3_reference():
    fx = gr.load_fixture("c3_borehole_mixed_n100.npz")
    o = gr.load_oracle(fx, qual_dict={0: 5, 5: 5})
    xt = gr.fixture_test_rows(fx, 12)
    g, S = gr.gradient_posterior(o, xt)
    return o, xt, g, S


def test_reference_mean_matches_central_differences_c3(c3_reference):
    """Central differences of the oracle's posterior mean with step h = 1e-4 of the inputs' O(1) range: truncation h^2 f''' / 6
    ~ 1e-8 of the slope's scale for a smooth posterior mean, rounding ~1e-15 / h = 1e-11.  Held to 1e-6 of the largest slope."""
    o, xt, g, _ = c3_reference
    h = 1e-4
    fd = torch.empty_like(g)
    with torch.no_grad():
        for j, c in enumerate(o.quant_index):
            e = torch.zeros(xt.shape[1], dtype=torch.float64)
            e[c] = h
            fd[:, j] = (gr.posterior_mean(o, xt + e) - gr.posterior_mean(o, xt - e)) / (2 * h) * o.y_std
    assert g.shape == (12, len(o.quant_index)) and len(o.quant_index) == xt.shape[1] - 2
    assert (g - fd).abs().max().item() <= 1e-6 * g.abs().max().item()


def test_reference_covariance_is_symmetric_psd(c3_reference):
    o, _, _, S = c3_reference
    assert torch.equal(S, S.transpose(1, 2))
    top = (gr.kappa(o) * o.y_std ** 2).max().item()
    assert torch.linalg.eigvalsh(S).min().item() >= -1e-10 * top
    # the data explain part of the prior variance, never more than all of it
    assert (torch.diagonal(S, dim1=1, dim2=2) <= gr.kappa(o) * o.y_std ** 2 * (1 + 1e-12)).all()
    A, mp, cp = gr.active_subspace(*c3_reference[2:])
    assert torch.allclose(A, mp + cp) and torch.linalg.eigvalsh(A).min().item() >= -1e-10 * top


def test_argument_errors_come_before_the_device_on_a_cpu_model():
    from gpplus_amd._lib import GppError
    from gpplus_amd.models import GP_Plus

    fx = gr.load_fixture("c3_borehole_mixed_n100.npz")
    X, y = torch.tensor(fx["Utrain"]), torch.tensor(fx["ytrain"])
    m = GP_Plus(X[:80], y[:80], qual_dict={0: 5, 5: 5}, dtype=torch.float64, device="cpu")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    good = X[80:90]
    bad_nan, bad_inf, bad_level = good.clone(), good.clone(), good.clone()
    bad_nan[1, 2] = float("nan")
    bad_inf[0, 3] = float("inf")
    bad_level[2, 5] = 9.0
    for what, rows in {"columns": good[:, :7], "empty": good[:0], "nan": bad_nan, "inf": bad_inf, "level": bad_level}.items():
        with pytest.raises(ValueError, match="predict_gradient|not seen"):
            m.predict_gradient(rows)
        with pytest.raises(ValueError, match="predict_gradient|not seen"):
            m.predict_gradient(rows, return_cov=True)
        with pytest.raises(ValueError, match="active_subspace|not seen"):
            m.active_subspace(rows)
    ones = torch.ones(good.shape[0], dtype=torch.float64)
    neg, nan = ones.clone(), ones.clone()
    neg[3] = -0.1
    nan[0] = float("nan")
    for what, wts in {"negative": neg, "nan": nan, "all zero": 0 * ones, "length": ones[:-1]}.items():
        with pytest.raises(ValueError, match="weights"):
            m.active_subspace(good, weights=wts)
    # valid calls reach the device, and there is none
    for call in (lambda: m.predict_gradient(good), lambda: m.predict_gradient(good, return_std=False),
                 lambda: m.active_subspace(good, weights=ones)):
        with pytest.raises(GppError, match="no CPU fallback"):
            call()
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    # a source the model has not seen
    fx = gr.load_fixture("c4_wing_mf_n300.npz")
    X, y = torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"])
    keep = X[:, 10] != 2
    m = GP_Plus(X[keep], y[keep], qual_dict={10: 3}, multiple_noise=True, m_gp="multiple_constant", dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="not seen"):
        m.predict_gradient(X[~keep][:4])
    # a model without a quantitative column
    rng = np.random.default_rng(2)
    Xc = torch.tensor(np.stack([rng.integers(0, 3, 40), rng.integers(0, 2, 40)], 1).astype(np.float64))
    mc = GP_Plus(Xc, torch.tensor(rng.standard_normal(40)), qual_dict={0: 3, 1: 2}, dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="no quantitative"):
        mc.predict_gradient(Xc[:5])
    with pytest.raises(ValueError, match="no quantitative"):
        mc.active_subspace(Xc[:5])


def test_sharded_setting_is_refused_by_the_linalg_entry():
    from gpplus_amd import linalg, settings

    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            linalg.gradient_from_cache(None, None, 0, 1, "std")
    with pytest.raises(ValueError, match="want"):
        linalg.gradient_from_cache(None, None, 0, 1, "variance")


def test_symbols_are_declared_exported_and_bound():
    from gpplus_amd import _lib, backend, linalg
    from gpplus_amd.models import GP_Plus

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_cross_kernel_dx\s*\(", header) and re.search(r"\bint gpp_point_gram\s*\(", header)
    assert "#define GPP_OP_POINT_GRAM 8" in header and backend.OP_POINT_GRAM == 8
    syms = _lib.exported_symbols()
    assert "gpp_cross_kernel_dx" in syms and len(_lib._SIGNATURES["gpp_cross_kernel_dx"][1]) == 14
    assert "gpp_point_gram" in syms and len(_lib._SIGNATURES["gpp_point_gram"][1]) == 9
    lib = _lib.load()
    assert lib.gpp_cross_kernel_dx.argtypes == _lib._SIGNATURES["gpp_cross_kernel_dx"][1]
    assert lib.gpp_point_gram.argtypes == _lib._SIGNATURES["gpp_point_gram"][1]
    assert callable(backend.GppContext.cross_kernel_dx) and callable(backend.GppContext.point_gram)
    assert callable(GP_Plus.predict_gradient) and callable(GP_Plus.active_subspace) and linalg.GRAD_CHUNK_BYTES == 256 << 20
    # the points' own matrices (when G is NULL) and one partial per 32 points: 70 points of 5 x 5 -> (70 + 3) * 25 doubles
    assert lib.gpp_workspace_bytes(None, backend.OP_POINT_GRAM, 0, 70, 5, 0) >= 73 * 25 * 8
    # a NULL handle is argument 1 of both, before anything else is looked at
    assert lib.gpp_cross_kernel_dx(None, None, 0, None, 0, 0, None, None, 0, 0, 0, 0, None, 0) == -1
    assert lib.gpp_point_gram(None, None, 0, 0, 0, 0, None, None, None) == -1

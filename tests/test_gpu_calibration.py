"""Deterministic calibration on the GPU: gpp_calib_grad_reduce against the dense CPU reference (tests/calibration_reference.py) and
against gpp_grad_reduce's feature gradients, and ``GP_Plus(..., calibration_id=[...])`` — objective, every gradient, predictions,
a fit — against the same reference.

The bar is the project's one for kernel derivatives against the oracle: 1e-6 of the largest reference magnitude."""
import functools

import numpy as np
import pytest
import torch

import calibration_reference as cr

pytestmark = pytest.mark.gpu

BAR = 1e-6
TILE = 64  # gpp_calib_tiles' tile edge (GT in gpp_reduce.hip)
ALL_QUANT = list(range(10))


@functools.lru_cache(maxsize=None)
def _oracle(ids, kclass="Rough_RBF", multiple_noise=True):
    """The reference on c4 at the fixture's parameters, theta away from the prior mean and from any optimum (built once per case)."""
    fx = cr.load_fixture()
    kw = dict(cr.C4_KW, multiple_noise=multiple_noise, quant_correlation_class=kclass)
    co = cr.CalibratedOracle(fx["Xtrain"], fx["ytrain"], list(ids), **kw)
    for k in list(co.params):
        if f"theta1::param::{k}" in fx:
            v = torch.as_tensor(fx[f"theta1::param::{k}"], dtype=torch.float64)
            co.params[k] = v.reshape(-1)[: co.params[k].numel()].reshape(co.params[k].shape)  # (S = 1: the first noise level)
    for i, n in enumerate(ids):
        co.params[f"Theta_{n}.constant"] = torch.tensor([0.7 - 0.35 * i], dtype=torch.float64)
    if len(ids) == len(ALL_QUANT):
        # every quantitative column calibrated: the 100 rows of source 0 coincide in ALL features, and cond(Ky) ~ 100 sf2 / tau.  At
        # the fixture's tau = 1e-4 ... 9e-4 that is ~1e6 and the reference's own two routes to g_theta on the CPU (autograd through
        # the Cholesky factor; sum_ij W_ij dK_ij from its alpha and Ky^-1) part by 2e-10 ... 6.5e-7 of the largest component,
        # at tau = 1e-2 by 7e-13 ... 1.4e-10: the noise of these cases is set to 1e-2, so that the bar measures the kernel
        raw = co.params["likelihood.noise_covar.raw_noise"]
        co.params["likelihood.noise_covar.raw_noise"] = torch.full_like(raw, float(np.log(1e-2 - 1e-8)))
    return co


def _rows(n, contiguous):
    """The first ``n`` rows of c4 (its sources alternate: a scattered membership), or the same rows sorted by source."""
    if n is None and not contiguous:
        return None
    src = torch.as_tensor(cr.load_fixture()["Xtrain"][:, -1])
    rows = torch.arange(src.shape[0] if n is None else n)
    return rows[torch.argsort(src[rows], stable=True)] if contiguous else rows


def _device_operands(ops):
    """The CPU operands on the GPU as the library takes them; Ky^-1 as the LAUUM leaves it: the LOWER triangle in a padded square,
    NaN above the diagonal (nothing there may be read into a result)."""
    from gpplus_amd.backend import square_buffer

    dev = torch.device("cuda:0")
    N = ops["U"].shape[0]
    Kinv = square_buffer(N, dev)
    Kinv.copy_(ops["Kinv"].to(dev))
    Kinv += torch.full((N, N), float("nan"), dtype=torch.float64, device=dev).triu(1)
    out = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in ops.items() if k != "Kinv"}
    out["Kinv"] = Kinv
    return out


def _calib(ctx, d, member=None, cols=None):
    cols = d["cols"] if cols is None else cols
    g = torch.full((cols.numel(),), float("nan"), dtype=torch.float64, device=d["U"].device)
    ctx.calib_grad_reduce(d["U"], d["w"], d["sf2"], d["alpha"], d["Kinv"], d["member"] if member is None else member, cols, g,
                          kind=d["kind"], d_split=d["d_split"])
    return g


def _assert_close(got, ref, what):
    got, ref = got.detach().cpu().reshape(-1), ref.detach().cpu().reshape(-1)
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"{what}: max |err| {err:.3e}, largest reference magnitude {scale:.3e}, ratio {err / scale if scale else 0.0:.2e}")
    assert err <= BAR * scale, (what, err, scale)


KERNEL_CASES = [
    # (ids, kernel class, S = 3 noise groups, rows, contiguous membership)
    ((2,), "Rough_RBF", True, 1, False),
    ((2,), "Rough_RBF", True, 2, False),
    ((2, 7), "Rough_RBF", True, TILE - 1, False),
    ((2, 7), "Rough_RBF", True, TILE, False),
    ((2, 7), "Rough_RBF", True, TILE + 1, False),
    ((2, 7), "Rough_RBF", True, TILE + 1, True),
    ((2,), "Rough_RBF", True, None, False),
    ((2,), "Rough_RBF", True, None, True),
    (tuple(ALL_QUANT), "Rough_RBF", True, None, False),
    (tuple(ALL_QUANT), "Rough_RBF", False, None, True),
    ((2,), "Rough_RBF", False, None, False),
    ((2, 7), "Matern32Kernel", True, None, False),
    ((2, 7), "Matern52Kernel", True, None, False),
    (tuple(ALL_QUANT), "Matern32Kernel", False, TILE + 1, True),
    (tuple(ALL_QUANT), "Matern52Kernel", True, None, True),
]


@pytest.mark.parametrize("ids,kclass,multi,n,contiguous", KERNEL_CASES)
def test_kernel_matches_reference(gpu_ctx, ids, kclass, multi, n, contiguous):
    ops = cr.kernel_operands(_oracle(ids, kclass, multi), _rows(n, contiguous))
    if n == 2:
        assert ops["member"].tolist() == [1, 0]  # one row of each source
    d = _device_operands(ops)
    g = _calib(gpu_ctx, d)
    assert bool(torch.isfinite(g).all())
    _assert_close(g, ops["g_theta"], f"g_theta {kclass} C={len(ids)} N={ops['U'].shape[0]} S={ops['S']} contiguous={contiguous}")
    assert torch.equal(g, _calib(gpu_ctx, d))  # bitwise, run to run


@pytest.mark.parametrize("kclass", ["Rough_RBF", "Matern32Kernel", "Matern52Kernel"])
@pytest.mark.parametrize("contiguous", [False, True])
def test_kernel_matches_feature_gradients_of_grad_reduce(gpu_ctx, kclass, contiguous):
    """g_theta[k] = sum over the member rows of grad_reduce(dU = D)'s g_U[i, c_k], for EVERY feature column: the latent ones
    (left of d_split, RBF factor) and the quantitative ones (right of it, the Matern factor for the Matern kinds)."""
    ops = cr.kernel_operands(_oracle((2, 7), kclass, True), _rows(None, contiguous))
    d = _device_operands(ops)
    dev, (N, D) = d["U"].device, d["U"].shape
    g_w, g_s, g_t = (torch.empty(k, dtype=torch.float64, device=dev) for k in (D, 1, ops["S"]))
    g_U = torch.empty(N, D, dtype=torch.float64, device=dev)
    gpu_ctx.grad_reduce(d["U"], d["w"], d["sf2"], d["grp"], ops["S"], d["alpha"], d["Kinv"], D, g_w, g_s, g_t, g_U, kind=d["kind"],
                        d_split=d["d_split"])
    ref = g_U[d["member"].bool()].sum(0)
    cols = torch.arange(D, dtype=torch.int32, device=dev)
    assert d["d_split"] in (0, 2) and D == 12
    _assert_close(_calib(gpu_ctx, d, cols=cols), ref, f"g_theta against sum g_U, {kclass}, contiguous={contiguous}")
    # and in any order of the columns
    perm = torch.tensor([9, 0, 4, 11], dtype=torch.int32, device=dev)
    _assert_close(_calib(gpu_ctx, d, cols=perm), ref[perm.long()], f"g_theta against sum g_U, permuted columns, {kclass}")


@pytest.mark.parametrize("n", [2, TILE + 1, None])
def test_one_membership_gives_exact_zeros(gpu_ctx, n):
    ops = cr.kernel_operands(_oracle((2, 7), "Matern52Kernel", True), _rows(n, False))
    d = _device_operands(ops)
    for value in (0, 1):
        member = torch.full_like(d["member"], value)
        g = _calib(gpu_ctx, d, member=member)
        assert torch.equal(g, torch.zeros_like(g)) and not bool(torch.signbit(g).any())


def test_wrapper_refuses_bad_arguments(gpu_ctx):
    from gpplus_amd._lib import GppError

    d = _device_operands(cr.kernel_operands(_oracle((2,)), _rows(TILE, False)))
    dev = d["U"].device
    with pytest.raises(GppError, match="out of range"):
        _calib(gpu_ctx, d, cols=torch.tensor([12], dtype=torch.int32, device=dev))
    with pytest.raises(GppError, match="out of range"):
        _calib(gpu_ctx, d, cols=torch.tensor([-1], dtype=torch.int32, device=dev))
    with pytest.raises(GppError, match="C <= D"):
        _calib(gpu_ctx, d, cols=torch.zeros(13, dtype=torch.int32, device=dev))
    with pytest.raises(GppError, match="int32"):
        _calib(gpu_ctx, d, member=d["member"].long())
    with pytest.raises(GppError, match="member"):
        _calib(gpu_ctx, d, member=d["member"][:-1].contiguous())


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _model(co, X, y, ids, **kw):
    from gpplus_amd.models import GP_Plus

    m = GP_Plus(torch.tensor(np.asarray(X)).clone(), torch.tensor(np.asarray(y)), dtype=torch.float64, device="cuda",
                calibration_id=list(ids), **kw)
    if co is not None:
        sd = m.state_dict()
        for k, v in co.params.items():
            sd[k] = v.reshape(sd[k].shape).to(sd[k])
        m.load_state_dict(sd)
    return m


def _loss_and_grads(m):
    from gpplus_amd.gpcore import ExactMarginalLogLikelihood

    m.train()
    mll = ExactMarginalLogLikelihood(m.likelihood, m)
    for p in m.parameters():
        p.grad = None
    loss = -mll(m(*m.train_inputs), m.train_targets)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("ids", [(2,), (2, 7)])
def test_model_objective_gradients_and_predictions_match_reference(gpu_ctx, ids):
    fx = cr.load_fixture()
    co = _oracle(ids)
    m = _model(co, fx["Xtrain"], fx["ytrain"], ids, **cr.C4_KW)
    loss, grads = _loss_and_grads(m)
    lo, go = co.loss_and_grad()
    print(f"loss {loss.item():.15e} reference {lo.item():.15e}")
    assert abs(loss.item() - lo.item()) <= BAR * abs(lo.item())
    assert set(grads) == set(go) and all(f"Theta_{n}.constant" in grads for n in ids)
    for k, g in go.items():
        _assert_close(grads[k], g, f"grad {k}")
    # predictions on test rows of all three sources; source 0's calibrated columns hold whatever the caller put there
    xt = torch.tensor(fx["Xtest"])
    assert sorted(set(xt[:, -1].tolist())) == [0.0, 1.0, 2.0]
    for include_noise in (True, False):
        mean, std = m.predict(xt, return_std=True, include_noise=include_noise)
        rm, rs = co.predict(xt, include_noise=include_noise)
        _assert_close(mean, rm, f"predict mean (noise={include_noise})")
        _assert_close(std, rs, f"predict std (noise={include_noise})")
    other = xt.clone()
    hf = other[:, -1] == 0
    for n in ids:
        other[hf, n] = 123.0
    mean2, std2 = m.predict(other, return_std=True, include_noise=True)
    mean1, std1 = m.predict(xt, return_std=True, include_noise=True)
    assert torch.equal(mean1, mean2) and torch.equal(std1, std2)
    # the estimate is what the model reports
    assert m.calibration_result() == {n: float(co.params[f"Theta_{n}.constant"]) for n in ids}


def test_model_without_calibration_is_untouched(gpu_ctx):
    """No ``calibration_id``: the evaluation is ExactMLLFunction's own launches and nothing else, and its loss and gradients are
    bitwise those of calling that Function on the model's operands."""
    from gpplus_amd import linalg
    from gpplus_amd.gpcore import ExactMarginalLogLikelihood

    fx = cr.load_fixture()
    m = _model(None, fx["Xtrain"], fx["ytrain"], (), **cr.C4_KW)
    sd = m.state_dict()
    for k in list(sd):
        if f"theta1::param::{k}" in fx:
            sd[k] = torch.as_tensor(fx[f"theta1::param::{k}"]).reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    assert not any(k.startswith("Theta_") for k in sd)
    linalg.STAGE_EVENTS = []
    try:
        loss, grads = _loss_and_grads(m)
        stages = [name for name, _, _ in linalg.STAGE_EVENTS]
    finally:
        linalg.STAGE_EVENTS = None
    assert stages == ["kernel_build", "potrf", "trtri", "mll_reduce", "alpha", "lauum", "grad_reduce"]
    # the same operands through the Function itself
    for p in m.parameters():
        p.grad = None
    out = m.likelihood(m(*m.train_inputs))
    cov = out.lazy_covariance_matrix
    assert cov.calib is None
    val = linalg.ExactMLLFunction.apply(cov.U1, cov.spec.w, cov.spec.sf2, cov.tau, out.mean, m.train_targets, cov.grp, cov.spec.kind,
                                        cov.spec.d_split, int(cov.n_grad_dims), 0)
    mll = ExactMarginalLogLikelihood(m.likelihood, m)
    loss2 = -((val + mll._prior_sum(val.dtype)) / out.event_shape.numel())
    loss2.backward()
    assert torch.equal(loss, loss2.detach())
    again = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert set(again) == set(grads) and len(grads) == 6
    for n, g in again.items():
        assert torch.equal(grads[n], g), n
    # with calibration parameters the extra stage is there, on the dense route
    mc = _model(_oracle((2,)), fx["Xtrain"], fx["ytrain"], (2,), **cr.C4_KW)
    linalg.STAGE_EVENTS = []
    try:
        _loss_and_grads(mc)
        stages = [name for name, _, _ in linalg.STAGE_EVENTS]
    finally:
        linalg.STAGE_EVENTS = None
    assert stages == ["kernel_build", "potrf", "trtri", "mll_reduce", "alpha", "lauum", "grad_reduce", "calib_grad_reduce"]


def test_fit_recovers_theta_on_the_analytic_problem(gpu_ctx):
    """``fit_model_scipy`` from the reference's start (theta at its prior mean 0) lowers the objective and ends nearer THETA_STAR
    than it began.  tests/test_calibration_host.py confirms the same of the reference's own L-BFGS run from this start."""
    from gpplus_amd.optim import fit_model_scipy
    from gpplus_amd.optim.mll_scipy import MLLObjective, marginal_log_likelihood
    from gpplus_amd.test_functions.calibration import THETA_STAR, calibration_problem, calibration_test_rows

    kw = {"qual_dict": {2: 2}, "m_gp": "multiple_constant"}
    X, y = calibration_problem(16, 64, seed=0)
    co = cr.CalibratedOracle(X, y, [1], **kw)
    m = _model(co, X, y, (1,), **kw)
    assert m.calibration_result() == {1: 0.0}
    m.train()
    with torch.no_grad():
        start = float(-marginal_log_likelihood(m, True))
    assert abs(start - co.loss(normalize=False).item()) <= BAR * abs(start)
    theta0 = MLLObjective(m, True, [0, 0]).pack_parameters()
    out, best = fit_model_scipy(m, add_prior=True, theta0_list=[theta0], bounds=True)
    theta_hat = m.calibration_result()[1]
    print(f"objective {start:.6f} -> {best:.6f} in {out[0].nit} iterations; theta {theta_hat:.6f} (THETA_STAR {THETA_STAR})")
    assert np.isfinite(best) and best < start
    assert abs(theta_hat - THETA_STAR) < abs(0.0 - THETA_STAR)
    # the fitted model predicts both sources (source 0 from rows that carry no theta) about as well as the fit promises
    Xt, yt = calibration_test_rows()
    mean = m.predict(torch.tensor(Xt), return_std=False)
    assert bool(torch.isfinite(mean).all())
    print(f"test RMSE {float(((mean.cpu() - torch.tensor(yt)) ** 2).mean().sqrt()):.3e}")

"""GP_Plus.predict_gradient and GP_Plus.active_subspace on the GPU against the dense fp64 reference of tests/gradpost_reference.py
(the CPU oracle's own pieces differentiated by autograd) and against the existing differentiable prediction (gpp_cross_grad), on
the models of tests/test_gpu_predict_grad.py at their fitted parameters plus a Matern-5/2 model; chunking, conditioned models, a
reused workspace, the wide (p > 16) route and the refusals.

The bar of every comparison with the reference is 1e-6 of the largest reference magnitude, the one ``_check_model_grads`` holds the
same kernel derivatives to against the same oracle."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradpost_reference as gr  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-6
M_TEST = 40
CASES = {
    "c1": ("c1_borehole_n500.npz", None, {}),
    "c3": ("c3_borehole_mixed_n100.npz", None, {"qual_dict": {0: 5, 5: 5}}),
    "c4": ("c4_wing_mf_n300.npz", None, {"qual_dict": {10: 3}, "multiple_noise": True, "m_gp": "multiple_constant"}),
    "c1-matern52": ("c1_borehole_n500.npz", 200, {"quant_correlation_class": "Matern52Kernel"}),
}
_cache = {}


def _model_from_oracle(o, X, y, **kw):
    from gpplus_amd.models import GP_Plus

    m = GP_Plus(torch.tensor(X), torch.tensor(y), dtype=torch.float64, device="cuda", **kw)
    sd = m.state_dict()
    for k, v in o.params.items():
        sd[k] = v.reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    return m


def _case(name):
    """(model, oracle, test rows, reference mean, reference covariance): built once per case and left unchanged."""
    if name not in _cache:
        fixture, n, kw = CASES[name]
        fx = gr.load_fixture(fixture)
        o = gr.load_oracle(fx, n, **kw)
        X, y = gr.fixture_xy(fx, n)
        xt = gr.fixture_test_rows(fx, M_TEST)
        g, S = gr.gradient_posterior(o, xt)
        _cache[name] = (_model_from_oracle(o, X, y, **kw), o, xt, g, S)
    return _cache[name]


def _close(got, ref, what, bar=BAR):
    scale = ref.abs().max().item()
    err = (got.detach().cpu() - ref).abs().max().item()
    print(f"{what}: max error {err:.3e} = {err / scale:.3e} of max|reference| {scale:.3e}")
    assert err <= bar * scale, (what, err, scale)


@pytest.mark.parametrize("name", list(CASES))
def test_predict_gradient_against_reference_and_autograd(gpu_ctx, name):
    from gpplus_amd import linalg

    m, o, xt, g_ref, S_ref = _case(name)
    p = len(o.quant_index)
    mean, std = m.predict_gradient(xt)
    mean_c, cov = m.predict_gradient(xt, return_cov=True)
    mean_only = m.predict_gradient(xt, return_std=False)
    assert mean.shape == (M_TEST, p) and std.shape == (M_TEST, p) and cov.shape == (M_TEST, p, p)
    assert p == xt.shape[1] - len(CASES[name][2].get("qual_dict", {}))  # the categorical columns are not in the output
    for t in (mean, std, mean_c, cov, mean_only):
        assert t.grad_fn is None and not t.requires_grad and t.is_cuda
    # the mean: the reference, the existing differentiable prediction (gpp_cross_grad), and the two routes against each other
    _close(mean, g_ref, f"{name} mean (predict_tn route)")
    _close(mean_only, g_ref, f"{name} mean (kernel_apply_grad route)")
    _close(mean_only, mean.cpu(), f"{name} mean: the two routes")
    assert torch.equal(mean, mean_c)
    x = xt.clone().cuda().requires_grad_(True)
    pm = m.predict_with_grad(x, return_std=False)
    gx, = torch.autograd.grad(pm.sum(), x)
    _close(mean, gx[:, m.quant_index.long()].cpu(), f"{name} mean against autograd of predict_with_grad")
    cat = [c for c in range(xt.shape[1]) if c not in o.quant_index]
    assert bool((gx[:, cat] == 0).all())
    # std and cov
    var_ref = torch.diagonal(S_ref, dim1=1, dim2=2)
    _close(std, var_ref.clamp_min(0).sqrt(), f"{name} std")
    _close(cov, S_ref, f"{name} cov")
    assert torch.equal(cov.view(torch.int64), cov.transpose(1, 2).contiguous().view(torch.int64)), "cov is not bitwise symmetric"
    _close(torch.diagonal(cov, dim1=1, dim2=2).clamp_min(0), (std ** 2).cpu(), f"{name} diag(cov) against std^2")
    # the linalg entry in the cache's units
    cache = m.prediction_strategy
    Us = m._features(xt.cuda())[0]
    gs, var = linalg.gradient_from_cache(cache, Us, Us.shape[1] - p, p, "std")
    assert torch.equal(gs * m.y_std, mean) and torch.equal(var.clamp_min(0).sqrt() * m.y_std.abs(), std)


@pytest.mark.parametrize("name", list(CASES))
def test_active_subspace(gpu_ctx, name):
    m, o, xt, g_ref, S_ref = _case(name)
    p = len(o.quant_index)
    mean, cov = m.predict_gradient(xt, return_cov=True)
    wts = torch.linspace(0.0, 2.0, M_TEST, dtype=torch.float64) ** 2  # non-uniform, one of them zero
    for label, w in (("uniform", None), ("weighted", wts)):
        res = m.active_subspace(xt, weights=w)
        A_ref, mp_ref, cp_ref = gr.active_subspace(g_ref, S_ref, w)
        _close(res.matrix, A_ref, f"{name} {label} matrix")
        _close(res.mean_part, mp_ref, f"{name} {label} mean part", bar=BAR * A_ref.abs().max().item() / mp_ref.abs().max().item())
        _close(res.cov_part, cp_ref, f"{name} {label} cov part", bar=BAR * A_ref.abs().max().item() / cp_ref.abs().max().item())
        wd = (torch.full((M_TEST,), 1.0 / M_TEST, dtype=torch.float64) if w is None else w).cuda()
        per_point = torch.einsum("a,ajk->jk", wd, mean[:, :, None] * mean[:, None, :] + cov)
        _close(res.matrix, per_point.cpu(), f"{name} {label} matrix against the per-point sum")
        assert res.matrix.shape == (p, p) and torch.equal(res.matrix, res.matrix.T)
        assert torch.equal(res.mean_part + res.cov_part, res.matrix)
        assert torch.equal(res.sensitivity, torch.diagonal(res.matrix))
        ev, V = res.eigenvalues, res.eigenvectors
        assert bool((ev[:-1] >= ev[1:]).all())
        assert (V.T @ V - torch.eye(p, dtype=torch.float64, device=V.device)).abs().max().item() <= 1e-12
        assert ev[-1].item() >= -BAR * ev[0].item()
        _close(V @ torch.diag(ev) @ V.T, res.matrix.cpu(), f"{name} {label} eigen-decomposition", bar=1e-12)
    assert not torch.allclose(m.active_subspace(xt).matrix, res.matrix)  # the weights are honoured


def test_active_subspace_finds_a_single_direction(gpu_ctx):
    """y = sin(3 a^T x): the response varies along a alone, so the leading eigenvector should point along a / |a|.  A sanity check,
    not a tolerance: it must be closer to a than the worst single coordinate axis is."""
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim import fit_model_torch

    rng = np.random.default_rng(11)
    a = np.array([0.8, -0.5, 0.3, 0.1])
    X = rng.uniform(-1.0, 1.0, (150, 4))
    y = np.sin(3.0 * X @ a)
    m = GP_Plus(torch.tensor(X), torch.tensor(y), dtype=torch.float64, device="cuda")
    fit_model_torch(model=m, num_iter=60, num_restarts=0, verbose=False)
    res = m.active_subspace(torch.tensor(rng.uniform(-1.0, 1.0, (64, 4))))
    unit = a / np.linalg.norm(a)
    align = abs(float(res.eigenvectors[:, 0].cpu().numpy() @ unit))
    print(f"alignment of the leading eigenvector with a / |a|: {align:.6f}; eigenvalues {res.eigenvalues.tolist()}")
    print(f"sensitivities {res.sensitivity.tolist()}")
    assert align > np.abs(unit).min()


def test_chunks_agree_with_one_chunk(gpu_ctx, monkeypatch):
    from gpplus_amd import linalg
    from gpplus_amd.backend import GppContext, row_stride

    m, o, xt, g_ref, S_ref = _case("c1")
    xt = xt[:37]
    p, N = len(o.quant_index), m.train_inputs[0].shape[0]
    wts = torch.linspace(0.5, 1.5, 37, dtype=torch.float64)
    one = (*m.predict_gradient(xt), m.predict_gradient(xt, return_cov=True)[1], m.active_subspace(xt, weights=wts).matrix)
    calls = []
    real = GppContext.cross_kernel_dx
    monkeypatch.setattr(GppContext, "cross_kernel_dx", lambda self, Ua, *a, **k: (calls.append(Ua.shape[0]), real(self, Ua, *a, **k))[1])
    monkeypatch.setattr(linalg, "GRAD_CHUNK_BYTES", 8 * p * row_stride(N) * 13)  # room for at most 13 points' rows of Q
    step = linalg._gradient_chunk_points(N, p)
    sizes = [min(step, 37 - a0) for a0 in range(0, 37, step)]
    assert len(sizes) >= 3 and sum(sizes) == 37
    many = (*m.predict_gradient(xt), m.predict_gradient(xt, return_cov=True)[1], m.active_subspace(xt, weights=wts).matrix)
    assert calls == sizes * 3
    refs = (g_ref[:37], torch.diagonal(S_ref[:37], dim1=1, dim2=2).clamp_min(0).sqrt(), S_ref[:37], gr.active_subspace(g_ref[:37], S_ref[:37], wts)[0])
    for what, a, b, ref in zip(("mean", "std", "cov", "active-subspace matrix"), one, many, refs):
        same = torch.equal(a, b)
        print(f"chunked {what}: bitwise equal to one chunk: {same}")
        assert (a - b).abs().max().item() <= BAR * ref.abs().max().item(), what


def test_after_condition_on(gpu_ctx):
    """The methods read the bordered cache of a conditioned model (owned factors): the same object with its cache dropped factors
    all rows from scratch and must agree."""
    from gpplus_amd.models import GP_Plus

    fx = gr.load_fixture("c1_borehole_n500.npz")
    o = gr.load_oracle(fx, 120)
    X, y = gr.fixture_xy(fx, 150)
    parent = _model_from_oracle(o, X[:120], y[:120])
    child = parent.condition_on(torch.tensor(X[120:]), torch.tensor(y[120:]))
    assert child.prediction_strategy.route in ("copy", "in_place")
    xt = gr.fixture_test_rows(fx, M_TEST)
    got = (*child.predict_gradient(xt), child.predict_gradient(xt, return_cov=True)[1], child.active_subspace(xt).matrix)
    assert child.prediction_strategy.route in ("copy", "in_place")  # still the bordered cache
    held, child.prediction_strategy = child.prediction_strategy, None
    try:
        scratch = (*child.predict_gradient(xt), child.predict_gradient(xt, return_cov=True)[1], child.active_subspace(xt).matrix)
        assert child.prediction_strategy.route is None
    finally:
        child.prediction_strategy = held
    for what, a, b in zip(("mean", "std", "cov", "matrix"), got, scratch):
        _close(a, b.cpu(), f"conditioned model, {what}")
    # and the parent's own answers are those of a model that never had a child
    fresh = _model_from_oracle(o, X[:120], y[:120])
    assert torch.equal(parent.predict_gradient(xt)[0], fresh.predict_gradient(xt)[0])
    assert isinstance(child, GP_Plus) and child.train_inputs[0].shape[0] == 150


def test_after_another_model_took_the_workspace(gpu_ctx):
    fx = gr.load_fixture("c1_borehole_n500.npz")
    o = gr.load_oracle(fx, 200)
    X, y = gr.fixture_xy(fx, 200)
    a = _model_from_oracle(o, X, y)
    xt = gr.fixture_test_rows(fx, M_TEST)
    first = (*a.predict_gradient(xt), a.predict_gradient(xt, return_cov=True)[1], a.active_subspace(xt).matrix)
    ob = gr.load_oracle(fx, 200)
    ob.params["covar_module.raw_outputscale"] = ob.params["covar_module.raw_outputscale"] + 0.5
    b = _model_from_oracle(ob, X, y)
    b.predict(xt.cuda())  # same N: factors into the shared prediction workspace
    assert a.prediction_strategy.stale()
    again = (*a.predict_gradient(xt), a.predict_gradient(xt, return_cov=True)[1])
    assert not a.prediction_strategy.stale()
    b.predict(xt.cuda())
    again = (*again, a.active_subspace(xt).matrix)
    for what, r, g in zip(("mean", "std", "cov", "matrix"), first, again):
        assert torch.equal(r, g), what


def test_wide_model_takes_the_bmm_route(gpu_ctx, monkeypatch):
    from oracle.gp_oracle import OracleGP
    from gpplus_amd.backend import GppContext

    rng = np.random.default_rng(17)
    p, N = 17, 60
    X = rng.uniform(-1.0, 1.0, (N, p))
    y = np.sin(X[:, 0] + 0.5 * X[:, 3]) + 0.1 * X[:, 16] ** 2
    o = OracleGP(X, y)
    o.params[o.ls_key] = torch.tensor(rng.uniform(-1.5, -0.5, (1, p)))
    o.params["likelihood.noise_covar.raw_noise"] = torch.tensor([-7.0], dtype=torch.float64)
    m = _model_from_oracle(o, X, y)
    xt = torch.tensor(rng.uniform(-1.0, 1.0, (9, p)))
    g_ref, S_ref = gr.gradient_posterior(o, xt)

    def no_gram(*a, **k):
        raise AssertionError("gpp_point_gram takes at most 16 rows per point")

    monkeypatch.setattr(GppContext, "point_gram", no_gram)
    mean, cov = m.predict_gradient(xt, return_cov=True)
    _close(mean, g_ref, "p = 17 mean")
    _close(cov, S_ref, "p = 17 cov")
    _close(m.predict_gradient(xt)[1], torch.diagonal(S_ref, dim1=1, dim2=2).clamp_min(0).sqrt(), "p = 17 std")
    wts = torch.linspace(0.2, 1.0, 9, dtype=torch.float64)
    _close(m.active_subspace(xt, weights=wts).matrix, gr.active_subspace(g_ref, S_ref, wts)[0], "p = 17 matrix")


def test_refusals(gpu_ctx):
    from gpplus_amd import settings

    m, _, xt, _, _ = _case("c3")
    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            m.predict_gradient(xt)
        with pytest.raises(NotImplementedError):
            m.active_subspace(xt)
    with pytest.raises(ValueError):
        m.predict_gradient(xt[:, :-1])
    assert m.predict_gradient(xt)[0].shape == (M_TEST, xt.shape[1] - 2)

"""``ensemble.HyperparameterEnsemble`` on the GPU: the members against ``load_state_dict`` + ``model.predict`` one by one, the
mixture against numpy, a one-member ensemble against the model itself, the fused launch against the composed route, chunking bit for
bit, ``GP_Plus.fit(keep_restarts=...)`` against the same fit without the keyword, independence from a refit of the receiver, and a
member whose covariance is not positive definite as it stands.

Models: N = 60 with two quantitative columns and one categorical column (the latent map differs per member, so the features are not
shared), and N = 90 with two sources and ``multiple_noise=True`` (a constant mean and a noise level per source).
Bar: 1e-6 of the largest magnitude of what is compared.  Every comparison prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_reference as E  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 1e-6
DT = torch.float64
K = 4


def _bits(t):
    return t.contiguous().view(torch.int64)


def _data(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    levels = 3 if kind == "mixed" else 2
    X = np.stack([rng.uniform(0, 1, n), rng.uniform(0, 1, n), (np.arange(n) % levels).astype(float)], 1)
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + 0.3 * X[:, 2] + 0.01 * rng.standard_normal(n)
    return X, y


def _model(kind, **kw):
    from gpplus_amd.models import GP_Plus

    if kind == "mixed":
        X, y = _data(kind, 60)
        return GP_Plus(torch.tensor(X), torch.tensor(y), qual_dict={2: 3}, dtype=DT, device="cuda", **kw)
    X, y = _data(kind, 90)
    return GP_Plus(torch.tensor(X), torch.tensor(y), qual_dict={2: 2}, multiple_noise=True, m_gp="multiple_constant", dtype=DT,
                   device="cuda", **kw)


def _test_rows(kind, m=20):
    """Rows of every level / of both sources, one of them a training row."""
    X, _ = _data(kind, 60 if kind == "mixed" else 90)
    Xt, _ = _data(kind, m, seed=7)
    Xt[0] = X[4]
    return torch.tensor(Xt)


def _stacked(model, k=K, seed=1, spread=0.3):
    g = torch.Generator().manual_seed(seed)
    return {n: (p.detach().cpu().unsqueeze(0) + spread * torch.randn(k, *p.shape, generator=g, dtype=p.dtype)).to(p.device)
            for n, p in model.named_parameters() if p.requires_grad}


@pytest.fixture(scope="module", params=["mixed", "two_sources"])
def setup(request, gpu_ctx):
    from gpplus_amd.ensemble import HyperparameterEnsemble

    kind = request.param
    m = _model(kind)
    ens = HyperparameterEnsemble(m, _stacked(m), losses=[0.31, 0.30, 0.305, 0.33], num_data=int(m.train_targets.shape[0]))
    return kind, m, ens, _test_rows(kind).to("cuda")


def _rel(a, b):
    a, b = a.detach().cpu().numpy().astype(E.LD), b.detach().cpu().numpy().astype(E.LD)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("include_noise", [True, False])
def test_members_against_the_model_with_their_parameters_loaded(setup, include_noise):
    kind, m, ens, Xt = setup
    mu, sd, mus, sds = ens.predict(Xt, include_noise=include_noise, return_members=True)
    assert mus.shape == sds.shape == (K, Xt.shape[0]) and mu.shape == sd.shape == (Xt.shape[0],)
    twin = m._copy_without_factors()
    for b in range(K):
        twin.train()
        twin.load_state_dict(ens.state(b))
        rm, rs = twin.predict(Xt, return_std=True, include_noise=include_noise)
        em, es = _rel(mus[b], rm), _rel(sds[b], rs)
        print(f"{kind} include_noise={include_noise} member {b}: mean {em:.3e} std {es:.3e} (jitter {float(ens.jitter[b]):.1e})")
        assert em <= BAR and es <= BAR
    # the mean alone: the same numbers
    mu_only, mus_only = ens.predict(Xt, return_std=False, return_members=True)
    assert torch.equal(_bits(mus_only), _bits(mus)) and torch.equal(_bits(ens.predict(Xt, return_std=False)), _bits(mu_only))
    if kind == "two_sources" and include_noise:
        noiseless = ens.predict(Xt, include_noise=False, return_members=True)[3]
        assert bool((sds > noiseless).all())


def test_mixture_against_numpy_from_the_members(setup):
    kind, m, ens, Xt = setup
    mu, sd, mus, sds = ens.predict(Xt, return_members=True)
    pi = E.posterior_weights(ens.losses.numpy(), ens.num_data)
    assert float(np.abs(ens.weights.numpy().astype(E.LD) - pi).max()) <= 8 * 2.0 ** -53
    rm, rv = E.mixture(pi, mus.cpu().numpy(), sds.cpu().numpy().astype(E.LD) ** 2)
    em = float(np.abs(mu.cpu().numpy().astype(E.LD) - rm).max() / np.abs(rm).max())
    es = float(np.abs(sd.cpu().numpy().astype(E.LD) - np.sqrt(rv)).max() / np.sqrt(rv).max())
    spread = float((mus.max(0).values - mus.min(0).values).max())
    print(f"{kind} mixture: mean {em:.3e} std {es:.3e}; weights {ens.weights.tolist()}; largest spread of the member means {spread:.3e}")
    assert em <= BAR and es <= BAR
    # the mixture is at least as wide as the weighted members
    assert bool((sd ** 2 >= (ens.weights.to(sd).reshape(-1, 1) * sds ** 2).sum(0) * (1 - 1e-12)).all())


def test_one_member_of_the_models_own_parameters_is_the_model(setup):
    from gpplus_amd.ensemble import HyperparameterEnsemble

    kind, m, _, Xt = setup
    own = {n: p.detach().unsqueeze(0).clone() for n, p in m.named_parameters() if p.requires_grad}
    one = HyperparameterEnsemble(m, own, weights="uniform")
    for include_noise in (True, False):
        mu, sd = one.predict(Xt, include_noise=include_noise)
        rm, rs = m.predict(Xt, return_std=True, include_noise=include_noise)
        em, es = _rel(mu, rm), _rel(sd, rs)
        print(f"{kind} K = 1 include_noise={include_noise}: mean {em:.3e} std {es:.3e}")
        assert em <= BAR and es <= BAR
    m.train()


def test_fused_against_composed_and_chunking_bit_for_bit(setup, monkeypatch):
    from gpplus_amd import ensemble

    kind, m, ens, Xt = setup
    fused = ens.predict(Xt, return_members=True, route="fused")
    comp = ens.predict(Xt, return_members=True, route="composed")
    default = ens.predict(Xt, return_members=True)
    for name, a, b in zip(("mean", "std", "member means", "member stds"), fused, comp):
        e = _rel(a, b)
        print(f"{kind} fused against composed, {name}: {e:.3e}")
        assert e <= BAR
    assert ens._N <= ensemble.ENSEMBLE_FUSED_MAX_N and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(default, fused))
    # seven rows per fused chunk: three launches for the twenty rows, and not a bit changes
    monkeypatch.setattr(ensemble, "ENSEMBLE_CHUNK_BYTES", 7 * 16 * K * ((ens._N + 63) // 64))
    assert ens._chunk_rows(True) == 7
    chunked = ens.predict(Xt, return_members=True, route="fused")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(chunked, fused))
    monkeypatch.setattr(ensemble, "ENSEMBLE_CHUNK_BYTES", 1)
    assert ens._chunk_rows(True) == 1 and ens._chunk_rows(False) == 1
    rows = ens.predict(Xt[:3], return_members=True, route="fused")
    assert all(torch.equal(_bits(a), _bits(b[..., :3])) for a, b in zip(rows, fused))
    comp_rows = ens.predict(Xt[:3], return_members=True, route="composed")
    assert all(_rel(a, b[..., :3]) <= BAR for a, b in zip(comp_rows, fused))


def test_a_refit_of_the_receiver_leaves_the_ensemble_alone(setup):
    from gpplus_amd.optim import fit_model_torch_batched

    kind, m, ens, Xt = setup
    before = ens.predict(Xt, return_members=True)
    was = {k: v.clone() for k, v in m.state_dict().items()}
    if hasattr(m.likelihood, "fidel_indices"):
        # an earlier predict() of the receiver has left the TEST rows' source column in its likelihood (GPR.predict does, as the
        # reference's): a fit needs the training rows' there
        m.likelihood.fidel_indices = m.train_inputs[0][:, -1]
    torch.manual_seed(3)
    fit_model_torch_batched(m, num_iter=4, num_restarts=1)
    assert any(not torch.equal(v, was[k]) for k, v in m.state_dict().items()), "the refit did not move the receiver"
    m.predict(Xt)  # (and the receiver's own prediction cache, in the shared workspaces)
    after = ens.predict(Xt, return_members=True)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(after, before))
    m.load_state_dict(was)
    m.train()
    if hasattr(m.likelihood, "fidel_indices"):
        m.likelihood.fidel_indices = m.train_inputs[0][:, -1]


def test_fit_keeps_the_best_restarts_and_changes_nothing_else():
    import math

    from gpplus_amd.optim import fit_model_torch_batched

    def run(**kw):
        torch.manual_seed(11)  # (before the model: its construction draws the initial latent map)
        np.random.seed(11)
        m = _model("mixed")
        out = m.fit(optim_type="adam_torch", **kw)
        return m, out

    m0, (f0, h0) = run()
    assert m0.restart_ensemble is None and fit_model_torch_batched.last_restarts is None
    m1, (f1, h1) = run(keep_restarts=4)
    assert f1 == f0 and h1 == h0, "keep_restarts changed the fit"
    sd0, sd1 = m0.state_dict(), m1.state_dict()
    assert all(torch.equal(_bits(sd0[k]), _bits(sd1[k])) for k in sd0)
    ens = m1.restart_ensemble
    finite = sum(1 for h in h1 if h and math.isfinite(h[-1]))
    losses = ens.losses.tolist()
    print(f"kept {len(ens)} of {len(h1)} restarts ({finite} end finite): losses {losses}, weights {ens.weights.tolist()}, f_inc {f1}")
    assert len(ens) == min(4, finite) and losses == sorted(losses) and losses[0] == f1
    assert ens.num_data == 60 and int(ens.weights.argmax()) == 0
    s0 = ens.state(0)
    assert all(torch.equal(_bits(s0[k].to(sd1[k].device)), _bits(sd1[k])) for k in sd1)
    mu, sd, mus, sds = ens.predict(_test_rows("mixed"), return_members=True)
    rm, rs = m1.predict(_test_rows("mixed"), return_std=True)
    print(f"member 0 against the fitted model: mean {_rel(mus[0], rm):.3e} std {_rel(sds[0], rs):.3e}; "
          f"mixture std / winner std: {float((sd / sds[0]).min()):.4f} .. {float((sd / sds[0]).max()):.4f}")
    assert _rel(mus[0], rm) <= BAR and _rel(sds[0], rs) <= BAR and bool(torch.isfinite(sd).all())


def test_a_member_that_is_not_positive_definite_as_it_stands():
    """Ten duplicated rows and a fixed noise at its lower bound (``fix_noise``, 1.01e-12 over ``lb_noise=1e-12``): the duplicates make
    the covariance singular up to that noise.  What the jitter schedule (1e-8, 1e-7, 1e-6) does at this shape depends on the
    member's outputscale, so both ends are asserted here, each as observed on an MI355X and as the arithmetic says:
      * outputscale 1e5: the noise is below half an ulp of the diagonal and vanishes, the unjittered attempt fails, and the first
        jitter (1e-8, well above the rounding of a matrix of that size) rescues the member: finite predictions, ``jitter[1] == 1e-8``
        recorded, the other members untouched at 0;
      * outputscale 1e12 with lengthscales of 1e4: even the last jitter (1e-6) is below half an ulp of the diagonal (1.2e-4), the
        matrix stays exactly singular and ``NotPSDError`` names member 1."""
    from gpplus_amd.ensemble import HyperparameterEnsemble
    from gpplus_amd.errors import NotPSDError
    from gpplus_amd.models import GP_Plus

    X, y = _data("mixed", 60)
    X[50:60] = X[0:10]
    y[50:60] = y[0:10]
    m = GP_Plus(torch.tensor(X), torch.tensor(y), qual_dict={2: 3}, dtype=DT, device="cuda", lb_noise=1e-12, fix_noise=True,
                fix_noise_val=1.01e-12)
    assert not m.likelihood.raw_noise.requires_grad and abs(float(m.likelihood.noise) - 1.01e-12) < 1e-15
    Xt = _test_rows("mixed", 7).to("cuda")

    def members(outputscale, lengthscale=None):
        st = {n: p.detach().unsqueeze(0).repeat(3, *([1] * p.dim())).clone() for n, p in m.named_parameters() if p.requires_grad}
        assert "likelihood.noise_covar.raw_noise" not in st
        st["covar_module.raw_outputscale"][1] = outputscale
        if lengthscale is not None:
            st["covar_module.base_kernel.kernels.1.raw_lengthscale"][1] = lengthscale
        return HyperparameterEnsemble(m, st, weights="uniform")

    rescued = members(1e5)
    mu, sd, mus, sds = rescued.predict(Xt, return_members=True)
    print(f"outputscale 1e5: jitter {rescued.jitter.tolist()}, member 1 mean {mus[1].tolist()}, std {sds[1].tolist()}")
    assert rescued.jitter.tolist() == [0.0, 1e-8, 0.0]
    assert bool(torch.isfinite(mus).all() and torch.isfinite(sds).all() and torch.isfinite(mu).all() and torch.isfinite(sd).all())
    assert torch.equal(_bits(mus[0]), _bits(mus[2])) and torch.equal(_bits(sds[0]), _bits(sds[2]))  # equal members, equal bits
    bad = members(1e12, -8.0)
    with pytest.raises(NotPSDError, match=r"member 1 not positive definite"):
        bad.predict(Xt)
    assert bad.jitter is None and bad._cache is None
    with pytest.raises(NotPSDError, match=r"member 1 "):  # and again: nothing half-built is kept
        bad.predict(Xt, route="composed")

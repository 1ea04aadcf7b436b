"""Hyperparameter ensembles without a GPU: the declarations of gpp_predict_gen / gpp_predict_gen_batched, the three weight modes and
the total-variance formula against numpy long double (tests/ensemble_reference.py), every validation error and refusal (each raised
with the model on the CPU: no device is touched), ``fit(keep_restarts=...)`` refusing on the routes that are not batched before any
work, and the operand helper lifted out of ``BatchedObjective._pre`` against the code it was lifted from.  Every comparison prints
its figures before it asserts."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_reference as cr  # noqa: E402
import ensemble_reference as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"gpp_predict_gen": 15, "gpp_predict_gen_batched": 21}
DT = torch.float64


def _mixed_model(n=40, seed=0, **kw):
    """Two quantitative columns and one categorical column (three levels): the latent map differs from member to member."""
    from gpplus_amd.models import GP_Plus

    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(0, 1, n), rng.uniform(0, 1, n), (np.arange(n) % 3).astype(float)], 1)
    y = np.sin(3 * X[:, 0]) + X[:, 1] + 0.3 * X[:, 2]
    return GP_Plus(torch.tensor(X), torch.tensor(y), qual_dict={2: 3}, dtype=DT, device="cpu", **kw), torch.tensor(X[:5])


def _stacked(model, K, seed=1):
    g = torch.Generator().manual_seed(seed)
    return {n: p.detach().unsqueeze(0) + 0.1 * torch.randn(K, *p.shape, generator=g, dtype=p.dtype)
            for n, p in model.named_parameters() if p.requires_grad}


def test_the_two_symbols_are_declared_exported_and_bound():
    """In a library of their own (include/gpp_ensemble.h, libgpp_ensemble_hip.so): libgpp_hip.so and gpp.h are as they were."""
    from gpplus_amd import _lib

    header = open(os.path.join(ROOT, "include", "gpp_ensemble.h")).read()
    declared = set(re.findall(r"\b(gpp_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib._ENSEMBLE_SIGNATURES), declared ^ set(_lib._ENSEMBLE_SIGNATURES)
    assert not declared & set(_lib.exported_symbols())
    lib = _lib.load_ensemble()
    for name, nargs in SYMBOLS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs, (name, decl.group(1))
        assert len(_lib._ENSEMBLE_SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib._ENSEMBLE_SIGNATURES[name][1]
        # a null handle is refused before anything else is looked at
        assert getattr(lib, name)(*[None if t is _lib.c_void_p else 0 for t in _lib._ENSEMBLE_SIGNATURES[name][1]]) == -1
    assert b"gfx950" in lib.gpp_ensemble_version() and b"src " in lib.gpp_ensemble_version()
    # batch * ceil(N / 64) * M * 2 doubles
    assert lib.gpp_predict_gen_workspace_bytes(130, 70, 5) == 5 * 3 * 70 * 2 * 8
    assert lib.gpp_predict_gen_workspace_bytes(64, 1, 1) == 1 * 1 * 1 * 2 * 8
    assert lib.gpp_predict_gen_workspace_bytes(0, 1, 1) == 0


def test_weight_modes_against_numpy():
    from gpplus_amd.ensemble import mixture_weights

    losses = torch.tensor([0.31, 0.30, 0.305, 0.42], dtype=DT)
    for n in (1, 60, 500):
        got = mixture_weights("posterior", losses, n, 4).numpy()
        ref = E.posterior_weights(losses.numpy(), n)
        err = float(np.abs(got.astype(E.LD) - ref).max())
        print(f"posterior weights n={n}: {got}, max error {err:.3e}")
        assert err <= 8 * 2.0 ** -53 and abs(float(got.sum()) - 1.0) <= 4 * 2.0 ** -53
        assert int(got.argmax()) == 1
    # a gap large enough to underflow every weight but one: exp(-500 * 2) = 0 in fp64, and nothing becomes NaN
    got = mixture_weights("posterior", torch.tensor([3.0, 1.0, 5.0], dtype=DT), 500, 3)
    print("underflowing weights:", got.tolist())
    assert got.tolist() == [0.0, 1.0, 0.0]
    assert mixture_weights("uniform", None, None, 4).tolist() == [0.25] * 4
    got = mixture_weights(torch.tensor([2.0, 0.0, 6.0]), None, None, 3)
    assert np.allclose(got.numpy(), [0.25, 0.0, 0.75], rtol=0, atol=2.0 ** -52) and got.dtype == DT
    for bad, msg in (([1.0, -1.0, 1.0], "non-negative"), ([0.0, 0.0, 0.0], "positive sum"), ([1.0, float("nan"), 1.0], "finite"),
                     ([1.0, 1.0], "2 weights for 3")):
        with pytest.raises(ValueError, match=msg):
            mixture_weights(torch.tensor(bad), None, None, 3)
    with pytest.raises(ValueError, match="posterior"):
        mixture_weights("laplace", losses, 10, 4)
    with pytest.raises(ValueError, match="needs the losses"):
        mixture_weights("posterior", None, 10, 4)
    with pytest.raises(ValueError, match="num_data"):
        mixture_weights("posterior", losses, 0, 4)


def test_total_variance_against_brute_force_moments():
    from gpplus_amd.ensemble import mixture_moments

    rng = np.random.default_rng(3)
    K, M = 7, 33
    mu, var = rng.normal(2.0, 1.5, (K, M)), rng.uniform(1e-6, 2.0, (K, M))
    pi = rng.uniform(0, 1, K)
    pi[2] = 0.0
    pi /= pi.sum()
    m, v = mixture_moments(torch.tensor(pi), torch.tensor(mu), torch.tensor(var))
    rm, rv = E.mixture(pi, mu, var)
    bm, bv = E.mixture_brute(pi, mu, var)
    # the raw second moment is of size mu^2 + var: that is the scale both forms are exact to
    scale = float((np.abs(mu) ** 2 + var).max())
    e_ref = float(np.abs(rv - bv).max())
    e_m, e_v = float(np.abs(m.numpy().astype(E.LD) - rm).max()), float(np.abs(v.numpy().astype(E.LD) - rv).max())
    print(f"mixture: law of total variance against raw moments {e_ref:.3e}; torch against long double: mean {e_m:.3e}, var {e_v:.3e} "
          f"(scale {scale:.3e})")
    assert e_ref <= 1e-15 * scale and float(np.abs(rm - bm).max()) == 0.0
    assert e_m <= 4 * K * 2.0 ** -53 * float(np.abs(mu).max()) and e_v <= 8 * K * 2.0 ** -53 * scale
    # one member: the mixture is that member
    m1, v1 = mixture_moments(torch.ones(1, dtype=DT), torch.tensor(mu[:1]), torch.tensor(var[:1]))
    assert torch.equal(m1, torch.tensor(mu[0])) and torch.equal(v1, torch.tensor(var[0]))


def test_validation_errors_are_raised_on_the_host():
    from gpplus_amd.ensemble import HyperparameterEnsemble as HE

    m, _ = _mixed_model()
    good = _stacked(m, 3)
    names = sorted(good)
    ens = HE(m, good, weights="uniform")
    assert len(ens) == 3 and ens.losses is None and ens.weights.tolist() == [1 / 3] * 3 and ens.num_data == 40
    assert list(ens.states) == [n for n, p in m.named_parameters() if p.requires_grad]
    # a list of state dicts is the same ensemble
    as_list = [{n: good[n][b] for n in good} for b in range(3)]
    ens_l = HE(m, as_list, losses=[0.3, 0.1, 0.2], num_data=40)
    assert all(torch.equal(ens_l.states[n], ens.states[n]) for n in names)
    assert torch.equal(ens_l.losses, torch.tensor([0.3, 0.1, 0.2], dtype=DT)) and int(ens_l.weights.argmax()) == 1
    # state(b): a complete state dict, member b's values in the trainable entries, the model's own elsewhere
    sd = ens.state(1)
    assert set(sd) == set(m.state_dict()) and all(torch.equal(sd[n], good[n][1]) for n in names)
    m.load_state_dict(sd)
    with pytest.raises(IndexError):
        ens.state(3)

    def without(n):
        return {k: v for k, v in good.items() if k != n}

    bad_shape = dict(good)
    bad_shape[names[0]] = good[names[0]][..., None]
    short = dict(good)
    short[names[0]] = good[names[0]][:2]
    nan = dict(good)
    nan[names[-1]] = good[names[-1]].clone()
    nan[names[-1]].view(-1)[0] = float("inf")
    unstacked = {n: v[0] for n, v in good.items()}
    for states, kw, msg in ((without(names[0]), {}, "trainable parameters"),
                            ({**good, "nope": good[names[0]]}, {}, "trainable parameters"),
                            (bad_shape, {}, "stacked as"), (unstacked, {}, "stacked as"), (short, {}, "members where the others"),
                            (nan, {}, "NaN or an inf"), ([], {}, "at least one member"),
                            ({n: v[:0] for n, v in good.items()}, {}, "at least one member"),
                            ([as_list[0], {"x": 1}], {}, "member 1"), (torch.zeros(3), {}, "trainable parameters"),
                            (good, dict(losses=[0.1, 0.2]), "2 losses for 3"),
                            (good, dict(losses=[0.1, float("nan"), 0.3]), "losses must be finite"),
                            (good, dict(), "needs the losses"), (good, dict(weights=[1.0, 2.0]), "2 weights for 3"),
                            (good, dict(weights="best"), "posterior"),
                            (good, dict(losses=[0.1, 0.2, 0.3], num_data=0), "num_data")):
        with pytest.raises(ValueError, match=msg):
            HE(m, states, **kw)


def test_refusals_are_raised_without_a_device(monkeypatch):
    from gpplus_amd import settings
    from gpplus_amd.ensemble import HyperparameterEnsemble as HE
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim import mll_batched

    m, xt = _mixed_model()
    ens = HE(m, _stacked(m, 2), weights="uniform")
    # test rows are validated first, on the host
    with pytest.raises(ValueError, match=r"Xtest must be \(m, 3\)"):
        ens.predict(xt[:, :2])
    with pytest.raises(ValueError, match="finite"):
        ens.predict(torch.full_like(xt, float("nan")))
    unseen = xt.clone()
    unseen[:, 2] = 7.0
    with pytest.raises(ValueError, match="not seen"):
        ens.predict(unseen)
    with pytest.raises(ValueError, match="route"):
        ens.predict(xt, route="gemm")
    # sharded evaluation, then the device: the model sits on the CPU and there is no CPU path
    with settings.sharded_evaluation({"group": None, "nb": 1024}):
        with pytest.raises(NotImplementedError, match="not available under settings.sharded_evaluation"):
            ens.predict(xt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ens.predict(xt)
    # a graph capture (a stand-in for the device: nothing is captured here)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="not available inside a graph capture"):
        ens._refusals("HyperparameterEnsemble.predict", SimpleNamespace(type="cuda"))
    monkeypatch.undo()
    # too many rows for the batched kernels
    monkeypatch.setattr(mll_batched, "BATCHED_MAX_N", 39)
    with pytest.raises(NotImplementedError, match="beyond the batched kernels' range"):
        HE(m, _stacked(m, 2), weights="uniform")
    monkeypatch.undo()
    # a calibrated model
    fx = cr.load_fixture()
    cal = GP_Plus(torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"]), dtype=DT, device="cpu", calibration_id=[2], **cr.C4_KW)
    with pytest.raises(NotImplementedError, match="calibration parameters"):
        HE(cal, _stacked(cal, 2), weights="uniform")
    # the memory rule, with its byte figures: a stand-in context and a device that reports little free memory
    ens._N, ens._K = 1000, 65
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (3 * (ens.cache_bytes() + 3 * 8 * 65 * 1000 * 1008) - 3, 1 << 50))
    with pytest.raises(MemoryError, match=rf"owned cache \({ens.cache_bytes()} bytes\) and the batched workspace \({3 * 8 * 65 * 1000 * 1008} bytes\)"):
        ens._ensure_cache(SimpleNamespace(device=torch.device("cpu")))
    assert ens.cache_bytes() == 8 * 65 * (1000 * 1008 + 1000)


def test_fit_refuses_keep_restarts_where_the_route_is_not_batched(monkeypatch, capsys):
    """Before any work: the model is on the CPU, where a fit that got as far as its device check would raise RuntimeError."""
    from gpplus_amd import settings
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim import fit_model_torch_batched, mll_batched

    m, _ = _mixed_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.restart_ensemble is None
    with pytest.raises(NotImplementedError, match='keep_restarts.*objective="cv" has no batched form'):
        m.fit(optim_type="adam_torch", objective="cv", folds=4, keep_restarts=3)
    with settings.batched_restarts(False):
        with pytest.raises(NotImplementedError, match="settings.batched_restarts is off"):
            m.fit(optim_type="adam_torch", keep_restarts=3)
    monkeypatch.setattr(mll_batched, "BATCHED_MAX_N", 39)
    with pytest.raises(NotImplementedError, match="40 rows are beyond the batched kernels' range"):
        m.fit(optim_type="adam_torch", keep_restarts=3)
    with pytest.raises(NotImplementedError, match="keep is available on the batched restarts only"):
        fit_model_torch_batched(m, num_iter=2, num_restarts=1, keep=2)
    monkeypatch.undo()
    with pytest.raises(NotImplementedError, match="keep is available on the batched restarts only"):
        fit_model_torch_batched(m, num_iter=2, num_restarts=1, objective="cv", folds=4, keep=2)
    fx = cr.load_fixture()
    cal = GP_Plus(torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"]), dtype=DT, device="cpu", calibration_id=[2], **cr.C4_KW)
    with pytest.raises(NotImplementedError, match="calibration parameters"):
        cal.fit(optim_type="adam_torch", keep_restarts=3)
    for bad in (-1,):
        with pytest.raises(ValueError, match="keep_restarts"):
            m.fit(optim_type="adam_torch", keep_restarts=bad)
        with pytest.raises(ValueError, match="keep must be"):
            fit_model_torch_batched(m, keep=bad)
    assert "Learning the model's parameters has started" not in capsys.readouterr().out
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items()) and m.restart_ensemble is None
    # without the keyword the fit gets as far as it always did on a CPU model
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.fit(optim_type="adam_torch")


def _pre_as_it_was(self, params):
    """``BatchedObjective._pre`` as it stood before the operand helper was lifted out of it (the "mll" / "loo" form)."""
    from torch.func import functional_call

    from gpplus_amd.gpcore.kernels import LazyKernelMatrix

    model = self.model
    full = dict(self.fixed)
    full.update(params)
    full.update(self.buffers)
    x = model.train_inputs[0]
    note = {}

    def run(m):
        out = torch.nn.Module.__call__(m, x)
        cov = out.lazy_covariance_matrix
        assert isinstance(cov, LazyKernelMatrix)
        noisy = m.likelihood(out).lazy_covariance_matrix
        prior = out.mean.new_zeros(())
        for _, module, pr, closure, _ in m.named_priors():
            prior = prior + pr.log_prob(closure(module)).sum().to(prior)
        note["static"] = (noisy.grp, cov.spec.kind, cov.spec.d_split)
        return cov.U1, cov.spec.w, cov.spec.sf2.reshape(()), noisy.tau.reshape(-1), out.mean, prior

    class _Shim(torch.nn.Module):
        def __init__(s, inner):
            super().__init__()
            s.inner = inner

        def forward(s):
            return run(s.inner)

    return functional_call(_Shim(model), {"inner." + k: v for k, v in full.items()}, ()), note["static"]


@pytest.mark.parametrize("kind", ["mixed", "two_sources"])
def test_the_lifted_operand_helper_gives_what_the_objective_consumed(kind):
    """On the training rows, bit for bit: through ``BatchedObjective._pre`` (the objective's own call), through the helper with the
    training rows handed over explicitly (the ensemble's call) and through the ensemble itself.  The model sits on the CPU and
    nothing is launched."""
    from gpplus_amd.ensemble import HyperparameterEnsemble as HE
    from gpplus_amd.models import GP_Plus
    from gpplus_amd.optim import BatchedObjective
    from gpplus_amd.optim.mll_batched import member_operands

    if kind == "mixed":
        m, xt = _mixed_model()
    else:
        rng = np.random.default_rng(5)
        X = np.stack([rng.uniform(0, 1, 36), rng.uniform(0, 1, 36), (np.arange(36) % 2).astype(float)], 1)
        m = GP_Plus(torch.tensor(X), torch.tensor(np.sin(3 * X[:, 0]) + 0.4 * X[:, 2]), qual_dict={2: 2}, multiple_noise=True,
                    m_gp="multiple_constant", dtype=DT, device="cpu")
        xt = torch.tensor(X[:5])
    K = 3
    obj = BatchedObjective(m, K)
    theta = _stacked(m, K)
    for n in obj.names:
        obj.theta[n].data.copy_(theta[n])
    static_old = {}

    def old(p):
        tensors, static = _pre_as_it_was(obj, p)
        static_old["v"] = static
        return tensors

    with torch.no_grad():
        was = torch.vmap(old, in_dims=(0,), randomness="error")(dict(obj.theta))
        now = torch.vmap(obj._pre, in_dims=(0,), randomness="error")(dict(obj.theta))
    assert len(was) == len(now) == 6
    for a, b, name in zip(was, now, ("U", "w", "sf2", "tau", "mean", "prior")):
        print(name, tuple(a.shape), "max difference", float((a - b).detach().abs().max()))
        assert a.shape == b.shape and torch.equal(a, b), name
    for a, b in zip(static_old["v"], obj._static):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    # the ensemble: the same tensors at the training rows handed over as rows (log priors left out), whatever a predict() has left
    # in the likelihood's source column
    ens = HE(m, theta, weights="uniform")
    if hasattr(ens._model.likelihood, "fidel_indices"):
        ens._model.likelihood.fidel_indices = xt[:, -1]
    (U, w, sf2, tau, mean), (grp, kind_id, d_split) = ens._operands(ens._model.train_inputs[0])
    for a, b, name in zip(was[:5], (U, w, sf2, tau, mean), ("U", "w", "sf2", "tau", "mean")):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert (kind_id, d_split) == tuple(obj._static[1:])
    assert (grp is None and obj._static[0] is None) or torch.equal(grp, obj._static[0])
    assert ens._shared_features() is False and U.shape == (K, m.train_targets.shape[0], w.shape[1])
    assert float((U[0] - U[1]).abs().max()) > 0  # the latent map differs from member to member
    # at other rows: the features and prior means of those rows, the noise groups of their own sources
    (Ut, _, _, taut, meant), (grpt, _, _) = ens._operands(xt)
    assert Ut.shape == (K, 5, w.shape[1]) and meant.shape[-1] == 5 and torch.equal(taut, tau)
    if kind == "two_sources":
        assert grpt.tolist() == [int(v) for v in xt[:, 2].tolist()] and tau.shape == (K, 2)
        assert float((meant[:, 0] - meant[:, 1]).abs().max()) > 0  # one constant mean per source
    got = member_operands(m, {**obj.fixed, **{n: theta[n][0] for n in obj.names}, **obj.buffers}, m.train_inputs[0], lambda s: None,
                          priors=False)
    assert torch.equal(got[0], was[0][0]) and float(got[5]) == 0.0

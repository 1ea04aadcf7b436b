"""GP_Plus.variance_reduction and select_by_variance_reduction on the GPU, on models built from the committed fixtures with the
parameters tests/test_gpu_condition.py gives them:

    c1  60 training rows, 7 candidates (the next training rows), 33 reference rows (test rows)
    c3  80 training rows, two categorical columns; candidates and reference rows: the other 20
    c4  250 training rows, three sources with a noise and a mean each; candidates: the other 50, reference rows: the source-0 rows
        among them

against (a) tests/alc_reference.py — explicit long-double refits, on c1 from RAW features, targets' scaling and the parameters' closed
forms, on c3 / c4 from the model's own latent features and parameters — and (b) the package's independent route, for every candidate:
sum_r w_r (predict(Xref, include_noise=False) std^2 before - after condition_on(x_c, 0.0)).  Both are held to 1e-10 of sf2 y_std^2,
the bar tests/test_gpu_condition.py holds its outputs to.  Every test prints its observed errors before asserting (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alc_reference as alc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-10
C1_PARAMS = {"covar_module.base_kernel.raw_lengthscale": -1.0, "covar_module.raw_outputscale": 0.3,
             "likelihood.noise_covar.raw_noise": -6.0, "mean_module.constant": 0.4}
_memo = {}


def _load(name):
    return dict(np.load(os.path.join(GOLD, name)))


def _build(fx, tag, n, device="cuda", **kw):
    """tests/test_gpu_condition.py's builder on the first ``n`` rows of a fixture."""
    from gpplus_amd.models import GP_Plus

    xkey = "Xtrain" if "Xtrain" in fx else "Utrain"
    m = GP_Plus(torch.tensor(fx[xkey][:n]), torch.tensor(fx["ytrain"][:n]), dtype=torch.float64, device=device, **kw)
    sd = m.state_dict()
    for k in list(sd):
        fk = f"{tag}::param::{k}"
        if fk in fx:
            sd[k] = torch.as_tensor(fx[fk]).reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    return m


def _c1(device="cuda"):
    from gpplus_amd.models import GP_Plus

    fx = _load("c1_borehole_n500.npz")
    m = GP_Plus(torch.tensor(fx["Xtrain"][:60]), torch.tensor(fx["ytrain"][:60]), dtype=torch.float64, device=device)
    sd = m.state_dict()
    for k, v in C1_PARAMS.items():
        sd[k] = torch.full_like(sd[k], v)
    m.load_state_dict(sd)
    return m, torch.tensor(fx["Xtrain"][60:67]), torch.tensor(fx["Xtest"][:33])


def _c3(device="cuda"):
    fx = _load("c3_borehole_mixed_n100.npz")
    m = _build(fx, "theta1", 80, device, qual_dict={0: 5, 5: 5})
    other = torch.tensor(fx["Utrain"][80:])
    return m, other, other


def _c4(device="cuda"):
    fx = _load("c4_wing_mf_n300.npz")
    m = _build(fx, "theta1", 250, device, qual_dict={10: 3}, multiple_noise=True, m_gp="multiple_constant")
    other = torch.tensor(fx["Xtrain"][250:])
    ref = other[other[:, 10] == 0]
    assert set(other[:, 10].tolist()) == {0.0, 1.0, 2.0} and 5 <= ref.shape[0] < 50
    return m, other, ref


CASES = {"c1": _c1, "c3": _c3, "c4": _c4}


def _noise_rows(m, X):
    """The noise level of each row's own source, from the likelihood's parameters."""
    lik = m.likelihood
    noise = lik.noise_covar.noise.detach().reshape(-1).cpu().numpy().astype(np.float64)
    if noise.size == 1:
        return np.full(X.shape[0], noise[0])
    src = X[:, -1].cpu().numpy()
    out = np.zeros(X.shape[0])
    for k, lvl in enumerate(lik.noise_indices):
        out[src == lvl] = noise[k]
    return out


def _operands(m, Xc, Xr, raw=False, jitter=0.0):
    """What alc_reference needs, on the host: features, noise (with the factorisation's jitter), kernel.  ``raw`` (c1): nothing is
    taken from the model's tensors."""
    if raw:
        fx = _load("c1_borehole_n500.npz")
        w = np.full(8, 10.0 ** C1_PARAMS["covar_module.base_kernel.raw_lengthscale"])  # Rough_RBF: w = 10^x
        sf2 = np.log1p(np.exp(C1_PARAMS["covar_module.raw_outputscale"]))
        noise = np.exp(C1_PARAMS["likelihood.noise_covar.raw_noise"]) + 1e-8 + jitter
        y = fx["ytrain"][:60]
        return dict(U=fx["Xtrain"][:60], noise=np.full(60, noise), Uc=Xc.numpy(), noise_c=np.full(Xc.shape[0], noise), Ur=Xr.numpy(),
                    w=w, sf2=sf2, kind=0, d_split=0), float((y.max() - y.min()) ** 2)
    dev = m.train_inputs[0].device
    with torch.no_grad():
        feats = [m._features(X.to(dev))[0].detach().cpu().numpy().astype(np.float64) for X in (m.train_inputs[0], Xc, Xr)]
        spec = m.covar_module(m._features(m.train_inputs[0])[0]).spec
    ops = dict(U=feats[0], noise=_noise_rows(m, m.train_inputs[0]) + jitter, Uc=feats[1], noise_c=_noise_rows(m, Xc) + jitter, Ur=feats[2],
               w=spec.w.detach().cpu().numpy().astype(np.float64), sf2=float(spec.sf2), kind=int(spec.kind), d_split=int(spec.d_split))
    return ops, float(m.y_std) ** 2


def _reference(name, m, Xc, Xr, omega, jitter):
    key = (name, None if omega is None else omega.tobytes(), jitter)
    if key not in _memo:
        ops, scale = _operands(m, Xc, Xr, raw=(name == "c1"), jitter=jitter)
        _memo[key] = (alc.score_by_refit(omega=omega, **ops) * scale, ops, scale)
    return _memo[key]


def _snapshot(m):
    c = m.prediction_strategy
    return [v.clone() for v in m.state_dict().values()] + [m.train_inputs[0].clone(), m.train_targets.clone()] + \
        ([] if c is None else [c.L.clone(), c.Linv.clone(), c.alpha.clone(), c.z.clone(), c.U.clone()])


def _weighted_variance(m, Xr, omega):
    _, std = m.predict(Xr, return_std=True, include_noise=False)
    return float((omega * std.double() ** 2).sum())


@pytest.mark.parametrize("name", ["c1", "c3", "c4"])
@pytest.mark.parametrize("weighted", [False, True])
def test_scores_against_refits_and_against_condition_on(gpu_ctx, name, weighted):
    m, Xc, Xr = CASES[name]()
    Mc, Mr = Xc.shape[0], Xr.shape[0]
    omega = np.random.default_rng(11).uniform(0.0, 2.0, size=Mr) if weighted else None
    m.predict(Xr[:3], return_std=True)  # a warm cache: the calls below reuse it
    cache = m.prediction_strategy
    snap = _snapshot(m)
    got = m.variance_reduction(Xc, Xr, weights=None if omega is None else torch.tensor(omega))
    assert got.shape == (Mc,) and got.dtype == torch.float64 and m.prediction_strategy is cache and not m.training
    again = m.variance_reduction(Xc, Xr, weights=None if omega is None else torch.tensor(omega))
    assert torch.equal(got, again)
    ref, ops, scale = _reference(name, m, Xc, Xr, omega, float(cache.jitter))
    bar = TOL * ops["sf2"] * scale
    g = got.cpu().numpy().astype(np.longdouble)
    e_ref = float(np.abs(g - ref).max())
    om = torch.full((Mr,), 1.0 / Mr, dtype=torch.float64, device="cuda") if omega is None else torch.tensor(omega, device="cuda")
    before = _weighted_variance(m, Xr, om)
    own = np.array([before - _weighted_variance(m.condition_on(Xc[c:c + 1], torch.zeros(1, dtype=torch.float64)), Xr, om)
                    for c in range(Mc)])
    e_own = float(np.abs(got.cpu().numpy() - own).max())
    print(f"{name} weighted {weighted}: scores in [{float(g.min()):.3e}, {float(g.max()):.3e}], bar {bar:.3e}: "
          f"against refits {e_ref:.2e}, against condition_on {e_own:.2e}")
    assert np.all(g > 0) and e_ref <= bar and e_own <= bar, (e_ref, e_own, bar)
    for a, b in zip(snap, _snapshot(m)):
        assert torch.equal(a, b), "the receiver changed"


@pytest.mark.parametrize("name,with_cost", [("c1", False), ("c3", False), ("c3", True), ("c4", True)])
def test_greedy_batch_of_five(gpu_ctx, name, with_cost):
    from gpplus_amd.bayesian_optimizations import select_by_variance_reduction

    m, Xc, Xr = CASES[name]()
    Mc, Mr, q = Xc.shape[0], Xr.shape[0], 5
    cost = None
    if with_cost:  # c4: the price of each candidate's source; c3: any positive numbers
        cost = np.array([30.0, 5.0, 1.0])[Xc[:, 10].long().numpy()] if name == "c4" else np.random.default_rng(2).uniform(1.0, 3.0, Mc)
    m.predict(Xr[:3], return_std=True)  # a warm cache
    ops, scale = _operands(m, Xc, Xr, raw=(name == "c1"), jitter=float(m.prediction_strategy.jitter))
    ref_picks, ref_gains, margins = alc.greedy_by_refit(q=q, cost=cost, **ops)
    print(f"{name} cost {with_cost}: reference picks {ref_picks}, margins of the five rounds {['%.2e' % x for x in margins]}")
    assert min(margins) > 1e-6, margins
    snap = _snapshot(m)
    picks, gains = select_by_variance_reduction(m, q, Xc, Xr, cost=None if cost is None else torch.tensor(cost))
    assert picks.dtype == torch.int64 and picks.tolist() == ref_picks, (picks.tolist(), ref_picks)
    bar = TOL * ops["sf2"] * scale
    e_gain = float(np.abs(gains.cpu().numpy().astype(np.longdouble) - ref_gains * scale).max())
    om = torch.full((Mr,), 1.0 / Mr, dtype=torch.float64, device="cuda")
    before = _weighted_variance(m, Xr, om)
    child = m.condition_on(Xc[picks.cpu()], torch.zeros(q, dtype=torch.float64))
    e_sum = abs(float(gains.sum()) - (before - _weighted_variance(child, Xr, om)))
    print(f"{name} cost {with_cost}: gains against refits {e_gain:.2e}, their sum against one condition_on of all five {e_sum:.2e}, "
          f"bar {bar:.2e}")
    assert e_gain <= bar and e_sum <= bar, (e_gain, e_sum, bar)
    # the first round is the single-candidate score, and with a cost the order follows gain / cost while the gains stay undivided
    single = m.variance_reduction(Xc, Xr)
    rank = single if cost is None else single / torch.tensor(cost, device="cuda")
    assert int(torch.argmax(rank)) == int(picks[0]) and torch.equal(single[picks[0]], gains[0])
    if with_cost:
        plain, _ = select_by_variance_reduction(m, q, Xc, Xr)
        assert plain.tolist() != picks.tolist(), "the cost does not change the order in this case"
    for a, b in zip(snap, _snapshot(m)):
        assert torch.equal(a, b), "the receiver changed"


def test_settings_and_argument_errors_on_the_device(gpu_ctx):
    from gpplus_amd import settings
    from gpplus_amd.bayesian_optimizations import select_by_variance_reduction

    m, Xc, Xr = _c1()
    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            m.variance_reduction(Xc, Xr)
        with pytest.raises(NotImplementedError):
            select_by_variance_reduction(m, 2, Xc, Xr)
    for q in (0, 8):
        with pytest.raises(ValueError):
            select_by_variance_reduction(m, q, Xc, Xr)
    with pytest.raises(ValueError):
        m.variance_reduction(Xc, Xr, weights=torch.zeros(33))
    # a cold model is factorised by the call, and all seven candidates may be picked
    assert m.prediction_strategy is None
    picks, gains = select_by_variance_reduction(m, 7, Xc, Xr)
    assert sorted(picks.tolist()) == list(range(7)) and bool((gains > 0).all()) and m.prediction_strategy is not None
    assert bool((gains[1:] <= gains[:-1] * (1 + 1e-12)).all())  # submodular: greedy gains do not grow

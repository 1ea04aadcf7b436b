"""GP_Plus.knowledge_gradient and select_by_knowledge_gradient on the GPU, on the multi-fidelity fixture c4_wing_mf_n300 with the
fixture's parameters (250 training rows, three sources with a noise and a mean each; candidates: the other 50 rows, of every source;
reference rows: the 14 high-fidelity rows among them), against tests/kg_reference.py — dense long double, from the model's own latent
features and parameters.

Bar.  The project holds the posterior cross-covariance c to 1e-10 sf2 (tests/test_gpu_alc.py, tests/test_gpu_condition.py), hence
sigma = c / sqrt(s_c) to 1e-10 sf2 / sqrt(s_c) and the means (of the order sqrt(sf2)) to 1e-10 sqrt(sf2).  The score is a W-weighted
(sum 1) mean of minima over r of m_r + z_k sigma_cr, and a minimum is 1-Lipschitz in the sup norm:
    |KG - ref| <= 1e-10 |y_std| sqrt(sf2) (max_k |z_k| max_c sqrt(sf2 / s_c) + 1).
Every test prints its observed errors before asserting (pytest -s)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_fixture  # noqa: E402
import kg_reference as kg  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-10
Q = 32
COST = np.array([30.0, 5.0, 1.0])  # the price of a run of each source
_memo = {}


def _model():
    m, Xc, Xr = kg_fixture.build_c4("cuda")
    m.predict(Xr[:3], return_std=True)  # a warm cache: the calls below reuse it
    return m, Xc, Xr


def _reference(m, Xc, Xr, key):
    """The reference operands of a model (shared by the tests that use the same model: computed once, never modified)."""
    if key not in _memo:
        ops, sf2, ystd = kg_fixture.operands(m, Xc, Xr, jitter=float(m.prediction_strategy.jitter))
        C, s, mu = kg_fixture.dense_of(ops)
        _memo[key] = (ops, sf2, ystd, C, s, mu)
    return _memo[key]


def _bar(sf2, ystd, s, num_nodes=Q):
    factor = float(np.sqrt(sf2 / s).max())
    zmax = float(np.abs(kg.nodes(num_nodes)[0]).max())
    return TOL * ystd * np.sqrt(sf2) * (zmax * factor + 1.0), factor


def _snapshot(m):
    c = m.prediction_strategy
    return [v.clone() for v in m.state_dict().values()] + [m.train_inputs[0].clone(), m.train_targets.clone()] + \
        ([] if c is None else [c.L.clone(), c.Linv.clone(), c.alpha.clone(), c.z.clone(), c.U.clone()])


def _assert_unchanged(snap, m):
    """Bit for bit, not by value: the triangle of the cached factor's buffer that no kernel writes holds whatever the allocator
    handed out, NaN included, and a NaN does not equal itself."""
    now = _snapshot(m)
    assert len(now) == len(snap)
    for a, b in zip(snap, now):
        assert a.dtype == b.dtype and a.shape == b.shape, "the receiver changed"
        assert torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)), \
            "the receiver changed"


@pytest.mark.parametrize("maximize", [False, True])
def test_scores_against_the_reference(gpu_ctx, maximize):
    m, Xc, Xr = _model()
    cache = m.prediction_strategy
    snap = _snapshot(m)
    got = m.knowledge_gradient(Xc, Xr, maximize=maximize)
    assert got.shape == (50,) and got.dtype == torch.float64 and m.prediction_strategy is cache and not m.training
    assert torch.equal(got, m.knowledge_gradient(Xc, Xr, maximize=maximize, num_nodes=Q)), "a second call differs"
    ops, sf2, ystd, C, s, mu = _reference(m, Xc, Xr, "c4")
    ref = kg.kg_quadrature(C, s, mu, Q, maximize) * ystd
    bar, factor = _bar(sf2, ystd, s)
    g = got.cpu().numpy().astype(np.longdouble)
    err = float(np.abs(g - ref).max())
    print(f"maximize {maximize}: scores in [{float(g.min()):.3e}, {float(g.max()):.3e}] (y units), max_c sqrt(sf2 / s_c) = {factor:.3f}, "
          f"bar {bar:.3e}: against the reference {err:.2e}")
    assert np.all(g >= 0) and float(g.max()) > 1e3 * bar and err <= bar, (err, bar)
    _assert_unchanged(snap, m)
    # other rules: one node scores exactly 0, 64 nodes meet the bar of their own widest node
    assert bool((m.knowledge_gradient(Xc, Xr, maximize=maximize, num_nodes=1) == 0).all())
    g64 = m.knowledge_gradient(Xc, Xr, maximize=maximize, num_nodes=64).cpu().numpy().astype(np.longdouble)
    e64 = float(np.abs(g64 - kg.kg_quadrature(C, s, mu, 64, maximize) * ystd).max())
    print(f"maximize {maximize}: 64 nodes against the reference {e64:.2e}, bar {_bar(sf2, ystd, s, 64)[0]:.3e}")
    assert e64 <= _bar(sf2, ystd, s, 64)[0]


@pytest.mark.parametrize("with_cost", [False, True])
def test_greedy_batch_of_four(gpu_ctx, with_cost):
    from gpplus_amd.bayesian_optimizations import select_by_knowledge_gradient

    m, Xc, Xr = _model()
    q = 4
    cost = COST[Xc[:, 10].long().numpy()] if with_cost else None
    ops, sf2, ystd, C, s, mu = _reference(m, Xc, Xr, "c4")
    ref_picks, ref_gains, margins, _ = kg.greedy_believer(ops["fit"], ops["resid"], ops["Uc"], ops["noise_c"], ops["Ur"], q, Q, cost=cost,
                                                          prior_r=ops["prior_r"])
    print(f"cost {with_cost}: reference picks {ref_picks}, margins of the four rounds {['%.2e' % x for x in margins]}")
    assert min(margins) > 1e-6, margins
    snap = _snapshot(m)
    picks, gains = select_by_knowledge_gradient(m, q, Xc, Xr, cost=None if cost is None else torch.tensor(cost))
    assert picks.dtype == torch.int64 and picks.tolist() == ref_picks, (picks.tolist(), ref_picks)
    bar, _ = _bar(sf2, ystd, s)
    e_gain = float(np.abs(gains.cpu().numpy().astype(np.longdouble) - ref_gains * ystd).max())
    print(f"cost {with_cost}: gains against the reference {e_gain:.2e}, bar {bar:.2e}")
    assert e_gain <= bar, (e_gain, bar)
    # the first round is the single-candidate score, and with a cost the order follows score / cost while the gains stay undivided
    single = m.knowledge_gradient(Xc, Xr)
    rank = single if cost is None else single / torch.tensor(cost, device="cuda")
    assert int(torch.argmax(rank)) == int(picks[0]) and torch.equal(single[picks[0]], gains[0])
    if with_cost:
        plain, _ = select_by_knowledge_gradient(m, q, Xc, Xr)
        assert plain.tolist() != picks.tolist(), "the cost does not change the order in this case"
    _assert_unchanged(snap, m)


def test_maximising_is_minimising_the_negated_targets(gpu_ctx):
    """A model of -y: targets and prior means negated in the scaled units (the constructor would shift -y back into [0, 1], which a
    constant prior mean of 0 for the first source cannot follow).  Its minimising score is this model's maximising score."""
    m, Xc, Xr = _model()
    up = m.knowledge_gradient(Xc, Xr, maximize=True)
    neg, _, _ = kg_fixture.build_c4("cuda")
    sd = neg.state_dict()
    for k in sd:
        if k.startswith("mean_module") and k.endswith(".constant"):
            sd[k] = -sd[k]
    neg.load_state_dict(sd)
    neg.train_targets = -neg.train_targets
    neg.y_scaled = neg.train_targets
    down = neg.knowledge_gradient(Xc, Xr)
    _, sf2, ystd, _, s, _ = _reference(m, Xc, Xr, "c4")
    bar, _ = _bar(sf2, ystd, s)
    err = float((up - down).abs().max())
    print(f"maximising against minimising -y: {err:.2e}, bar {bar:.2e} (scores up to {float(up.max()):.3e})")
    assert float(up.max()) > 1e3 * bar and err <= bar


def test_the_loop_select_condition_score(gpu_ctx):
    from gpplus_amd.bayesian_optimizations import select_by_knowledge_gradient

    m, Xc, Xr = _model()
    cost = torch.tensor(COST[Xc[:, 10].long().numpy()])
    picks, _ = select_by_knowledge_gradient(m, 1, Xc, Xr, cost=cost)
    j = int(picks[0])
    value = kg_fixture.load_c4()["ytrain"][250 + j]  # the run's result
    child = m.condition_on(Xc[j:j + 1], torch.tensor([value]))
    rest = torch.cat([Xc[:j], Xc[j + 1:]])
    got = child.knowledge_gradient(rest, Xr)
    ops, sf2, ystd, C, s, mu = _reference(child, rest, Xr, "c4 + 1")
    assert ops["fit"].U.shape[0] == 251
    ref = kg.kg_quadrature(C, s, mu, Q) * ystd
    bar, factor = _bar(sf2, ystd, s)
    err = float(np.abs(got.cpu().numpy().astype(np.longdouble) - ref).max())
    print(f"after conditioning on candidate {j}: scores up to {float(got.max()):.3e}, factor {factor:.3f}, against a reference fit "
          f"on 251 rows {err:.2e}, bar {bar:.2e}")
    assert got.shape == (49,) and err <= bar
    nxt, _ = select_by_knowledge_gradient(child, 1, rest, Xr, cost=torch.cat([cost[:j], cost[j + 1:]]))
    assert 0 <= int(nxt[0]) < 49


def test_settings_and_argument_errors_on_the_device(gpu_ctx):
    from gpplus_amd import settings
    from gpplus_amd.bayesian_optimizations import select_by_knowledge_gradient

    m, Xc, Xr = kg_fixture.build_c4("cuda")
    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            m.knowledge_gradient(Xc, Xr)
        with pytest.raises(NotImplementedError):
            select_by_knowledge_gradient(m, 2, Xc, Xr)
    for q in (0, 51):
        with pytest.raises(ValueError):
            select_by_knowledge_gradient(m, q, Xc, Xr)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="num_nodes"):
            m.knowledge_gradient(Xc, Xr, num_nodes=bad)
    # a cold model is factorised by the call
    assert m.prediction_strategy is None
    picks, gains = select_by_knowledge_gradient(m, 3, Xc, Xr, num_nodes=16)
    assert len(set(picks.tolist())) == 3 and bool((gains >= 0).all()) and m.prediction_strategy is not None

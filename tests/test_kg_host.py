"""Host side of the knowledge-gradient scores (no GPU): the reference's exact expectation against brute-force integration, its
fantasy route against the quadrature form, the quadrature rule's properties and its accuracy on the multi-fidelity fixture, the C
symbol and its binding, the argument errors of ``knowledge_gradient`` / ``select_by_knowledge_gradient`` on a CPU model, and
``linalg.knowledge_gradient`` (both operand forms) on a stand-in context that does the kernel's work with plain torch.  Every test
prints its observed error before asserting (pytest -s)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_fixture  # noqa: E402
import kg_reference as kg  # noqa: E402
from alc_reference import Fit  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
W, SF2 = np.array([2.0, 1.0, 0.5]), 1.3


def _problem(N=37, Mc=9, Mr=11, seed=3, kind=0, d_split=0):
    rng = np.random.default_rng(seed)
    U, Uc, Ur = rng.uniform(size=(N, 3)), rng.uniform(size=(Mc, 3)), rng.uniform(size=(Mr, 3))
    noise = np.full(N, 0.05)
    noise_c = rng.choice([0.05, 0.2], size=Mc)  # two sources among the candidates
    # (targets flat enough for the reference means to compete: with well-separated means every score is 0)
    y = 0.15 * (np.sin(3.0 * U[:, 0]) + U[:, 1] ** 2 - U[:, 2]) + 0.05 * rng.standard_normal(N)
    return Fit(U, noise, W, SF2, kind, d_split), y, Uc, noise_c, Ur


def test_exact_expectation_against_brute_force():
    """E[min_r (a_r + b_r Z)] by the envelope against the trapezoid rule on 4e5 points of [-12, 12] (h = 6e-5).  The integrand
    is piecewise smooth with at most M_r kinks: the trapezoid error is O(h^2 (max |a| + 12 max |b|)) ~ 1e-8 of the lines' scale, the
    tail beyond 12 is below 1e-30, and Phi / phi are float64.  Bar: 1e-7 of max(|a|, |b|)."""
    rng = np.random.default_rng(5)
    zs = np.linspace(-12.0, 12.0, 400_001)
    pdf = np.exp(-0.5 * zs * zs) / np.sqrt(2.0 * np.pi)
    worst = 0.0
    for trial in range(12):
        n = int(rng.integers(1, 40))
        a, b = rng.uniform(0.0, 2.0, n), rng.standard_normal(n) * rng.choice([0.1, 1.0, 5.0])
        if trial % 3 == 0 and n > 3:  # equal slopes (different and equal intercepts) and zero slopes
            b[1], b[2], a[2] = b[0], b[0], a[0]
            b[3] = 0.0
        if trial == 4:
            b[:] = 0.0
        f = (a[None, :] + b[None, :] * zs[:, None]).min(1) * pdf
        brute = float(((f[1:] + f[:-1]) * 0.5).sum() * (zs[1] - zs[0]))
        err = abs(kg.expected_min_of_lines(a, b) - brute) / max(np.abs(a).max(), np.abs(b).max())
        worst = max(worst, err)
    print(f"exact envelope against brute force: worst {worst:.2e}")
    assert worst <= 1e-7, worst


@pytest.mark.parametrize("kind,d_split", [(0, 0), (1, 1), (2, 2)])
def test_fantasy_route_matches_the_quadrature_form(kind, d_split):
    fit, y, Uc, noise_c, Ur = _problem(kind=kind, d_split=d_split)
    assert len(set(noise_c.tolist())) == 2
    C, s, mu = kg.dense(fit, y, Uc, noise_c, Ur)
    quad = kg.kg_quadrature(C, s, mu, 8)
    fant = kg.kg_by_fantasy(fit, y, Uc, noise_c, Ur, 8)
    err = float(np.abs(quad - fant).max() / np.abs(quad).max())
    print(f"kind {kind}: fantasies against the quadrature form {err:.2e} (scores up to {float(quad.max()):.3e})")
    assert quad.shape == (9,) and float(quad.max()) > 0 and err <= 1e-12, err


def test_rule_is_symmetric_and_scores_are_nonnegative():
    from gpplus_amd.linalg import gauss_hermite_rule

    fit, y, Uc, noise_c, Ur = _problem()
    C, s, mu = kg.dense(fit, y, Uc, noise_c, Ur)
    for Q in (1, 2, 3, 16, 17, 32, 64):
        z, Wt = kg.nodes(Q)
        zl, Wl = gauss_hermite_rule(Q)
        assert np.array_equal(z.astype(np.float64), zl) and np.array_equal(Wt.astype(np.float64), Wl)  # the library's own rule
        assert np.array_equal(z, -z[::-1]) and np.array_equal(Wt, Wt[::-1]) and abs(float(Wt.sum()) - 1.0) <= 1e-15
        assert np.all(Wt > 0) and abs(float((Wt * z * z).sum()) - (1.0 if Q > 1 else 0.0)) <= 1e-13
        g = kg.kg_quadrature(C, s, mu, Q)
        print(f"Q {Q}: smallest score {float(g.min()):.3e}")
        assert np.all(g >= -1e-18)
        if Q == 1:
            assert np.all(g == 0)
        for mx in (False, True):
            assert np.all(kg.kg_exact(C, s, mu, mx) >= -1e-15)


def test_quadrature_accuracy_on_the_multifidelity_fixture():
    """max_c |KG_Q - KG_exact| / max_c KG_exact on c4_wing_mf_n300 (250 training rows; candidates: the other 50 rows, of all three
    sources; reference rows: the 14 high-fidelity rows among them), measured on a CPU:
        Q = 16: 2.66e-2      Q = 32: 2.35e-2      Q = 64: 7.87e-3
    asserted at twice these values (the rule is deterministic: the margin only absorbs libm differences).  The exact best candidate
    (row 40) beats the runner-up by 8.13e-2 of the largest score, more than twice the largest error above, and every rule finds
    it."""
    m, Xc, Xr = kg_fixture.build_c4("cpu")
    assert set(Xc[:, 10].tolist()) == {0.0, 1.0, 2.0} and Xr.shape[0] == 14
    ops, _, _ = kg_fixture.operands(m, Xc, Xr)
    C, s, mu = kg_fixture.dense_of(ops)
    exact = kg.kg_exact(C, s, mu)
    order = np.argsort(-exact)
    gap = float((exact[order[0]] - exact[order[1]]) / exact.max())
    measured = {16: 2.66e-2, 32: 2.35e-2, 64: 7.87e-3}
    print(f"exact best {int(order[0])}, gap to the runner-up {gap:.3e} of the largest score")
    assert gap > 2 * max(measured.values())  # (the exact winner is not within the rule's error of the runner-up)
    for Q, meas in measured.items():
        g = kg.kg_quadrature(C, s, mu, Q).astype(np.float64)
        err = float(np.abs(g - exact).max() / exact.max())
        print(f"Q {Q}: error {err:.3e} of the largest score (measured {meas:.3e}), arg-max {int(np.argmax(g))}")
        assert err <= 2 * meas and int(np.argmax(g)) == int(order[0])


def test_symbol_is_declared_exported_and_bound():
    from gpplus_amd import _lib, backend
    from gpplus_amd.bayesian_optimizations import select_by_knowledge_gradient  # noqa: F401

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_post_cross_min\s*\(", header) and "#define GPP_OP_POST_CROSS_MIN 7" in header
    assert "gpp_post_cross_min" in _lib.exported_symbols() and len(_lib._SIGNATURES["gpp_post_cross_min"][1]) == 21
    lib = _lib.load()
    assert lib.gpp_post_cross_min.argtypes == _lib._SIGNATURES["gpp_post_cross_min"][1]
    assert callable(backend.GppContext.post_cross_min) and backend.OP_POST_CROSS_MIN == 7
    # Q minima per row and tile: 3 x 3 tiles at M_c = 300, M_r = 257
    assert lib.gpp_workspace_bytes(None, backend.OP_POST_CROSS_MIN, 257, 300, 0, 17) >= 9 * 128 * 17 * 8
    assert backend.post_cross_min_workspace_bytes(300, 257, 17) == lib.gpp_workspace_bytes(None, 7, 257, 300, 0, 17)
    assert lib.gpp_workspace_bytes(None, backend.OP_POST_CROSS_MIN, 128, 1, 0, 1) >= 128 * 8


def test_argument_errors_come_before_the_device_on_a_cpu_model():
    from gpplus_amd._lib import GppError
    from gpplus_amd.bayesian_optimizations import select_by_knowledge_gradient
    from gpplus_amd.models import GP_Plus

    fx = dict(np.load(os.path.join(GOLD, "c3_borehole_mixed_n100.npz")))
    X, y = torch.tensor(fx["Utrain"]), torch.tensor(fx["ytrain"])
    m = GP_Plus(X[:80], y[:80], qual_dict={0: 5, 5: 5}, dtype=torch.float64, device="cpu")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    good, ref = X[80:90], X[90:]
    bad_nan, bad_inf, bad_level = good.clone(), good.clone(), good.clone()
    bad_nan[1, 2] = float("nan")
    bad_inf[0, 3] = float("inf")
    bad_level[2, 5] = 9.0
    cases = {"columns": (good[:, :7], ref), "columns of the reference": (good, ref[:, :7]), "empty candidates": (good[:0], ref),
             "empty reference": (good, ref[:0]), "nan": (bad_nan, ref), "inf": (bad_inf, ref), "nan in the reference": (good, bad_nan),
             "level": (bad_level, ref), "level in the reference": (good, bad_level)}
    for what, (Xc, Xr) in cases.items():
        with pytest.raises(ValueError, match="knowledge_gradient|not seen|level"):
            m.knowledge_gradient(Xc, Xr)
        with pytest.raises(ValueError):
            select_by_knowledge_gradient(m, 2, Xc, Xr)
    for Q in (0, -3, 65):
        with pytest.raises(ValueError, match="num_nodes"):
            m.knowledge_gradient(good, ref, num_nodes=Q)
        with pytest.raises(ValueError, match="num_nodes"):
            select_by_knowledge_gradient(m, 2, good, ref, num_nodes=Q)
    for q in (0, -1, 11):
        with pytest.raises(ValueError, match="q must be"):
            select_by_knowledge_gradient(m, q, good, ref)
    cost = torch.ones(10, dtype=torch.float64)
    for bad_cost in (cost[:-1], -cost, 0 * cost):
        with pytest.raises(ValueError, match="cost"):
            select_by_knowledge_gradient(m, 2, good, ref, cost=bad_cost)
    # valid calls reach the device, and there is none
    with pytest.raises(GppError, match="no CPU fallback"):
        m.knowledge_gradient(good, ref, maximize=True, num_nodes=64)
    with pytest.raises(GppError, match="no CPU fallback"):
        select_by_knowledge_gradient(m, 3, good, ref, cost=cost)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items()) and m.train_inputs[0].shape[0] == 80
    # a source the model has not seen, among the candidates or the reference rows
    fx = kg_fixture.load_c4()
    X, y = torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"])
    keep = X[:, 10] != 2
    m = GP_Plus(X[keep], y[keep], qual_dict={10: 3}, multiple_noise=True, m_gp="multiple_constant", dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="not seen"):
        m.knowledge_gradient(X[~keep][:4], X[keep][:5])
    with pytest.raises(ValueError, match="not seen"):
        m.knowledge_gradient(X[keep][:5], X[~keep][:4])


# ---- linalg.knowledge_gradient on a stand-in context -----------------------------------------------------------------------------
class _StubContext:
    """What ``linalg.knowledge_gradient`` asks of a context, in float64 torch on the CPU (RBF only)."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _rbf(Ua, Ub, w, sf2):
        return sf2 * torch.exp(-(((Ua[:, None, :] - Ub[None, :, :]) ** 2) * w).sum(-1))

    def cross_kernel(self, Ua, Ub, w, sf2, out, *, kind=0, d_split=0):
        out.copy_(self._rbf(Ua, Ub, w, sf2))
        return out

    def predict_tn(self, Linv, z, Kns, kss, V, mean_out, var_out):
        V.copy_(Kns.T @ torch.tril(Linv).T)
        mean_out.copy_(V @ z)
        var_out.copy_(kss - (V * V).sum(1))

    def transpose(self, src, dst):
        dst.copy_(src.T)

    def gemm(self, transA, transB, M, N, K, alpha, A, B, beta, C, **kw):
        opA = A[:K, :M].T if transA else A[:M, :K]
        opB = B[:N, :K].T if transB else B[:K, :N]
        C[:M, :N] = beta * C[:M, :N] + alpha * (opA @ opB)

    def post_cross_min(self, Uc, Ur, w, sf2, Vc, Vr, K, m, scale, nodes, out, *, kind=0, d_split=0, transposed=False):
        self.calls.append((K, Ur.shape[0]))
        assert (Vc.shape[0] == K) if transposed else (Vc.shape[1] == K)
        assert Ur.is_contiguous() and m.is_contiguous() and m.numel() == Ur.shape[0] and out.shape == (Uc.shape[0], nodes.numel())
        # entry by entry as the kernel: the dot products one reference row at a time, so that a column's value does not depend on
        # which other columns share the call, then fma-like m + t c and the exact minimum
        P = torch.stack([(Vc.T if transposed else Vc) @ (Vr[:, r] if transposed else Vr[r]) for r in range(Ur.shape[0])], 1)
        C = self._rbf(Uc, Ur, w, sf2) - P
        t = nodes[None, :] * scale[:, None]  # M_c x Q
        out.copy_((m[None, :, None] + C[:, :, None] * t[:, None, :]).min(1).values)
        return out


def _cache(ctx, fit, y):
    from gpplus_amd.backend import square_buffer
    from gpplus_amd.linalg import FactorCache, KernelSpec

    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    U, N = fit.U, fit.U.shape[0]
    w, sf2 = torch.tensor(W), torch.tensor(SF2, dtype=torch.float64)
    L = torch.linalg.cholesky(ctx._rbf(t(U), t(U), w, sf2) + torch.diag(t(fit.noise)))
    Li = torch.linalg.inv(L)
    A, B = square_buffer(N, "cpu"), square_buffer(N, "cpu")
    A.copy_(L.T)
    B.copy_(torch.tril(Li) + torch.tril(Li, -1).T)
    z = Li @ t(y)
    return FactorCache(ctx, A, B, Li.T @ z, t(U), KernelSpec(w, sf2), 0.0, None, z=z, refactor=(t(fit.noise[:1]), None, z.clone()))


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("with_cost", [False, True])
@pytest.mark.parametrize("maximize", [False, True])
def test_linalg_on_a_stand_in_context(monkeypatch, transposed, with_cost, maximize):
    from gpplus_amd import linalg

    fit, y, Uc, noise_c, Ur = _problem(Mc=12, Mr=15)
    N, q, Q = fit.U.shape[0], 4, 16
    cost = np.where(noise_c > 0.1, 1.0, 6.0) if with_cost else None
    ctx = _StubContext()
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    cache = _cache(ctx, fit, y)
    snap = [x.clone() for x in (cache.L, cache.Linv, cache.alpha, cache.z, cache.U)]
    monkeypatch.setattr(linalg, "cross_kernel", lambda Ua, Ub, spec: ctx._rbf(Ua, Ub, spec.w, spec.sf2))
    mu = kg.post_mean(fit, y, Ur)
    mean_r = t(mu)
    first, picks, gains = linalg.knowledge_gradient(cache, t(Uc), t(noise_c), t(Ur), mean_r, q=q, cost=None if cost is None else t(cost),
                                                    maximize=maximize, num_nodes=Q, transposed=transposed)
    assert ctx.calls == [(N + i, 15) for i in range(q)]
    ref_picks, ref_gains, margins, ref_first = kg.greedy_believer(fit, y, Uc, noise_c, Ur, q, Q, cost=cost, maximize=maximize)
    assert min(margins) > 1e-6 and picks.tolist() == ref_picks, (picks.tolist(), ref_picks, margins)
    e1 = float(np.abs(first.numpy() - ref_first).max() / np.abs(ref_first).max())
    e2 = float(np.abs(gains.numpy() - ref_gains).max() / np.abs(ref_gains).max())
    print(f"transposed {transposed} cost {with_cost} maximize {maximize}: picks {ref_picks}, scores {e1:.2e}, gains {e2:.2e}")
    assert bool((first >= 0).all()) and e1 <= 1e-9 and e2 <= 1e-9
    assert torch.equal(first[picks[0]], gains[0])
    if with_cost:  # the costs change the order here, and the gains stay undivided
        plain = kg.greedy_believer(fit, y, Uc, noise_c, Ur, q, Q, maximize=maximize)[0]
        assert plain != ref_picks
    # maximising equals minimising the negated means, bit for bit
    neg, _, _ = linalg.knowledge_gradient(cache, t(Uc), t(noise_c), t(Ur), -mean_r, maximize=not maximize, num_nodes=Q,
                                          transposed=transposed)
    assert torch.equal(neg, first)
    for x, s in zip((cache.L, cache.Linv, cache.alpha, cache.z, cache.U), snap):
        assert torch.equal(x, s)
    with pytest.raises(ValueError):
        linalg.knowledge_gradient(cache, t(Uc), t(noise_c), t(Ur), mean_r, q=13)
    with pytest.raises(ValueError):
        linalg.knowledge_gradient(cache, t(Uc), t(noise_c[:-1]), t(Ur), mean_r)
    with pytest.raises(ValueError):
        linalg.knowledge_gradient(cache, t(Uc), t(noise_c), t(Ur), mean_r[:-1])
    for bad in (0, 65):
        with pytest.raises(ValueError, match="num_nodes"):
            linalg.knowledge_gradient(cache, t(Uc), t(noise_c), t(Ur), mean_r, num_nodes=bad)


@pytest.mark.parametrize("transposed", [False, True])
def test_column_chunks_compose_bit_for_bit(monkeypatch, transposed):
    from gpplus_amd import linalg
    from gpplus_amd.backend import post_cross_min_workspace_bytes

    fit, y, Uc, noise_c, Ur = _problem(Mc=10, Mr=300, seed=8)
    Q, q = 5, 3
    ctx = _StubContext()
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    cache = _cache(ctx, fit, y)
    monkeypatch.setattr(linalg, "cross_kernel", lambda Ua, Ub, spec: ctx._rbf(Ua, Ub, spec.w, spec.sf2))
    mean_r = t(kg.post_mean(fit, y, Ur))
    args = (cache, t(Uc), t(noise_c), t(Ur), mean_r)
    whole = linalg.knowledge_gradient(*args, q=q, num_nodes=Q, transposed=transposed)
    assert [c[1] for c in ctx.calls] == [300] * q
    ctx.calls.clear()
    monkeypatch.setattr(linalg, "KG_WORKSPACE_CAP", post_cross_min_workspace_bytes(10, 128, Q))  # one column tile per launch
    parts = linalg.knowledge_gradient(*args, q=q, num_nodes=Q, transposed=transposed)
    assert [c[1] for c in ctx.calls] == [128, 128, 44] * q
    print(f"transposed {transposed}: {len(ctx.calls) // q} chunks per round, picks {parts[1].tolist()}")
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)


def test_sharded_setting_is_refused():
    from gpplus_amd import linalg, settings

    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            linalg.knowledge_gradient(None, None, None, None, None)

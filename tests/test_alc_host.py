"""Host side of the expected-variance-reduction scores (no GPU): the reference's refit route against the closed form, the greedy
gains against one refit on all picks, the C symbol and its binding, ``variance_reduction``'s and ``select_by_variance_reduction``'s
argument errors on a CPU model, and the greedy loop of ``linalg.variance_reduction`` (both operand forms) on a stand-in context that
does the kernel's work with plain torch."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alc_reference as alc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble
W, SF2 = np.array([2.0, 1.0, 0.5]), 1.3


def _problem(N=37, Mc=9, Mr=11, seed=3):
    rng = np.random.default_rng(seed)
    U, Uc, Ur = rng.uniform(size=(N, 3)), rng.uniform(size=(Mc, 3)), rng.uniform(size=(Mr, 3))
    noise = np.full(N, 0.05)
    noise_c = rng.choice([0.05, 0.2], size=Mc)  # two sources among the candidates
    omega = rng.uniform(0.0, 1.0, size=Mr)
    return U, noise, Uc, noise_c, Ur, omega


@pytest.mark.parametrize("kind,d_split", [(0, 0), (1, 1), (2, 2)])
@pytest.mark.parametrize("weighted", [False, True])
def test_refit_route_matches_the_closed_form(kind, d_split, weighted):
    U, noise, Uc, noise_c, Ur, omega = _problem()
    om = omega if weighted else None
    refit = alc.score_by_refit(U, noise, Uc, noise_c, Ur, W, SF2, kind, d_split, om)
    closed = alc.closed_form(U, noise, Uc, noise_c, Ur, W, SF2, kind, d_split, om)
    err = float(np.abs(refit - closed).max() / np.abs(closed).max())
    print(f"kind {kind} weighted {weighted}: refit against closed form {err:.2e}")
    assert refit.shape == (9,) and np.all(closed > 0) and err <= 1e-12, err


@pytest.mark.parametrize("with_cost", [False, True])
def test_greedy_gains_sum_to_the_batch_reduction(with_cost):
    U, noise, Uc, noise_c, Ur, omega = _problem()
    cost = np.where(noise_c > 0.1, 1.0, 3.0) if with_cost else None
    picks, gains, margins = alc.greedy_by_refit(U, noise, Uc, noise_c, Ur, W, SF2, 4, omega=omega, cost=cost)
    assert len(set(picks)) == 4 and np.all(gains > 0) and all(m > 0 for m in margins)
    total = alc.reduction_of_batch(U, noise, Uc[picks], noise_c[picks], Ur, W, SF2, omega=omega)
    err = float(abs(gains.sum() - total) / abs(total))
    print(f"cost {with_cost}: picks {picks}, sum of gains against one refit on all picks {err:.2e}")
    assert err <= 1e-14, err
    # the first pick is the best single score (per unit cost)
    single = alc.score_by_refit(U, noise, Uc, noise_c, Ur, W, SF2, omega=omega)
    assert picks[0] == int(np.argmax(single if cost is None else single / cost))
    if with_cost:  # the costs change the order here, and the gains stay undivided
        plain = alc.greedy_by_refit(U, noise, Uc, noise_c, Ur, W, SF2, 4, omega=omega)[0]
        assert plain != picks and abs(float(gains[0] - single[picks[0]])) <= 1e-15


def test_symbol_is_declared_exported_and_bound():
    from gpplus_amd import _lib, backend
    from gpplus_amd.bayesian_optimizations import select_by_variance_reduction, thompson_sample  # noqa: F401

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_post_cross_sq\s*\(", header) and "#define GPP_OP_POST_CROSS 6" in header
    assert "gpp_post_cross_sq" in _lib.exported_symbols() and len(_lib._SIGNATURES["gpp_post_cross_sq"][1]) == 18
    lib = _lib.load()
    assert lib.gpp_post_cross_sq.argtypes == _lib._SIGNATURES["gpp_post_cross_sq"][1]
    assert callable(backend.GppContext.post_cross_sq) and backend.OP_POST_CROSS == 6
    # one record of 128 row sums per 128 x 128 tile: 3 x 3 tiles at M_c = 300, M_r = 257
    assert lib.gpp_workspace_bytes(None, backend.OP_POST_CROSS, 257, 300, 0, 0) >= 9 * 128 * 8
    assert lib.gpp_workspace_bytes(None, backend.OP_POST_CROSS, 128, 1, 0, 0) >= 128 * 8


def test_argument_errors_come_before_the_device_on_a_cpu_model():
    from gpplus_amd._lib import GppError
    from gpplus_amd.bayesian_optimizations import select_by_variance_reduction
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
    ones = torch.ones(ref.shape[0], dtype=torch.float64)
    neg = ones.clone()
    neg[3] = -0.1
    cases = {"columns": (good[:, :7], ref, None), "columns of the reference": (good, ref[:, :7], None),
             "empty candidates": (good[:0], ref, None), "empty reference": (good, ref[:0], None),
             "nan": (bad_nan, ref, None), "inf": (bad_inf, ref, None), "nan in the reference": (good, bad_nan, None),
             "level": (bad_level, ref, None), "level in the reference": (good, bad_level, None),
             "negative weights": (good, ref, neg), "zero weights": (good, ref, 0 * ones), "weights length": (good, ref, ones[:-1])}
    for what, (Xc, Xr, wts) in cases.items():
        with pytest.raises(ValueError):
            m.variance_reduction(Xc, Xr, weights=wts)
        with pytest.raises(ValueError):
            select_by_variance_reduction(m, 2, Xc, Xr, weights=wts)
    for q in (0, -1, 11):
        with pytest.raises(ValueError, match="q must be"):
            select_by_variance_reduction(m, q, good, ref)
    cost = torch.ones(10, dtype=torch.float64)
    for bad_cost in (cost[:-1], -cost, 0 * cost):
        with pytest.raises(ValueError, match="cost"):
            select_by_variance_reduction(m, 2, good, ref, cost=bad_cost)
    # valid calls reach the device, and there is none
    with pytest.raises(GppError, match="no CPU fallback"):
        m.variance_reduction(good, ref, weights=ones)
    with pytest.raises(GppError, match="no CPU fallback"):
        select_by_variance_reduction(m, 3, good, ref, cost=cost)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items()) and m.train_inputs[0].shape[0] == 80
    # a source the model has not seen, among the candidates or the reference rows
    fx = dict(np.load(os.path.join(GOLD, "c4_wing_mf_n300.npz")))
    X, y = torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"])
    keep = X[:, 10] != 2
    m = GP_Plus(X[keep], y[keep], qual_dict={10: 3}, multiple_noise=True, m_gp="multiple_constant", dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="not seen"):
        m.variance_reduction(X[~keep][:4], X[keep][:5])
    with pytest.raises(ValueError, match="not seen"):
        m.variance_reduction(X[keep][:5], X[~keep][:4])


# ---- the greedy loop on a stand-in context ---------------------------------------------------------------------------------------
class _StubContext:
    """What ``linalg.variance_reduction`` asks of a context, in float64 torch on the CPU (RBF only)."""

    def __init__(self):
        self.K_seen = []

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

    def post_cross_sq(self, Uc, Ur, w, sf2, Vc, Vr, K, out, *, omega=None, kind=0, d_split=0, transposed=False):
        self.K_seen.append(K)
        assert (Vc.shape[0] == K) if transposed else (Vc.shape[1] == K)
        P = Vc.T @ Vr if transposed else Vc @ Vr.T
        C = self._rbf(Uc, Ur, w, sf2) - P
        out[:Uc.shape[0]] = (C * C) @ (torch.ones(Ur.shape[0], dtype=torch.float64) if omega is None else omega)
        return out


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("with_cost", [False, True])
def test_greedy_loop_on_a_stand_in_context(monkeypatch, transposed, with_cost):
    from gpplus_amd import linalg
    from gpplus_amd.backend import square_buffer
    from gpplus_amd.linalg import FactorCache, KernelSpec

    U, noise, Uc, noise_c, Ur, omega = _problem()
    N, q = U.shape[0], 4
    cost = np.where(noise_c > 0.1, 1.0, 3.0) if with_cost else None
    ctx = _StubContext()
    w, sf2 = torch.tensor(W), torch.tensor(SF2, dtype=torch.float64)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    L = torch.linalg.cholesky(ctx._rbf(t(U), t(U), w, sf2) + torch.diag(t(noise)))
    Li = torch.linalg.inv(L)
    A, B = square_buffer(N, "cpu"), square_buffer(N, "cpu")
    A.copy_(L.T)
    B.copy_(torch.tril(Li) + torch.tril(Li, -1).T)
    r = torch.zeros(N, dtype=torch.float64)
    cache = FactorCache(ctx, A, B, r.clone(), t(U), KernelSpec(w, sf2), 0.0, None, z=r.clone(), refactor=(t(noise[:1]), None, r))
    snap = [x.clone() for x in (cache.L, cache.Linv, cache.alpha, cache.z, cache.U)]
    monkeypatch.setattr(linalg, "cross_kernel", lambda Ua, Ub, spec: ctx._rbf(Ua, Ub, spec.w, spec.sf2))
    first, picks, gains = linalg.variance_reduction(cache, t(Uc), t(noise_c), t(Ur), omega=t(omega), q=q,
                                                    cost=None if cost is None else t(cost), transposed=transposed)
    assert ctx.K_seen == [N, N + 1, N + 2, N + 3]
    ref_first = alc.score_by_refit(U, noise, Uc, noise_c, Ur, W, SF2, omega=omega)
    ref_picks, ref_gains, margins = alc.greedy_by_refit(U, noise, Uc, noise_c, Ur, W, SF2, q, omega=omega, cost=cost)
    assert min(margins) > 1e-6 and picks.tolist() == ref_picks, (picks.tolist(), ref_picks, margins)
    e1 = float(np.abs(first.numpy() - ref_first).max() / np.abs(ref_first).max())
    e2 = float(np.abs(gains.numpy() - ref_gains).max() / np.abs(ref_gains).max())
    print(f"transposed {transposed} cost {with_cost}: scores {e1:.2e}, gains {e2:.2e}")
    assert e1 <= 1e-9 and e2 <= 1e-9
    for x, s in zip((cache.L, cache.Linv, cache.alpha, cache.z, cache.U), snap):
        assert torch.equal(x, s)
    with pytest.raises(ValueError):
        linalg.variance_reduction(cache, t(Uc), t(noise_c), t(Ur), q=10)
    with pytest.raises(ValueError):
        linalg.variance_reduction(cache, t(Uc), t(noise_c[:-1]), t(Ur))


def test_sharded_setting_is_refused():
    from gpplus_amd import linalg, settings

    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            linalg.variance_reduction(None, None, None, None)

"""Host side of appending observations to a fitted GP (no GPU): the reference's block formulas against a dense long-double
factorisation, the C symbol and its binding, ``condition_on``'s argument errors on a CPU model, and the copy / in-place / second-child
ownership rule of ``linalg.append_to_cache`` on a stand-in context that borders the factor with plain torch."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import append_reference as ar  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, 3))
    return ar.rbf(X, X, np.array([2.0, 1.0, 0.5]), 1.3) + LD(0.05) * np.eye(n, dtype=LD), rng


@pytest.mark.parametrize("q", [1, 5])
def test_block_formulas_match_a_dense_factorisation(q):
    N = 37
    K, rng = _spd(N + q, 10 + q)
    r = rng.standard_normal(N + q).astype(LD)
    Lf = ar.chol(K)
    Lif = ar.tri_inv(Lf)
    zf = Lif @ r
    af = Lif.T @ zf
    L = ar.chol(K[:N, :N])
    Li = ar.tri_inv(L)
    z = Li @ r[:N]
    out = ar.bordered(L, Li, z, Li.T @ z, K[:N, N:], K[N:, N:], r[N:])
    for name, got, ref in (("L", out["L"], Lf), ("Linv", out["Linv"], Lif), ("z", out["z"], zf), ("alpha", out["alpha"], af)):
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"q={q} {name}: {err:.2e}")
        assert err <= 1e-15, (name, err)
    # the leading windows are the old factors themselves
    assert np.array_equal(out["L"][:N, :N], L) and np.array_equal(out["Linv"][:N, :N], Li)


def test_symbol_is_declared_exported_and_bound():
    from gpplus_amd import _lib, backend

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_chol_append\s*\(", header) and "#define GPP_OP_APPEND 5" in header
    assert "gpp_chol_append" in _lib.exported_symbols()
    assert len(_lib._SIGNATURES["gpp_chol_append"][1]) == 15
    lib = _lib.load()
    assert lib.gpp_chol_append.argtypes == _lib._SIGNATURES["gpp_chol_append"][1]
    assert callable(backend.GppContext.chol_append) and backend.OP_APPEND == 5
    # the scratch of both routes, without a handle: q <= 16 takes two 16-row strips, q > 16 grows with q
    small = lib.gpp_workspace_bytes(None, backend.OP_APPEND, 1000, 16, 0, 0)
    wide = lib.gpp_workspace_bytes(None, backend.OP_APPEND, 1000, 17, 0, 0)
    assert small == lib.gpp_workspace_bytes(None, backend.OP_APPEND, 1000, 1, 0, 0) > 2 * 16 * 1000 * 8
    assert wide > 2 * 17 * 1000 * 8


def test_argument_errors_come_before_the_device_on_a_cpu_model():
    from gpplus_amd._lib import GppError
    from gpplus_amd.models import GP_Plus

    fx = dict(np.load(os.path.join(GOLD, "c3_borehole_mixed_n100.npz")))
    X, y = torch.tensor(fx["Utrain"]), torch.tensor(fx["ytrain"])
    m = GP_Plus(X[:80], y[:80], qual_dict={0: 5, 5: 5}, dtype=torch.float64, device="cpu")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    bad_nan, bad_inf, bad_level = X[80:83].clone(), y[80:83].clone(), X[80:83].clone()
    bad_nan[1, 2] = float("nan")
    bad_inf[0] = float("inf")
    bad_level[2, 5] = 9.0
    for what, (Xq, yq) in {"columns": (X[80:83, :7], y[80:83]), "length": (X[80:83], y[80:82]), "nan": (bad_nan, y[80:83]),
                           "inf": (X[80:83], bad_inf), "empty": (X[80:80], y[80:80]), "level": (bad_level, y[80:83])}.items():
        with pytest.raises(ValueError):
            m.condition_on(Xq, yq)
    with pytest.raises(GppError, match="no CPU fallback"):  # a valid call reaches the device, and there is none
        m.condition_on(X[80:], y[80:])
    assert m.train_inputs[0].shape[0] == 80 and all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    # a single-noise model reads no source column, even after GPR.predict has left ``fidel_indices`` on its likelihood
    fx = dict(np.load(os.path.join(GOLD, "c1_borehole_n500.npz")))
    X, y = torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"])
    m = GP_Plus(X[:60], y[:60], dtype=torch.float64, device="cpu")
    m.likelihood.fidel_indices = X[:5, -1]
    with pytest.raises(GppError, match="no CPU fallback"):
        m.condition_on(X[60:63], y[60:63])
    # a source the model has not seen
    fx = dict(np.load(os.path.join(GOLD, "c4_wing_mf_n300.npz")))
    X, y = torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"])
    keep = X[:, 10] != 2
    m = GP_Plus(X[keep], y[keep], qual_dict={10: 3}, multiple_noise=True, m_gp="multiple_constant", dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="not seen"):
        m.condition_on(X[~keep][:4], y[~keep][:4])


# ---- the ownership rule on a stand-in context ------------------------------------------------------------------------------------
class _StubContext:
    """What ``append_to_cache`` asks of a context, in float64 torch on the CPU.  ``fail`` makes the next chol_append report info = 1
    with nothing written."""

    def __init__(self):
        self.calls, self.fail = [], 0

    @staticmethod
    def _rbf(Ua, Ub, w, sf2):
        return sf2 * torch.exp(-(((Ua[:, None, :] - Ub[None, :, :]) ** 2) * w).sum(-1))

    def cross_kernel(self, Ua, Ub, w, sf2, out, *, kind=0, d_split=0):
        out.copy_(self._rbf(Ua, Ub, w, sf2))
        return out

    def kernel_build(self, U, w, sf2, tau, grp, out, *, jitter=0.0, kind=0, d_split=0, uplo=0):
        g = torch.zeros(U.shape[0], dtype=torch.long) if grp is None else grp.long()
        out.copy_(self._rbf(U, U, w, sf2) + torch.diag(tau[g] + jitter))
        return out

    def chol_append(self, A, Linv, N, q, k, C, rq, z, alpha, info):
        self.calls.append((A.data_ptr(), N, q))
        assert A.shape[0] >= N + q and Linv.shape[1] >= N + q and z.numel() >= N + q
        if self.fail:
            self.fail -= 1
            info.fill_(1)
            return
        Li = torch.tril(Linv[:N, :N])
        V = (Li @ k).T
        Ls = torch.linalg.cholesky(torch.triu(C) + torch.triu(C, 1).T - V @ V.T)
        Lsi = torch.linalg.inv(Ls)
        W = -Lsi @ (V @ Li)
        zq = Lsi @ (rq - V @ z[:N])
        A[:N, N:N + q], A[N:N + q, N:N + q] = V.T, Ls.T
        Linv[N:N + q, :N], Linv[:N, N:N + q] = W, W.T
        Linv[N:N + q, N:N + q] = Lsi + torch.tril(Lsi, -1).T
        z[N:N + q] = zq
        alpha[:N] += W.T @ zq
        alpha[N:N + q] = Lsi.T @ zq
        info.fill_(0)


def _dense_cache(ctx, U, r, w, sf2, tau, shared):
    """A FactorCache as ``linalg._factorize`` leaves it (upper factor; inverse factor with its mirror), by dense torch on the CPU."""
    from gpplus_amd.backend import square_buffer
    from gpplus_amd.linalg import FactorCache, KernelSpec

    N = U.shape[0]
    L = torch.linalg.cholesky(ctx._rbf(U, U, w, sf2) + tau * torch.eye(N, dtype=torch.float64))
    Li = torch.linalg.inv(L)
    A, B = square_buffer(N, "cpu"), square_buffer(N, "cpu")
    A.copy_(L.T)
    B.copy_(torch.tril(Li) + torch.tril(Li, -1).T)
    z = Li @ r
    ws = SimpleNamespace(epoch=3) if shared else None
    return FactorCache(ctx, A, B, Li.T @ z, U.clone(), KernelSpec(w, sf2), 0.0, ws, z=z, refactor=(tau, None, r.clone()))


def _parent(N, D=3, shared=True):
    g = torch.Generator().manual_seed(5)
    U = torch.rand(N + 40, D, generator=g, dtype=torch.float64)
    y = torch.randn(N + 40, generator=g, dtype=torch.float64)
    w, sf2, tau = torch.tensor([2.0, 1.0, 0.5], dtype=torch.float64), torch.tensor(1.3, dtype=torch.float64), \
        torch.tensor([0.05], dtype=torch.float64)
    ctx = _StubContext()
    mean = torch.full((N + 40,), 0.2, dtype=torch.float64)
    cache = _dense_cache(ctx, U[:N], (y - mean)[:N], w, sf2, tau, shared)
    return ctx, cache, U, y, mean, (w, sf2, tau)


def _append(cache, U, y, mean, tau, lo, hi, reserve):
    from gpplus_amd.linalg import append_to_cache

    return append_to_cache(cache, U[lo:hi], tau, None, mean[lo:hi], y[lo:hi], reserve)


def _check_against_dense(cache, U, y, mean, params):
    w, sf2, tau = params
    n = cache.U.shape[0]
    ref = ar.dense_posterior(U[:n].numpy(), y[:n].numpy(), mean[:n].numpy(), w.numpy(), float(sf2), float(tau))
    err = float(np.abs(cache.alpha.numpy() - ref["alpha"]).max() / np.abs(ref["alpha"]).max())
    assert cache.L.shape == (n, n) and cache.Linv.shape == (n, n) and cache.z.numel() == n and err < 1e-9, err
    d = (torch.triu(cache.Linv) ** 2).sum(1).numpy()  # diag(Ky^-1) off the mirror, as gpp_loo_scalars reads it
    assert float(np.abs(1 / d - ref["loo_var"]).max() / np.abs(ref["loo_var"]).max()) < 1e-9
    assert torch.equal(cache._refactor[2], (y - mean)[:n]) and cache._ws is None and not cache.stale()


def test_ownership_copy_in_place_and_second_child():
    N = 23
    ctx, parent, U, y, mean, params = _parent(N)
    tau = params[2]
    snap = [t.clone() for t in (parent.L, parent.Linv, parent.alpha, parent.z)]
    a = _append(parent, U, y, mean, tau, N, N + 2, reserve=6)          # shared workspace -> copy, capacity N + 8
    assert a.route == "copy" and a._own.capacity == N + 8 and a.L.data_ptr() != parent.L.data_ptr()
    b = _append(a, U, y, mean, tau, N + 2, N + 5, reserve=6)           # owned, filled == extent, fits -> in place
    assert b.route == "in_place" and b.L.data_ptr() == a.L.data_ptr() and b._own is a._own and a._own.filled == N + 5
    b2 = _append(a, U, y, mean, tau, N + 2, N + 4, reserve=6)          # second child of a: somebody appended behind it -> copy
    assert b2.route == "copy" and b2.L.data_ptr() != a.L.data_ptr()
    c = _append(b, U, y, mean, tau, N + 5, N + 8, reserve=6)           # fills the pair exactly
    assert c.route == "in_place" and c._own.filled == c._own.capacity == N + 8
    d = _append(c, U, y, mean, tau, N + 8, N + 9, reserve=0)           # full -> copy
    assert d.route == "copy" and d._own.capacity == N + 9
    for cache in (a, b, b2, c, d):
        _check_against_dense(cache, U, y, mean, params)
        cache.refresh()  # a no-op for an owned cache
    # two children of one parent did not clobber each other, and the first parent is bitwise what it was
    assert torch.equal(b.L[:N + 2, :N + 2], a.L) and torch.equal(b2.Linv[:N + 2, :N + 2], a.Linv)
    for t, s in zip((parent.L, parent.Linv, parent.alpha, parent.z), snap):
        assert torch.equal(t, s)
    assert parent._ws is not None and parent.route is None


def test_failed_schur_complement_and_wide_appends_refactor(monkeypatch):
    from gpplus_amd import linalg

    N = 23
    ctx, parent, U, y, mean, params = _parent(N, shared=False)
    w, sf2, tau = params
    seen = []

    def fake_factorize(U2, spec, tau2, grp2, mean2, r2):
        seen.append(U2.shape[0])
        return _dense_cache(ctx, U2, r2 - mean2, spec.w, spec.sf2, tau2, shared=True)

    monkeypatch.setattr(linalg, "_factorize", fake_factorize)
    ctx.fail = 1
    a = _append(parent, U, y, mean, tau, N, N + 3, reserve=4)
    assert a.route == "refactor" and seen == [N + 3] and a._ws is None and a._own.capacity == N + 7 and len(ctx.calls) == 1
    _check_against_dense(a, U, y, mean, params)
    monkeypatch.setattr(linalg, "APPEND_MAX_Q", 2)
    b = _append(parent, U, y, mean, tau, N, N + 3, reserve=4)  # q above the crossover: no bordering attempted
    assert b.route == "refactor" and len(ctx.calls) == 1
    c = _append(parent, U, y, mean, tau, N, N + 2, reserve=4)
    assert c.route == "copy" and len(ctx.calls) == 2


def test_noise_levels_must_match_the_cache():
    _, parent, U, y, mean, params = _parent(9)
    with pytest.raises(ValueError, match="noise levels"):
        _append(parent, U, y, mean, params[2] * 2, 9, 10, reserve=0)
    longer = torch.cat([params[2], torch.zeros(1, dtype=torch.float64)])  # (the zero-noise group of an unlisted source)
    assert _append(parent, U, y, mean, longer, 9, 10, reserve=0)._refactor[0].numel() == 2


def test_sharded_setting_is_refused():
    from gpplus_amd import settings

    _, parent, U, y, mean, params = _parent(9)
    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            _append(parent, U, y, mean, params[2], 9, 10, reserve=0)

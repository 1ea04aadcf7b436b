"""gpp_chol_append on the GPU, stage by stage against tests/append_reference.py (numpy, long double).

Every stage of the device's result is compared with the reference applied to the device's OWN previous stage, so each comparison
sees one stage's rounding and every bound is a derived one (append_reference, part 2; ``gemm_reference.error_bound`` for V and S):
  V      against (Linv k)^T from the device's Linv window                      error_bound of the product
  Ls     S is not an output: with S_ref = C - V V^T from the device's V, |S_ref - Ls Ls^T| <= error_bound(S) + the Cholesky
         residual bound gamma_{q+1} |Ls| |Ls^T| (Higham, Theorem 10.3)
  Ls^-1  against the long-double inverse of the device's Ls: |X^ - X| <= 4 gamma_{q+1} |X| |L| |X| (append_reference.tri_inv_bound)
  W      against -Ls^-1 (V Linv) from the device's Ls^-1, V, Linv             the two-product bound
  zq, alpha'  against the device's own Ls^-1, V, W, zq                        the dot-product bounds
The setup: L is a real factor from gpp_potrf + gpp_trtri; the buffers have N + q + 2 rows and a leading dimension of N + q + 6,
rounded up to even (every entry point requires an even leading dimension); NaN sits everywhere outside the N x N windows and in
every output beforehand.  Every test prints largest observed / bound before asserting (pytest -s)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import append_reference as ar  # noqa: E402
from gemm_reference import error_bound  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (2, 63, 64, 65, 129, 300)
QS = (1, 2, 15, 16, 17, 64, 65, 130)
QMAX = max(QS)
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def _data(N):
    """Features of N cached and QMAX new points, the full covariance and residuals (float64 numpy), shared by every q."""
    rng = np.random.default_rng(100 + N)
    X = rng.uniform(size=(N + QMAX, 4))
    w = np.array([3.0, 1.5, 0.7, 0.2])
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2 * w).sum(-1)
    K = 1.7 * np.exp(-d2) + 0.05 * np.eye(N + QMAX)
    return K, rng.standard_normal(N + QMAX)


def _bits(t):
    return t.contiguous().view(torch.int64)


class _Problem:
    def __init__(self, ctx, N, q, corner=None):
        from gpplus_amd.backend import rows_buffer, square_buffer

        dev = ctx.device
        K, r = _data(N)
        self.N, self.q, self.ctx = N, q, ctx
        f = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
        # a real factor: potrf + trtri in buffers of their own
        A0, L0, T0 = square_buffer(N, dev), square_buffer(N, dev), square_buffer(N, dev)
        A0.copy_(f(K[:N, :N]))
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        ctx.potrf(A0, L0, info, T0)
        ctx.trtri(A0, L0, T0)
        assert int(info.item()) == 0
        self.ld = N + q + 6 + ((N + q) & 1)
        self.rows = N + q + 2
        self.A = torch.full((self.rows, self.ld), float("nan"), dtype=torch.float64, device=dev)
        self.Li = torch.full((self.rows, self.ld), float("nan"), dtype=torch.float64, device=dev)
        self.A[:N, :N] = torch.triu(A0) + torch.tril(torch.full_like(A0, float("nan")), -1)  # the strict lower triangle is not the factor's
        self.Li[:N, :N] = L0
        self.k = rows_buffer(N, q, dev)
        self.k.copy_(f(K[:N, N:N + q]))
        self.C = square_buffer(q, dev)
        self.C.copy_(f(K[N:N + q, N:N + q] if corner is None else corner))
        self.rq = f(r[N:N + q])
        Lw = torch.tril(L0).cpu().numpy().astype(LD)
        z = Lw @ r[:N].astype(LD)
        self.z0 = np.asarray(z, dtype=np.float64)
        self.a0 = np.asarray(Lw.T @ z, dtype=np.float64)
        self.info = torch.full((1,), -7, dtype=torch.int32, device=dev)
        self.reset_vectors()
        self.A_before, self.Li_before = self.A.clone(), self.Li.clone()

    def reset_vectors(self):
        dev, N = self.ctx.device, self.N
        self.z = torch.full((self.rows,), float("nan"), dtype=torch.float64, device=dev)
        self.alpha = torch.full((self.rows,), float("nan"), dtype=torch.float64, device=dev)
        self.z[:N] = torch.tensor(self.z0, device=dev)
        self.alpha[:N] = torch.tensor(self.a0, device=dev)

    def run(self):
        self.ctx.chol_append(self.A, self.Li, self.N, self.q, self.k, self.C, self.rq, self.z, self.alpha, self.info)
        torch.cuda.synchronize()
        return int(self.info.item())

    def windows_untouched(self):
        N = self.N
        return torch.equal(_bits(self.A[:N, :N]), _bits(self.A_before[:N, :N])) and \
            torch.equal(_bits(self.Li[:N, :N]), _bits(self.Li_before[:N, :N]))

    def outside_is_nan(self):
        n = self.N + self.q
        ok = all(bool(torch.isnan(M[n:, :]).all()) and bool(torch.isnan(M[:, n:]).all()) for M in (self.A, self.Li))
        ok = ok and bool(torch.isnan(self.z[n:]).all()) and bool(torch.isnan(self.alpha[n:]).all())
        # the factor buffer below its diagonal is nobody's: the block under the window and the corner's strict lower triangle
        ok = ok and bool(torch.isnan(self.A[self.N:n, :self.N]).all())
        low = torch.tril(torch.ones(self.q, self.q, dtype=torch.bool, device=self.A.device), -1)
        return ok and bool(torch.isnan(self.A[self.N:n, self.N:n][low]).all())

    def outputs(self):
        N, n = self.N, self.N + self.q
        g = lambda t: t.cpu().numpy()  # noqa: E731
        return dict(V=g(self.A[:N, N:n]).T, Ls=np.triu(g(self.A[N:n, N:n])).T, W=g(self.Li[N:n, :N]), Wm=g(self.Li[:N, N:n]).T,
                    Lsi_buf=g(self.Li[N:n, N:n]), zq=g(self.z[N:n]), alpha=g(self.alpha[:n]), Linv=np.tril(g(self.Li[:N, :N])),
                    k=g(self.k), C=np.triu(g(self.C)) + np.triu(g(self.C), 1).T, rq=g(self.rq))


def _ratio(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all()
    tiny = np.finfo(np.float64).tiny
    return float((err / np.maximum(bound, tiny)).max())


def _stage_ratios(P, o):
    """largest observed / bound of every stage, from the device's own previous stages."""
    N, q = P.N, P.q
    zeros = np.zeros((q, N))
    out = {}
    out["V"] = _ratio(o["V"], ar.stage_V(o["Linv"], o["k"]), error_bound(o["k"].T, o["Linv"].T, 0, 0, 1.0, 0.0, zeros))
    S_ref = ar.stage_S(o["C"], o["V"])
    E_S = error_bound(o["V"], o["V"].T, 0, 0, -1.0, 1.0, o["C"])
    Ls = o["Ls"].astype(LD)
    out["Ls"] = _ratio(np.triu(Ls @ Ls.T), np.triu(S_ref), np.triu(E_S + ar.chol_residual_bound(o["Ls"])) + np.tril(np.ones((q, q)), -1))
    Lsi = np.tril(o["Lsi_buf"])
    out["Lsinv"] = _ratio(Lsi, ar.tri_inv(o["Ls"]), ar.tri_inv_bound(o["Ls"]) + np.triu(np.ones((q, q)), 1))
    out["W"] = _ratio(o["W"], ar.stage_W(Lsi, o["V"], o["Linv"]), ar.two_product_bound(Lsi, o["V"], o["Linv"]))
    out["zq"] = _ratio(o["zq"], ar.stage_zq(Lsi, o["rq"], o["V"], P.z0), ar.zq_bound(Lsi, o["rq"], o["V"], P.z0))
    out["alpha"] = _ratio(o["alpha"], ar.stage_alpha(P.a0, o["W"], o["zq"], Lsi), ar.alpha_bound(P.a0, o["W"], o["zq"], Lsi))
    return out


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("N", NS)
def test_stages_layout_and_repeatability(gpu_ctx, N, q):
    P = _Problem(gpu_ctx, N, q)
    assert P.run() == 0
    assert P.windows_untouched() and P.outside_is_nan()
    o = P.outputs()
    # the mirrors are copies: the new columns of Linv are the new rows transposed, the corner is symmetric
    assert np.array_equal(o["W"], o["Wm"]) and np.array_equal(o["Lsi_buf"], o["Lsi_buf"].T)
    ratios = _stage_ratios(P, o)
    print(f"N={N} q={q} observed/bound: " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for name, v in ratios.items():
        assert v <= 1.0, (name, v)
    # a second launch on the same inputs, outputs NaN again: bit for bit the same
    first = [_bits(t).clone() for t in (P.A, P.Li, P.z, P.alpha)]
    P.A.copy_(P.A_before)
    P.Li.copy_(P.Li_before)
    P.reset_vectors()
    assert P.run() == 0
    for a, b in zip(first, (P.A, P.Li, P.z, P.alpha)):
        assert torch.equal(a, _bits(b))


@pytest.mark.parametrize("N", (65, 300))
def test_skinny_and_wide_routes_agree(gpu_ctx, N):
    """q = 16 runs the dedicated kernels, q = 17 the composed route on the same first 16 points: V's first 16 rows and the leading
    16 x 16 block of Ls Ls^T are the same quantities, each within its own bound of the exact one."""
    P16, P17 = _Problem(gpu_ctx, N, 16), _Problem(gpu_ctx, N, 17)
    assert P16.run() == 0 and P17.run() == 0
    a, b = P16.outputs(), P17.outputs()
    EV = error_bound(a["k"].T, a["Linv"].T, 0, 0, 1.0, 0.0, np.zeros((16, N)))
    rv = float((np.abs(a["V"].astype(LD) - b["V"][:16]) / (2 * EV)).max())
    ES = error_bound(a["V"], a["V"].T, 0, 0, -1.0, 1.0, a["C"]) + ar.chol_residual_bound(a["Ls"])
    ES = ES + (error_bound(b["V"], b["V"].T, 0, 0, -1.0, 1.0, b["C"]) + ar.chol_residual_bound(b["Ls"]))[:16, :16]
    # (the two S differ by the two V: 2 |dV| |V|^T, inside 2 EV |V|^T)
    ES = ES + 2 * (2 * EV) @ np.abs(a["V"]).T.astype(LD)
    La, Lb = a["Ls"].astype(LD), b["Ls"].astype(LD)[:16, :16]
    rs = float((np.abs(La @ La.T - Lb @ Lb.T) / ES).max())
    print(f"N={N} skinny vs wide: V {rv:.3f}  Ls Ls^T {rs:.3f}")
    assert rv <= 1.0 and rs <= 1.0


@pytest.mark.parametrize("q", (2, 17))
def test_zero_corner_reports_leading_minor_one(gpu_ctx, q):
    N = 65
    P = _Problem(gpu_ctx, N, q, corner=np.zeros((q, q)))  # S = -V V^T: its first pivot is not positive
    assert P.run() == 1
    assert P.windows_untouched() and P.outside_is_nan()
    # alpha's first N entries are the caller's: a failed append leaves them as they were, on both routes
    assert torch.equal(_bits(P.alpha[:N]), _bits(torch.tensor(P.a0, device=P.alpha.device)))


def test_binding_refuses_before_any_launch(gpu_ctx):
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import NO_WORKSPACE, OP_APPEND

    N, q = 65, 17
    P = _Problem(gpu_ctx, N, q)
    snap = [_bits(t).clone() for t in (P.A, P.Li, P.z, P.alpha)]
    args = dict(A=P.A, Linv=P.Li, N=N, q=q, k=P.k, C=P.C, rq=P.rq, z=P.z, alpha=P.alpha, info=P.info)
    bad = {"rows of A": dict(A=P.A[:N + q - 1]), "columns of Linv": dict(Linv=P.Li[:, :N + q - 1]), "z": dict(z=P.z[:N + q - 1]),
           "alpha": dict(alpha=P.alpha[:N]), "k": dict(k=P.k[:, :q - 1]), "C": dict(C=P.C[:q - 1, :q - 1]), "rq": dict(rq=P.rq[:-1]),
           "odd leading dimension": dict(A=P.A[:, :-1].contiguous()),
           "alignment": dict(Linv=P.Li[:, 1:]), "dtype": dict(k=P.k.float()), "q": dict(q=0)}
    for what, change in bad.items():
        with pytest.raises(GppError):
            gpu_ctx.chol_append(**{**args, **change})
    # too small a workspace on the handle: the C entry point itself reports it and enqueues nothing
    lib, h = gpu_ctx.lib, gpu_ctx.h
    need = lib.gpp_workspace_bytes(h, OP_APPEND, N, q, 0, 0)
    small = torch.empty(need - 512, dtype=torch.uint8, device=gpu_ctx.device)
    try:
        assert lib.gpp_set_workspace(h, small.data_ptr(), small.numel()) == 0
        status = lib.gpp_chol_append(h, P.A.data_ptr(), P.ld, P.Li.data_ptr(), P.ld, N, q, P.k.data_ptr(), P.k.stride(0),
                                     P.C.data_ptr(), P.C.stride(0), P.rq.data_ptr(), P.z.data_ptr(), P.alpha.data_ptr(),
                                     P.info.data_ptr())
        assert status == NO_WORKSPACE
    finally:
        gpu_ctx._ws = None  # the context attaches a workspace of its own at the next call that needs one
        lib.gpp_set_workspace(h, None, 0)
    torch.cuda.synchronize()
    for a, b in zip(snap, (P.A, P.Li, P.z, P.alpha)):
        assert torch.equal(a, _bits(b))
    assert int(P.info.item()) == -7
    assert P.run() == 0  # and the same problem runs once the operands are right

"""Host side of the variance reduction of runs that return y and gradient components (no GPU): the reference's joint refit against the
closed form, the b = 1 case against tests/alc_reference.py, the FLOOR of every model-level case of tests/test_gpu_alc_gradient.py
(|fp64 closed form - long double| / sf2 and max cond(S_c), printed and held to 1e-11: the condition under which the GPU test may ask
for 1e-10), the C symbol and its binding, the argument errors of the three public entries on a CPU model, and
``linalg.variance_reduction_block`` on a stand-in context that does the kernels' work with plain torch (both operand forms, a forced
three-chunk run, and 17 directions: the ``torch.bmm`` route)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alc_gradient_cases as C  # noqa: E402
import alc_gradient_reference as AG  # noqa: E402
import alc_reference as alc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
W, SF2 = np.array([2.0, 1.0, 0.5]), 1.3


def _problem(N=37, Mc=9, Mr=11, seed=3, D=3):
    rng = np.random.default_rng(seed)
    U, Uc, Ur = rng.uniform(size=(N, D)), rng.uniform(size=(Mc, D)), rng.uniform(size=(Mr, D))
    noise = np.full(N, 0.05)
    noise_c = rng.choice([0.05, 0.2], size=Mc)
    omega = rng.uniform(0.0, 1.0, size=Mr)
    return U, noise, Uc, noise_c, Ur, omega


def _kappa(w, sf2, kind, d_split):
    D = len(w)
    split = D if kind == 0 else d_split
    return np.where(np.arange(D) < split, 2.0, 6.0 if kind == 1 else 10.0 / 3.0) * w * sf2


@pytest.mark.parametrize("kind,d_split", [(0, 0), (1, 1), (2, 2)])
@pytest.mark.parametrize("dirs", [(0, 1, 2), (0, 2), (1,)])
@pytest.mark.parametrize("weighted", [False, True])
def test_joint_refit_matches_the_closed_form(kind, d_split, dirs, weighted):
    U, noise, Uc, noise_c, Ur, omega = _problem()
    om = omega if weighted else None
    m = AG.Model(U, noise, W, SF2, kind, d_split)
    gn = np.tile(1e-3 * _kappa(W, SF2, kind, d_split)[list(dirs)], (9, 1)) * np.linspace(1.0, 3.0, 9)[:, None]
    refit = AG.score_by_refit(m, Uc, noise_c, gn, dirs, Ur, om)
    closed, value = AG.closed_form(m, Uc, noise_c, gn, dirs, Ur, om)
    err = float(np.abs(refit - closed).max() / np.abs(closed).max())
    print(f"kind {kind} dirs {dirs} weighted {weighted}: refit against closed form {err:.2e}; the gradient multiplies the gain by "
          f"{float((closed / value).min()):.2f} .. {float((closed / value).max()):.2f}")
    assert refit.shape == (9,) and np.all(value > 0) and np.all(closed >= value) and err <= 1e-12, err
    # the value alone is tests/alc_reference.py's score, and so is the whole thing without a direction
    plain = alc.closed_form(U, noise, Uc, noise_c, Ur, W, SF2, kind, d_split, om)
    assert float(np.abs(value - plain).max() / np.abs(plain).max()) <= 1e-15
    c1, v1 = AG.closed_form(m, Uc, noise_c, np.zeros((9, 0)), (), Ur, om)
    r1 = AG.score_by_refit(m, Uc, noise_c, np.zeros((9, 0)), (), Ur, om)
    assert float(np.abs(c1 - plain).max() / np.abs(plain).max()) <= 1e-15 and float(np.abs(c1 - v1).max() / np.abs(plain).max()) <= 1e-15
    assert float(np.abs(r1 - alc.score_by_refit(U, noise, Uc, noise_c, Ur, W, SF2, kind, d_split, om)).max() / np.abs(plain).max()) <= 1e-15


def test_a_model_with_gradient_observations_refit_against_closed_form():
    U, noise, Uc, noise_c, Ur, omega = _problem()
    kap = _kappa(W, SF2, 2, 1)
    Ug = np.repeat(np.random.default_rng(5).uniform(size=(4, 3)), 2, 0)
    gd = np.tile([0, 2], 4)
    m = AG.Model(U, noise, W, SF2, 2, 1, Ug, gd, 1e-4 * kap[gd])
    gn = np.tile(1e-4 * kap[[1, 2]], (9, 1))
    refit = AG.score_by_refit(m, Uc, noise_c, gn, (1, 2), Ur, omega)
    closed, value = AG.closed_form(m, Uc, noise_c, gn, (1, 2), Ur, omega)
    err = float(np.abs(refit - closed).max() / np.abs(closed).max())
    print(f"with 8 gradient observations in the model: refit against closed form {err:.2e}")
    assert err <= 1e-12 and np.all(closed >= value) and np.all(value > 0)
    bare = AG.closed_form(AG.Model(U, noise, W, SF2, 2, 1), Uc, noise_c, gn, (1, 2), Ur, omega)[0]
    assert float(np.abs(bare - closed).max()) > 1e-6 * float(np.abs(closed).max())  # the model's gradients matter


@pytest.mark.parametrize("name", C.NAMES)
def test_floor_of_the_model_level_cases(name):
    """What fp64 can deliver on the cases of tests/test_gpu_alc_gradient.py: the closed form in float64 numpy against long double."""
    m, Xc, Xr = C.build(name, "cpu")
    ops, scale, p, d0, kappa = C.host_inputs(name, m, Xc, Xr)
    ref = C.reference_model(ops)
    for what, mask in (("all", np.ones(p, dtype=bool)), ("half", C.half_mask(p).numpy())):
        rel, gn = C.run_noise(name, kappa, mask, Xc.shape[0])
        dirs = d0 + rel
        exact, _ = AG.closed_form(ref, ops["Uc"], ops["noise_c"], gn, dirs, ops["Ur"])
        got, _, cond = AG.closed_form(ref, ops["Uc"], ops["noise_c"], gn, dirs, ops["Ur"], fp64=True)
        floor = float(np.abs(got - exact).max() / ops["sf2"])
        print(f"{name} ({ops['U'].shape[0]} rows, {Xc.shape[0]} candidates, {Xr.shape[0]} reference rows, p = {p}) {what} directions "
              f"at noise {C.NOISE_REL[name]:g} of the prior curvature: floor {floor:.2e} of sf2, max cond(S_c) {cond:.1f}, "
              f"scores up to {float(exact.max() / ops['sf2']):.3e} of sf2")
        assert floor <= 1e-11, (name, what, floor)


def test_symbol_is_declared_exported_and_bound():
    from gpplus_amd import _lib, backend, linalg
    from gpplus_amd.bayesian_optimizations import select_run_by_variance_reduction  # noqa: F401

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    assert re.search(r"\bint gpp_post_cross_lin_sq\s*\(", header) and "#define GPP_OP_POST_CROSS_LIN 10" in header
    assert "gpp_post_cross_lin_sq" in _lib.exported_symbols() and len(_lib._SIGNATURES["gpp_post_cross_lin_sq"][1]) == 22
    lib = _lib.load()
    assert lib.gpp_post_cross_lin_sq.argtypes == _lib._SIGNATURES["gpp_post_cross_lin_sq"][1]
    assert callable(backend.GppContext.post_cross_lin_sq) and backend.OP_POST_CROSS_LIN == 10
    # one record of 128 row sums per 128 x 128 tile, as gpp_post_cross_sq
    for Mr, Mf in ((257, 300), (128, 1)):
        assert lib.gpp_workspace_bytes(None, backend.OP_POST_CROSS_LIN, Mr, Mf, 0, 0) == \
            lib.gpp_workspace_bytes(None, backend.OP_POST_CROSS, Mr, Mf, 0, 0) >= 128 * 8
    assert linalg.ALC_GRADIENT_CHUNK_BYTES > 0 and linalg._alc_gradient_chunk_points(20000, 9) >= 1


def test_argument_errors_come_before_the_device_on_a_cpu_model():
    from gpplus_amd._lib import GppError
    from gpplus_amd.bayesian_optimizations import select_run_by_variance_reduction
    from gpplus_amd.gradient_enhanced import GradientEnhancedPosterior

    m, Xc, Xr = C.build("c3", "cpu")
    p = int(m.quant_index.numel())
    post = GradientEnhancedPosterior(m, None)  # (the checks come before anything reads the cache)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    Mc = Xc.shape[0]
    nan_noise = torch.full((p,), 1e-3, dtype=torch.float64)
    nan_noise[0] = float("nan")
    bad = {"gradient=False": dict(gradient=False), "short mask": dict(gradient=[True] * (p - 1)), "long mask": dict(gradient=[True] * (p + 1)),
           "2-D mask": dict(gradient=torch.ones(Mc, p, dtype=torch.bool)), "empty mask": dict(gradient=[False] * p),
           "mask of numbers": dict(gradient=[0.5] * p), "noise without gradient": dict(gradient_noise=1e-3),
           "negative noise": dict(gradient=True, gradient_noise=-1.0), "nan noise": dict(gradient=True, gradient_noise=nan_noise),
           "noise shape": dict(gradient=True, gradient_noise=torch.ones(Mc + 1, p)), "noise length": dict(gradient=True, gradient_noise=torch.ones(p + 1)),
           "weights": dict(gradient=True, weights=torch.zeros(Xr.shape[0])), "weights length": dict(gradient=True, weights=torch.ones(Xr.shape[0] + 1))}
    for what, kw in bad.items():
        for who in (m, post):
            with pytest.raises(ValueError):
                who.variance_reduction(Xc, Xr, **kw)
    for who in (m, post):
        with pytest.raises(ValueError):
            who.variance_reduction(Xc[:, :3], Xr, gradient=True)
        with pytest.raises(ValueError):
            who.variance_reduction(Xc, Xr[:0], gradient=True)
        for kw in (dict(cost_value=0.0), dict(cost_gradient=-1.0), dict(cost_value=torch.ones(Mc + 1)), dict(gradient=None),
                   dict(gradient=[False] * p), dict(cost_gradient=float("nan"))):
            with pytest.raises(ValueError):
                select_run_by_variance_reduction(who, Xc, Xr, **kw)
    # NaN under a False of the mask is not read; valid calls reach the device, and there is none
    mask = C.half_mask(p)
    noise = torch.where(mask, torch.tensor(1e-3, dtype=torch.float64), torch.tensor(float("nan"), dtype=torch.float64))
    for who in (m, post):
        with pytest.raises(GppError, match="no CPU fallback"):
            who.variance_reduction(Xc, Xr, gradient=mask, gradient_noise=noise)
        with pytest.raises(GppError, match="no CPU fallback"):
            select_run_by_variance_reduction(who, Xc, Xr, cost_value=torch.ones(Mc), cost_gradient=3.0)
    with pytest.raises(GppError, match="no CPU fallback"):
        m.variance_reduction(Xc, Xr)  # (the path without the new keywords)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


def test_a_calibrated_model_is_refused():
    from gpplus_amd.models import GP_Plus

    class _Calibrated(GP_Plus):
        def __init__(self):  # (only what the refusal reads)
            pass

        calibration_id = [3]

    with pytest.raises(NotImplementedError, match="calibration"):
        GP_Plus.variance_reduction(_Calibrated(), None, None, gradient=True)


# ---- linalg.variance_reduction_block on a stand-in context -------------------------------------------------------------------------
class _StubContext:
    """What ``linalg.variance_reduction_block`` asks of a context, in float64 torch on the CPU (RBF only)."""

    def __init__(self):
        self.launches = []

    @staticmethod
    def _rbf(Ua, Ub, w, sf2):
        return sf2 * torch.exp(-(((Ua[:, None, :] - Ub[None, :, :]) ** 2) * w).sum(-1))

    def _dx(self, Ua, Ub, w, sf2, d):
        """d/dUa[a, d] sf2 k(Ua_a, Ub_n): M x N."""
        return -2.0 * w[d] * (Ua[:, None, d] - Ub[None, :, d]) * self._rbf(Ua, Ub, w, sf2)

    def cross_kernel_dx(self, Ua, Ub, w, sf2, d0, nd, out, *, kind=0, d_split=0, sel=None):
        full = torch.stack([self._dx(Ua, Ub, w, sf2, d0 + j).T for j in range(nd)], 2)  # N x M x nd
        full = full.reshape(Ub.shape[0], Ua.shape[0] * nd)
        out.copy_(full if sel is None else full[:, sel.flat])
        return out

    def predict_tn(self, Linv, z, Kns, kss, V, mean_out, var_out):
        V.copy_(Kns.T @ torch.tril(Linv).T)
        mean_out.copy_(V @ z)
        var_out.copy_(kss - (V * V).sum(1))

    def point_gram(self, Q, nd, G=None, Gsum=None, *, omega=None):
        assert nd <= 16
        Q3 = Q.unflatten(0, (Q.shape[0] // nd, nd))
        G.copy_(torch.bmm(Q3, Q3.transpose(1, 2)))

    def transpose(self, src, dst):
        dst.copy_(src.T)

    def post_cross_lin_sq(self, Uf, Ur, w, sf2, A, d0, nd, Vf, Vr, K, out, *, omega=None, kind=0, d_split=0, transposed=False):
        self.launches.append((Uf.shape[0], d0, nd, K))
        assert A.shape == (Uf.shape[0], 1 + nd) and ((Vf.shape[0] == K) if transposed else (Vf.shape[1] == K))
        P = Vf.T @ Vr if transposed else Vf @ Vr.T
        g = A[:, :1] * self._rbf(Uf, Ur, w, sf2)
        for j in range(nd):
            g = g + A[:, 1 + j:2 + j] * self._dx(Uf, Ur, w, sf2, d0 + j)
        c = g - P
        out[:Uf.shape[0]] = (c * c) @ (torch.ones(Ur.shape[0], dtype=torch.float64) if omega is None else omega)
        return out


def _stub_cache(ctx, U, noise, w, sf2):
    from gpplus_amd.backend import square_buffer
    from gpplus_amd.linalg import FactorCache, KernelSpec

    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    N = U.shape[0]
    L = torch.linalg.cholesky(ctx._rbf(t(U), t(U), w, sf2) + torch.diag(t(noise)))
    Li = torch.linalg.inv(L)
    A, B = square_buffer(N, "cpu"), square_buffer(N, "cpu")
    A.copy_(L.T)
    B.copy_(torch.tril(Li) + torch.tril(Li, -1).T)
    r = torch.zeros(N, dtype=torch.float64)
    return FactorCache(ctx, A, B, r.clone(), t(U), KernelSpec(w, sf2), 0.0, None, z=r.clone(), refactor=(t(noise[:1]), None, r))


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dirs,chunks", [((0, 1, 2), 1), ((0, 2), 1), ((1,), 1), ((0, 1, 2), 3)])
def test_block_scores_on_a_stand_in_context(monkeypatch, transposed, dirs, chunks):
    from gpplus_amd import linalg
    from gpplus_amd.backend import row_stride

    U, noise, Uc, noise_c, Ur, omega = _problem()
    ctx = _StubContext()
    w, sf2 = torch.tensor(W), torch.tensor(SF2, dtype=torch.float64)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    cache = _stub_cache(ctx, U, noise, w, sf2)
    snap = [x.clone() for x in (cache.L, cache.Linv, cache.alpha, cache.z, cache.U)]
    monkeypatch.setattr(linalg, "cross_kernel", lambda Ua, Ub, spec: ctx._rbf(Ua, Ub, spec.w, spec.sf2))
    if chunks == 3:  # three candidates of four functionals per chunk
        monkeypatch.setattr(linalg, "ALC_GRADIENT_CHUNK_BYTES", 8 * 37 * row_stride(12))
        assert linalg._alc_gradient_chunk_points(37, 4) == 3
    gn = np.tile(1e-3 * _kappa(W, SF2, 0, 0)[list(dirs)], (9, 1)) * np.linspace(1.0, 3.0, 9)[:, None]
    with_g, value = linalg.variance_reduction_block(cache, t(Uc), t(noise_c), t(gn), list(dirs), t(Ur), omega=t(omega), transposed=transposed)
    b, span = 1 + len(dirs), dirs[-1] - dirs[0] + 1
    assert ctx.launches == [(9 * b // chunks, dirs[0], span, 37)] * chunks
    ref, ref_value = AG.closed_form(AG.Model(U, noise, W, SF2), Uc, noise_c, gn, dirs, Ur, omega)
    e1 = float(np.abs(with_g.numpy() - ref).max() / np.abs(ref).max())
    e2 = float(np.abs(value.numpy() - ref_value).max() / np.abs(ref).max())
    print(f"transposed {transposed} dirs {dirs} chunks {chunks}: with the gradient {e1:.2e}, the value alone {e2:.2e}")
    assert e1 <= 1e-9 and e2 <= 1e-9
    for x, s in zip((cache.L, cache.Linv, cache.alpha, cache.z, cache.U), snap):
        assert torch.equal(x, s)
    for bad in ([], [1, 1], [2, 1], [3], [-1]):
        with pytest.raises(ValueError, match="dirs"):
            linalg.variance_reduction_block(cache, t(Uc), t(noise_c), t(gn), bad, t(Ur))
    with pytest.raises(ValueError, match="gnoise"):
        linalg.variance_reduction_block(cache, t(Uc), t(noise_c), t(gn)[:, :0], list(dirs), t(Ur))
    with pytest.raises(ValueError):
        linalg.variance_reduction_block(cache, t(Uc), t(noise_c[:-1]), t(gn), list(dirs), t(Ur))


def test_seventeen_directions_take_the_bmm_route_and_a_singular_block_is_named(monkeypatch):
    from gpplus_amd import linalg
    from gpplus_amd.errors import NotPSDError

    D = 20
    rng = np.random.default_rng(8)
    wv = rng.uniform(0.5, 2.0, size=D) / D
    U, noise, Uc, noise_c, Ur, omega = _problem(N=45, Mc=5, Mr=7, seed=4, D=D)
    ctx = _StubContext()
    w, sf2 = torch.tensor(wv), torch.tensor(SF2, dtype=torch.float64)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    cache = _stub_cache(ctx, U, noise, w, sf2)
    monkeypatch.setattr(linalg, "cross_kernel", lambda Ua, Ub, spec: ctx._rbf(Ua, Ub, spec.w, spec.sf2))
    dirs = list(range(2, 19))  # 17 directions, b = 18: beyond gpp_point_gram
    gn = np.tile(1e-3 * _kappa(wv, SF2, 0, 0)[dirs], (5, 1))
    with_g, value = linalg.variance_reduction_block(cache, t(Uc), t(noise_c), t(gn), dirs, t(Ur), omega=t(omega))
    assert ctx.launches == [(5 * 18, 2, 17, 45)]
    ref, ref_value = AG.closed_form(AG.Model(U, noise, wv, SF2), Uc, noise_c, gn, dirs, Ur, omega)
    e1 = float(np.abs(with_g.numpy() - ref).max() / np.abs(ref).max())
    e2 = float(np.abs(value.numpy() - ref_value).max() / np.abs(ref).max())
    print(f"17 of 20 directions: with the gradient {e1:.2e}, the value alone {e2:.2e}")
    assert e1 <= 1e-9 and e2 <= 1e-9
    gn_bad = gn.copy()
    gn_bad[3, 5] = -10.0  # (the public entries refuse it; here it makes candidate 3's block indefinite)
    with pytest.raises(NotPSDError, match="candidate 3"):
        linalg.variance_reduction_block(cache, t(Uc), t(noise_c), t(gn_bad), dirs, t(Ur))


def test_sharded_setting_is_refused():
    from gpplus_amd import linalg, settings

    with settings.sharded_evaluation({"group": None}):
        with pytest.raises(NotImplementedError):
            linalg.variance_reduction_block(None, None, None, None, None, None)
        with pytest.raises(NotImplementedError):
            linalg.variance_reduction_from_gradient_cache(None, None, None, None)

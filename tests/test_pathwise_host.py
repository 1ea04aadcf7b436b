"""Pathwise posterior draws without a GPU: the spectral sampler against the kernel it represents, the algebra of the dense
reference (``tests/pathwise_reference.py``), the statistical assertions of the GPU model-level test on the reference alone, and
argument validation / seeding of ``gpplus_amd.pathwise``."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pathwise_reference as R


def _spec(w, sf2, kind, d_split):
    return SimpleNamespace(w=torch.as_tensor(w, dtype=torch.float64), sf2=torch.tensor(float(sf2), dtype=torch.float64), kind=kind,
                           d_split=d_split)


@pytest.mark.parametrize("kind", [R.KIND_RBF, R.KIND_MATERN32, R.KIND_MATERN52])
def test_spectral_sampler_reproduces_the_kernel(kind):
    """phi(x)^T phi(x') estimates k(x, x') from F = 65 536 features at 200 random pairs (D = 5, d_split = 3, one zero weight).
    phi(x)^T phi(x') is the mean over f of sf2 (cos(omega_f (x - x')) + cos(omega_f (x + x') + 2 b_f)); the two cosines are
    uncorrelated, with variances <= 1 and 1/2, so the mean has standard deviation <= sf2 sqrt(1.5 / F).  The bound is 6 of those."""
    from gpplus_amd.pathwise import draw_spectral

    rng = np.random.default_rng(100 + kind)
    D, d_split, F, sf2 = 5, 3, 65536, 1.7
    w = rng.uniform(0.3, 2.0, D)
    w[1 if kind == R.KIND_RBF else 4] = 0.0
    omega, phase = draw_spectral(_spec(w, sf2, kind, d_split), D, F, torch.Generator().manual_seed(5 + kind))
    assert omega.shape == (F, D) and phase.shape == (F,) and omega.dtype == torch.float64 and omega.device.type == "cpu"
    assert bool((omega[:, w == 0.0] == 0).all())
    assert 0.0 <= float(phase.min()) and float(phase.max()) < 2 * math.pi
    X, Y = rng.uniform(-1, 1, (200, D)), rng.uniform(-1, 1, (200, D))
    pa = R.rff_matrix(X, omega.numpy(), phase.numpy(), sf2, ld=np.float64)
    pb = R.rff_matrix(Y, omega.numpy(), phase.numpy(), sf2, ld=np.float64)
    est = (pa * pb).sum(1)
    exact = np.array([R.kernel_matrix(X[i:i + 1], Y[i:i + 1], w, sf2, kind, d_split, ld=np.float64)[0, 0] for i in range(200)])
    err = np.abs(est - exact).max()
    bound = 6 * sf2 * math.sqrt(1.5 / F)
    print(f"kind {kind}: max |phi.phi - k| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_reference_spectral_draw_reproduces_the_kernel():
    """The reference's own sampler (numpy) under the same bound: the statistical tests below rest on it."""
    rng = np.random.default_rng(3)
    D, d_split, F, sf2 = 5, 3, 65536, 0.8
    w = rng.uniform(0.3, 2.0, D)
    X, Y = rng.uniform(-1, 1, (200, D)), rng.uniform(-1, 1, (200, D))
    for kind in (R.KIND_RBF, R.KIND_MATERN32, R.KIND_MATERN52):
        omega, phase = R.spectral_draw(w, kind, d_split, F, rng)
        est = (R.rff_matrix(X, omega, phase, sf2, ld=np.float64) * R.rff_matrix(Y, omega, phase, sf2, ld=np.float64)).sum(1)
        exact = np.array([R.kernel_matrix(X[i:i + 1], Y[i:i + 1], w, sf2, kind, d_split, ld=np.float64)[0, 0] for i in range(200)])
        assert np.abs(est - exact).max() <= 6 * sf2 * math.sqrt(1.5 / F)


def _small_problem(kind, seed=0, N=60, D=4):
    rng = np.random.default_rng(seed)
    U = rng.uniform(0, 1, (N, D))
    w = rng.uniform(0.5, 3.0, D)
    noise = np.where(np.arange(N) % 2 == 0, 1e-2, 3e-2)
    y = np.sin(3 * U[:, 0]) + U[:, 1] ** 2
    return R.PathReference(U, y - 0.2, noise, w, 1.3, kind, 2), rng


@pytest.mark.parametrize("kind", [R.KIND_RBF, R.KIND_MATERN52])
def test_reference_training_identity(kind):
    """f_s(X) = y - eps_s - T c_s: the path through the kernel block and the features equals the closed form (K = Ky - T)."""
    ref, rng = _small_problem(kind)
    omega, phase, theta, eps = ref.draw(S=5, F=64, rng=rng)
    c = ref.coef(omega, phase, theta, eps)
    mean = np.full(ref.U.shape[0], 0.2)
    f = ref.paths(ref.U, mean, omega, phase, theta, eps)
    closed = ref.train_identity(eps, c) + torch.as_tensor(mean)
    assert (f - closed).abs().max().item() <= 1e-9 * f.abs().max().item()


def test_reference_mean_of_paths_is_the_posterior_mean_and_variance_formula():
    """Linear algebra, no sampling: with theta = 0 and eps = 0 the path IS the posterior mean, and the RFF-exact variance equals the
    empirical one of the linear map (theta, eps) -> f evaluated on its covariance."""
    ref, rng = _small_problem(R.KIND_MATERN32, seed=4)
    Ua = rng.uniform(0, 1, (7, ref.U.shape[1]))
    mean_a = np.full(7, 0.2)
    omega, phase, theta, eps = ref.draw(S=3, F=32, rng=rng)
    f0 = ref.paths(Ua, mean_a, omega, phase, np.zeros_like(theta), np.zeros_like(eps))
    pm, pv = ref.posterior(Ua, mean_a)
    assert (f0 - pm[None, :]).abs().max().item() <= 1e-10
    # f - E f = (Phi_* - k* Ky^-1 Phi_X) theta - k* Ky^-1 eps: its variance, written out
    Ps, Px = ref.features(Ua, omega, phase), ref.features(ref.U, omega, phase)
    A = ref.solve(ref.kernel(Ua, ref.U).T).T
    lin = Ps - A @ Px
    var = (lin * lin).sum(1) + (A * A * ref.noise[None, :]).sum(1)
    assert torch.allclose(var, ref.rff_variance(Ua, omega, phase), rtol=1e-9, atol=1e-13)
    assert (pv > 0).all()


@pytest.fixture(scope="module")
def c1():
    return R.c1_problem()


def test_c1_problem_matches_the_oracle_kernel(c1):
    o, ref = c1["oracle"], c1["ref"]
    K = o.prior_cov(ref.U, ref.U)
    assert (K - ref.K).abs().max().item() <= 1e-12 * c1["sf2"]


def test_model_level_assertions_hold_on_the_reference_alone(c1):
    """The two statistical assertions of tests/test_gpu_pathwise.py::test_model_level_statistics with the reference's own draws,
    same sizes (c1, S = 4096, F = 2048, 64 held-out points): the inputs keep them satisfiable."""
    ref = c1["ref"]
    S, F = 4096, 2048
    omega, phase, theta, eps = ref.draw(S, F, np.random.default_rng(2024))
    f = ref.paths(c1["Ut"], c1["mean_t"], omega, phase, theta, eps)
    pm, pv = ref.posterior(c1["Ut"], c1["mean_t"])
    sd = f.std(0, unbiased=True)
    zmean = ((f.mean(0) - pm).abs() / (sd / math.sqrt(S))).max().item()
    rv = ref.rff_variance(c1["Ut"], omega, phase)
    zvar = ((f.var(0, unbiased=True) / rv - 1.0).abs() / math.sqrt(2.0 / (S - 1))).max().item()
    print(f"reference alone: mean z {zmean:.2f}, variance z {zvar:.2f}, max |rff var / true var - 1| = "
          f"{(rv / pv - 1).abs().max().item():.3f}")
    assert zmean <= 6.0
    assert zvar <= 6.0


def test_device_cosine_polynomial_meets_its_stated_error():
    """gpp_cos_turns of csrc/gpp_apply.hip — fold at a quarter turn, x = 2 pi r', 11 Horner steps in x^2 — re-evaluated with its own
    coefficients (read from the source) and EXACT fused multiply-adds (rational arithmetic, rounded once per operation as the
    hardware does), against cos(2 pi r) in long double: absolute error <= 4 * 2^-53, the figure the apply tests' bound uses."""
    import os
    import re
    from fractions import Fraction

    src = open(os.path.join(os.path.dirname(__file__), "..", "gp-plus_amd", "csrc", "gpp_apply.hip")).read()
    body = src[src.index("GppCosConsts k = {"):src.index("asm volatile", src.index("GppCosConsts k = {"))]
    nums = [float(x) for x in re.findall(r"(-?\d\.\d+e[+-]\d+|-0\.5)[,}]", body)]
    two_pi, c = nums[0], nums[1:]
    assert len(c) == 11 and two_pi == 2 * math.pi and c[-1] == -0.5

    def fma(a, b, d):
        return float(Fraction(a) * Fraction(b) + Fraction(d))  # one rounding

    def cos_turns(r):
        a = abs(r)
        flip = a > 0.25
        x = (0.5 - a if flip else a) * two_pi
        z = x * x
        p = c[0]
        for ci in c[1:]:
            p = fma(p, z, ci)
        p = fma(p, z, 1.0)
        return -p if flip else p

    rng = np.random.default_rng(0)
    rs = np.concatenate([np.linspace(-0.5, 0.5, 4001), rng.uniform(-0.5, 0.5, 8000), 0.25 + rng.uniform(-1e-9, 1e-9, 200)])
    got = np.array([cos_turns(float(r)) for r in rs])
    ld = np.longdouble
    want = np.cos(2 * ld(np.pi) * rs.astype(ld) + 2 * ld(1.2246467991473532e-16) * rs.astype(ld))  # pi = fl(pi) + 1.22e-16
    err = np.abs(got.astype(ld) - want).max()
    print(f"cosine polynomial: max abs error {float(err) / R.U53:.2f} * 2^-53 over {rs.size} arguments")
    assert err <= R.COS_ABS_ERR


def test_draw_spectral_validation_and_seeding():
    from gpplus_amd.pathwise import draw_spectral

    spec = _spec([1.0, 2.0, 0.5], 1.0, R.KIND_MATERN52, 1)
    a = draw_spectral(spec, 3, 16, torch.Generator().manual_seed(1))
    b = draw_spectral(spec, 3, 16, torch.Generator().manual_seed(1))
    c = draw_spectral(spec, 3, 16, torch.Generator().manual_seed(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    with pytest.raises(ValueError):
        draw_spectral(spec, 4, 16)           # D does not match the weights
    with pytest.raises(ValueError):
        draw_spectral(spec, 3, 0)
    with pytest.raises(ValueError):
        draw_spectral(_spec([1.0, -1.0], 1.0, 0, 0), 2, 4)
    with pytest.raises(ValueError):
        draw_spectral(_spec([1.0, 1.0], 1.0, 7, 0), 2, 4)
    with pytest.raises(TypeError):
        draw_spectral(spec, 3, 16, generator=123)


def test_posterior_paths_rejects_bad_arguments_before_touching_the_gpu():
    from gpplus_amd.pathwise import PosteriorPaths

    for kw in ({"size": 0}, {"num_features": 0}, {"generator": "seed"}):
        with pytest.raises((ValueError, TypeError)):
            PosteriorPaths(None, None, **kw)


def test_new_entry_points_are_bound():
    from gpplus_amd import _lib

    assert {"gpp_kernel_apply", "gpp_rff_apply"} <= set(_lib.exported_symbols())

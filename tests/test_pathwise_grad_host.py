"""The gradient reference of tests/pathwise_grad_reference.py without a GPU: against central differences of the generated matrices
in long double, against torch autograd on the dense products, its edge cases (coinciding rows, zero weights), and the condition
that keeps the bound of tests/test_gpu_apply_grad.py meaningful: on every GPU case the bound is at most 1e-9 of the reference."""
import numpy as np
import pytest
import torch

import pathwise_grad_reference as G
import pathwise_reference as R

LD = np.longdouble
KINDS = [("rbf", R.KIND_RBF), ("m32", R.KIND_MATERN32), ("m52", R.KIND_MATERN52)]


def _small(kind, seed=0, M=5, L=7, D=5, d_split=2):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.3, 2.0, D)
    return rng.uniform(-1, 1, (M, D)), rng.uniform(-1, 1, (L, D)), w, 1.3, kind, (0 if kind == R.KIND_RBF else d_split)


@pytest.mark.parametrize("name,kind", KINDS)
def test_kernel_derivative_matches_central_differences(name, kind):
    """dG/dUa[:, d] against (G(ua + h e_d) - G(ua - h e_d)) / 2h in long double, h = 1e-6: truncation h^2 |G'''| / 6 ~ 1e-12, rounding
    2^-64 / h ~ 1e-13 of |G|."""
    Ua, Ub, w, sf2, kind, split = _small(kind)
    h = LD(1e-6)
    for d in range(Ua.shape[1]):
        up, dn = Ua.astype(LD), Ua.astype(LD)
        up[:, d] += h
        dn[:, d] -= h
        fd = (R.kernel_matrix(up, Ub, w, sf2, kind, split) - R.kernel_matrix(dn, Ub, w, sf2, kind, split)) / (2 * h)
        got = G.kernel_dgen(Ua, Ub, w, sf2, kind, split, d)
        assert float(np.abs(got - fd).max()) <= 1e-9 * sf2, (name, d)


def test_feature_derivative_matches_central_differences():
    rng = np.random.default_rng(1)
    Ua, omega, phase, sf2 = rng.uniform(-1, 1, (5, 4)), rng.standard_normal((9, 4)) * 2, rng.uniform(0, 2 * np.pi, 9), 0.7
    h = LD(1e-6)
    for d in range(4):
        up, dn = Ua.astype(LD), Ua.astype(LD)
        up[:, d] += h
        dn[:, d] -= h
        fd = (R.rff_matrix(up, omega, phase, sf2) - R.rff_matrix(dn, omega, phase, sf2)) / (2 * h)
        assert float(np.abs(G.rff_dgen(Ua, omega, phase, sf2, d) - fd).max()) <= 1e-9


@pytest.mark.parametrize("name,kind", KINDS[1:])
def test_matern_multiplier_is_finite_where_rows_coincide(name, kind):
    """r = 0: h' = -3 (Matern 3/2), -5/3 (Matern 5/2); the derivative itself is 0 there, and so are its error terms."""
    Ua, Ub, w, sf2, kind, split = _small(kind)
    Ua[1] = Ub[3]
    m = G.kernel_multipliers(Ua, Ub, w, sf2, kind, split)
    dm = G.kernel_multiplier_errors(Ua, Ub, w, sf2, kind, split)
    assert all(np.isfinite(x).all() for x in m + dm)
    assert float(m[0][1, 3]) == pytest.approx(-sf2) and float(m[1][1, 3]) == pytest.approx(sf2 * (-3.0 if kind == R.KIND_MATERN32 else -5.0 / 3.0))
    for d in range(Ua.shape[1]):
        assert float(G.kernel_dgen(Ua, Ub, w, sf2, kind, split, d)[1, 3]) == 0.0


def _case(cid):
    c = next(c for c in G.cases() if c[0] == cid)
    _, name, M, L, S, D, beta, copies = c
    gen, p = G.case_inputs(name, M, L, S, D, copies)
    return gen, p, beta


def test_zero_weight_column_is_exactly_zero():
    for cid in ("rbf-M65-L65-S17-D8-b0.0", "m52-M65-L65-S17-D17-b1.0"):
        gen, p, _ = _case(cid)
        ref, bound = G.grad_reference(gen, p, 0.0)
        z = np.flatnonzero(p["w"] == 0.0)
        assert z.size == 1
        assert (ref[:, z] == 0).all() and (bound[:, z] == 0).all()
        assert (np.abs(ref[:, p["w"] > 0]).max(0) > 0).all()


@pytest.mark.parametrize("name", ["rbf", "m32", "m52", "rff"])
def test_reference_matches_dense_autograd(name):
    """sum(Gbar o (G C)) built densely in torch fp64 and differentiated by autograd, against the closed form."""
    gen, kind = G.GENS[name]
    p = G.inputs(gen, 9, 21, 4, 6, kind, seed=5)
    if gen != "rff":
        p["Ua"][2] = p["second"][7]  # a row of Ua that is a row of Ub: the autograd reference must stay finite there
    Ua = torch.tensor(p["Ua"], requires_grad=True)
    Ub, C, Gbar, sf2 = torch.tensor(p["second"]), torch.tensor(p["C"]), torch.tensor(p["Gbar"]), p["sf2"]
    if gen == "rff":  # the feature term alone, the kernel term alone
        out = G.dense_path_values(Ua, torch.zeros(1, 6, dtype=torch.float64), torch.ones(6, dtype=torch.float64), sf2, 0, 0, Ub,
                                  torch.tensor(p["phase"]), C, torch.zeros(1, 4, dtype=torch.float64))
    else:
        out = G.dense_path_values(Ua, Ub, torch.tensor(p["w"]), sf2, kind, p["d_split"], torch.zeros(1, 6, dtype=torch.float64),
                                  torch.zeros(1, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64), C)
    (Gbar * out).sum().backward()
    ref, _ = G.grad_reference(gen, p, 0.0)
    err = np.abs(Ua.grad.numpy() - ref.astype(np.float64)).max()
    assert err <= 1e-12 * float(np.abs(ref).max())


def test_bound_is_small_against_the_reference_on_every_gpu_case():
    """So the bound cannot hide a wrong kernel: max_a bound[a, d] <= 1e-9 max_a |ref[a, d]| on every column with w_d > 0."""
    worst = (0.0, None)
    for cid, name, M, L, S, D, beta, copies in G.cases():
        gen, p = G.case_inputs(name, M, L, S, D, copies)
        ref, bound = G.grad_reference(gen, p, 0.0)
        cols = np.arange(D) if p["w"] is None else np.flatnonzero(p["w"] > 0)
        assert np.isfinite(ref).all() and np.isfinite(bound).all(), cid
        ratio = float((bound[:, cols].max(0) / np.abs(ref[:, cols]).max(0)).max())
        worst = max(worst, (ratio, cid))
        assert ratio <= 1e-9, (cid, ratio)
    print(f"largest max bound / max |ref| over {len(G.cases())} cases: {worst[0]:.3e} ({worst[1]})")


def test_gradient_entry_points_are_bound():
    from gpplus_amd import _lib

    assert {"gpp_kernel_apply_grad", "gpp_rff_apply_grad"} <= set(_lib.exported_symbols())

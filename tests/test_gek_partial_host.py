"""Partial gradients without a GPU: the partial reference of tests/gek_partial_reference.py against the dense one (exactly with an
all-True mask; in the limit of a huge noise on the unobserved entries otherwise — an independent pin of the selection), the masks
the model tests use, the validation of ``observed=`` on a CPU model (raised before a device is touched), the 4-tuple of
``gradients=``, ``backend.GradientSelection`` and the new symbols' declarations."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_partial_reference as P  # noqa: E402
import gek_reference as G  # noqa: E402
import gek_train_reference as T  # noqa: E402
import gradpost_reference as gr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("mean", "var", "gmean", "gvar")
_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = G.gek_case(name)
    return _cases[name]


def test_the_pattern_gives_the_stated_counts_and_both_append_routes():
    """2 to 4 components per point and an odd q; c3 and c1-matern52 stay on gpp_chol_append's dedicated q <= 16 kernels, c1 takes the
    composed route (as ``test_the_cases_cover_both_append_routes`` asserts for the dense cases)."""
    qs = {}
    for name, (fixture, _, kw, Mg) in G.GEK_CASES.items():
        p = gr.fixture_test_rows(gr.load_fixture(fixture), 1).shape[1] - len(kw.get("qual_dict", {}))
        m = P.pattern_mask(Mg, p)
        per = m.sum(1)
        assert m.shape == (Mg, p) and int(per.min()) >= 2 and int(per.max()) <= 4, (name, per)
        qs[name] = int(m.sum())
    print(f"observed gradient components per case: {qs}")
    assert (qs["c3"], qs["c1-matern52"], qs["c4"], qs["c1"]) == (5, 7, 12, 17)
    assert all(q % 2 == 1 for q in (qs["c3"], qs["c1-matern52"], qs["c1"]))
    assert qs["c3"] <= 16 and qs["c1-matern52"] <= 16 and qs["c1"] > 16
    # a point the pattern leaves empty gets column 0; one direction (a column mask) is the same everywhere
    assert bool(P.pattern_mask(40, 1).all()) and not bool((((3 * torch.arange(40)) % 7) < 3).all())
    assert P.alternating_row(5).tolist() == [True, False, True, False, True]


@pytest.mark.parametrize("name", ["c3", "c1-matern52", "c4"])
def test_an_all_true_mask_is_the_dense_reference_exactly(name):
    o, X, y, kw, xg, dY, noise, xt = _case(name)
    p = len(o.quant_index)
    dense = G.gek_posterior(o, xg, dY, noise, xt, "joint")
    for mask in (torch.ones(xg.shape[0], p, dtype=torch.bool), torch.ones(p, dtype=torch.bool)):
        part = P.gek_posterior_partial(o, xg, dY, noise, xt, mask)
        for key in dense:
            assert torch.equal(part[key], dense[key]), (name, key)
    a = T.gek_loss_and_grad(o, xg, dY, noise)
    b = P.gek_loss_and_grad_partial(o, xg, dY, noise, torch.ones(xg.shape[0], p, dtype=torch.bool))
    # the value goes through the same operations; the gradient's backward pass goes through the index selection, which adds in
    # another order: rounding noise of an fp64 sum over (N + q)^2 entries, held to 1e-11 of the largest entry
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert float((a[1][k] - b[1][k]).abs().max()) <= 1e-11 * float(a[1][k].abs().max()), k


@pytest.mark.parametrize("name", ["c3", "c1-matern52", "c4"])
def test_the_selection_is_the_limit_of_a_huge_noise_on_the_unobserved_entries(name):
    """An observation with noise variance ratio x (prior curvature) carries at most 1 / ratio of the information of an exact one, so
    the dense posterior with that noise on the unobserved entries (and 0 for their dY) tends to the partial one like 1 / ratio:
    within 2 / ratio of max|reference| on every output, falling by 1000 x between ratio = 1e6 and 1e9."""
    o, X, y, kw, xg, dY, noise, xt = _case(name)
    Mg, p = dY.shape
    mask = P.pattern_mask(Mg, p)
    poisoned = torch.where(mask, dY, torch.full_like(dY, float("nan")))  # what lies under a False entry is never used
    part = P.gek_posterior_partial(o, xg, poisoned, noise, xt, mask)
    worst = {}
    for ratio in (1e6, 1e9):
        big = G.prior_curvature_noise(o, ratio)
        dense = G.gek_posterior(o, xg, torch.where(mask, dY, torch.zeros_like(dY)), torch.where(mask, noise.expand(Mg, p), big.expand(Mg, p)),
                                xt, "joint")
        worst[ratio] = max(float((dense[k] - part[k]).abs().max() / part[k].abs().max()) for k in KEYS)
        print(f"{name} ratio {ratio:g}: dense with a huge noise against the partial reference: {worst[ratio] * ratio:.3f} / ratio")
        assert worst[ratio] <= 2.0 / ratio, (name, ratio, worst[ratio])
    # the selection matters: the partial posterior is not the dense one
    full = G.gek_posterior(o, xg, dY, noise, xt, "joint")
    assert float((full["mean"] - part["mean"]).abs().max()) > 1e-6 * float(part["mean"].abs().max())


def _cpu_model():
    from gpplus_amd.models import GP_Plus

    fx = gr.load_fixture("c3_borehole_mixed_n100.npz")
    X, y = torch.tensor(fx["Utrain"]), torch.tensor(fx["ytrain"])
    return GP_Plus(X[:80], y[:80], qual_dict={0: 5, 5: 5}, dtype=torch.float64, device="cpu"), X


def test_the_mask_is_validated_before_the_device_on_a_cpu_model():
    from gpplus_amd._lib import GppError

    m, X = _cpu_model()
    good, dY = X[80:84], torch.ones(4, 6, dtype=torch.float64)
    mask = P.pattern_mask(4, 6)
    empty_row = mask.clone()
    empty_row[2] = False
    bad = {"columns": torch.ones(4, 5, dtype=torch.bool), "rows": torch.ones(3, 6, dtype=torch.bool),
           "3-d": torch.ones(1, 4, 6, dtype=torch.bool), "float": torch.full((4, 6), 0.5), "int 2": 2 * mask.to(torch.int64),
           "empty row": empty_row, "nothing": torch.zeros(6, dtype=torch.bool)}
    for what, ob in bad.items():
        with pytest.raises(ValueError, match="observed"):
            m.condition_on_gradients(good, dY, observed=ob)
    with pytest.raises(ValueError, match="gradient point 2 has no observed component"):
        m.condition_on_gradients(good, dY, observed=empty_row)
    # NaN / inf under a False entry are not read, in dY and in the noise; under a True entry they are refused
    nan_off = torch.where(mask, dY, torch.full_like(dY, float("nan")))
    nz_off = torch.where(mask, torch.full_like(dY, 1e-3), torch.full_like(dY, float("inf")))
    nan_on = dY.clone()
    nan_on[tuple(mask.nonzero()[0])] = float("nan")
    neg_on = torch.full_like(dY, 1e-3)
    neg_on[tuple(mask.nonzero()[0])] = -1.0
    valid = [dict(observed=mask), dict(observed=mask.to(torch.int32)), dict(observed=mask.numpy()), dict(observed=mask[0]),
             dict(observed=mask[0].tolist()), dict(noise=1e-3, observed=mask), dict(noise=nz_off, observed=mask)]
    for kw in valid:
        full = torch.broadcast_to(torch.as_tensor(kw["observed"]).to(torch.bool), (4, 6))
        poisoned = torch.where(full, dY, torch.full_like(dY, float("nan")))
        with pytest.raises(GppError, match="no CPU fallback"):  # valid calls reach the device, and there is none
            m.condition_on_gradients(good, poisoned, **kw)
    with pytest.raises(ValueError, match="finite"):
        m.condition_on_gradients(good, nan_on, observed=mask)
    with pytest.raises(ValueError, match="noise"):
        m.condition_on_gradients(good, dY, noise=neg_on, observed=mask)
    # NaN does not become "missing": without a mask it is refused as before
    with pytest.raises(ValueError, match="finite"):
        m.condition_on_gradients(good, nan_off)
    with pytest.raises(ValueError, match="finite"):
        m.condition_on_gradients(good, nan_off, observed=None)


def test_the_limit_counts_the_observed_entries():
    from gpplus_amd._lib import GppError

    m, X = _cpu_model()
    rows, dY = X[:14], torch.ones(14, 6, dtype=torch.float64)  # 84 > N = 80
    with pytest.raises(ValueError, match="84 gradient observations exceed"):
        m.condition_on_gradients(rows, dY)
    with pytest.raises(ValueError, match="84 gradient observations .* exceed"):
        m.condition_on_gradients(rows, dY, observed=torch.ones(6, dtype=torch.bool))
    with pytest.raises(GppError, match="no CPU fallback"):  # 42 <= 80: past every host check
        m.condition_on_gradients(rows, dY, observed=P.alternating_row(6))


def test_the_four_tuple_of_gradients():
    from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood
    from gpplus_amd.optim.mll_torch import check_objective_gradients

    m, X = _cpu_model()
    xg, dY = X[80:84], torch.ones(4, 6, dtype=torch.float64)
    mask = P.pattern_mask(4, 6)
    assert check_objective_gradients("gek", (xg, dY)) == (xg, dY, None)
    got = check_objective_gradients("gek", (xg, dY, None, mask))
    assert len(got) == 4 and got[0] is xg and got[1] is dY and got[2] is None and got[3] is mask
    with pytest.raises(ValueError, match="gradients="):
        check_objective_gradients("gek", (xg, dY, None, mask, None))
    with pytest.raises(ValueError, match="gek"):
        check_objective_gradients("mll", (xg, dY, None, mask))
    nan_off = torch.where(mask, dY, torch.full_like(dY, float("nan")))
    mll = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, nan_off, 1e-3, mask)
    q = int(mask.sum())
    assert mll.r_g.shape == (q,) and mll.noise.shape == (q,) and bool(torch.isfinite(mll.r_g).all())
    assert mll.selection.q == q and torch.equal(mll.selection.mask, mask)
    assert torch.equal(mll.r_g, (dY / m.y_std.to(torch.float64)).reshape(-1)[mask.reshape(-1)])
    dense = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, 1e-3)
    assert dense.selection is None and dense.r_g.shape == (4, 6)
    with pytest.raises(ValueError, match="observed"):
        GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, dY, None, mask[:3])
    with pytest.raises(ValueError, match="finite"):
        GradientEnhancedMarginalLogLikelihood(m.likelihood, m, xg, nan_off)


def test_gradient_selection_arrays():
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import GradientSelection

    mask = torch.tensor([[True, False, True], [False, False, False], [False, True, True], [True, True, True]])
    s = GradientSelection(mask)
    assert s.q == 7 and (s.num_points, s.nd) == (4, 3)
    assert s.first.dtype == torch.int32 and s.first.tolist() == [0, 2, 2, 4, 7]
    assert s.dir.dtype == torch.int32 and s.dir.tolist() == [0, 2, 1, 2, 0, 1, 2]
    assert s.flat.dtype == torch.int64 and s.flat.tolist() == [0, 2, 7, 8, 9, 10, 11]
    assert torch.equal(s.mask, mask) and s.mask is not mask
    for bad in (mask.to(torch.int32), mask[0], torch.zeros(3, 2, dtype=torch.bool)):
        with pytest.raises(GppError, match="selection"):
            GradientSelection(bad)


def test_symbols_are_declared_exported_and_bound():
    from gpplus_amd import _lib, backend
    from gpplus_amd.gradient_enhanced import GradientEnhancedPosterior
    from gpplus_amd.models import GP_Plus

    header = open(os.path.join(ROOT, "include", "gpp.h")).read()
    lib = _lib.load()
    for name, nargs in (("gpp_cross_kernel_dx_sel", 17), ("gpp_kernel_dxdx_sel", 20), ("gpp_gek_grad_reduce_sel", 23)):
        assert re.search(r"\bint %s\s*\(" % name, header)
        assert name in _lib.exported_symbols() and len(_lib._SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
        null = [None if t is ctypes.c_void_p else 0 for t in _lib._SIGNATURES[name][1]]
        assert getattr(lib, name)(*null) == -1  # a NULL handle is argument 1, before anything else is looked at
    assert callable(backend.GradientSelection)
    assert "observed" in GP_Plus.condition_on_gradients.__doc__ and "no partial gradients" not in GP_Plus.condition_on_gradients.__doc__
    assert isinstance(GradientEnhancedPosterior.num_gradient_observations, property)
    assert isinstance(GradientEnhancedPosterior.observed, property)

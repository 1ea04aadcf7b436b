"""Grouped cross-validation, the parts that need no GPU: the dense references against each other and against the limits the
identity must reproduce (singleton folds = leave-one-out, one fold = the marginal likelihood), the fold normalisation
(``cv.FoldIndex``, ``cv.group_labels``) and the host-side wiring (exports, bindings, argument errors of the fit drivers)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cv_reference import cv_autograd, cv_closed_form, cv_dense, cv_moments_dense, folds_from_labels  # noqa: E402
from loo_reference import KIND_RBF, LOG_2PI, _kernel, _noise, loo_dense, make_inputs  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dense(N=60, D=4, S=3, seed=5):
    inp = make_inputs(N, D, seed=seed, S=S)
    K, _ = _kernel(inp["U"], inp["w"], inp["sf2"], KIND_RBF, 0)
    return inp, K + torch.diag(_noise(inp["tau"], inp["grp"], N)), inp["y"] - inp["mean"]


def _ragged_labels(N, seed=0):
    """Labels with fold sizes 1, 2, 3, ... (the last fold takes the rest), shuffled over the rows."""
    sizes, left = [], N
    while left > 0:
        s = min(len(sizes) + 1, left)
        sizes.append(s)
        left -= s
    labels = np.repeat(np.arange(len(sizes)), sizes)
    return np.random.default_rng(seed).permutation(labels)


# ---- the references ---------------------------------------------------------------------------------------------------------------
def test_singleton_folds_are_leave_one_out():
    _, Ky, r = _dense()
    got, want = cv_dense(Ky, r, [np.array([i]) for i in range(60)]), loo_dense(Ky, r)
    assert abs(got - want) <= 1e-12 * abs(want), (float(got), float(want))


def test_singleton_folds_match_leave_one_out_in_every_gradient():
    """``loo_autograd`` stands in for ``cv_autograd`` in ONE GPU case (singleton folds at N = 1537): value and every gradient (U, w,
    sf2, tau, mean, y) of the two agree to 1e-10 of the largest entry here, with the Matern kind and three noise groups."""
    from loo_reference import KIND_MATERN52, loo_autograd

    inp = make_inputs(60, 5, seed=7, S=3)
    v0, g0 = loo_autograd(**inp, kind=KIND_MATERN52, d_split=2)
    v1, g1 = cv_autograd(**inp, folds=[np.array([i]) for i in range(60)], kind=KIND_MATERN52, d_split=2)
    assert abs(v1 - v0) <= 1e-10 * abs(v0)
    assert set(g0) == set(g1) == {"U", "w", "sf2", "tau", "mean", "y"}
    for name, ref in g0.items():
        err = (g1[name] - ref).abs().max().item()
        assert err <= 1e-10 * ref.abs().max().item(), (name, err)


def test_one_fold_of_everything_is_the_marginal_likelihood():
    _, Ky, r = _dense()
    L = torch.linalg.cholesky(Ky)
    z = torch.linalg.solve_triangular(L, r[:, None], upper=False)[:, 0]
    want = -0.5 * (z * z).sum() - L.diagonal().log().sum() - 0.5 * 60 * LOG_2PI
    got = cv_dense(Ky, r, [np.arange(60)])
    assert abs(got - want) <= 1e-12 * abs(want), (float(got), float(want))


def test_closed_form_matches_delete_fold_conditioning_on_ragged_folds():
    inp, Ky, r = _dense()
    folds = folds_from_labels(_ragged_labels(60))
    assert sorted(len(F) for F in folds)[:2] == [1, 2]
    want = cv_dense(Ky, r, folds).item()
    val, W, beta = cv_closed_form(Ky.numpy(), r.numpy(), folds)
    assert abs(val - want) <= 1e-11 * abs(want), (val, want)
    # ... and its weights: dcv/dy = beta and dcv/dtau_s = sum of W_ii over the group, against autograd through the deletions
    _, grads = cv_autograd(**inp, folds=folds)
    assert np.abs(beta - grads["y"].numpy()).max() <= 1e-9 * np.abs(beta).max()
    g_tau = np.array([np.diag(W)[inp["grp"].numpy() == s].sum() for s in range(3)])
    assert np.abs(g_tau - grads["tau"].numpy()).max() <= 1e-9 * np.abs(g_tau).max()
    # the moments: y_F + a_F and diag(P_FF^-1)
    mu, s2 = cv_moments_dense(Ky, r, folds)
    P = np.linalg.inv(Ky.numpy())
    for F in folds:
        Q = np.linalg.inv(P[np.ix_(F, F)])
        np.testing.assert_allclose(mu[F].numpy(), r.numpy()[F] - Q @ (P @ r.numpy())[F], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(s2[F].numpy(), np.diag(Q), rtol=1e-8)


# ---- FoldIndex --------------------------------------------------------------------------------------------------------------------
def _check_partition(fi, N):
    assert fi.idx.dtype == np.int32 and fi.off.dtype == np.int32
    assert fi.off[0] == 0 and fi.off[-1] == N and fi.off.shape[0] == fi.nfolds + 1
    assert sorted(fi.idx.tolist()) == list(range(N))  # every index exactly once
    for f in range(fi.nfolds):
        F = fi.fold(f)
        assert np.all(np.diff(F) > 0)  # ascending inside a fold


@pytest.mark.parametrize("as_tensor", [False, True])
def test_fold_index_from_labels(as_tensor):
    from gpplus_amd.cv import FoldIndex

    labels = np.array([7, -3, 7, 100, -3, 7, 0, 100, 7, -3, 2**40])
    fi = FoldIndex(torch.from_numpy(labels) if as_tensor else labels, labels.shape[0])
    _check_partition(fi, labels.shape[0])
    assert fi.labels.tolist() == [-3, 0, 7, 100, 2**40]  # folds ordered by label
    assert fi.sizes.tolist() == [3, 1, 4, 2, 1]
    assert fi.fold(2).tolist() == [0, 2, 5, 8] and fi.fold(0).tolist() == [1, 4, 9]
    b, = fi.buckets()
    assert b.mp == 32 and b.off.tolist() == [0, 3, 4, 8, 10, 11] and np.array_equal(b.idx, fi.idx)
    assert FoldIndex.make(fi, labels.shape[0]) is fi


def test_fold_index_k_fold_is_balanced_and_seeded():
    from gpplus_amd.cv import FoldIndex

    a, b, c = FoldIndex(5, 23, seed=3), FoldIndex(5, 23, seed=3), FoldIndex(5, 23, seed=4)
    _check_partition(a, 23)
    assert sorted(a.sizes.tolist(), reverse=True) == [5, 5, 5, 4, 4]
    assert np.array_equal(a.idx, b.idx) and np.array_equal(a.off, b.off)
    assert not np.array_equal(a.idx, c.idx)
    g = torch.Generator(device="cpu")
    g.manual_seed(3)
    assert np.array_equal(FoldIndex(5, 23, generator=g).idx, a.idx)
    assert FoldIndex(23, 23).sizes.tolist() == [1] * 23 and FoldIndex(1, 23).sizes.tolist() == [23]


def test_fold_index_buckets_follow_the_ladder():
    from gpplus_amd.cv import LADDER, FoldIndex

    sizes = [1, 32, 33, 128, 129, 600]
    labels = np.repeat(np.arange(len(sizes)), sizes)
    fi = FoldIndex(labels, labels.shape[0])
    got = [(b.mp, b.sizes.tolist()) for b in fi.buckets()]
    assert got == [(32, [1, 32]), (128, [33, 128]), (512, [129]), (2048, [600])] and LADDER[-1] == 6144
    assert [b.base for b in fi.buckets()] == [0, 33, 194, 323]
    # padded storage within a constant factor: pairs beside one large fold do not take the large fold's block size
    labels = np.r_[np.repeat(np.arange(800), 2), np.full(4000, 10 ** 6)]
    small, large = FoldIndex(labels, labels.shape[0]).buckets()
    assert (small.mp, small.folds.shape[0], large.mp, large.folds.shape[0]) == (32, 800, 6144, 1)


def test_fold_index_errors_come_before_any_device():
    from gpplus_amd.cv import MAX_FOLD, FoldIndex

    with pytest.raises(ValueError, match="length"):
        FoldIndex(np.zeros(9, dtype=np.int64), 10)
    with pytest.raises(ValueError, match="length"):
        FoldIndex(np.zeros((10, 1), dtype=np.int64), 10)
    for k in (0, -2, 11):
        with pytest.raises(ValueError, match="k"):
            FoldIndex(k, 10)
    with pytest.raises(ValueError, match=str(MAX_FOLD)):
        FoldIndex(np.zeros(MAX_FOLD + 1, dtype=np.int64), MAX_FOLD + 1)
    with pytest.raises(ValueError, match=str(MAX_FOLD)):
        FoldIndex(1, MAX_FOLD + 1)
    for bad in (np.zeros(10), torch.zeros(10), torch.zeros(10, dtype=torch.bool), np.array(["a"] * 10)):
        with pytest.raises(TypeError, match="integer"):
            FoldIndex(bad, 10)
    assert FoldIndex(np.zeros(MAX_FOLD, dtype=np.int64), MAX_FOLD).nfolds == 1


def test_group_labels_on_the_mixed_fixture():
    from gpplus_amd.cv import FoldIndex, group_labels

    X = dict(np.load(os.path.join(GOLD, "c3_borehole_mixed_n100.npz")))["Utrain"]
    labels = group_labels(X, (0, 5))
    pairs = {(a, b) for a, b in X[:, [0, 5]]}
    assert labels.shape == (X.shape[0],) and labels.dtype.kind == "i" and len(set(labels.tolist())) == len(pairs)
    for lab in set(labels.tolist()):
        assert len({(a, b) for a, b in X[labels == lab][:, [0, 5]]}) == 1  # one level combination per label
    assert np.array_equal(group_labels(torch.from_numpy(X), [0, 5]), labels)
    assert FoldIndex(labels, X.shape[0]).nfolds == len(pairs)


# ---- exports and wiring -----------------------------------------------------------------------------------------------------------
def _small_model():
    from gpplus_amd.models import GP_Plus

    fx = dict(np.load(os.path.join(GOLD, "c1_borehole_n500.npz")))
    return GP_Plus(torch.tensor(fx["Xtrain"][:40]), torch.tensor(fx["ytrain"][:40]), dtype=torch.float64, device="cpu")


def test_entry_points_are_declared_exported_and_bound():
    from gpplus_amd import _lib
    from gpplus_amd.backend import GppContext

    header = open(os.path.join(os.path.dirname(GOLD), os.pardir, "include", "gpp.h")).read()
    lib = _lib.load()
    for name in ("gpp_cv_blocks", "gpp_cv_rows"):
        assert f"int {name}(gpp_handle_t h" in header
        assert name in _lib._SIGNATURES and name in _lib.exported_symbols() and hasattr(lib, name)
    assert callable(GppContext.cv_blocks) and callable(GppContext.cv_rows)


def test_objective_class_is_exported_and_rejects_non_gaussian_input():
    from gpplus_amd import gpcore
    from gpplus_amd.gpcore import CrossValidationPseudoLikelihood, ExactMarginalLogLikelihood
    from gpplus_amd.gpcore.mlls import CrossValidationPseudoLikelihood as from_mlls

    assert CrossValidationPseudoLikelihood is from_mlls and hasattr(gpcore, "CrossValidationPseudoLikelihood")
    m = _small_model()
    cv = CrossValidationPseudoLikelihood(m.likelihood, m, 5)
    assert isinstance(cv, ExactMarginalLogLikelihood) and cv.folds.nfolds == 5  # the same priors, the same 1 / N
    with pytest.raises(RuntimeError, match="Gaussian"):
        cv(torch.zeros(40, dtype=torch.float64), m.train_targets)
    with pytest.raises(ValueError, match="length"):
        CrossValidationPseudoLikelihood(m.likelihood, m, np.zeros(39, dtype=np.int64))


def test_exact_cv_has_no_cpu_fallback():
    from gpplus_amd._lib import GppError
    from gpplus_amd.gpcore import CrossValidationPseudoLikelihood
    from gpplus_amd.linalg import KernelSpec, exact_cv

    inp = make_inputs(16, 3, seed=1, S=1)
    spec = KernelSpec(inp["w"], inp["sf2"], KIND_RBF, 0)
    with pytest.raises(GppError, match="no CPU fallback"):
        exact_cv(inp["U"], spec, inp["tau"], inp["mean"], inp["y"], 4)
    with pytest.raises(ValueError, match="k"):  # the folds are checked first
        exact_cv(inp["U"], spec, inp["tau"], inp["mean"], inp["y"], 17)
    m = _small_model()
    m.train()
    with pytest.raises(GppError, match="no CPU fallback"):
        CrossValidationPseudoLikelihood(m.likelihood, m, 5)(m(*m.train_inputs), m.train_targets)


def test_sharded_evaluation_is_refused():
    from gpplus_amd import settings
    from gpplus_amd.linalg import KernelSpec, exact_cv

    inp = make_inputs(16, 3, seed=1, S=1)
    spec = KernelSpec(inp["w"], inp["sf2"], KIND_RBF, 0)
    with settings.sharded_evaluation({"nb": 1024}):
        with pytest.raises(NotImplementedError, match="sharded"):
            exact_cv(inp["U"], spec, inp["tau"], inp["mean"], inp["y"], 4)


def test_objective_and_folds_argument_errors_of_the_drivers():
    from gpplus_amd.optim import MLLObjective, fit_model_scipy, fit_model_torch, fit_model_torch_batched
    from gpplus_amd.optim.mll_torch import OBJECTIVES

    assert OBJECTIVES == ("mll", "loo", "cv")
    m = _small_model()
    # "cv" without folds
    with pytest.raises(ValueError, match="folds"):
        fit_model_torch(m, num_iter=1, verbose=False, objective="cv")
    with pytest.raises(ValueError, match="folds"):
        fit_model_torch_batched(m, num_iter=1, objective="cv")
    with pytest.raises(ValueError, match="folds"):
        fit_model_scipy(m, num_restarts=0, objective="cv")
    with pytest.raises(ValueError, match="folds"):
        MLLObjective(m, True, [0, 0], objective="cv")
    with pytest.raises(ValueError, match="folds"):
        m.fit(objective="cv")
    # folds with another objective
    for objective in ("mll", "loo"):
        with pytest.raises(ValueError, match="folds"):
            fit_model_torch(m, num_iter=1, verbose=False, objective=objective, folds=5)
        with pytest.raises(ValueError, match="folds"):
            fit_model_torch_batched(m, num_iter=1, objective=objective, folds=5)
        with pytest.raises(ValueError, match="folds"):
            fit_model_scipy(m, num_restarts=0, objective=objective, folds=5)
        with pytest.raises(ValueError, match="folds"):
            MLLObjective(m, True, [0, 0], objective=objective, folds=5)
        with pytest.raises(ValueError, match="folds"):
            m.fit(objective=objective, folds=5)
    # bad folds with the right objective: FoldIndex's own errors, still on the host
    with pytest.raises(ValueError, match="k"):
        m.fit(objective="cv", folds=41)
    with pytest.raises(TypeError, match="integer"):
        fit_model_torch(m, num_iter=1, verbose=False, objective="cv", folds=np.zeros(40))
    # an unknown objective is still the first complaint
    with pytest.raises(ValueError, match="objective"):
        fit_model_torch(m, num_iter=1, verbose=False, objective="kfold", folds=5)
    assert MLLObjective(m, True, [0, 0], objective="cv", folds=5).folds.nfolds == 5

"""Dense fp64 CPU reference of the grouped (k-fold) cross-validation log pseudo-likelihood, INDEPENDENT of the identity the library
uses (p(y_F | y_-F) = N(y_F - P_FF^-1 alpha_F, P_FF^-1) with P = Ky^-1): every fold is deleted from the training set, the
remaining (N - m)-point system is solved, and the Gaussian log density of the held-out fold under its conditional is evaluated.

  ``cv_dense``          the value from a dense covariance and the residual r = y - mean;
  ``cv_moments_dense``  the held-out means (of r) and variances, by the same delete-fold solves;
  ``cv_autograd``       the same from (U, w, sf2, tau, mean, y, grp) of ``loo_reference.make_inputs`` with autograd gradients;
  ``cv_closed_form``    value and gradients through P in numpy, for the one case where k solves of size N - m are too slow
                        (checked against ``cv_dense`` in tests/test_cv_host.py).

``folds`` is a list of index arrays (a partition of range(N)).
"""
import numpy as np
import torch

from loo_reference import KIND_RBF, LOG_2PI, _kernel, _noise


def folds_from_labels(labels):
    labels = np.asarray(labels)
    return [np.flatnonzero(labels == v) for v in np.unique(labels)]


def _conditional(Ky, r, F):
    """Mean (of r_F) and covariance of r_F given r_-F under N(0, Ky), by conditioning on the kept rows."""
    N = Ky.shape[0]
    keep = torch.ones(N, dtype=torch.bool)
    keep[torch.as_tensor(F, dtype=torch.int64)] = False
    Fi = torch.as_tensor(F, dtype=torch.int64)
    Kff = Ky[Fi][:, Fi]
    if not bool(keep.any()):
        return torch.zeros(len(F), dtype=Ky.dtype), Kff
    Kkk, Kkf = Ky[keep][:, keep], Ky[keep][:, Fi]
    sol = torch.linalg.solve(Kkk, torch.cat([r[keep, None], Kkf], dim=1))
    return Kkf.T @ sol[:, 0], Kff - Kkf.T @ sol[:, 1:]


def cv_dense(Ky, r, folds):
    """sum_F log N(r_F | E[r_F | r_-F], Cov[r_F | r_-F]) by delete-fold conditioning (not divided by N)."""
    total = Ky.new_zeros(())
    for F in folds:
        mu, C = _conditional(Ky, r, F)
        L = torch.linalg.cholesky(C)
        diff = r[torch.as_tensor(F, dtype=torch.int64)] - mu
        z = torch.linalg.solve_triangular(L, diff[:, None], upper=False)[:, 0]
        total = total - 0.5 * (z * z).sum() - L.diagonal().log().sum() - 0.5 * len(F) * LOG_2PI
    return total


def cv_moments_dense(Ky, r, folds):
    """(mu, s2): the held-out mean of r and the held-out variance at every row, by the same delete-fold solves."""
    N = Ky.shape[0]
    mu, s2 = torch.empty(N, dtype=Ky.dtype), torch.empty(N, dtype=Ky.dtype)
    for F in folds:
        m, C = _conditional(Ky, r, F)
        Fi = torch.as_tensor(F, dtype=torch.int64)
        mu[Fi], s2[Fi] = m, C.diagonal()
    return mu, s2


def cv_autograd(U, w, sf2, tau, grp, mean, y, folds, kind=KIND_RBF, d_split=0):
    """Value and gradients (dict: U, w, sf2, tau, mean, y) of ``cv_dense`` by autograd."""
    leaves = {k: v.detach().clone().to(torch.float64).requires_grad_(True)
              for k, v in dict(U=U, w=w, sf2=sf2, tau=tau, mean=mean, y=y).items()}
    K, _ = _kernel(leaves["U"], leaves["w"], leaves["sf2"], kind, d_split)
    Ky = K + torch.diag(_noise(leaves["tau"], grp, U.shape[0]))
    val = cv_dense(Ky, leaves["y"] - leaves["mean"], folds)
    grads = torch.autograd.grad(val, list(leaves.values()))
    return val.detach(), dict(zip(leaves, grads))


def cv_closed_form(Ky, r, folds):
    """(value, W, beta) through P = Ky^-1 in numpy: value = sum_F [-1/2 alpha_F' P_FF^-1 alpha_F + 1/2 log|P_FF|] - (N / 2) log 2 pi,
    dcv = sum_ij W_ij dKy_ij, dcv/dy = beta = -dcv/dmean."""
    Ky, r = np.asarray(Ky, dtype=np.float64), np.asarray(r, dtype=np.float64)
    N = Ky.shape[0]
    P = np.linalg.inv(Ky)
    P = 0.5 * (P + P.T)
    alpha = P @ r
    val = -0.5 * N * LOG_2PI
    a = np.zeros(N)
    C = np.zeros((N, N))
    for F in folds:
        F = np.asarray(F)
        Pff = P[np.ix_(F, F)]
        Q = np.linalg.inv(Pff)
        aF = -Q @ alpha[F]
        val += 0.5 * alpha[F] @ aF + 0.5 * np.linalg.slogdet(Pff)[1]
        a[F] = aF
        C += P[:, F] @ (0.5 * (np.outer(aF, aF) + Q)) @ P[F, :]
    beta = P @ a
    W = -0.5 * (np.outer(alpha, beta) + np.outer(beta, alpha)) - C
    return val, W, beta


def closed_form_grads(U, w, sf2, tau, grp, W, beta):
    """Gradients (w, sf2, tau, mean, y) of sum_ij W_ij Ky_ij for the RBF kind (the larger test case has no feature gradients)."""
    U, w = np.asarray(U, dtype=np.float64), np.asarray(w, dtype=np.float64)
    N, D = U.shape
    r2 = np.zeros((N, N))
    diffs2 = []
    for d in range(D):
        diff = U[:, d, None] - U[None, :, d]
        diffs2.append(diff * diff)
        r2 += w[d] * diffs2[-1]
    K = float(sf2) * np.exp(-r2)
    WK = W * K
    g = dict(w=torch.tensor([-(WK * d2).sum() for d2 in diffs2]), sf2=torch.tensor(WK.sum() / float(sf2)))
    Wd = np.diag(W)
    if grp is None:
        g["tau"] = torch.tensor([Wd.sum()])
    else:
        gi = np.asarray(grp, dtype=np.int64)
        g["tau"] = torch.tensor([Wd[gi == s].sum() for s in range(int(np.asarray(tau).size))])
    g["mean"], g["y"] = torch.from_numpy(-beta), torch.from_numpy(beta.copy())
    return g

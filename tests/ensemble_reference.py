"""CPU reference of the hyperparameter-ensemble prediction (``gpp_predict_gen`` / ``gpp_predict_gen_batched`` in ``include/gpp_ensemble.h``,
``gpplus_amd.ensemble``), in numpy long double: per member the dense kernel matrix, its Cholesky factor, V = K_*N L^-T, the mean
V z and the variance sf2 - rowsum(V o V); and the moments of the mixture.  The kernel is ``pathwise_reference.kernel_matrix``."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pathwise_reference as R  # noqa: E402

LD = np.longdouble
KIND_RBF, KIND_MATERN32, KIND_MATERN52 = R.KIND_RBF, R.KIND_MATERN32, R.KIND_MATERN52


def cholesky(A):
    """Lower Cholesky factor of a symmetric positive definite matrix in its own dtype (numpy's LAPACK has no long double)."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError(f"leading minor {j + 1} is not positive definite")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, B):
    """L^-1 B by forward substitution (B: vector or matrix), long double."""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def member(Ua, Ub, w, sf2, tau_rows, r, kind=KIND_RBF, d_split=0):
    """One member: (mean, var, z) with K = sf2 k(Ub, Ub; w) + diag(tau_rows), L its Cholesky factor, z = L^-1 r,
    V = K_*N L^-T, mean = V z and var = sf2 - rowsum(V o V), all long double.  ``Ua``: test features, ``Ub``: training features."""
    K = R.kernel_matrix(Ub, Ub, w, sf2, kind, d_split, LD) + np.diag(np.asarray(tau_rows, dtype=LD))
    L = cholesky(K)
    z = solve_lower(L, np.asarray(r, dtype=LD))
    Vt = solve_lower(L, R.kernel_matrix(Ub, Ua, w, sf2, kind, d_split, LD))  # N x M: V^T = L^-1 K_N*
    return Vt.T @ z, LD(sf2) - (Vt * Vt).sum(0), z


def posterior_weights(losses, n):
    """pi_b proportional to exp(-n (loss_b - min loss)), long double."""
    l = np.asarray(losses, dtype=LD)
    e = np.exp(-LD(n) * (l - l.min()))
    return e / e.sum()


def mixture(pi, mu, var):
    """Mean and variance of sum_b pi_b N(mu_b, var_b) by the law of total variance; mu, var: (K, M)."""
    p = np.asarray(pi, dtype=LD)[:, None]
    mu, var = np.asarray(mu, dtype=LD), np.asarray(var, dtype=LD)
    m = (p * mu).sum(0)
    return m, (p * var).sum(0) + (p * (mu - m) ** 2).sum(0)


def mixture_brute(pi, mu, var):
    """The same two moments from the raw moments of the mixture: E[y] = sum pi mu, E[y^2] = sum pi (var + mu^2)."""
    p = np.asarray(pi, dtype=LD)[:, None]
    mu, var = np.asarray(mu, dtype=LD), np.asarray(var, dtype=LD)
    m1 = (p * mu).sum(0)
    m2 = (p * (var + mu * mu)).sum(0)
    return m1, m2 - m1 * m1

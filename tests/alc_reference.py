"""CPU reference of the expected-variance-reduction scores (``gpp_post_cross_sq``, ``linalg.variance_reduction``,
``GP_Plus.variance_reduction``, ``select_by_variance_reduction``), in plain numpy with ``np.longdouble``.  Nothing here imports torch,
the library or a GPU.

The library scores a candidate by an identity on the cached factor, dV(c) = sum_r omega_r c(x_r, x_c)^2 / s_c.  The reference shares
nothing with it: ``score_by_refit`` FACTORISES the N + 1 points [training; candidate] from raw features for every candidate, solves
against that factor at every reference point and subtracts the weighted latent variances; ``greedy_by_refit`` does the same for
the batch, round by round.  (The one saving: the first N columns of the factor of N + 1 points are the factor of the first N and
are not computed again per candidate; every variance is a full solve.)
``closed_form`` is the identity itself in long double, for the host test that holds the two against each other.

The kernel is the library's (``pathwise_reference.kernel_matrix``); ``noise`` is the diagonal added to the training covariance
(noise level of each row's source plus the factorisation's jitter).
"""
import numpy as np

from pathwise_reference import kernel_matrix

LD = np.longdouble


def _ld(a):
    return np.asarray(a, dtype=LD)


def chol(A, lead=None):
    """Lower Cholesky factor in long double (no library call).  ``lead``: the factor of the leading block A[:n0, :n0], if the caller
    has it — the leading columns of a Cholesky factor do not depend on the rows behind them, so only the rows from n0 on are
    computed (row by row); without it, every column."""
    A = _ld(A)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    n0 = 0 if lead is None else lead.shape[0]
    if n0:
        L[:n0, :n0] = lead
        for i in range(n0, n):
            L[i, :i] = forward_solve(L[:i, :i], A[i, :i])
            d = A[i, i] - L[i, :i] @ L[i, :i]
            if not d > 0:
                raise np.linalg.LinAlgError(f"leading minor {i + 1} is not positive definite")
            L[i, i] = np.sqrt(d)
        return L
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"leading minor {j + 1} is not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward_solve(L, B):
    """L^-1 B for lower triangular L, row by row."""
    L, B = _ld(L), _ld(B)
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


class Fit:
    """Noisy observations at ``U``: Ky = K(U, U) + diag(noise) and its factor.  ``extended`` is the fit of [U; one more row]: the
    (N + 1) x (N + 1) matrix is assembled and factorised (the leading N columns of its factor are this fit's, see ``chol``)."""

    def __init__(self, U, noise, w, sf2, kind=0, d_split=0, _Ky=None, _L=None):
        self.U, self.noise, self.kern = np.asarray(U), _ld(noise), (w, sf2, kind, d_split)
        self.Ky = kernel_matrix(self.U, self.U, *self.kern) + np.diag(self.noise) if _Ky is None else _Ky
        self.L = chol(self.Ky) if _L is None else _L

    def extended(self, u, noise_u):
        n = self.U.shape[0]
        U1 = np.concatenate([self.U, u.reshape(1, -1)])
        Ky = np.zeros((n + 1, n + 1), dtype=LD)
        Ky[:n, :n] = self.Ky
        row = kernel_matrix(u.reshape(1, -1), U1, *self.kern)[0]
        Ky[n, :], Ky[:, n] = row, row
        Ky[n, n] += LD(noise_u)
        return Fit(U1, np.concatenate([self.noise, [LD(noise_u)]]), *self.kern, _Ky=Ky, _L=chol(Ky, lead=self.L))

    def latent_variance(self, Ur):
        """sf2 - diag(K_rN Ky^-1 K_Nr): the whole solve against this fit's factor."""
        V = forward_solve(self.L, kernel_matrix(self.U, Ur, *self.kern))
        return LD(self.kern[1]) - (V * V).sum(0)


def latent_variance(U, noise, Ur, w, sf2, kind=0, d_split=0):
    """Posterior variance of the latent f at ``Ur`` given noisy observations at ``U``, by a factorisation from scratch."""
    return Fit(U, noise, w, sf2, kind, d_split).latent_variance(Ur)


def _weights(omega, Mr):
    return np.full(Mr, LD(1) / Mr, dtype=LD) if omega is None else _ld(omega)


def _scores(fit, Uc, noise_c, Ur, om):
    before = om @ fit.latent_variance(Ur)
    return np.array([before - om @ fit.extended(Uc[c], noise_c[c]).latent_variance(Ur) for c in range(Uc.shape[0])], dtype=LD)


def score_by_refit(U, noise, Uc, noise_c, Ur, w, sf2, kind=0, d_split=0, omega=None):
    """For every candidate c: sum_r omega_r var(x_r | U) - sum_r omega_r var(x_r | U and one observation at Uc_c with noise
    noise_c[c]), the second term from the factorised N + 1 points."""
    return _scores(Fit(U, noise, w, sf2, kind, d_split), Uc, _ld(noise_c), Ur, _weights(omega, Ur.shape[0]))


def closed_form(U, noise, Uc, noise_c, Ur, w, sf2, kind=0, d_split=0, omega=None):
    """The identity in long double: sum_r omega_r c(x_r, x_c)^2 / (c(x_c, x_c) + noise_c), c = sf2 k - v^T v, v = L^-1 k(X, .)."""
    om = _weights(omega, Ur.shape[0])
    L = chol(kernel_matrix(U, U, w, sf2, kind, d_split) + np.diag(_ld(noise)))
    Vc = forward_solve(L, kernel_matrix(U, Uc, w, sf2, kind, d_split))
    Vr = forward_solve(L, kernel_matrix(U, Ur, w, sf2, kind, d_split))
    C = kernel_matrix(Uc, Ur, w, sf2, kind, d_split) - Vc.T @ Vr
    s = LD(sf2) - (Vc * Vc).sum(0) + _ld(noise_c)
    return (C * C) @ om / s


def greedy_by_refit(U, noise, Uc, noise_c, Ur, w, sf2, q, kind=0, d_split=0, omega=None, cost=None):
    """q greedy rounds by refits: each round scores every remaining candidate against the training points plus the picks so far
    (as ``score_by_refit``) and takes the largest gain (per unit ``cost`` when given).  Returns (picks, gains, margins): margins[t]
    is the relative gap between the best and the second-best ranking value of round t (inf with one candidate left)."""
    om, noise_c = _weights(omega, Ur.shape[0]), _ld(noise_c)
    fit = Fit(U, noise, w, sf2, kind, d_split)
    left = list(range(Uc.shape[0]))
    picks, gains, margins = [], [], []
    for _ in range(q):
        g = _scores(fit, Uc[left], noise_c[left], Ur, om)
        rank = g if cost is None else g / _ld(cost)[left]
        order = np.argsort(-rank)
        margins.append(float((rank[order[0]] - rank[order[1]]) / abs(rank[order[0]])) if len(left) > 1 else float("inf"))
        j = left[int(order[0])]
        picks.append(j)
        gains.append(g[int(order[0])])
        fit = fit.extended(Uc[j], noise_c[j])
        left.remove(j)
    return picks, np.array(gains, dtype=LD), margins


def reduction_of_batch(U, noise, Uq, noise_q, Ur, w, sf2, kind=0, d_split=0, omega=None):
    """sum_r omega_r (var before - var after) of conditioning on ALL rows of ``Uq`` at once, by one factorisation of N + q points."""
    om = _weights(omega, Ur.shape[0])
    after = latent_variance(np.concatenate([U, Uq]), np.concatenate([_ld(noise), _ld(noise_q)]), Ur, w, sf2, kind, d_split)
    return om @ (latent_variance(U, noise, Ur, w, sf2, kind, d_split) - after)

"""CPU reference of the knowledge-gradient scores (``gpp_post_cross_min``, ``linalg.knowledge_gradient``, ``GP_Plus.knowledge_gradient``,
``select_by_knowledge_gradient``), dense, in plain numpy with ``np.longdouble``.  Written from the formulas; nothing here imports
torch, the library or a GPU.

With v(x) = L^-1 k(X, x), c(x, x') = sf2 k(x, x') - v(x)^T v(x') and s_c = c(x_c, x_c) + noise_c, one noisy observation at x_c moves
the posterior mean at x_r to mu_r + c(x_r, x_c) / sqrt(s_c) Z, Z ~ N(0, 1), so (for minimisation)
    KG(c) = min_r mu_r - E_Z[ min_r (mu_r + c_cr Z / sqrt(s_c)) ].
``kg_quadrature`` replaces E_Z by the Gauss-Hermite rule ``nodes`` — what the library computes; ``kg_by_fantasy`` gets the same number
with no identity at all: per node it EXTENDS the fit by the candidate with the fantasised value and predicts the reference means
(``alc_reference.Fit``); ``kg_exact`` is the expectation itself through the lower envelope of the M_r lines; ``greedy_believer`` is
the batch heuristic, each round on a fit extended by the picks so far.  ``noise`` is the diagonal added to the training covariance.
"""
import math

import numpy as np

from alc_reference import Fit, forward_solve
from pathwise_reference import kernel_matrix

LD = np.longdouble


def _ld(a):
    return np.asarray(a, dtype=LD)


def nodes(Q):
    """(z, W): the Q-point Gauss-Hermite rule for N(0, 1) — numpy's float64 nodes and weights, the nodes exactly antisymmetric, the
    weights exactly symmetric and normalised to sum 1 — as long doubles."""
    z, W = np.polynomial.hermite_e.hermegauss(int(Q))
    z = 0.5 * (z - z[::-1])
    W = 0.5 * (W + W[::-1])
    W = W / W.sum()
    return _ld(z), _ld(W)


def post_cov(fit, A, B):
    """c(A, B) = K(A, B) - V_A^T V_B under ``fit``."""
    VA = forward_solve(fit.L, kernel_matrix(fit.U, A, *fit.kern))
    VB = forward_solve(fit.L, kernel_matrix(fit.U, B, *fit.kern))
    return kernel_matrix(A, B, *fit.kern) - VA.T @ VB


def post_mean(fit, resid, A, prior=0.0):
    """prior + K(A, X) Ky^-1 resid, resid = y - prior mean at the training rows."""
    VA = forward_solve(fit.L, kernel_matrix(fit.U, A, *fit.kern))
    return _ld(prior) + VA.T @ forward_solve(fit.L, _ld(resid))


def dense(fit, resid, Uc, noise_c, Ur, prior_r=0.0):
    """(C: M_c x M_r cross-covariance, s: M_c predictive variances of the observation, mu: M_r means)."""
    C = post_cov(fit, Uc, Ur)
    VC = forward_solve(fit.L, kernel_matrix(fit.U, Uc, *fit.kern))
    s = LD(fit.kern[1]) - (VC * VC).sum(0) + _ld(noise_c)
    return C, s, post_mean(fit, resid, Ur, prior_r)


def kg_quadrature(C, s, mu, Q, maximize=False):
    """-sum_k W_k min_r (m_r + z_k c_cr / sqrt(s_c)), m = mu - min mu (max mu - mu under ``maximize``)."""
    z, W = nodes(Q)
    mu = _ld(mu)
    m = (mu.max() - mu) if maximize else (mu - mu.min())
    sig = _ld(C) / np.sqrt(_ld(s))[:, None]
    mins = np.stack([(m[None, :] + zk * sig).min(1) for zk in z], 1)  # M_c x Q
    return -(mins @ W)


def kg_by_fantasy(fit, resid, Uc, noise_c, Ur, Q):
    """For every candidate and node: extend the fit by the candidate observed at mean + sqrt(s) z_k, predict the reference means
    from the N + 1 rows, take their minimum; min mu - sum_k W_k (that).  Zero prior mean."""
    z, W = nodes(Q)
    noise_c = _ld(noise_c)
    mu_r = post_mean(fit, resid, Ur)
    out = np.zeros(Uc.shape[0], dtype=LD)
    for c in range(Uc.shape[0]):
        uc = Uc[c:c + 1]
        mu_c = post_mean(fit, resid, uc)[0]
        s_c = post_cov(fit, uc, uc)[0, 0] + noise_c[c]
        ext = fit.extended(Uc[c], noise_c[c])
        acc = LD(0)
        for zk, wk in zip(z, W):
            r1 = np.concatenate([_ld(resid), [mu_c + np.sqrt(s_c) * zk]])
            acc += wk * post_mean(ext, r1, Ur).min()
        out[c] = mu_r.min() - acc
    return out


def _Phi(x):
    return 0.5 * math.erfc(-float(x) / math.sqrt(2.0)) if np.isfinite(x) else (0.0 if x < 0 else 1.0)


def _phi(x):
    return math.exp(-0.5 * float(x) ** 2) / math.sqrt(2.0 * math.pi) if np.isfinite(x) else 0.0


def expected_min_of_lines(a, b):
    """E[min_r (a_r + b_r Z)], Z ~ N(0, 1), exactly: the lower envelope of the lines in sorted-slope order (towards z = -inf the
    steepest line is the lowest), each piece integrated with Phi and phi:
        int_l^u (a + b z) phi(z) dz = a (Phi(u) - Phi(l)) + b (phi(l) - phi(u))."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    order = np.lexsort((a, -b))  # slope descending; among equal slopes the smallest intercept first
    hull, start = [], []  # lines of the envelope from left to right, and where each one starts
    for i in order:
        if hull and b[i] == b[hull[-1]]:
            continue  # parallel and not lower
        while hull:
            j = hull[-1]
            x = (a[i] - a[j]) / (b[j] - b[i])  # line i is below line j to the right of x
            if x <= start[-1]:
                hull.pop()
                start.pop()
            else:
                break
        if not hull:
            hull.append(i)
            start.append(-np.inf)
        else:
            hull.append(i)
            start.append(x)
    total = 0.0
    for n, i in enumerate(hull):
        lo, hi = start[n], (start[n + 1] if n + 1 < len(hull) else np.inf)
        total += a[i] * (_Phi(hi) - _Phi(lo)) + b[i] * (_phi(lo) - _phi(hi))
    return total


def kg_exact(C, s, mu, maximize=False):
    """The knowledge gradient with the exact expectation (float64 Phi / phi)."""
    mu = np.asarray(mu, dtype=np.float64)
    m = (mu.max() - mu) if maximize else (mu - mu.min())
    sig = np.asarray(C, dtype=np.float64) / np.sqrt(np.asarray(s, dtype=np.float64))[:, None]
    return np.array([-expected_min_of_lines(m, sig[c]) for c in range(sig.shape[0])])


def greedy_believer(fit, resid, Uc, noise_c, Ur, q, Q, cost=None, maximize=False, prior_r=0.0):
    """q greedy rounds of the Kriging believer: the means stay those of ``fit``; each round scores the remaining candidates with the
    covariances of the fit EXTENDED by the picks so far (a factorisation of N + t rows from features) and takes the largest score
    (per unit ``cost`` when given).  Returns (picks, gains, margins, first-round scores); margins[t] is the relative gap between the
    best and the second-best ranking value of round t."""
    noise_c = _ld(noise_c)
    mu = post_mean(fit, resid, Ur, prior_r)
    left = list(range(Uc.shape[0]))
    picks, gains, margins, first = [], [], [], None
    for _ in range(q):
        C, s, _ = dense(fit, np.zeros(fit.U.shape[0]), Uc[left], noise_c[left], Ur)
        g = kg_quadrature(C, s, mu, Q, maximize)
        if first is None:
            first = g
        rank = g if cost is None else g / _ld(cost)[left]
        order = np.argsort(-rank)
        margins.append(float((rank[order[0]] - rank[order[1]]) / abs(rank[order[0]])) if len(left) > 1 else float("inf"))
        j = left[int(order[0])]
        picks.append(j)
        gains.append(g[int(order[0])])
        fit = fit.extended(Uc[j], noise_c[j])
        left.remove(j)
    return picks, np.array(gains, dtype=LD), margins, first

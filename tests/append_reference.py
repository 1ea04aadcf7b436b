"""CPU reference for appending q observations to a factorised exact GP (``gpp_chol_append``, ``linalg.append_to_cache``,
``GPR.condition_on``), in plain numpy with ``np.longdouble``.  Nothing here imports torch, the library or a GPU.

Notation: Ky = L L^T is the factorised N x N covariance, Linv = L^-1, z = Linv r, alpha = Linv^T z.  k = K(X, Xq) (N x q),
C = K(Xq, Xq) + noise (q x q), r_q the new residuals.

Part 1 — the bordered quantities, one function per stage, each from GIVEN operands (a test hands every stage the device's own result
of the stage before, so that each comparison sees one stage's rounding only):
    stage_V       V  = (Linv k)^T
    stage_S       S  = C - V V^T
    chol          Ls with S = Ls Ls^T                     (the new factor rows are [V, Ls])
    tri_inv       Ls^-1
    stage_W       W  = -Ls^-1 (V Linv)                    (the new inverse rows are [W, Ls^-1])
    stage_zq      zq = Ls^-1 (r_q - V z)
    stage_alpha   alpha' = [alpha + W^T zq ; Ls^-T zq]
Part 2 — the elementwise bounds a fp64 implementation of each stage must meet, derived, not measured.
Part 3 — a dense posterior (mean, variance, leave-one-out moments) from raw features and parameters.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53  # unit roundoff of fp64


def _ld(a):
    return np.asarray(a, dtype=LD)


# ---- part 1: stages --------------------------------------------------------------------------------------------------------------
def chol(A):
    """Lower Cholesky factor of a symmetric positive definite matrix in long double (column by column, no library call)."""
    A = _ld(A).copy()
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"leading minor {j + 1} is not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inv(L):
    """Inverse of a lower triangular matrix in long double, by forward substitution on the identity."""
    L = _ld(L)
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        rhs = -(L[i, :i] @ X[:i, :])
        rhs[i] += 1
        X[i, :] = rhs / L[i, i]
    return np.tril(X)


def stage_V(Linv, k):
    return (np.tril(_ld(Linv)) @ _ld(k)).T


def stage_S(C, V):
    V = _ld(V)
    return _ld(C) - V @ V.T


def stage_P(V, Linv):
    return _ld(V) @ np.tril(_ld(Linv))


def stage_W(Lsinv, V, Linv):
    return -(np.tril(_ld(Lsinv)) @ stage_P(V, Linv))


def stage_t(rq, V, z):
    return _ld(rq) - _ld(V) @ _ld(z)


def stage_zq(Lsinv, rq, V, z):
    return np.tril(_ld(Lsinv)) @ stage_t(rq, V, z)


def stage_alpha(alpha, W, zq, Lsinv):
    return np.concatenate([_ld(alpha) + _ld(W).T @ _ld(zq), np.tril(_ld(Lsinv)).T @ _ld(zq)])


def bordered(L, Linv, z, alpha, k, C, rq):
    """Every stage chained in long double: dict with V, S, Ls, Lsinv, W, zq, alpha, and the assembled L', Linv', z'."""
    V = stage_V(Linv, k)
    S = stage_S(C, V)
    Ls = chol(S)
    Lsinv = tri_inv(Ls)
    W = stage_W(Lsinv, V, Linv)
    zq = stage_zq(Lsinv, rq, V, z)
    al = stage_alpha(alpha, W, zq, Lsinv)
    N, q = _ld(k).shape
    Lp = np.zeros((N + q, N + q), dtype=LD)
    Lp[:N, :N], Lp[N:, :N], Lp[N:, N:] = np.tril(_ld(L)), V, Ls
    Lip = np.zeros((N + q, N + q), dtype=LD)
    Lip[:N, :N], Lip[N:, :N], Lip[N:, N:] = np.tril(_ld(Linv)), W, Lsinv
    return dict(V=V, S=S, Ls=Ls, Lsinv=Lsinv, W=W, zq=zq, alpha=al, L=Lp, Linv=Lip, z=np.concatenate([_ld(z), zq]))


# ---- part 2: bounds --------------------------------------------------------------------------------------------------------------
# gamma_n = n u / (1 - n u) bounds the relative error of a sum of n products in ANY order (Higham, Accuracy and Stability of
# Numerical Algorithms, 2nd ed., section 3.1): |fl(x . y) - x . y| <= gamma_n |x| . |y|.
def gamma(n):
    return n * U / (1 - n * U)


def dot_bound(A, B, extra=2):
    """|fl(A B) - A B| <= gamma_{K + extra} |A| |B| elementwise, K the contracted length: the dot-product bound; ``extra`` roundings
    for what is done to the sum afterwards (a subtraction from another term, a sign: one rounding each)."""
    A, B = np.abs(_ld(A)), np.abs(_ld(B))
    return gamma(A.shape[1] + extra) * (A @ B)


def chol_residual_bound(Ls):
    """|S - Ls Ls^T| <= gamma_{q+1} |Ls| |Ls^T| elementwise for the computed Cholesky factor of a q x q matrix (Higham, Theorem
    10.3), in any order of the inner sums."""
    Ls = np.abs(np.tril(_ld(Ls)))
    return gamma(Ls.shape[0] + 1) * (Ls @ Ls.T)


def tri_inv_bound(Ls):
    """|X^ - X| <= 4 gamma_{q+1} |X| |L| |X| elementwise, X = L^-1 (lower, q x q).  Substitution (one column per solve) computes a
    column x^_j with (L + dL_j) x^_j = e_j, |dL_j| <= gamma_q |L| (Higham, Theorem 8.5), hence x^_j - x_j = -X dL_j x^_j and
    |X^ - X| <= gamma_q |X| |L| |X^|; the blocked inversion that merges pairs of diagonal blocks by two products,
    X21 = -(X22 L21) X11, obeys a bound of the same form (Higham, section 14.3, the block methods' forward error).  The factor 4
    covers |X^| <= |X| + |X^ - X| at first order and the two products of a merge (each entry is formed by one merge only)."""
    L = np.tril(_ld(Ls))
    X = np.abs(tri_inv(L))
    return 4 * gamma(L.shape[0] + 1) * (X @ np.abs(L) @ X)


def t_bound(rq, V, z):
    """t = r_q - V z: the dot product of length N and one subtraction."""
    V = np.abs(_ld(V))
    return gamma(V.shape[1] + 2) * (np.abs(_ld(rq)) + V @ np.abs(_ld(z)))


def two_product_bound(Lsinv, V, Linv):
    """W = -Ls^-1 (V Linv) evaluated as two products.  P^ = fl(V Linv) = P + E_P with |E_P| <= gamma_{N+2} |V| |Linv| (dot product);
    W^ = fl(Ls^-1 P^) = Ls^-1 P^ + E_W with |E_W| <= gamma_{q+2} |Ls^-1| |P^| and |P^| <= |P| + |E_P|.  Against the exact product of
    the SAME operands: |W^ - W| <= |Ls^-1| |E_P| + gamma_{q+2} |Ls^-1| (|P| + |E_P|)."""
    Li = np.abs(np.tril(_ld(Lsinv)))
    P = np.abs(stage_P(V, Linv))
    EP = dot_bound(V, np.tril(_ld(Linv)))
    return Li @ EP + gamma(Li.shape[0] + 2) * (Li @ (P + EP))


def zq_bound(Lsinv, rq, V, z):
    """zq = Ls^-1 t from the computed t: the error of t propagated through |Ls^-1| plus the dot product of length q."""
    Li = np.abs(np.tril(_ld(Lsinv)))
    t = np.abs(stage_t(rq, V, z))
    Et = t_bound(rq, V, z)
    return Li @ Et + gamma(Li.shape[0] + 2) * (Li @ (t + Et))


def alpha_bound(alpha, W, zq, Lsinv):
    """alpha' from the device's own W, zq and Ls^-1: head alpha + W^T zq (dot product of length q and one addition), tail
    Ls^-T zq (dot product of length q)."""
    Wa, za, Li = np.abs(_ld(W)), np.abs(_ld(zq)), np.abs(np.tril(_ld(Lsinv)))
    q = za.shape[0]
    head = gamma(q + 2) * (np.abs(_ld(alpha)) + Wa.T @ za)
    tail = gamma(q + 2) * (Li.T @ za)
    return np.concatenate([head, tail])


# ---- part 3: a dense posterior from raw features and parameters ------------------------------------------------------------------
def rbf(Ua, Ub, w, sf2):
    """sf2 exp(-sum_d w_d (a_d - b_d)^2) in long double."""
    Ua, Ub, w = _ld(Ua), _ld(Ub), _ld(w).reshape(-1)
    d2 = ((Ua[:, None, :] - Ub[None, :, :]) ** 2 * w).sum(-1)
    return LD(sf2) * np.exp(-d2)


def dense_posterior(U, y, mean, w, sf2, noise, Us=None, mean_s=None):
    """From features U (N x D), targets y, prior means, RBF weights w, outputscale sf2 and per-row noise variances: dict with
    alpha, loo_mean / loo_var (Rasmussen & Williams 5.4.2) and, for test features Us, the latent posterior mean / var."""
    U, y, mean = _ld(U), _ld(y).reshape(-1), _ld(mean).reshape(-1)
    N = U.shape[0]
    Ky = rbf(U, U, w, sf2) + np.diag(np.broadcast_to(_ld(noise), (N,)))
    Li = tri_inv(chol(Ky))
    P = Li.T @ Li
    alpha = P @ (y - mean)
    d = np.diag(P)
    out = dict(alpha=alpha, loo_mean=y - alpha / d, loo_var=1 / d)
    if Us is not None:
        Ks = rbf(Us, U, w, sf2)
        Vs = Ks @ Li.T
        out["mean"] = np.broadcast_to(_ld(mean_s), (Ks.shape[0],)) + Ks @ alpha
        out["var"] = LD(sf2) - (Vs * Vs).sum(-1)
    return out

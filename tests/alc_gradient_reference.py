"""CPU reference of the expected variance reduction of a run that returns y AND gradient components (``gpp_post_cross_lin_sq``,
``linalg.variance_reduction_block``, ``variance_reduction(..., gradient=)``, ``select_run_by_variance_reduction``), in plain numpy with
``np.longdouble``.  Nothing here imports torch, the library or a GPU.

A ``Model`` is a set of noisy linear observations of f: function values at ``U`` and, for a gradient-enhanced posterior, gradient
components (``Ug``, ``gdirs``: one point and one feature column per observation).  A candidate x_c adds b = 1 + p' more: its value and
its derivatives by the columns ``dirs``.

  ``score_by_refit``   for every candidate the joint covariance of ALL observations [model; candidate value; candidate gradient
                       components] is assembled from ``pathwise_reference.kernel_matrix``, the first-derivative block
                       (``pathwise_grad_reference.kernel_dgen``) and ``gek_reference.d2k``, factorised from scratch, and the weighted
                       latent variance over the reference rows is subtracted from the one without the candidate;
  ``closed_form``      separately, the identity the library evaluates: dV(c) = sum_r omega_r c_r^T S_c^-1 c_r with c_r the posterior
                       cross-covariance of f(x_r) with the b functionals and S_c their posterior covariance plus the noise diagonal;
                       in long double, or with ``fp64=True`` in float64 numpy, where it also returns max cond(S_c): the distance of
                       the two is the FLOOR no fp64 evaluation of the identity can be expected to beat.
With ``dirs`` empty both are tests/alc_reference.py's."""
import numpy as np

import alc_reference as alc
import pathwise_reference as R
from gek_reference import d2k
from pathwise_grad_reference import kernel_dgen

LD = np.longdouble


class Model:
    def __init__(self, U, noise, w, sf2, kind=0, d_split=0, Ug=None, gdirs=None, gnoise=None):
        self.U, self.noise, self.kern = np.asarray(U, dtype=np.float64), np.asarray(noise), (np.asarray(w), sf2, kind, d_split)
        D = self.U.shape[1]
        self.Ug = np.zeros((0, D)) if Ug is None else np.asarray(Ug, dtype=np.float64)
        self.gdirs = np.zeros(0, dtype=int) if gdirs is None else np.asarray(gdirs, dtype=int)
        self.gnoise = np.zeros(0) if gnoise is None else np.asarray(gnoise)
        assert self.Ug.shape[0] == self.gdirs.shape[0] == self.gnoise.shape[0]


def _vg(Pv, Pg, gd, kern, ld):
    """cov(f(Pv_i), d f / du_{gd_k}(Pg_k)): (values) x (gradient observations)."""
    out = np.zeros((Pv.shape[0], Pg.shape[0]), dtype=ld)
    for d in np.unique(gd):
        k = np.nonzero(gd == d)[0]
        out[:, k] = kernel_dgen(Pg[k], Pv, *kern, int(d), ld=ld).T
    return out


def _gg(Pa, da, Pb, db, kern, ld):
    """cov of two sets of gradient observations."""
    D = Pa.shape[1]
    H = d2k(Pa, Pb, *kern, 0, D, ld=ld).reshape(Pa.shape[0], D, Pb.shape[0], D)
    return H[np.arange(Pa.shape[0])[:, None], da[:, None], np.arange(Pb.shape[0])[None, :], db[None, :]]


def _cov(A, B, kern, ld):
    """Prior covariance of two observation sets A = (Pv, Pg, gd), B likewise: values first, gradient observations behind."""
    (Av, Ag, ad), (Bv, Bg, bd) = A, B
    top = [R.kernel_matrix(Av, Bv, *kern, ld=ld), _vg(Av, Bg, bd, kern, ld)]
    bot = [_vg(Bv, Ag, ad, kern, ld).T, _gg(Ag, ad, Bg, bd, kern, ld) if Ag.shape[0] and Bg.shape[0]
           else np.zeros((Ag.shape[0], Bg.shape[0]), dtype=ld)]
    return np.block([top, bot]).astype(ld)


def _sets(m, uc, dirs):
    D = m.U.shape[1]
    dirs = np.asarray(dirs, dtype=int)
    base = (m.U, m.Ug, m.gdirs)
    cand = (uc.reshape(1, D), np.repeat(uc.reshape(1, D), len(dirs), 0), dirs)
    return base, cand


def _extend(L, V, Kbc, Kcc, Kcr):
    """The factor of [[Kbb, Kbc], [Kbc^T, Kcc]] given the factor L of Kbb — its leading columns do not depend on the rows behind them
    (``alc_reference.chol``), only the new rows are computed — and the new rows of L^-1 K(., Ur) given the leading rows V."""
    n, b = L.shape[0], Kcc.shape[0]
    J = np.zeros((n + b, n + b), dtype=LD)  # (the leading block is never read: only the new rows are)
    J[:n, n:], J[n:, :n], J[n:, n:] = Kbc, Kbc.T, Kcc
    Lj = alc.chol(J, lead=L)
    B = np.concatenate([np.zeros_like(V), Kcr])
    X = np.concatenate([V, np.zeros_like(Kcr)])
    for i in range(n, n + b):
        X[i] = (B[i] - Lj[i, :i] @ X[:i]) / Lj[i, i]
    return X[n:]


def score_by_refit(m, Uc, noise_c, gnoise_c, dirs, Ur, omega=None):
    """For every candidate c: sum_r omega_r (var(x_r | model) - var(x_r | model, y(x_c), d_dirs y(x_c))), the second term from the
    factorised joint covariance of [model's observations; candidate value; candidate gradient components] (the leading columns of its
    factor, the model's own, are not computed again per candidate).  ``noise_c``: M_c value noises, ``gnoise_c``: M_c x p' gradient
    noises."""
    om = alc._weights(omega, Ur.shape[0])
    Ur = np.asarray(Ur, dtype=np.float64)
    base = (m.U, m.Ug, m.gdirs)
    ref = (Ur, Ur[:0], np.zeros(0, dtype=int))
    Kbb = _cov(base, base, m.kern, LD) + np.diag(np.concatenate([np.asarray(m.noise, dtype=LD), np.asarray(m.gnoise, dtype=LD)]))
    L = alc.chol(Kbb)
    V = alc.forward_solve(L, _cov(base, ref, m.kern, LD))
    before = LD(m.kern[1]) - (V * V).sum(0)
    out = []
    for c in range(Uc.shape[0]):
        _, cand = _sets(m, np.asarray(Uc[c], dtype=np.float64), dirs)
        noise = np.concatenate([[LD(noise_c[c])], np.asarray(gnoise_c[c], dtype=LD).reshape(-1)])
        Vn = _extend(L, V, _cov(base, cand, m.kern, LD), _cov(cand, cand, m.kern, LD) + np.diag(noise), _cov(cand, ref, m.kern, LD))
        after = before - (Vn * Vn).sum(0)
        out.append(om @ before - om @ after)
    return np.array(out, dtype=LD)


def closed_form(m, Uc, noise_c, gnoise_c, dirs, Ur, omega=None, fp64=False):
    """sum_r omega_r c_r^T S_c^-1 c_r per candidate (module docstring), and the value-only score c_r0^2 / S_c00.  Returns (with the
    gradient, value alone) in long double, or with ``fp64`` (float64 numpy throughout) (with, value, max cond(S_c))."""
    ld = np.float64 if fp64 else LD
    Ur = np.asarray(Ur, dtype=np.float64)
    om = np.asarray(alc._weights(omega, Ur.shape[0]), dtype=ld)
    base = (m.U, m.Ug, m.gdirs)
    ref = (Ur, Ur[:0], np.zeros(0, dtype=int))
    Ky = _cov(base, base, m.kern, ld) + np.diag(np.concatenate([np.asarray(m.noise, dtype=ld), np.asarray(m.gnoise, dtype=ld)]))
    if fp64:
        L = np.linalg.cholesky(Ky)
        solve = lambda B: np.linalg.solve(L, B)  # noqa: E731
    else:
        L = alc.chol(Ky)
        solve = lambda B: alc.forward_solve(L, B)  # noqa: E731
    Vr = solve(_cov(base, ref, m.kern, ld))
    with_g, value, cond = [], [], 0.0
    for c in range(Uc.shape[0]):
        _, cand = _sets(m, np.asarray(Uc[c], dtype=np.float64), dirs)
        Vc = solve(_cov(base, cand, m.kern, ld))
        C = _cov(cand, ref, m.kern, ld) - Vc.T @ Vr                      # b x M_r
        S = _cov(cand, cand, m.kern, ld) - Vc.T @ Vc + np.diag(np.concatenate([[ld(noise_c[c])], np.asarray(gnoise_c[c], dtype=ld).reshape(-1)]))
        if fp64:
            Lc = np.linalg.cholesky(S)
            Ct = np.linalg.solve(Lc, C)
            cond = max(cond, float(np.linalg.cond(S)))
        else:
            Ct = alc.forward_solve(alc.chol(S), C)
        with_g.append((Ct * Ct).sum(0) @ om)
        value.append((C[0] * C[0]) @ om / S[0, 0])
    if fp64:
        return np.array(with_g), np.array(value), cond
    return np.array(with_g, dtype=LD), np.array(value, dtype=LD)

"""CPU references of conditioning on gradient observations (``GP_Plus.condition_on_gradients``, gpp_kernel_dxdx in ``include/gpp.h``).

  ``d2k``              the block H[a nd + j][b nd + l] = d^2 (sf2 k(u, v; w)) / du_{d0+j} dv_{d0+l} at u = Ua_a, v = Ub_b in ``np.longdouble``,
                       by the chain rule on F(q1, q2) = sf2 exp(-q1) H(q2), q_f = sum over the dims of factor f of w_d (u_d - v_d)^2:
                           d^2 F / du_j dv_l = F_ab (dq_a / du_j) (dq_b / dv_l) + [j == l] F_a d^2 q_a / du_j dv_j,     a = f(j), b = f(l),
                       with dq / du_j = 2 w_j D_j, dq / dv_l = -2 w_l D_l, d^2 q / du_j dv_j = -2 w_j, F_1 = -F, F_11 = F, F_2 = sf2 e1 H',
                       F_12 = -sf2 e1 H', F_22 = sf2 e1 H'' and, with r = sqrt(2 nu 2 q2), H' = -3 e^-r, H'' = 9 e^-r / r (Matern 3/2) or
                       H' = -(5/3)(1 + r) e^-r, H'' = (25/3) e^-r (Matern 5/2).  The Matern-3/2 F_22 term is 36 w_j w_l D_j D_l e^-r / r
                       with |sqrt(w_j) D_j| <= r / sqrt(6): at most 6 sqrt(w_j w_l) r e^-r, and 0 where r = 0;
  ``d2k_bound``        the elementwise bound an fp64 evaluation by gpp_kernel_dxdx must meet (below);
  ``oracle_spec``      (w, sf2, kind, d_split, d0, nd) of an ``OracleGP``'s kernel over its feature rows;
  ``gek_posterior``    the dense fp64 gradient-enhanced posterior on the pieces of ``tests/gradpost_reference.py``: the joint (N + q)^2
                       covariance of [y; grad f at the gradient points] is formed, factored and solved (``route="joint"``), or the
                       same posterior by the Schur complement of the function block (``route="schur"``).

The bound (first order in u = 2^-53).  The kernel forms g = 2 w (exact), p_j = fl(g_j fl(ua_j - vb_j)) (2 u), the product fl(p_j p_l)
(u) and one fused multiply-add fl(p_j p_l m_F - [j == l] fl(g_j m_f)) (u of the result, u of the rounded diagonal term): with
t1 = -[j == l] g_j m_f and t2 = p_j p_l m_F the error is at most 2 u |t1| + 6 u |t2| plus the multipliers' own errors, taken as
    |H - ref| <= 4 u |t1| + 8 u |t2| + [j == l] g_j dm_f + |p_j p_l| dm_F,        f = f(j), F = f(j) + f(l),
dm_0 and dm_1 those of ``pathwise_grad_reference.kernel_multiplier_errors`` (the staged arithmetic the kernel repeats) and, in the same
style, dm_2 = sf2 e1 (|h''| (dr2_rbf + EXP_REL_ERR + 3 u) + c'' dr + 12 u |h''|) for m_2 = -sf2 e1 h'': c'' = sup |dh''/dr| = 25 / 3 for
Matern 5/2; for Matern 3/2 |dh''/dr| = 9 e^-r (1 / r + 1 / r^2) is decreasing, so c'' is its value at r - dr (the mean value theorem; no
bound where dr >= r), and where r == 0 the kernel's multiplier is an exact 0 by construction, like the reference's term: dm_2 = 0.

Nothing here touches a GPU or the library."""
import numpy as np
import torch

import gradpost_reference as gr
import pathwise_grad_reference as PG
import pathwise_reference as R
from oracle.gp_oracle import softplus

LD = np.longdouble
U53 = R.U53
KINDS = {"Matern32Kernel": R.KIND_MATERN32, "Matern52Kernel": R.KIND_MATERN52}


def _parts(Ua, Ub, w, sf2, kind, d_split, ld):
    """(F, F_2 = sf2 e1 H', F_22 = sf2 e1 H'', r, split) per pair; the Matern-3/2 F_22 is 0 where r = 0 (its term's limit)."""
    D = Ua.shape[1]
    s = R._split(D, kind, d_split)
    e1 = ld(sf2) * np.exp(-R._r2(Ua, Ub, w, 0, s, ld))
    if kind == R.KIND_RBF:
        return e1, None, None, None, s
    q2 = R._r2(Ua, Ub, w, s, D, ld)
    two_nu = 3 if kind == R.KIND_MATERN32 else 5
    r = np.sqrt(ld(2 * two_nu) * q2)
    er = np.exp(-r)
    if kind == R.KIND_MATERN32:
        H, H1 = (1 + r) * er, -ld(3) * er
        with np.errstate(divide="ignore", invalid="ignore"):
            H2 = np.where(r > 0, ld(9) * er / np.where(r > 0, r, 1), ld(0))
    else:
        H, H1, H2 = (1 + r + r * r / 3) * er, -(ld(5) / ld(3)) * (1 + r) * er, (ld(25) / ld(3)) * er
    return e1 * H, e1 * H1, e1 * H2, r, s


def _terms(Ua, Ub, w, sf2, kind, d_split, d0, nd, ld=LD):
    """(t1, t2, |p_j p_l|) as (Ma, nd, Mb, nd) arrays, the factor f(j) of each differentiated feature and their weights."""
    Ma, Mb = Ua.shape[0], Ub.shape[0]
    F, F2, F22, _, s = _parts(Ua, Ub, w, sf2, kind, d_split, ld)
    wd = np.asarray(w, dtype=ld)[d0:d0 + nd]
    Dl = Ua[:, None, d0:d0 + nd].astype(ld) - Ub[None, :, d0:d0 + nd].astype(ld)  # Ma x Mb x nd
    du = 2 * wd * Dl     # dq / du_j
    dv = -2 * wd * Dl    # dq / dv_l
    fac = (np.arange(d0, d0 + nd) >= s).astype(int)
    t1 = np.zeros((Ma, nd, Mb, nd), dtype=ld)
    t2 = np.zeros((Ma, nd, Mb, nd), dtype=ld)
    for j in range(nd):
        Fa = -F if fac[j] == 0 else F2
        t1[:, j, :, j] = Fa * (-2 * wd[j])
        for l in range(nd):
            Fab = F if fac[j] + fac[l] == 0 else (-F2 if fac[j] + fac[l] == 1 else F22)
            t2[:, j, :, l] = Fab * du[:, :, j] * dv[:, :, l]
    pp = np.abs(du[:, :, :, None] * dv[:, :, None, :]).transpose(0, 2, 1, 3)
    return t1, t2, pp, fac, wd


def d2k(Ua, Ub, w, sf2, kind=R.KIND_RBF, d_split=0, d0=0, nd=None, ld=LD):
    """H as an (Ma nd) x (Mb nd) array of ``ld``."""
    nd = Ua.shape[1] - d0 if nd is None else nd
    t1, t2, _, _, _ = _terms(np.asarray(Ua), np.asarray(Ub), w, sf2, kind, d_split, d0, nd, ld)
    return (t1 + t2).reshape(Ua.shape[0] * nd, Ub.shape[0] * nd)


def multiplier_errors(Ua, Ub, w, sf2, kind, d_split, ld=LD):
    """[dm_0] (RBF kind) or [dm_0, dm_1, dm_2] (module docstring)."""
    dms = PG.kernel_multiplier_errors(Ua, Ub, w, sf2, kind, d_split, ld)
    if kind == R.KIND_RBF:
        return dms
    D = Ua.shape[1]
    s = R._split(D, kind, d_split)
    e1 = np.exp(-R._r2(Ua, Ub, w, 0, s, ld))
    rel = R._dr2(Ua, Ub, w, 0, s, ld) + R.EXP_REL_ERR + 3 * U53
    r2m = R._r2(Ua, Ub, w, s, D, ld)
    dr2 = R._dr2(Ua, Ub, w, s, D, ld)
    c = ld(2 * (3 if kind == R.KIND_MATERN32 else 5))
    r = np.sqrt(c * r2m)
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(r2m > 0, dr2 / (2 * np.sqrt(r2m)), np.inf)
    dr = np.sqrt(c) * np.minimum(np.sqrt(dr2), lin) + 4 * U53 * r
    er = np.exp(-r)
    if kind == R.KIND_MATERN52:
        h2, slope = (ld(25) / ld(3)) * er, ld(25) / ld(3)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            lo = r - dr
            ok = lo > 0
            lo = np.where(ok, lo, 1)
            h2 = np.where(r > 0, 9 * er / np.where(r > 0, r, 1), 0)
            slope = np.where(ok, 9 * np.exp(-lo) * (1 / lo + 1 / (lo * lo)), np.where(r > 0, np.inf, 0))
    with np.errstate(invalid="ignore"):
        dm2 = ld(sf2) * e1 * (np.abs(h2) * rel + np.where(dr > 0, slope * dr, 0) + 12 * U53 * np.abs(h2))
    return [dms[0], dms[1], dm2]


def d2k_bound(Ua, Ub, w, sf2, kind, d_split, d0, nd, ld=LD):
    """(ref, bound), both (Ma nd) x (Mb nd)."""
    Ua, Ub = np.asarray(Ua), np.asarray(Ub)
    Ma, Mb = Ua.shape[0], Ub.shape[0]
    t1, t2, pp, fac, wd = _terms(Ua, Ub, w, sf2, kind, d_split, d0, nd, ld)
    dms = multiplier_errors(Ua, Ub, w, sf2, kind, d_split, ld)
    bound = 4 * U53 * np.abs(t1) + 8 * U53 * np.abs(t2)
    for j in range(nd):
        bound[:, j, :, j] += 2 * wd[j] * dms[fac[j]]
        for l in range(nd):
            bound[:, j, :, l] += pp[:, j, :, l] * dms[fac[j] + fac[l]]
    return (t1 + t2).reshape(Ma * nd, Mb * nd), bound.reshape(Ma * nd, Mb * nd)


# ---- the dense gradient-enhanced posterior ------------------------------------------------------------------------------------------
def oracle_spec(o):
    """(w, sf2, kind, d_split, d0, nd) over the rows of ``o.features``: unit lengthscales on the latent dims, the ARD ones behind."""
    wq = 0.5 / o.lengthscale().reshape(-1) ** 2
    w = torch.cat([torch.full((o.dz,), 0.5, dtype=torch.float64), wq]).detach().numpy()
    sf2 = float(softplus(o.params["covar_module.raw_outputscale"]))
    return w, sf2, KINDS.get(o.kclass, R.KIND_RBF), o.dz, o.dz, len(o.quant_index)


def _dk(o, x_diff, U_other):
    """[n, a p + j] = d/dx_{a, quant j} sf2 k(features(x_a), U_other_n): rows = the other points, as ``gradient_posterior`` forms it."""
    qi = list(o.quant_index)
    J = torch.autograd.functional.jacobian(lambda x: o.prior_cov(o.features(x), U_other).sum(0), x_diff)  # n x Ma x C
    return J[:, :, qi].reshape(U_other.shape[0], x_diff.shape[0] * len(qi)).detach()


def _d2k_t(o, xa, xb):
    w, sf2, kind, d_split, d0, nd = oracle_spec(o)
    Ua, Ub = o.features(xa).detach().numpy(), o.features(xb).detach().numpy()
    return torch.tensor(d2k(Ua, Ub, w, sf2, kind, d_split, d0, nd).astype(np.float64))


def gek_posterior(o, xg, dY, noise, xt, route="joint"):
    """The posterior at the raw rows ``xt`` of the oracle's GP conditioned on its training data and on the gradients ``dY`` (Mg x p, y
    per input unit) at the raw rows ``xg`` with noise variances ``noise`` (broadcast to Mg x p, (y per input unit)^2).  Returns a dict,
    everything in the units of y: ``mean`` (M), ``var`` (M, latent), ``std`` (M, with the test rows' own noise), ``gmean`` (M x p),
    ``gvar`` (M x p, unclamped)."""
    with torch.no_grad():
        xg, xt = torch.as_tensor(xg, dtype=torch.float64), torch.as_tensor(xt, dtype=torch.float64)
        p = len(o.quant_index)
        Mg, M, N = xg.shape[0], xt.shape[0], o.train_x.shape[0]
        ys = float(o.y_std)
        rg = (torch.as_tensor(dY, dtype=torch.float64) / ys).reshape(Mg * p)
        ng = (torch.as_tensor(noise, dtype=torch.float64) / ys ** 2).expand(Mg, p).reshape(Mg * p)
        m_tr, K_tr = o.forward(o.train_x)
        Kff = K_tr + torch.diag(o.noise_vector(o.train_x))
        rf = o.y_sc - m_tr
        Utr, Us = o.features(o.train_x), o.features(xt)
    Kfg = _dk(o, xg, Utr)                      # N x q
    Ksg = _dk(o, xg, Us)                       # M x q: cov(f(xt_s), d_j f(xg_a))
    Dsf = _dk(o, xt, Utr).T                    # (M p) x N: cov(d_j f(xt_s), f(x_n))
    with torch.no_grad():
        Kgg = _d2k_t(o, xg, xg) + torch.diag(ng)
        Dsg = _d2k_t(o, xt, xg)                # (M p) x q
        Ksf = o.prior_cov(Us, Utr)
        kss = softplus(o.params["covar_module.raw_outputscale"]).expand(M)
        kap = gr.kappa(o).repeat(M)
        A = torch.cat([Ksf, Ksg], 1)           # M x (N + q)
        B = torch.cat([Dsf, Dsg], 1)           # (M p) x (N + q)
        r = torch.cat([rf, rg])
        if route == "joint":
            S = torch.cat([torch.cat([Kff, Kfg], 1), torch.cat([Kfg.T, Kgg], 1)], 0)
            L = torch.linalg.cholesky(S)
            z = torch.linalg.solve_triangular(L, r[:, None], upper=False)[:, 0]
            VA = torch.linalg.solve_triangular(L, A.T, upper=False)
            VB = torch.linalg.solve_triangular(L, B.T, upper=False)
        elif route == "schur":
            L = torch.linalg.cholesky(Kff)
            W = torch.linalg.solve_triangular(L, Kfg, upper=False)          # L^-1 k
            Ls = torch.linalg.cholesky(Kgg - W.T @ W)
            zf = torch.linalg.solve_triangular(L, rf[:, None], upper=False)[:, 0]
            zg = torch.linalg.solve_triangular(Ls, (rg - W.T @ zf)[:, None], upper=False)[:, 0]
            z = torch.cat([zf, zg])

            def half(Op):
                top = torch.linalg.solve_triangular(L, Op[:, :N].T, upper=False)
                bot = torch.linalg.solve_triangular(Ls, Op[:, N:].T - W.T @ top, upper=False)
                return torch.cat([top, bot], 0)

            VA, VB = half(A), half(B)
        else:
            raise ValueError(route)
        mean = o.mean(xt) + VA.T @ z
        var = kss - (VA * VA).sum(0)
        gmean = (VB.T @ z).reshape(M, p)
        gvar = (kap - (VB * VB).sum(0)).reshape(M, p)
        return {"mean": o.y_min + ys * mean, "var": var * ys ** 2,
                "std": (var.clamp_min(0) + o.noise_vector(xt)).sqrt() * abs(ys),
                "gmean": gmean * ys, "gvar": gvar * ys ** 2}


def prior_curvature_noise(o, rel):
    """``rel`` times the prior curvature of each quantitative direction, in (y per input unit)^2."""
    return rel * gr.kappa(o).detach() * float(o.y_std) ** 2


# ---- the fixture cases shared by tests/test_gek_host.py and tests/test_gpu_gek.py -----------------------------------------------------
#: name -> (fixture, training rows, model keywords, gradient points Mg).  Mg p <= 16 takes gpp_chol_append's dedicated kernels, above
#: it the composed route: c3 (12) and c1-matern52 (16) are on the first, c1 (40), c4 (30) and c1-matern32 (24) on the second.
GEK_CASES = {
    "c1": ("c1_borehole_n500.npz", None, {}, 5),
    "c3": ("c3_borehole_mixed_n100.npz", None, {"qual_dict": {0: 5, 5: 5}}, 2),
    "c4": ("c4_wing_mf_n300.npz", None, {"qual_dict": {10: 3}, "multiple_noise": True, "m_gp": "multiple_constant"}, 3),
    "c1-matern52": ("c1_borehole_n500.npz", 200, {"quant_correlation_class": "Matern52Kernel"}, 2),
    "c1-matern32": ("c1_borehole_n500.npz", 200, {"quant_correlation_class": "Matern32Kernel"}, 3),
}
#: the explicit noise of the model-level fixtures, as a fraction of the prior curvature of each direction (1e-4 unless the host test's
#: measured floor asks for more on a case; none does: tests/test_gek_host.py prints the floors)
GEK_NOISE_REL = {name: 1e-4 for name in GEK_CASES}
M_TEST = 24


def gek_case(name):
    """(oracle, X, y, model keywords, gradient rows xg, gradients dY, noise (p), test rows xt) of a case.  The gradient points are
    fixture test rows (on c4: the first of a low-fidelity source); the test rows are the fixture's first ``M_TEST``, the gradient
    points among them.  dY is the base posterior's own gradient there, stretched and shifted by a fixed pattern (y per input unit)."""
    fixture, n, kw, Mg = GEK_CASES[name]
    fx = gr.load_fixture(fixture)
    o = gr.load_oracle(fx, n, **kw)
    X, y = gr.fixture_xy(fx, n)
    xt = gr.fixture_test_rows(fx, M_TEST)
    if name == "c4":
        xg = xt[xt[:, -1] != 0][:Mg]
    else:
        xg = xt[:Mg]
    g0, _ = gr.gradient_posterior(o, xg)
    pattern = torch.sin(torch.arange(g0.numel(), dtype=torch.float64)).reshape(g0.shape)
    dY = 1.25 * g0 + 0.05 * g0.abs().max() * pattern
    noise = prior_curvature_noise(o, GEK_NOISE_REL[name])
    return o, X, y, kw, xg.clone(), dY, noise, xt

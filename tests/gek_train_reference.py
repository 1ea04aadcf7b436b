"""CPU fp64 reference of training on gradient observations (``objective="gek"``, gpp_gek_grad_reduce in ``include/gpp.h``).

  ``blocks``          the two derivative blocks as closed-form torch expressions of (U, Ug, w, sf2) — the formulas ``gek_reference.d2k``
                      states: Kfg[i, a nd + j] = d/du_j F(u = Ug_a, v = U_i) = F_f(j) 2 w_j D_j and Kgg[a nd + j, b nd + l] =
                      F_f(j)f(l) (2 w_j D_j)(-2 w_l D_l) + [j == l] F_f(j) (-2 w_j), with F_0 = -F, F_1 = sf2 e1 H', F_00 = F, F_01 = -F_1,
                      F_11 = sf2 e1 H''.  Where the Matern distance of a pair is 0 its r is the CONSTANT 0 (and H'' of Matern 3/2 the
                      constant 0), so that autograd never differentiates sqrt at 0: every derivative by that distance is multiplied
                      by a difference of features that vanishes there, so the masked terms are exact zeros of the true gradient;
  ``block_sums``      sum over the entries of Kfg (both triangles) and Kgg of W dK / dtheta for an arbitrary symmetric W, by autograd:
                      what gpp_gek_grad_reduce adds.  Independent of the hand-derived third-order terms;
  ``gek_mll``         log N([y - mean; dY / y_std] | 0, Kj) on an ``OracleGP``, differentiable in its raw parameters;
  ``gek_loss`` / ``gek_loss_and_grad``   -(gek_mll + priors) / n with n = N + q, and its autograd gradient by every trainable parameter.

Nothing here touches a GPU or the library."""
import math

import torch

import gek_reference as G
import pathwise_reference as R
from oracle.gp_oracle import psd_safe_cholesky, softplus

DT = torch.float64


def _split(D, kind, d_split):
    return D if kind == R.KIND_RBF else int(d_split)


def _pair_parts(Ua, Ub, w, sf2, kind, d_split):
    """(D (Ma x Mb x D), F, F_1, F_11) per pair: F = sf2 e1 H, F_1 = sf2 e1 H', F_11 = sf2 e1 H'' (None for the RBF kind)."""
    D = Ua.shape[1]
    s = _split(D, kind, d_split)
    Dl = Ua[:, None, :] - Ub[None, :, :]
    q1 = (w[:s] * Dl[..., :s] ** 2).sum(-1)
    e1 = sf2 * torch.exp(-q1)
    if kind == R.KIND_RBF:
        return Dl, e1, None, None
    q2 = (w[s:] * Dl[..., s:] ** 2).sum(-1)
    pos = q2 > 0
    c = 6.0 if kind == R.KIND_MATERN32 else 10.0
    r = torch.where(pos, torch.sqrt(c * torch.where(pos, q2, torch.ones_like(q2))), torch.zeros_like(q2))
    er = torch.exp(-r)
    if kind == R.KIND_MATERN32:
        H, H1 = (1 + r) * er, -3.0 * er
        H2 = torch.where(pos, 9.0 * er / torch.where(pos, r, torch.ones_like(r)), torch.zeros_like(r))
    else:
        H, H1, H2 = (1 + r + r * r / 3) * er, -(5.0 / 3.0) * (1 + r) * er, (25.0 / 3.0) * er
    return Dl, e1 * H, e1 * H1, e1 * H2


def blocks(U, Ug, w, sf2, kind, d_split, d0, nd):
    """(Kfg (N x q), Kgg (q x q)), q = Mg nd, as differentiable fp64 torch tensors."""
    N, D = U.shape
    Mg = Ug.shape[0]
    s = _split(D, kind, d_split)
    fac = [1 if d0 + j >= s else 0 for j in range(nd)]
    wd = w[d0:d0 + nd]
    # function / gradient block: u = Ug_a, v = U_i
    Dl, F, F1, _ = _pair_parts(Ug, U, w, sf2, kind, d_split)
    du = 2 * wd * Dl[..., d0:d0 + nd]                                # Mg x N x nd
    Fa = torch.stack([(-F if f == 0 else F1) for f in fac], -1)       # Mg x N x nd
    Kfg = (Fa * du).permute(1, 0, 2).reshape(N, Mg * nd)
    # gradient / gradient block: u = Ug_a, v = Ug_b
    Dl, F, F1, F11 = _pair_parts(Ug, Ug, w, sf2, kind, d_split)
    du = 2 * wd * Dl[..., d0:d0 + nd]                                # Mg x Mg x nd
    Fa = torch.stack([(-F if f == 0 else F1) for f in fac], -1)
    rows = []
    for j in range(nd):
        cols = []
        for l in range(nd):
            m = fac[j] + fac[l]
            Fab = F if m == 0 else (-F1 if m == 1 else F11)
            e = Fab * du[..., j] * (-du[..., l])
            if j == l:
                e = e + Fa[..., j] * (-2 * wd[j])
            cols.append(e)
        rows.append(torch.stack(cols, -1))                            # Mg x Mg x nd (l)
    Kgg = torch.stack(rows, 1)                                        # Mg (a) x nd (j) x Mg (b) x nd (l)
    return Kfg, Kgg.reshape(Mg * nd, Mg * nd)


def block_sums(U, Ug, w, sf2, kind, d_split, d0, nd, W, dU):
    """(g_w (D), g_sf2, g_U (N x dU), g_Ug (Mg x dU)): sum of W_rc dKj_rc / dtheta over the entries of the Kfg block — counted for both
    triangles — and of the Kgg block, for a symmetric n x n ``W``; g_sf2 = d / dsf2 = sum of W_rc Kj_rc / sf2."""
    N = U.shape[0]
    U, Ug, w = (t.detach().clone().requires_grad_(True) for t in (U, Ug, w))
    sf2 = torch.as_tensor(sf2, dtype=DT).detach().clone().requires_grad_(True)
    Kfg, Kgg = blocks(U, Ug, w, sf2, kind, d_split, d0, nd)
    total = 2 * (W[:N, N:] * Kfg).sum() + (W[N:, N:] * Kgg).sum()
    g_U, g_Ug, g_w, g_s = torch.autograd.grad(total, [U, Ug, w, sf2])
    return g_w, g_s, g_U[:, :dU].contiguous(), g_Ug[:, :dU].contiguous()


def spec_tensors(o, p=None):
    """(w, sf2, kind, d_split, d0, nd) over the rows of ``o.features``, differentiable in the raw parameters ``p``."""
    p = o.params if p is None else p
    wq = 0.5 / o.lengthscale(p).reshape(-1) ** 2
    w = torch.cat([torch.full((o.dz,), 0.5, dtype=DT), wq])
    sf2 = softplus(p["covar_module.raw_outputscale"])
    return w, sf2, G.KINDS.get(o.kclass, R.KIND_RBF), o.dz, o.dz, len(o.quant_index)


def curvature(o, p=None):
    """The prior curvature c_j w_j sf2 of each quantitative direction (scaled units), differentiable in ``p``."""
    w, sf2, kind, _, d0, nd = spec_tensors(o, p)
    c = {R.KIND_MATERN32: 6.0, R.KIND_MATERN52: 10.0 / 3.0}.get(kind, 2.0)
    return c * w[d0:d0 + nd] * sf2


def joint_matrix(o, xg, noise, p=None, nugget_rel=None):
    """Kj, (N + q)^2.  ``noise``: variances in (y per input unit)^2 that broadcast to (Mg, p), or None for ``nugget_rel`` times the
    prior curvature at the parameters ``p`` (which then depends on them)."""
    p = o.params if p is None else p
    xg = torch.as_tensor(xg, dtype=DT)
    Mg, nd = xg.shape[0], len(o.quant_index)
    w, sf2, kind, d_split, d0, _ = spec_tensors(o, p)
    U, Ug = o.features(o.train_x, p), o.features(xg, p)
    Kff = o.prior_cov(U, U, p) + torch.diag(o.noise_vector(o.train_x, p))
    Kfg, Kgg = blocks(U, Ug, w, sf2, kind, d_split, d0, nd)
    if noise is None:
        nu = (nugget_rel * curvature(o, p)).expand(Mg, nd).reshape(-1)
    else:
        nu = (torch.as_tensor(noise, dtype=DT) / float(o.y_std) ** 2).expand(Mg, nd).reshape(-1)
    return torch.cat([torch.cat([Kff, Kfg], 1), torch.cat([Kfg.T, Kgg + torch.diag(nu)], 1)], 0)


def gek_mll(o, xg, dY, noise, p=None, nugget_rel=None):
    """log N([y_scaled - mean; dY / y_std] | 0, Kj)."""
    p = o.params if p is None else p
    S = joint_matrix(o, xg, noise, p, nugget_rel)
    r = torch.cat([o.y_sc - o.mean(o.train_x, p), (torch.as_tensor(dY, dtype=DT) / float(o.y_std)).reshape(-1)])
    L, _ = psd_safe_cholesky(S)
    z = torch.linalg.solve_triangular(L, r.unsqueeze(-1), upper=False)
    return -0.5 * ((z * z).sum() + 2 * torch.log(torch.diagonal(L)).sum() + r.numel() * math.log(2 * math.pi))


def gek_loss(o, xg, dY, noise, p=None, nugget_rel=None, normalize=True):
    """-(gek_mll + priors) / n, n = N + q: the loss ``GradientEnhancedMarginalLogLikelihood`` defines (``normalize=False``: the
    un-normalised objective of the scipy driver)."""
    p = o.params if p is None else p
    n = o.N + torch.as_tensor(dY).numel()
    val = gek_mll(o, xg, dY, noise, p, nugget_rel) + o.log_priors(p)
    return -(val / n if normalize else val)


def gek_loss_and_grad(o, xg, dY, noise, nugget_rel=None, normalize=True):
    p = {k: v.clone().requires_grad_(k in o.trainable) for k, v in o.params.items()}
    loss = gek_loss(o, xg, dY, noise, p, nugget_rel, normalize)
    names = list(o.trainable)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    return loss.detach(), dict(zip(names, grads))


# ---- the fit shared by tests/test_gek_train_host.py and tests/test_gpu_gek_train.py --------------------------------------------------
FIT_N, FIT_MG = 60, 12


def fit_case():
    """(oracle, X, y, xg, dY, noise): c1 cut to ``FIT_N`` rows with ``FIT_MG`` fixture test rows as gradient points, the gradients
    made as ``gek_reference.gek_case`` makes them at the fixture's parameters, the noise 1e-4 of the prior curvature there; the
    oracle is returned with its length scales moved away from those parameters by a fixed pattern (the start of the fit)."""
    import gradpost_reference as gr

    fx = gr.load_fixture("c1_borehole_n500.npz")
    o = gr.load_oracle(fx, FIT_N)
    X, y = gr.fixture_xy(fx, FIT_N)
    xg = gr.fixture_test_rows(fx, FIT_MG).clone()
    g0, _ = gr.gradient_posterior(o, xg)
    pattern = torch.sin(torch.arange(g0.numel(), dtype=DT)).reshape(g0.shape)
    dY = 1.25 * g0 + 0.05 * g0.abs().max() * pattern
    noise = G.prior_curvature_noise(o, 1e-4)
    ls = o.params[o.ls_key]
    o.params[o.ls_key] = ls + 0.6 * torch.cos(torch.arange(ls.numel(), dtype=DT)).reshape(ls.shape)
    return o, X, y, xg, dY, noise


def fit_lbfgs(o, xg, dY, noise, nugget_rel=None, options=None):
    """The scipy driver's L-BFGS-B run (``oracle_fit_scipy``'s defaults) on the un-normalised gradient-enhanced objective from the
    oracle's current parameters, which are replaced by the result.  Returns (objective at the start, OptimizeResult)."""
    import numpy as np
    from scipy.optimize import minimize

    from oracle.gp_oracle import _pack, _unpack

    names = list(o.trainable)
    opts = {'ftol': 1e-6, 'gtol': 1e-5, 'maxfun': 5000, 'maxiter': 2000}
    opts.update(options or {})

    def fun(x):
        _unpack(o, names, x)
        p = {k: v.clone().requires_grad_(k in names) for k, v in o.params.items()}
        obj = gek_loss(o, xg, dY, noise, p, nugget_rel, normalize=False)
        grads = torch.autograd.grad(obj, [p[k] for k in names])
        return obj.item(), np.concatenate([g.numpy().ravel() for g in grads]).astype(np.float64)

    x0 = _pack(o, names)
    start = fun(x0)[0]
    res = minimize(fun=fun, x0=x0, jac=True, method='L-BFGS-B', options=opts)
    _unpack(o, names, res.x)
    return start, res

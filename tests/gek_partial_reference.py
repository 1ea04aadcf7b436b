"""CPU fp64 references of gradient-enhanced Kriging with PARTIAL gradients (``condition_on_gradients(..., observed=mask)`` and
``objective="gek"`` with ``gradients=(Xg, dY, noise, observed)``), built from the pieces of tests/gek_reference.py (``_dk``,
``_d2k_t``) and tests/gek_train_reference.py (``joint_matrix``): the joint Gaussian of the function values and of ALL Mg p gradient
components is formed as there, and the rows and columns N + nonzero(observed.reshape(-1)) of its covariance and of its right-hand
side are kept.  Marginalising a Gaussian over the unobserved components is exactly that.

  ``pattern_mask``               observed[a, j] = ((3 a + 5 j) mod 7) < 3, column 0 switched on for a point left empty;
  ``alternating_row``            [True, False, True, ...]: the same directions at every point, as a single row;
  ``gek_posterior_partial``      ``gek_reference.gek_posterior`` ("joint" route) on the observed entries;
  ``gek_loss_and_grad_partial``  ``gek_train_reference.gek_loss_and_grad`` on the observed entries, n = N + q.

Nothing here touches a GPU or the library."""
import math

import torch

import gek_reference as G
import gek_train_reference as T
import gradpost_reference as gr
from oracle.gp_oracle import psd_safe_cholesky, softplus

DT = torch.float64


def pattern_mask(Mg, p):
    a, j = torch.arange(Mg)[:, None], torch.arange(p)[None, :]
    m = ((3 * a + 5 * j) % 7) < 3
    m[~m.any(1), 0] = True
    return m


def alternating_row(p):
    return (torch.arange(p) % 2) == 0


def _keep(observed, Mg, p):
    m = torch.broadcast_to(torch.as_tensor(observed, dtype=torch.bool), (Mg, p))
    return m.reshape(-1).nonzero().reshape(-1)


def gek_posterior_partial(o, xg, dY, noise, xt, observed):
    """``gek_reference.gek_posterior(o, xg, dY, noise, xt, "joint")`` with only the entries of ``dY`` under the True entries of
    ``observed`` (broadcast to Mg x p) observed; what lies under a False entry of ``dY`` or ``noise`` is never used."""
    with torch.no_grad():
        xg, xt = torch.as_tensor(xg, dtype=DT), torch.as_tensor(xt, dtype=DT)
        p = len(o.quant_index)
        Mg, M = xg.shape[0], xt.shape[0]
        keep = _keep(observed, Mg, p)
        ys = float(o.y_std)
        rg = (torch.as_tensor(dY, dtype=DT) / ys).reshape(Mg * p)[keep]
        ng = (torch.as_tensor(noise, dtype=DT) / ys ** 2).expand(Mg, p).reshape(Mg * p)[keep]
        m_tr, K_tr = o.forward(o.train_x)
        Kff = K_tr + torch.diag(o.noise_vector(o.train_x))
        rf = o.y_sc - m_tr
        Utr, Us = o.features(o.train_x), o.features(xt)
    Kfg = G._dk(o, xg, Utr)[:, keep]           # N x q
    Ksg = G._dk(o, xg, Us)[:, keep]            # M x q
    Dsf = G._dk(o, xt, Utr).T                  # (M p) x N: the test side stays dense
    with torch.no_grad():
        Kgg = G._d2k_t(o, xg, xg)[keep][:, keep] + torch.diag(ng)
        Dsg = G._d2k_t(o, xt, xg)[:, keep]     # (M p) x q
        Ksf = o.prior_cov(Us, Utr)
        kss = softplus(o.params["covar_module.raw_outputscale"]).expand(M)
        kap = gr.kappa(o).repeat(M)
        A = torch.cat([Ksf, Ksg], 1)
        B = torch.cat([Dsf, Dsg], 1)
        r = torch.cat([rf, rg])
        S = torch.cat([torch.cat([Kff, Kfg], 1), torch.cat([Kfg.T, Kgg], 1)], 0)
        L = torch.linalg.cholesky(S)
        z = torch.linalg.solve_triangular(L, r[:, None], upper=False)[:, 0]
        VA = torch.linalg.solve_triangular(L, A.T, upper=False)
        VB = torch.linalg.solve_triangular(L, B.T, upper=False)
        mean = o.mean(xt) + VA.T @ z
        var = kss - (VA * VA).sum(0)
        gmean = (VB.T @ z).reshape(M, p)
        gvar = (kap - (VB * VB).sum(0)).reshape(M, p)
        return {"mean": o.y_min + ys * mean, "var": var * ys ** 2,
                "std": (var.clamp_min(0) + o.noise_vector(xt)).sqrt() * abs(ys),
                "gmean": gmean * ys, "gvar": gvar * ys ** 2}


def _clean(t, observed, Mg, p):
    """``t`` broadcast to (Mg, p) with zeros under the False entries (what lies there is dropped with its row and column)."""
    m = torch.broadcast_to(torch.as_tensor(observed, dtype=torch.bool), (Mg, p))
    t = torch.as_tensor(t, dtype=DT).expand(Mg, p)
    return torch.where(m, t, torch.zeros((), dtype=DT))


def gek_mll_partial(o, xg, dY, noise, observed, p=None, nugget_rel=None):
    """log N([y_scaled - mean; observed entries of dY / y_std] | 0, the same rows and columns of Kj)."""
    p = o.params if p is None else p
    xg = torch.as_tensor(xg, dtype=DT)
    Mg, nd, N = xg.shape[0], len(o.quant_index), o.N
    keep = _keep(observed, Mg, nd)
    idx = torch.cat([torch.arange(N), N + keep])
    S = T.joint_matrix(o, xg, None if noise is None else _clean(noise, observed, Mg, nd), p, nugget_rel)[idx][:, idx]
    r = torch.cat([o.y_sc - o.mean(o.train_x, p), (_clean(dY, observed, Mg, nd) / float(o.y_std)).reshape(-1)])[idx]
    L, _ = psd_safe_cholesky(S)
    z = torch.linalg.solve_triangular(L, r.unsqueeze(-1), upper=False)
    return -0.5 * ((z * z).sum() + 2 * torch.log(torch.diagonal(L)).sum() + r.numel() * math.log(2 * math.pi))


def gek_loss_partial(o, xg, dY, noise, observed, p=None, nugget_rel=None, normalize=True):
    """-(gek_mll_partial + priors) / n with n = N + q, q the number of observed entries."""
    p = o.params if p is None else p
    xg = torch.as_tensor(xg, dtype=DT)
    n = o.N + int(_keep(observed, xg.shape[0], len(o.quant_index)).numel())
    val = gek_mll_partial(o, xg, dY, noise, observed, p, nugget_rel) + o.log_priors(p)
    return -(val / n if normalize else val)


def gek_loss_and_grad_partial(o, xg, dY, noise, observed, nugget_rel=None, normalize=True):
    p = {k: v.clone().requires_grad_(k in o.trainable) for k, v in o.params.items()}
    loss = gek_loss_partial(o, xg, dY, noise, observed, p, nugget_rel, normalize)
    names = list(o.trainable)
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    return loss.detach(), dict(zip(names, grads))

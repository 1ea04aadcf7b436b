"""Dense fp64 CPU reference of the leave-one-out log pseudo-likelihood (Rasmussen & Williams, section 5.4.2; gpytorch's
LeaveOneOutPseudoLikelihood), in plain torch:

  ``loo_autograd``      gpytorch's formula through ``torch.linalg.inv``, differentiated by autograd;
  ``loo_closed_form``   the same value and the gradients from W = -(alpha beta^T + beta alpha^T) / 2 - P diag(b) P, no autograd.

The two routes share nothing beyond the covariance function; they agree to 1.5e-13 at N = 1537 on the inputs of ``make_inputs``.
The covariance is the library's: K_ij = sf2 exp(-sum_{d < split} w_d (u_id - u_jd)^2) m(a_ij), a_ij = sqrt(10 sum_{d >= split} w_d
(u_id - u_jd)^2), m(a) = (1 + a + a^2 / 3) exp(-a) for the Matern 5/2 kind (m = 1, split = D for the RBF kind), plus
diag(tau[grp]).
"""
import math

import numpy as np
import torch

KIND_RBF, KIND_MATERN52 = 0, 2
LOG_2PI = math.log(2.0 * math.pi)


def make_inputs(N, D, seed, S=3):
    """Seeded inputs of the leave-one-out tests: U uniform in [0, 1]^D, w in [0.5, 2.5], sf2 = 1, tau = (1e-2, 3e-2, 2e-2)[:S]
    by grp = i mod S (S = 1: one noise level, grp None), y = sin 3 u_0 + u_1^2 + 0.1 noise, mean = 0.2."""
    rng = np.random.default_rng(seed)
    U = torch.from_numpy(rng.uniform(0.0, 1.0, (N, D)))
    w = torch.from_numpy(rng.uniform(0.5, 2.5, D))
    sf2 = torch.tensor(1.0, dtype=torch.float64)
    tau = torch.tensor([1e-2, 3e-2, 2e-2], dtype=torch.float64)[:S]
    grp = None if S == 1 else (torch.arange(N) % S).to(torch.int32)
    y = torch.sin(3.0 * U[:, 0]) + U[:, 1 if D > 1 else 0] ** 2 + 0.1 * torch.from_numpy(rng.standard_normal(N))
    mean = torch.full((N,), 0.2, dtype=torch.float64)
    return dict(U=U, w=w, sf2=sf2, tau=tau, grp=grp, mean=mean, y=y)


def _r2(U, w, lo, hi):
    r2 = torch.zeros(U.shape[0], U.shape[0], dtype=torch.float64)
    for d in range(lo, hi):
        diff = U[:, d, None] - U[None, :, d]
        r2 = r2 + w[d] * diff * diff
    return r2


def _kernel(U, w, sf2, kind, d_split):
    """(K, KD): the noise-free covariance and sf2 * d k / d(-r2_mat), the factor of the Matern dims' derivatives."""
    D = U.shape[1]
    split = D if kind == KIND_RBF else d_split
    er = torch.exp(-_r2(U, w, 0, split))
    if kind == KIND_RBF:
        return sf2 * er, None
    # (the clamp keeps autograd's d sqrt / d r2 finite on the diagonal, where the chain rule multiplies it by an exact zero)
    a = torch.sqrt(10.0 * _r2(U, w, split, D).clamp_min(1e-300))
    ea = torch.exp(-a)
    return sf2 * er * (1.0 + a + a * a / 3.0) * ea, sf2 * er * (5.0 / 3.0) * (1.0 + a) * ea


def _noise(tau, grp, N):
    t = tau.reshape(-1)
    return t[0].expand(N) if grp is None else t[grp.to(torch.int64)]


def loo_dense(Ky, r):
    """gpytorch's LeaveOneOutPseudoLikelihood on a dense covariance and the residual r = y - mean (not divided by N)."""
    P = torch.linalg.inv(Ky)
    sigma2 = 1.0 / P.diagonal()
    diff = (P @ r) * sigma2  # y - mu
    return (-0.5 * sigma2.log() - 0.5 * diff * diff / sigma2).sum() - 0.5 * r.shape[0] * LOG_2PI


def loo_autograd(U, w, sf2, tau, grp, mean, y, kind=KIND_RBF, d_split=0):
    """Value and gradients (dict: U, w, sf2, tau, mean, y) by autograd through ``torch.linalg.inv``."""
    leaves = {k: v.detach().clone().to(torch.float64).requires_grad_(True)
              for k, v in dict(U=U, w=w, sf2=sf2, tau=tau, mean=mean, y=y).items()}
    K, _ = _kernel(leaves["U"], leaves["w"], leaves["sf2"], kind, d_split)
    Ky = K + torch.diag(_noise(leaves["tau"], grp, U.shape[0]))
    val = loo_dense(Ky, leaves["y"] - leaves["mean"])
    grads = torch.autograd.grad(val, list(leaves.values()))
    return val.detach(), dict(zip(leaves, grads))


def loo_closed_form(U, w, sf2, tau, grp, mean, y, kind=KIND_RBF, d_split=0, dU=None):
    """Value and gradients from the closed form, without autograd; dU: feature columns whose gradient is wanted (None: all)."""
    with torch.no_grad():
        U, w, sf2, tau, mean, y = (t.to(torch.float64) for t in (U, w, sf2, tau, mean, y))
        N, D = U.shape
        dU = D if dU is None else dU
        split = D if kind == KIND_RBF else d_split
        K, KD = _kernel(U, w, sf2, kind, d_split)
        P = torch.linalg.inv(K + torch.diag(_noise(tau, grp, N)))
        d = P.diagonal().clone()
        alpha = P @ (y - mean)
        val = (0.5 * d.log() - 0.5 * alpha * alpha / d).sum() - 0.5 * N * LOG_2PI
        a = -alpha / d
        b = 0.5 / d + 0.5 * alpha * alpha / (d * d)
        beta = P @ a
        W = -0.5 * (alpha[:, None] * beta[None, :] + beta[:, None] * alpha[None, :]) - (P * b[None, :]) @ P
        g = dict(w=torch.zeros(D, dtype=torch.float64), U=torch.zeros(N, D, dtype=torch.float64))
        WK = W * K
        WKD = None if KD is None else W * KD
        for dd in range(D):
            G = WK if dd < split else WKD
            diff = U[:, dd, None] - U[None, :, dd]
            g["w"][dd] = -(G * diff * diff).sum()
            if dd < dU:
                g["U"][:, dd] = -4.0 * w[dd] * (G * diff).sum(dim=1)  # row i and column i of the symmetric K both move with U_i
        g["sf2"] = WK.sum() / sf2
        Wd = W.diagonal()
        if grp is None:
            g["tau"] = Wd.sum().reshape(1)
        else:
            g["tau"] = torch.stack([Wd[grp.to(torch.int64) == s].sum() for s in range(tau.numel())])
        g["mean"], g["y"] = -beta, beta.clone()
        return val, g

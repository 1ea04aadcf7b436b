"""Dense CPU fp64 reference of the posterior of the gradient (``GP_Plus.predict_gradient`` / ``active_subspace``), built on
``oracle.gp_oracle.OracleGP`` as ``tests/test_gpu_predict_grad.py::_oracle_grads`` builds its own:

    grad f(x_a) | data ~ N(g_a, S_a),   g_a = d mean(x_a) / dx,   S_a = diag(kappa) - Q_a^T Q_a,   Q_a = L^-1 Dk_a

  ``kappa``            the prior variances of the gradient's components in closed form, c_j w_j sf2 with w_j = 1 / (2 l_j^2) and
                       c_j = 2 (RBF kinds), 6 (Matern 3/2) or 10 / 3 (Matern 5/2);
  ``posterior_mean``   the oracle's posterior mean at raw test rows (scaled units), differentiable;
  ``gradient_posterior``   (g, S) in the units of y: g by ``torch.autograd.functional.jacobian`` of the posterior mean with respect
                       to the test rows, Dk by autograd of ``o.prior_cov(o.features(xt), o.features(train))``, Q by a dense
                       triangular solve;
  ``active_subspace``  sum_a w_a (g_a g_a^T + S_a) and its two parts;
  ``load_oracle``      an oracle at a fixture's ``theta1``.

Only the quantitative columns (``o.quant_index``, in that order) are differentiated.  Nothing here touches a GPU or the library."""
import os

import numpy as np
import torch

from oracle.gp_oracle import OracleGP, psd_safe_cholesky, softplus

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def load_fixture(name):
    return dict(np.load(os.path.join(GOLD, name)))


def fixture_xy(fx, n=None):
    xkey = "Xtrain" if "Xtrain" in fx else "Utrain"
    return fx[xkey][:n], fx["ytrain"][:n]


def fixture_test_rows(fx, m=40):
    return torch.tensor(fx["Xtest"] if "Xtest" in fx else fx["Utest"], dtype=torch.float64)[:m]


def load_oracle(fx, n=None, **kw):
    """The oracle on the fixture's first ``n`` training rows with the parameters of its ``theta1``."""
    X, y = fixture_xy(fx, n)
    o = OracleGP(X, y, **kw)
    for k in list(o.params):
        o.params[k] = torch.as_tensor(fx[f"theta1::param::{k}"], dtype=torch.float64).reshape(o.params[k].shape)
    return o


def kappa(o):
    """kappa_j = d^2 (sf2 k) / du_j du'_j at u' = u for the quantitative columns (scaled units)."""
    w = 0.5 / o.lengthscale().reshape(-1) ** 2
    c = {"Matern32Kernel": 6.0, "Matern52Kernel": 10.0 / 3.0}.get(o.kclass, 2.0)
    return c * w * softplus(o.params["covar_module.raw_outputscale"])


def _factor(o):
    m_tr, K_tr = o.forward(o.train_x)
    L, _ = psd_safe_cholesky(K_tr + torch.diag(o.noise_vector(o.train_x)))
    alpha = torch.cholesky_solve((o.y_sc - m_tr).unsqueeze(-1), L).squeeze(-1)
    return L, alpha


def posterior_mean(o, xt, alpha=None):
    if alpha is None:
        alpha = _factor(o)[1]
    return o.mean(xt) + o.prior_cov(o.features(xt), o.features(o.train_x)) @ alpha


def gradient_posterior(o, xt):
    """(g (M, p), S (M, p, p)) in the units of y per input unit."""
    with torch.no_grad():
        L, alpha = _factor(o)
    M, N = xt.shape[0], o.train_x.shape[0]
    qi = list(o.quant_index)
    p = len(qi)
    J = torch.autograd.functional.jacobian(lambda x: posterior_mean(o, x, alpha), xt)  # M x M x C: row a depends on xt[a] alone
    g = J[torch.arange(M), torch.arange(M)][:, qi]
    Utr = o.features(o.train_x).detach()
    # column n of the cross block summed over the test rows: only row a of it depends on xt[a]
    Jk = torch.autograd.functional.jacobian(lambda x: o.prior_cov(o.features(x), Utr).sum(0), xt)  # N x M x C
    Dk = Jk[:, :, qi].reshape(N, M * p)
    Q = torch.linalg.solve_triangular(L, Dk, upper=False).reshape(N, M, p)
    G = torch.einsum("naj,nak->ajk", Q, Q)
    S = torch.diag(kappa(o)).unsqueeze(0) - G
    S = 0.5 * (S + S.transpose(1, 2))
    return g.detach() * o.y_std, S.detach() * o.y_std ** 2


def active_subspace(g, S, weights=None):
    """(matrix, mean part, covariance part) from ``gradient_posterior``'s outputs."""
    M = g.shape[0]
    w = torch.full((M,), 1.0 / M, dtype=torch.float64) if weights is None else torch.as_tensor(weights, dtype=torch.float64)
    mean_part = torch.einsum("a,aj,ak->jk", w, g, g)
    cov_part = torch.einsum("a,ajk->jk", w, S)
    return mean_part + cov_part, mean_part, cov_part

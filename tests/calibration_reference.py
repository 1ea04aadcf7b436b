"""Dense CPU fp64 reference of deterministic calibration (``GP_Plus(..., calibration_id=[...])``), built on
``oracle.gp_oracle.OracleGP`` the way ``tests/gradpost_reference.py`` is.

The reference model (models/gp_plus.py:311-320, 439-461) gives every id ``n`` of ``calibration_id`` a parameter ``Theta_<n>.constant``
with a ``NormalPrior(mean_prior, std_prior)``, zeroes column ``n`` of the training rows of source 0 and, in every forward, writes
the parameter into feature column ``d_z + position of n among the quantitative columns`` of the rows whose last column is 0.  Here:

  ``CalibratedOracle``      an ``OracleGP`` on the zeroed inputs plus the ``Theta_<n>.constant`` entries in ``params``;
  ``.features``             the oracle's features with theta substituted (out of place: autograd reaches theta);
  ``.loss``                 -(log N(y | m, K + diag(noise)) + priors, theta's included), divided by N as ``ExactMarginalLogLikelihood``
                            does (``normalize=True``) or not, as ``fit_model_scipy`` does;
  ``.loss_and_grad``        the value and the gradient by every parameter, theta included, by torch autograd;
  ``.predict``              posterior mean and standard deviation at test rows, un-scaled, as ``OracleGP.predict``;
  ``.fit_lbfgs``            scipy L-BFGS-B on ``loss(normalize=False)`` from the current parameters (``oracle_fit_scipy``'s options);
  ``central_differences``   (f(v + h) - f(v - h)) / 2h of ``loss`` by one scalar entry of one parameter;
  ``kernel_operands``       what gpp_calib_grad_reduce / gpp_grad_reduce take — U, w, sf2, kind, d_split, alpha, Ky^-1, member, cols —
                            and the reference value of g_theta = d mll / d theta, by autograd through the dense mll.

Nothing here touches a GPU or the library."""
import math
import os

import numpy as np
import torch

from oracle.gp_oracle import OracleGP, normal_log_prob, psd_safe_cholesky, softplus

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DT = torch.float64
C4_KW = {"qual_dict": {10: 3}, "multiple_noise": True, "m_gp": "multiple_constant"}


def load_fixture(name="c4_wing_mf_n300.npz"):
    return dict(np.load(os.path.join(GOLD, name)))


class CalibratedOracle:
    def __init__(self, train_x, train_y, calibration_id, mean_prior_cal=None, std_prior_cal=None, source_index=0, **kw):
        X = torch.as_tensor(np.asarray(train_x), dtype=DT).clone()
        self.ids = list(calibration_id)
        self.source_index = source_index
        self.mean_prior = [0.0] * len(self.ids) if mean_prior_cal is None else [float(v) for v in mean_prior_cal]
        self.std_prior = [1.0] * len(self.ids) if std_prior_cal is None else [float(v) for v in std_prior_cal]
        if torch.isnan(X).any():  # models/gp_plus.py:604-618 (the calibrated entries are zeroed below whatever stood there)
            means = torch.nanmean(X, dim=0)
            nan = torch.isnan(X)
            X[nan] = means.repeat(X.shape[0], 1)[nan]
        rows = X[:, -1] == source_index
        for n in self.ids:
            X[rows, n] = 0.0  # models/gp_plus.py:320
        self.o = OracleGP(X, train_y, **kw)
        for n in self.ids:
            assert n in self.o.quant_index, n
            self.o.params[f"Theta_{n}.constant"] = torch.zeros(1, dtype=DT)
            self.o.trainable.append(f"Theta_{n}.constant")
        self.cols = [self.o.dz + self.o.quant_index.index(n) for n in self.ids]

    @property
    def params(self):
        return self.o.params

    def member(self, x):
        return x[:, -1] == self.source_index

    def features(self, x, p=None):
        p = self.o.params if p is None else p
        U = self.o.features(x, p)
        m = self.member(x)
        columns = [U[:, c] for c in range(U.shape[1])]
        for n, c in zip(self.ids, self.cols):
            columns[c] = torch.where(m, p[f"Theta_{n}.constant"].reshape(()).expand(U.shape[0]), U[:, c])
        return torch.stack(columns, dim=1)

    def log_priors(self, p=None):
        p = self.o.params if p is None else p
        tot = self.o.log_priors(p)
        for n, mu, sd in zip(self.ids, self.mean_prior, self.std_prior):
            tot = tot + normal_log_prob(p[f"Theta_{n}.constant"], mu, sd).sum()
        return tot

    def mll(self, p=None, rows=None):
        """log N(y | m, Ky) of the training rows (or of the subset ``rows`` of them, with the scaling of the whole set)."""
        o = self.o
        p = o.params if p is None else p
        x, y = (o.train_x, o.y_sc) if rows is None else (o.train_x[rows], o.y_sc[rows])
        U = self.features(x, p)
        Ky = o.prior_cov(U, U, p) + torch.diag(o.noise_vector(x, p))
        L, _ = psd_safe_cholesky(Ky)
        z = torch.linalg.solve_triangular(L, (y - o.mean(x, p)).unsqueeze(-1), upper=False)
        return -0.5 * ((z * z).sum() + 2 * torch.log(torch.diagonal(L)).sum() + x.shape[0] * math.log(2 * math.pi))

    def loss(self, p=None, normalize=True, add_prior=True):
        val = self.mll(p)
        if add_prior:
            val = val + self.log_priors(p)
        return -(val / self.o.N if normalize else val)

    def loss_and_grad(self, normalize=True):
        names = list(self.o.trainable)
        p = {k: v.clone().requires_grad_(k in names) for k, v in self.o.params.items()}
        loss = self.loss(p, normalize)
        grads = torch.autograd.grad(loss, [p[k] for k in names])
        return loss.detach(), dict(zip(names, grads))

    @torch.no_grad()
    def predict(self, xtest, include_noise=True):
        o = self.o
        xtest = torch.as_tensor(np.asarray(xtest), dtype=DT)
        Utr, Ute = self.features(o.train_x), self.features(xtest)
        L, _ = psd_safe_cholesky(o.prior_cov(Utr, Utr) + torch.diag(o.noise_vector(o.train_x)))
        alpha = torch.cholesky_solve((o.y_sc - o.mean(o.train_x)).unsqueeze(-1), L).squeeze(-1)
        Ksn = o.prior_cov(Ute, Utr)
        mean = o.mean(xtest) + Ksn @ alpha
        V = torch.linalg.solve_triangular(L, Ksn.T, upper=False)
        var = softplus(o.params["covar_module.raw_outputscale"]).expand(xtest.shape[0]) - (V * V).sum(0)
        if include_noise:
            var = var + o.noise_vector(xtest)
        return o.y_min + o.y_std * mean, var.clamp_min(1e-10).sqrt() * o.y_std

    def fit_lbfgs(self, options=None):
        """L-BFGS-B on -(mll + priors), not divided by N, from the current parameters; the best point is left in ``params``."""
        from scipy.optimize import minimize

        opts = {'ftol': 1e-6, 'gtol': 1e-5, 'maxfun': 5000, 'maxiter': 2000}
        opts.update(options or {})
        names = list(self.o.trainable)
        shapes = [self.o.params[k].shape for k in names]

        def unpack(x):
            i = 0
            for k, s in zip(names, shapes):
                n = int(np.prod(s)) if len(s) else 1
                self.o.params[k] = torch.from_numpy(np.asarray(x[i:i + n], dtype=np.float64).copy()).reshape(s)
                i += n

        def fun(x):
            unpack(x)
            v, g = self.loss_and_grad(normalize=False)
            return v.item(), np.concatenate([g[k].numpy().ravel() for k in names]).astype(np.float64)

        x0 = np.concatenate([self.o.params[k].numpy().ravel() for k in names]).astype(np.float64)
        f0 = fun(x0)[0]
        res = minimize(fun, x0, jac=True, method='L-BFGS-B', options=opts)
        unpack(res.x)
        return f0, res


def central_differences(co, name, index, h, normalize=True):
    """(loss(v + h) - loss(v - h)) / 2h by entry ``index`` (flat) of parameter ``name``."""
    saved = co.params[name].clone()
    out = []
    for sgn in (1.0, -1.0):
        v = saved.clone().reshape(-1)
        v[index] += sgn * h
        co.params[name] = v.reshape(saved.shape)
        with torch.no_grad():
            out.append(co.loss(normalize=normalize).item())
    co.params[name] = saved
    return (out[0] - out[1]) / (2.0 * h)


KINDS = {"Rough_RBF": 0, "RBFKernel": 0, "Matern32Kernel": 1, "Matern52Kernel": 2}


def kernel_operands(co, rows=None):
    """The operands of the calibration reduction at ``co``'s parameters for the training rows (or the subset ``rows``, in that
    order), on the CPU, and the reference gradient: dict(U, w, sf2, kind, d_split, alpha, Kinv, member, cols, grp, S, g_theta)
    with g_theta[k] = d mll / d Theta_k by autograd through the dense mll of those rows."""
    o = co.o
    names = [f"Theta_{n}.constant" for n in co.ids]
    p = {k: v.clone().requires_grad_(k in names) for k, v in o.params.items()}
    g = torch.autograd.grad(co.mll(p, rows), [p[k] for k in names], allow_unused=True)
    g = [torch.zeros(1, dtype=DT) if v is None else v.reshape(1) for v in g]
    with torch.no_grad():
        x, y = (o.train_x, o.y_sc) if rows is None else (o.train_x[rows], o.y_sc[rows])
        U = co.features(x)
        Ky = o.prior_cov(U, U) + torch.diag(o.noise_vector(x))
        L, _ = psd_safe_cholesky(Ky)
        Kinv = torch.cholesky_inverse(L)
        alpha = Kinv @ (y - o.mean(x))
        w = torch.zeros(U.shape[1], dtype=DT)
        w[: o.dz] = 0.5
        w[o.dz:] = 0.5 / o.lengthscale().reshape(-1) ** 2
        kind = KINDS[o.kclass]
        S = max(1, len(o.noise_indices))
        grp = x[:, -1].to(torch.int32) if o.noise_indices else None
    return dict(U=U.contiguous(), w=w, sf2=softplus(o.params["covar_module.raw_outputscale"]).reshape(1), kind=kind,
                d_split=o.dz if kind else 0, alpha=alpha, Kinv=Kinv, member=co.member(x).to(torch.int32),
                cols=torch.tensor(co.cols, dtype=torch.int32), grp=grp, S=S, g_theta=torch.cat(g))

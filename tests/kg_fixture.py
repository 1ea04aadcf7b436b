"""The multi-fidelity fixture c4_wing_mf_n300 as the knowledge-gradient tests use it (host and GPU): the model with the fixture's
parameters on the first 250 rows, and what tests/kg_reference.py needs of it on the host — latent features, per-source noise, prior
means, scaled targets — taken from the model's own modules (no device work: the feature map and the means are small torch modules)."""
import os

import numpy as np
import torch

import kg_reference as kg
from alc_reference import Fit

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_c4():
    return dict(np.load(os.path.join(GOLD, "c4_wing_mf_n300.npz")))


def build_c4(device, n=250, negate=False):
    """tests/test_gpu_condition.py's builder: three sources with a noise and a mean each."""
    from gpplus_amd.models import GP_Plus

    fx = load_c4()
    y = torch.tensor(fx["ytrain"][:n])
    m = GP_Plus(torch.tensor(fx["Xtrain"][:n]), -y if negate else y, dtype=torch.float64, device=device, qual_dict={10: 3},
                multiple_noise=True, m_gp="multiple_constant")
    sd = m.state_dict()
    for k in list(sd):
        fk = f"theta1::param::{k}"
        if fk in fx:
            sd[k] = torch.as_tensor(fx[fk]).reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    other = torch.tensor(fx["Xtrain"][n:])
    return m, other, other[other[:, 10] == 0]


def noise_rows(m, X):
    """The noise level of each row's own source, from the likelihood's parameters."""
    lik = m.likelihood
    noise = lik.noise_covar.noise.detach().reshape(-1).cpu().numpy().astype(np.float64)
    if noise.size == 1:
        return np.full(X.shape[0], noise[0])
    src = X[:, -1].cpu().numpy()
    out = np.zeros(X.shape[0])
    for k, lvl in enumerate(lik.noise_indices):
        out[src == lvl] = noise[k]
    return out


def operands(m, Xc, Xr, jitter=0.0):
    """(fit, resid, Uc, noise_c, Ur, prior_r, sf2, |y_std|) for kg_reference, in the model's scaled units."""
    from gpplus_amd.gpcore.module import Module

    X = m.train_inputs[0]
    dev = X.device
    m.eval()
    with torch.no_grad():
        U, Uc_, Ur_ = [m._features(Z.to(dev))[0].detach().cpu().numpy().astype(np.float64) for Z in (X, Xc, Xr)]
        spec = m.covar_module(m._features(X)[0]).spec
        prior, prior_r = [Module.__call__(m, Z.to(dev)).mean.detach().cpu().numpy().astype(np.float64) for Z in (X, Xr)]
    fit = Fit(U, noise_rows(m, X) + jitter, spec.w.detach().cpu().numpy().astype(np.float64), float(spec.sf2), int(spec.kind),
              int(spec.d_split))
    resid = m.train_targets.detach().cpu().numpy().astype(np.float64) - prior
    return dict(fit=fit, resid=resid, Uc=Uc_, noise_c=noise_rows(m, Xc) + jitter, Ur=Ur_, prior_r=prior_r), float(spec.sf2), \
        abs(float(m.y_std))


def dense_of(ops):
    return kg.dense(ops["fit"], ops["resid"], ops["Uc"], ops["noise_c"], ops["Ur"], ops["prior_r"])

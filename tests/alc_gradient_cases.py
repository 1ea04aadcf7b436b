"""The model-level cases tests/test_alc_gradient_host.py (their floors, on CPU models) and tests/test_gpu_alc_gradient.py (the scores, on
the GPU) share: the models c1 / c3 / c4 as tests/test_gpu_alc.py builds them and c1-matern52 / c1-matern32 (200 rows) from
``gek_reference.GEK_CASES``, each with candidates, reference rows and what tests/alc_gradient_reference.py needs on the host."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alc_gradient_reference as AG  # noqa: E402
import gek_reference as G  # noqa: E402
import test_gpu_alc as TA  # noqa: E402  (its builders and host operands; nothing of it runs on import)

NAMES = ("c1", "c3", "c4", "c1-matern52", "c1-matern32")
#: the gradient noise of a case, as a fraction of the prior curvature of each direction: 1e-4 unless the floor the host test prints
#: (|fp64 closed form - long double| / sf2) exceeds 1e-11 there, then raised in decade steps until it does not.  None needed it.
NOISE_REL = {name: 1e-4 for name in NAMES}
#: candidates per case: c3 / c4 take every other / every fifth of test_gpu_alc.py's (all three sources of c4 stay among them)
_STRIDE = {"c1": 1, "c3": 2, "c4": 5}
_oracles = {}


def half_mask(p):
    """About half the directions: every other quantitative column, the first included."""
    return torch.arange(p) % 2 == 0


def oracle_case(name):
    if name not in _oracles:
        _oracles[name] = G.gek_case(name)
    return _oracles[name]


def model_from_oracle(name, device):
    from gpplus_amd.models import GP_Plus

    o, X, y, kw = oracle_case(name)[:4]
    m = GP_Plus(torch.tensor(X), torch.tensor(y), dtype=torch.float64, device=device, **kw)
    sd = m.state_dict()
    for k, v in o.params.items():
        sd[k] = v.reshape(sd[k].shape).to(sd[k])
    m.load_state_dict(sd)
    return m


def build(name, device):
    """(model on ``device``, candidates, reference rows)."""
    if name in TA.CASES:
        m, Xc, Xr = TA.CASES[name](device)
        return m, Xc[::_STRIDE[name]].clone(), Xr
    xt = oracle_case(name)[7]
    return model_from_oracle(name, device), xt[8:14].clone(), xt[12:].clone()


def host_inputs(name, m, Xc, Xr, jitter=0.0):
    """(operands of the reference as tests/test_gpu_alc.py forms them, y_std^2, p, d0, kappa): kappa the prior curvature of the p
    quantitative directions in the model's scaled units (c_d w_d sf2: 2 on the RBF factor, 6 / (10 / 3) on a Matern factor)."""
    ops, scale = TA._operands(m, Xc, Xr, raw=(name == "c1"), jitter=jitter)
    p = int(m.quant_index.numel())
    D = ops["U"].shape[1]
    d0 = D - p
    split = D if ops["kind"] == 0 else ops["d_split"]
    coef = np.where(np.arange(D) < split, 2.0, 6.0 if ops["kind"] == 1 else 10.0 / 3.0)
    kappa = (coef * ops["w"] * ops["sf2"])[d0:]
    return ops, scale, p, d0, kappa


def reference_model(ops, Ug=None, gdirs=None, gnoise=None):
    return AG.Model(ops["U"], ops["noise"], ops["w"], ops["sf2"], ops["kind"], ops["d_split"], Ug, gdirs, gnoise)


def run_noise(name, kappa, mask, Mc, jitter=0.0):
    """(dirs relative to d0, gnoise (M_c x p') in scaled units with the factorisation's jitter) of a case under ``mask``."""
    rel = np.nonzero(np.asarray(mask))[0]
    return rel, np.tile(NOISE_REL[name] * kappa[rel] + jitter, (Mc, 1))

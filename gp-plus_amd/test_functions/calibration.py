"""A two-source analytic calibration problem (no reference counterpart: written for this build).

A simulator f(x, theta) = sin(3 x + theta) + theta x / 2 on x in [0, 1] takes a parameter theta the experiment does not expose.
  source 0 (high fidelity, the "experiment"):  y = f(x, THETA_STAR)             theta unknown: NaN in the data
  source 1 (low fidelity, the "simulator"):    y = f(x, theta) + BIAS           on a space-filling design over (x, theta)
The phase shift makes theta identifiable from a handful of experiments; the constant bias is what a per-source mean
(``m_gp='multiple_constant'``) or the latent map absorbs.  Columns of X: [x, theta, source]; fit with

    GP_Plus(X, y, qual_dict={2: 2}, calibration_id=[1], ...)

and read the estimate with ``model.calibration_result()``."""
import numpy as np
from scipy.stats.qmc import Sobol

THETA_STAR = 0.8
BIAS = 0.15
THETA_RANGE = (-1.0, 2.0)


def simulator(x, theta):
    x, theta = np.asarray(x, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    return np.sin(3.0 * x + theta) + 0.5 * theta * x


def calibration_problem(n_high=16, n_low=64, theta_star=THETA_STAR, bias=BIAS, noise_std=0.0, seed=0):
    """(X, y): ``n_high`` rows of source 0 (theta column NaN) followed by ``n_low`` rows of source 1, Sobol designs from ``seed``."""
    rng = np.random.default_rng(seed)
    xh = Sobol(d=1, seed=seed).random(n_high)[:, 0]
    lo = Sobol(d=2, seed=seed + 1).random(n_low)
    xl, tl = lo[:, 0], THETA_RANGE[0] + (THETA_RANGE[1] - THETA_RANGE[0]) * lo[:, 1]
    X = np.vstack([np.column_stack([xh, np.full(n_high, np.nan), np.zeros(n_high)]),
                   np.column_stack([xl, tl, np.ones(n_low)])])
    y = np.concatenate([simulator(xh, theta_star), simulator(xl, tl) + bias])
    if noise_std > 0.0:
        y = y + noise_std * rng.standard_normal(y.shape)
    return X, y


def calibration_test_rows(n=20, theta=THETA_STAR, seed=7):
    """Test rows of both sources on a grid of x: source 0 with any theta (the model writes its own estimate there) and source 1
    at ``theta``, with the responses of both."""
    x = np.linspace(0.02, 0.98, n)
    X = np.vstack([np.column_stack([x, np.zeros(n), np.zeros(n)]), np.column_stack([x, np.full(n, theta), np.ones(n)])])
    y = np.concatenate([simulator(x, THETA_STAR), simulator(x, theta) + BIAS])
    return X, y

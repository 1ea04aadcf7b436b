"""Dense CPU reference of the pathwise posterior draws (``gpplus_amd.pathwise``) and of the two generated-matrix products behind
them (``gpp_kernel_apply`` / ``gpp_rff_apply`` in ``include/gpp.h``).

  ``kernel_matrix`` / ``rff_matrix``   the generated matrices G in ``np.longdouble`` (or any numpy float type);
  ``kernel_gen_error`` / ``rff_gen_error``   first-order bounds on |G_computed - G| of the fp64 generators, elementwise;
  ``apply_bound``      the elementwise bound a product beta Out0 + G C computed in fp64 must meet;
  ``spectral_draw``    frequencies and phases from the kernel's spectral measure, by numpy's generator (independent of the
                       library's ``draw_spectral``);
  ``PathReference``    Ky = K + T by ``torch.linalg.cholesky`` and solves: coefficients, paths f_s from given (omega, b, theta, eps),
                       the exact posterior moments and the RFF-exact path variance.

The kernel is the library's: k(u, u') = sf2 exp(-sum_{d < split} w_d delta_d^2) h(r), r = sqrt(2 nu 2 sum_{d >= split} w_d delta_d^2),
h = 1 (RBF kind, split = D), (1 + r) e^-r (Matern 3/2, nu = 3/2) or (1 + r + r^2 / 3) e^-r (Matern 5/2).
Nothing here touches a GPU or the library.
"""
import math

import numpy as np
import torch

KIND_RBF, KIND_MATERN32, KIND_MATERN52 = 0, 1, 2
U53 = 2.0 ** -53  # unit roundoff of fp64
#: absolute error the device cosine states for cos(2 pi r), |r| <= 1/2 (csrc/gpp_apply.hip), and the relative error of the
#: exponential (2 ulp)
COS_ABS_ERR = 4 * U53
EXP_REL_ERR = 4 * U53


def _split(D, kind, d_split):
    return D if kind == KIND_RBF else d_split


def _r2(Ua, Ub, w, lo, hi, ld):
    r2 = np.zeros((Ua.shape[0], Ub.shape[0]), dtype=ld)
    for d in range(lo, hi):
        diff = Ua[:, d, None].astype(ld) - Ub[None, :, d].astype(ld)
        r2 += ld(w[d]) * diff * diff
    return r2


def _matern(r2m, kind, ld):
    """(h, |h'| bound helper r) of the Matern factor from r2m = sum_{d >= split} w_d delta_d^2."""
    two_nu = 3 if kind == KIND_MATERN32 else 5
    r = np.sqrt(ld(2 * two_nu) * r2m)
    poly = 1 + r if kind == KIND_MATERN32 else 1 + r + r * r / 3
    return poly * np.exp(-r), r


def kernel_matrix(Ua, Ub, w, sf2, kind=KIND_RBF, d_split=0, ld=np.longdouble):
    """G[a, j] = sf2 k(Ua_a, Ub_j; w), computed in ``ld``."""
    D = Ua.shape[1]
    s = _split(D, kind, d_split)
    G = ld(sf2) * np.exp(-_r2(Ua, Ub, w, 0, s, ld))
    if kind != KIND_RBF:
        G = G * _matern(_r2(Ua, Ub, w, s, D, ld), kind, ld)[0]
    return G


def rff_matrix(Ua, omega, phase, sf2, ld=np.longdouble):
    """G[a, f] = sqrt(2 sf2 / F) cos(omega_f . Ua_a + phase_f), computed in ``ld``."""
    F = omega.shape[0]
    arg = Ua.astype(ld) @ omega.astype(ld).T + phase.astype(ld)[None, :]
    return np.sqrt(ld(2) * ld(sf2) / ld(F)) * np.cos(arg)


def _dr2(Ua, Ub, w, lo, hi, ld):
    """Bound on the error of the fp64 sum r2 = sum_d (a_d - b_d)^2 over dims [lo, hi), a_d = fl(u_d fl(sqrt(w_d))): each staged value
    carries 3 u relative (square root 2 u, product u), the difference another u, so |delta df_d| <= 3 u (|a_d| + |b_d|) + u |df_d|;
    the sum of n fused multiply-adds adds (n + 1) u r2.  First order in u."""
    n = hi - lo
    e = np.zeros((Ua.shape[0], Ub.shape[0]), dtype=ld)
    for d in range(lo, hi):
        sw = np.sqrt(ld(w[d]))
        a, b = np.abs(Ua[:, d, None].astype(ld)) * sw, np.abs(Ub[None, :, d].astype(ld)) * sw
        df = np.abs(Ua[:, d, None].astype(ld) - Ub[None, :, d].astype(ld)) * sw
        e += 2 * df * (3 * U53 * (a + b) + U53 * df)
    return e + (n + 1) * U53 * _r2(Ua, Ub, w, lo, hi, ld)


def kernel_gen_error(Ua, Ub, w, sf2, kind=KIND_RBF, d_split=0, ld=np.longdouble):
    """|G_computed - G| <= G (dr2_rbf + EXP_REL_ERR + 3 u) + sf2 e1 dh, with e1 the RBF factor and, for the Matern kinds,
    dh <= 0.4 dr + 12 u h: |h'| <= 0.37 for both kinds, the polynomial, the second exponential and the products cost at most 12 u of
    h, and dr = sqrt(2 nu 2) min(sqrt(dr2_mat), dr2_mat / (2 sqrt(r2_mat))) + 4 u r is the error of r = sqrt(c r2_mat) (the square
    root of a perturbed argument, then its own roundings)."""
    D = Ua.shape[1]
    s = _split(D, kind, d_split)
    e1 = np.exp(-_r2(Ua, Ub, w, 0, s, ld))
    rel = _dr2(Ua, Ub, w, 0, s, ld) + EXP_REL_ERR + 3 * U53
    if kind == KIND_RBF:
        return ld(sf2) * e1 * rel
    r2m = _r2(Ua, Ub, w, s, D, ld)
    h, r = _matern(r2m, kind, ld)
    dr2 = _dr2(Ua, Ub, w, s, D, ld)
    c = ld(2 * (3 if kind == KIND_MATERN32 else 5))
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(r2m > 0, dr2 / (2 * np.sqrt(r2m)), np.inf)
    dr = np.sqrt(c) * np.minimum(np.sqrt(dr2), lin) + 4 * U53 * r
    dh = 0.4 * dr + 12 * U53 * h
    return ld(sf2) * e1 * (h * rel + dh)


def rff_gen_error(Ua, omega, phase, sf2, ld=np.longdouble):
    """The phase is summed in turns, t = sum_d fl(omega_d / 2 pi) u_d + fl(b / 2 pi): each term carries 2 u from its factor 1 / 2 pi
    (the constant's rounding and the product's) and the D fused multiply-adds add (D + 1) u of the partial sums, all bounded by
    T = (sum_d |omega_d u_d| + |b|) / 2 pi: dt <= (D + 3) u T.  r = t - rint(t) is exact; the cosine then errs by 2 pi dt plus the
    polynomial's COS_ABS_ERR, and the amplitude sqrt(2 sf2 / F) and the final product cost 4 u of |G|."""
    D, F = Ua.shape[1], omega.shape[0]
    T = (np.abs(Ua).astype(ld) @ np.abs(omega).astype(ld).T + np.abs(phase).astype(ld)[None, :]) / (2 * ld(math.pi))
    amp = np.sqrt(ld(2) * ld(sf2) / ld(F))
    return amp * (2 * ld(math.pi) * (D + 3) * U53 * T + COS_ABS_ERR) + 4 * U53 * np.abs(rff_matrix(Ua, omega, phase, sf2, ld))


def apply_bound(G, dG, C, beta, Out0, ld=np.longdouble):
    """(K + 4) u (|G| @ |C| + |beta| |Out0|) + dG @ |C|: the dot-product bound of ``gemm_reference.error_bound`` for any summation
    order of the K terms (the pieces of a split contraction included) plus the first-order effect of the generator's error."""
    K = G.shape[1]
    absC = np.abs(C).astype(ld)
    return (K + 4) * ld(U53) * (np.abs(G) @ absC + abs(ld(beta)) * np.abs(Out0).astype(ld)) + dG @ absC


# ---- spectral measure ------------------------------------------------------------------------------------------------------------
def spectral_draw(w, kind, d_split, F, rng):
    """(omega F x D, phase F) by ``rng`` (a numpy Generator): N(0, 2 w_d) on the RBF dims, the multivariate Student-t with 2 nu
    degrees of freedom (one chi^2_{2 nu} per feature) on the Matern dims, phases uniform on [0, 2 pi)."""
    w = np.asarray(w, dtype=np.float64)
    D = w.shape[0]
    omega = rng.standard_normal((F, D)) * np.sqrt(2.0 * w)
    if kind != KIND_RBF:
        two_nu = 3 if kind == KIND_MATERN32 else 5
        g = rng.chisquare(two_nu, F)
        omega[:, d_split:] *= np.sqrt(two_nu / g)[:, None]
    return omega, rng.uniform(0.0, 2.0 * math.pi, F)


# ---- dense paths -------------------------------------------------------------------------------------------------------------------
def _t(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64)) if not torch.is_tensor(x) else x.detach().to("cpu", torch.float64)


class PathReference:
    """Dense fp64 algebra of the paths for training features U (N x D), residual y - m(X) (N), noise diag(T) (N) and the kernel
    (w, sf2, kind, d_split).  All inputs numpy arrays or tensors; everything is computed with torch on the CPU."""

    def __init__(self, U, resid, noise, w, sf2, kind=KIND_RBF, d_split=0):
        self.U, self.resid, self.noise, self.w = _t(U), _t(resid).reshape(-1), _t(noise).reshape(-1), _t(w).reshape(-1)
        self.sf2, self.kind, self.d_split = float(sf2), int(kind), int(d_split)
        self.K = self.kernel(self.U, self.U)
        self.L = torch.linalg.cholesky(self.K + torch.diag(self.noise))

    def kernel(self, Ua, Ub):
        G = kernel_matrix(_t(Ua).numpy(), _t(Ub).numpy(), self.w.numpy(), self.sf2, self.kind, self.d_split, ld=np.float64)
        return torch.from_numpy(G)

    def features(self, Ua, omega, phase):
        """Phi (M x F)."""
        omega, phase = _t(omega), _t(phase)
        return math.sqrt(2.0 * self.sf2 / omega.shape[0]) * torch.cos(_t(Ua) @ omega.T + phase)

    def solve(self, B):
        return torch.cholesky_solve(B, self.L)

    def coef(self, omega, phase, theta, eps):
        """c = Ky^-1 (y - m(X) - Phi_X theta - eps), N x S."""
        return self.solve(self.resid[:, None] - self.features(self.U, omega, phase) @ _t(theta) - _t(eps))

    def paths(self, Ua, mean_a, omega, phase, theta, eps, coef=None):
        """f_s at features Ua with prior mean mean_a: S x M."""
        c = self.coef(omega, phase, theta, eps) if coef is None else _t(coef)
        f = _t(mean_a).reshape(-1, 1) + self.features(Ua, omega, phase) @ _t(theta) + self.kernel(Ua, self.U) @ c
        return f.T

    def train_identity(self, eps, coef):
        """f_s(X) - m(X) = y - m(X) - eps_s - T c_s, exactly (K = Ky - T): S x N."""
        return (self.resid[:, None] - _t(eps) - self.noise[:, None] * _t(coef)).T

    def posterior(self, Ua, mean_a):
        """Exact posterior mean and variance of the latent f at Ua."""
        ks = self.kernel(Ua, self.U)
        mean = _t(mean_a).reshape(-1) + ks @ self.solve(self.resid[:, None]).reshape(-1)
        V = torch.linalg.solve_triangular(self.L, ks.T, upper=False)
        return mean, self.sf2 - (V * V).sum(0)

    def rff_variance(self, Ua, omega, phase):
        """Variance of f_s(x) over (theta, eps) for FIXED (omega, b): khat** - 2 k*^T Ky^-1 khat_* + k*^T Ky^-1 (Khat + T) Ky^-1 k*,
        khat = Phi Phi^T."""
        Ps, Px = self.features(Ua, omega, phase), self.features(self.U, omega, phase)
        A = self.solve(self.kernel(Ua, self.U).T)  # Ky^-1 k*, N x M
        PxA = Px.T @ A                              # F x M
        return (Ps * Ps).sum(1) - 2.0 * (Ps.T * PxA).sum(0) + (PxA * PxA).sum(0) + (self.noise[:, None] * A * A).sum(0)

    def draw(self, S, F, rng):
        """The reference's own (omega, phase, theta, eps)."""
        omega, phase = spectral_draw(self.w.numpy(), self.kind, self.d_split, F, rng)
        theta = rng.standard_normal((F, S))
        eps = rng.standard_normal((self.U.shape[0], S)) * np.sqrt(self.noise.numpy())[:, None]
        return omega, phase, theta, eps


def c1_problem():
    """The inputs of the model-level test without a GPU: the c1 fixture at its fitted parameters through the CPU oracle — training
    features, residual, noise, kernel, and the first 64 held-out points with their prior mean."""
    import os

    from oracle.gp_oracle import OracleGP, softplus

    fx = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "c1_borehole_n500.npz")))
    o = OracleGP(fx["Xtrain"], fx["ytrain"])
    for k in list(o.params):
        o.params[k] = torch.as_tensor(fx[f"theta1::param::{k}"], dtype=torch.float64).reshape(o.params[k].shape)
    xt = torch.as_tensor(fx["Xtest"][:64], dtype=torch.float64)
    U, Ut = o.features(o.train_x), o.features(xt)
    # the quantitative kernel as the oracle evaluates it: exp(-0.5 sum_d (delta_d / l_d)^2), i.e. w_d = 1 / (2 l_d^2)
    w = 0.5 / o.lengthscale().reshape(-1) ** 2
    sf2 = float(softplus(o.params["covar_module.raw_outputscale"]))
    ref = PathReference(U, o.y_sc - o.mean(o.train_x), o.noise_vector(o.train_x), w, sf2)
    return dict(ref=ref, oracle=o, Ut=Ut, mean_t=o.mean(xt), xt=xt, w=w, sf2=sf2)

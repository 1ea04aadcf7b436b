"""Dense CPU reference of the gradients of the two generated-matrix products (``gpp_kernel_apply_grad`` / ``gpp_rff_apply_grad`` in
``include/gpp.h``) with respect to Ua, on top of ``tests/pathwise_reference.py``:

    g[a, d] = beta g0[a, d] + sum_j V[a, j] dG[a, j] / dUa[a, d],        V = Gbar C^T

  ``kernel_multipliers`` / ``rff_multiplier``   the factors m with dG/dua_d = 2 w_d (ua_d - ub_jd) m_f (kernel; f = 0 on the RBF dims,
                       1 on the Matern dims) and dG/dua_d = m omega_fd (random features), in ``np.longdouble``;
  ``kernel_dgen`` / ``rff_dgen``   dG/dUa[:, d] itself (M x L), for the finite-difference checks;
  ``grad_reference``   (ref, bound): the gradient in long double and the elementwise bound an fp64 evaluation must meet;
  ``dense_path_values``   g_s + k c_s at feature rows, dense and differentiable in torch fp64 (the autograd references);
  ``inputs`` / ``cases``   the inputs and the case list of tests/test_gpu_apply_grad.py, shared with the host test that holds the
                       bound to 1e-9 of the reference on every one of them.

The bound (first order in u = 2^-53, in the style of ``pathwise_reference.apply_bound``).  The gradient is evaluated as
g_d = s_d (a_d sum_j W_j - sum_j W_j b_jd) with the staged a = fl(sqrt(w) ua), b = fl(sqrt(w) ub), s_d = 2 fl(sqrt(w_d)) and
W_j = fl(V_j m_j), V_j a dot product of length S, the two sums over j dot products of length L.  With Vabs = |Gbar| |C|^T and
T_d = sum_j |W_j| (|a_d| + |b_jd|) — the magnitudes |a_d| + |b_jd|, not |a_d - b_jd|: the row-sum form cancels —

    |g_d - ref_d| <= s_d [ (L + 16 + pieces) u T_d + sum_j dW_j (|a_d| + |b_jd|) ] + u |beta g0_d|
    dW_j = |m_j| (S + 4) u Vabs_j + |V_j| dm_j + u |V_j m_j|

(L + 16 + pieces) u: the two dot products in any order, pieces of a split contraction included (L + 4), the staged values (3 u), the
fused multiply-add of the epilogue (u), s_d and its product (3 u), the accumulation into beta g0 (u), the finish kernel's additions
(pieces u) and slack.  dm_j extends the generator errors of ``kernel_gen_error`` / ``rff_gen_error`` to the multipliers:

  m_0 = -G:            dm_0 = kernel_gen_error (the same operations in another order)
  m_1 = sf2 e1 h':     dm_1 = sf2 e1 (|h'| (dr2_rbf + EXP_REL_ERR + 3 u) + c' dr + 12 u |h'|),  c' = sup |dh'/dr| = 3 (Matern 3/2,
                       h' = -3 e^-r) or 0.62 (Matern 5/2, h' = -(5/3)(1 + r) e^-r, |dh'/dr| = (5/3) r e^-r <= 5 / (3 e)), dr as in
                       kernel_gen_error
  features:            m = -amp sin(arg) evaluated as -(amp 2 pi) sin(2 pi r) against frequencies staged as omega / 2 pi:
                       dm = amp (2 pi (D + 3) u T + SIN_ABS_ERR) + 8 u |m|, SIN_ABS_ERR = COS_ABS_ERR + 2 pi 2^-56 (the quarter-turn
                       shift |r| - 1/4 is exact from |r| = 1/8 on and errs by at most 2^-56 turns below); |a_d| + |b_jd| becomes
                       |omega_jd| and s_d = 1.

A feature with w_d = 0 has a_d = b_jd = s_d = 0: reference and bound are exactly 0.  Nothing here touches a GPU or the library."""
import math
import zlib

import numpy as np

import pathwise_reference as R

LD = np.longdouble
U53 = R.U53
SIN_ABS_ERR = R.COS_ABS_ERR + 2 * math.pi * 2.0 ** -56
SPLIT = 2048  # longest contraction without pieces (backend.APPLY_SPLIT)


def _matern_parts(r2m, kind, ld):
    """(h, h', r) of the Matern factor from r2m = sum_{d >= split} w_d delta_d^2; h' = (dh/dr2m) / 2 ... i.e. dh/dua_d = 2 w_d delta_d h'."""
    two_nu = 3 if kind == R.KIND_MATERN32 else 5
    r = np.sqrt(ld(2 * two_nu) * r2m)
    er = np.exp(-r)
    if kind == R.KIND_MATERN32:
        return (1 + r) * er, -ld(3) * er, r
    return (1 + r + r * r / 3) * er, -(ld(5) / ld(3)) * (1 + r) * er, r


def kernel_multipliers(Ua, Ub, w, sf2, kind=R.KIND_RBF, d_split=0, ld=LD):
    """[m_0] (RBF kind) or [m_0, m_1]: M x L each.  h' is formed without a division by r: finite at r = 0."""
    D = Ua.shape[1]
    s = R._split(D, kind, d_split)
    e1 = ld(sf2) * np.exp(-R._r2(Ua, Ub, w, 0, s, ld))
    if kind == R.KIND_RBF:
        return [-e1]
    h, hp, _ = _matern_parts(R._r2(Ua, Ub, w, s, D, ld), kind, ld)
    return [-e1 * h, e1 * hp]


def _factor(d, D, kind, d_split):
    return 0 if d < R._split(D, kind, d_split) else 1


def kernel_dgen(Ua, Ub, w, sf2, kind, d_split, d, ld=LD):
    """dG[a, j] / dUa[a, d]."""
    m = kernel_multipliers(Ua, Ub, w, sf2, kind, d_split, ld)[_factor(d, Ua.shape[1], kind, d_split)]
    return 2 * ld(w[d]) * (Ua[:, d, None].astype(ld) - Ub[None, :, d].astype(ld)) * m


def rff_multiplier(Ua, omega, phase, sf2, ld=LD):
    F = omega.shape[0]
    arg = Ua.astype(ld) @ omega.astype(ld).T + phase.astype(ld)[None, :]
    return -np.sqrt(ld(2) * ld(sf2) / ld(F)) * np.sin(arg)


def rff_dgen(Ua, omega, phase, sf2, d, ld=LD):
    return rff_multiplier(Ua, omega, phase, sf2, ld) * omega[None, :, d].astype(ld)


def kernel_multiplier_errors(Ua, Ub, w, sf2, kind=R.KIND_RBF, d_split=0, ld=LD):
    """dm_f for the multipliers of ``kernel_multipliers`` (module docstring)."""
    D = Ua.shape[1]
    dm0 = R.kernel_gen_error(Ua, Ub, w, sf2, kind, d_split, ld)
    if kind == R.KIND_RBF:
        return [dm0]
    s = R._split(D, kind, d_split)
    e1 = np.exp(-R._r2(Ua, Ub, w, 0, s, ld))
    rel = R._dr2(Ua, Ub, w, 0, s, ld) + R.EXP_REL_ERR + 3 * U53
    r2m = R._r2(Ua, Ub, w, s, D, ld)
    _, hp, r = _matern_parts(r2m, kind, ld)
    dr2 = R._dr2(Ua, Ub, w, s, D, ld)
    c = ld(2 * (3 if kind == R.KIND_MATERN32 else 5))
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(r2m > 0, dr2 / (2 * np.sqrt(r2m)), np.inf)
    dr = np.sqrt(c) * np.minimum(np.sqrt(dr2), lin) + 4 * U53 * r
    slope = 3.0 if kind == R.KIND_MATERN32 else 0.62
    return [dm0, ld(sf2) * e1 * (np.abs(hp) * rel + slope * dr + 12 * U53 * np.abs(hp))]


def rff_multiplier_error(Ua, omega, phase, sf2, ld=LD):
    D, F = Ua.shape[1], omega.shape[0]
    T = (np.abs(Ua).astype(ld) @ np.abs(omega).astype(ld).T + np.abs(phase).astype(ld)[None, :]) / (2 * ld(math.pi))
    amp = np.sqrt(ld(2) * ld(sf2) / ld(F))
    return amp * (2 * ld(math.pi) * (D + 3) * U53 * T + SIN_ABS_ERR) + 8 * U53 * np.abs(rff_multiplier(Ua, omega, phase, sf2, ld))


def grad_reference(gen, p, beta, ld=LD):
    """(ref, bound), M x D each, for the inputs ``p`` of :func:`inputs`."""
    Ua, second, C, Gbar, g0 = p["Ua"], p["second"], p["C"], p["Gbar"], p["g0"]
    M, D = Ua.shape
    L, S = C.shape
    pieces = -(-L // SPLIT)
    V = Gbar.astype(ld) @ C.astype(ld).T
    Vabs = np.abs(Gbar).astype(ld) @ np.abs(C).astype(ld).T
    if gen == "rff":
        ms = [rff_multiplier(Ua, second, p["phase"], p["sf2"], ld)]
        dms = [rff_multiplier_error(Ua, second, p["phase"], p["sf2"], ld)]
    else:
        ms = kernel_multipliers(Ua, second, p["w"], p["sf2"], p["kind"], p["d_split"], ld)
        dms = kernel_multiplier_errors(Ua, second, p["w"], p["sf2"], p["kind"], p["d_split"], ld)
    W = [V * m for m in ms]
    dW = [np.abs(m) * (S + 4) * U53 * Vabs + np.abs(V) * dm + U53 * np.abs(V * m) for m, dm in zip(ms, dms)]
    ref = np.zeros((M, D), dtype=ld)
    bound = np.zeros((M, D), dtype=ld)
    for d in range(D):
        if gen == "rff":
            om = second[None, :, d].astype(ld)
            ref[:, d] = (W[0] * om).sum(1)
            mag, s_d, f = np.abs(om), ld(1), 0
        else:
            f = _factor(d, D, p["kind"], p["d_split"])
            wd = ld(p["w"][d])
            ref[:, d] = 2 * wd * (W[f] * (Ua[:, d, None].astype(ld) - second[None, :, d].astype(ld))).sum(1)
            sw = np.sqrt(wd)
            mag, s_d = sw * (np.abs(Ua[:, d, None]).astype(ld) + np.abs(second[None, :, d]).astype(ld)), 2 * sw
        T = (np.abs(W[f]) * mag).sum(1)
        bound[:, d] = s_d * ((L + 16 + pieces) * U53 * T + (dW[f] * mag).sum(1))
    b = ld(beta)
    return b * g0.astype(ld) + ref, bound + U53 * np.abs(b * g0.astype(ld))


def dense_path_values(Us, U, w, sf2, kind, d_split, omega, phase, theta, coef):
    """Phi(Us) theta + sf2 k(Us, U; w) coef (M x S) from dense matrices in torch fp64 on the CPU, differentiable in ``Us`` by autograd.
    Where a row of Us equals a row of U the Matern factor is entered as the constant h(0) = 1, so the square root is not
    differentiated at 0; the pair's true contribution to the gradient, h'(0) * 2 w_d (ua_d - ub_d), is 0 as well."""
    import torch

    D = Us.shape[1]
    s = D if kind == R.KIND_RBF else d_split
    d2 = (Us[:, None, :] - U[None, :, :]) ** 2 * w
    K = sf2 * torch.exp(-d2[..., :s].sum(-1))
    if kind != R.KIND_RBF:
        q = (6.0 if kind == R.KIND_MATERN32 else 10.0) * d2[..., s:].sum(-1)
        r = torch.sqrt(torch.where(q > 0, q, torch.ones_like(q)))
        h = ((1 + r) if kind == R.KIND_MATERN32 else (1 + r + r * r / 3)) * torch.exp(-r)
        K = K * torch.where(q > 0, h, torch.ones_like(h))
    Phi = math.sqrt(2.0 * sf2 / omega.shape[0]) * torch.cos(Us @ omega.T + phase)
    return Phi @ theta + K @ coef


# ---- the cases of tests/test_gpu_apply_grad.py ---------------------------------------------------------------------------------------
BASE = dict(M=65, L=65, S=17, D=8)
GENS = {"rbf": ("kernel", 0), "m32": ("kernel", 1), "m52": ("kernel", 2), "rff": ("rff", 0)}


def inputs(gen, M, L, S, D, kind, seed, copies=False):
    """The recipe of tests/test_gpu_apply.py::_inputs, plus Gbar ~ N(0, 1) and a start value g0 of the gradient.  ``copies``: the rows
    of Ua are copies of rows of the second operand (kernel generators)."""
    rng = np.random.default_rng(seed)
    Ua = rng.uniform(-1.0, 1.0, (M, D))
    C = rng.standard_normal((L, S))
    Out0 = rng.standard_normal((M, S))  # (drawn to keep the recipe's stream; unused)
    sf2 = 1.3
    if gen == "rff":
        w = rng.uniform(0.2, 2.0, D)
        second = rng.standard_normal((L, D)) * np.sqrt(2.0 * w)  # frequencies
        phase = rng.uniform(0.0, 2.0 * np.pi, L)
        out = dict(Ua=Ua, second=second, phase=phase, sf2=sf2, C=C, w=None, kind=0, d_split=0)
    else:
        w = rng.uniform(0.2, 2.0, D) / D
        if D > 2:
            w[D // 2] = 0.0
        second = rng.uniform(-1.0, 1.0, (L, D))
        if copies:
            Ua = second[rng.integers(0, L, M)].copy()
        out = dict(Ua=Ua, second=second, phase=None, sf2=sf2, C=C, w=w, kind=kind, d_split=0 if kind == 0 else D // 2)
    del Out0
    out["Gbar"] = rng.standard_normal((M, S))
    out["g0"] = rng.standard_normal((M, D))
    return out


def cases():
    """[(id, name, M, L, S, D, beta, copies)]: both generators along every axis from the base case, one axis at a time; the Matern
    kinds along D (d_split = D // 2: inside a 16-column block, on a block boundary, the two row-sum columns in one block and in two)
    and with a split contraction; every edge at once; the smallest case; rows of Ua that are rows of Ub."""
    out = []

    def add(name, beta, copies=False, **kw):
        c = dict(BASE, **kw)
        cid = f"{name}-M{c['M']}-L{c['L']}-S{c['S']}-D{c['D']}-b{beta}" + ("-copies" if copies else "")
        out.append((cid, name, c["M"], c["L"], c["S"], c["D"], beta, copies))

    for name in ("rbf", "rff"):
        for beta in (0.0, 1.0):
            add(name, beta)
        for i, M in enumerate((1, 63, 64, 130)):
            add(name, float(i & 1), M=M)
        for i, L in enumerate((1, 15, 16, 17, 33, 200, SPLIT, SPLIT + 1, SPLIT + 2)):
            add(name, float(i & 1), L=L)
        for i, S in enumerate((1, 3, 4, 5, 16, 64, 65, 130)):
            add(name, float(i & 1), S=S)
        for i, D in enumerate((1, 15, 16, 17, 64)):
            add(name, float(i & 1), D=D)
        add(name, 1.0, M=130, L=SPLIT + 1, S=65, D=64)  # every edge at once, the largest LDS request
    for name in ("m32", "m52"):
        for beta in (0.0, 1.0):
            add(name, beta)
        for i, D in enumerate((1, 15, 16, 17, 64)):
            add(name, float(i & 1), D=D)
        add(name, 1.0, L=SPLIT + 1, M=130, S=65)
        add(name, 0.0, copies=True)
    add("m52", 1.0, M=130, L=SPLIT + 1, S=65, D=64)
    add("rbf", 0.0, copies=True)
    add("rbf", 0.0, M=1, L=1, S=1, D=1)
    add("rff", 0.0, M=1, L=1, S=1, D=1)
    return out


def case_inputs(name, M, L, S, D, copies):
    gen, kind = GENS[name]
    return gen, inputs(gen, M, L, S, D, kind, seed=zlib.crc32(f"grad-{name}-{M}-{L}-{S}-{D}-{int(copies)}".encode()), copies=copies)

"""CPU reference of the training-path reductions of ``csrc/gpp_reduce.hip``, in plain numpy with every sum in ``np.longdouble``:

  ``grad_sums`` / ``grad_bound``   the gradient reduction (gpp_grad_tiles and its finish kernels) and the error a fp64 evaluation of
                                   it may have, whatever its summation order; ``entries`` gives one rank's partial sums;
  ``trmv_lower``, ``trmv_upper``, ``mll_scalars``, ``predict_rows``   the vector reductions, each as (value, bound);
  ``Window`` & co.                 the operands as the kernels are handed them: interior windows of NaN- or sentinel-filled buffers;
  ``gradient_cases``               the seeded case list of tests/test_gpu_reduce_conformance.py (its coverage is asserted on the host).

All inputs are fp64 values that the kernel receives bit-identically.  Nothing here imports torch or touches a GPU.
"""
import collections

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a long double with at least 64 significant bits"

#: unit roundoff of fp64, and its smallest denormal step
U64 = LD(2.0) ** -53
ETA = LD(2.0) ** -1074
#: gpp_exp_nonpos: "max error 2 ulp on [-745, 0]" (gpp_internal.h); one ulp is at most 2 u relative
EXP_ULP = 2
EXP_REL = EXP_ULP * 2 * U64
#: log of the device library: its documentation is not shipped with the toolchain, so no ulp figure is stated: 2 ulp are assumed
LOG_ULP = 2
LOG_REL = LOG_ULP * 2 * U64
#: roundings of one r^2 term beyond its place in the fma chain: the difference u_i - u_j (it enters squared: 2), the product w d
#: (1), and one more where the chain is a multiply and an add instead of an fma (1)
R2_EXTRA = 4
#: roundings of W: alpha_i beta_j, beta_i alpha_j, their sum, the difference with C_ij (the plain weights have two fewer)
W_ROUNDINGS = 4
#: the handful of multiplications behind the kernel value, on the longest path (g_w): W_ROUNDINGS, then W sf2 and (W sf2) k (2), the
#: difference of the features twice (2), g d and (g d) d where the last is not fused into the sum (2)
CHAIN = W_ROUNDINGS + 6
#: operations of a term that may round in the denormal range: the two ldexp of the exponentials and two products behind them
DENORMAL_STEPS = 4
TILE = 64
SENTINEL = 7777.0
LOG_2PI = LD("1.8378770664093454835606594728112352797227949472755668")

GradSums = collections.namedtuple("GradSums", "g_w g_sf2 g_tau g_U")


def gamma(n):
    """n u / (1 - n u): the relative error of n successive roundings (Higham, Accuracy and Stability, lemma 3.1)."""
    n = np.asarray(n, dtype=LD)
    return n * U64 / (1 - n * U64)


def _both(a, b):
    """(1 + a)(1 + b) - 1 for two relative errors."""
    return a + b + a * b


def tile_col(first, b):
    """gpp_tile_col: column b = 0..3 of a thread whose first column is ``first``: the pairs {0, 1} and {32, 33}."""
    return first + (b & 1) + ((b >> 1) << 5)


# ---- the covariance factor -----------------------------------------------------------------------------------------------------
def kernel_factors(kind, r2_rbf, r2_mat, dt=LD):
    """kv = exp(-r2_rbf) h(r2_mat) and kd = -exp(-r2_rbf) dh/d r2_mat, h the Matern factor of gpp_internal.h in r = sqrt(2 nu r2_mat):
    kind 1: h = (1 + r) e^-r, dh = -3 e^-r; kind 2: h = (1 + r + r^2 / 3) e^-r, dh = -(5/3)(1 + r) e^-r; kind 0: kv = exp(-r2_rbf),
    kd = 0.  No division by r: finite where two points agree.  Also returns r and the polynomial factors (p, dp)."""
    r2_rbf, r2_mat = np.asarray(r2_rbf, dtype=dt), np.asarray(r2_mat, dtype=dt)
    er = np.exp(-r2_rbf)
    if kind == 0:
        one = np.ones_like(er)
        return er, np.zeros_like(er), np.zeros_like(er), one, np.zeros_like(er)
    r = np.sqrt(dt(6 if kind == 1 else 10) * r2_mat)
    mer = np.exp(-r)
    if kind == 1:
        p, dp = 1 + r, np.full_like(r, 3)
    else:
        p, dp = 1 + r + r * r * (dt(1) / dt(3)), (dt(5) / dt(3)) * (1 + r)
    return er * p * mer, er * dp * mer, r, p, dp


def _kernel_rel(kind, D, r2_abs, r, want_d):
    """Relative error of kv (and kd) of a fp64 evaluation; see ``grad_bound``."""
    g_r2 = gamma(D + R2_EXTRA)
    rel_er = _both(np.expm1(g_r2 * r2_abs), EXP_REL)
    if kind == 0:
        return rel_er, None
    rho = g_r2 / 2 + 2 * U64
    rel_mer = _both(np.expm1(rho * r), EXP_REL)
    rel_p = rho + U64 if kind == 1 else 2 * rho + 5 * U64
    rel_v = _both(_both(_both(rel_er, rel_p), rel_mer), gamma(2))
    if not want_d:
        return rel_v, None
    rel_dp = LD(0) if kind == 1 else rho + 2 * U64
    return rel_v, _both(_both(_both(rel_er, rel_dp), rel_mer), gamma(3))


def split_of(kind, d_split, D):
    """First Matern feature: kind 0 has none, whatever d_split says (the RBF instantiations never read it)."""
    return D if kind == 0 else int(d_split)


def unit_terms(U, w, sf2, kind, d_split, dU, i0, i1, dt=LD, want_rel=False):
    """The factors of W_ij in the terms of rows [i0, i1) against columns [0, i1), in ``dt``:
      kv[i, j]       of g_sf2;   uw[i, j, d] = -sf2 k' (u_id - u_jd)^2   of g_w[d];
      urow[i, j, d] = -2 w_d sf2 k' (u_id - u_jd)   of g_U[i, d] (its negative is the factor of g_U[j, d]),
    k' = kv for the RBF features (d < d_split, or kind 0) and kd for the Matern ones.  want_rel: also the relative errors of kv and kd
    and the maxima the denormal floor needs."""
    D = U.shape[1]
    dsp = split_of(kind, d_split, D)
    wd = np.asarray(w, dtype=dt)
    df = np.asarray(U[i0:i1], dtype=dt)[:, None, :] - np.asarray(U[:i1], dtype=dt)[None, :, :]
    df2 = df * df
    wdf2 = wd * df2
    r2, r2m = wdf2[..., :dsp].sum(-1), wdf2[..., dsp:].sum(-1)
    kv, kd, r, p, dp = kernel_factors(kind, r2, r2m, dt)
    s = dt(sf2)
    uw = np.empty_like(df2)
    uw[..., :dsp] = -(s * kv)[..., None] * df2[..., :dsp]
    uw[..., dsp:] = -(s * kd)[..., None] * df2[..., dsp:]
    urow = np.empty(df.shape[:2] + (dU,), dtype=dt)
    a = min(dU, dsp)
    urow[..., :a] = (-2 * s * kv)[..., None] * (wd[:a] * df[..., :a])
    urow[..., a:] = (-2 * s * kd)[..., None] * (wd[a:dU] * df[..., a:dU])
    out = {"kv": kv, "uw": uw, "urow": urow}
    if want_rel:
        assert dt is LD and np.all(wd >= 0), "the bound of sqrt(r2_mat) assumes weights that are not negative"
        if dsp < D:  # (the weights are not negative: sum |w| d^2 is r2 itself)
            rel_v, rel_d = _kernel_rel(kind, D, r2, r, True)
        else:
            rel_v, rel_d = _kernel_rel(0, D, r2, r, False)[0], None
            if kind != 0:  # a Matern kind without a Matern feature: r = 0, p = e^-r = 1, but the two products with them are still made
                rel_v = _both(rel_v, gamma(2))
        out.update(rel_v=rel_v, rel_d=rel_d, pmax=max(LD(1), p.max(initial=0), dp.max(initial=0)),
                   df2max=df2.max(initial=0), dfmax=np.abs(df).max(initial=0))
    return out


def weights(alpha, Kinv_lower, beta, i0, i1, dt=LD):
    """W and the sum of the magnitudes it is formed from, rows [i0, i1) against columns [0, i1); only Kinv[i][j], j <= i, is read
    (W is 0 above the diagonal)."""
    a = np.asarray(alpha, dtype=dt)
    i, j = np.arange(i0, i1)[:, None], np.arange(i1)[None, :]
    low = j <= i
    K = np.where(low, np.asarray(Kinv_lower)[i0:i1, :i1], 0).astype(dt)
    if beta is None:
        aa = a[i0:i1, None] * a[None, :i1]
        W, Wabs = dt(0.5) * (aa - K), dt(0.5) * (np.abs(aa) + np.abs(K))
    else:
        b = np.asarray(beta, dtype=dt)
        ab, ba = a[i0:i1, None] * b[None, :i1], b[i0:i1, None] * a[None, :i1]
        W, Wabs = dt(-0.5) * (ab + ba) - K, dt(0.5) * (np.abs(ab) + np.abs(ba)) + np.abs(K)
    return np.where(low, W, 0), np.where(low, Wabs, 0)


def multiplicity(N, i0, i1, entries=None):
    """2 for the kept entries below the diagonal (they stand for (i, j) and (j, i)), 1 for the kept diagonal ones, 0 elsewhere."""
    i, j = np.arange(i0, i1)[:, None], np.arange(i1)[None, :]
    m = np.where(j < i, 2, np.where(j == i, 1, 0))
    if entries is not None:
        m = np.where(np.asarray(entries, dtype=bool)[i0:i1, :i1], m, 0)
    return m


def _groups(grp, N):
    return np.zeros(N, dtype=np.int64) if grp is None else np.asarray(grp, dtype=np.int64)


def _grad_eval(U, w, sf2, grp, S, kind, d_split, alpha, Kinv_lower, dU, beta, entries, want_bound, rows):
    U = np.asarray(U, dtype=np.float64)
    N, D = U.shape
    dsp = split_of(kind, d_split, D)
    g = _groups(grp, N)
    val = GradSums(np.zeros(D, LD), np.zeros((), LD), np.zeros(S, LD), np.zeros((N, dU), LD))
    err = GradSums(np.zeros(D, LD), np.zeros((), LD), np.zeros(S, LD), np.zeros((N, dU), LD))  # sums of |term| x its relative error
    mag = GradSums(np.zeros(D, LD), np.zeros((), LD), np.zeros(S, LD), np.zeros((N, dU), LD))  # sums of |term|
    nterms, ntau = 0, np.zeros(S, dtype=np.int64)
    cmax = {"sf2": LD(0), "w": LD(0), "U": LD(0)}
    g_sf2 = e_sf2 = m_sf2 = LD(0)
    chain = gamma(CHAIN)
    for i0 in range(0, N, rows):
        i1 = min(N, i0 + rows)
        m = multiplicity(N, i0, i1, entries)
        if not m.any():
            continue
        ut = unit_terms(U, w, sf2, kind, d_split, dU, i0, i1, LD, want_bound)
        W, Wabs = weights(alpha, Kinv_lower, beta, i0, i1)
        mw = m * W
        g_sf2 = g_sf2 + (mw * ut["kv"]).sum()
        val.g_w[:] += (mw[..., None] * ut["uw"]).sum((0, 1))
        rc = mw[..., None] * ut["urow"]
        val.g_U[i0:i1] += rc.sum(1)
        val.g_U[:i1] -= rc.sum(0)
        ii = np.arange(i0, i1)
        kept = m[ii - i0, ii] > 0
        np.add.at(val.g_tau, g[ii][kept], W[ii - i0, ii][kept])
        if not want_bound:
            continue
        ma = m * Wabs
        nterms += int((m > 0).sum())
        np.add.at(ntau, g[ii][kept], 1)
        np.add.at(mag.g_tau, g[ii][kept], Wabs[ii - i0, ii][kept])
        tv = _both(ut["rel_v"], chain)
        td = tv if ut["rel_d"] is None else _both(ut["rel_d"], chain)
        av = ma * ut["kv"]
        m_sf2, e_sf2 = m_sf2 + av.sum(), e_sf2 + (av * tv).sum()
        aw = np.abs(ut["uw"])
        mag.g_w[:] += (ma[..., None] * aw).sum((0, 1))
        err.g_w[:dsp] += ((ma * tv)[..., None] * aw[..., :dsp]).sum((0, 1))
        err.g_w[dsp:] += ((ma * td)[..., None] * aw[..., dsp:]).sum((0, 1))
        ar = np.abs(ut["urow"])
        a = min(dU, dsp)
        rm = ma[..., None] * ar
        re = np.concatenate([(ma * tv)[..., None] * ar[..., :a], (ma * td)[..., None] * ar[..., a:]], axis=-1)
        mag.g_U[i0:i1] += rm.sum(1)
        mag.g_U[:i1] += rm.sum(0)
        err.g_U[i0:i1] += re.sum(1)
        err.g_U[:i1] += re.sum(0)
        wmax = 2 * Wabs.max(initial=0) * ut["pmax"]
        s, wm = abs(LD(sf2)), np.abs(np.asarray(w, dtype=LD)).max()
        cmax["sf2"] = max(cmax["sf2"], wmax)
        cmax["w"] = max(cmax["w"], wmax * s * ut["df2max"])
        cmax["U"] = max(cmax["U"], wmax * s * 2 * wm * ut["dfmax"])
    val = val._replace(g_sf2=np.asarray(g_sf2, dtype=LD))
    if not want_bound:
        return val, None
    floor = DENORMAL_STEPS * ETA
    bound = GradSums(
        g_w=err.g_w + gamma(nterms) * mag.g_w + floor * nterms * (1 + cmax["w"]),
        g_sf2=np.asarray(e_sf2 + gamma(nterms) * m_sf2 + floor * nterms * (1 + cmax["sf2"]), dtype=LD),
        g_tau=_both(gamma(W_ROUNDINGS), gamma(ntau)) * mag.g_tau + floor * ntau,
        g_U=err.g_U + gamma(N + 1) * mag.g_U + floor * N * (1 + cmax["U"]))
    return val, bound


def grad_sums(U, w, sf2, grp, S, kind, d_split, alpha, Kinv_lower, dU, *, beta=None, entries=None, rows=TILE):
    """The sums the header comment of the gradient section of gpp_reduce.hip states, over the lower triangle with weight 2 below the
    diagonal, in long double:
        W_ij = (alpha_i alpha_j - Kinv_ij) / 2,  or with ``beta``  -(alpha_i beta_j + beta_i alpha_j) / 2 - C_ij  (C in Kinv_lower)
        k_ij = exp(-r2_rbf) h(r2_mat)  (``kernel_factors``),  k' = k for an RBF feature, -dk / d r2_mat for a Matern one
        g_sf2 = sum mult W k      g_w[d] = -sum mult W sf2 k' (u_id - u_jd)^2      g_tau[s] = sum over i in group s of W_ii
        g_U[i, d] = -2 w_d sum_j mult W sf2 k' (u_id - u_jd)  over the entries (i, j) AND (j, i) of the lower triangle  (d < dU).
    Only Kinv_lower[i][j], j <= i, is read.  ``entries`` (N x N bool over the lower triangle) keeps a subset: one rank's partial sums
    (``shard_entries``); g_U[i] then receives the row contribution of the kept (i, j) and the column contribution of the kept (j, i),
    g_tau the W_ii of the kept diagonal entries.  Computed in blocks of ``rows`` rows: no N x N x D array."""
    return _grad_eval(U, w, sf2, grp, S, kind, d_split, alpha, Kinv_lower, dU, beta, entries, False, rows)[0]


def grad_bound(U, w, sf2, grp, S, kind, d_split, alpha, Kinv_lower, dU, *, beta=None, entries=None, rows=TILE):
    """What a fp64 evaluation of ``grad_sums`` may differ from it by, in any summation order, with or without fused multiply-adds;
    same shapes.  Derived, not fitted.  With u = 2^-53 (``U64``), gamma_n = n u / (1 - n u) and (1 + a)(1 + b) - 1 written a (+) b:

    A term is  mult W c k'  with c the remaining factors (1; sf2 d^2; 2 w_d sf2 d;  d = u_id - u_jd).  Its computed value differs by
      * r^2 (either half): each product (w d) d carries the roundings of d (twice), of w d and its own place in the chain of at most D
        fused steps, one more per step without fma (``R2_EXTRA`` = 4 beyond the chain): |r^2^ - r^2| <= gamma_{D+4} sum |w| d^2;
      * exp(-r2_rbf): that error amplified through exp, expm1(gamma_{D+4} sum |w| d^2), (+) the ``EXP_ULP`` = 2 ulp = 4 u of
        gpp_exp_nonpos;
      * the Matern factor (weights >= 0, so r^2 is known to gamma_{D+4} relative): r = sqrt(2 nu r2_mat) to rho = gamma_{D+4} / 2 + 2 u
        (half the error of the product 2 nu r2_mat, the rounding of sqrt, second order); e^-r to expm1(rho r) (+) 4 u; the polynomial
        1 + r to rho + u, 1 + r + r^2 / 3 to 2 rho + 5 u (all its terms are positive), (5/3)(1 + r) to rho + 2 u, 3 exactly; then
        k = er p e^-r and kd = er dp' e^-r with 2 resp. 3 more products;
      * W: ``W_ROUNDINGS`` = 4 roundings relative to Wabs = (|alpha_i beta_j| + |beta_i alpha_j|) / 2 + |C_ij| (W may cancel, so its
        error is taken against the magnitudes it is formed from; likewise (|alpha_i alpha_j| + |Kinv_ij|) / 2);
      * the handful of multiplications after it: ``CHAIN`` = 10 roundings with those of W, on the longest path (g_w),
    so  |term^ - term| <= A (rel_k' (+) gamma_10),  A = mult Wabs |c| k' >= |term|.
    The sum of the n kept terms in any order adds gamma_n sum A (n = N + 1 for a row of g_U: N - 1 terms, the partial sums of the
    tile columns, the final product with -2 w_d).  g_tau[s]: gamma_4 (+) gamma_{n_s} times the sum of Wabs_ii over its n_s members.
    Floor: an exponential below 2^-1022 is rounded to the denormal grid (absolute error one step eta = 2^-1074, and exactly 0 below
    -745.2 where long double is not), as may two products behind it: ``DENORMAL_STEPS`` = 4 steps per term, each amplified by at most
    the largest |mult Wabs c| max(p, dp') of the call.  (gpp_exp_nonpos also clamps below -800: the result is 0 by then.)"""
    return _grad_eval(U, w, sf2, grp, S, kind, d_split, alpha, Kinv_lower, dU, beta, entries, True, rows)[1]


def grad_sums_and_bound(U, w, sf2, grp, S, kind, d_split, alpha, Kinv_lower, dU, *, beta=None, entries=None, rows=TILE):
    """(grad_sums, grad_bound) in one pass."""
    return _grad_eval(U, w, sf2, grp, S, kind, d_split, alpha, Kinv_lower, dU, beta, entries, True, rows)


def shard_entries(N, nb, rank, nranks, by_cols):
    """The lower-triangle entries whose 64 x 64 tile ``rank`` owns: block-cyclic over the tile row's block of ``nb`` rows
    (grad_reduce_rows), or over its column block (grad_reduce_cols)."""
    assert nb % TILE == 0
    i, j = np.indices((N, N))
    return (j <= i) & ((((j if by_cols else i) // nb) % nranks) == rank)


def kinv_load_paths(N, ldk):
    """Which loads of Kinv gpp_grad_tiles takes for a matrix of leading dimension ``ldk``: 'vector' (two 16-byte loads, taken when
    pjb + 34 <= ldk) and / or 'scalar' (four guarded loads), over the threads of every tile column."""
    return {"vector" if j0 + 2 * tx + 34 <= ldk else "scalar" for j0 in range(0, N, TILE) for tx in range(16)}


# ---- vector reductions: (value, bound) ---------------------------------------------------------------------------------------
def _dot_rows(A, x, keep):
    A, x = np.where(keep, A, 0).astype(LD), np.asarray(x, dtype=LD)
    n = keep.sum(1)
    return A @ x, gamma(n + 2) * (np.abs(A) @ np.abs(x))


def trmv_lower(T, x):
    """y_i = sum_{k <= i} T[i][k] x_k; bound gamma_{i+3} sum |T_ik x_k| (i + 1 products and their sum, in any order)."""
    N = len(x)
    i, k = np.indices((N, N))
    return _dot_rows(np.asarray(T)[:N, :N], x, k <= i)


def trmv_upper(T, x):
    """y_j = sum_{i >= j} T[j][i] x_i  (row j of the upper triangle); bound as ``trmv_lower``."""
    N = len(x)
    j, i = np.indices((N, N))
    return _dot_rows(np.asarray(T)[:N, :N], x, i >= j)


def mll_scalars(Udiag, z):
    """(quad, logdet, mll) = (z'z, 2 sum log U_ii, -(quad + logdet + N log 2 pi) / 2) and their bounds: quad gamma_{N+1} z'z; logdet
    (``LOG_ULP`` ulp of each log (+) gamma_N) 2 sum |log U_ii|; mll half of both, of the roundings of N log 2 pi (the constant, the
    product) and of the two additions (gamma_2 of the magnitudes); the last product, by -1/2, is exact."""
    d, z = np.asarray(Udiag, dtype=LD), np.asarray(z, dtype=LD)
    N = len(z)
    lg = np.log(d)
    quad, logdet, c = (z * z).sum(), 2 * lg.sum(), N * LOG_2PI
    mll = -(quad + logdet + c) / 2
    bq = gamma(N + 1) * quad
    bl = _both(LOG_REL, gamma(N)) * 2 * np.abs(lg).sum()
    bm = (bq + bl + gamma(2) * c + gamma(2) * (quad + abs(logdet) + c)) / 2
    return np.array([quad, logdet, mll], dtype=LD), np.array([bq, bl, bm], dtype=LD)


def predict_rows(Ksn, V, alpha, kss):
    """mean_a = sum_j Ksn[a][j] alpha_j (bound gamma_{N+2} sum |Ksn alpha|) and, with V, var_a = kss_a - sum_j V[a][j]^2: its bound is
    on the difference as computed, gamma_{N+2} (|kss_a| + sum V^2), not relative to the result."""
    K, a = np.asarray(Ksn, dtype=LD), np.asarray(alpha, dtype=LD)
    N = len(a)
    mean, bmean = K @ a, gamma(N + 2) * (np.abs(K) @ np.abs(a))
    if V is None:
        return (mean, None), (bmean, None)
    q = (np.asarray(V, dtype=LD) ** 2).sum(1)
    k = np.asarray(kss, dtype=LD)
    return (mean, k - q), (bmean, gamma(N + 2) * (np.abs(k) + q))


# ---- storage -------------------------------------------------------------------------------------------------------------------
class Window:
    """A float64 buffer and the window of it that holds a matrix, as a kernel with 16-byte loads is handed it: the window starts at
    an even column ``col0`` of row ``row0`` (16-byte aligned when the buffer is), the leading dimension ``ld`` is even; everything
    else holds ``fill`` (NaN where the kernel may load but not use, a finite sentinel where it may not write).  Default ld: two
    guard columns on either side; ``ld`` = the smallest even number >= the width with ``col0`` = 0 gives the tightest legal rows."""

    def __init__(self, X, fill, ld=None, row0=1, col0=2, rows_below=2):
        X = np.asarray(X, dtype=np.float64)
        self.rows, self.cols = X.shape
        self.row0, self.col0 = row0, col0
        self.ld = col0 + self.cols + 2 + (self.cols & 1) if ld is None else ld
        assert self.ld % 2 == 0 and col0 % 2 == 0 and self.ld >= col0 + self.cols and rows_below >= 1
        self.buf = np.full((row0 + self.rows + rows_below, self.ld), fill, dtype=np.float64)
        self.window(self.buf)[...] = X

    def window(self, buf=None):
        """The window of ``buf`` (an array or tensor of the buffer's shape; default: the buffer itself)."""
        buf = self.buf if buf is None else buf
        return buf[self.row0:self.row0 + self.rows, self.col0:self.col0 + self.cols]

    def guard_mask(self):
        g = np.ones(self.buf.shape, dtype=bool)
        self.window(g)[...] = False
        return g


class VectorWindow:
    """n contiguous doubles at an even offset of a longer buffer of ``fill``; ``shape`` reshapes the window (a contiguous matrix)."""
    LEAD, TRAIL = 2, 3

    def __init__(self, n, fill, x=None, shape=None):
        self.n, self.shape = n, shape
        self.buf = np.full(self.LEAD + n + self.TRAIL, fill, dtype=np.float64)
        if x is not None:
            self.buf[self.LEAD:self.LEAD + n] = np.asarray(x, dtype=np.float64).reshape(-1)

    def window(self, buf=None):
        buf = self.buf if buf is None else buf
        v = buf[self.LEAD:self.LEAD + self.n]
        return v if self.shape is None else v.reshape(self.shape)

    def guard_mask(self):
        g = np.ones(self.buf.shape, dtype=bool)
        g[self.LEAD:self.LEAD + self.n] = False
        return g


def lower_only(K, fill=np.nan):
    """K with ``fill`` in the strict upper triangle."""
    K = np.array(K, dtype=np.float64)
    K[np.triu_indices(K.shape[0], 1)] = fill
    return K


def even_ld(n):
    return max(2, n + (n & 1))


def same_bits(a, b):
    """Bitwise equality of two float64 arrays (distinguishes -0.0 from 0.0, equates identical NaNs)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def noise_groups(mode, N, rng):
    """(grp, S): 'one' = a single level and no index vector; 'gap' = three levels of which level 1 has no member; 'max' = 64."""
    if mode == "one":
        return None, 1
    if mode == "gap":
        return rng.choice(np.array([0, 2], dtype=np.int32), N), 3
    assert mode == "max"
    return rng.integers(0, 64, N).astype(np.int32), 64


def gradient_inputs(N, D, seed, special=False, loo=False):
    """U ~ 0.7 N(0, 1), w uniform in [0.05, 2], alpha (beta) ~ N(0, 1), Kinv (C) a random symmetric matrix, sf2.  ``special``: two
    pairs of coincident rows, one inside a tile (rows 0 and 1) and one across tiles (rows 2 and N - 2 once N >= 67), the last
    max(1, N / 8) rows at r^2 > 800 from the rest (N >= 4), and row 3 at r^2 = 725 from row 0 along feature 0 (N >= 6), where
    exp(-r^2) is a denormal.  A smaller N keeps what fits."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((N, D)) * 0.7
    w = rng.uniform(0.05, 2.0, D)
    alpha = rng.standard_normal(N)
    beta = rng.standard_normal(N) if loo else None
    K = rng.standard_normal((N, N))
    K = K + K.T
    if special:
        if N >= 2:
            U[1] = U[0]
        if N >= 4:
            far = max(1, N // 8)
            U[N - far:] += 45.0 / np.sqrt(w)  # every feature alone gives w d^2 ~ 45^2 > 800
        if N >= 6:
            U[3] = U[0]
            U[3, 0] += np.sqrt(725.0 / w[0])
        if N >= 67:
            U[N - 2] = U[2]
    return dict(U=U, w=w, sf2=float(rng.uniform(0.5, 1.5)), alpha=alpha, beta=beta, K=K)


Case = collections.namedtuple("Case", "N D dU kind d_split smode ld special loo seed")
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 191)
FEATURES = {8: (1, 8), 16: (9, 16), 32: (17, 32), 64: (33, 64)}  # both edges of each DT instantiation
SMODES = ("one", "gap", "max")
LDS = ("min", "pad")


def instantiation(c):
    """(DT, MAT, HASU, LOO) of gpp_grad_tiles that a case runs."""
    return (next(dt for dt in sorted(FEATURES) if c.D <= dt), c.kind != 0, c.dU > 0, bool(c.loo))


def _cycle(values, n, rng):
    return [values[k] for k in rng.permutation(np.arange(n) % len(values))]


def gradient_cases(seed=20240):
    """One call per (template instantiation, size): 32 x 9.  Inside an instantiation every other axis is a seeded shuffle of its
    values repeated to nine (D, d_split and dU one joint shuffle), so each value of each axis meets each instantiation; tests/test_reduce_reference_host.py asserts that and
    the cross coverage (every N with dU > 0 for all three kinds)."""
    rng = np.random.default_rng(seed)
    cases = []
    for dt in sorted(FEATURES):
        for mat in (False, True):
            for hasu in (False, True):
                for loo in (False, True):
                    n = len(SIZES)
                    # (D, d_split, dU) jointly: both D with each of d_split = 0, 1, D - 1, D and with dU = 1 and D
                    joint = [(FEATURES[dt][k % 2], (0, 1, -1, None)[(k // 2) % 4], bool((k // 2) % 2)) for k in rng.permutation(n)]
                    Ds, splits, wide = zip(*joint)
                    kinds = _cycle((1, 2), n, rng) if mat else [0] * n
                    sm, lds, sp = _cycle(SMODES, n, rng), _cycle(LDS, n, rng), _cycle((False, True), n, rng)
                    for k, N in enumerate(rng.permutation(SIZES)):
                        D = Ds[k]
                        ds = {0: 0, 1: min(1, D), -1: D - 1, None: D}[splits[k]] if mat else 0
                        dU = (D if wide[k] else 1) if hasu else 0
                        cases.append(Case(int(N), D, dU, kinds[k], ds, sm[k], lds[k], sp[k], loo, len(cases)))
    return cases

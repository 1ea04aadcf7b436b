"""CPU reference of the factorisation chain potrf -> trtri -> lauum at the sizes that leaf steps serve (N <= 513): the 128-row leaf
(gpp_leaf_potrf_inv), the leaf-step chain (potrf_blk, potrf_blk_batched), the cooperative panel (gpp_panel_potrf_inv) and the pair
merges of the inverse (trtri_level).  Plain numpy, every product and sum of the checkers in ``np.longdouble``.

  ``plan``              which identity covers which block of U (upper triangle) and of X = inv(L) (lower triangle), per driver;
  ``evaluate``          (item, err, bound) of every item of a plan, each step held to what the kernel itself wrote;
  ``lauum_check``, ``mirror_ok``, ``entry_bounds``, ``implied_inverse_residual``
  ``emulate``           a fp64 emulation of each driver's operation order (tests/test_factor_reference_host.py keeps it inside the
                        bounds and mutates it);
  ``matrix`` / ``cases``   the seeded case matrices and the case list of tests/test_gpu_factor_conformance.py.

Notation: A the matrix, U the upper factor read back (A = U^T U, L = U^T), X the lower triangle of the inverse read back, W_k its
diagonal block k (the inverse of leaf k), L_ab = U_ba^T.  u = 2^-53, gamma_n = n u / (1 - n u).  A sum of n products accumulated in any
order, starting from the value it is added to, differs from the exact one by gamma_n times the sum of magnitudes (Higham, Accuracy
and Stability of Numerical Algorithms, lemma 8.4: every (1 + delta) of the running sum divides out against the first summand); this
covers whatever order the MFMA chain, the K-loop of a GEMM tile or the strips of the panel take.  The constants below are the
roundings BEYOND that sum, read off the code (csrc/gpp_leaf.hip, csrc/gpp_api.hip); they are counted, not fitted.

Largest entry bound / max|U| over the case list, measured on the fp64 emulation (``RECORDED_ENTRY_BOUND``; the host tests assert
that it is reached, not exceeded, and below the 1e-10 max|L| of the older factorisation tests): this is what the sharpness of the GPU
suite rests on.
    well 7.9e-14    cov 7.9e-13    graded 7.4e-14
Largest implied bound of |X L - I| (``RECORDED_INVERSE_RESIDUAL``, below the older 1e-8):
    well 1.2e-13    cov 1.45e-11   graded 9.8e-14

Nothing here imports torch or touches a GPU.
"""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reduce_reference import LD, U64, SENTINEL, Window, VectorWindow, gamma, same_bits  # noqa: E402,F401

NBLK = 128  # rows of a leaf (GPP_TILE)
TS = 16     # rows of a tile of the leaf

#: the reciprocal pivot (gpp_leaf.hip chol_pivots): r = rsq(a) refined by two Newton steps, each fma(r/2, fma(-a r, r, 1), r).  The
#: product a r inside the last step is rounded (its error enters r halved) and the outer fma rounds once: r = a^-1/2 (1 + e),
#: |e| <= 2 u once the quadratic term of the first step is gone.  The diagonal is stored as l = fl(a r) and every other entry of the
#: column is multiplied by r, so relative to the STORED l: l^2 = a (1+e)^2 (1+d)^2 and x l = s (1+d) (1+e)^2 (1+d'): 6 roundings.
C_PIVOT = 6
#: one v_mfma_f64_16x16x4_f64 adds four products to the accumulator in an order the ISA does not state: 4 additions for the summand
#: that enters last, and 1 for a product that is not fused.  (The chain ACROSS the instructions starts from the accumulator, so
#: lemma 8.4 applies to it: n products cost gamma_n, not gamma_2n.)
C_MFMA = 5
#: leaf, diagonal block: |S - U^T U| <= gamma_{n + C_LEAF} |U|^T |U|: the <= n products of an entry (trailing MFMA updates of
#: leaf_body step (4), then the fused chains of chol_update or of the substitution in step (3)) and the two constants above
C_LEAF = C_PIVOT + C_MFMA
#: one rank-128 update C <- beta C + alpha acc (potrf_blk's ``u``; the panel's ``cold - x``): the K = 128 sum (gamma_128 on the
#: products, the any-order bound), then the epilogue of gpp_gemm.hip, ``v = alpha * acc`` and ``v = fma(beta, cold, v)``: one
#: rounding each.  After k updates an entry of A has met k such additions and each product at most 128 + k + 1 roundings:
#: gamma_{k (128 + 1) + C_UPDATE} is above that
C_UPDATE = 2
#: block row right of a leaf, U_kj = W_k S_kj (potrf_blk's ``g``, a_mask = 1, alpha = 1, beta = 0; the panel's S step): K = n_k
#: products that need not be fused (1) and the product with alpha (1)
C_SOLVE = 2
#: pair merge X21 = -X22 (L21 X11), two products in a row (leaf: merge_level phases a and b; trtri_level: g1 and g2), each with a
#: product that need not be fused (1) and its alpha (1: exact for 1 and -1, counted; the leaf negates an operand, exact)
C_MERGE = 4
#: bordering strip of the panel (inverse_row): the sum over m continues in the same accumulators (128 (j - i) products), then the
#: product with W_j (n_j): one unfused product each; the final negation is exact
C_BORDER = 2
#: 16 x 16 diagonal tile of a leaf inverse (leaf_body, "inverse of the 8 diagonal tiles"): lane j solves L x = e_j by forward
#: substitution in column order, x_r = (e_r - sum_{k<r} L_rk x_k) rd_r with fused updates: at most 15 fused steps and the product
#: with rd = 1/l (1 + theta_5) (C_PIVOT without the rounding of l itself, plus the product's own): the residual it guarantees is the
#: one with L on the LEFT, |L_tt X_tt - I| <= gamma_{16 + C_TILE} |L_tt| |X_tt|
C_TILE = C_PIVOT
#: lauum (gpp_lauum: one masked GEMM, K <= N, alpha = 1, beta = 0): an unfused product (1) and alpha (1)
C_LAUUM = 2

#: the measured figures of the module docstring (tests/test_factor_reference_host.py)
RECORDED_ENTRY_BOUND = {"well": 7.9e-14, "cov": 7.9e-13, "graded": 7.4e-14}
RECORDED_INVERSE_RESIDUAL = {"well": 1.2e-13, "cov": 1.45e-11, "graded": 9.8e-14}

Item = collections.namedtuple("Item", "identity r0 r1 c0 c1 tri k s")  # block [r0, r1) x [c0, c1); tri: 'upper', 'lower' or None
Plan = collections.namedtuple("Plan", "U X")
DRIVERS = ("chain", "panel", "batched")


def leaves(N):
    return [(o, min(NBLK, N - o)) for o in range(0, N, NBLK)]


def _leaf_inverse_items(o, n):
    """The items of one leaf's inverse: its 16 x 16 diagonal tiles, then the merge levels of 16, 32 and 64 rows (merge_level<1, 2, 4>),
    clipped to the n rows the leaf has (the padding is the identity: a clipped pair is the ragged pair of that level)."""
    items = [Item("inv_tile", t, min(t + TS, o + n), t, min(t + TS, o + n), "lower", 0, TS) for t in range(o, o + n, TS)]
    for s in (16, 32, 64):
        for b in range(o, o + n, 2 * s):
            if b + s < o + n:
                items.append(Item("inv_merge_leaf", b + s, min(b + 2 * s, o + n), b, b + s, None, 0, s))
    return items


def plan(driver, N):
    """Which identity covers which block, following the drivers' own block boundaries:
      U  per leaf k (potrf_blk / potrf_blk_batched step, or the panel's block row): 'factor_diag' on the upper triangle of the leaf,
         'factor_row' on the block row right of it;
      X  per leaf its tiles and internal merges; then for 'chain' and 'batched' the pairs of trtri_level at s = 128, 256, ... < N
         (full pairs and the ragged last one: rem > s), which no ``skip`` drops below the panel's sizes; for 'panel' the bordering
         strips (block row j against block column i < j), after which gpp_trtri skips every pair."""
    assert driver in DRIVERS and N >= 1
    Us, Xs = [], []
    for k, (o, n) in enumerate(leaves(N)):
        Us.append(Item("factor_diag", o, o + n, o, o + n, "upper", k, n))
        if o + n < N:
            Us.append(Item("factor_row", o, o + n, o + n, N, None, k, n))
        Xs += _leaf_inverse_items(o, n)
    if driver == "panel":
        lv = leaves(N)
        for j, (oj, nj) in enumerate(lv):
            for i in range(j):
                Xs.append(Item("inv_border", oj, oj + nj, lv[i][0], lv[i][0] + NBLK, None, j, i))
    else:
        s = NBLK
        while s < N:
            for b in range(0, N, 2 * s):
                if b + s < N:
                    Xs.append(Item("inv_merge_level", b + s, min(b + 2 * s, N), b, b + s, None, 0, s))
            s *= 2
    return Plan(Us, Xs)


def coverage(items, N):
    """How many items cover each entry (an N x N count)."""
    cnt = np.zeros((N, N), dtype=np.int64)
    for it in items:
        m = np.ones((it.r1 - it.r0, it.c1 - it.c0), dtype=np.int64)
        if it.tri == "upper":
            m = np.triu(m)
        elif it.tri == "lower":
            m = np.tril(m)
        cnt[it.r0:it.r1, it.c0:it.c1] += m
    return cnt


def _ld(x):
    return np.asarray(x, dtype=LD)


def evaluate(pl, A, U, X):
    """[(item, err, bound)] for every item of the plan: A the matrix (its upper triangle is read), U the factor and X the inverse as
    the kernel wrote them (upper resp. lower triangle read).  err and bound have the item's shape; outside its triangle both are 0.

      factor_diag  S_kk = A_kk - sum_{i<k} U_ik^T U_ik:  |S_kk - U_kk^T U_kk| <= gamma_{n_k + C_LEAF} |U_kk|^T |U_kk| + delta_kk
      factor_row   |U_kj - W_k S_kj| <= gamma_{n_k + C_SOLVE} |W_k| |S_kj| + (1 + gamma) |W_k| delta_kj
                   delta = gamma_{k (128 + 1) + C_UPDATE} (|A_kj| + sum_{i<k} |U_ik|^T |U_ij|)   (0 for k = 0: no update has run)
      inv_tile     |L_tt X_tt - I| <= gamma_{16 + C_TILE} |L_tt| |X_tt|
      inv_merge_*  |X_21 + X_22 (L_21 X_11)| <= gamma_{s + m2 + C_MERGE} |X_22| |L_21| |X_11|
      inv_border   |X_ji + W_j sum_{m=i}^{j-1} L_jm X_mi| <= gamma_{128 (j - i) + n_j + C_BORDER} |W_j| sum |L_jm| |X_mi|
    """
    N = A.shape[0]
    Au, Uu, Xl = np.triu(_ld(A)), np.triu(_ld(U)), np.tril(_ld(X))
    aA, aU, aX = np.abs(Au), np.abs(Uu), np.abs(Xl)
    out = []
    schur = {}
    for it in pl.U:
        o, n, k = it.r0, it.s, it.k
        if k not in schur:
            P = Uu[:o, o:o + n].T @ Uu[:o, o:] if o else np.zeros((n, N - o), LD)
            Pa = aU[:o, o:o + n].T @ aU[:o, o:] if o else np.zeros((n, N - o), LD)
            delta = (gamma(k * (NBLK + 1) + C_UPDATE) if k else LD(0)) * (aA[o:o + n, o:] + Pa)
            schur = {k: (Au[o:o + n, o:] - P, delta)}
        S, delta = schur[k]
        if it.identity == "factor_diag":
            Ud, aUd = Uu[o:o + n, o:o + n], aU[o:o + n, o:o + n]
            err = np.triu(np.abs(S[:, :n] - Ud.T @ Ud))
            bound = np.triu(gamma(n + C_LEAF) * (aUd.T @ aUd) + delta[:, :n])
        else:
            W, aW = Xl[o:o + n, o:o + n], aX[o:o + n, o:o + n]
            g = gamma(n + C_SOLVE)
            err = np.abs(Uu[o:o + n, o + n:] - W @ S[:, n:])
            bound = g * (aW @ np.abs(S[:, n:])) + (1 + g) * (aW @ delta[:, n:])
        out.append((it, err, bound))
    for it in pl.X:
        r0, r1, c0, c1 = it.r0, it.r1, it.c0, it.c1
        if it.identity == "inv_tile":
            Lt, Xt = Uu[r0:r1, r0:r1].T, Xl[r0:r1, r0:r1]
            err = np.tril(np.abs(Lt @ Xt - np.eye(r1 - r0, dtype=LD)))
            bound = np.tril(gamma(TS + C_TILE) * (np.abs(Lt) @ np.abs(Xt)))
        elif it.identity in ("inv_merge_leaf", "inv_merge_level"):
            X11, X22, L21 = Xl[c0:c1, c0:c1], Xl[r0:r1, r0:r1], Uu[c0:c1, r0:r1].T
            err = np.abs(Xl[r0:r1, c0:c1] + X22 @ (L21 @ X11))
            bound = gamma(it.s + (r1 - r0) + C_MERGE) * (np.abs(X22) @ (np.abs(L21) @ np.abs(X11)))
        else:
            assert it.identity == "inv_border"
            Wj, Ljm, Xmi = Xl[r0:r1, r0:r1], Uu[c0:r0, r0:r1].T, Xl[c0:r0, c0:c1]
            err = np.abs(Xl[r0:r1, c0:c1] + Wj @ (Ljm @ Xmi))
            bound = gamma(NBLK * (it.k - it.s) + (r1 - r0) + C_BORDER) * (np.abs(Wj) @ (np.abs(Ljm) @ np.abs(Xmi)))
        out.append((it, err, bound))
    return out


def lauum_check(X, Kinv):
    """(err, bound) of the lower triangle of Kinv against (X^T X) of the X the kernel wrote: gamma_{N + C_LAUUM} |X|^T |X|."""
    Xl = np.tril(_ld(X))
    N = Xl.shape[0]
    aX = np.abs(Xl)
    return np.tril(np.abs(np.tril(_ld(Kinv)) - Xl.T @ Xl)), np.tril(gamma(N + C_LAUUM) * (aX.T @ aX))


def mirror_ok(Xfull):
    """The strict upper triangle of the inverse is the transpose of the strict lower one, bit for bit."""
    Xfull = np.asarray(Xfull, dtype=np.float64)
    return same_bits(np.triu(Xfull, 1), np.tril(Xfull, -1).T)


def ratio(err, bound):
    """Largest err / bound; inf where an entry is outside (an entry whose bound is 0 must be exact) or not finite."""
    err, bound = _ld(err), _ld(bound)
    if not (np.isfinite(err).all() and np.isfinite(bound).all()):
        return float("inf")
    pos = bound > 0
    if (err[~pos] != 0).any():
        return float("inf")
    return float((err[pos] / bound[pos]).max(initial=0))


def entry_bounds(results, U):
    """(EU, EX): how far one entry of U (upper) or of X (lower) may move, all others fixed, before its identity flags it.  Where the
    identity states the entry itself (factor_row, the merges, the bordering) that is the bound; where it states a residual
    (factor_diag: d/dU_ij of (U^T U)_ij is U_ii; inv_tile: d/dX_rj of (L X)_rj is L_rr) it is the bound over that coefficient."""
    N = U.shape[0]
    EU, EX = np.zeros((N, N), LD), np.zeros((N, N), LD)
    for it, _, bound in results:
        dst = EU if it.identity.startswith("factor") else EX
        b = bound
        if it.identity in ("factor_diag", "inv_tile"):
            d = np.abs(np.diag(_ld(U)[it.r0:it.r1, it.r0:it.r1]))
            b = bound / d[:, None]
        dst[it.r0:it.r1, it.c0:it.c1] += b
    return EU, EX


def implied_inverse_residual(EX, U):
    """What |X L - I| may reach when every entry of X sits at its entry bound from one that meets its identity exactly: EX |L|."""
    return EX @ np.abs(np.triu(_ld(U)).T)


# ---- case matrices -------------------------------------------------------------------------------------------------------------
CLASSES = ("well", "cov", "graded")


def matrix(cls, N, seed=0):
    """Seeded SPD fp64 matrices:
      well    B B^T / N + I;
      cov     an RBF Gram matrix exp(-|x - y|^2 / (2 l^2)) of uniform points in [0, 1]^6, l = 0.35, plus 1e-6 I: the project's own
              workload shape (l chosen so that the entry bounds stay below the tolerances of the existing tests);
      graded  ``well`` scaled from both sides by 10^e, e uniform in [-1, 1]: normwise agreement would hide a wrong small row."""
    rng = np.random.default_rng(1000 * CLASSES.index(cls) + 7 * N + seed)
    if cls == "cov":
        P = rng.uniform(0, 1, (N, 6))
        d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)
        K = np.exp(-d2 / (2 * 0.35 ** 2)) + 1e-6 * np.eye(N)
    else:
        B = rng.standard_normal((N, N))
        K = B @ B.T / N + np.eye(N)
        if cls == "graded":
            d = 10.0 ** rng.uniform(-1, 1, N)
            K = d[:, None] * K * d[None, :]
    return np.ascontiguousarray((K + K.T) / 2)


Case = collections.namedtuple("Case", "driver N cls use_ws panel")
LEAF_EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128)
CHAIN_SIZES = (129, 143, 256, 257, 300, 384, 385, 513)
PANEL_SIZES = (257, 300, 384, 385, 513)
BATCH, BATCHED_SIZES = 3, (1, 16, 127, 129, 257, 385)


def _cls_of(N, k=0):
    return CLASSES[(N + k) % 3]


def cases():
    """The case list of the GPU suite.  One leaf: every n = 1 .. 128 on ``well`` and the edges on the other two classes; the chain
    at each of its sizes without and with the scratch (panel off); the panel; the batched call (its three elements take the three
    classes in an order that depends on N).  The chain and panel sizes rotate through the classes."""
    out = [Case("chain", n, "well", False, False) for n in range(1, NBLK + 1)]
    out += [Case("chain", n, c, False, False) for n in LEAF_EDGES for c in ("cov", "graded")]
    for N in CHAIN_SIZES:
        out += [Case("chain", N, _cls_of(N), False, False), Case("chain", N, _cls_of(N, 1), True, False)]
    out += [Case("panel", N, _cls_of(N, 2), True, True) for N in PANEL_SIZES]
    out += [Case("batched", N, _cls_of(N, b), False, False) for N in BATCHED_SIZES for b in range(BATCH)]
    return out


# ---- fp64 emulation of the drivers' operation order ------------------------------------------------------------------------------
def _emulate_leaf(S, n, mut):
    """Factor and inverse of one leaf in fp64, in the kernel's order: right-looking by columns with the reciprocal pivot; the
    16 x 16 diagonal tiles inverted by forward substitution with those reciprocals; merges of 16, 32 and 64 rows."""
    a = np.tril(S.T).copy()  # L = U^T
    rd = np.empty(n)
    for k in range(n):
        r = 1.0 / np.sqrt(a[k, k])
        if mut.get("pivot_fp32") == k:
            r = float(np.float32(r))
        rd[k] = r
        a[k, k] = a[k, k] * r
        a[k + 1:, k] *= r
        a[k + 1:, k + 1:] -= np.tril(np.outer(a[k + 1:, k], a[k + 1:, k]))
    X = np.zeros((n, n))
    for t in range(0, n, TS):
        e = min(t + TS, n)
        x = np.eye(e - t)
        for r in range(e - t):
            x[r, :] *= rd[t + r]
            x[r + 1:, :] -= np.outer(a[t + r + 1:e, t + r], x[r, :])
        X[t:e, t:e] = np.tril(x)
    for s in (16, 32, 64):
        for b in range(0, n, 2 * s):
            if b + s < n:
                e = min(b + 2 * s, n)
                X[b + s:e, b:b + s] = -X[b + s:e, b + s:e] @ (a[b + s:e, b:b + s] @ X[b:b + s, b:b + s])
                f = mut.get("flip_tile")
                if f and b + s <= f[0] < e and b <= f[1] < b + s:
                    X[f[0]:f[0] + TS, f[1]:f[1] + TS] *= -1
    return a.T, X


def emulate(driver, A, mut=None):
    """(U, Xfull, Kinv) of a fp64 emulation of the driver: leaf steps with the explicit inverse (potrf_blk), then pair merges
    (trtri_level) or, for the panel, bordering by block rows; the mirror; lauum.  ``mut`` names one mutation:
      skip_update  (k, c0): the rank-128 update of step k skips the 32 columns from c0;   flip_tile  (r, c): the 16 x 16 tile at
      (r, c) of the merge that covers it gets the wrong sign;   pivot_fp32  (k, p): pivot p of leaf k through fp32."""
    mut = mut or {}
    N = A.shape[0]
    W = np.triu(np.asarray(A, dtype=np.float64)).copy()
    X = np.zeros((N, N))
    lv = leaves(N)
    for k, (o, n) in enumerate(lv):
        pm = {"pivot_fp32": mut["pivot_fp32"][1]} if mut.get("pivot_fp32", (None,))[0] == k else {}
        f = mut.get("flip_tile")
        if f and o <= f[1] <= f[0] < o + n:
            pm["flip_tile"] = (f[0] - o, f[1] - o)
        Ukk, Xkk = _emulate_leaf(W[o:o + n, o:o + n], n, pm)
        W[o:o + n, o:o + n] = np.triu(Ukk)
        X[o:o + n, o:o + n] = Xkk
        if o + n < N:
            W[o:o + n, o + n:] = Xkk @ W[o:o + n, o + n:]
            R = W[o:o + n, o + n:]
            upd = R.T @ R
            if mut.get("skip_update", (None,))[0] == k:
                c = mut["skip_update"][1] - (o + n)
                upd[:, c:c + 32] = 0
            W[o + n:, o + n:] -= np.triu(upd)

    def flip(r0, r1, c0, c1):
        f = mut.get("flip_tile")
        if f and r0 <= f[0] < r1 and c0 <= f[1] < c1:
            X[f[0]:f[0] + TS, f[1]:f[1] + TS] *= -1

    if driver == "panel":
        for j, (oj, nj) in enumerate(lv):
            for i in range(j):
                oi = lv[i][0]
                X[oj:oj + nj, oi:oi + NBLK] = -X[oj:oj + nj, oj:oj + nj] @ (W[oi:oj, oj:oj + nj].T @ X[oi:oj, oi:oi + NBLK])
                flip(oj, oj + nj, oi, oi + NBLK)
    else:
        s = NBLK
        while s < N:
            for b in range(0, N, 2 * s):
                if b + s < N:
                    e = min(b + 2 * s, N)
                    X[b + s:e, b:b + s] = -X[b + s:e, b + s:e] @ (W[b:b + s, b + s:e].T @ X[b:b + s, b:b + s])
                    flip(b + s, e, b, b + s)
            s *= 2
    Kinv = np.tril(X.T @ X)
    return np.triu(W), X + np.tril(X, -1).T, Kinv

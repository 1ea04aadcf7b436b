"""CPU reference of the library's masked GEMM (``gpp_gemm`` in ``include/gpp.h``), in plain numpy:

  ``masked_product``   C = beta*C0 + alpha*Am@Bm on the entries ``c_tri`` selects, C0 elsewhere, from the LOGICAL operands op(A)
                       (M x K) and op(B) (K x N): integer inputs are multiplied in int64 (exact), real ones in ``np.longdouble``;
  ``error_bound``      the elementwise bound a fp64 product of real inputs must meet, whatever its summation order;
  ``legal_hints``      the K-range modes each mask pair permits (they never enter the reference: a legal hint only skips zeros);
  ``store`` & co.      the operands as the kernel is handed them: interior windows of larger NaN- or sentinel-filled buffers.

Nothing here imports torch or touches a GPU.
"""
import itertools

import numpy as np

#: name -> (transA, transB) of the three supported layouts
VARIANTS = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0)}
#: value of the tile option -> work-group tile (rows, columns)
TILES = {1: (32, 32), 2: (64, 64), 3: (128, 128), 4: (128, 32)}
MASK_PAIRS = tuple(itertools.product((0, 1, 2), repeat=2))
#: what the guard of an output buffer holds: finite, so that it can be compared after the run, and outside the range of C0
SENTINEL = 7777.0


def keep(mask, rows, K):
    """(rows x K) boolean: element [r, k] of an operand survives its triangular mask."""
    r = np.arange(rows)[:, None]
    k = np.arange(K)[None, :]
    if mask == 0:
        return np.ones((rows, K), dtype=bool)
    if mask == 1:
        return k <= r
    if mask == 2:
        return k >= r
    raise ValueError(mask)


def masked_operands(A_op, B_op, a_mask, b_mask):
    """op(A) and op(B) with the dropped entries zeroed: op(A)[m, k] by (mask, k, m), op(B)[k, n] by (mask, k, n)."""
    M, K = A_op.shape
    K2, N = B_op.shape
    assert K == K2
    return np.where(keep(a_mask, M, K), A_op, 0), np.where(keep(b_mask, N, K).T, B_op, 0)


def selected(c_tri, M, N):
    """(M x N) boolean: the entries of C the product writes."""
    m = np.arange(M)[:, None]
    n = np.arange(N)[None, :]
    if c_tri == 0:
        return np.ones((M, N), dtype=bool)
    assert M == N
    return n <= m if c_tri == 1 else n >= m


def _is_exact(*arrays):
    return all(np.issubdtype(a.dtype, np.integer) for a in arrays)


def masked_matmul(A_op, B_op, a_mask, b_mask):
    """Am @ Bm: in int64 for integer operands, in ``np.longdouble`` otherwise."""
    Am, Bm = masked_operands(A_op, B_op, a_mask, b_mask)
    acc = np.int64 if _is_exact(A_op, B_op) else np.longdouble
    return Am.astype(acc) @ Bm.astype(acc)


def masked_product(A_op, B_op, a_mask, b_mask, c_tri, alpha, beta, C0, P=None):
    """Integer A_op, B_op, C0: the exact result as float64 (asserted representable, with every partial sum, below 2^53).
    Real inputs: the result in ``np.longdouble``.  P: ``masked_matmul`` of the same operands and masks, if the caller kept it."""
    if P is None:
        P = masked_matmul(A_op, B_op, a_mask, b_mask)
    M, N = C0.shape
    if _is_exact(A_op, B_op, C0):
        # alpha*P and beta*C0 are exact when 2 alpha and beta are integers; every partial sum of P, in any order, is an integer
        # of magnitude at most K max|A| max|B|
        assert P.dtype == np.int64
        assert float(2 * alpha).is_integer() and float(beta).is_integer(), (alpha, beta)
        K = A_op.shape[1]
        amax = int(np.abs(A_op).max(initial=0)) * int(np.abs(B_op).max(initial=0))
        assert 2 * (abs(alpha) * K * amax + abs(beta) * int(np.abs(C0).max(initial=0))) < 2 ** 53
        full = beta * C0.astype(np.float64) + alpha * P.astype(np.float64)
        out = C0.astype(np.float64)
    else:
        ld = np.longdouble
        assert P.dtype == ld
        full = ld(beta) * C0.astype(ld) + ld(alpha) * P
        out = C0.astype(ld)
    sel = selected(c_tri, M, N)
    out[sel] = full[sel]
    return out


def error_bound(A_op, B_op, a_mask, b_mask, alpha, beta, C0):
    """(K + 4) 2^-53 (|alpha| |Am| @ |Bm| + |beta| |C0|), elementwise, in ``np.longdouble``: the dot-product bound gamma_{K+2} of
    any accumulation order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1) plus the roundings of alpha
    and beta.  Derived, not measured."""
    ld = np.longdouble
    Am, Bm = masked_operands(A_op, B_op, a_mask, b_mask)
    K = A_op.shape[1]
    return (K + 4) * ld(2.0) ** -53 * (abs(ld(alpha)) * (np.abs(Am).astype(ld) @ np.abs(Bm).astype(ld)) + abs(ld(beta)) * np.abs(C0).astype(ld))


# ---- K-range hints -------------------------------------------------------------------------------------------------------------
def legal_klo(a_mask, b_mask):
    out = []
    if a_mask == 2:
        out.append(1)
    if b_mask == 2:
        out.append(2)
    if a_mask == 2 and b_mask == 2:
        out.append(3)
    return out


def legal_khi(a_mask, b_mask):
    out = []
    if a_mask == 1:
        out.append(1)
    if b_mask == 1:
        out.append(2)
    return out


def legal_hints(a_mask, b_mask):
    """Every (klo_mode, khi_mode) but (0, 0) the mask pair permits: each legal mode alone, and a legal lower with a legal upper."""
    los, his = [0] + legal_klo(a_mask, b_mask), [0] + legal_khi(a_mask, b_mask)
    return [(lo, hi) for lo in los for hi in his if (lo, hi) != (0, 0)]


def k_range(klo_mode, khi_mode, m0, n0, tile_m, tile_n, K):
    """[klo, khi) of the tile whose first row is m0 and first column n0, as include/gpp.h defines the modes."""
    klo = {0: 0, 1: m0, 2: n0, 3: max(m0, n0)}[klo_mode]
    khi = {0: K, 1: min(K, m0 + tile_m), 2: min(K, n0 + tile_n)}[khi_mode]
    return klo, khi


def empty_range_tiles(klo_mode, khi_mode, M, N, K, tile_m, tile_n):
    """(M x N) boolean: entries of the tiles whose K range is empty."""
    out = np.zeros((M, N), dtype=bool)
    for m0 in range(0, M, tile_m):
        for n0 in range(0, N, tile_n):
            klo, khi = k_range(klo_mode, khi_mode, m0, n0, tile_m, tile_n, K)
            if khi <= klo:
                out[m0:m0 + tile_m, n0:n0 + tile_n] = True
    return out


def hinted_product(A_op, B_op, a_mask, b_mask, klo_mode, khi_mode, tile_m, tile_n):
    """Am @ Bm with every tile's sum restricted to its hinted K range (float64 on integer inputs: exact)."""
    Am, Bm = masked_operands(A_op, B_op, a_mask, b_mask)
    Am, Bm = Am.astype(np.float64), Bm.astype(np.float64)
    M, K = Am.shape
    N = Bm.shape[1]
    P = np.zeros((M, N))
    for m0 in range(0, M, tile_m):
        for n0 in range(0, N, tile_n):
            klo, khi = k_range(klo_mode, khi_mode, m0, n0, tile_m, tile_n, K)
            if khi > klo:
                P[m0:m0 + tile_m, n0:n0 + tile_n] = Am[m0:m0 + tile_m, klo:khi] @ Bm[klo:khi, n0:n0 + tile_n]
    return P


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def exact_inputs(M, N, K, seed):
    """op(A), op(B) integers in [-3, 3], C0 integers in [-100, 100] (int64)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, (M, K), dtype=np.int64), rng.integers(-3, 4, (K, N), dtype=np.int64),
            rng.integers(-100, 101, (M, N), dtype=np.int64))


def real_inputs(M, N, K, seed):
    """Seeded standard normals (float64)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))


# ---- storage -------------------------------------------------------------------------------------------------------------------
class Stored:
    """A float64 buffer and the window of it that holds a matrix.  The window starts at an even column (16-byte aligned when the
    buffer is) in row 1; the leading dimension is even and at least 2 greater than the window's width, so the 16-byte load that
    straddles the end of an odd extent reads the fill; two guard rows follow the window.  A window of 0 rows or columns is widened
    to 1 (a pointer is needed even where nothing may be read) and holds the fill."""
    ROW0, COL0, ROWS_BELOW = 1, 2, 2

    def __init__(self, X, fill):
        X = np.asarray(X, dtype=np.float64)
        r, c = X.shape
        self.rows, self.cols = max(r, 1), max(c, 1)
        self.ld = self.COL0 + self.cols + 2 + (self.cols & 1)
        self.buf = np.full((self.ROW0 + self.rows + self.ROWS_BELOW, self.ld), fill, dtype=np.float64)
        self.buf[self.ROW0:self.ROW0 + r, self.COL0:self.COL0 + c] = X
        assert self.ld % 2 == 0 and self.ld > self.cols and self.COL0 % 2 == 0

    def window(self, buf=None):
        """The window of ``buf`` (any 2-D array or tensor of the buffer's shape; default: the buffer itself)."""
        buf = self.buf if buf is None else buf
        return buf[self.ROW0:self.ROW0 + self.rows, self.COL0:self.COL0 + self.cols]

    def guard_mask(self):
        g = np.ones(self.buf.shape, dtype=bool)
        self.window(g)[...] = False
        return g


def store_operands(A_op, B_op, variant):
    """op(A), op(B) in the layout the variant stores (transA: K x M, transB: N x K), NaN all around."""
    tA, tB = VARIANTS[variant]
    return Stored(A_op.T if tA else A_op, np.nan), Stored(B_op.T if tB else B_op, np.nan)


def store_output(C_init):
    return Stored(C_init, SENTINEL)


def same_bits(a, b):
    """Bitwise equality of two float64 arrays (distinguishes -0.0 from 0.0, equates identical NaNs)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))

"""The CPU reference of the masked GEMM (tests/gemm_reference.py) against explicit numpy, and the consistency of its hint table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_reference as gr  # noqa: E402


def test_masked_product_matches_tril_triu():
    """The five products of test_gemm_masks_and_lower, written out with np.tril / np.triu."""
    n = 37
    A, B, C0 = gr.real_inputs(n, n, n, seed=2)
    ld = np.longdouble
    Al, Bl, Cl = A.astype(ld), B.astype(ld), C0.astype(ld)
    # op(B)[k, n] keep k <= n: upper triangle of op(B) (X @ Lo^T);  keep k >= n: lower triangle (X @ Lo)
    np.testing.assert_array_equal(gr.masked_product(A, B, 0, 1, 0, 1.0, 0.0, C0), Al @ np.triu(Bl))
    np.testing.assert_array_equal(gr.masked_product(A, B, 0, 2, 0, 1.0, 0.0, C0), Al @ np.tril(Bl))
    # op(A)[m, k] keep k <= m: lower triangle of op(A) (Lo @ X)
    np.testing.assert_array_equal(gr.masked_product(A, B, 1, 0, 0, 1.0, 0.0, C0), np.tril(Al) @ Bl)
    # lauum: both keep k >= row, lower output only, the rest is C0
    got = gr.masked_product(A, B, 2, 2, 1, 1.0, 0.0, C0)
    full = np.triu(Al) @ np.tril(Bl)
    np.testing.assert_array_equal(np.tril(got), np.tril(full))
    np.testing.assert_array_equal(np.triu(got, 1), np.triu(Cl, 1))
    # syrk-style update of the upper triangle: C -= A B
    got = gr.masked_product(A, B, 0, 0, 2, -1.0, 1.0, C0)
    np.testing.assert_array_equal(np.triu(got), np.triu(Cl - Al @ Bl))
    np.testing.assert_array_equal(np.tril(got, -1), np.tril(Cl, -1))


def test_exact_and_real_paths_agree():
    """Integer inputs through int64 equal the same numbers through the longdouble path, masks, triangle and scalars included."""
    A, B, C0 = gr.exact_inputs(45, 38, 51, seed=3)
    for (am, bm), (alpha, beta) in zip(gr.MASK_PAIRS, [(1.0, 0.0), (-0.5, 2.0)] * 5):
        exact = gr.masked_product(A, B, am, bm, 0, alpha, beta, C0)
        assert exact.dtype == np.float64
        real = gr.masked_product(A.astype(np.float64), B.astype(np.float64), am, bm, 0, alpha, beta, C0.astype(np.float64))
        assert real.dtype == np.longdouble
        np.testing.assert_array_equal(exact.astype(np.longdouble), real)
    A, B, C0 = gr.exact_inputs(33, 33, 7, seed=4)
    for c_tri in (1, 2):
        got = gr.masked_product(A, B, 0, 0, c_tri, -1.0, 1.0, C0)
        sel = gr.selected(c_tri, 33, 33)
        np.testing.assert_array_equal(got[sel], (C0 - A @ B)[sel])
        np.testing.assert_array_equal(got[~sel], C0[~sel])


def test_hint_table_lists_the_documented_pairs():
    assert gr.legal_khi(1, 0) == [1] and gr.legal_klo(2, 0) == [1]
    assert gr.legal_khi(0, 1) == [2] and gr.legal_klo(0, 2) == [2]
    assert gr.legal_klo(2, 2) == [1, 2, 3] and gr.legal_khi(1, 1) == [1, 2]
    assert gr.legal_hints(0, 0) == []
    assert sorted(gr.legal_hints(1, 2)) == [(0, 1), (2, 0), (2, 1)]
    assert sum(len(gr.legal_hints(*p)) for p in gr.MASK_PAIRS) == 15


@pytest.mark.parametrize("tile", sorted(gr.TILES))
def test_legal_hints_change_nothing(tile):
    """Restricting every tile's sum to its hinted K range leaves the masked product as it is, for every legal (mask pair, hint)."""
    tm, tn = gr.TILES[tile]
    M, N, K = 3 * tm + 1, 2 * tn + 3, 3 * tm + 5
    A, B, _ = gr.exact_inputs(M, N, K, seed=5)
    for am, bm in gr.MASK_PAIRS:
        full = gr.hinted_product(A, B, am, bm, 0, 0, tm, tn)
        for klo, khi in gr.legal_hints(am, bm):
            np.testing.assert_array_equal(gr.hinted_product(A, B, am, bm, klo, khi, tm, tn), full, err_msg=str((am, bm, klo, khi)))


def test_illegal_hints_are_told_apart():
    """The table is not vacuous: a hint the masks do not cover drops terms."""
    A, B, _ = gr.exact_inputs(97, 70, 101, seed=6)
    full = gr.hinted_product(A, B, 0, 0, 0, 0, 32, 32)
    for klo, khi in [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2)]:
        assert not np.array_equal(gr.hinted_product(A, B, 0, 0, klo, khi, 32, 32), full)
    # the lower hint of A's mask is no hint for B's
    assert not np.array_equal(gr.hinted_product(A, B, 2, 0, 2, 0, 32, 32), gr.hinted_product(A, B, 2, 0, 0, 0, 32, 32))


def test_empty_ranges_lie_above_the_diagonal():
    for tile, (tm, tn) in gr.TILES.items():
        n = 3 * tm + 1
        e = gr.empty_range_tiles(2, 1, n, n, n, tm, tn)
        m0 = (np.arange(n) // tm * tm)[:, None]
        n0 = (np.arange(n) // tn * tn)[None, :]
        np.testing.assert_array_equal(e, n0 >= m0 + tm)
        assert e.any() and not gr.empty_range_tiles(0, 1, n, n, n, tm, tn).any()


def test_exact_inputs_stay_below_2_53():
    A, B, C0 = gr.exact_inputs(50, 40, 400, seed=7)
    assert A.dtype == np.int64 and np.abs(A).max() <= 3 and np.abs(B).max() <= 3 and np.abs(C0).max() <= 100
    assert A.min() == -3 and A.max() == 3 and C0.min() < -90 and C0.max() > 90
    for alpha, beta in [(1.0, 0.0), (-0.5, 2.0), (-1.0, 1.0)]:
        out = gr.masked_product(A, B, 0, 0, 0, alpha, beta, C0)
        assert np.abs(out).max() < 2.0 ** 53 and np.array_equal(out * 2, np.round(out * 2))
    # the helper refuses inputs whose sums could leave the exact range, and scalars that are not exact
    big = np.full((2, 2), 2 ** 27, dtype=np.int64)
    with pytest.raises(AssertionError):
        gr.masked_product(big, big, 0, 0, 0, 1.0, 0.0, np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(AssertionError):
        gr.masked_product(A, B, 0, 0, 0, 0.3, 0.0, C0)


def test_storage_windows():
    X = np.arange(15.0).reshape(3, 5)
    s = gr.Stored(X, np.nan)
    assert s.ld % 2 == 0 and s.ld >= 5 + 2 and s.COL0 % 2 == 0
    np.testing.assert_array_equal(s.window(), X)
    assert np.isnan(s.buf[s.guard_mask()]).all() and s.guard_mask().sum() == s.buf.size - 15
    assert np.isnan(s.buf[s.ROW0:s.ROW0 + 3, s.COL0 + 5]).all()        # what a 16-byte load across the end of a row reads
    assert s.buf.shape[0] - (s.ROW0 + 3) >= 2 and np.isnan(s.buf[s.ROW0 + 3:]).all()
    e = gr.Stored(np.zeros((4, 0)), np.nan)                                # K = 0: a 1-wide window of fill
    assert e.window().shape == (4, 1) and np.isnan(e.buf).all()
    a, b = gr.store_operands(np.zeros((6, 3)), np.zeros((3, 8)), "TN")
    assert a.window().shape == (3, 6) and b.window().shape == (3, 8)
    a, b = gr.store_operands(np.zeros((6, 3)), np.zeros((3, 8)), "NT")
    assert a.window().shape == (6, 3) and b.window().shape == (8, 3)
    c = gr.store_output(np.full((2, 2), np.nan))
    assert (c.buf[c.guard_mask()] == gr.SENTINEL).all()
    assert gr.same_bits(np.array([np.nan, 0.0]), np.array([np.nan, 0.0])) and not gr.same_bits(np.array([0.0]), np.array([-0.0]))

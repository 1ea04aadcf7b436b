"""The factorisation chain potrf -> trtri -> lauum at the sizes the leaf steps serve (N <= 513) against the long-double identities of
tests/factor_reference.py: the 128-row leaf (gpp_leaf_potrf_inv), the leaf-step chain (potrf_blk, potrf_blk_batched), the cooperative
panel (gpp_panel_potrf_inv) and the pair merges of trtri_level with the GEMM modes only they use.

Every comparison is |got - ref| <= bound elementwise, each step held to what the kernel itself wrote (``factor_reference.evaluate``):
no rtol, no condition number.  Operands are windows of NaN-filled buffers (row offset 1, column offset 2, an even leading dimension
larger than needed) or the package's own ``square_buffer`` with NaN in its padding; Kinv, which is only written, sits in a sentinel.
After every call the guards are bit-identical, the strict lower triangle of A still holds its NaN, and the inverse, pre-filled
with NaN like the scratch T, has no NaN left.  The last test prints, per driver and identity, the largest err / bound of the file.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_reference as fr  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = fr.cases()
MODES = ("window", "square")
#: "driver.identity" -> largest err / bound seen
RATIOS = {}
_matrices = {}


def _matrix(cls, N):
    """Each (class, N) matrix is built once per module."""
    if (cls, N) not in _matrices:
        _matrices[(cls, N)] = fr.matrix(cls, N)
    return _matrices[(cls, N)]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _upper_only(K):
    """K with NaN in the strict lower triangle: never to be read, never to be written."""
    K = np.array(K, dtype=np.float64)
    K[np.tril_indices(K.shape[0], -1)] = np.nan
    return K


class _Mat:
    """An N x N operand on the device inside its guard: 'window' = an interior window of a buffer of ``fill``; 'square' = the
    package's ``square_buffer``, whose padding columns hold ``fill``."""

    def __init__(self, X, fill, mode):
        from gpplus_amd.backend import square_buffer

        X = np.asarray(X, dtype=np.float64)
        self.N = N = X.shape[0]
        if mode == "square":
            self.win = square_buffer(N, "cuda")
            self.full = self.win._base if self.win._base is not None else self.win
            self.full.fill_(fill)
            self.win.copy_(_dev(X))
            self.r0 = self.c0 = 0
        else:
            w = fr.Window(X, fill)
            self.full = _dev(w.buf)
            self.win = w.window(self.full)
            self.r0, self.c0 = w.row0, w.col0
        assert self.win.data_ptr() % 16 == 0 and self.full.stride(0) % 2 == 0
        self.before = self.full.cpu().numpy().copy()
        self.guard = np.ones(self.before.shape, dtype=bool)
        self.guard[self.r0:self.r0 + N, self.c0:self.c0 + N] = False

    def read(self, what):
        now = self.full.cpu().numpy()
        assert fr.same_bits(now[self.guard], self.before[self.guard]), f"{what}: written outside its window"
        return now[self.r0:self.r0 + self.N, self.c0:self.c0 + self.N].copy()


def _record(driver, identity, err, bound, label):
    """Records err / bound, then asserts err <= bound elementwise (an entry whose bound is 0 must be exact)."""
    key = f"{driver}.{identity}"
    r = fr.ratio(err, bound)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    bad = ~(err <= bound)
    if bad.any():
        k = tuple(int(v) for v in np.argwhere(bad)[0])
        pytest.fail(f"{label}: {identity} entry {list(k)}: error {float(err[k]):.3e} against the bound {float(bound[k]):.3e} "
                    f"({int(bad.sum())} of {bad.size} entries outside, largest ratio {r:.3g})")


def _hold(driver, K, U, Xfull, Kinv, label, report=None):
    """Every identity of the driver's plan, the mirror and LAUUM, all on what the GPU wrote (reported under ``report``)."""
    N = K.shape[0]
    report = report or driver
    for it, err, bound in fr.evaluate(fr.plan(driver, N), K, U, Xfull):
        _record(report, it.identity, err, bound, f"{label} block [{it.r0}:{it.r1}, {it.c0}:{it.c1}]")
    assert fr.mirror_ok(Xfull), f"{label}: the strict upper triangle of the inverse is not the mirror of the lower one"
    _record(report, "lauum", *fr.lauum_check(Xfull, Kinv), label)


class _panel_option:
    """OPT_COOP_PANEL set for the block and put back after it (the context is session-scoped)."""

    def __init__(self, ctx, on):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        from gpplus_amd.backend import OPT_COOP_PANEL

        self.opt, self.old = OPT_COOP_PANEL, int(bool(self.ctx.coop_panel))
        self.ctx.set_option(self.opt, int(self.on))

    def __exit__(self, *exc):
        self.ctx.set_option(self.opt, self.old)


def _run_single(ctx, K, use_ws, mode, panel=False, expect_info=0):
    """potrf (with the scratch or without), trtri, lauum on guarded operands; returns (U, Xfull, Kinv, info)."""
    N = K.shape[0]
    nan = np.full((N, N), np.nan)
    dA, dL, dT = _Mat(_upper_only(K), np.nan, mode), _Mat(nan, np.nan, mode), _Mat(nan, np.nan, mode)
    dK = _Mat(np.full((N, N), fr.SENTINEL), fr.SENTINEL, mode)
    info = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ctx.potrf(dA.win, dL.win, info, dT.win if use_ws else None)
    got = int(info.item())
    if expect_info is not None:
        assert got == expect_info, f"info = {got}, expected {expect_info}"
    Ua = dA.read("A after potrf")
    assert np.isnan(Ua[np.tril_indices(N, -1)]).all(), "the strict lower triangle of A was written"
    after_potrf = dL.read("Linv after potrf")
    dT.read("T after potrf")
    ctx.trtri(dA.win, dL.win, dT.win)
    Xfull = dL.read("Linv after trtri")
    dT.read("T after trtri")
    assert fr.same_bits(dA.read("A after trtri"), Ua), "trtri changed A"
    if got == 0:
        assert not np.isnan(Xfull).any(), "trtri left (or read from T) a NaN in the inverse"
    if panel:
        assert fr.same_bits(after_potrf, Xfull), "the panel's inverse was not complete: trtri changed it"
    ctx.lauum(dL.win, dK.win)
    Kinv = dK.read("Kinv")
    assert fr.same_bits(dL.read("Linv after lauum"), Xfull), "lauum changed Linv"
    return np.triu(Ua), Xfull, Kinv, got


def _run_case(ctx, c, mode):
    K = _matrix(c.cls, c.N)
    with _panel_option(ctx, c.panel):
        U, Xfull, Kinv, _ = _run_single(ctx, K, c.use_ws, mode, c.panel)
    # (a single leaf is reported apart: one launch, no GEMM before lauum)
    _hold(c.driver, K, U, Xfull, Kinv, f"{c} {mode}", report="leaf" if c.N <= fr.NBLK else c.driver)


# ---- one leaf: every n = 1 .. 128 ----------------------------------------------------------------------------------------------
LEAF_WELL = [c for c in CASES if c.driver == "chain" and c.N <= fr.NBLK and c.cls == "well"]
LEAF_OTHER = [c for c in CASES if c.driver == "chain" and c.N <= fr.NBLK and c.cls != "well"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", range(8))
def test_one_leaf_every_size(gpu_ctx, chunk, mode):
    mine = LEAF_WELL[16 * chunk:16 * (chunk + 1)]
    assert len(mine) == 16
    for c in mine:
        _run_case(gpu_ctx, c, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cls", ("cov", "graded"))
def test_one_leaf_edges_on_the_other_classes(gpu_ctx, cls, mode):
    mine = [c for c in LEAF_OTHER if c.cls == cls]
    assert [c.N for c in mine] == list(fr.LEAF_EDGES)
    for c in mine:
        _run_case(gpu_ctx, c, mode)


# ---- the chain and the panel ---------------------------------------------------------------------------------------------------
BIG = [c for c in CASES if c.driver in ("chain", "panel") and c.N > fr.NBLK]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", BIG, ids=lambda c: f"{c.driver}-{c.N}-{c.cls}-ws{int(c.use_ws)}")
def test_chain_and_panel(gpu_ctx, case, mode):
    _run_case(gpu_ctx, case, mode)


# ---- batched -------------------------------------------------------------------------------------------------------------------
class _Slab:
    """B matrices, each a window (row 1, column 2) of its own slab of ``fill`` with an even stride."""

    def __init__(self, mats, fill):
        B, N = len(mats), mats[0].shape[0]
        self.N = N
        ld = N + (N & 1) + 4
        buf = np.full((B, N + 3, ld), fill)
        buf[:, 1:1 + N, 2:2 + N] = np.stack(mats)
        self.full = _dev(buf)
        self.win = self.full[:, 1:1 + N, 2:2 + N]
        assert self.win.stride(0) % 2 == 0 and self.win.stride(1) % 2 == 0 and self.win.data_ptr() % 16 == 0
        self.before = buf
        self.guard = np.ones(buf.shape, dtype=bool)
        self.guard[:, 1:1 + N, 2:2 + N] = False

    def read(self, what):
        now = self.full.cpu().numpy()
        assert fr.same_bits(now[self.guard], self.before[self.guard]), f"{what}: written outside its windows"
        return now[:, 1:1 + self.N, 2:2 + self.N].copy()


def _run_batched(ctx, Ks):
    """potrf_batched, trtri_batched, lauum_batched; returns (U, Xfull, Kinv, info), each with the batch in front."""
    B, N = len(Ks), Ks[0].shape[0]
    nan = [np.full((N, N), np.nan)] * B
    sA, sL, sT = _Slab([_upper_only(K) for K in Ks], np.nan), _Slab(nan, np.nan), _Slab(nan, np.nan)
    sK = _Slab([np.full((N, N), fr.SENTINEL)] * B, fr.SENTINEL)
    info = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ctx.potrf_batched(sA.win, sL.win, info)
    Ua = sA.read("A after potrf_batched")
    il = np.tril_indices(N, -1)
    assert np.isnan(Ua[:, il[0], il[1]]).all(), "the strict lower triangle of A was written"
    ctx.trtri_batched(sA.win, sL.win, sT.win)
    Xfull = sL.read("Linv after trtri_batched")
    sT.read("T after trtri_batched")
    assert fr.same_bits(sA.read("A after trtri_batched"), Ua), "trtri_batched changed A"
    ctx.lauum_batched(sL.win, sK.win)
    Kinv = sK.read("Kinv")
    assert fr.same_bits(sL.read("Linv after lauum_batched"), Xfull), "lauum_batched changed Linv"
    return np.triu(Ua), Xfull, Kinv, info.cpu().numpy()


@pytest.mark.parametrize("N", fr.BATCHED_SIZES)
def test_batched(gpu_ctx, N):
    mine = [c for c in CASES if c.driver == "batched" and c.N == N]
    assert len(mine) == fr.BATCH and len({c.cls for c in mine}) == fr.BATCH
    Ks = [_matrix(c.cls, N) for c in mine]
    U, Xfull, Kinv, info = _run_batched(gpu_ctx, Ks)
    assert (info == 0).all()
    assert not np.isnan(Xfull).any(), "trtri_batched left (or read from T) a NaN in the inverse"
    for b, c in enumerate(mine):
        _hold("batched", Ks[b], U[b], Xfull[b], Kinv[b], f"{c} element {b}")


# ---- the status word -----------------------------------------------------------------------------------------------------------
def _bad_minor(K, ps, value=None):
    """K with the leading minors ``ps`` (1-based, ascending) not positive definite while every smaller one stays so.  The diagonal
    entry is set through the Schur complement: A_pp = half of sum_j<p L_pj^2 of the factor so far, which leaves A_pp positive and the
    pivot at minus that half (p = 1 has no such sum: A_11 = -1).  ``value``: that diagonal entry instead (a NaN)."""
    K = np.array(K, dtype=np.float64)
    L = np.linalg.cholesky(K)  # (a second bad minor is placed as if the first were not there: only the first can be reported)
    for p in ps:
        q = p - 1
        s = float(L[q, :q] @ L[q, :q])
        if value is not None:
            K[q, q] = value
        elif q == 0:
            K[0, 0] = -1.0
        else:
            assert s > 1e-6
            K[q, q] = 0.5 * s
    return K


def _info_of(ctx, driver, K):
    if driver == "batched":
        N = K.shape[0]
        return int(_run_batched(ctx, [_matrix("cov", N), K, _matrix("graded", N)])[3][1])
    with _panel_option(ctx, driver == "panel"):
        return _run_single(ctx, K, driver == "panel", "window", expect_info=None)[3]


STATUS = [("chain", 300), ("panel", 300), ("batched", 130), ("batched", 300)]


@pytest.mark.parametrize("driver,N", STATUS)
def test_status_word_names_the_first_bad_minor(gpu_ctx, driver, N):
    K = _matrix("well", N)
    for p in (1, 16, 17, 128, 129, N):
        assert _info_of(gpu_ctx, driver, _bad_minor(K, [p])) == p, f"non-positive pivot at minor {p}"
    for p in (16, 129):
        assert _info_of(gpu_ctx, driver, _bad_minor(K, [p], np.nan)) == p, f"NaN on the diagonal at minor {p}"
    for p1, p2 in ((16, 17), (17, 129), (128, N)):
        assert _info_of(gpu_ctx, driver, _bad_minor(K, [p1, p2])) == p1, f"bad minors {p1} and {p2}"


@pytest.mark.parametrize("N", (130, 300))
def test_one_bad_element_leaves_the_rest_of_the_batch_alone(gpu_ctx, N):
    good = [_matrix(cls, N) for cls in fr.CLASSES]
    ref = _run_batched(gpu_ctx, good)
    assert (ref[3] == 0).all()
    for b in range(fr.BATCH):
        Ks = list(good)
        Ks[b] = _bad_minor(good[b], [129])
        got = _run_batched(gpu_ctx, Ks)
        assert [int(v) for v in got[3]] == [129 if e == b else 0 for e in range(fr.BATCH)]
        for e in range(fr.BATCH):
            if e != b:
                for name, x, y in zip(("U", "Linv", "Kinv"), got[:3], ref[:3]):
                    assert fr.same_bits(x[e], y[e]), f"element {e} beside a bad element {b}: {name} differs"


# ---- repeatability -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", fr.DRIVERS)
def test_same_bits_twice(gpu_ctx, driver):
    N = 385
    if driver == "batched":
        Ks = [_matrix(cls, N) for cls in fr.CLASSES]
        a, b = _run_batched(gpu_ctx, Ks), _run_batched(gpu_ctx, Ks)
    else:
        K = _matrix("cov", N)
        with _panel_option(gpu_ctx, driver == "panel"):
            a = _run_single(gpu_ctx, K, True, "window", driver == "panel")
            b = _run_single(gpu_ctx, K, True, "window", driver == "panel")
    for name, x, y in zip(("U", "Linv", "Kinv"), a[:3], b[:3]):
        assert fr.same_bits(x, y), f"{driver}: {name} differs between two runs"


def test_zz_report_largest_error_to_bound_ratios(gpu_ctx, capsys):
    """Runs last in the module: how much room the derived bounds leave on the hardware."""
    line = "factor conformance, largest err / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIOS.items()))
    with capsys.disabled():
        print("\n" + line)
    assert RATIOS and all(v <= 1.0 for v in RATIOS.values())

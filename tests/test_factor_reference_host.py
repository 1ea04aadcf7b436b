"""tests/factor_reference.py checked on the CPU: a fp64 emulation of each driver's operation order stays inside every bound on every
case; each of five mutations of that emulation is flagged; the plans cover every entry exactly once and the case list holds the sizes
the GPU suite is meant to run; and no bound is weaker than the tolerance the older factorisation tests apply to the same entry.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import factor_reference as fr  # noqa: E402

CASES = fr.cases()


def _plan_driver(driver):
    return "panel" if driver == "panel" else "chain"  # (the batched call runs the chain's steps: the same plan, the same emulation)


#: (plan driver, N, class), every one of the case list once
KEYS = sorted({(_plan_driver(c.driver), c.N, c.cls) for c in CASES}, key=lambda k: (k[1], k[0], k[2]))
_cache = {}


def _result(key):
    """The emulation of one case and everything the checkers say about it, computed once."""
    if key not in _cache:
        driver, N, cls = key
        A = fr.matrix(cls, N)
        U, Xfull, Kinv = fr.emulate(driver, A)
        res = fr.evaluate(fr.plan(driver, N), A, U, Xfull)
        _cache[key] = dict(A=A, U=U, X=Xfull, Kinv=Kinv, res=res, lauum=fr.lauum_check(Xfull, Kinv))
    return _cache[key]


def _worst(res, lauum=None):
    w = {}
    for it, err, bound in res:
        w[it.identity] = max(w.get(it.identity, 0.0), fr.ratio(err, bound))
    if lauum is not None:
        w["lauum"] = fr.ratio(*lauum)
    return w


def _groups():
    small = [k for k in KEYS if k[1] <= fr.NBLK]
    out = [small[i:i + 32] for i in range(0, len(small), 32)]
    for N in sorted({k[1] for k in KEYS if k[1] > fr.NBLK}):
        out.append([k for k in KEYS if k[1] == N])
    return out


GROUPS = _groups()


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"N{g[0][1]}-{g[-1][1]}")
def test_the_emulation_stays_inside_every_bound(group):
    for key in group:
        r = _result(key)
        assert fr.mirror_ok(r["X"])
        for identity, v in _worst(r["res"], r["lauum"]).items():
            assert v <= 1.0, f"{key}: {identity} err / bound = {v}"


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"N{g[0][1]}-{g[-1][1]}")
def test_no_weaker_than_the_existing_tolerances(group):
    """test_potrf_trtri_lauum holds every entry of the factor to 1e-10 max|L| and |Linv L - I| to 1e-8: every entry bound here is
    below the first, the residual the entry bounds of X imply below the second, and neither exceeds the figure the module records."""
    for key in group:
        r = _result(key)
        EU, EX = fr.entry_bounds(r["res"], r["U"])
        rel = float(EU.max() / np.abs(r["U"]).max())
        imp = float(fr.implied_inverse_residual(EX, r["U"]).max())
        assert rel < 1e-10 and imp < 1e-8, (key, rel, imp)
        assert rel <= fr.RECORDED_ENTRY_BOUND[key[2]] < 1e-10, (key, rel)
        assert imp <= fr.RECORDED_INVERSE_RESIDUAL[key[2]] < 1e-8, (key, imp)


def test_the_recorded_figures_are_the_measured_ones():
    """(after the two tests above have filled the cache: the recorded maxima are reached to within 10 %)"""
    for cls in fr.CLASSES:
        rel = imp = 0.0
        for key in KEYS:
            if key[2] == cls:
                r = _result(key)
                EU, EX = fr.entry_bounds(r["res"], r["U"])
                rel = max(rel, float(EU.max() / np.abs(r["U"]).max()))
                imp = max(imp, float(fr.implied_inverse_residual(EX, r["U"]).max()))
        assert 0.9 * fr.RECORDED_ENTRY_BOUND[cls] <= rel <= fr.RECORDED_ENTRY_BOUND[cls], (cls, rel)
        assert 0.9 * fr.RECORDED_INVERSE_RESIDUAL[cls] <= imp <= fr.RECORDED_INVERSE_RESIDUAL[cls], (cls, imp)


# ---- the checkers bite -----------------------------------------------------------------------------------------------------------
MUT_N = 300  # three leaves, the last ragged; a full pair and a ragged pair at s = 128, a ragged pair at s = 256; the panel's size range


def _flagged(driver, A, U, Xfull, Kinv):
    w = _worst(fr.evaluate(fr.plan(driver, A.shape[0]), A, U, Xfull), fr.lauum_check(Xfull, Kinv))
    return {k for k, v in w.items() if v > 1.0}


@pytest.mark.parametrize("driver", ("chain", "panel"))
def test_structural_mutations_are_flagged(driver):
    A = fr.matrix("well", MUT_N)
    assert not _flagged(driver, A, *fr.emulate(driver, A))
    # one 32-column strip of the rank-128 update behind leaf 0 skipped: the Schur complement of leaf 1 is wrong from column 160 on
    f = _flagged(driver, A, *fr.emulate(driver, A, {"skip_update": (0, 160)}))
    assert "factor_diag" in f or "factor_row" in f, f
    # one pivot reciprocal (pivot 5 of leaf 1) rounded through fp32
    f = _flagged(driver, A, *fr.emulate(driver, A, {"pivot_fp32": (1, 5)}))
    assert "factor_diag" in f, f
    # one 16 x 16 tile of one merge with the wrong sign: inside a leaf (level 32 of leaf 1), and in a merge of whole leaves
    f = _flagged(driver, A, *fr.emulate(driver, A, {"flip_tile": (128 + 48, 128)}))
    assert f == {"inv_merge_leaf"}, f
    U, Xfull, Kinv = fr.emulate(driver, A, {"flip_tile": (256 + 16, 32)})
    Kinv = np.tril(np.tril(Xfull).T @ np.tril(Xfull))  # (lauum of the mutated inverse: only the merge itself is wrong)
    f = _flagged(driver, A, U, Xfull, Kinv)
    assert f == {"inv_border" if driver == "panel" else "inv_merge_level"}, f


ENTRIES = {  # identity -> an entry it covers at MUT_N (row, column)
    "factor_diag": (130, 200), "factor_row": (5, 290), "inv_tile": (143, 130), "inv_merge_leaf": (299, 257),
    "inv_merge_level": (299, 3), "inv_border": (299, 3), "lauum": (200, 7)}


@pytest.mark.parametrize("driver", ("chain", "panel"))
def test_an_entry_moved_by_four_bounds_is_flagged(driver):
    A = fr.matrix("graded", MUT_N)
    U, Xfull, Kinv = fr.emulate(driver, A)
    pl = fr.plan(driver, MUT_N)
    res = fr.evaluate(pl, A, U, Xfull)
    EU, EX = fr.entry_bounds(res, U)
    Kb = fr.lauum_check(Xfull, Kinv)[1]
    for identity, (i, j) in ENTRIES.items():
        if identity not in {it.identity for it in pl.U + pl.X} | {"lauum"}:
            continue
        covering = [it for it in pl.U + pl.X if it.identity == identity and it.r0 <= i < it.r1 and it.c0 <= j < it.c1]
        assert identity == "lauum" or len(covering) == 1, identity
        U2, X2, K2 = U.copy(), Xfull.copy(), Kinv.copy()
        if identity == "lauum":
            K2[i, j] += 4 * float(Kb[i, j])
        elif identity.startswith("factor"):
            U2[i, j] += 4 * float(EU[i, j])
        else:
            X2[i, j] += 4 * float(EX[i, j])
            X2[j, i] = X2[i, j]
        assert (U2 != U).any() or (X2 != Xfull).any() or (K2 != Kinv).any()
        assert identity in _flagged(driver, A, U2, X2, K2), identity


def test_the_mirror_is_held_to_the_last_bit():
    A = fr.matrix("cov", 129)
    _, Xfull, _ = fr.emulate("chain", A)
    assert fr.mirror_ok(Xfull)
    X2 = Xfull.copy()
    X2[3, 128] = np.nextafter(X2[3, 128], np.inf)
    assert not fr.mirror_ok(X2)
    X2 = Xfull.copy()
    X2[0, 1] = -X2[0, 1] if X2[0, 1] == 0 else np.nextafter(X2[0, 1], 0)
    assert not fr.mirror_ok(X2)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_every_entry_is_covered_by_exactly_one_identity():
    for driver, N in sorted({(c.driver, c.N) for c in CASES}):
        pl = fr.plan(driver, N)
        assert (fr.coverage(pl.U, N) == np.triu(np.ones((N, N), dtype=np.int64))).all(), (driver, N)
        assert (fr.coverage(pl.X, N) == np.tril(np.ones((N, N), dtype=np.int64))).all(), (driver, N)
        kinds = {it.identity for it in pl.X}
        assert ("inv_border" in kinds) == (driver == "panel" and N > fr.NBLK)
        assert ("inv_merge_level" in kinds) == (driver != "panel" and N > fr.NBLK)


def test_the_plans_follow_the_drivers_block_boundaries():
    # 385: a full pair and a ragged pair (m2 = 1) at s = 128, a ragged pair at s = 256
    lv = [(it.s, it.r0, it.r1, it.c0, it.c1) for it in fr.plan("chain", 385).X if it.identity == "inv_merge_level"]
    assert lv == [(128, 128, 256, 0, 128), (128, 384, 385, 256, 384), (256, 256, 385, 0, 256)]
    # 513: a RUN of two full pairs at s = 128 (one batched launch), a full pair at s = 256, the ragged pair of s = 512
    lv = [(it.s, it.r0, it.r1, it.c0, it.c1) for it in fr.plan("batched", 513).X if it.identity == "inv_merge_level"]
    assert lv == [(128, 128, 256, 0, 128), (128, 384, 512, 256, 384), (256, 256, 512, 0, 256), (512, 512, 513, 0, 512)]
    # 129: the second leaf is one row: a ragged pair with m2 = 1, and a leaf of one tile of one row
    pl = fr.plan("chain", 129)
    assert [(it.r0, it.r1, it.c0, it.c1) for it in pl.X if it.identity == "inv_merge_level"] == [(128, 129, 0, 128)]
    assert [(it.identity, it.r0, it.r1) for it in pl.X if it.r0 >= 128 and it.c0 >= 128] == [("inv_tile", 128, 129)]
    # a leaf of 40 rows: tiles of 16, 16 and 8; the 16-merge of the first pair, none for the lone third tile; the ragged 32-merge
    lf = [(it.identity, it.r0, it.r1, it.c0, it.c1) for it in fr.plan("chain", 40).X]
    assert lf == [("inv_tile", 0, 16, 0, 16), ("inv_tile", 16, 32, 16, 32), ("inv_tile", 32, 40, 32, 40),
                  ("inv_merge_leaf", 16, 32, 0, 16), ("inv_merge_leaf", 32, 40, 0, 32)]
    # the panel borders by block rows of 128
    bd = [(it.r0, it.r1, it.c0, it.c1) for it in fr.plan("panel", 300).X if it.identity == "inv_border"]
    assert bd == [(128, 256, 0, 128), (256, 300, 0, 128), (256, 300, 128, 256)]


def test_the_case_list_holds_the_sizes_of_the_issue():
    def has(**kw):
        return any(all(getattr(c, k) == v for k, v in kw.items()) for c in CASES)

    for n in range(1, 129):
        assert has(driver="chain", N=n, cls="well", use_ws=False)
    for n in (1, 15, 16, 17, 63, 64, 65, 127, 128):
        assert has(driver="chain", N=n, cls="cov") and has(driver="chain", N=n, cls="graded")
    for N in (129, 143, 256, 257, 300, 384, 385, 513):
        assert has(driver="chain", N=N, use_ws=False, panel=False) and has(driver="chain", N=N, use_ws=True, panel=False)
    for N in (257, 300, 384, 385, 513):
        assert has(driver="panel", N=N, use_ws=True, panel=True)
    for N in (1, 16, 127, 129, 257, 385):
        assert {c.cls for c in CASES if c.driver == "batched" and c.N == N} == set(fr.CLASSES)
    assert max(c.N for c in CASES) == 513
    # every class meets the chain and the panel above one leaf
    for drv in ("chain", "panel"):
        assert {c.cls for c in CASES if c.driver == drv and c.N > fr.NBLK} == set(fr.CLASSES)
    # the matrices are seeded: the same bits every time
    assert fr.same_bits(fr.matrix("cov", 65), fr.matrix("cov", 65))

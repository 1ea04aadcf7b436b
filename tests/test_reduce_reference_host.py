"""The reference of tests/reduce_reference.py is checked before it judges a kernel (CPU only):

  values      ``grad_sums`` against torch fp64 autograd of sum_ij W_ij Ky_ij with W held constant; coincident rows;
  the bound   holds for plain fp64 numpy evaluations in three summation orders, and rejects every planted mistake evaluated in long
              double (the mistake is then its only error), for every case of the list the GPU file runs;
  coverage    of that list, and of the ``entries`` masks of the sharded modes.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_reference as rr  # noqa: E402

LD = rr.LD
CASES = rr.gradient_cases()
INSTANTIATIONS = sorted({rr.instantiation(c) for c in CASES})
#: fp64 evaluations in three orders are made for the cases up to this many N^2 D (the planted mistakes for all)
ORDERS_LIMIT = 128 * 128 * 33


def _case_inputs(c):
    inp = rr.gradient_inputs(c.N, c.D, c.seed, c.special, c.loo)
    grp, S = rr.noise_groups(c.smode, c.N, np.random.default_rng(c.seed + 5000))
    inp.update(grp=grp, S=S, Kl=rr.lower_only(inp["K"]))
    return inp


def _inside(got, ref, bound):
    """Elementwise |got - ref| <= bound over the four outputs -> {name: bool}."""
    return {n: bool(np.all(np.abs(np.asarray(getattr(got, n), dtype=LD) - getattr(ref, n)) <= getattr(bound, n)))
            for n in rr.GradSums._fields}


# ---- dense evaluation of one case, in any type and order ---------------------------------------------------------------------------
class Dense:
    """Every term of a case at once (N is small): ``sums`` adds them in long double for any multiplicity, weights and groups — the
    planted mistakes —, ``ordered_fp64`` in fp64 in a given order of the entries."""

    def __init__(self, c, inp, dt, d_split=None):
        self.c, self.N, self.dt = c, c.N, dt
        ds = c.d_split if d_split is None else d_split
        self.ut = rr.unit_terms(inp["U"], inp["w"], inp["sf2"], c.kind, ds, c.dU, 0, c.N, dt)
        self.W, _ = rr.weights(inp["alpha"], inp["Kl"], inp["beta"], 0, c.N, dt)
        self.m = rr.multiplicity(c.N, 0, c.N)
        self.grp, self.S = rr._groups(inp["grp"], c.N), inp["S"]

    def sums(self, m=None, W=None, rows=None, columns=True):
        """The sums over the entries of the rows ``rows`` (default: all), with multiplicity ``m`` and weights ``W`` of those rows."""
        rows = np.arange(self.N) if rows is None else np.asarray(rows)
        m = self.m[rows] if m is None else m
        W = self.W[rows] if W is None else W
        mw = m * W
        rc = mw[..., None] * self.ut["urow"][rows]
        g_U = -rc.sum(0) if columns else np.zeros((self.N, rc.shape[2]), self.dt)
        g_U[rows] += rc.sum(1)
        g_tau = np.zeros(self.S, self.dt)
        kept = m[np.arange(len(rows)), rows] > 0
        np.add.at(g_tau, self.grp[rows][kept], W[np.arange(len(rows)), rows][kept])
        return rr.GradSums(mw.reshape(-1) @ self.ut["uw"][rows].reshape(mw.size, -1), (mw * self.ut["kv"][rows]).sum(), g_tau, g_U)

    def ordered_fp64(self, order):
        """Sequential fp64 sums (cumsum) of the kept entries in the order ``order`` = (rows, columns) lists them; a row of g_U adds
        its N - 1 terms in the order the entries' partners appear in."""
        assert self.dt is np.float64
        i, j = order
        mw = (self.m * self.W)[i, j]
        g_sf2 = np.cumsum(mw * self.ut["kv"][i, j])[-1]
        g_w = np.cumsum(mw[:, None] * self.ut["uw"][i, j], axis=0)[-1]
        full = (self.m * self.W)[..., None] * self.ut["urow"]       # [i, j]: what entry (i, j) gives row i; minus that to row j
        full = full - np.transpose(full, (1, 0, 2))
        rank = np.empty((self.N, self.N), dtype=np.int64)
        rank[i, j] = np.arange(len(i))
        rank = np.where(np.tri(self.N, dtype=bool), rank, rank.T)   # position of the entry that pairs rows i and j
        cols = np.argsort(rank, axis=1)
        g_U = np.cumsum(np.take_along_axis(full, cols[..., None], axis=1), axis=1)[:, -1]
        d = np.arange(self.N)
        g_tau = np.array([np.cumsum(np.append(self.W[d, d][self.grp == s], 0.0))[-1] for s in range(self.S)])
        return rr.GradSums(g_w, g_sf2, g_tau, g_U)


def _orders(N, seed):
    i, j = np.tril_indices(N)
    yield "row-major", (i, j)
    # the kernel's: tile by tile; in a tile thread (ty, tx) owns rows 4 ty + 2 h + a and the column pairs of gpp_tile_col
    r, c = i % rr.TILE, j % rr.TILE
    ti, tj = i // rr.TILE, j // rr.TILE
    tx, b = (c % 32) // 2, (c % 2) + 2 * (c // 32)
    assert np.array_equal(rr.tile_col(2 * tx, b), c)
    key = np.lexsort((b, r % 2, (r % 4) // 2, tx, r // 4, ti * (ti + 1) // 2 + tj))
    yield "tiles", (i[key], j[key])
    p = np.random.default_rng(seed).permutation(len(i))
    yield "random", (i[p], j[p])


# ---- planted mistakes ----------------------------------------------------------------------------------------------------------------
def _plus(x, y, sign=1):
    return rr.GradSums(*(p + sign * q for p, q in zip(x, y)))


def _mistakes(c, inp, dense, base):
    """(name, sums with the mistake) for every mistake the case can show; the rules that skip one are written out here.  The sums
    are linear in the entries: a mistake that touches one row is ``base``, the sums of the case, plus the difference of that row."""
    N, last = c.N, c.N - 1
    distinct = not (c.special and N == 2)           # rule: the special rows of N = 2 are one point twice: every difference is 0
    row = dense.sums(rows=[last])
    only = np.zeros((1, N), dtype=np.int64)
    only[0, last] = 1                               # the last entry of the last diagonal tile, ragged unless 64 divides N
    yield "entry dropped", _plus(base, dense.sums(m=only, rows=[last]), -1)
    yield "diagonal weighted 2", base._replace(g_sf2=base.g_sf2 + np.trace(dense.W))  # (the other terms of the diagonal are 0)
    # the entry below the diagonal with the largest kernel value takes the value stored above the diagonal: any other number
    kv = np.where(np.tri(N, k=-1, dtype=bool), dense.ut["kv"], -1)
    i, j = np.unravel_index(np.argmax(kv), kv.shape)
    Kl = inp["Kl"].copy()
    Kl[i, j] = inp["K"][i, j] + 1.0
    dW = rr.weights(inp["alpha"], Kl, inp["beta"], 0, N)[0][[i]] - dense.W[[i]]
    yield "read above the diagonal", _plus(base, dense.sums(W=dW, rows=[i])._replace(g_tau=0 * base.g_tau))
    if c.kind != 0 and distinct:                    # rule: kind 0 never reads d_split
        moved = c.d_split + 1 if c.d_split < c.D else c.d_split - 1
        yield "feature across d_split", Dense(c, inp, LD, d_split=moved).sums()
    yield "last row omitted", _plus(base, row, -1)
    if c.dU > 0 and distinct:                       # rule: without feature gradients there is no column contribution
        yield "column contribution omitted", base._replace(g_U=dense.sums(columns=False).g_U)
    if inp["S"] > 1:                                # rule: a single noise level has no neighbouring group
        g_tau = base.g_tau.copy()
        g_tau[dense.grp[last]] -= dense.W[last, last]
        g_tau[(dense.grp[last] + 1) % inp["S"]] += dense.W[last, last]
        yield "W_ii in the neighbouring group", base._replace(g_tau=g_tau)


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda t: "DT%d-MAT%d-HASU%d-LOO%d" % t)
def test_bound_holds_and_bites(inst):
    for c in (c for c in CASES if rr.instantiation(c) == inst):
        inp = _case_inputs(c)
        args = (inp["U"], inp["w"], inp["sf2"], inp["grp"], inp["S"], c.kind, c.d_split, inp["alpha"], inp["Kl"], c.dU)
        ref, bound = rr.grad_sums_and_bound(*args, beta=inp["beta"])
        for x in ref + bound:
            assert np.all(np.isfinite(x)), c
        dense = Dense(c, inp, LD)
        # the blockwise and the dense evaluation are two summation orders of long double: 2^-64 n of the magnitudes, far inside
        base = dense.sums()
        assert all(_inside(base, ref, rr.GradSums(*(b * LD(1e-3) for b in bound))).values()), c
        if c.N * c.N * c.D <= ORDERS_LIMIT:
            d64 = Dense(c, inp, np.float64)
            for name, order in _orders(c.N, c.seed):
                ok = _inside(d64.ordered_fp64(order), ref, bound)
                assert all(ok.values()), (c, name, ok)
        if c.N < 2:
            continue
        for name, wrong in _mistakes(c, inp, dense, base):
            ok = _inside(wrong, ref, bound)
            assert not all(ok.values()), (c, name)


# ---- the case list -----------------------------------------------------------------------------------------------------------------
def test_case_list_coverage():
    assert len(CASES) <= 300 and len(INSTANTIATIONS) == 32
    by_inst = {t: [c for c in CASES if rr.instantiation(c) == t] for t in INSTANTIATIONS}
    for (dt, mat, hasu, loo), cs in by_inst.items():
        assert {c.N for c in cs} == set(rr.SIZES)
        assert {c.D for c in cs} == set(rr.FEATURES[dt])
        assert {c.smode for c in cs} == set(rr.SMODES) and {c.ld for c in cs} == set(rr.LDS)
        assert {c.special for c in cs} == {False, True}
        if hasu:
            assert any(c.dU == c.D > 1 for c in cs) and any(c.dU == 1 < c.D for c in cs)
        else:
            assert {c.dU for c in cs} == {0}
        if mat:
            assert {c.kind for c in cs} == {1, 2}
            big = [c for c in cs if c.D >= 3]
            assert any(c.d_split == 0 for c in cs) and any(c.d_split == c.D for c in cs)      # all Matern, all RBF under a Matern kind
            assert any(c.d_split == 1 for c in big) and any(c.d_split == c.D - 1 for c in big)  # mixed, at both ends
        else:
            assert {c.kind for c in cs} == {0}
    for N in rr.SIZES:  # every size meets feature gradients under all three kinds
        assert {c.kind for c in CASES if c.N == N and c.dU > 0} == {0, 1, 2}, N
    assert {c.kind for c in CASES if c.special and c.N >= 67} == {0, 1, 2}
    # both load paths of Kinv occur under both leading dimensions, and the tightest rows put the last tile column on the scalar one
    for c in CASES:
        if c.ld == "min" and c.N % rr.TILE not in (0, rr.TILE - 1):
            assert "scalar" in rr.kinv_load_paths(c.N, rr.even_ld(c.N))
    assert any(rr.kinv_load_paths(c.N, rr.even_ld(c.N)) == {"vector"} for c in CASES if c.ld == "min")


# ---- values ------------------------------------------------------------------------------------------------------------------------
def _ky(U, w, sf2, tau, grp, kind, d_split):
    """Ky in torch fp64, differentiable; the diagonal's distance is cut out before the square root (its derivative there is not
    finite), which is also why this check has no coincident rows."""
    D = U.shape[1]
    dsp = rr.split_of(kind, d_split, D)
    d2 = (U[:, None, :] - U[None, :, :]) ** 2 * w
    r2, r2m = d2[..., :dsp].sum(-1), d2[..., dsp:].sum(-1)
    k = torch.exp(-r2)
    if kind != 0 and dsp < D:
        eye = torch.eye(U.shape[0], dtype=torch.bool)
        r = torch.sqrt((6.0 if kind == 1 else 10.0) * torch.where(eye, torch.ones_like(r2m), r2m))
        h = (1 + r) * torch.exp(-r) if kind == 1 else (1 + r + r * r / 3) * torch.exp(-r)
        k = k * torch.where(eye, torch.ones_like(h), h)
    return sf2 * k + torch.diag(tau[grp])


@pytest.mark.parametrize("kind", (0, 1, 2))
@pytest.mark.parametrize("split", ("0", "1", "D"))
@pytest.mark.parametrize("loo", (False, True))
def test_values_against_autograd(kind, split, loo):
    N, D, S = 41, 4, 3
    d_split = {"0": 0, "1": 1, "D": D}[split]
    inp = rr.gradient_inputs(N, D, 77 + 10 * kind + d_split, False, loo)
    grp = np.random.default_rng(3).integers(0, S, N).astype(np.int32)
    Kl = rr.lower_only(inp["K"])
    args = (inp["U"], inp["w"], inp["sf2"], grp, S, kind, d_split, inp["alpha"], Kl, D)
    ref, bound = rr.grad_sums_and_bound(*args, beta=inp["beta"])
    a, K = inp["alpha"], inp["K"]
    W = 0.5 * (np.outer(a, a) - K) if not loo else -0.5 * (np.outer(a, inp["beta"]) + np.outer(inp["beta"], a)) - K
    U, w = (torch.tensor(inp[k], requires_grad=True) for k in ("U", "w"))
    sf2 = torch.tensor(inp["sf2"], dtype=torch.float64, requires_grad=True)
    tau = torch.full((S,), 0.1, dtype=torch.float64, requires_grad=True)
    (torch.tensor(W) * _ky(U, w, sf2, tau, torch.tensor(grp, dtype=torch.long), kind, d_split)).sum().backward()
    got = rr.GradSums(w.grad.numpy(), sf2.grad.numpy(), tau.grad.numpy(), U.grad.numpy())
    # autograd is one more fp64 evaluation (of the symmetric sum: both halves of every pair, twice the roundings at most)
    ok = _inside(got, ref, rr.GradSums(*(2 * b for b in bound)))
    assert all(ok.values()), ok


@pytest.mark.parametrize("kind", (1, 2))
def test_coincident_rows_are_finite_and_at_their_limits(kind):
    """r = 0 off the diagonal: h = 1 and dh / d r2_mat = -3 resp. -5/3 (gpp_internal.h), no division by r."""
    kv, kd, r, p, dp = rr.kernel_factors(kind, LD(0.25), LD(0))
    assert r == 0 and kv == np.exp(LD(-0.25)) and kd == (3 if kind == 1 else LD(5) / 3) * np.exp(LD(-0.25))
    U = np.array([[0.3, -1.2, 0.5], [0.3, -1.2, 0.5], [0.9, 0.1, 0.5]])  # rows 0 and 1 coincide; row 2 shares the Matern feature 2
    w, sf2, alpha = np.array([0.7, 1.1, 0.4]), 1.3, np.array([0.5, -1.0, 2.0])
    K = rr.lower_only(np.array([[1.0, 0, 0], [0.2, 2.0, 0], [-0.4, 0.6, 3.0]]))
    out = rr.grad_sums(U, w, sf2, None, 1, kind, 2, alpha, K, 3)
    assert all(np.all(np.isfinite(x)) for x in out)
    W = (np.outer(alpha.astype(LD), alpha.astype(LD)) - np.nan_to_num(K)) / 2
    # rows 0, 1 against row 2: RBF features only, r = 0, h = 1
    e = np.exp(-(LD(w[0]) * (LD(U[2, 0]) - LD(U[0, 0])) ** 2 + LD(w[1]) * (LD(U[2, 1]) - LD(U[0, 1])) ** 2))
    want = LD(W[0, 0]) + W[1, 1] + W[2, 2] + 2 * LD(W[1, 0]) + 2 * (LD(W[2, 0]) + W[2, 1]) * e
    assert abs(out.g_sf2 - want) <= 1e-17 * abs(want)
    assert out.g_w[2] == 0 and np.all(out.g_U[:, 2] == 0) and np.all(out.g_U[0] == out.g_U[0]) and out.g_w[0] != 0


# ---- partial sums ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_cols", (False, True))
@pytest.mark.parametrize("nranks,nb,N", [(2, 64, 129), (3, 64, 191), (2, 128, 257), (3, 128, 129), (3, 128, 257)])
def test_partials_partition_and_add_up(by_cols, nranks, nb, N):
    masks = [rr.shard_entries(N, nb, r, nranks, by_cols) for r in range(nranks)]
    assert np.array_equal(sum(m.astype(int) for m in masks), np.tri(N, dtype=int))
    D, S, dU = 3, 3, 2
    inp = rr.gradient_inputs(N, D, 900 + N + nb, True, False)
    grp, _ = rr.noise_groups("gap", N, np.random.default_rng(N))
    args = (inp["U"], inp["w"], inp["sf2"], grp, S, 2, 1, inp["alpha"], rr.lower_only(inp["K"]), dU)
    full, bound = rr.grad_sums_and_bound(*args)
    parts = [rr.grad_sums_and_bound(*args, entries=m) for m in masks]
    total = rr.GradSums(*(sum(p[0][k] for p in parts) for k in range(4)))
    assert all(_inside(total, full, rr.GradSums(*(b * LD(1e-3) for b in bound))).values())   # long-double rounding only
    for k in range(4):  # the partial bounds are bounds of parts of the same sums
        assert np.all(sum(p[1][k] for p in parts) <= bound[k] * (1 + LD(1e-9)) + 0)
    # teeth: the last diagonal tile handed to the next rank
    t0 = (N - 1) // rr.TILE * rr.TILE
    owner = ((t0 // nb) % nranks)
    wrong = masks[owner].copy()
    wrong[t0:, t0:] = False
    got = rr.grad_sums(*args, entries=wrong)
    assert not all(_inside(got, *parts[owner]).values())
    other = (owner + 1) % nranks
    wrong = masks[other].copy()
    wrong[t0:, t0:] = np.tri(N - t0, dtype=bool)
    assert not all(_inside(rr.grad_sums(*args, entries=wrong), *parts[other]).values())


# ---- vector reductions -------------------------------------------------------------------------------------------------------------
def _seq(terms, order):
    return np.cumsum(np.append(terms[order], 0.0))[-1]


def _three_orders(n, seed):
    return [np.arange(n), np.arange(n)[::-1], np.random.default_rng(seed).permutation(n)]


@pytest.mark.parametrize("N", (1, 2, 3, 64, 129, 257))
def test_vector_bounds_hold_and_bite(N):
    rng = np.random.default_rng(N)
    T, x = rng.standard_normal((N, N)), rng.standard_normal(N)
    for fn, low in ((rr.trmv_lower, True), (rr.trmv_upper, False)):
        ref, bound = fn(T, x)
        for i in range(N):
            k = np.arange(0, i + 1) if low else np.arange(i, N)
            for o in _three_orders(len(k), i):
                assert abs(_seq(T[i, k] * x[k], o) - ref[i]) <= bound[i]
        if N >= 2:
            # teeth: the other triangle's neighbour of the diagonal joins the sum; the last term of the longest row is dropped
            i = 0 if low else N - 1
            extra = T[i, 1] * x[1] if low else T[i, N - 2] * x[N - 2]
            assert abs(extra) > bound[i]
            i = N - 1 if low else 0
            assert abs(LD(T[i, N - 1]) * x[N - 1]) > bound[i]
    # mll_scalars
    diag, z = 10.0 ** rng.uniform(-8, 3, N), rng.standard_normal(N)
    ref, bound = rr.mll_scalars(diag, z)
    for o in _three_orders(N, N):
        q, l = _seq(z * z, o), 2.0 * _seq(np.log(diag), o)
        got = np.array([q, l, -0.5 * (q + l + N * 1.8378770664093454835606594728112)])
        assert np.all(np.abs(got - ref) <= bound), (got, ref, bound)
    assert abs(ref[2] + (ref[0] + ref[1] + N * np.log(2 * LD(np.pi))) / 2) <= 1e-15 * N   # the N log 2 pi term is in (pi in fp64)
    k = np.argmax(np.abs(np.log(diag)))
    wrong = rr.mll_scalars(np.where(np.arange(N) == k, 1.0, diag), z)[0]                  # the largest logarithm dropped
    assert abs(wrong[1] - ref[1]) > bound[1] and abs(wrong[2] - ref[2]) > bound[2]
    assert np.abs(rr.mll_scalars(diag, np.append(z[:-1], 0.0))[0] - ref)[0] > bound[0]   # the last z dropped
    # predict_rows
    M = 5
    Ksn, V, kss = rng.standard_normal((M, N)), rng.standard_normal((M, N)), rng.uniform(1, 2, M) + N
    (mean, var), (bmean, bvar) = rr.predict_rows(Ksn, V, x, kss)
    for a in range(M):
        for o in _three_orders(N, a):
            assert abs(_seq(Ksn[a] * x, o) - mean[a]) <= bmean[a]
            assert abs((kss[a] - _seq(V[a] * V[a], o)) - var[a]) <= bvar[a]
    assert rr.predict_rows(Ksn, None, x, None)[0][1] is None
    (m2, v2), _ = rr.predict_rows(Ksn[:, ::-1], V[:, :N - 1] if N > 1 else 0 * V, x, kss)  # alpha reversed; the last column of V dropped
    assert np.all(np.abs(v2 - var) > bvar) and (N == 1 or np.any(np.abs(m2 - mean) > bmean))


def test_windows():
    X = np.arange(15.0).reshape(3, 5)
    for kw in (dict(), dict(ld=rr.even_ld(5), col0=0)):
        wdw = rr.Window(X, np.nan, **kw)
        assert np.array_equal(wdw.window(), X) and wdw.ld % 2 == 0 and (wdw.row0 * wdw.ld + wdw.col0) % 2 == 0
        assert np.isnan(wdw.buf[wdw.guard_mask()]).all() and wdw.guard_mask().sum() == wdw.buf.size - 15
    v = rr.VectorWindow(6, rr.SENTINEL, shape=(3, 2))
    assert v.window().shape == (3, 2) and (v.buf == rr.SENTINEL).all() and v.guard_mask().sum() == v.buf.size - 6
    assert np.isnan(rr.lower_only(X[:, :3])[0, 1]) and rr.lower_only(X[:, :3])[2, 1] == X[2, 1]

"""The HBM-bound reductions of the training path (gpp_reduce.hip: gpp_grad_tiles and its finish kernels, the two trmv kernels,
gpp_mll_scalars, gpp_predict_rows) against the long-double reference of tests/reduce_reference.py.

Every comparison is |got - ref| <= bound elementwise, the bound derived in ``reduce_reference.grad_bound`` & co.: no rtol.  Inputs are
random, with no factorisation anywhere: the matrix in the place of Ky^-1 is stored lower-triangle-only with NaN above the diagonal and
in all padding (the 16-byte loads fetch such entries; the j <= i branch must discard them), outputs are windows of sentinel-filled
buffers whose guards are checked, and the context's workspace holds the NaN bit pattern before each unsharded call (every slot of
it that is read must have been written).  The last test prints, per output, the largest err / bound of the file.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu

LD = rr.LD
CASES = rr.gradient_cases()
INSTANTIATIONS = sorted({rr.instantiation(c) for c in CASES})
CHUNK = 3  # calls per parameter
#: output -> largest err / bound seen
RATIOS = {}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _compare(name, got, ref, bound, label):
    """Records err / bound, then asserts |got - ref| <= bound elementwise (an entry whose bound is 0 must be exact)."""
    got, ref, bound = (np.atleast_1d(np.asarray(x, dtype=LD)) for x in (got, ref, bound))
    err = np.abs(got - ref)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max(initial=0)) if np.isfinite(err).all() else float("inf")
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    bad = ~(err <= bound)
    if bad.any():
        k = tuple(int(v) for v in np.argwhere(bad)[0])
        pytest.fail(f"{label}: {name}{list(k)} = {float(got[k])!r}, reference {float(ref[k])!r}: error {float(err[k]):.3e} against the "
                    f"bound {float(bound[k]):.3e} ({int(bad.sum())} of {bad.size} entries outside, largest ratio {ratio:.3g})")


def _poison_workspace(ctx, N, D, S, batch=0):
    from gpplus_amd.backend import OP_MLL_EVAL

    if batch:
        ctx.ensure_workspace_batched(batch, N, D, S)
    else:
        ctx.ensure_workspace(OP_MLL_EVAL, N, 0, D, S)
    ctx._ws.fill_(0xFF)  # every double of it is the NaN 0xFFFFFFFFFFFFFFFF


class _Out:
    """An output vector (or contiguous matrix) on the device inside its sentinel guard."""

    def __init__(self, n, shape=None):
        self.vw = rr.VectorWindow(n, rr.SENTINEL, shape=shape)
        self.dev = _dev(self.vw.buf)
        self.t = self.vw.window(self.dev)

    def read(self, what):
        out = self.dev.cpu().numpy()
        g = self.vw.guard_mask()
        assert rr.same_bits(out[g], self.vw.buf[g]), f"{what}: written outside its window"
        return self.vw.window(out).copy()


class _GradOut:
    def __init__(self, N, D, S, dU):
        self.g_w, self.g_sf2, self.g_tau = _Out(D), _Out(1), _Out(S)
        self.g_U = _Out(N * dU, shape=(N, dU)) if dU else None

    def tensors(self):
        return self.g_w.t, self.g_sf2.t, self.g_tau.t, None if self.g_U is None else self.g_U.t

    def read(self):
        return rr.GradSums(self.g_w.read("g_w"), self.g_sf2.read("g_sf2")[0], self.g_tau.read("g_tau"),
                           None if self.g_U is None else self.g_U.read("g_U"))


def _compare_grad(got, ref, bound, label, prefix="grad"):
    for n in rr.GradSums._fields:
        if getattr(got, n) is not None:
            _compare(f"{prefix}.{n}", getattr(got, n), getattr(ref, n), getattr(bound, n), label)


def _stored_kinv(Kl, ld_mode):
    """The lower-triangle-only matrix inside a NaN buffer: 'min' = the smallest even leading dimension, 'pad' = the one of
    ``square_buffer`` (both with the window at column 0, as the package stores it), None = an interior window."""
    from gpplus_amd.backend import row_stride

    N = Kl.shape[0]
    if ld_mode is None:
        return rr.Window(Kl, np.nan)
    return rr.Window(Kl, np.nan, ld=rr.even_ld(N) if ld_mode == "min" else row_stride(N), col0=0)


def _run_single(ctx, inp, grp, S, kind, d_split, dU, stored, poison=True):
    """grad_reduce, or loo_grad_reduce when the inputs carry beta; returns the outputs read back."""
    N, D = inp["U"].shape
    out = _GradOut(N, D, S, dU)
    Kd = stored.window(_dev(stored.buf))
    dsf2 = torch.tensor([inp["sf2"]], dtype=torch.float64, device="cuda")
    dgrp = None if grp is None else _dev(grp)
    if poison:
        _poison_workspace(ctx, N, D, S)
    if inp["beta"] is None:
        ctx.grad_reduce(_dev(inp["U"]), _dev(inp["w"]), dsf2, dgrp, S, _dev(inp["alpha"]), Kd, dU, *out.tensors(), kind=kind,
                        d_split=d_split)
    else:
        ctx.loo_grad_reduce(_dev(inp["U"]), _dev(inp["w"]), dsf2, dgrp, S, _dev(inp["alpha"]), _dev(inp["beta"]), Kd, dU,
                            *out.tensors(), kind=kind, d_split=d_split)
    return out.read()


# ---- the gradient family, one call per (instantiation, size) -------------------------------------------------------------------------
@pytest.mark.parametrize("inst,chunk", [(t, k) for t in INSTANTIATIONS for k in range(len(rr.SIZES) // CHUNK)],
                         ids=lambda v: "DT%d-MAT%d-HASU%d-LOO%d" % v if isinstance(v, tuple) else str(v))
def test_grad_reduce_cases(gpu_ctx, inst, chunk):
    from gpplus_amd.backend import row_stride

    mine = [c for c in CASES if rr.instantiation(c) == inst][CHUNK * chunk:CHUNK * (chunk + 1)]
    assert len(mine) == CHUNK
    for c in mine:
        inp = rr.gradient_inputs(c.N, c.D, c.seed, c.special, c.loo)
        grp, S = rr.noise_groups(c.smode, c.N, np.random.default_rng(c.seed + 5000))
        Kl = rr.lower_only(inp["K"])
        stored = _stored_kinv(Kl, c.ld)
        # which loads the last tile column takes: the two 16-byte ones only when the row reaches 64 columns past its first
        tiles = (c.N + rr.TILE - 1) // rr.TILE
        ld = rr.even_ld(c.N) if c.ld == "min" else row_stride(c.N)
        assert stored.ld == ld and ("scalar" in rr.kinv_load_paths(c.N, ld)) == (ld < rr.TILE * tiles)
        assert ("vector" in rr.kinv_load_paths(c.N, ld)) == (tiles > 1 or ld >= rr.TILE)
        got = _run_single(gpu_ctx, inp, grp, S, c.kind, c.d_split, c.dU, stored)
        ref, bound = rr.grad_sums_and_bound(inp["U"], inp["w"], inp["sf2"], grp, S, c.kind, c.d_split, inp["alpha"], Kl, c.dU,
                                            beta=inp["beta"])
        _compare_grad(got, ref, bound, str(c))


# ---- the grid-stride loop: 2145 tiles on 2048 work-groups ------------------------------------------------------------------------
_large = {}


def _large_case(loo):
    """N = 4097 is the smallest size at which a work-group owns two tiles.  The inputs, and each reference, are computed once."""
    if not _large:
        N, D = 4097, 2
        inp = rr.gradient_inputs(N, D, 4097, False, True)
        grp, S = rr.noise_groups("gap", N, np.random.default_rng(4097))
        Kl = rr.lower_only(inp["K"])
        _large.update(inp=inp, grp=grp, S=S, Kl=Kl, stored=_stored_kinv(Kl, None))
    if loo not in _large:
        inp = _large["inp"]
        _large[loo] = rr.grad_sums_and_bound(inp["U"], inp["w"], inp["sf2"], _large["grp"], _large["S"], 2, 1, inp["alpha"],
                                             _large["Kl"], 2, beta=inp["beta"] if loo else None, rows=128)
    return _large


@pytest.mark.parametrize("loo", (False, True), ids=("grad_reduce", "loo_grad_reduce"))
def test_grad_reduce_two_tiles_per_work_group(gpu_ctx, loo):
    L = _large_case(loo)
    inp = dict(L["inp"], beta=L["inp"]["beta"] if loo else None)
    got = _run_single(gpu_ctx, inp, L["grp"], L["S"], 2, 1, 2, L["stored"])
    _compare_grad(got, *L[loo], f"N = 4097 loo = {loo}", prefix="grad4097")


# ---- batched: the same kernel, the same grid, the same order -------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 65, 129))
@pytest.mark.parametrize("shared_U", (True, False))
@pytest.mark.parametrize("loo", (False, True))
def test_grad_reduce_batched_is_the_single_call_bit_for_bit(gpu_ctx, N, shared_U, loo):
    B, D, dU, kind, d_split = 3, 3, 2, 2, 1
    inps = [rr.gradient_inputs(N, D, 7000 + 10 * N + b, b == 1, loo) for b in range(B)]
    if shared_U:
        for p in inps:
            p["U"] = inps[0]["U"]
    grp, S = rr.noise_groups("gap", N, np.random.default_rng(N))
    ld = rr.even_ld(N) + 2
    # B matrices, each a window (rows 1 .. N) of its own NaN slab
    slab = np.full((B, N + 3, ld), np.nan)
    for b, p in enumerate(inps):
        slab[b, 1:1 + N, :N] = rr.lower_only(p["K"])
    dK = _dev(slab)[:, 1:1 + N, :N]
    sv = N + (N & 1) + 2                                   # a padded, even stride
    def vec(key):
        v = np.full((B, sv), np.nan)
        for b, p in enumerate(inps):
            v[b, :N] = p[key]
        return _dev(v)[:, :N]
    dU_all = _dev(inps[0]["U"]) if shared_U else _dev(np.stack([p["U"] for p in inps]))
    dw, dsf2 = _dev(np.stack([p["w"] for p in inps])), _dev(np.array([p["sf2"] for p in inps]))
    dgrp = _dev(grp)
    outs = _Out(B * D, (B, D)), _Out(B), _Out(B * S, (B, S)), _Out(B * N * dU, (B, N, dU))
    _poison_workspace(gpu_ctx, N, D, S, batch=B)
    if loo:
        gpu_ctx.loo_grad_reduce_batched(dU_all, dw, dsf2, dgrp, S, vec("alpha"), vec("beta"), dK, dU, *(o.t for o in outs), kind=kind,
                                        d_split=d_split)
    else:
        gpu_ctx.grad_reduce_batched(dU_all, dw, dsf2, dgrp, S, vec("alpha"), dK, dU, *(o.t for o in outs), kind=kind, d_split=d_split)
    bw, bs, bt, bU = (o.read(n) for o, n in zip(outs, rr.GradSums._fields))
    for b, p in enumerate(inps):
        Kl = rr.lower_only(p["K"])
        one = _run_single(gpu_ctx, p, grp, S, kind, d_split, dU, rr.Window(Kl, np.nan, ld=ld, col0=0))
        ref, bound = rr.grad_sums_and_bound(p["U"], p["w"], p["sf2"], grp, S, kind, d_split, p["alpha"], Kl, dU, beta=p["beta"])
        _compare_grad(one, ref, bound, f"element {b} alone", prefix="batched")
        for name, x, y in zip(rr.GradSums._fields, (bw[b], bs[b], bt[b], bU[b]), one):
            assert rr.same_bits(x, y), f"element {b}: {name} of the batched call differs from the single call: {x!r} {y!r}"


# ---- sharded: every rank's partial sums ----------------------------------------------------------------------------------------------
def _compact(Kl, N, nb, rank, nranks):
    """Only the owned column blocks, side by side (at least two columns: the pointer must be valid where a rank owns nothing)."""
    blocks = [Kl[:, b * nb:min(N, (b + 1) * nb)] for b in range(rank, (N + nb - 1) // nb, nranks)]
    own = np.concatenate(blocks, axis=1) if blocks else np.empty((N, 0))
    out = np.full((N, max(own.shape[1], 2)), np.nan)
    out[:, :own.shape[1]] = own
    return out


@pytest.mark.parametrize("N", (129, 191, 257))
@pytest.mark.parametrize("nb", (64, 128))
@pytest.mark.parametrize("nranks", (2, 3))
def test_grad_reduce_sharded_partials_per_rank(gpu_ctx, N, nb, nranks):
    D, dU, kind, d_split = 3, 2, 2, 1
    inp = rr.gradient_inputs(N, D, 9000 + N + nb + nranks, True, False)
    grp, S = rr.noise_groups("gap", N, np.random.default_rng(N))
    Kl = rr.lower_only(inp["K"])
    dsf2 = torch.tensor([inp["sf2"]], dtype=torch.float64, device="cuda")
    dev = [_dev(inp[k]) for k in ("U", "w")] + [dsf2, _dev(grp), S, _dev(inp["alpha"])]
    for by_cols, compact in ((False, False), (True, False), (True, True)):
        for rank in range(nranks):
            mask = rr.shard_entries(N, nb, rank, nranks, by_cols)
            ref, bound = rr.grad_sums_and_bound(inp["U"], inp["w"], inp["sf2"], grp, S, kind, d_split, inp["alpha"], Kl, dU,
                                                entries=mask)
            mine = np.where(mask, Kl, np.nan)  # NaN in the block rows (columns) of the other ranks, and above the diagonal
            stored = rr.Window(_compact(mine, N, nb, rank, nranks) if compact else mine, np.nan)
            Kd = stored.window(_dev(stored.buf))
            out = _GradOut(N, D, S, dU)
            if by_cols:
                gpu_ctx.grad_reduce_cols(*dev, Kd, dU, nb, rank, nranks, *out.tensors(), kind=kind, d_split=d_split, compact=compact)
            else:
                gpu_ctx.grad_reduce_rows(*dev, Kd, dU, nb, rank, nranks, *out.tensors(), kind=kind, d_split=d_split)
            mode = "cols-compact" if compact else "cols" if by_cols else "rows"
            _compare_grad(out.read(), ref, bound, f"N {N} nb {nb} rank {rank} of {nranks} {mode}", prefix="sharded")


# ---- vector reductions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 130, 257))
def test_vector_reductions(gpu_ctx, N):
    rng = np.random.default_rng(31 * N)
    # one random lower-triangular matrix, and an INDEPENDENT one in the strict upper triangle: not each other's transposes
    T = np.tril(rng.standard_normal((N, N))) + np.triu(rng.standard_normal((N, N)), 1)
    sT = rr.Window(T, np.nan)
    dT = sT.window(_dev(sT.buf))
    diag = 10.0 ** np.linspace(-8, 3, N) if N > 1 else np.array([1e-8])
    F = np.full((N, N), np.nan)
    F[np.arange(N), np.arange(N)] = rng.permutation(diag)
    sF = rr.Window(F, np.nan)
    dF = sF.window(_dev(sF.buf))
    r = rng.standard_normal(N)
    rin = rr.VectorWindow(N, np.nan, x=r)
    dr = rin.window(_dev(rin.buf))
    label = f"N = {N}"

    # mll_reduce: z = (lower triangle) r, then the three scalars of the z the kernel wrote
    z, o3 = _Out(N), _Out(3)
    gpu_ctx.mll_reduce(dF, dT, dr, z.t, o3.t)
    zg = z.read("z")
    _compare("z", zg, *rr.trmv_lower(T, r), label)
    sref, sbound = rr.mll_scalars(np.diag(F), zg)
    for k, name in enumerate(("quad", "logdet", "mll")):
        _compare(name, o3.read("out3")[k], sref[k], sbound[k], label + " mll_reduce")
    # mll_scalars alone
    o3 = _Out(3)
    gpu_ctx.mll_scalars(dF, dr, o3.t)
    sref, sbound = rr.mll_scalars(np.diag(F), r)
    for k, name in enumerate(("quad", "logdet", "mll")):
        _compare(name, o3.read("out3")[k], sref[k], sbound[k], label + " mll_scalars")
    # alpha = (upper triangle with the diagonal) z
    al = _Out(N)
    gpu_ctx.alpha(dT, dr, al.t)
    _compare("alpha", al.read("alpha"), *rr.trmv_upper(T, r), label)

    for M in (1, 3, 4, 5):
        Ksn, kss = rng.standard_normal((M, N)), rng.uniform(0.5, 2.0, M) + N
        sK = rr.Window(Ksn, np.nan)
        dKsn, dkss = sK.window(_dev(sK.buf)), _dev(kss)
        (mref, _), (mbound, _) = rr.predict_rows(Ksn, None, r, None)
        # predict without V: the mean alone
        mean = _Out(M)
        gpu_ctx.predict(dT, dr, dKsn, None, None, mean.t, None)
        _compare("mean", mean.read("mean"), mref, mbound, f"{label} M = {M} predict without V")
        # predict with V: the product is the GEMM's business; the variance is held to the V the kernel itself wrote
        sV = rr.Window(np.full((M, N), rr.SENTINEL), rr.SENTINEL)
        dVb = _dev(sV.buf)
        mean, var = _Out(M), _Out(M)
        gpu_ctx.predict(dT, dr, dKsn, dkss, sV.window(dVb), mean.t, var.t)
        Vb = dVb.cpu().numpy()
        g = sV.guard_mask()
        assert rr.same_bits(Vb[g], sV.buf[g]), "V: written outside its window"
        (_, vref), (_, vbound) = rr.predict_rows(Ksn, sV.window(Vb), r, kss)
        _compare("mean", mean.read("mean"), mref, mbound, f"{label} M = {M} predict")
        _compare("var", var.read("var"), vref, vbound, f"{label} M = {M} predict")
        # predict_tn: mean and variance are both reductions of the V it wrote
        sKns = rr.Window(Ksn.T.copy(), np.nan)
        dVb = _dev(sV.buf)
        mean, var = _Out(M), _Out(M)
        gpu_ctx.predict_tn(dT, dr, sKns.window(_dev(sKns.buf)), dkss, sV.window(dVb), mean.t, var.t)
        Vb = dVb.cpu().numpy()
        assert rr.same_bits(Vb[g], sV.buf[g]), "V: written outside its window"
        Vg = sV.window(Vb)
        (mref2, vref2), (mbound2, vbound2) = rr.predict_rows(Vg, Vg, r, kss)
        _compare("mean", mean.read("mean"), mref2, mbound2, f"{label} M = {M} predict_tn")
        _compare("var", var.read("var"), vref2, vbound2, f"{label} M = {M} predict_tn")


def test_zz_report_largest_error_to_bound_ratios(gpu_ctx, capsys):
    """Runs last in the module: how much room the derived bounds leave on the hardware."""
    line = "reduce conformance, largest err / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIOS.items()))
    with capsys.disabled():
        print("\n" + line)
    assert all(v <= 1.0 for v in RATIOS.values())

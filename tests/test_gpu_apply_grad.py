"""gpp_kernel_apply_grad / gpp_rff_apply_grad (csrc/gpp_apply.hip) against the long-double gradient of
tests/pathwise_grad_reference.py.

Tolerance (elementwise, derived in that module's docstring): with W_j = V_j m_j, V = Gbar C^T, T_d = sum_j |W_j| (|a_d| + |b_jd|),

    |g_d - ref_d| <= s_d [ (L + 16 + pieces) u T_d + sum_j dW_j (|a_d| + |b_jd|) ] + u |beta g0_d|,      u = 2^-53

tests/test_pathwise_grad_host.py holds this bound to at most 1e-9 of max |ref| per column on every case below, so it cannot hide a
wrong kernel.  Every case prints observed / bound (``pytest -s``)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import pathwise_grad_reference as G  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
SPLIT = G.SPLIT


def _guarded(a, pad=7):
    """A contiguous device copy of ``a`` inside a NaN-filled allocation: a read outside the extents that reaches a result shows."""
    flat = torch.full((a.size + 2 * pad,), float("nan"), dtype=torch.float64, device="cuda")
    flat[pad:pad + a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    return flat[pad:pad + a.size].view(*a.shape)


def _strided(a, slack, fill=float("nan")):
    """``a`` (rows x cols) as a view with leading dimension cols + slack; the slack holds ``fill``."""
    rows, cols = a.shape
    buf = torch.full((rows, cols + slack), fill, dtype=torch.float64, device="cuda")
    buf[:, :cols] = torch.from_numpy(a).cuda()
    return buf, buf[:, :cols]


def _device(p):
    dev = {k: _guarded(p[k]) for k in ("Ua", "second")}
    dev["phase"] = None if p["phase"] is None else _guarded(p["phase"])
    dev["w"] = None if p["w"] is None else _guarded(p["w"])
    dev["Cbuf"], dev["C"] = _strided(p["C"], 3)
    dev["Gbuf"], dev["Gbar"] = _strided(p["Gbar"], 5)
    return dev


def _run(ctx, gen, p, dev, beta):
    """One launch into a fresh NaN-slack gradient (NaN-prefilled when beta = 0): (whole buffer, the M x D window)."""
    init = p["g0"] if beta != 0.0 else np.full(p["g0"].shape, np.nan)
    buf, out = _strided(init, 2)
    sf2 = torch.tensor([p["sf2"]], dtype=torch.float64, device="cuda")
    if gen == "rff":
        ctx.rff_apply_grad(dev["Ua"], dev["second"], dev["phase"], sf2, dev["C"], dev["Gbar"], out, beta=beta)
    else:
        ctx.kernel_apply_grad(dev["Ua"], dev["second"], dev["w"], sf2, dev["C"], dev["Gbar"], out, beta=beta, kind=p["kind"],
                              d_split=p["d_split"])
    return buf, out


@pytest.mark.parametrize("name,M,L,S,D,beta,copies", [pytest.param(*c[1:], id=c[0]) for c in G.cases()])
def test_apply_grad_against_longdouble_reference(gpu_ctx, name, M, L, S, D, beta, copies):
    gen, p = G.case_inputs(name, M, L, S, D, copies)
    dev = _device(p)
    buf, out = _run(gpu_ctx, gen, p, dev, beta)
    buf2, _ = _run(gpu_ctx, gen, p, dev, beta)
    torch.cuda.synchronize()
    ref, bound = G.grad_reference(gen, p, beta)
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), "beta = 0 must overwrite a NaN-prefilled g_Ua; no NaN may come from outside the extents"
    assert bool(torch.isnan(buf[:, D:]).all()), "the slack of g_Ua was written"
    assert bool(torch.isnan(dev["Cbuf"][:, S:]).all()) and bool(torch.isnan(dev["Gbuf"][:, S:]).all())
    assert torch.equal(buf[:, :D], buf2[:, :D]), "two launches differ"
    err = np.abs(got.astype(LD) - ref)
    if p["w"] is not None:
        assert (got[:, p["w"] == 0.0] == (beta * p["g0"])[:, p["w"] == 0.0]).all(), "a feature with w_d = 0 gets an exact 0"
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())
    scale = float(err.max() / max(float(np.abs(ref).max()), 1e-300))
    print(f"{name} M={M} L={L} S={S} D={D} beta={beta}: max err {float(err.max()):.3e} ({scale:.2e} of max |ref|), "
          f"observed / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", ["rbf", "m52", "rff"])
@pytest.mark.parametrize("L", [200, SPLIT + 1])
def test_rows_do_not_depend_on_the_other_rows_of_the_call(gpu_ctx, name, L):
    """Rows idx of a call on Ua equal the call on (Ua[idx], Gbar[idx]), bit for bit (another position in the tile, another tile count)."""
    gen, kind = G.GENS[name]
    p = G.inputs(gen, 130, L, 17, 8, kind, seed=L)
    dev = _device(p)
    _, full = _run(gpu_ctx, gen, p, dev, 0.0)
    idx = np.array([129, 5, 64, 0, 63, 70, 65])
    q = dict(p, Ua=p["Ua"][idx], Gbar=p["Gbar"][idx], g0=p["g0"][idx])
    devq = dict(dev, Ua=_guarded(q["Ua"]))
    devq["Gbuf"], devq["Gbar"] = _strided(q["Gbar"], 5)
    _, part = _run(gpu_ctx, gen, q, devq, 0.0)
    assert torch.equal(full[torch.from_numpy(idx).cuda()], part)


def test_missing_workspace_and_bad_arguments_are_reported(gpu_ctx):
    from gpplus_amd._lib import GppError

    p = G.inputs("kernel", 4, 8, 2, 3, 0, seed=1)
    dev = _device(p)
    out = torch.zeros(4, 3, dtype=torch.float64, device="cuda")
    sf2 = torch.ones(1, dtype=torch.float64, device="cuda")
    with pytest.raises(GppError):
        gpu_ctx.kernel_apply_grad(dev["Ua"], dev["second"][:, :2].contiguous(), dev["w"], sf2, dev["C"], dev["Gbar"], out)  # D mismatch
    with pytest.raises(GppError):
        gpu_ctx.kernel_apply_grad(dev["Ua"], dev["second"], dev["w"], sf2, dev["C"], dev["Gbar"][:3], out)  # wrong Gbar
    with pytest.raises(GppError):
        gpu_ctx.kernel_apply_grad(dev["Ua"], dev["second"], dev["w"], sf2, dev["C"], dev["Gbar"], out[:, :2])  # wrong g_Ua
    with pytest.raises(GppError):
        gpu_ctx.rff_apply_grad(dev["Ua"], dev["second"], dev["second"][:3, 0].contiguous(), sf2, dev["C"], dev["Gbar"], out)  # phase
    lib, h = gpu_ctx.lib, gpu_ctx.h
    args = (h, dev["Ua"].data_ptr(), 4, dev["second"].data_ptr(), 8, 3, dev["w"].data_ptr(), sf2.data_ptr(), 0, 0,
            dev["C"].data_ptr(), 5, 2, dev["Gbar"].data_ptr(), 7, 0.0, out.data_ptr(), 3)
    assert lib.gpp_kernel_apply_grad(*args) == 0
    torch.cuda.synchronize()
    before = out.clone()
    for pos, value, status in ((11, 1, -12), (14, 1, -15), (17, 2, -18), (5, 65, -6), (13, None, -14), (16, None, -17)):
        bad = list(args)
        bad[pos] = value
        assert lib.gpp_kernel_apply_grad(*bad) == status
    phase = torch.zeros(8, dtype=torch.float64, device="cuda")
    rargs = (h, dev["Ua"].data_ptr(), 4, 3, dev["second"].data_ptr(), phase.data_ptr(), 8, sf2.data_ptr(), dev["C"].data_ptr(), 5, 2,
             dev["Gbar"].data_ptr(), 7, 0.0, out.data_ptr(), 3)
    for pos, value, status in ((9, 1, -10), (12, 1, -13), (15, 2, -16), (11, None, -12), (14, None, -15)):
        bad = list(rargs)
        bad[pos] = value
        assert lib.gpp_rff_apply_grad(*bad) == status
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # the workspace: pieces * M * D doubles above a contracted length of 2048 (+ the 256 bytes every id carries); ids 0-3 as before
    assert int(lib.gpp_workspace_bytes(h, 4, SPLIT, 4, 3, 2)) == 256
    assert int(lib.gpp_workspace_bytes(h, 4, SPLIT + 1, 4, 3, 2)) == 2 * 4 * 3 * 8 + 256
    assert int(lib.gpp_workspace_bytes(h, 4, 3 * SPLIT, 130, 64, 17)) == 3 * 130 * 64 * 8 + 256
    assert int(lib.gpp_workspace_bytes(h, 3, SPLIT + 1, 4, 3, 2)) == 2 * 4 * 2 * 8 + 256
    assert int(lib.gpp_workspace_bytes(h, 1, 100, 4, 3, 2)) == 256
    # a split contraction without the workspace: GPP_NO_WORKSPACE, nothing enqueued
    saved = gpu_ctx._ws
    try:
        assert lib.gpp_set_workspace(h, None, 0) == 0
        # operands of the stated size: were the check to regress, the launch would stay inside its buffers
        big_ub = torch.zeros(SPLIT + 1, 3, dtype=torch.float64, device="cuda")
        big_c = torch.zeros(SPLIT + 1, 5, dtype=torch.float64, device="cuda")
        big_ph = torch.zeros(SPLIT + 1, dtype=torch.float64, device="cuda")
        long_args = list(args)
        long_args[3], long_args[4], long_args[10] = big_ub.data_ptr(), SPLIT + 1, big_c.data_ptr()
        assert lib.gpp_kernel_apply_grad(*long_args) == 2002
        long_r = list(rargs)
        long_r[4], long_r[5], long_r[6], long_r[8] = big_ub.data_ptr(), big_ph.data_ptr(), SPLIT + 1, big_c.data_ptr()
        assert lib.gpp_rff_apply_grad(*long_r) == 2002
        torch.cuda.synchronize()
        assert torch.equal(out, before)
    finally:
        if saved is not None:
            assert lib.gpp_set_workspace(h, ctypes.c_void_p(saved.data_ptr()), saved.numel()) == 0
    torch.cuda.synchronize()

"""gpp_kernel_apply / gpp_rff_apply (csrc/gpp_apply.hip) against the generated matrix of tests/pathwise_reference.py times C in
``np.longdouble``.

Tolerance (elementwise, derived — ``pathwise_reference.apply_bound``):

    |Out - ref| <= (K + 4) u (|G| @ |C| + |beta| |Out0|) + dG @ |C|,        u = 2^-53, K the contracted length

the first term is the dot-product bound of ``gemm_reference.error_bound`` (any summation order, the pieces of a split
contraction included), the second the first-order effect of the generator's own error dG:

  kernel:   dG = G (dr2_rbf + 4 u [2-ulp exp, DESIGN.md 3.4] + 3 u) + sf2 e1 dh,
            dr2 = sum_d 2 |df_d| (3 u (|a_d| + |b_d|) + u |df_d|) + (n + 1) u r2   (staged a_d = fl(u_d fl(sqrt w_d)), n fused adds),
            dh = 0.4 dr + 12 u h,  dr = sqrt(4 nu) min(sqrt(dr2_mat), dr2_mat / (2 sqrt(r2_mat))) + 4 u r      (Matern kinds only)
  features: dG = amp (2 pi (D + 3) u T + 4 u [the cosine polynomial's stated error]) + 4 u |G|,
            T = (sum_d |omega_d u_d| + |b|) / 2 pi   (the phase is summed in turns)

Every case prints observed / bound (``pytest -s``)."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import pathwise_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
SPLIT = 2048  # longest contraction without pieces (backend.APPLY_SPLIT)


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


def _inputs(gen, M, L, S, D, kind, seed):
    rng = np.random.default_rng(seed)
    Ua = rng.uniform(-1.0, 1.0, (M, D))
    C = rng.standard_normal((L, S))
    Out0 = rng.standard_normal((M, S))
    sf2 = 1.3
    if gen == "rff":
        w = rng.uniform(0.2, 2.0, D)
        second = rng.standard_normal((L, D)) * np.sqrt(2.0 * w)  # frequencies
        phase = rng.uniform(0.0, 2.0 * np.pi, L)
        return dict(Ua=Ua, second=second, phase=phase, sf2=sf2, C=C, Out0=Out0, w=None, kind=0, d_split=0)
    w = rng.uniform(0.2, 2.0, D) / D
    if D > 2:
        w[D // 2] = 0.0
    second = rng.uniform(-1.0, 1.0, (L, D))
    return dict(Ua=Ua, second=second, phase=None, sf2=sf2, C=C, Out0=Out0, w=w, kind=kind, d_split=0 if kind == 0 else D // 2)


def _reference(gen, p, beta):
    if gen == "rff":
        G = R.rff_matrix(p["Ua"], p["second"], p["phase"], p["sf2"])
        dG = R.rff_gen_error(p["Ua"], p["second"], p["phase"], p["sf2"])
    else:
        G = R.kernel_matrix(p["Ua"], p["second"], p["w"], p["sf2"], p["kind"], p["d_split"])
        dG = R.kernel_gen_error(p["Ua"], p["second"], p["w"], p["sf2"], p["kind"], p["d_split"])
    ref = LD(beta) * p["Out0"].astype(LD) + G @ p["C"].astype(LD)
    return ref, R.apply_bound(G, dG, p["C"], beta, p["Out0"])


def _launch(ctx, gen, p, dev, beta, out):
    sf2 = torch.tensor([p["sf2"]], dtype=torch.float64, device="cuda")
    if gen == "rff":
        ctx.rff_apply(dev["Ua"], dev["second"], dev["phase"], sf2, dev["C"], out, beta=beta)
    else:
        ctx.kernel_apply(dev["Ua"], dev["second"], dev["w"], sf2, dev["C"], out, beta=beta, kind=p["kind"], d_split=p["d_split"])


def _device(p):
    dev = {k: _guarded(p[k]) for k in ("Ua", "second")}
    dev["phase"] = None if p["phase"] is None else _guarded(p["phase"])
    dev["w"] = None if p["w"] is None else _guarded(p["w"])
    dev["Cbuf"], dev["C"] = _strided(p["C"], 3)
    return dev


def _run(ctx, gen, p, dev, beta):
    """One launch into a fresh NaN-slack output: (whole buffer, the M x S window)."""
    M, S = p["Out0"].shape
    init = p["Out0"] if beta != 0.0 else np.full((M, S), np.nan)
    buf, out = _strided(init, 2)
    _launch(ctx, gen, p, dev, beta, out)
    return buf, out


BASE = dict(M=65, L=65, S=17, D=8)
GENS = {"rbf": ("kernel", 0), "m32": ("kernel", 1), "m52": ("kernel", 2), "rff": ("rff", 0)}


def _cases():
    out = []

    def add(name, beta, **kw):
        c = dict(BASE, **kw)
        out.append(pytest.param(name, c["M"], c["L"], c["S"], c["D"], beta, id=f"{name}-M{c['M']}-L{c['L']}-S{c['S']}-D{c['D']}-b{beta}"))

    for name in ("rbf", "rff"):  # the two generators: every edge of every axis
        for beta in (0.0, 1.0):
            add(name, beta)
        for i, M in enumerate((1, 63, 64, 130)):
            add(name, float(i & 1), M=M)
        for i, L in enumerate((1, 15, 16, 17, 200, SPLIT, SPLIT + 1, SPLIT + 2)):
            add(name, float(i & 1), L=L)
        for i, S in enumerate((1, 3, 16, 64, 65)):
            add(name, float(i & 1), S=S)
        for i, D in enumerate((1, 17, 64)):
            add(name, float(i & 1), D=D)
    for name in ("m32", "m52"):  # the second distance accumulator and d_split: along D and across the split
        for beta in (0.0, 1.0):
            add(name, beta)
        for i, D in enumerate((1, 17, 64)):
            add(name, float(i & 1), D=D)
        add(name, 1.0, L=SPLIT + 1, M=130, S=65)
    add("rff", 1.0, M=130, L=SPLIT + 1, S=65, D=64)  # every edge at once, the largest LDS request
    add("rbf", 0.0, M=1, L=1, S=1, D=1)
    return out


@pytest.mark.parametrize("name,M,L,S,D,beta", _cases())
def test_apply_against_longdouble_reference(gpu_ctx, name, M, L, S, D, beta):
    gen, kind = GENS[name]
    p = _inputs(gen, M, L, S, D, kind, seed=zlib.crc32(f"{name}-{M}-{L}-{S}-{D}".encode()))
    dev = _device(p)
    buf, out = _run(gpu_ctx, gen, p, dev, beta)
    buf2, _ = _run(gpu_ctx, gen, p, dev, beta)
    torch.cuda.synchronize()
    ref, bound = _reference(gen, p, beta)
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), "beta = 0 must overwrite a NaN-prefilled Out; no NaN may come from outside the extents"
    assert bool(torch.isnan(buf[:, S:]).all()), "the slack of Out was written"
    assert bool(torch.isnan(dev["Cbuf"][:, S:]).all())
    assert torch.equal(buf[:, :S], buf2[:, :S]), "two launches differ"
    err = np.abs(got.astype(LD) - ref)
    ratio = float((err / bound).max())
    print(f"{name} M={M} L={L} S={S} D={D} beta={beta}: max err {float(err.max()):.3e}, observed / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", ["rbf", "m52", "rff"])
@pytest.mark.parametrize("L", [200, SPLIT + 1])
def test_rows_do_not_depend_on_the_other_rows_of_the_call(gpu_ctx, name, L):
    """Rows idx of a call on Ua equal the call on Ua[idx], bit for bit (another position in the tile, another tile count)."""
    gen, kind = GENS[name]
    p = _inputs(gen, 130, L, 17, 8, kind, seed=L)
    dev = _device(p)
    _, full = _run(gpu_ctx, gen, p, dev, 0.0)
    idx = np.array([129, 5, 64, 0, 63, 70, 65])
    q = dict(p, Ua=p["Ua"][idx], Out0=p["Out0"][idx])
    devq = dict(dev, Ua=_guarded(q["Ua"]))
    _, part = _run(gpu_ctx, gen, q, devq, 0.0)
    assert torch.equal(full[torch.from_numpy(idx).cuda()], part)


def test_missing_workspace_and_bad_arguments_are_reported(gpu_ctx):
    import ctypes

    from gpplus_amd._lib import GppError

    p = _inputs("kernel", 4, 8, 2, 3, 0, seed=1)
    dev = _device(p)
    out = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    sf2 = torch.ones(1, dtype=torch.float64, device="cuda")
    with pytest.raises(GppError):
        gpu_ctx.kernel_apply(dev["Ua"], dev["second"][:, :2].contiguous(), dev["w"], sf2, dev["C"], out)  # D mismatch
    with pytest.raises(GppError):
        gpu_ctx.kernel_apply(dev["Ua"], dev["second"], dev["w"], sf2, dev["C"], out[:3])  # wrong Out
    lib, h = gpu_ctx.lib, gpu_ctx.h
    args = (h, dev["Ua"].data_ptr(), 4, dev["second"].data_ptr(), 8, 3, dev["w"].data_ptr(), sf2.data_ptr(), 0, 0,
            dev["C"].data_ptr(), 5, 2, 0.0, out.data_ptr(), 2)
    assert lib.gpp_kernel_apply(*args) == 0
    bad = list(args)
    bad[11] = 1  # ldc < S
    assert lib.gpp_kernel_apply(*bad) == -12
    # a split contraction without the workspace: GPP_NO_WORKSPACE, nothing enqueued
    assert int(lib.gpp_workspace_bytes(h, 3, SPLIT, 4, 3, 2)) == 256
    assert int(lib.gpp_workspace_bytes(h, 3, SPLIT + 1, 4, 3, 2)) == 2 * 4 * 2 * 8 + 256
    saved = gpu_ctx._ws
    try:
        assert lib.gpp_set_workspace(h, None, 0) == 0
        # operands of the stated size: were the check to regress, the launch would stay inside its buffers
        big_ub = torch.zeros(SPLIT + 1, 3, dtype=torch.float64, device="cuda")
        big_c = torch.zeros(SPLIT + 1, 5, dtype=torch.float64, device="cuda")
        long_args = list(args)
        long_args[3], long_args[4], long_args[10] = big_ub.data_ptr(), SPLIT + 1, big_c.data_ptr()
        before = out.clone()
        assert lib.gpp_kernel_apply(*long_args) == 2002
        torch.cuda.synchronize()
        assert torch.equal(out, before)
    finally:
        if saved is not None:
            assert lib.gpp_set_workspace(h, ctypes.c_void_p(saved.data_ptr()), saved.numel()) == 0
    torch.cuda.synchronize()

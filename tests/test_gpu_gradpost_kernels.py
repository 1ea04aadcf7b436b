"""The two kernels behind the posterior of the gradient on the GPU: gpp_cross_kernel_dx against the long-double derivative of the
generated kernel (tests/pathwise_grad_reference.py) within that file's multiplier bound, gpp_point_gram against a float64 numpy Gram
within the dot-product bound; extents (sentinels in the padding and in a guard band, NaN behind the rows that are read), exact
zeros, bitwise repeatability and independence of a point from its neighbours, argument codes and the missing workspace."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pathwise_grad_reference as PG  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = 2.0 ** -53
SENTINEL = -7.25
GUARD = 64  # doubles in front of and behind the buffer (512 bytes: the window stays 16-byte aligned)

DX_CASES = [(5, 70, 5, 2, 3), (1, 1, 1, 0, 1), (3, 130, 6, 0, 6), (7, 65, 4, 3, 1)]  # M, N, D, d0, nd


def _dx_inputs(M, N, D, d0, nd, kind):
    rng = np.random.default_rng(1000 * M + 10 * N + D + 7 * kind)
    Ua = rng.uniform(-1.0, 1.0, (M, D))
    Ub = rng.uniform(-1.0, 1.0, (N, D))
    w = rng.uniform(0.2, 2.0, D) / D
    zero = d0 if nd >= 2 else None
    if zero is not None:
        w[zero] = 0.0  # a differentiated feature without weight
    copy = None
    if M > 1:
        copy = (M - 1, min(3, N - 1))
        Ua[copy[0]] = Ub[copy[1]]  # a test row that is a training row
    return Ua, Ub, w, 1.3, zero, copy


def _guarded(N, cols, dev):
    """An N x cols window (leading dimension: cols padded to even, plus 2) of a sentinel-filled buffer with a guard band."""
    ld = (cols + 1) // 2 * 2 + 2
    flat = torch.full((2 * GUARD + N * ld,), SENTINEL, dtype=torch.float64, device=dev)
    return flat, flat[GUARD:GUARD + N * ld].view(N, ld), ld


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("M,N,D,d0,nd", DX_CASES)
def test_cross_kernel_dx(gpu_ctx, M, N, D, d0, nd, kind):
    """Bound per entry: the kernel forms (2 w_d) (ua_d - ub_d) in fp64 from the raw features — the doubling is exact, the difference
    and the two products round once each, 3 u of the value, taken as 4 u — times a multiplier that errs by at most the dm of
    ``kernel_multiplier_errors`` (the staged arithmetic of gpp_kernel_apply_grad, which the kernel repeats)."""
    dev = gpu_ctx.device
    d_split = d0
    Ua, Ub, w, sf2, zero, copy = _dx_inputs(M, N, D, d0, nd, kind)
    c = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    dUa, dUb, dw, ds = c(Ua), c(Ub), c(w), c([sf2])

    def run():
        flat, buf, ld = _guarded(N, M * nd, dev)
        gpu_ctx.cross_kernel_dx(dUa, dUb, dw, ds, d0, nd, buf[:, :M * nd], kind=kind, d_split=d_split)
        torch.cuda.synchronize()
        return flat.cpu(), buf.cpu(), ld

    flat, buf, ld = run()
    assert (M * nd) % 2 == 0 or ld == M * nd + 3  # odd widths are padded to even before the two spare columns
    assert bool((buf[:, M * nd:] == SENTINEL).all()), "padding columns were written"
    assert bool((flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all()), "guard band was written"
    got = buf[:, :M * nd].numpy().reshape(N, M, nd)
    assert np.isfinite(got).all()
    dms = PG.kernel_multiplier_errors(Ua, Ub, w, sf2, kind, d_split)
    worst = 0.0
    for j in range(nd):
        d = d0 + j
        ref = PG.kernel_dgen(Ua, Ub, w, sf2, kind, d_split, d)  # M x N
        dm = dms[PG._factor(d, D, kind, d_split)]
        delta = np.abs(Ua[:, d, None].astype(LD) - Ub[None, :, d].astype(LD))
        bound = 2 * LD(w[d]) * delta * dm + 4 * U53 * np.abs(ref)
        err = np.abs(got[:, :, j].T.astype(LD) - ref)
        assert (err <= bound).all(), (j, float((err - bound).max()))
        worst = max(worst, float((err / np.maximum(np.abs(ref), 1e-300)).max()))
    print(f"cross_kernel_dx M={M} N={N} D={D} d0={d0} nd={nd} kind={kind}: worst relative error {worst:.3e}")
    if zero is not None:
        assert (got[:, :, zero - d0] == 0.0).all(), "a feature with w_d == 0 must give an exact 0"
    if copy is not None:
        assert (got[copy[1], copy[0], :] == 0.0).all(), "a test row equal to a training row: exact zeros in that pair"
    flat2, _, _ = run()
    assert torch.equal(flat.view(torch.int64), flat2.view(torch.int64)), "two launches differ"


def test_cross_kernel_dx_argument_codes(gpu_ctx):
    from gpplus_amd._lib import GppError

    dev = gpu_ctx.device
    M, N, D, d0, nd = 3, 9, 4, 1, 3
    Ua = torch.rand(M, D, dtype=torch.float64, device=dev)
    Ub = torch.rand(N, D, dtype=torch.float64, device=dev)
    w = torch.rand(D, dtype=torch.float64, device=dev)
    sf2 = torch.ones(1, dtype=torch.float64, device=dev)
    flat, buf, ld = _guarded(N, M * nd, dev)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    gpu_ctx._stream()

    def raw(D_=D, kind=1, d_split=1, d0_=d0, nd_=nd, ptr=buf.data_ptr(), ld_=ld, M_=M):
        return lib.gpp_cross_kernel_dx(h, Ua.data_ptr(), M_, Ub.data_ptr(), N, D_, w.data_ptr(), sf2.data_ptr(), kind, d_split, d0_, nd_,
                                       ptr, ld_)

    assert raw(D_=65) == -6 and raw(D_=0) == -6
    assert raw(kind=3) == -9 and raw(d_split=5) == -10
    assert raw(d0_=-1) == -11 and raw(d0_=4) == -11
    assert raw(nd_=0) == -12 and raw(d0_=2, nd_=3) == -12
    assert raw(ptr=buf.data_ptr() + 8) == -13 and raw(ptr=None) == -13
    assert raw(ld_=ld + 1) == -14 and raw(ld_=M * nd - 1) == -14
    assert raw(M_=0) == -3
    torch.cuda.synchronize()
    assert bool((flat == SENTINEL).all()), "a refused call wrote something"
    assert raw() == 0
    torch.cuda.synchronize()
    assert bool((buf[:, :M * nd] != SENTINEL).all())
    # the binding refuses the same things in words
    with pytest.raises(GppError, match="leading dimension"):
        gpu_ctx.cross_kernel_dx(Ua, Ub, w, sf2, d0, nd, torch.zeros((N, M * nd + 2), dtype=torch.float64, device=dev)[:, :M * nd])
    with pytest.raises(GppError, match="differentiated columns"):
        gpu_ctx.cross_kernel_dx(Ua, Ub, w, sf2, 2, 3, buf[:, :M * nd])


# ---- gpp_point_gram --------------------------------------------------------------------------------------------------------------------
PG_CASES = [(3, 1, 1), (4, 3, 63), (2, 16, 130), (5, 8, 2049)]  # M, nd, N


def _bits(t):
    return t.contiguous().view(torch.int64)


def _q_buffer(Qh, dev):
    """Q on the device behind a leading dimension > N whose spare columns hold NaN."""
    rows, N = Qh.shape
    ldq = (N + 1) // 2 * 2 + 2
    buf = torch.full((rows, ldq), float("nan"), dtype=torch.float64, device=dev)
    buf[:, :N] = torch.tensor(Qh, device=dev)
    return buf[:, :N]


@pytest.mark.parametrize("M,nd,N", PG_CASES)
def test_point_gram(gpu_ctx, M, nd, N):
    """Each entry is a dot product of length N in fp64: |error| <= N 2^-52 sum |terms| for any order of the additions (first order,
    with room to spare: the standard bound is N u, u = 2^-53).  The weighted total adds M such values: (N + M + 2) 2^-52 of the
    weighted sum of the absolute terms."""
    dev = gpu_ctx.device
    rng = np.random.default_rng(100 * M + nd + N)
    Qh = rng.standard_normal((M * nd, N))
    om_h = rng.uniform(0.1, 2.0, M)
    Q = _q_buffer(Qh, dev)
    om = torch.tensor(om_h, device=dev)
    Q3 = Qh.reshape(M, nd, N)
    ref = np.einsum("ajn,akn->ajk", Q3, Q3)
    mag = np.einsum("ajn,akn->ajk", np.abs(Q3), np.abs(Q3))

    def run(Qd, omega, want_G=True, want_sum=True):
        m = Qd.shape[0] // nd
        G = torch.full((m, nd, nd), float("nan"), dtype=torch.float64, device=dev) if want_G else None
        Gs = torch.full((nd, nd), float("nan"), dtype=torch.float64, device=dev) if want_sum else None
        gpu_ctx.point_gram(Qd, nd, G=G, Gsum=Gs, omega=omega)
        torch.cuda.synchronize()
        return (None if G is None else G.cpu()), (None if Gs is None else Gs.cpu())

    G, Gs = run(Q, om)
    err = np.abs(G.numpy() - ref)
    assert (err <= N * 2.0 ** -52 * mag).all(), float((err / mag).max())
    assert torch.equal(_bits(G), _bits(G.transpose(1, 2))), "G is not bitwise symmetric"
    ref_sum = np.einsum("a,ajk->jk", om_h, ref)
    assert (np.abs(Gs.numpy() - ref_sum) <= (N + M + 2) * 2.0 ** -52 * np.einsum("a,ajk->jk", om_h, mag)).all()
    assert torch.equal(_bits(Gs), _bits(Gs.T))
    # two calls agree bit for bit
    G2, Gs2 = run(Q, om)
    assert torch.equal(_bits(G), _bits(G2)) and torch.equal(_bits(Gs), _bits(Gs2))
    # only the sum, only the matrices, no weights
    Gn, Gs_only = run(Q, om, want_G=False)
    assert Gn is None and torch.equal(_bits(Gs_only), _bits(Gs))
    G_only, none = run(Q, None, want_sum=False)
    assert none is None and torch.equal(_bits(G_only), _bits(G))
    _, Gs_ones = run(Q, None)
    ones_sum = ref.sum(0)
    assert (np.abs(Gs_ones.numpy() - ones_sum) <= (N + M + 2) * 2.0 ** -52 * mag.sum(0)).all()
    # a point's matrix does not depend on its neighbours or on its index
    for a in range(M):
        alone, _ = run(_q_buffer(Qh[a * nd:(a + 1) * nd], dev), None, want_sum=False)
        assert torch.equal(_bits(alone[0]), _bits(G[a])), f"point {a} differs when it is alone"
    rev = np.concatenate([Qh[a * nd:(a + 1) * nd] for a in reversed(range(M))])
    Gr, _ = run(_q_buffer(rev, dev), None, want_sum=False)
    assert torch.equal(_bits(Gr.flip(0)), _bits(G)), "a point's matrix depends on its index"


def test_point_gram_refusals(gpu_ctx):
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import NO_WORKSPACE, OP_POINT_GRAM

    dev = gpu_ctx.device
    M, nd, N = 70, 5, 33
    Q = _q_buffer(np.random.default_rng(0).standard_normal((M * nd, N)), dev)
    ldq = Q.stride(0)
    G = torch.full((M, nd, nd), float("nan"), dtype=torch.float64, device=dev)
    Gs = torch.full((nd, nd), float("nan"), dtype=torch.float64, device=dev)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    gpu_ctx._stream()

    def raw(nd_=nd, M_=M, ldq_=ldq, ptr=Q.data_ptr(), g=G.data_ptr(), gs=Gs.data_ptr()):
        return lib.gpp_point_gram(h, ptr, ldq_, M_, nd_, N, None, g, gs)

    need = int(lib.gpp_workspace_bytes(h, OP_POINT_GRAM, 0, M, nd, 0))
    small = torch.empty(need - 512, dtype=torch.uint8, device=dev)
    try:
        assert lib.gpp_set_workspace(h, small.data_ptr(), small.numel()) == 0
        assert raw() == NO_WORKSPACE and raw(g=None) == NO_WORKSPACE
        assert lib.gpp_set_workspace(h, None, 0) == 0
        assert raw() == NO_WORKSPACE
        assert raw(gs=None) == 0  # the matrices alone need no workspace
    finally:
        gpu_ctx._ws = None  # the context attaches a workspace of its own at the next call that needs one
        lib.gpp_set_workspace(h, None, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Gs).all()) and not bool(torch.isnan(G).any())
    G.fill_(float("nan"))
    assert raw(nd_=17) == -5 and raw(nd_=0) == -5
    assert raw(ldq_=ldq + 1) == -3 and raw(ldq_=N - 1) == -3
    assert raw(ptr=Q.data_ptr() + 8) == -2 and raw(M_=0) == -4
    assert raw(g=None, gs=None) == -9
    torch.cuda.synchronize()
    assert bool(torch.isnan(G).all()) and bool(torch.isnan(Gs).all()), "a refused call wrote something"
    with pytest.raises(GppError, match="1..16"):
        gpu_ctx.point_gram(Q[:M * nd // 17 * 17], 17, G=None, Gsum=Gs)
    with pytest.raises(GppError, match="leading dimension"):
        gpu_ctx.point_gram(torch.zeros((M * nd, N + 2), dtype=torch.float64, device=dev)[:, :N], nd, G=G)

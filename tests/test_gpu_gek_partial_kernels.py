"""The three ``_sel`` entry points (partial gradients) on the GPU.  gpp_cross_kernel_dx_sel and gpp_kernel_dxdx_sel must equal, BIT FOR
BIT, the dense call's rows and columns gathered — the dense kernels are pinned to the long-double references by
tests/test_gpu_gradpost_kernels.py and tests/test_gpu_gek_kernels.py — on masks that give odd counts and tiles that start at odd
columns, a tile of points without any entry, entries at the last point only, and everything (the dense buffer itself); with
sentinel-filled padding columns and a guard band, and twice.  gpp_gek_grad_reduce_sel against ``gek_train_reference.block_sums`` with
the compact weights scattered into the dense layout (zeros in the unobserved rows and columns), at the bar and with the floor check
of tests/test_gpu_gek_train_kernel.py.  The argument codes of the three."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gek_partial_reference as P  # noqa: E402
import gek_train_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 64  # doubles in front of and behind the buffer (512 bytes: the window stays 16-byte aligned)
BAR = 1e-6

DX_CASES = [(1, 1, 1, 0, 1, 0), (17, 33, 5, 2, 3, 2), (35, 70, 6, 0, 6, 3), (3, 130, 4, 3, 1, 3)]  # M, N, D, d0, nd, d_split
HX_CASES = [(1, 1, 1, 0, 1, 0), (5, 70, 5, 2, 3, 2), (17, 33, 6, 0, 6, 3), (3, 130, 4, 3, 1, 3)]  # as tests/test_gpu_gek_kernels.py
MASKS = ("pattern", "first tile empty", "last point only", "all")


def _raw_pattern(M, nd):
    """((3 a + 5 j) mod 7) < 3 WITHOUT the fix-up of empty points: at the C level a point may have no entry."""
    a, j = torch.arange(M)[:, None], torch.arange(nd)[None, :]
    return ((3 * a + 5 * j) % 7) < 3


def _mask(which, M, nd):
    if which == "pattern":
        m = _raw_pattern(M, nd)
        if not bool(m.any()):
            m[0, 0] = True
        return m
    if which == "first tile empty":  # points 0..15 without an entry: a tile that owns no column (nothing at all for M <= 16)
        m = P.pattern_mask(M, nd)
        m[:16] = False
        return m
    if which == "last point only":
        m = torch.zeros(M, nd, dtype=torch.bool)
        m[M - 1] = _raw_pattern(M, nd)[M - 1]
        m[M - 1, nd - 1] = True
        return m
    return torch.ones(M, nd, dtype=torch.bool)


def _selection(which, M, nd, dev):
    """The selection of a mask, or None where the mask selects nothing — which ``GradientSelection`` must refuse."""
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import GradientSelection

    m = _mask(which, M, nd)
    if not bool(m.any()):
        with pytest.raises(GppError, match="at least one"):
            GradientSelection(m, dev)
        return None
    s = GradientSelection(m, dev)
    assert s.q == int(m.sum()) and int(s.first[-1]) == s.q
    return s


def _inputs(Ma, Mb, D, d0, nd, kind):
    rng = np.random.default_rng(1000 * Ma + 10 * Mb + D + 7 * kind)
    Ua, Ub = rng.uniform(-1.0, 1.0, (Ma, D)), rng.uniform(-1.0, 1.0, (Mb, D))
    w = rng.uniform(0.2, 2.0, D) / D
    if Ma > 1:
        Ua[Ma - 1] = Ub[min(3, Mb - 1)]  # a coincident pair
    return Ua, Ub, w, 1.3


def _guarded(rows, cols, dev):
    ld = (cols + 1) // 2 * 2 + 2
    flat = torch.full((2 * GUARD + rows * ld,), SENTINEL, dtype=torch.float64, device=dev)
    return flat, flat[GUARD:GUARD + rows * ld].view(rows, ld), ld


def _dev(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check_window(flat, buf, cols, what):
    assert bool((buf[:, cols:] == SENTINEL).all()), f"{what}: padding columns were written"
    assert bool((flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all()), f"{what}: guard band was written"
    assert bool(torch.isfinite(buf[:, :cols]).all()), what


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("M,N,D,d0,nd,d_split", DX_CASES)
def test_cross_kernel_dx_sel_is_the_dense_block_gathered(gpu_ctx, M, N, D, d0, nd, d_split, kind):
    dev = gpu_ctx.device
    Ua, Ub, w, sf2 = _inputs(M, N, D, d0, nd, kind)
    dUa, dUb, dw, ds = _dev(Ua, dev), _dev(Ub, dev), _dev(w, dev), _dev([sf2], dev)
    dflat, dbuf, _ = _guarded(N, M * nd, dev)
    gpu_ctx.cross_kernel_dx(dUa, dUb, dw, ds, d0, nd, dbuf[:, :M * nd], kind=kind, d_split=d_split)
    dense = dbuf[:, :M * nd].clone()
    for which in MASKS:
        sel = _selection(which, M, nd, dev)
        if sel is None:
            continue
        runs = []
        for _ in range(2):
            flat, buf, ld = _guarded(N, sel.q, dev)
            gpu_ctx.cross_kernel_dx(dUa, dUb, dw, ds, d0, nd, buf[:, :sel.q], kind=kind, d_split=d_split, sel=sel)
            torch.cuda.synchronize()
            runs.append(flat)
        _check_window(flat, buf, sel.q, which)
        assert torch.equal(_bits(buf[:, :sel.q]), _bits(dense[:, sel.flat])), f"{which}: not the dense columns gathered"
        assert torch.equal(_bits(runs[0]), _bits(runs[1])), f"{which}: two launches differ"
        if which == "all":
            assert torch.equal(_bits(flat), _bits(dflat)), "the full selection is not the dense buffer"


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("Ma,Mb,D,d0,nd,d_split", HX_CASES)
def test_kernel_dxdx_sel_is_the_dense_block_gathered(gpu_ctx, Ma, Mb, D, d0, nd, d_split, kind):
    dev = gpu_ctx.device
    Ua, Ub, w, sf2 = _inputs(Ma, Mb, D, d0, nd, kind)
    dUa, dUb, dw, ds = _dev(Ua, dev), _dev(Ub, dev), _dev(w, dev), _dev([sf2], dev)
    dflat, dbuf, _ = _guarded(Ma * nd, Mb * nd, dev)
    gpu_ctx.kernel_dxdx(dUa, dUb, dw, ds, d0, nd, dbuf[:, :Mb * nd], kind=kind, d_split=d_split)
    dense = dbuf[:, :Mb * nd].clone()
    for which in MASKS:
        sa, sb = _selection(which, Ma, nd, dev), _selection(which, Mb, nd, dev)
        for side, (ra, cb) in {"rows": (sa, None), "columns": (None, sb), "both": (sa, sb)}.items():
            if (side != "columns" and sa is None) or (side != "rows" and sb is None):
                continue
            rows = Ma * nd if ra is None else ra.q
            cols = Mb * nd if cb is None else cb.q
            runs = []
            for _ in range(2):
                flat, buf, ld = _guarded(rows, cols, dev)
                gpu_ctx.kernel_dxdx(dUa, dUb, dw, ds, d0, nd, buf[:, :cols], kind=kind, d_split=d_split, sel_a=ra, sel_b=cb)
                torch.cuda.synchronize()
                runs.append(flat)
            what = f"{which}, selection on {side}"
            _check_window(flat, buf, cols, what)
            want = dense
            if ra is not None:
                want = want[ra.flat]
            if cb is not None:
                want = want[:, cb.flat]
            assert torch.equal(_bits(buf[:, :cols]), _bits(want)), f"{what}: not the dense block gathered"
            assert torch.equal(_bits(runs[0]), _bits(runs[1])), f"{what}: two launches differ"
            if which == "all":
                assert torch.equal(_bits(flat), _bits(dflat)), f"{what}: the full selection is not the dense buffer"


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_kernel_dxdx_sel_is_bitwise_symmetric_on_equal_rows(gpu_ctx, kind):
    dev = gpu_ctx.device
    M, D, d0, nd, d_split = 37, 6, 1, 5, 3
    Ua, _, w, sf2 = _inputs(M, M, D, d0, nd, kind)
    Ua[5] = Ua[20]
    dU, dw, ds = _dev(Ua, dev), _dev(w, dev), _dev([sf2], dev)
    for which in ("pattern", "first tile empty"):
        sel = _selection(which, M, nd, dev)
        flat, buf, ld = _guarded(sel.q, sel.q, dev)
        gpu_ctx.kernel_dxdx(dU, dU.clone(), dw, ds, d0, nd, buf[:, :sel.q], kind=kind, d_split=d_split, sel_a=sel, sel_b=sel)
        torch.cuda.synchronize()
        _check_window(flat, buf, sel.q, which)
        H = buf[:, :sel.q].contiguous()
        assert torch.equal(_bits(H), _bits(H.T)), f"{which}: H is not bitwise symmetric"


# ---- gpp_gek_grad_reduce_sel ---------------------------------------------------------------------------------------------------------
#: N, Mg, D, d0, nd, dU, coincident points: the shapes of tests/test_gpu_gek_train_kernel.py
SHAPES = [(1, 1, 1, 0, 1, 0, False), (16, 16, 3, 2, 1, 0, False), (37, 19, 5, 2, 3, 2, True), (130, 33, 9, 1, 8, 1, True),
          (40, 17, 20, 8, 12, 4, False)]
_refs = {}


def _d_split(d0, nd):
    return d0 + (1 if nd >= 3 else 0)


def _reduce_mask(Mg, nd):
    """The raw pattern (points without an entry where it leaves them so), and point 1 emptied where there are three or more."""
    m = _raw_pattern(Mg, nd)
    if Mg >= 3:
        m[1] = False
    if not bool(m.any()):
        m[0, 0] = True
    return m


def _reduce_inputs(shape, kind, mask):
    N, Mg, D, d0, nd, dU, coincide = shape
    rng = np.random.default_rng(100 * N + 10 * Mg + D + 7 * kind)
    U, Ug = rng.uniform(-1.0, 1.0, (N, D)), rng.uniform(-1.0, 1.0, (Mg, D))
    if coincide:
        Ug[0] = U[3]
        Ug[1] = U[3]
        Ug[Mg - 1] = Ug[5]
        Ug[7] = U[N - 1]
    w = rng.uniform(0.2, 2.0, D) / D
    n = N + int(mask.sum())
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    return tuple(torch.tensor(np.ascontiguousarray(a)) for a in (U, Ug, w, A + A.T, rng.standard_normal(n))) + (1.3,)


def _reduce_reference(shape, kind):
    """(mask, inputs, reference sums, floor) once per (shape, kind): ``block_sums`` on W = (alpha alpha' - Kinv) / 2 of the compact
    operands scattered into the dense (N + Mg nd)^2 layout; the floor is the same with the points of both sets reversed."""
    key = (shape, kind)
    if key not in _refs:
        N, Mg, D, d0, nd, dU, _ = shape
        mask = _reduce_mask(Mg, nd)
        U, Ug, w, Kinv, alpha, sf2 = inp = _reduce_inputs(shape, kind, mask)
        idx = torch.cat([torch.arange(N), N + mask.reshape(-1).nonzero().reshape(-1)])
        W = torch.zeros(N + Mg * nd, N + Mg * nd, dtype=torch.float64)
        W[idx[:, None], idx[None, :]] = 0.5 * (torch.outer(alpha, alpha) - Kinv)
        ds = _d_split(d0, nd)
        ref = T.block_sums(U, Ug, w, sf2, kind, ds, d0, nd, W, dU)
        pi, pa = torch.arange(N - 1, -1, -1), torch.arange(Mg - 1, -1, -1)
        perm = torch.cat([pi, N + (pa[:, None] * nd + torch.arange(nd)[None, :]).reshape(-1)])
        alt = T.block_sums(U[pi], Ug[pa], w, sf2, kind, ds, d0, nd, W[perm][:, perm], dU)
        floor = max(((alt[0] - ref[0]).abs().max() / ref[0].abs().max()).item(), (abs(alt[1] - ref[1]) / abs(ref[1])).item())
        if dU:
            floor = max(floor, ((alt[2][pi] - ref[2]).abs().max() / ref[2].abs().max()).item(),
                        ((alt[3][pa] - ref[3]).abs().max() / ref[3].abs().max()).item())
        _refs[key] = (mask, inp, ref, floor)
    return _refs[key]


def _reduce_run(ctx, shape, kind, inp, sel, prefill=None):
    from gpplus_amd.backend import square_buffer

    N, Mg, D, d0, nd, dU, _ = shape
    U, Ug, w, Kinv, alpha, sf2 = inp
    dev = ctx.device
    n = Kinv.shape[0]
    buf = square_buffer(n, dev)
    buf.copy_(Kinv.to(dev))
    buf += torch.full((n, n), float("nan"), dtype=torch.float64, device=dev).triu(1)  # only the lower triangle may be read
    c = lambda t: t.to(dev).contiguous()  # noqa: E731
    if prefill is None:
        g_w, g_s = torch.zeros(D, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        g_U = torch.zeros(N, dU, dtype=torch.float64, device=dev) if dU else None
    else:
        g_w, g_s = c(prefill[0]).clone(), c(prefill[1]).clone()
        g_U = c(prefill[2]).clone() if dU else None
    g_Ug = torch.full((Mg, dU), float("nan"), dtype=torch.float64, device=dev) if dU else None  # written, not added to
    ctx.gek_grad_reduce(c(U), c(Ug), c(w), torch.tensor([sf2], dtype=torch.float64, device=dev), d0, nd, c(alpha), buf, dU, g_w, g_s,
                        g_U, g_Ug, kind=kind, d_split=_d_split(d0, nd), sel=sel)
    torch.cuda.synchronize()
    return g_w.cpu(), g_s.cpu(), (g_U.cpu() if dU else None), (g_Ug.cpu() if dU else None)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-Mg%d-D%d-d0%d-nd%d-dU%d" % s[:6])
def test_gek_grad_reduce_sel_against_the_block_reference(gpu_ctx, shape, kind):
    from gpplus_amd.backend import GradientSelection

    N, Mg, D, d0, nd, dU, _ = shape
    mask, inp, ref, floor = _reduce_reference(shape, kind)
    sel = GradientSelection(mask, gpu_ctx.device)
    got = _reduce_run(gpu_ctx, shape, kind, inp, sel)
    for name, g, r in zip(("g_w", "g_sf2", "g_U", "g_Ug"), got, (ref[0], ref[1].reshape(1), ref[2], ref[3])):
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), name
        scale = r.abs().max().item()
        err = (g - r).abs().max().item()
        print(f"{shape[:6]} kind={kind} q={sel.q} {name}: max error {err:.3e} = {err / scale:.3e} of max|reference| {scale:.3e}; "
              f"host floor {floor:.1e}")
        assert err <= BAR * scale, (name, err, scale)
    assert floor <= 1e-2 * BAR, floor
    if dU:
        empty = ~mask.any(1)
        assert bool((got[3][empty] == 0.0).all()), "g_Ug of a point without an entry is not an exact 0"
    again = _reduce_run(gpu_ctx, shape, kind, inp, sel)
    for g, h in zip(got, again):
        assert g is None or torch.equal(_bits(g), _bits(h)), "two calls differ"
    rng = np.random.default_rng(3)
    pre = (torch.tensor(rng.standard_normal(D)), torch.tensor(rng.standard_normal(1)), torch.tensor(rng.standard_normal((N, dU))))
    acc = _reduce_run(gpu_ctx, shape, kind, inp, sel, prefill=pre)
    assert torch.equal(acc[0], pre[0] + got[0]) and torch.equal(acc[1], pre[1] + got[1])
    if dU:
        assert torch.equal(acc[2], pre[2] + got[2]) and torch.equal(_bits(acc[3]), _bits(got[3]))


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-Mg%d-D%d-d0%d-nd%d-dU%d" % s[:6])
def test_gek_grad_reduce_sel_with_everything_selected_is_the_dense_call(gpu_ctx, shape, kind):
    from gpplus_amd.backend import GradientSelection

    N, Mg, D, d0, nd, dU, _ = shape
    mask = torch.ones(Mg, nd, dtype=torch.bool)
    inp = _reduce_inputs(shape, kind, mask)
    dense = _reduce_run(gpu_ctx, shape, kind, inp, None)
    full = _reduce_run(gpu_ctx, shape, kind, inp, GradientSelection(mask, gpu_ctx.device))
    for name, a, b in zip(("g_w", "g_sf2", "g_U", "g_Ug"), dense, full):
        assert a is None or torch.equal(_bits(a), _bits(b)), name


# ---- argument codes ------------------------------------------------------------------------------------------------------------------
def test_argument_codes_of_the_sel_entry_points(gpu_ctx):
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import OP_GEK_GRAD, GradientSelection, square_buffer

    dev = gpu_ctx.device
    Ma, Mb, D, d0, nd = 3, 9, 4, 1, 3
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)  # noqa: E731
    Ua = torch.rand(Ma, D, dtype=torch.float64, device=dev)
    Ub = torch.rand(Mb, D, dtype=torch.float64, device=dev)
    w = torch.rand(D, dtype=torch.float64, device=dev)
    sf2 = torch.ones(1, dtype=torch.float64, device=dev)
    sa, sb = GradientSelection(P.pattern_mask(Ma, nd), dev), GradientSelection(P.pattern_mask(Mb, nd), dev)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    gpu_ctx._stream()
    V = ctypes.c_void_p
    Pt = lambda t: V(t.data_ptr())  # noqa: E731

    # gpp_cross_kernel_dx_sel: Dk is Mb x sa.q (the selected side is Ua)
    assert sa.q % 2 == 1
    flat, buf, ld = _guarded(Mb, sa.q, dev)

    def dx(first=Pt(sa.first), dirs=Pt(sa.dir), q=sa.q, ptr=buf.data_ptr(), ld_=ld, h_=h):
        return lib.gpp_cross_kernel_dx_sel(h_, Pt(Ua), Ma, Pt(Ub), Mb, D, Pt(w), Pt(sf2), 1, 1, d0, nd, first, dirs, q, V(ptr), ld_)

    assert dx(h_=None) == -1
    assert dx(first=None) == -14 and dx(dirs=None) == -14                    # a pair of which one is NULL
    assert dx(q=0) == -15 and dx(q=Ma * nd + 1) == -15                       # q outside [1, M nd]
    assert dx(first=None, dirs=None, q=sa.q) == -15                          # dense on this side: q must be M nd
    assert dx(ptr=buf.data_ptr() + 8) == -16 and dx(ptr=None) == -16         # misaligned output
    assert dx(ld_=ld + 1) == -17 and dx(ld_=sa.q - 1) == -17                 # odd, or shorter than q
    torch.cuda.synchronize()
    assert bool((flat == SENTINEL).all()), "a refused gpp_cross_kernel_dx_sel wrote something"
    assert dx() == 0
    torch.cuda.synchronize()
    assert bool((buf[:, :sa.q] != SENTINEL).all()) and bool((buf[:, sa.q:] == SENTINEL).all())

    # gpp_kernel_dxdx_sel: H is sa.q x sb.q
    flat, buf, ld = _guarded(sa.q, sb.q, dev)

    def hx(fa=Pt(sa.first), da=Pt(sa.dir), qa=sa.q, fb=Pt(sb.first), db=Pt(sb.dir), qb=sb.q, ptr=buf.data_ptr(), ld_=ld, h_=h):
        return lib.gpp_kernel_dxdx_sel(h_, Pt(Ua), Ma, Pt(Ub), Mb, D, Pt(w), Pt(sf2), 2, 1, d0, nd, fa, da, qa, fb, db, qb, V(ptr), ld_)

    assert hx(h_=None) == -1
    assert hx(fa=None) == -14 and hx(da=None) == -14 and hx(fb=None) == -17 and hx(db=None) == -17
    assert hx(qa=0) == -15 and hx(qa=Ma * nd + 1) == -15 and hx(qb=0) == -18 and hx(qb=Mb * nd + 1) == -18
    assert hx(fa=None, da=None) == -15 and hx(fb=None, db=None) == -18      # a dense side with a compact count
    assert hx(ptr=buf.data_ptr() + 8) == -19 and hx(ptr=None) == -19
    assert hx(ld_=ld + 1) == -20 and hx(ld_=sb.q - (sb.q % 2) - 2) == -20
    torch.cuda.synchronize()
    assert bool((flat == SENTINEL).all()), "a refused gpp_kernel_dxdx_sel wrote something"
    assert hx() == 0
    torch.cuda.synchronize()
    assert bool((buf[:, :sb.q] != SENTINEL).all()) and bool((buf[:, sb.q:] == SENTINEL).all())

    # gpp_gek_grad_reduce_sel: N = Mb function rows, Mg = Ma gradient points
    N, Mg, n = Mb, Ma, Mb + sa.q
    alpha = z(n)
    Kinv = square_buffer(n + 2, dev)
    Kinv.zero_()
    pre = 0.5
    g_w, g_s, g_U, g_Ug = z(D) + pre, z(1) + pre, z(N, 1) + pre, z(Mg, 1) + pre
    gpu_ctx.ensure_workspace(OP_GEK_GRAD, N, Mg, D, 1)

    def gk(first=Pt(sa.first), dirs=Pt(sa.dir), q=sa.q, ptr=Kinv.data_ptr(), ld_=Kinv.stride(0), dU=1):
        return lib.gpp_gek_grad_reduce_sel(h, Pt(Ub), N, Pt(Ua), Mg, D, Pt(w), Pt(sf2), 0, 1, d0, nd, first, dirs, q, Pt(alpha), V(ptr),
                                           ld_, dU, Pt(g_w), Pt(g_s), Pt(g_U), Pt(g_Ug))

    assert gk(first=None) == -14 and gk(dirs=None) == -14
    assert gk(q=0) == -15 and gk(q=Mg * nd + 1) == -15 and gk(first=None, dirs=None) == -15
    assert gk(ptr=Kinv.data_ptr() + 8) == -17
    assert gk(ld_=Kinv.stride(0) + 1) == -18 and gk(ld_=n - 1 - (n - 1) % 2) == -18
    assert gk(dU=2) == -19
    torch.cuda.synchronize()
    for t in (g_w, g_s, g_U, g_Ug):
        assert bool((t == pre).all()), "a refused gpp_gek_grad_reduce_sel wrote something"
    assert gk() == 0
    torch.cuda.synchronize()
    # the binding refuses a selection of another shape, and a window that is not N x q, in words
    with pytest.raises(GppError, match="selection"):
        gpu_ctx.cross_kernel_dx(Ua, Ub, w, sf2, d0, nd, buf[:Mb, :sb.q], sel=sb)
    with pytest.raises(GppError, match="must be"):
        gpu_ctx.cross_kernel_dx(Ua, Ub, w, sf2, d0, nd, buf[:Mb, :sa.q + 1], sel=sa)
    with pytest.raises(GppError, match="selection"):
        gpu_ctx.kernel_dxdx(Ua, Ub, w, sf2, d0, nd, buf[:, :sb.q], sel_a=sb, sel_b=sb)

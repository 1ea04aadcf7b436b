"""gpp_predict_gen / gpp_predict_gen_batched on the GPU: the prediction from a generated cross block, batched over parameter sets.

B = 5 elements with per-element w, sf2 and (unless shared) features, scaled as ``test_gpu_gek_batched._inputs`` scales them; Linv and z
come from gpp_potrf_batched / gpp_trtri_batched / gpp_mll_reduce_batched on the kernel matrix with tau = 1e-2.  The shapes stand at
the tile edges: 64-row and 64-column tiles, chunks of 32 of the contracted index, the LDS opt-in above D = 19.  One test row equals
a training row in every shape.  Checked: every element of the batched call against the single-problem call bit for bit, two launches
bit for bit, a row of an M-row call against the M = 1 call on it bit for bit, the strictly lower triangle of Linv never read, and the
long-double reference of tests/ensemble_reference.py with the composed route (gpp_cross_kernel + gpp_predict_tn) beside it.

Bar: 1e-6 of the largest reference magnitude (``BAR`` of tests/test_gpu_gek_batched.py); the variance is judged relative to sf2_b,
since var itself is near tau at the coincident row.  Every comparison prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_reference as E  # noqa: E402

pytestmark = pytest.mark.gpu

B = 5
BAR = 1e-6
TAU = 1e-2
DT = torch.float64

#: N, M, D, kind, d_split, shared U
SHAPES = [
    (30, 1, 4, E.KIND_RBF, 0, False),         # one partial tile, one test row
    (64, 64, 1, E.KIND_RBF, 0, True),         # exactly one tile each way, one feature
    (65, 63, 6, E.KIND_MATERN52, 2, False),   # a second column tile of one column; both factors
    (77, 65, 12, E.KIND_MATERN32, 1, True),   # a second row tile of one row; a partial chunk
    (130, 130, 24, E.KIND_RBF, 0, False),     # three tiles each way; more than 48 KiB of LDS
]
_IDS = ["N%d-M%d-D%d" % s[:3] for s in SHAPES]
_cache = {}


def _bits(t):
    return t.contiguous().view(torch.int64)


def _inputs(shape):
    """The B elements of a shape as CPU tensors and their long-double reference, made once and left unchanged."""
    if shape not in _cache:
        N, M, D, kind, d_split, shared = shape
        rng = np.random.default_rng(1000 * N + 10 * M + D)
        U0, Ua0 = torch.tensor(rng.uniform(-1.0, 1.0, (N, D))), torch.tensor(rng.uniform(-1.0, 1.0, (M, D)))
        Ua0[0] = U0[3]  # a test row that is a training row
        w0 = torch.tensor(rng.uniform(0.2, 2.0, D) / D)
        scale = lambda b: 1.0 + 0.02 * b  # noqa: E731
        U = U0.clone() if shared else torch.stack([U0 * scale(b) for b in range(B)])
        Ua = Ua0.clone() if shared else torch.stack([Ua0 * scale(b) for b in range(B)])
        w = torch.stack([w0 * (0.6 + 0.2 * b) for b in range(B)])
        sf2 = torch.tensor([1.3 * (0.5 + 0.25 * b) for b in range(B)], dtype=DT)
        r = torch.tensor(rng.standard_normal((B, N)))
        el = lambda t, b: t if t.dim() == 2 else t[b]  # noqa: E731
        ref = [E.member(el(Ua, b).numpy(), el(U, b).numpy(), w[b].numpy(), float(sf2[b]), np.full(N, TAU), r[b].numpy(), kind, d_split)
               for b in range(B)]
        _cache[shape] = dict(U=U, Ua=Ua, w=w, sf2=sf2, r=r, mean=np.stack([m for m, _, _ in ref]), var=np.stack([v for _, v, _ in ref]),
                             z=np.stack([z for _, _, z in ref]))
    return _cache[shape]


class _Problem:
    """The operands of a shape on the device, factored by the batched entry points."""

    def __init__(self, ctx, shape):
        from gpplus_amd.backend import UPLO_UPPER
        from gpplus_amd.batched import _even_elements

        N, M, D, kind, d_split, shared = shape
        inp = _inputs(shape)
        dev = ctx.device
        c = lambda t: t.to(dev).contiguous()  # noqa: E731
        self.shape, self.inp, self.ctx = shape, inp, ctx
        self.U, self.Ua = _even_elements(c(inp["U"])), _even_elements(c(inp["Ua"]))
        self.w, self.sf2 = c(inp["w"]), c(inp["sf2"])
        A, self.Li, T = (ctx.batched_buffer(B, N) for _ in range(3))
        self.Li.fill_(0.0)
        r, self.z = ctx.batched_vector(B, N), ctx.batched_vector(B, N)
        r.copy_(c(inp["r"]))
        info = torch.zeros(B, dtype=torch.int32, device=dev)
        tau = torch.full((B, 1), TAU, dtype=DT, device=dev)
        ctx.kernel_build_batched(self.U, self.w, self.sf2, tau, None, A, kind=kind, d_split=d_split, uplo=UPLO_UPPER)
        ctx.potrf_batched(A, self.Li, info)
        ctx.trtri_batched(A, self.Li, T)
        ctx.mll_reduce_batched(A, self.Li, r, self.z, torch.empty(B, 3, dtype=DT, device=dev))
        assert info.tolist() == [0] * B

    def el(self, t, b):
        return t if t.dim() == 2 else t[b]

    def batched(self, Li=None, nb=B):
        N, M, D, kind, d_split, shared = self.shape
        mo, vo = self.ctx.batched_vector(nb, M), self.ctx.batched_vector(nb, M)
        mo.fill_(float("nan"))
        vo.fill_(float("nan"))
        Ua = self.Ua if self.Ua.dim() == 2 else self.Ua[:nb]
        U = self.U if self.U.dim() == 2 else self.U[:nb]
        self.ctx.predict_gen_batched(Ua, U, self.w[:nb], self.sf2[:nb], (self.Li if Li is None else Li)[:nb], self.z[:nb], mo, vo,
                                     kind=kind, d_split=d_split)
        return mo, vo

    def single(self, b, rows=None):
        N, M, D, kind, d_split, shared = self.shape
        Ua = self.el(self.Ua, b)
        Ua = Ua if rows is None else Ua[rows].contiguous()
        mo, vo = (torch.full((Ua.shape[0],), float("nan"), dtype=DT, device=self.ctx.device) for _ in range(2))
        self.ctx.predict_gen(Ua, self.el(self.U, b), self.w[b], self.sf2[b:b + 1], self.Li[b], self.z[b], mo, vo, kind=kind,
                             d_split=d_split)
        return mo, vo

    def composed(self, b):
        from gpplus_amd.backend import rows_buffer

        N, M, D, kind, d_split, shared = self.shape
        dev = self.ctx.device
        Kns, V = rows_buffer(N, M, dev), rows_buffer(M, N, dev)
        mo, vo = (torch.empty(M, dtype=DT, device=dev) for _ in range(2))
        self.ctx.cross_kernel(self.el(self.U, b), self.el(self.Ua, b), self.w[b], self.sf2[b:b + 1], Kns, kind=kind, d_split=d_split)
        self.ctx.predict_tn(self.Li[b], self.z[b], Kns, self.sf2[b:b + 1].expand(M).contiguous(), V, mo, vo)
        return mo, vo


@pytest.fixture(scope="module", params=SHAPES, ids=_IDS)
def problem(request, gpu_ctx):
    return _Problem(gpu_ctx, request.param)


def test_batched_elements_equal_the_single_problem_call_and_two_launches_agree(problem):
    mo, vo = problem.batched()
    mo2, vo2 = problem.batched()
    assert bool(torch.isfinite(mo).all()) and bool(torch.isfinite(vo).all())
    assert torch.equal(_bits(mo), _bits(mo2)) and torch.equal(_bits(vo), _bits(vo2)), "two launches differ"
    for b in range(B):
        ms, vs = problem.single(b)
        assert torch.equal(_bits(mo[b]), _bits(ms)) and torch.equal(_bits(vo[b]), _bits(vs)), f"element {b} differs from the single call"
    # fewer elements in the launch: the same bits for those that remain
    m3, v3 = problem.batched(nb=2)
    assert torch.equal(_bits(m3), _bits(mo[:2])) and torch.equal(_bits(v3), _bits(vo[:2]))


def test_a_row_does_not_depend_on_the_other_rows_of_the_call(problem):
    M = problem.shape[1]
    b = B - 1
    mo, vo = problem.single(b)
    for a in sorted({0, M // 2, M - 1, min(63, M - 1), min(64, M - 1)}):
        m1, v1 = problem.single(b, rows=slice(a, a + 1))
        assert torch.equal(_bits(m1), _bits(mo[a:a + 1])) and torch.equal(_bits(v1), _bits(vo[a:a + 1])), f"row {a}"


def test_only_the_mirror_in_the_upper_triangle_is_read(problem):
    N = problem.shape[0]
    mo, vo = problem.batched()
    Li = problem.ctx.batched_buffer(B, N)
    Li.copy_(problem.Li)
    Li += torch.full((N, N), float("nan"), dtype=DT, device=Li.device).tril(-1)
    assert N == 1 or bool(torch.isnan(Li[:, 1:, 0]).all())
    mn, vn = problem.batched(Li=Li)
    assert torch.equal(_bits(mn), _bits(mo)) and torch.equal(_bits(vn), _bits(vo))


def test_against_the_long_double_reference_with_the_composed_route_beside_it(problem):
    inp = problem.inp
    mo, vo = problem.batched()
    z_err = float(np.abs(problem.z.cpu().numpy().astype(E.LD) - inp["z"]).max() / np.abs(inp["z"]).max())
    worst = dict(fm=0.0, fv=0.0, cm=0.0, cv=0.0)
    for b in range(B):
        mc, vc = problem.composed(b)
        scale_m, sf2 = float(np.abs(inp["mean"][b]).max()), float(inp["sf2"][b])
        err = lambda t, key: float(np.abs(t.cpu().numpy().astype(E.LD) - inp[key][b]).max())  # noqa: E731
        fm, fv, cm, cv = err(mo[b], "mean") / scale_m, err(vo[b], "var") / sf2, err(mc, "mean") / scale_m, err(vc, "var") / sf2
        print(f"{problem.shape[:3]} element {b}: fused mean {fm:.3e} var {fv:.3e} | composed mean {cm:.3e} var {cv:.3e} "
              f"(of max |mean| {scale_m:.3e}, sf2 {sf2:.3f}; var at the coincident row {float(inp['var'][b][0]):.3e})")
        for k, v in zip(("fm", "fv", "cm", "cv"), (fm, fv, cm, cv)):
            worst[k] = max(worst[k], v)
    print(f"{problem.shape[:3]} worst: fused mean {worst['fm']:.3e} var {worst['fv']:.3e}, composed mean {worst['cm']:.3e} "
          f"var {worst['cv']:.3e}; z against long double {z_err:.3e}")
    assert worst["fm"] <= BAR and worst["fv"] <= BAR


def test_argument_errors_and_a_missing_workspace(gpu_ctx):
    from gpplus_amd._lib import GppError
    from gpplus_amd.backend import NO_WORKSPACE

    P = _Problem(gpu_ctx, SHAPES[2])  # N = 65, M = 63, D = 6: per-element features
    N, M, D, kind, d_split, _ = P.shape
    lib, h, dev = gpu_ctx.lib, gpu_ctx.h, gpu_ctx.device
    elib = gpu_ctx._ensemble_lib()  # the two entry points live in libgpp_ensemble_hip.so, on the handle of libgpp_hip.so
    mo, vo = gpu_ctx.batched_vector(B, M), gpu_ctx.batched_vector(B, M)
    good = dict(h=h, Ua=P.Ua.data_ptr(), sUa=P.Ua.stride(0), M=M, Ub=P.U.data_ptr(), sUb=P.U.stride(0), N=N, D=D, w=P.w.data_ptr(),
                sf2=P.sf2.data_ptr(), kind=kind, d_split=d_split, Linv=P.Li.data_ptr(), ldi=P.Li.stride(1), sLi=P.Li.stride(0),
                z=P.z.data_ptr(), sv=P.z.stride(0), mean=mo.data_ptr(), var=vo.data_ptr(), so=mo.stride(0), batch=B)
    assert good["sUa"] % 2 == 0 and good["sUb"] % 2 == 0

    def raw(**change):
        return elib.gpp_predict_gen_batched(*{**good, **change}.values())

    gpu_ctx._ensure_predict_gen_workspace(N, M, B)
    mo.fill_(float("nan"))
    codes = [(-1, dict(h=None)), (-2, dict(Ua=None)), (-3, dict(sUa=good["sUa"] + 1)), (-3, dict(sUa=-2)), (-4, dict(M=0)),
             (-5, dict(Ub=None)), (-6, dict(sUb=N * D + 1)), (-7, dict(N=0)), (-8, dict(D=0)), (-8, dict(D=65)), (-9, dict(w=None)),
             (-10, dict(sf2=None)), (-11, dict(kind=3)), (-12, dict(d_split=D + 1)), (-13, dict(Linv=None)),
             (-14, dict(Linv=good["Linv"] + 8)), (-14, dict(ldi=good["ldi"] + 1)), (-14, dict(ldi=N - 1)), (-15, dict(sLi=good["sLi"] + 1)),
             (-16, dict(z=None)), (-16, dict(z=good["z"] + 8)), (-17, dict(sv=good["sv"] + 1)), (-17, dict(sv=N - 1)),
             (-18, dict(mean=None)), (-19, dict(var=None)), (-20, dict(so=good["so"] + 1)), (-20, dict(so=M - 1)), (-21, dict(batch=0)),
             (-21, dict(batch=65536))]
    for code, change in codes:
        assert raw(**change) == code, (code, change)
    one = dict(h=h, Ua=P.Ua.data_ptr(), M=M, Ub=P.U.data_ptr(), N=N, D=D, w=P.w.data_ptr(), sf2=P.sf2.data_ptr(), kind=kind,
               d_split=d_split, Linv=P.Li.data_ptr(), ldi=P.Li.stride(1), z=P.z.data_ptr(), mean=mo.data_ptr(), var=vo.data_ptr())
    for code, change in [(-3, dict(M=0)), (-5, dict(N=0)), (-6, dict(D=65)), (-9, dict(kind=-1)), (-12, dict(ldi=one["ldi"] + 1)),
                         (-13, dict(z=one["z"] + 8)), (-15, dict(var=None))]:
        assert elib.gpp_predict_gen(*{**one, **change}.values()) == code, (code, change)
    # too small a workspace, or none: the entry point reports it and enqueues nothing
    need = elib.gpp_predict_gen_workspace_bytes(N, M, B)
    assert need == B * 2 * M * 2 * 8
    small = torch.empty(B * 2 * M * 2 * 8 - 16, dtype=torch.uint8, device=dev)
    try:
        assert lib.gpp_set_workspace(h, small.data_ptr(), small.numel()) == 0
        assert raw() == NO_WORKSPACE
        assert lib.gpp_set_workspace(h, None, 0) == 0
        assert raw() == NO_WORKSPACE
        assert elib.gpp_predict_gen(*one.values()) == NO_WORKSPACE
    finally:
        gpu_ctx._ws = None  # the context attaches a workspace of its own at the next call that needs one
        lib.gpp_set_workspace(h, None, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(mo).all()), "a refused call wrote its output"
    # the binding's own checks, and the same operands run once they are right
    with pytest.raises(GppError, match="even row stride"):
        gpu_ctx.predict_gen_batched(P.Ua, P.U, P.w, P.sf2, P.Li, P.z, torch.empty(B, M, dtype=DT, device=dev),
                                    torch.empty(B, M, dtype=DT, device=dev), kind=kind, d_split=d_split)
    with pytest.raises(GppError, match="contiguous"):
        gpu_ctx.predict_gen_batched(P.Ua[:, :, :D - 1], P.U[:, :, :D - 1], P.w[:, :D - 1].contiguous(), P.sf2, P.Li, P.z, mo, vo)
    with pytest.raises(GppError, match=r"z must be"):
        gpu_ctx.predict_gen_batched(P.Ua, P.U, P.w, P.sf2, P.Li, P.z[:, :N - 1], mo, vo, kind=kind, d_split=d_split)
    assert raw() == NO_WORKSPACE  # (still none attached)
    # a noise-group index of another length than N (a likelihood left with the test rows' sources) is refused by the batched build
    # on the host: the kernels index it unchecked
    A = gpu_ctx.batched_buffer(B, N)
    with pytest.raises(GppError, match="stale fidel_indices"):
        gpu_ctx.kernel_build_batched(P.U, P.w, P.sf2, torch.full((B, 2), TAU, dtype=DT, device=dev),
                                     torch.zeros(N - 5, dtype=torch.int32, device=dev), A, kind=kind, d_split=d_split)
    gpu_ctx.predict_gen_batched(P.Ua, P.U, P.w, P.sf2, P.Li, P.z, mo, vo, kind=kind, d_split=d_split)
    ref, _ = P.batched()
    assert torch.equal(_bits(mo), _bits(ref))

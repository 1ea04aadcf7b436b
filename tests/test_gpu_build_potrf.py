"""``gpp_build_potrf_ws``: the covariance build and the factorisation as one call — most of Ky written beside the first panel where
the ticket list runs — must leave byte for byte what ``gpp_kernel_build`` + ``gpp_potrf_ws`` leave: the same kernels on the same
values.  6912 is the list's first size, 7000 a ragged one, 3000 takes the fallback (the two plain calls)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [6912, 7000, 3000]


def _sq(n):
    from gpplus_amd.backend import square_buffer

    m = square_buffer(n, "cuda")
    m.fill_(float("nan"))
    return m


def _bits(t):
    return t.contiguous().view(torch.int64)


def _inputs(n, d=6, tau=(2e-2, 5e-2), seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + n)
    U = torch.rand(n, d, generator=g, dtype=torch.float64).cuda()
    w = (torch.rand(d, generator=g, dtype=torch.float64) * 0.5 + 0.1).cuda()
    sf2 = torch.tensor([0.9], dtype=torch.float64, device="cuda")
    tau = torch.tensor(tau, dtype=torch.float64, device="cuda")
    grp = (torch.arange(n, device="cuda") % tau.numel()).to(torch.int32)
    return U, w, sf2, tau, grp


@pytest.fixture(autouse=True)
def _list_on(gpu_ctx):
    """The shared context may have had its ticket list or cooperative panel switched off by an earlier test's time-out recovery:
    these tests are about the list's path, so both are on here, and put back afterwards."""
    from gpplus_amd.backend import OPT_COOP_PANEL, OPT_DAG_SCHED

    was = (gpu_ctx.coop_panel, gpu_ctx.dag_sched)
    gpu_ctx.set_option(OPT_COOP_PANEL, 1)
    gpu_ctx.set_option(OPT_DAG_SCHED, 1)
    yield
    gpu_ctx.set_option(OPT_COOP_PANEL, int(was[0]))
    gpu_ctx.set_option(OPT_DAG_SCHED, int(was[1]))


def _split_builds(ctx):
    """Calls of gpp_build_potrf_ws on this handle that built Ky split around panel 0 (a debug entry, not part of gpp.h)."""
    import ctypes

    f = ctx.lib.gpp_debug_split_builds
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p]
    return int(f(ctx.h))


def _both(ctx, n, U, w, sf2, tau, grp, jitter=0.0):
    """(A, Linv, info) of the two plain calls and of the single one, each into NaN-filled buffers of its own.  The single call
    must really have taken the path its size stands for: the split build from 6912 rows on, the two plain calls below."""
    out = []
    for fused in (False, True):
        A, Li, T = _sq(n), _sq(n), _sq(n)
        info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        if fused:
            before = _split_builds(ctx)
            ctx.build_potrf(U, w, sf2, tau, grp, A, Li, info, T, jitter=jitter)
            assert _split_builds(ctx) - before == (1 if n >= 6912 else 0)
        else:
            ctx.kernel_build(U, w, sf2, tau, grp, A, jitter=jitter, uplo=2)
            ctx.potrf(A, Li, info, T)
        torch.cuda.synchronize()
        out.append((A, Li, info))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_same_bytes_as_the_two_calls(gpu_ctx, n):
    U, w, sf2, tau, grp = _inputs(n)
    (A0, L0, i0), (A1, L1, i1) = _both(gpu_ctx, n, U, w, sf2, tau, grp)
    assert int(i0.item()) == 0 and int(i1.item()) == 0
    assert torch.equal(_bits(A0), _bits(A1))
    assert torch.equal(_bits(L0), _bits(L1))
    # and it is a factor of Ky: the first rows of U^T U against the kernel's definition
    k = 64
    Uf = torch.triu(A1)[:, :]
    d2 = ((U[:k, None, :] - U[None, :, :]) ** 2 * w).sum(-1)
    Ky = 0.9 * torch.exp(-d2)
    Ky[torch.arange(k), torch.arange(k)] += tau[grp[:k].long()]
    torch.testing.assert_close(Uf[:k, :k].T @ Uf[:k, :], Ky, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("n", SIZES)
def test_not_positive_definite_reports_the_same_minor(gpu_ctx, n):
    U, w, sf2, tau, grp = _inputs(n, tau=(2e-2, -5.0))
    first_bad = n // 2 + 37
    grp = (torch.arange(n, device="cuda") >= first_bad).to(torch.int32)  # the noise turns negative at row first_bad
    (_, _, i0), (_, _, i1) = _both(gpu_ctx, n, U, w, sf2, tau, grp)
    assert int(i0.item()) == int(i1.item()) == first_bad + 1


@pytest.mark.parametrize("n", SIZES)
def test_jitter_lands_on_the_diagonal(gpu_ctx, n):
    U, w, sf2, tau, grp = _inputs(n)
    jitter = 0.25
    (A0, L0, i0), (A1, L1, i1) = _both(gpu_ctx, n, U, w, sf2, tau, grp, jitter=jitter)
    assert int(i0.item()) == 0 and int(i1.item()) == 0
    assert torch.equal(_bits(A0), _bits(A1))
    assert torch.equal(_bits(L0), _bits(L1))
    # U_00 = sqrt(Ky_00), and row 0 of U^T U carries the jitter in its first entry only
    assert abs(float(A1[0, 0]) ** 2 - (0.9 + float(tau[0]) + jitter)) <= 1e-14
    last = n - 1
    col = torch.triu(A1)[:, last]
    assert abs(float(col @ col) - (0.9 + float(tau[int(grp[last])]) + jitter)) <= 1e-12


def test_under_capture_it_is_the_two_calls(gpu_ctx):
    """Recorded into a HIP graph (the single-stream factorisation's sizes, as gp-plus_amd/graphed.py captures it) the call builds
    all of Ky on the capturing stream and factors it: a replay leaves the bytes of the eager pair, and no split build is counted."""
    n = 1000
    U, w, sf2, tau, grp = _inputs(n)
    A0, L0, T0 = _sq(n), _sq(n), _sq(n)
    i0 = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    gpu_ctx.kernel_build(U, w, sf2, tau, grp, A0, uplo=2)
    gpu_ctx.potrf(A0, L0, i0, T0)
    A1, L1, T1 = _sq(n), _sq(n), _sq(n)
    i1 = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: one-time checks and attributes outside the capture
        gpu_ctx.build_potrf(U, w, sf2, tau, grp, A1, L1, i1, T1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in (A1, L1, T1):
        t.fill_(float("nan"))
    i1.fill_(-7)
    before = _split_builds(gpu_ctx)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gpu_ctx.build_potrf(U, w, sf2, tau, grp, A1, L1, i1, T1)
    assert _split_builds(gpu_ctx) == before
    torch.cuda.synchronize()
    assert bool(torch.isnan(A1).all())  # recorded, not run
    graph.replay()
    torch.cuda.synchronize()
    assert int(i0.item()) == 0 and int(i1.item()) == 0
    assert torch.equal(_bits(A0), _bits(A1))
    assert torch.equal(_bits(L0), _bits(L1))

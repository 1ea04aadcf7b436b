"""Pathwise posterior draws at N training points of the C2 generator (d = 8), S paths on F random features, factor cached:
  construction    PosteriorPaths (random numbers on the CPU, gpp_rff_apply at the training features, the two triangular products);
  paths(X)        per stage — model forward (features, prior mean), gpp_rff_apply, gpp_kernel_apply, the add / transpose — for
                  M in {1, 1024, 65 536, 10^6};
  materialised    the update term k(X*, X) C by the existing route: gpp_cross_kernel into a row buffer, then gpp_gemm, in row chunks
                  that fit memory (the M x N block is what gpp_kernel_apply never forms);
  sample_y        GP_Plus.sample_y(size = S, X) at M = 8192, the only posterior draw there was.
Medians of ``repeats`` runs, each between two device synchronisations (stages: HIP events).  For each M the floor
max(2 M N S / 78.6 TFLOP/s, M N V / 3.9e13) is printed beside the measured kernel time, V = VALU instructions per generated
entry (``--valu``; count them in the disassembly of gpp_apply_tile).
``--grad`` times the backward of a path instead, for M in {1, 1024, 65 536}: gpp_rff_apply_grad and gpp_kernel_apply_grad (HIP events,
each kernel alone), the forward gpp_kernel_apply at the same M beside them, and the materialised route — gpp_gemm for the M x N
block Gbar C^T, then gpp_cross_grad with gvar = 1 and that block as B, in row chunks of at most 8192 — whose gradient is checked
in the same run to agree with the fused one to 1e-10 of max |g|.  Floor of gpp_kernel_apply_grad:
max(2 M N (S + D + 1) / 78.6 TFLOP/s, M N V' / 3.9e13), V' the VALU instructions per generated entry of gpp_apply_grad_tile.
usage: python tools/bench_paths.py [N] [S] [F] [repeats] [--valu V] [--max-m M] [--grad]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd.backend import rows_buffer  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402


def _opt(name, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return type(default)(v)
    return default


GRAD = "--grad" in sys.argv
if GRAD:
    sys.argv.remove("--grad")
VALU = _opt("--valu", 0.0)
MAX_M = _opt("--max-m", 1000000)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
S = int(sys.argv[2]) if len(sys.argv) > 2 else 64
F = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 5


def median_ms(fn, reps=REPS, warm=1):
    ts = []
    for r in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2]


def event_ms(fn, reps=REPS, warm=1):
    """Median device time of what ``fn`` enqueues."""
    ts = []
    for r in range(reps + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


X, y, kw, theta = make_config("C2", N)
m = GP_Plus(X, y, dtype=torch.float64, device="cuda", **kw)
apply_theta(m, theta)
m.eval()
with torch.no_grad():
    m(m.train_inputs[0][:4])  # the factor cache
torch.cuda.synchronize()
print(f"N={N} d={X.shape[1]} S={S} F={F}, medians of {REPS} [ms]")
gen = torch.Generator().manual_seed(0)
t_build = median_ms(lambda: m.sample_paths(size=S, num_features=F, generator=gen))
paths = m.sample_paths(size=S, num_features=F, generator=gen)
print(f"construction (factor cached)                       {t_build:10.3f}")

gctx, spec = paths.gctx, paths.spec
lo, hi = X.min(0)[0], X.max(0)[0]


def grad_section():
    D = X.shape[1]
    Cb = rows_buffer(N, S, "cuda")
    Cb.copy_(paths.coef)
    for M in (1, 1024, 65536):
        if M > MAX_M:
            continue
        Us = (lo + (hi - lo) * torch.rand(M, D, dtype=torch.float64, generator=torch.Generator().manual_seed(M))).cuda().contiguous()
        gbar = torch.randn(M, S, dtype=torch.float64, generator=torch.Generator().manual_seed(M + 1)).cuda()
        buf = torch.empty(M, S, dtype=torch.float64, device="cuda")
        g = torch.empty(M, D, dtype=torch.float64, device="cuda")
        t_fwd = event_ms(lambda: gctx.kernel_apply(Us, paths.U, spec.w, paths._sf2, paths.coef, buf, kind=spec.kind, d_split=spec.d_split))
        t_rff = event_ms(lambda: gctx.rff_apply_grad(Us, paths.omega, paths.phase, paths._sf2, paths.theta, gbar, g))
        t_ker = event_ms(lambda: gctx.kernel_apply_grad(Us, paths.U, spec.w, paths._sf2, paths.coef, gbar, g, kind=spec.kind,
                                                        d_split=spec.d_split))
        fused = g.clone()  # the kernel term alone (beta = 0)
        mc = min(M, 8192)
        Bb, ones = rows_buffer(mc, N, "cuda"), torch.ones(mc, dtype=torch.float64, device="cuda")
        gm = torch.empty(M, D, dtype=torch.float64, device="cuda")

        def materialised(i0=0):
            gctx.gemm(0, 1, mc, N, S, 1.0, gbar[i0:i0 + mc], Cb, 0.0, Bb)
            gctx.cross_grad(Us[i0:i0 + mc], paths.U, spec.w, paths._sf2, None, None, ones, Bb, gm[i0:i0 + mc], None, None, None,
                            kind=spec.kind, d_split=spec.d_split)

        t_mat = (M / mc) * event_ms(materialised)
        for i0 in range(0, M, mc):  # (M is a multiple of the chunk)
            materialised(i0)
        torch.cuda.synchronize()
        err = (fused - gm).abs().max().item() / gm.abs().max().item()
        floor_mfma = 1e3 * 2.0 * M * N * (S + D + 1) / 78.6e12
        line = (f"backward M={M:8d}: gpp_rff_apply_grad {t_rff:9.3f}   gpp_kernel_apply_grad {t_ker:10.3f}   forward gpp_kernel_apply "
                f"{t_fwd:10.3f}   floor(kernel_apply_grad) MFMA {floor_mfma:9.3f}")
        if VALU:
            line += f" VALU {1e3 * M * N * VALU / 3.9e13:9.3f}"
        print(line + f"   materialised route {t_mat:10.3f}   fused / materialised {t_ker / t_mat:5.2f}   "
              f"max |fused - materialised| / max |g| {err:.2e}")
        if not err <= 1e-10:
            raise SystemExit("the fused and the materialised gradients differ")
        del Bb, gm, Us, gbar, buf, g


if GRAD:
    grad_section()
    sys.exit(0)
for M in (1, 1024, 65536, 1000000):
    if M > MAX_M:
        continue
    Xs = (lo + (hi - lo) * torch.rand(M, X.shape[1], dtype=torch.float64, generator=torch.Generator().manual_seed(M))).cuda()
    total = median_ms(lambda: paths.paths(Xs))
    rows = min(M, paths._chunk_rows())
    Us = Xs[:rows].contiguous()  # C2 has no categorical column: the features are the inputs
    buf = torch.empty(rows, S, dtype=torch.float64, device="cuda")
    scale = M / rows  # the stages are timed on one chunk and scaled to M rows
    t_rff = scale * event_ms(lambda: gctx.rff_apply(Us, paths.omega, paths.phase, paths._sf2, paths.theta, buf))
    t_ker = scale * event_ms(lambda: gctx.kernel_apply(Us, paths.U, spec.w, paths._sf2, paths.coef, buf, beta=1.0, kind=spec.kind,
                                                       d_split=spec.d_split))
    floor_mfma = 1e3 * 2.0 * M * N * S / 78.6e12
    floor_valu = 1e3 * M * N * VALU / 3.9e13
    line = (f"paths(X) M={M:8d}: total {total:10.3f}   gpp_rff_apply {t_rff:9.3f}   gpp_kernel_apply {t_ker:10.3f}   "
            f"forward + add {max(total - t_rff - t_ker, 0.0):8.3f}   floor(kernel_apply) MFMA {floor_mfma:9.3f}")
    if VALU:
        line += f" VALU {floor_valu:9.3f}"
    # the update term by the existing route, in row chunks of at most 8192 (8192 x N doubles = 1.3 GB at N = 20 000)
    mc = min(M, 8192)
    Ksn, out = rows_buffer(mc, N, "cuda"), rows_buffer(mc, S, "cuda")
    Cb = rows_buffer(N, S, "cuda")
    Cb.copy_(paths.coef)
    Uc = Xs[:mc].contiguous()

    def materialised():
        gctx.cross_kernel(Uc, paths.U, spec.w, paths._sf2, Ksn, kind=spec.kind, d_split=spec.d_split)
        gctx.gemm(0, 0, mc, S, N, 1.0, Ksn, Cb, 0.0, out)

    t_mat = (M / mc) * event_ms(materialised)
    print(line + f"   materialised route {t_mat:10.3f}   fused / materialised {t_ker / t_mat:5.2f}")
    del Ksn, out, Us, buf, Xs

if MAX_M >= 8192:
    Xs = (lo + (hi - lo) * torch.rand(8192, X.shape[1], dtype=torch.float64, generator=torch.Generator().manual_seed(8192))).cuda()
    t_sy = median_ms(lambda: m.sample_y(size=S, X=Xs), reps=max(1, min(REPS, 3)))
    print(f"sample_y(size={S}, X) at M=8192                      {t_sy:10.3f}")

"""Expected variance reduction (linalg.variance_reduction, gpp_post_cross_sq) at N training points of the C2 generator (d = 8) with
M_c = M_r = M candidates and reference points, M in {1024, 4096, 16384}.  Times, each the median of the repeats after warm-up, between
two device synchronisations, on the V = K_*N Linv^T of ``predict_from_cache`` (made once per M, outside the timings):
  (a) the fused launch, gpp_post_cross_sq, in both operand forms: NT on V (points x N) and TN on V^T (N x points);
  (b) the composed route from entry points that were there before: ``cross_kernel`` into an M x M block, the library GEMM on it with
      alpha = -1, beta = 1, then the weighted square-and-row-sum in torch;
  (c) the GEMM of the same shape alone (M x M x N into an M x M block), in both forms.
Peak device memory of (a) and (b) beyond the operands (torch's allocator, which also holds the library's workspace), and one greedy
run of q = 16 picks (``linalg.variance_reduction``, everything included: both V, the 16 launches and the 15 appended coordinates).
Results of (a), both forms, and (b) are compared at every M.
usage: python tools/bench_alc.py [N] [repeats] > profiles/r11_alc_bench.txt"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.backend import rows_buffer  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

MS = (1024, 4096, 16384)
N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
X, y, kw, theta = make_config("C2", N + 2 * max(MS))
m = GP_Plus(X[:N], y[:N], dtype=torch.float64, device="cuda", **kw)
apply_theta(m, theta)
m.eval()


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * sorted(ts)[len(ts) // 2], 1e3 * min(ts), 1e3 * max(ts), out


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def line(what, t, extra=""):
    print(f"  {what:66s} {t[0]:10.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}) {extra}", flush=True)


with torch.no_grad():
    out = m.forward(X.to("cuda"))
    U = out.lazy_covariance_matrix.U1.to(torch.float64).contiguous()
    cache = m._ensure_prediction_cache()
    gctx, spec = cache.gctx, cache.spec
    w, sf2 = spec.w, spec.sf2.reshape(1)
    tau = m.likelihood.noise_covar.noise.detach().reshape(-1).to(torch.float64)
    print(f"N={N}, d={U.shape[1]}, kind={spec.kind}, {reps} repeats; flops of the product 2 M^2 N")
    for M in MS:
        print(f"-- M_c = M_r = {M}")
        Uc, Ur = U[N:N + M].contiguous(), U[N + max(MS):N + max(MS) + M].contiguous()
        omega = torch.full((M,), 1.0 / M, dtype=torch.float64, device="cuda")
        _, var_c, Vc = linalg.predict_from_cache(cache, Uc, need_V=True)
        _, _, Vr = linalg.predict_from_cache(cache, Ur, need_V=True)
        Vct, Vrt = rows_buffer(N, M, "cuda"), rows_buffer(N, M, "cuda")
        gctx.transpose(Vc, Vct)
        gctx.transpose(Vr, Vrt)
        num = torch.empty(M, dtype=torch.float64, device="cuda")
        flops = 2.0 * M * M * N

        def fused(vt):
            return gctx.post_cross_sq(Uc, Ur, w, sf2, Vct if vt else Vc, Vrt if vt else Vr, N, num, omega=omega, kind=spec.kind,
                                      d_split=spec.d_split, transposed=vt).clone()

        def composed():
            C = gctx.cross_kernel(Uc, Ur, w, sf2, rows_buffer(M, M, "cuda"), kind=spec.kind, d_split=spec.d_split)
            gctx.gemm(0, 1, M, M, N, -1.0, Vc, Vr, 1.0, C)
            return (C * C) @ omega

        Cbuf = rows_buffer(M, M, "cuda")

        def gemm_only(vt):
            if vt:
                gctx.gemm(1, 0, M, M, N, 1.0, Vct, Vrt, 0.0, Cbuf)
            else:
                gctx.gemm(0, 1, M, M, N, 1.0, Vc, Vr, 0.0, Cbuf)

        ta, tat, tb = timed(lambda: fused(False)), timed(lambda: fused(True)), timed(composed)
        tc, tct = timed(lambda: gemm_only(False)), timed(lambda: gemm_only(True))
        line("(a) fused, NT on V", ta, f"{flops / ta[0] / 1e9:7.2f} TFLOP/s")
        line("(a) fused, TN on V^T", tat, f"{flops / tat[0] / 1e9:7.2f} TFLOP/s")
        line("(b) composed: cross_kernel + GEMM (NT) + square-and-row-sum", tb)
        line("(c) GEMM alone, NT", tc, f"{flops / tc[0] / 1e9:7.2f} TFLOP/s")
        line("(c) GEMM alone, TN", tct, f"{flops / tct[0] / 1e9:7.2f} TFLOP/s")
        print(f"  ratios: (a)/(c) NT {ta[0] / tc[0]:.3f}, TN {tat[0] / tct[0]:.3f};  (a)/(b) NT {ta[0] / tb[0]:.3f}, TN {tat[0] / tb[0]:.3f};"
              f"  TN/NT fused {tat[0] / ta[0]:.3f}")
        scale = float(tb[3].abs().max())
        print(f"  results: NT against composed {float((ta[3] - tb[3]).abs().max()) / scale:.2e}, TN against composed "
              f"{float((tat[3] - tb[3]).abs().max()) / scale:.2e} of max|.|")
        del Cbuf
        print(f"  peak memory beyond the operands: (a) {peak(lambda: fused(False)):.1f} MiB, (b) {peak(composed):.1f} MiB")
        if M <= 4096:
            tau_c = tau[:1].expand(M)
            for vt in (False, True):
                tg = timed(lambda: linalg.variance_reduction(cache, Uc, tau_c, Ur, q=16, transposed=vt), warm=1)
                line(f"greedy q = 16, all included, {'TN' if vt else 'NT'}", tg, f"picks {tg[3][1][:4].tolist()}...")
        del Vc, Vr, Vct, Vrt

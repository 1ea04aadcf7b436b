"""Variance reduction of runs that return y and gradient components (linalg.variance_reduction_block, gpp_post_cross_lin_sq) at N
training points of the C2 generator (d = 8, p = 8) with all 8 and with 3 of 8 gradient components, M_c x M_r = 1024 x 4096 and
4096 x 4096.  Times, each the median of the repeats after warm-up, between two device synchronisations:
  (a) the fused launch, gpp_post_cross_lin_sq, on the M_c b rows of ONE call (b = 1 + p'), in both operand forms (NT on W V,
      TN on its transpose), with random whitening rows and explained parts of realistic size — its time does not depend on the values;
  (b) the composed route it replaces, from entry points that were there before: the whitened prior block by ``cross_kernel`` +
      ``cross_kernel_dx`` (on a selection for 3 of 8) + ``torch.bmm`` into an (M_c b) x M_r block, the library GEMM on it with
      alpha = -1, beta = 1, then the weighted square-and-row-sum in torch;
  (c) gpp_post_cross_sq on the same rows: the same tile body with the plain generator, the yardstick of the epilogue's extra work;
then the whole ``variance_reduction_block`` by stage (``linalg.STAGE_EVENTS``) at ``ALC_GRADIENT_CHUNK_BYTES`` = 64, 256 and 1024 MiB.
Results of (a), both forms, and (b) are compared at every shape.
usage: python tools/bench_alc_gradient.py [N] [repeats] > profiles/r18_alc_gradient_bench.txt"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.backend import GradientSelection, rows_buffer  # noqa: E402
from gpplus_amd.gradient_enhanced import GRADIENT_NUGGET_REL  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

SHAPES = ((1024, 4096), (4096, 4096))
DIRS = (tuple(range(8)), (1, 4, 6))
N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
X, y, kw, theta = make_config("C2", N + 2 * 4096)
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


def line(what, t, extra=""):
    print(f"  {what:72s} {t[0]:10.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}) {extra}", flush=True)


with torch.no_grad():
    out = m.forward(X.to("cuda"))
    U = out.lazy_covariance_matrix.U1.to(torch.float64).contiguous()
    cache = m._ensure_prediction_cache()
    gctx, spec = cache.gctx, cache.spec
    w, sf2 = spec.w, spec.sf2.reshape(1)
    D = U.shape[1]
    tau = m.likelihood.noise_covar.noise.detach().reshape(-1).to(torch.float64)
    print(f"N={N}, d={D}, kind={spec.kind}, {reps} repeats; flops of the product 2 M_c b M_r N")
    gen = torch.Generator(device="cuda").manual_seed(7)
    for Mc, Mr in SHAPES:
        Uc, Ur = U[N:N + Mc].contiguous(), U[N + 4096:N + 4096 + Mr].contiguous()
        omega = torch.full((Mr,), 1.0 / Mr, dtype=torch.float64, device="cuda")
        _, _, Vr = linalg.predict_from_cache(cache, Ur, need_V=True)
        Vrt = rows_buffer(N, Mr, "cuda")
        gctx.transpose(Vr, Vrt)
        for dirs in DIRS:
            pn = len(dirs)
            b, k0, kn = 1 + pn, dirs[0], dirs[-1] - dirs[0] + 1
            Mf = Mc * b
            print(f"-- M_c = {Mc}, M_r = {Mr}, directions {list(dirs)}: {Mf} rows, launch range [{k0}, {k0 + kn})")
            Vf = rows_buffer(Mf, N, "cuda")
            Vf.copy_(torch.randn(Mf, N, generator=gen, dtype=torch.float64, device="cuda") * float(0.5 * sf2 / N) ** 0.5)
            Vft = rows_buffer(N, Mf, "cuda")
            gctx.transpose(Vf, Vft)
            Wc = torch.tril(torch.randn(Mc, b, b, generator=gen, dtype=torch.float64, device="cuda"))
            A = torch.zeros(Mc, b, 1 + kn, dtype=torch.float64, device="cuda")
            A[:, :, 0] = Wc[:, :, 0]
            A[:, :, [1 + d - k0 for d in dirs]] = Wc[:, :, 1:]
            A = A.view(Mf, 1 + kn)
            Uf = Uc.repeat_interleave(b, 0)
            mask = torch.zeros(kn, dtype=torch.bool)
            mask[[d - k0 for d in dirs]] = True
            sel = None if pn == kn else GradientSelection(mask.expand(Mc, kn).contiguous(), "cuda")
            num = torch.empty(Mf, dtype=torch.float64, device="cuda")
            flops = 2.0 * Mf * Mr * N

            def fused(vt):
                return gctx.post_cross_lin_sq(Uf, Ur, w, sf2, A, k0, kn, Vft if vt else Vf, Vrt if vt else Vr, N, num, omega=omega,
                                              kind=spec.kind, d_split=spec.d_split, transposed=vt).clone()

            def value_rows(vt):
                return gctx.post_cross_sq(Uf, Ur, w, sf2, Vft if vt else Vf, Vrt if vt else Vr, N, num, omega=omega, kind=spec.kind,
                                          d_split=spec.d_split, transposed=vt)

            def composed():
                P = torch.empty(Mc, b, Mr, dtype=torch.float64, device="cuda")
                P[:, 0] = gctx.cross_kernel(Uc, Ur, w, sf2, rows_buffer(Mc, Mr, "cuda"), kind=spec.kind, d_split=spec.d_split)
                Dk = gctx.cross_kernel_dx(Uc, Ur, w, sf2, k0, kn, rows_buffer(Mr, Mc * pn, "cuda"), kind=spec.kind, d_split=spec.d_split,
                                          sel=sel)
                P[:, 1:] = Dk.unflatten(1, (Mc, pn)).permute(1, 2, 0)
                C = rows_buffer(Mf, Mr, "cuda")
                C.unflatten(0, (Mc, b)).copy_(torch.bmm(Wc, P))
                gctx.gemm(0, 1, Mf, Mr, N, -1.0, Vf, Vr, 1.0, C)
                return (C * C) @ omega

            ta, tat, tb = timed(lambda: fused(False)), timed(lambda: fused(True)), timed(composed)
            tc, tct = timed(lambda: value_rows(False)), timed(lambda: value_rows(True))
            line("(a) fused gpp_post_cross_lin_sq, NT", ta, f"{flops / ta[0] / 1e9:7.2f} TFLOP/s")
            line("(a) fused gpp_post_cross_lin_sq, TN", tat, f"{flops / tat[0] / 1e9:7.2f} TFLOP/s")
            line("(b) composed: cross_kernel + cross_kernel_dx + bmm + GEMM (NT) + square-and-row-sum", tb)
            line("(c) gpp_post_cross_sq on the same rows, NT", tc, f"{flops / tc[0] / 1e9:7.2f} TFLOP/s")
            line("(c) gpp_post_cross_sq on the same rows, TN", tct, f"{flops / tct[0] / 1e9:7.2f} TFLOP/s")
            print(f"  ratios: (a)/(b) NT {ta[0] / tb[0]:.3f}, TN {tat[0] / tb[0]:.3f};  (a)/(c) NT {ta[0] / tc[0]:.3f}, TN {tat[0] / tct[0]:.3f};"
                  f"  TN/NT fused {tat[0] / ta[0]:.3f}")
            scale = float(tb[3].abs().max())
            print(f"  results: NT against composed {float((ta[3] - tb[3]).abs().max()) / scale:.2e}, TN against composed "
                  f"{float((tat[3] - tb[3]).abs().max()) / scale:.2e} of max|.|")
            del Vf, Vft, A, Wc, Uf
            # the whole score, by stage
            tau_c = tau[:1].expand(Mc)
            gnoise = (GRADIENT_NUGGET_REL * linalg.gradient_prior_curvature(spec, 0, D))[list(dirs)].expand(Mc, pn).contiguous()
            for mib in (64, 256, 1024):
                linalg.ALC_GRADIENT_CHUNK_BYTES = mib << 20
                step = linalg._alc_gradient_chunk_points(N, b)
                run = lambda: linalg.variance_reduction_block(cache, Uc, tau_c, gnoise, list(dirs), Ur)  # noqa: E731
                tw = timed(run, warm=1)
                linalg.STAGE_EVENTS = []
                run()
                torch.cuda.synchronize()
                stages = {}
                for name, e0, e1 in linalg.STAGE_EVENTS:
                    stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1)
                linalg.STAGE_EVENTS = None
                line(f"variance_reduction_block, chunks of {mib} MiB ({step} candidates, {-(-Mc // step)} chunks)", tw,
                     f"gain of the gradient x{float((tw[3][0] / tw[3][1]).median()):.2f}")
                print("      stages (ms): " + ", ".join(f"{k} {v:.1f}" for k, v in stages.items()), flush=True)
        del Vr, Vrt

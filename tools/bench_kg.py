"""Knowledge gradient (linalg.knowledge_gradient, gpp_post_cross_min) at N training points of the C2 generator (d = 8) with
M_c = M_r = M candidates and reference points, M in {1024, 4096, 16384}, Q = 32 nodes.  Times, each the median of the repeats after
warm-up, between two device synchronisations, on the V = K_*N Linv^T of ``predict_from_cache`` (made once per M, outside the timings):
  (k) the fused launch, gpp_post_cross_min, in both operand forms: NT on V (points x N) and TN on V^T (N x points);
  (a) gpp_post_cross_sq at the same shapes and forms — the same tile body with the sum-of-squares epilogue: the yardstick for what the
      Q-node epilogue costs;
  (b) the composed route: ``cross_kernel`` into an M x M block, the library GEMM on it with alpha = -1, beta = 1, then Q times
      (m + t_k c).min(1) in torch.
Peak device memory of (k) and (b) beyond the operands (torch's allocator, which also holds the library's workspace), and one greedy
run of q = 4 picks (``linalg.knowledge_gradient``, everything included: both V, the launches — in column chunks under
KG_WORKSPACE_CAP —, the appended coordinates).  Results of (k), both forms, and (b) are compared at every M.
usage: python tools/bench_kg.py [N] [repeats] > profiles/r12_kg_bench.txt"""
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
Q = 32
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
    z, _ = linalg.gauss_hermite_rule(Q)
    nodes = torch.tensor(z, dtype=torch.float64, device="cuda")
    print(f"N={N}, d={U.shape[1]}, kind={spec.kind}, Q={Q}, {reps} repeats; flops of the product 2 M^2 N")
    for M in MS:
        print(f"-- M_c = M_r = {M}")
        Uc, Ur = U[N:N + M].contiguous(), U[N + max(MS):N + max(MS) + M].contiguous()
        omega = torch.full((M,), 1.0 / M, dtype=torch.float64, device="cuda")
        mean_r, _, Vr = linalg.predict_from_cache(cache, Ur, need_V=True)
        _, var_c, Vc = linalg.predict_from_cache(cache, Uc, need_V=True)
        Vct, Vrt = rows_buffer(N, M, "cuda"), rows_buffer(N, M, "cuda")
        gctx.transpose(Vc, Vct)
        gctx.transpose(Vr, Vrt)
        mr = (mean_r - mean_r.min()).contiguous()
        scale = 1.0 / (var_c.clamp_min(0.0) + tau[0] + cache.jitter).sqrt()
        num, mins = torch.empty(M, dtype=torch.float64, device="cuda"), torch.empty(M, Q, dtype=torch.float64, device="cuda")
        flops = 2.0 * M * M * N

        def fused_min(vt):
            return gctx.post_cross_min(Uc, Ur, w, sf2, Vct if vt else Vc, Vrt if vt else Vr, N, mr, scale, nodes, mins, kind=spec.kind,
                                       d_split=spec.d_split, transposed=vt).clone()

        def fused_sq(vt):
            return gctx.post_cross_sq(Uc, Ur, w, sf2, Vct if vt else Vc, Vrt if vt else Vr, N, num, omega=omega, kind=spec.kind,
                                      d_split=spec.d_split, transposed=vt)

        def composed():
            C = gctx.cross_kernel(Uc, Ur, w, sf2, rows_buffer(M, M, "cuda"), kind=spec.kind, d_split=spec.d_split)
            gctx.gemm(0, 1, M, M, N, -1.0, Vc, Vr, 1.0, C)
            res = torch.empty(M, Q, dtype=torch.float64, device="cuda")
            for k in range(Q):
                res[:, k] = torch.addcmul(mr[None, :], C, (nodes[k] * scale)[:, None]).min(1).values
            return res

        tk, tkt = timed(lambda: fused_min(False)), timed(lambda: fused_min(True))
        ta, tat = timed(lambda: fused_sq(False)), timed(lambda: fused_sq(True))
        tb = timed(composed)
        line("(k) fused minima, NT on V", tk, f"{flops / tk[0] / 1e9:7.2f} TFLOP/s")
        line("(k) fused minima, TN on V^T", tkt, f"{flops / tkt[0] / 1e9:7.2f} TFLOP/s")
        line("(a) gpp_post_cross_sq, NT", ta, f"{flops / ta[0] / 1e9:7.2f} TFLOP/s")
        line("(a) gpp_post_cross_sq, TN", tat, f"{flops / tat[0] / 1e9:7.2f} TFLOP/s")
        line(f"(b) composed: cross_kernel + GEMM (NT) + {Q} torch minima", tb)
        print(f"  ratios: (k)/(a) NT {tk[0] / ta[0]:.3f}, TN {tkt[0] / tat[0]:.3f};  (k)/(b) NT {tk[0] / tb[0]:.3f}, TN {tkt[0] / tb[0]:.3f};"
              f"  TN/NT fused {tkt[0] / tk[0]:.3f}")
        span = float(tb[3].abs().max())
        print(f"  results: NT against composed {float((tk[3] - tb[3]).abs().max()) / span:.2e}, TN against composed "
              f"{float((tkt[3] - tb[3]).abs().max()) / span:.2e} of max|.|; NT and TN bitwise equal: {bool(torch.equal(tk[3], tkt[3]))}")
        print(f"  peak memory beyond the operands: (k) {peak(lambda: fused_min(True)):.1f} MiB, (b) {peak(composed):.1f} MiB")
        if M <= 4096:
            tau_c = tau[:1].expand(M)
            for vt in (False, True):
                tg = timed(lambda: linalg.knowledge_gradient(cache, Uc, tau_c, Ur, mean_r, q=4, num_nodes=Q, transposed=vt), warm=1)
                line(f"greedy q = 4, all included, {'TN' if vt else 'NT'}", tg, f"picks {tg[3][1].tolist()}")
        del Vc, Vr, Vct, Vrt

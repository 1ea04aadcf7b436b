"""Posterior of the gradient (GP_Plus.predict_gradient / active_subspace; gpp_cross_kernel_dx, gpp_point_gram) at N training points of
the C2 generator (d = 8, all quantitative: p = 8) with M test points, M in {1024, 4096}.  Times, each the median of the repeats after
warm-up, between two device synchronisations:
  (g) ``predict_gradient`` with the std and with the covariance, ``active_subspace``, and the mean alone (one gpp_kernel_apply_grad);
  (s) the three stages of ONE chunk of ``linalg.gradient_from_cache`` (as many points as ``GRAD_CHUNK_BYTES`` admits) on their own:
      gpp_cross_kernel_dx, gpp_predict_tn on its block, gpp_point_gram (per-point matrices, and the weighted sum alone), with each
      stage's share of their total;
  (b) the two new kernels' achieved bandwidth — cross_kernel_dx writes 8 mc p N bytes, point_gram reads them once — against the
      8.0 TB/s peak and the 6.29 TB/s measured copy rate of the HBM.
usage: python tools/bench_gradpost.py [N] [repeats] > profiles/r13_gradpost_bench.txt"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.backend import rows_buffer  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

MS = (1024, 4096)
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
X, y, kw, theta = make_config("C2", N + max(MS))
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
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * sorted(ts)[len(ts) // 2], 1e3 * min(ts), 1e3 * max(ts)


def line(what, t, extra=""):
    print(f"  {what:66s} {t[0]:10.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}) {extra}", flush=True)


with torch.no_grad():
    Xt = X[N:].to("cuda")
    U = m.forward(X.to("cuda")).lazy_covariance_matrix.U1.to(torch.float64).contiguous()
    cache = m._ensure_prediction_cache()
    gctx, spec = cache.gctx, cache.spec
    w, sf2 = spec.w, spec.sf2.reshape(1)
    p = int(m.quant_index.numel())
    d0 = U.shape[1] - p
    print(f"N={N}, D={U.shape[1]}, p={p}, kind={spec.kind}, {reps} repeats; chunk cap {linalg.GRAD_CHUNK_BYTES >> 20} MiB; "
          f"flops of the product 2 N^2 M p / 2 (triangular operand)")
    for M in MS:
        print(f"-- M = {M}")
        xm = Xt[:M]
        line("(g) predict_gradient, mean alone", timed(lambda: m.predict_gradient(xm, return_std=False)))
        t_std = timed(lambda: m.predict_gradient(xm))
        line("(g) predict_gradient, mean and std", t_std, f"{1.0 * N * N * M * p / t_std[0] / 1e9:7.2f} TFLOP/s overall")
        line("(g) predict_gradient, mean and cov", timed(lambda: m.predict_gradient(xm, return_cov=True)))
        line("(g) active_subspace", timed(lambda: m.active_subspace(xm)))
    # one chunk, stage by stage
    mc = min(linalg._gradient_chunk_points(N, p), max(MS))
    Us = U[N:N + mc].contiguous()
    Dk, Q = rows_buffer(N, mc * p, "cuda"), rows_buffer(mc * p, N, "cuda")
    kss = linalg.gradient_prior_curvature(spec, d0, p).repeat(mc)
    g, v = torch.empty(mc * p, dtype=torch.float64, device="cuda"), torch.empty(mc * p, dtype=torch.float64, device="cuda")
    G = torch.empty((mc, p, p), dtype=torch.float64, device="cuda")
    Gs = torch.empty((p, p), dtype=torch.float64, device="cuda")
    omega = torch.full((mc,), 1.0 / mc, dtype=torch.float64, device="cuda")
    print(f"-- one chunk: {mc} points, Dk and Q {8 * mc * p * N / 2 ** 20:.1f} MiB each")
    t_dx = timed(lambda: gctx.cross_kernel_dx(Us, cache.U, w, sf2, d0, p, Dk, kind=spec.kind, d_split=spec.d_split))
    t_tn = timed(lambda: gctx.predict_tn(cache.Linv, cache.z, Dk, kss, Q, g, v))
    t_pg = timed(lambda: gctx.point_gram(Q, p, G=G))
    t_ps = timed(lambda: gctx.point_gram(Q, p, Gsum=Gs, omega=omega))
    total = t_dx[0] + t_tn[0] + t_pg[0]
    nbytes = 8.0 * mc * p * N
    for what, t in (("(s) gpp_cross_kernel_dx", t_dx), ("(s) gpp_predict_tn", t_tn), ("(s) gpp_point_gram, per-point matrices", t_pg)):
        line(what, t, f"{100.0 * t[0] / total:5.1f} % of the three")
    line("(s) gpp_point_gram, weighted sum alone", t_ps)
    print(f"  product: {1.0 * N * N * mc * p / t_tn[0] / 1e9:.2f} TFLOP/s")
    for what, t in (("gpp_cross_kernel_dx (writes)", t_dx), ("gpp_point_gram (reads)", t_pg)):
        bw = nbytes / (t[0] * 1e-3)
        print(f"  (b) {what:32s} {bw / 1e12:6.3f} TB/s = {100 * bw / HBM_PEAK:5.1f} % of the 8.0 TB/s peak, "
              f"{100 * bw / HBM_COPY:5.1f} % of the 6.29 TB/s copy rate")

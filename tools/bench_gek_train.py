"""Training on gradient observations (objective="gek": linalg.exact_gek_mll, gpp_gek_grad_reduce) at N training points of the C2
generator (d = p = 8), for q = Mg p in {256, 2048} gradient observations.  Times, each the median of the repeats after warm-up,
between two device synchronisations, all in the same run:
  one evaluation of ``GradientEnhancedMarginalLogLikelihood`` (value + gradient: forward and backward);
  one evaluation of ``ExactMarginalLogLikelihood`` on n = N + q plain function rows — the baseline: what the parent commit pays for a
  matrix of that size (above N = 5120 its gradient reduction is the LAUUM's epilogue where the library supports it);
  the three block builds of the joint matrix alone (gpp_kernel_build into the N x N view, gpp_cross_kernel_dx, gpp_kernel_dxdx);
  gpp_gek_grad_reduce alone, which reads the n^2 - N^2 entries of Ky^-1 outside the function block once, against gpp_grad_reduce on
  the whole n x n matrix (its lower triangle): 20 launches back to back between two device events, per launch.
usage: python tools/bench_gek_train.py [N] [repeats] [output file]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.backend import UPLO_UPPER  # noqa: E402
from gpplus_amd.gpcore import ExactMarginalLogLikelihood, GradientEnhancedMarginalLogLikelihood  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

QS = (256, 2048)

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_file = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
X, y, kw, theta = make_config("C2", N + max(QS))


def say(text):
    print(text, flush=True)
    if out_file is not None:
        out_file.write(text + "\n")
        out_file.flush()


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


def timed_launches(fn, n=20):
    """Per-launch (median, min, max) ms of ``n`` launches back to back between two device events."""
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n)
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def line(what, t, extra=""):
    say(f"  {what:72s} {t[0]:10.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}) {extra}")


def evaluation(model, mll):
    def run():
        model.zero_grad()
        loss = -mll(model(*model.train_inputs), model.train_targets)
        loss.backward()
        return loss
    return run


m = GP_Plus(X[:N], y[:N], dtype=torch.float64, device="cuda", **kw)
apply_theta(m, theta)
p = int(m.quant_index.numel())
say(f"N={N}, p={p}, {reps} repeats")
for q in QS:
    Mg = q // p
    n = N + q
    say(f"-- Mg = {Mg}, q = Mg p = {q}, n = N + q = {n}")
    Xg = X[N:N + Mg]
    m.eval()
    with torch.no_grad():
        dY = m.predict_gradient(Xg, return_std=False) * 1.1
    m.train()
    gek = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, Xg, dY)
    t_g = timed(evaluation(m, gek))
    line('one "gek" evaluation (value + gradient)', t_g)
    # the kernels alone, on the operands that evaluation left in the workspace (alpha and Ky^-1 of the joint matrix)
    with torch.no_grad():
        gctx = linalg.get_context(torch.device("cuda", torch.cuda.current_device()))
        ws = linalg.get_workspace(gctx, n, 0)
        cov = m.likelihood(m(*m.train_inputs)).lazy_covariance_matrix
        U = cov.U1.detach().to(torch.float64).contiguous()
        Ug = m._features(Xg.to(m.train_inputs[0]))[0].detach().to(torch.float64).contiguous()
        w, sf2, kind, ds = cov.spec.w.detach().contiguous(), cov.spec.sf2.detach().reshape(1), cov.spec.kind, cov.spec.d_split
        tau = cov.tau.detach().reshape(-1).to(torch.float64)
        D, d0 = U.shape[1], U.shape[1] - p
        alpha, Kinv = ws.alpha.clone(), ws.Ki.clone()
        g_w, g_s, g_t = (torch.zeros(k, dtype=torch.float64, device="cuda") for k in (D, 1, 1))
        t_r = timed_launches(lambda: gctx.gek_grad_reduce(U, Ug, w, sf2, d0, p, alpha, Kinv, 0, g_w, g_s, kind=kind, d_split=ds))
        read = 8.0 * (n * n - N * N) / 2
        line("gpp_gek_grad_reduce alone, per launch of 20", t_r, f"{read / 1e6:.1f} MB of Ky^-1 read: {read / (1e-3 * t_r[0]) / 1e12:.3f} TB/s")
        Un = torch.cat([U, Ug.repeat((q + Mg - 1) // Mg, 1)[:q]]).contiguous()
        t_f = timed_launches(lambda: gctx.grad_reduce(Un, w, sf2, None, 1, alpha, Kinv, 0, g_w, g_s, g_t, None, kind=kind, d_split=ds))
        line(f"gpp_grad_reduce on the {n} x {n} matrix, per launch of 20", t_f,
             f"{8.0 * n * n / 2 / 1e6:.1f} MB read; the new reduction takes {t_r[0] / t_f[0]:.2f} of it")
        A = ws.A
        t_b = timed_launches(lambda: (gctx.kernel_build(U, w, sf2, tau, None, A[:N, :N], kind=kind, d_split=ds, uplo=UPLO_UPPER),
                                      gctx.cross_kernel_dx(Ug, U, w, sf2, d0, p, A[:N, N:n], kind=kind, d_split=ds),
                                      gctx.kernel_dxdx(Ug, Ug, w, sf2, d0, p, A[N:n, N:n], kind=kind, d_split=ds)))
        line("the three block builds of the joint matrix, per round of 20", t_b)
        del alpha, Kinv, Un
    del gek
    m2 = GP_Plus(X[:n], y[:n], dtype=torch.float64, device="cuda", **kw)
    apply_theta(m2, theta)
    m2.train()
    t_m = timed(evaluation(m2, ExactMarginalLogLikelihood(m2.likelihood, m2)))
    line(f"one exact_mll evaluation on {n} function rows (the baseline)", t_m, f'"gek" takes {t_g[0] / t_m[0]:.2f} of it')
    del m2

"""Differentiable prediction (GP_Plus.predict_with_grad: forward as predict(), backward by gpp_cross_grad) at the C2 theta against
a cached factorisation, next to what it replaces: finite differences, (2 D + 1) x predict().
For each M: mean + std forward; forward + backward; mean-only forward and forward + backward; the finite-difference equivalent;
gpp_cross_grad's own kernel time (G = gmean alpha^T + diag(gvar) B, dA = D) and the bandwidth it reaches on B (M x N doubles).
usage: python tools/bench_predict_grad.py [N] [M ...]"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd.models import GP_Plus
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
Ms = [int(a) for a in sys.argv[2:]] or [1, 64, 1024, 8192]
X, y, kw, theta = make_config("C2", N)
m = GP_Plus(X, y, dtype=torch.float64, device="cuda", **kw)
apply_theta(m, theta)
D = X.shape[1]
g = torch.Generator().manual_seed(0)
m.predict(X[:16].cuda(), return_std=True)
torch.cuda.synchronize()


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3


print(f"N={N} D={D} (C2 theta); median of 5, ms")
print(f"{'M':>6} {'fwd m+s':>9} {'fwd+bwd':>9} {'ratio':>6} {'fwd m':>8} {'fwd+bwd m':>10} {'ratio':>6} {'FD (2D+1)':>10} "
      f"{'kernel':>8} {'GB/s on B':>10}")
for M in Ms:
    Xt = (X[torch.randint(0, N, (M,), generator=g)] + 0.01 * torch.randn(M, D, generator=g, dtype=X.dtype)).cuda()

    def fwd():
        m.predict(Xt, return_std=True)

    def fwd_bwd():
        x = Xt.clone().requires_grad_(True)
        mean, std = m.predict_with_grad(x, return_std=True)
        (mean.sum() + std.sum()).backward()

    def fwd_m():
        m.predict(Xt, return_std=False)

    def fwd_bwd_m():
        x = Xt.clone().requires_grad_(True)
        m.predict_with_grad(x, return_std=False).sum().backward()

    reps = 3 if M >= 4096 else 5
    t_f, t_fb, t_fm, t_fbm = timed(fwd, reps), timed(fwd_bwd, reps), timed(fwd_m, reps), timed(fwd_bwd_m, reps)
    # the kernel alone, with the variance operand B
    cache = m.prediction_strategy
    gctx = cache.gctx
    ld = (N + 15) // 16 * 16
    B = torch.randn(M, ld, dtype=torch.float64, device="cuda")[:, :N]
    gm, gv = torch.randn(M, dtype=torch.float64, device="cuda"), torch.randn(M, dtype=torch.float64, device="cuda")
    gA = torch.empty(M, D, dtype=torch.float64, device="cuda")
    gw, gs = torch.empty(D, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
    Ua = Xt.contiguous()

    def kern():
        gctx.cross_grad(Ua, cache.U, cache.spec.w, cache.spec.sf2.reshape(1), gm, cache.alpha, gv, B, gA, None, gw, gs,
                        kind=cache.spec.kind, d_split=cache.spec.d_split)

    kern(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        kern()
    e1.record(); torch.cuda.synchronize()
    t_k = e0.elapsed_time(e1) / 10
    print(f"{M:6d} {t_f:9.3f} {t_fb:9.3f} {t_fb / t_f:6.2f} {t_fm:8.3f} {t_fbm:10.3f} {t_fbm / t_fm:6.2f} {(2 * D + 1) * t_f:10.2f} "
          f"{t_k:8.3f} {M * N * 8 / (t_k * 1e-3) / 1e9:10.0f}", flush=True)
    del B

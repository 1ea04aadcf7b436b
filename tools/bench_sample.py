"""Posterior sampling, GP_Plus.sample_y(size) (models/gp_plus.py:985-998), through its two covariance routes at N training points
of the C2 generator (d = 8):
  training inputs   Sigma = T - T Ky^-1 T + diag(noise): LAUUM of the cached inverse factor + gpp_post_cov_train, then the
                    Cholesky factor and one GEMM for the draws;
  held-out inputs   Sigma = Kss + diag(noise) - V V^T: V = K_*N L^-T (M N^2), the upper triangle of V V^T (M^2 N), the factor,
                    the draws — with M = N points generated beside the training set and held out of it.
The training covariance is factored once (the first call of the eval() phase) and not counted.  Prints the median of the
repeats and the stage times of the last one.
usage: python tools/bench_sample.py [N] [size] [repeats]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
size = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
X, y, kw, theta = make_config("C2", 2 * N)
m = GP_Plus(X[:N], y[:N], dtype=torch.float64, device="cuda", **kw)
apply_theta(m, theta)
Xh = X[N:].cuda()
torch.cuda.synchronize()
t0 = time.perf_counter()
m.predict(Xh[:16], return_std=False)
torch.cuda.synchronize()
print(f"N={N}, size={size}: factorisation of the training covariance (once per eval() phase) {1e3 * (time.perf_counter() - t0):.1f} ms")
res = {}
for name, Xs in (("training inputs", None), ("held-out inputs", Xh)):
    m.sample_y(size=size, X=Xs)  # warm-up (plans, allocator)
    ts = []
    for r in range(reps):
        if r == reps - 1:
            linalg.STAGE_EVENTS = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        draws = m.sample_y(size=size, X=Xs)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    stages, linalg.STAGE_EVENTS = linalg.STAGE_EVENTS, None
    res[name] = sorted(ts)[len(ts) // 2]
    assert draws.shape == (size, N) and bool(torch.isfinite(draws).all())
    parts = ", ".join(f"{s} {a.elapsed_time(b):.1f}" for s, a, b in stages)
    print(f"  {name:16s} {1e3 * res[name]:8.1f} ms (median of {reps}; min {1e3 * min(ts):.1f})   stages [ms]: {parts}")
print(f"  speed-up of the training-input route: {res['held-out inputs'] / res['training inputs']:.2f}x")

"""Appending q observations to a factorised GP (linalg.append_to_cache, gpp_chol_append) at N training points of the C2 generator
(d = 8), q in {1, 16, 17, 256, 2048}.  Times, each the median of the repeats after warm-up, between two device synchronisations:
  the append by copy (a parent in the shared prediction workspace: two N x N window copies, then the bordering);
  the append in place (a parent that owns its matrices with room to spare);
  gpp_chol_append alone (the bordering without the cross block, the corner and the status read-back);
  the same script's from-scratch ``linalg.factorize`` of the N + q rows — the code that was there before, i.e. the yardstick.
For q <= 16 the bordering alone is also given as bytes moved / time against the 6.3 TB/s HBM figure of the MI355X: the sweeps read
the N x N inverse-factor buffer once (8 N^2 bytes; the q-row operands stay in cache).
usage: python tools/bench_condition.py [N] [repeats]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

HBM = 6.3e12
QS = (1, 16, 17, 256, 2048)

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
X, y, kw, theta = make_config("C2", N + max(QS))
m = GP_Plus(X, y, dtype=torch.float64, device="cuda", **kw)
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
    print(f"  {what:58s} {t[0]:10.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}) {extra}", flush=True)


with torch.no_grad():
    # the operands of every row, as the model's own forward and likelihood give them
    out = m.forward(m.train_inputs[0])
    cov = out.lazy_covariance_matrix
    noisy = m.likelihood(out).lazy_covariance_matrix
    U, spec, tau, mean, yy = cov.U1.to(torch.float64).contiguous(), cov.spec, noisy.tau, out.mean, m.train_targets
    assert noisy.grp is None
    print(f"N={N}, d={U.shape[1]}, {reps} repeats")
    parent = linalg.factorize(U[:N], spec, tau, None, mean[:N], yy[:N])
    gctx = parent.gctx
    for q in QS:
        print(f"-- q = {q}")
        sl = slice(N, N + q)
        by_copy = lambda: linalg.append_to_cache(parent, U[sl], tau, None, mean[sl], yy[sl], reserve=0)  # noqa: E731
        t = timed(by_copy)
        assert t[3].route == "copy", t[3].route
        line("append by copy", t)
        owned = linalg.append_to_cache(parent, U[N:N + 1], tau, None, mean[N:N + 1], yy[N:N + 1], reserve=q)
        own = owned._own
        own.filled = N  # (the leading N x N windows are the parent's factors: append to THEM, again and again)
        base = linalg._owned_cache(gctx, own, N, parent.alpha, parent.U, parent.spec, parent.jitter, parent.z, parent._refactor, "copy")

        def in_place():
            own.filled = N
            return linalg.append_to_cache(base, U[sl], tau, None, mean[sl], yy[sl], reserve=0)

        t = timed(in_place)
        assert t[3].route == "in_place", t[3].route
        line("append in place", t)
        k = gctx.cross_kernel(parent.U, U[sl].contiguous(), parent.spec.w, parent.spec.sf2.reshape(1), linalg.rows_buffer(N, q, "cuda"))
        C = linalg.square_buffer(q, "cuda")
        gctx.kernel_build(U[sl].contiguous(), parent.spec.w, parent.spec.sf2.reshape(1), parent._refactor[0], None, C,
                          jitter=parent.jitter, uplo=2)
        rq = (yy[sl] - mean[sl]).to(torch.float64).contiguous()
        z, al = torch.empty(N + q, dtype=torch.float64, device="cuda"), torch.empty(N + q, dtype=torch.float64, device="cuda")
        info = torch.zeros(1, dtype=torch.int32, device="cuda")

        def bordering():
            z[:N].copy_(parent.z)
            al[:N].copy_(parent.alpha)
            gctx.chol_append(own.A, own.Linv, N, q, k, C, rq, z, al, info)

        t = timed(bordering)
        assert int(info.item()) == 0
        extra = ""
        if q <= 16:
            moved = 8.0 * N * N
            extra = f"{moved / 1e9:.2f} GB of Linv: {moved / (1e-3 * t[0]) / 1e12:.2f} TB/s, {100 * moved / (1e-3 * t[0]) / HBM:.1f}% of 6.3 TB/s"
        line("gpp_chol_append alone", t, extra)
        del owned, own, base, k, C
        t = timed(lambda: linalg.factorize(U[:N + q], spec, tau, None, mean[:N + q], yy[:N + q]), warm=1)
        line(f"linalg.factorize of {N + q} rows (from scratch)", t)
        parent.refresh()

"""Conditioning a factorised GP on gradient observations (GP_Plus.condition_on_gradients: gpp_cross_kernel_dx, gpp_kernel_dxdx,
gpp_chol_append) at N training points of the C2 generator (d = p = 8), for Mg p in {16, 256, 2048} gradient observations.  Times,
each the median of the repeats after warm-up, between two device synchronisations, all in the same run:
  ``condition_on_gradients`` (the window copies, the two block builds, the bordering, the copy of the model);
  ``condition_on`` of the same q function rows by copy (reserve = 0) — the first baseline: the same bordering on kernel-value blocks;
  the model's factorisation of the N rows — the second baseline: what the bordering avoids repeating;
  gpp_kernel_dxdx alone on the (Mg p)^2 corner and on a 2048 x 16384 block (268 MB), as achieved write bandwidth against the 6.3 TB/s
  HBM figure of the MI355X: 20 launches back to back between two device events, per launch (one launch between host
  synchronisations measures the launch);
  ``predict`` and ``predict_gradient`` of the returned object at 256 test rows.
usage: python tools/bench_gek.py [N] [repeats] [output file]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

HBM = 6.3e12
QS = (16, 256, 2048)

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_file = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
X, y, kw, theta = make_config("C2", N + max(QS))
m = GP_Plus(X[:N], y[:N], dtype=torch.float64, device="cuda", **kw)
apply_theta(m, theta)
m.eval()
p = int(m.quant_index.numel())


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
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * sorted(ts)[len(ts) // 2], 1e3 * min(ts), 1e3 * max(ts), out


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
    return sorted(ts)[len(ts) // 2], min(ts), max(ts), None


def line(what, t, extra=""):
    say(f"  {what:62s} {t[0]:10.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}) {extra}")


with torch.no_grad():
    say(f"N={N}, p={p}, {reps} repeats")
    Xnew, ynew = X[N:], y[N:]
    m.predict(Xnew[:4])
    cache = m.prediction_strategy
    t_fac = timed(lambda: (setattr(m, "prediction_strategy", None), m._ensure_prediction_cache())[1], warm=1)
    line(f"factorisation of {N} rows (model._ensure_prediction_cache)", t_fac)
    cache = m.prediction_strategy
    gctx, spec = cache.gctx, cache.spec
    Xt = Xnew[:256]
    for q in QS:
        Mg = q // p
        say(f"-- Mg = {Mg}, q = Mg p = {q}")
        Xg = Xnew[:Mg]
        dY = m.predict_gradient(Xg, return_std=False) * 1.1
        try:
            t_g = timed(lambda: m.condition_on_gradients(Xg, dY))
        except RuntimeError as e:  # (errors.NotPSDError: say so and go on with the next size)
            say(f"  condition_on_gradients failed: {e}")
            continue
        line("condition_on_gradients", t_g)
        t_c = timed(lambda: m.condition_on(Xnew[:q], ynew[:q], reserve=0))
        assert t_c[3].prediction_strategy.route == "copy"
        line(f"condition_on of {q} function rows (by copy)", t_c)
        say(f"  {'overhead over condition_on':62s} {t_g[0] - t_c[0]:10.3f} ms  ({t_g[0] / t_c[0]:.2f}x; {t_g[0] / t_fac[0]:.2f} of the factorisation)")
        Ug = m._features(Xg.to(m.train_inputs[0]))[0].to(torch.float64).contiguous()
        d0 = Ug.shape[1] - p
        H = linalg.square_buffer(q, "cuda")
        t_h = timed_launches(lambda: gctx.kernel_dxdx(Ug, Ug, spec.w, spec.sf2.reshape(1), d0, p, H, kind=spec.kind, d_split=spec.d_split))
        wrote = 8.0 * q * q
        line("gpp_kernel_dxdx alone (the corner), per launch of 20", t_h,
             f"{wrote / 1e6:.2f} MB written: {wrote / (1e-3 * t_h[0]) / 1e12:.3f} TB/s, {100 * wrote / (1e-3 * t_h[0]) / HBM:.1f}% of 6.3 TB/s")
        k = linalg.rows_buffer(N, q, "cuda")
        t_k = timed_launches(lambda: gctx.cross_kernel_dx(Ug, cache.U, spec.w, spec.sf2.reshape(1), d0, p, k, kind=spec.kind, d_split=spec.d_split))
        line("gpp_cross_kernel_dx alone (the N x q cross block), per launch of 20", t_k,
             f"{8.0 * N * q / 1e6:.2f} MB written: {8.0 * N * q / (1e-3 * t_k[0]) / 1e12:.3f} TB/s")
        post = t_g[3]
        line("predict at 256 rows from the enhanced posterior", timed(lambda: post.predict(Xt)))
        line("predict_gradient at 256 rows from the enhanced posterior", timed(lambda: post.predict_gradient(Xt)))
        line("predict at 256 rows from the base model", timed(lambda: m.predict(Xt)))
        del post, t_g, t_c, H, k
    # the same kernel where it is bandwidth that is measured: a 256 x 2048-point block of p = 8 directions (268 MB)
    Ua = m._features(Xnew[:256].to(m.train_inputs[0]))[0].to(torch.float64).contiguous()
    Ub = m._features(Xnew[:2048].to(m.train_inputs[0]))[0].to(torch.float64).contiguous()
    H = linalg.rows_buffer(256 * p, 2048 * p, "cuda")
    t_h = timed_launches(lambda: gctx.kernel_dxdx(Ua, Ub, spec.w, spec.sf2.reshape(1), d0, p, H, kind=spec.kind, d_split=spec.d_split))
    wrote = 8.0 * 256 * p * 2048 * p
    line("gpp_kernel_dxdx, 2048 x 16384 block, per launch of 20", t_h,
         f"{wrote / 1e6:.2f} MB written: {wrote / (1e-3 * t_h[0]) / 1e12:.3f} TB/s, {100 * wrote / (1e-3 * t_h[0]) / HBM:.1f}% of 6.3 TB/s")

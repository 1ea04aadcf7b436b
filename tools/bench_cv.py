"""Grouped cross-validation (gp-plus_amd/cv.py, linalg.exact_cv / cv_moments) at N training points of the C2 generator (d = 8), for
two fold structures: 10 folds of N / 10 rows, and N / 4 groups of 4.  Times, each the median of the repeats after warm-up, between
two device synchronisations:
  cv_predict from a warm cache, beside the explicit route it replaces (k ``linalg.factorize`` calls on the (N - m)-point subsets;
  measured for the 10-fold structure only);
  the objective's value, and value + every gradient, beside the leave-one-out objective at the same N;
  each new kernel alone (gpp_cv_blocks, gpp_cv_rows, per bucket) against its own flop count at the 78.6 TFLOP/s fp64 matrix peak.
usage: python tools/bench_cv.py [N] [repeats]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.cv import FoldIndex  # noqa: E402
from gpplus_amd.gpcore import CrossValidationPseudoLikelihood, LeaveOneOutPseudoLikelihood  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

PEAK = 78.6e12

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
X, y, kw, theta = make_config("C2", N)
m = GP_Plus(X, y, dtype=torch.float64, device="cuda", **kw)
apply_theta(m, theta)


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
    print(f"  {what:64s} {t[0]:10.2f} ms  (min {t[1]:.2f}, max {t[2]:.2f}) {extra}", flush=True)


def evaluate(obj, grad):
    """One evaluation of the objective; ``grad=False`` asks for the value alone (no input requires a gradient, so the evaluation
    enqueues neither the LAUUM nor the gradient products)."""
    params = list(m.parameters())
    flags = [p.requires_grad for p in params]
    for p in params:
        p.grad = None
        if not grad:
            p.requires_grad_(False)
    try:
        loss = -obj(m(*m.train_inputs), m.train_targets)
        if grad:
            loss.backward()
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)
    return loss


rng = np.random.default_rng(0)
structures = [(f"10 folds of {N // 10}", rng.permutation(np.arange(N) % 10)),
              (f"{N // 4} groups of 4", rng.permutation(np.arange(N) // 4))]

print(f"N={N}, d=8, {reps} repeats")
m.train()
loo = LeaveOneOutPseudoLikelihood(m.likelihood, m)
line("loo objective, value only", timed(lambda: evaluate(loo, False)))
line("loo objective, value + gradients", timed(lambda: evaluate(loo, True)))

for name, labels in structures:
    print(f"-- {name}")
    fi = FoldIndex(labels, N)
    m.train()
    obj = CrossValidationPseudoLikelihood(m.likelihood, m, fi)
    line("cv objective, value only", timed(lambda: evaluate(obj, False)))
    linalg.STAGE_EVENTS = None
    t = timed(lambda: evaluate(obj, True))
    linalg.STAGE_EVENTS = []
    evaluate(obj, True)
    torch.cuda.synchronize()
    stages, linalg.STAGE_EVENTS = linalg.STAGE_EVENTS, None
    line("cv objective, value + gradients", t, "stages [ms]: " + ", ".join(f"{s} {a.elapsed_time(b):.2f}" for s, a, b in stages))
    for p in m.parameters():
        p.grad = None

    m.eval()
    with torch.no_grad():
        m.cv_predict(fi)  # (factors once: the cache is warm from here on)
        line("cv_predict from the warm cache", timed(lambda: m.cv_predict(fi)))
        cache = m._ensure_prediction_cache()

        if fi.nfolds <= 16:
            tau, grp, r = cache._refactor
            zero = torch.zeros(N, dtype=torch.float64, device="cuda")

            def explicit():
                for f in range(fi.nfolds):
                    keep = torch.ones(N, dtype=torch.bool, device="cuda")
                    keep[torch.from_numpy(fi.fold(f).astype(np.int64)).cuda()] = False
                    linalg.factorize(cache.U[keep].contiguous(), cache.spec, tau, None if grp is None else grp[keep].contiguous(),
                                     zero[keep], r[keep])
            line(f"explicit route: {fi.nfolds} factorisations of {N - int(fi.sizes.max())} points (no prediction yet)", timed(explicit, warm=1))
            m._ensure_prediction_cache().refresh()
        else:
            print(f"  explicit route: {fi.nfolds} factorisations of {N - int(fi.sizes.max())} points: NOT MEASURED")

        # the two kernels alone, per bucket, against their flop counts
        cache = m._ensure_prediction_cache()
        cache.refresh()
        gctx = cache.gctx
        Psq = linalg.square_buffer(N, "cuda")
        Psq.normal_()
        S = linalg.square_buffer(N, "cuda")
        for b, hb in zip(fi.on("cuda"), fi.buckets()):
            blocks = gctx.batched_buffer(b.nf, b.mp)
            t = timed(lambda: gctx.cv_blocks(cache.Linv, b.idx, b.off, blocks))
            pos = np.arange(hb.idx.shape[0]) - np.repeat(hb.off[:-1], hb.sizes)  # b of every entry: (b + 1) pairs a <= b, N - i_b terms each
            flop = 2.0 * float(((pos + 1) * (N - hb.idx.astype(np.int64))).sum())
            line(f"gpp_cv_blocks, bucket {b.mp} x {b.nf}", t, f"{flop:.3e} flop, {flop / (1e-3 * t[0]) / 1e12:.2f} TFLOP/s, "
                 f"{100 * flop / (1e-3 * t[0]) / PEAK:.1f}% of peak")
            G = blocks
            G.normal_()
            t = timed(lambda: gctx.cv_rows(G, b.idx, b.off, Psq, S[b.base:b.base + b.rows]))
            flop = 2.0 * float((hb.sizes.astype(np.float64) ** 2).sum()) * N
            line(f"gpp_cv_rows, bucket {b.mp} x {b.nf}", t, f"{flop:.3e} flop, {flop / (1e-3 * t[0]) / 1e12:.2f} TFLOP/s, "
                 f"{100 * flop / (1e-3 * t[0]) / PEAK:.1f}% of peak")
            del blocks, G
        del Psq, S

"""Partial gradients (``condition_on_gradients(observed=...)``, ``objective="gek"`` with a mask: gpp_cross_kernel_dx_sel,
gpp_kernel_dxdx_sel, gpp_gek_grad_reduce_sel) at N training points of the C2 generator (d = p = 8), for the RBF and the Matern-5/2
kernel, with k = 2, 4 and 8 of the 8 directions observed at every gradient point (the same evenly spaced directions everywhere) and
q = 256 and 2048 observations, i.e. Mg = q / k gradient points.  Per setting, all in one run:
  each ``_sel`` kernel alone, 20 launches back to back between two device events, per launch; THREE such measurements (each the
  median of the repeats), so that their spread can be read beside every difference;
  the same compact block from the dense entry point on the Mg p entries, gathered with torch (``[:, flat]``, ``[flat][:, flat]``);
  for the reduction, the dense entry point on the Mg p layout (what a dense detour has to reduce; its scatter is not counted);
  one ``condition_on_gradients`` and one "gek" evaluation (value and gradient) with the mask.
``--dense-only`` measures nothing but the three dense entry points at Mg = q / 8 points, three measurements each, through calls
that exist without this feature: run from a checkout of the commit before it, it gives the figures the all-observed ``_sel`` calls
are to be compared with.
usage: python tools/bench_gek_partial.py [--dense-only] [N] [repeats] [output file]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.gpcore import GradientEnhancedMarginalLogLikelihood  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

QS = (256, 2048)
KS = (2, 4, 8)
KERNELS = ((0, "RBF", {}), (2, "Matern 5/2", {"quant_correlation_class": "Matern52Kernel"}))

args = [a for a in sys.argv[1:] if a != "--dense-only"]
dense_only = "--dense-only" in sys.argv[1:]
N = int(args[0]) if len(args) > 0 else 20000
reps = int(args[1]) if len(args) > 1 else 5
out_file = open(args[2], "w") if len(args) > 2 else None
P = 8
MG_MAX = max(QS) // min(KS)
X, y, kw0, theta = make_config("C2", N + MG_MAX)


def say(text):
    print(text, flush=True)
    if out_file is not None:
        out_file.write(text + "\n")
        out_file.flush()


def timed(fn, warm=1, n=None):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps if n is None else n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * sorted(ts)[len(ts) // 2], 1e3 * min(ts), 1e3 * max(ts), out


def launches(fn, n=20):
    """Per-launch ms of ``n`` launches back to back between two device events: the median of the repeats."""
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
    return sorted(ts)[len(ts) // 2]


def three(what, fn, extra=""):
    t = sorted(launches(fn) for _ in range(3))
    say(f"  {what:78s} {t[1]:9.4f} ms  (three measurements: {t[0]:.4f} .. {t[2]:.4f}) {extra}")
    return t[1]


def column_mask(k):
    m = torch.zeros(P, dtype=torch.bool)
    m[::P // k] = True
    return m


def evaluation(model, mll):
    def run():
        model.zero_grad()
        loss = -mll(model(*model.train_inputs), model.train_targets)
        loss.backward()
        return loss
    return run


say(f"N={N}, p={P}, {reps} repeats per measurement, {'the dense entry points alone' if dense_only else 'selected against dense'}")
for kind, kname, kkw in KERNELS:
    kw = dict(kw0)
    kw.update(kkw)
    m = GP_Plus(X[:N], y[:N], dtype=torch.float64, device="cuda", **kw)
    apply_theta(m, theta)
    m.eval()
    assert int(m.quant_index.numel()) == P
    with torch.no_grad():
        m.predict(X[N:N + 4])
        cache = m.prediction_strategy
        gctx, spec = cache.gctx, cache.spec
        assert spec.kind == kind
        w, sf2, ds = spec.w, spec.sf2.reshape(1), spec.d_split
        U = cache.U
        D = U.shape[1]
        d0 = D - P
        g_w, g_s = torch.zeros(D, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    for q in QS:
        for k in ((8,) if dense_only else KS):
            Mg = q // k
            dense_q = Mg * P
            say(f"-- {kname}: {k} of {P} directions at Mg = {Mg} points: q = {q} observations (dense layout Mg p = {dense_q})")
            Xg = X[N:N + Mg]
            with torch.no_grad():
                Ug = m._features(Xg.to(m.train_inputs[0]))[0].to(torch.float64).contiguous()
                kd = linalg.rows_buffer(N, dense_q, "cuda")
                Hd = linalg.square_buffer(dense_q, "cuda")
                nd_ = N + dense_q
                Kd = linalg.square_buffer(nd_, "cuda").normal_().mul_(1e-3)
                ad = torch.randn(nd_, dtype=torch.float64, device="cuda")
                dense_dx = lambda: gctx.cross_kernel_dx(Ug, U, w, sf2, d0, P, kd, kind=kind, d_split=ds)  # noqa: E731
                dense_hx = lambda: gctx.kernel_dxdx(Ug, Ug, w, sf2, d0, P, Hd, kind=kind, d_split=ds)  # noqa: E731
                dense_gk = lambda: gctx.gek_grad_reduce(U, Ug, w, sf2, d0, P, ad, Kd, 0, g_w, g_s, kind=kind, d_split=ds)  # noqa: E731
                if dense_only:
                    three(f"gpp_cross_kernel_dx, {N} x {dense_q}", dense_dx, f"{8.0 * N * dense_q / 1e6:.1f} MB written")
                    three(f"gpp_kernel_dxdx, {dense_q} x {dense_q}", dense_hx, f"{8.0 * dense_q ** 2 / 1e6:.1f} MB written")
                    three(f"gpp_gek_grad_reduce, n = {nd_}", dense_gk, f"{4.0 * (nd_ ** 2 - N ** 2) / 1e6:.1f} MB of Kinv read")
                    del kd, Hd, Kd, ad
                    continue
                from gpplus_amd.backend import GradientSelection

                sel = GradientSelection(column_mask(k).expand(Mg, P).contiguous(), "cuda")
                assert sel.q == q
                ks = linalg.rows_buffer(N, q, "cuda")
                Hs = linalg.square_buffer(q, "cuda")
                n = N + q
                Ks, as_ = Kd[:n, :n], ad[:n].contiguous()
                t_s = three(f"gpp_cross_kernel_dx_sel, {N} x {q}", lambda: gctx.cross_kernel_dx(Ug, U, w, sf2, d0, P, ks, kind=kind, d_split=ds, sel=sel),
                            f"{8.0 * N * q / 1e6:.1f} MB written")
                t_d = three(f"gpp_cross_kernel_dx ({N} x {dense_q}) and the gather [:, flat]", lambda: dense_dx()[:, sel.flat],
                            f"{8.0 * N * dense_q / 1e6:.1f} MB written, then gathered")
                say(f"  {'selected / dense-and-gather':78s} {t_s / t_d:9.3f}")
                t_s = three(f"gpp_kernel_dxdx_sel, {q} x {q}", lambda: gctx.kernel_dxdx(Ug, Ug, w, sf2, d0, P, Hs, kind=kind, d_split=ds, sel_a=sel, sel_b=sel),
                            f"{8.0 * q * q / 1e6:.1f} MB written")
                t_d = three(f"gpp_kernel_dxdx ({dense_q} x {dense_q}) and the gather [flat][:, flat]", lambda: dense_hx()[sel.flat][:, sel.flat],
                            f"{8.0 * dense_q ** 2 / 1e6:.1f} MB written, then gathered")
                say(f"  {'selected / dense-and-gather':78s} {t_s / t_d:9.3f}")
                t_s = three(f"gpp_gek_grad_reduce_sel, n = {n}", lambda: gctx.gek_grad_reduce(U, Ug, w, sf2, d0, P, as_, Ks, 0, g_w, g_s, kind=kind, d_split=ds, sel=sel),
                            f"{4.0 * (n ** 2 - N ** 2) / 1e6:.1f} MB of Kinv read")
                t_d = three(f"gpp_gek_grad_reduce on the dense layout, n = {nd_}", dense_gk, f"{4.0 * (nd_ ** 2 - N ** 2) / 1e6:.1f} MB of Kinv read")
                say(f"  {'selected / dense layout':78s} {t_s / t_d:9.3f}")
                del kd, Hd, Kd, ad, ks, Hs, Ks, as_
                dY = m.predict_gradient(Xg, return_std=False) * 1.1
                mask = column_mask(k)
                try:
                    t = timed(lambda: m.condition_on_gradients(Xg, dY, observed=mask), n=3)
                    say(f"  {'condition_on_gradients(observed=mask)':78s} {t[0]:9.2f} ms  (min {t[1]:.2f}, max {t[2]:.2f})")
                except RuntimeError as e:  # (errors.NotPSDError: say so and go on)
                    say(f"  condition_on_gradients failed: {e}")
            m.train()
            gek = GradientEnhancedMarginalLogLikelihood(m.likelihood, m, Xg, dY, None, mask)
            t = timed(evaluation(m, gek), n=3)
            say(f"  {'one gek evaluation with the mask (value + gradient), n = ' + str(n):78s} {t[0]:9.2f} ms  (min {t[1]:.2f}, max {t[2]:.2f})")
            del gek
            m.eval()
    del m, cache

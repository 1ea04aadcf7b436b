"""The batched gradient-enhanced objective (``batched.batched_gek_mll``: gpp_cross_kernel_dx_batched, gpp_kernel_dxdx_batched,
gpp_gek_grad_reduce_batched) against the eager one, on the C2 generator (d = p = 8, RBF), all in one run:
  one batched evaluation (value + gradient) of B = 65 parameter sets at (N, Mg) = (100, 20), (300, 50) and (1000, 250) — at the
  middle size also with every second direction masked — against 65 eager ``linalg.exact_gek_mll`` evaluations of the same sets;
  the three new launches alone, once for all 65 elements, against 65 calls of their single-problem twins (device events);
  a whole ``GP_Plus.fit(objective="gek")`` (65 restarts, 100 Adam steps) against the same fit under
  ``settings.batched_restarts(False)`` with the same 65 restarts (``fit_model_torch``), at (N, Mg) = (100, 20).
Every figure is the median of the repeats after a warm-up, the device synchronised around the timed region.
usage: python tools/bench_gek_batched.py [repeats] [output file]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import settings  # noqa: E402
from gpplus_amd.backend import GradientSelection, rows_buffer, square_buffer  # noqa: E402
from gpplus_amd.batched import batched_gek_mll  # noqa: E402
from gpplus_amd.linalg import KernelSpec, exact_gek_mll  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402
from gpplus_amd.utils import set_seed  # noqa: E402

B, P = 65, 8
SIZES = ((100, 20, False), (300, 50, False), (300, 50, True), (1000, 250, False))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_file = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
DT = torch.float64


def say(text):
    print(text, flush=True)
    if out_file is not None:
        out_file.write(text + "\n")
        out_file.flush()


def timed(fn, n=None, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps if n is None else n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return 1e3 * ts[len(ts) // 2], 1e3 * ts[0], 1e3 * ts[-1]


def device_ms(fn):
    """ms of ``fn`` between two device events: the median of the repeats after a warm-up."""
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def model_and_gradients(N, Mg):
    X, y, kw, theta = make_config("C2", N + Mg)
    m = GP_Plus(X[:N], y[:N], dtype=DT, device="cuda", **kw)
    apply_theta(m, theta)
    m.eval()
    Xg = X[N:N + Mg]
    with torch.no_grad():
        m.predict(X[N:N + 4])
        dY = m.predict_gradient(Xg, return_std=False) * 1.1
    return m, Xg, dY


say(f"B = {B} parameter sets, p = {P} directions, RBF, {reps} repeats per figure (median; min .. max in brackets)")
for N, Mg, masked in SIZES:
    m, Xg, dY = model_and_gradients(N, Mg)
    assert int(m.quant_index.numel()) == P
    with torch.no_grad():
        cache = m.prediction_strategy
        gctx, spec = cache.gctx, cache.spec
        U = cache.U.contiguous()
        Ug = m._features(Xg.to(m.train_inputs[0]))[0].to(DT).contiguous()
        D = U.shape[1]
        d0 = D - P
        kind, ds = spec.kind, spec.d_split
        sel = GradientSelection((torch.arange(P) % 2 == 0).expand(Mg, P).contiguous(), "cuda") if masked else None
        q = Mg * P if sel is None else sel.q
        n = N + q
        scale = (0.8 + 0.4 * torch.arange(B, dtype=DT, device="cuda") / B)
        w = (spec.w.reshape(1, D) * scale.unsqueeze(1)).contiguous()
        sf2 = (spec.sf2.reshape(()) * scale.flip(0)).contiguous()
        tau = (1e-3 * scale).reshape(B, 1).contiguous()
        mean = (0.01 * scale).reshape(B, 1).expand(B, N).contiguous()
        y = m.train_targets.to(DT)
        r_g = (dY.to("cuda", DT) / m.y_std.to("cuda", DT)).reshape(-1)
        noise = (1e-4 * 2.0 * spec.w[d0:] * spec.sf2.reshape(())).repeat(Mg)
        if sel is not None:
            r_g, noise = r_g[sel.flat].contiguous(), noise[sel.flat].contiguous()
    say(f"-- N = {N}, Mg = {Mg}{', every second direction masked' if masked else ''}: q = {q}, n = N + q = {n}")

    def batched():
        lv = [t.clone().requires_grad_(True) for t in (w, sf2, tau, mean)]
        val = batched_gek_mll(U, Ug, lv[0], lv[1], lv[2], lv[3], y, r_g, noise, None, kind, ds, d0, P, 0, sel=sel)
        val.sum().backward()
        return val

    def eager():
        out = []
        for b in range(B):
            lv = [t[b].clone().requires_grad_(True) for t in (w, sf2, tau, mean)]
            val = exact_gek_mll(U, Ug, KernelSpec(lv[0], lv[1], kind, ds), lv[2], lv[3], y, r_g, noise, None, d0, P, n_grad_dims=0, sel=sel)
            val.backward()
            out.append(val.detach())
        return torch.stack(out)

    vb, ve = batched().detach(), eager()
    assert bool(torch.isfinite(vb).all())
    say(f"  values: largest relative difference batched / eager {float(((vb - ve) / ve).abs().max()):.2e}")
    few = 3 if n >= 2000 else None
    tb, te = timed(batched, n=few), timed(eager, n=few)
    say(f"  {'one batched evaluation of 65 sets (value + gradient)':66s} {tb[0]:10.2f} ms  ({tb[1]:.2f} .. {tb[2]:.2f})")
    say(f"  {'65 eager evaluations (value + gradient)':66s} {te[0]:10.2f} ms  ({te[1]:.2f} .. {te[2]:.2f})")
    say(f"  {'eager / batched':66s} {te[0] / tb[0]:10.2f}")

    with torch.no_grad():
        A = gctx.batched_buffer(B, n)
        fg, gg = A[:, :N, N:n], A[:, N:n, N:n]
        Ki = gctx.batched_buffer(B, n).normal_().mul_(1e-3)
        al = gctx.batched_vector(B, n).normal_()
        g_w, g_s = torch.zeros(B, D, dtype=DT, device="cuda"), torch.zeros(B, dtype=DT, device="cuda")
        k1, H1, K1 = rows_buffer(N, q, "cuda"), square_buffer(q, "cuda"), square_buffer(n, "cuda").normal_().mul_(1e-3)
        a1 = al[0].contiguous()
        gw1, gs1 = torch.zeros(D, dtype=DT, device="cuda"), torch.zeros(1, dtype=DT, device="cuda")
        s1 = [sf2[b:b + 1] for b in range(B)]

        def loop(fn):
            def run():
                for b in range(B):
                    fn(b)
            return run

        pairs = (
            ("gpp_cross_kernel_dx", lambda: gctx.cross_kernel_dx_batched(Ug, U, w, sf2, d0, P, fg, kind=kind, d_split=ds, sel=sel),
             loop(lambda b: gctx.cross_kernel_dx(Ug, U, w[b], s1[b], d0, P, k1, kind=kind, d_split=ds, sel=sel))),
            ("gpp_kernel_dxdx", lambda: gctx.kernel_dxdx_batched(Ug, Ug, w, sf2, d0, P, gg, kind=kind, d_split=ds, sel_a=sel, sel_b=sel),
             loop(lambda b: gctx.kernel_dxdx(Ug, Ug, w[b], s1[b], d0, P, H1, kind=kind, d_split=ds, sel_a=sel, sel_b=sel))),
            ("gpp_gek_grad_reduce", lambda: gctx.gek_grad_reduce_batched(U, Ug, w, sf2, d0, P, al, Ki, 0, g_w, g_s, kind=kind, d_split=ds, sel=sel),
             loop(lambda b: gctx.gek_grad_reduce(U, Ug, w[b], s1[b], d0, P, a1, K1, 0, gw1, gs1, kind=kind, d_split=ds, sel=sel))),
        )
        for name, one, many in pairs:
            t1, t65 = device_ms(one), device_ms(many)
            say(f"  {name + '_batched, one launch for 65':50s} {t1:9.4f} ms   65 calls of {name:22s} {t65:9.4f} ms   ratio {t65 / t1:6.2f}")
        del A, fg, gg, Ki, al, k1, H1, K1
    del m, cache

# a whole fit: GP_Plus.fit's batched route against the sequential driver with the same 65 restarts
N, Mg = 100, 20
m0, Xg, dY = model_and_gradients(N, Mg)
X, y, kw, theta = make_config("C2", N + Mg)


def fresh():
    set_seed(3)
    mm = GP_Plus(X[:N], y[:N], dtype=DT, device="cuda", **kw)
    return mm


say(f"-- a whole fit at N = {N}, Mg = {Mg} (n = {N + Mg * P}): 65 restarts, up to 100 Adam steps each, default gradient nugget")
for what, on, runs in (("GP_Plus.fit(objective='gek'): the batched route", True, 2),
                       ("the same fit under settings.batched_restarts(False)", False, 1)):
    ts = []
    for _ in range(runs):  # (the batched route twice: its first run allocates the workspace; the sequential one finds the library warm)
        mm = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with settings.batched_restarts(on):
            best, hist = mm.fit(optim_type="adam_torch", objective="gek", gradients=(Xg, dY))
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    say(f"  {what:66s} {ts[-1]:10.2f} s   ({'first run %.2f s; ' % ts[0] if runs > 1 else ''}{len(hist)} runs, "
        f"{sum(len(h) for h in hist)} recorded losses, best {best:.6f})")

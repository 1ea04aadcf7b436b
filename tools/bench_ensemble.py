"""Hyperparameter-ensemble prediction (``ensemble.HyperparameterEnsemble``): the fused launch gpp_predict_gen_batched against the
composed route (per member gpp_cross_kernel + gpp_predict_tn on the owned cache), against the way to get the same numbers without
an ensemble — K x (``load_state_dict``, then ``model.predict``, factorisation included) — and the one batched factorisation, on the
C2 generator (p = 8, RBF) with M = 4096 test points at (N, K) = (100, 65), (500, 8), (500, 65), (2000, 16), (6144, 8).
Device events around each timed region, one warm-up, the median of the repeats; the fused and the composed route alternate inside
one loop of the same run.  FLOP/s are counted on the M N^2 product V = K_*N L^-T of each member (the triangle's M N^2 / 2
multiply-adds), whatever else a route does.
usage: python tools/bench_ensemble.py [repeats] [output file]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import ensemble  # noqa: E402
from gpplus_amd.backend import get_context  # noqa: E402
from gpplus_amd.batched import _even_elements  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402

M = 4096
CASES = ((100, 65), (500, 8), (500, 65), (2000, 16), (6144, 8))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_file = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
DT = torch.float64


def say(text):
    print(text, flush=True)
    if out_file is not None:
        out_file.write(text + "\n")
        out_file.flush()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median(ts):
    return sorted(ts)[len(ts) // 2]


say(f"M = {M} test points, p = 8, RBF, {reps} repeats per figure (median of device-event times after one warm-up)")
say(f"ENSEMBLE_FUSED_MAX_N = {ensemble.ENSEMBLE_FUSED_MAX_N} when this ran")
for N, K in CASES:
    X, y, kw, theta = make_config("C2", N + M)
    m = GP_Plus(X[:N], y[:N], dtype=DT, device="cuda", **kw)
    apply_theta(m, theta)
    Xt = X[N:N + M].to("cuda")
    g = torch.Generator().manual_seed(N + K)
    states = {n: (p.detach().cpu().unsqueeze(0) + 0.05 * torch.randn(K, *p.shape, generator=g, dtype=p.dtype)).to(p.device)
              for n, p in m.named_parameters() if p.requires_grad}
    ens = ensemble.HyperparameterEnsemble(m, states, weights="uniform")
    gctx = get_context(torch.device("cuda", torch.cuda.current_device()))

    def factor():
        ens._cache = None
        ens._ensure_cache(gctx)

    factor()
    t_factor = median([event_ms(factor) for _ in range(reps)])
    c = ens._cache
    with torch.no_grad():
        (Us, _, _, _, _), _ = ens._operands(Xt.to(m.train_inputs[0]))
        Us = (Us[0] if c.U.dim() == 2 else Us).to(DT).contiguous()
    mean = torch.empty(K, M, dtype=DT, device="cuda")
    var = torch.empty(K, M, dtype=DT, device="cuda")

    def route(fused):
        step = ens._chunk_rows(fused)
        chunk = ens._fused_chunk if fused else ens._composed_chunk

        def run():
            for a0 in range(0, M, step):
                mc = min(step, M - a0)
                chunk(gctx, c, Us[..., a0:a0 + mc, :], mean[:, a0:a0 + mc], var[:, a0:a0 + mc], _even_elements)
        return run

    fused, composed = route(True), route(False)
    fused()
    mf, vf = mean.clone(), var.clone()
    composed()
    dm = float((mean - mf).abs().max() / mf.abs().max())
    dv = float((var - vf).abs().max() / c.sf2.max())
    tf, tc = [], []
    for _ in range(reps):  # the two routes alternate
        tf.append(event_ms(fused))
        tc.append(event_ms(composed))
    tf, tc = median(tf), median(tc)

    twin = m._copy_without_factors()
    sds = [ens.state(b) for b in range(K)]

    def parent():
        for b in range(K):
            twin.train()
            twin.load_state_dict(sds[b])
            twin.predict(Xt, return_std=True)

    parent()
    tp = median([event_ms(parent) for _ in range(reps)])
    t_whole = median([event_ms(lambda: ens.predict(Xt)) for _ in range(reps)])
    flops = float(K) * M * N * N
    say(f"-- N = {N}, K = {K} (shared features: {c.U.dim() == 2}; chunks of {ens._chunk_rows(True)} / {ens._chunk_rows(False)} rows; "
        f"fused against composed: mean {dm:.1e}, var / sf2 {dv:.1e})")
    say(f"  {'fused: gpp_predict_gen_batched + finish':58s} {tf:10.3f} ms   {flops / tf * 1e-9:8.2f} TFLOP/s on K M N^2")
    say(f"  {'composed: K x (gpp_cross_kernel + gpp_predict_tn)':58s} {tc:10.3f} ms   {flops / tc * 1e-9:8.2f} TFLOP/s on K M N^2")
    say(f"  {'composed / fused':58s} {tc / tf:10.2f}")
    say(f"  {'the one batched factorisation (operands .. owned copies)':58s} {t_factor:10.3f} ms")
    say(f"  {'HyperparameterEnsemble.predict, cache in place':58s} {t_whole:10.3f} ms")
    say(f"  {'K x (load_state_dict, model.predict), factorisation incl.':58s} {tp:10.3f} ms   that / (factorisation + predict) "
        f"{tp / (t_factor + t_whole):6.2f}")
    del ens, c, m, twin, mean, var, Us, mf, vf
    torch.cuda.empty_cache()

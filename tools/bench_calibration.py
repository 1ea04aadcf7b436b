"""The gradient by calibration parameters at N training points of the three-source wing generator (10 quantitative inputs + the source
column, d_z = 2: D = 12 feature columns), for C = 1 and C = 4 calibrated columns.  In the same run, per C and per row order
(rows sorted by source: the cross-source rectangle is all gpp_calib_grad_reduce visits; rows shuffled: every tile is mixed):
  gpp_calib_grad_reduce                       the dedicated reduction, C sums;
  gpp_grad_reduce with dU = D                 the only route there was: g_w, g_sf2, g_tau and the N x D feature gradients (whose
                                              rows of source 0 would then be summed), on the same alpha and Ky^-1;
  gpp_grad_reduce with dU = d_z               what a training evaluation of these models launches anyway;
each launch alone between two device events, after warm-up, median / min / max of the repeats; and
  one training evaluation (loss + backward)   of the same model with and without ``calibration_id``, between two device
                                              synchronisations (host included), median / min / max of the repeats.
usage: python tools/bench_calibration.py [N] [repeats] [output file]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.backend import get_context  # noqa: E402
from gpplus_amd.gpcore import ExactMarginalLogLikelihood  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.multi_fidelity import multi_fidelity_wing  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_file = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
KW = {"qual_dict": {10: 3}, "multiple_noise": True, "m_gp": "multiple_constant"}
IDS = {1: [2], 4: [2, 4, 6, 8]}


def say(text):
    print(text, flush=True)
    if out_file is not None:
        out_file.write(text + "\n")
        out_file.flush()


def data(shuffle):
    n0 = N // 5
    n1 = (N - n0) // 2
    X, y = multi_fidelity_wing(n={'0': n0, '1': n1, '2': N - n0 - n1}, random_state=3)
    X[:, :-1] = (X[:, :-1] - X[:, :-1].mean(0)) / X[:, :-1].std(0)
    if shuffle:
        perm = np.random.default_rng(5).permutation(N)
        X, y = X[perm], y[perm]
    return torch.tensor(X), torch.tensor(y)


def model(X, y, ids):
    torch.manual_seed(11)
    m = GP_Plus(X.clone(), y.clone(), dtype=torch.float64, device="cuda", calibration_id=list(ids), **KW)
    sd = m.state_dict()
    for k in sd:
        if k.endswith("raw_lengthscale") and sd[k].numel() > 1:
            sd[k] = torch.full_like(sd[k], 0.6)  # Rough_RBF: l = 2^-1/2 10^-0.3, w ~ 4 per standardised input
        elif k.endswith("raw_noise"):
            sd[k] = torch.full_like(sd[k], -7.0)
        elif k.startswith("Theta_"):
            sd[k] = torch.full_like(sd[k], 0.4)
    m.load_state_dict(sd)
    m.train()
    return m


def evaluation(m):
    mll = ExactMarginalLogLikelihood(m.likelihood, m)

    def run():
        for p in m.parameters():
            p.grad = None
        loss = -mll(m(*m.train_inputs), m.train_targets)
        loss.backward()
        return loss
    return run


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def timed_launch(fn, warm=3):
    for _ in range(warm):
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
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def line(what, t, extra=""):
    say(f"  {what:66s} {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}) {extra}")


say(f"N={N}, three sources, D=12 feature columns, {reps} repeats, device {torch.cuda.get_device_name(0)}")
gctx = get_context("cuda:0")
for shuffle in (False, True):
    X, y = data(shuffle)
    say(f"== rows {'shuffled' if shuffle else 'sorted by source'} ({int((X[:, -1] == 0).sum())} rows of source 0)")
    plain = model(X, y, [])
    t_plain = timed(evaluation(plain))
    line("training evaluation, no calibration_id", t_plain)
    del plain
    for C, ids in IDS.items():
        say(f"-- C = {C} (calibration_id = {ids})")
        m = model(X, y, ids)
        run = evaluation(m)
        t_cal = timed(run)
        line("training evaluation with calibration_id", t_cal, f"{t_cal[0] - t_plain[0]:+.3f} ms against none")
        # the operands of that evaluation: the features and parameters as the Function took them, alpha and Ky^-1 as it left them
        run()
        torch.cuda.synchronize()
        with torch.no_grad():
            out = m.likelihood(m(*m.train_inputs))
        cov = out.lazy_covariance_matrix
        Ud, wd, sd, td, grp = linalg._operands(cov.U1, cov.spec.w, cov.spec.sf2, cov.tau, cov.grp)
        ws = linalg.get_workspace(gctx, N, 0)
        D, S = Ud.shape[1], td.numel()
        dz = D - int(m.quant_index.numel())
        cal = m._calibration(m.train_inputs[0], dz)
        g_theta = torch.empty(C, dtype=torch.float64, device="cuda")
        g_w, g_s, g_t = (torch.empty(k, dtype=torch.float64, device="cuda") for k in (D, 1, S))
        g_U = torch.empty(N, D, dtype=torch.float64, device="cuda")
        t_new = timed_launch(lambda: gctx.calib_grad_reduce(Ud, wd, sd, ws.alpha, ws.Ki, cal.member, cal.cols, g_theta,
                                                            kind=cov.spec.kind, d_split=cov.spec.d_split))
        new = g_theta.clone()
        t_old = timed_launch(lambda: gctx.grad_reduce(Ud, wd, sd, grp, S, ws.alpha, ws.Ki, D, g_w, g_s, g_t, g_U, kind=cov.spec.kind,
                                                      d_split=cov.spec.d_split))
        old = g_U[cal.member.bool()][:, cal.cols.long()].sum(0)
        g_Uz = torch.empty(N, dz, dtype=torch.float64, device="cuda")
        t_base = timed_launch(lambda: gctx.grad_reduce(Ud, wd, sd, grp, S, ws.alpha, ws.Ki, dz, g_w, g_s, g_t, g_Uz,
                                                       kind=cov.spec.kind, d_split=cov.spec.d_split))
        line("gpp_calib_grad_reduce", t_new)
        line(f"gpp_grad_reduce, dU = D = {D}", t_old, f"{t_old[0] / t_new[0]:.2f}x the dedicated reduction")
        line(f"gpp_grad_reduce, dU = d_z = {dz} (launched by the evaluation anyway)", t_base,
             f"dU = D costs {t_old[0] - t_base[0]:+.3f} ms over it")
        rel = float((new - old).abs().max() / old.abs().max())
        say(f"  g_theta {new.tolist()}; against the sum of g_U's member rows: {rel:.2e} of the largest")
        del m, run, g_U, g_Uz

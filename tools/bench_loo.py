"""One training evaluation (value + every gradient) with the leave-one-out log pseudo-likelihood as the objective
(gpcore.LeaveOneOutPseudoLikelihood -> linalg.ExactLOOFunction) beside the same evaluation with the exact marginal log-likelihood,
at N training points of the C2 generator (d = 8):
  mll   build + potrf, trtri, z, alpha, LAUUM fused with the gradient reduction (N^3 flop in all);
  loo   build + potrf, trtri, z, alpha, gpp_loo_scalars, beta, plain LAUUM, gpp_sym_rowscale, the N^3 product S^T S,
        gpp_loo_grad_reduce (2 N^3 flop in all).
Prints the median of the repeats, the stage times of the last one, and the value-only (no gradient) evaluation of each.
usage: python tools/bench_loo.py [N] [repeats]

``--batched``: one Adam step's evaluation (loss + gradients) of B = 65 restarts at N = 500 (d = 8), as ``GP_Plus.fit(objective="loo")``
runs it: the batched leave-one-out step (optim.BatchedObjective(objective="loo")) replayed as a HIP graph and issued eagerly, beside
the 65 sequential eager evaluations of the same parameter sets (the sequential driver's loop body) and the batched MLL step.  Each
repeat times a window of steps between two device synchronisations; the median of the repeats is printed per step.
usage: python tools/bench_loo.py --batched [N] [B] [repeats]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpplus_amd import linalg  # noqa: E402
from gpplus_amd.gpcore import ExactMarginalLogLikelihood, LeaveOneOutPseudoLikelihood  # noqa: E402
from gpplus_amd.models import GP_Plus  # noqa: E402
from gpplus_amd.test_functions.baseline_configs import apply_theta, make_config  # noqa: E402



def bench_batched(N=500, B=65, reps=5, steps=20):
    from gpplus_amd import settings
    from gpplus_amd.optim import BatchedObjective
    from gpplus_amd.optim.mll_batched import _GraphedLossAndGrad
    from gpplus_amd.utils import set_seed

    X, y, kw, theta = make_config("C2", N)
    set_seed(0)
    m = GP_Plus(X, y, dtype=torch.float64, device="cuda", **kw)
    apply_theta(m, theta)

    def timed(fn, n):
        """Median over ``reps`` windows of ``n`` calls, per call, in ms (two warm-up windows first)."""
        ts = []
        for r in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            if r >= 2:
                ts.append((time.perf_counter() - t0) / n)
        return 1e3 * sorted(ts)[len(ts) // 2], 1e3 * min(ts), 1e3 * max(ts)

    rows = []
    objs = {}
    for name in ("loo", "mll"):
        set_seed(1)
        obj = objs[name] = BatchedObjective(m, B, objective=name)
        obj.sample_restarts()
        params = list(obj.theta.values())
        active = torch.ones(B, dtype=torch.bool, device=params[0].device)

        def eager():
            for p in params:
                p.grad = None
            loss = obj.loss()
            torch.nansum(torch.where(active, loss, torch.zeros_like(loss))).backward()
            return loss

        finite = int(torch.isfinite(eager().detach()).sum())
        rows.append((f"batched {name} step, eager ({finite} of {B} elements positive definite)", timed(eager, steps)))
        with settings.graphed_objective(True):
            graphed = _GraphedLossAndGrad(obj, params, active)
        served = graphed.step()  # (False: an element needs jitter at these parameter sets and the driver would re-run the step eagerly)
        rows.append((f"batched {name} step, replayed graph" + ("" if served else " (handed back)"), timed(graphed.step, steps)))
        del graphed
        for p in params:
            p.grad = None

    # the sequential driver's loop body on the same B parameter sets, one after the other, every evaluation eager
    loo = LeaveOneOutPseudoLikelihood(m.likelihood, m)
    states = []
    for b in range(B):
        st = dict(m.state_dict())
        st.update(objs["loo"].row(b))
        states.append(st)
    m.train()

    from gpplus_amd.errors import NotPSDError

    def sequential():
        for st in states:
            m.load_state_dict(st)
            for p in m.parameters():
                p.grad = None
            try:
                loss = -loo(m(*m.train_inputs), m.train_targets)
                loss.backward()
                loss.item()  # (the driver reads every loss)
            except NotPSDError:  # (a start the batched step scores NaN)
                pass

    rows.append((f"{B} sequential eager loo evaluations", timed(sequential, 1)))
    print(f"N={N} B={B}: loss + gradients of one Adam step, median of {reps} windows (min, max) [ms]")
    for what, (med, lo, hi) in rows:
        print(f"  {what:72s} {med:9.3f}  ({lo:.3f}, {hi:.3f})")


if "--batched" in sys.argv:
    args = [int(a) for a in sys.argv[1:] if a != "--batched"]
    bench_batched(*args[:3])
    sys.exit(0)

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
X, y, kw, theta = make_config("C2", N)
m = GP_Plus(X, y, dtype=torch.float64, device="cuda", **kw)
apply_theta(m, theta)
m.train()


def evaluate(obj, grad):
    for p in m.parameters():
        p.grad = None
    with torch.set_grad_enabled(grad):
        loss = -obj(m(*m.train_inputs), m.train_targets)
        if grad:
            loss.backward()
    return loss


res = {}
for name, cls in (("mll", ExactMarginalLogLikelihood), ("loo", LeaveOneOutPseudoLikelihood)):
    obj = cls(m.likelihood, m)
    for grad in (True, False):
        for _ in range(2):  # warm-up (plans, allocator, workspaces)
            evaluate(obj, grad)
        ts = []
        for r in range(reps):
            if r == reps - 1:
                linalg.STAGE_EVENTS = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = evaluate(obj, grad)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        stages, linalg.STAGE_EVENTS = linalg.STAGE_EVENTS, None
        assert bool(torch.isfinite(loss))
        med = sorted(ts)[len(ts) // 2]
        res[name, grad] = med
        parts = ", ".join(f"{s} {a.elapsed_time(b):.2f}" for s, a, b in stages)
        what = "value + gradients" if grad else "value only       "
        print(f"N={N} {name} {what} {1e3 * med:8.2f} ms (median of {reps}; min {1e3 * min(ts):.2f}, max {1e3 * max(ts):.2f})"
              f"   loss {loss.item():.9f}   stages [ms]: {parts}")
print(f"  loo / mll, value + gradients: {res['loo', True] / res['mll', True]:.2f}x    value only: {res['loo', False] / res['mll', False]:.2f}x")

"""The bad calls whose refusals tests/golden/score_refusals.json records word for word (tools/score_refusals.py writes it from the
commit a rearrangement of the host code must stay identical to): ``HOST_CASES`` on two CPU models — every argument error of the
candidate scores, ``active_subspace`` and ``condition_on``, double faults that fix which one is reported first, and one valid call
per method, which ends at the missing device — and ``POST_CROSS_CASES``, the refusals of the three ``post_cross_*`` wrappers on tiny
device operands (nothing is launched: every case is refused first).  Each case is a function without arguments that makes the call;
``record`` turns what it raises into "{type name}: {message}"."""
import functools
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLD, "score_refusals.json")
DT = torch.float64


def record(case):
    try:
        case()
    except Exception as e:  # noqa: BLE001 (the table records whatever is raised)
        return f"{type(e).__name__}: {e}"
    return "no exception"


# ---- host part: two CPU models ------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _borehole():
    """The model of test_alc_host.test_argument_errors_come_before_the_device_on_a_cpu_model with its candidate and reference rows."""
    from gpplus_amd.models import GP_Plus

    fx = dict(np.load(os.path.join(GOLD, "c3_borehole_mixed_n100.npz")))
    X, y = torch.tensor(fx["Utrain"]), torch.tensor(fx["ytrain"])
    m = GP_Plus(X[:80], y[:80], qual_dict={0: 5, 5: 5}, dtype=DT, device="cpu")
    return m, X[80:90], X[90:], y[80:90]


@functools.lru_cache(None)
def _wing():
    """c4_wing_mf_n300 with the third source held out: (model, rows of seen sources, rows of the unseen one, targets of the former)."""
    from gpplus_amd.models import GP_Plus

    fx = dict(np.load(os.path.join(GOLD, "c4_wing_mf_n300.npz")))
    X, y = torch.tensor(fx["Xtrain"]), torch.tensor(fx["ytrain"])
    keep = X[:, 10] != 2
    m = GP_Plus(X[keep], y[keep], qual_dict={10: 3}, multiple_noise=True, m_gp="multiple_constant", dtype=DT, device="cpu")
    return m, X[keep][:5], X[~keep][:4], y[keep][:5]


def _row_faults(good):
    nan, inf, level = good.clone(), good.clone(), good.clone()
    nan[1, 2] = float("nan")
    inf[0, 3] = float("inf")
    level[2, 5] = 9.0
    return {"columns": good[:, :-1], "empty": good[:0], "nan": nan, "inf": inf, "level": level}


def _methods():
    """name -> (call(model, **kw), the valid keywords on the borehole model, the keywords that hold row sets)."""
    from gpplus_amd.bayesian_optimizations import (select_by_knowledge_gradient, select_by_variance_reduction,
                                                   select_run_by_variance_reduction)

    _, good, ref, y = _borehole()
    ones = torch.ones(ref.shape[0], dtype=DT)
    cost = torch.ones(good.shape[0], dtype=DT)
    sets = dict(Xcand=good, Xref=ref)
    return {
        "variance_reduction": (lambda m, **kw: m.variance_reduction(**kw), dict(sets, weights=ones), ("Xcand", "Xref")),
        "variance_reduction_gradient": (lambda m, **kw: m.variance_reduction(**kw),
                                        dict(sets, weights=ones, gradient=True, gradient_noise=0.01), ("Xcand", "Xref")),
        "knowledge_gradient": (lambda m, **kw: m.knowledge_gradient(**kw), dict(sets, maximize=False, num_nodes=8), ("Xcand", "Xref")),
        "select_by_variance_reduction": (lambda m, **kw: select_by_variance_reduction(m, **kw),
                                         dict(sets, q=3, weights=ones, cost=cost), ("Xcand", "Xref")),
        "select_by_knowledge_gradient": (lambda m, **kw: select_by_knowledge_gradient(m, **kw),
                                         dict(sets, q=2, cost=cost, num_nodes=8), ("Xcand", "Xref")),
        "select_run_by_variance_reduction": (lambda m, **kw: select_run_by_variance_reduction(m, **kw),
                                             dict(sets, weights=ones, gradient=True, cost_value=1.0, cost_gradient=2.0),
                                             ("Xcand", "Xref")),
        "active_subspace": (lambda m, **kw: m.active_subspace(**kw), dict(X=ref, weights=ones), ("X",)),
        "condition_on": (lambda m, **kw: m.condition_on(**kw), dict(X=good, y=y), ("X",)),
    }


def _faults(kw):
    """fault name -> the keywords it replaces, for every fault the valid keywords ``kw`` of a method leave room for."""
    out = {}
    if "weights" in kw:
        w = kw["weights"]
        neg = w.clone()
        neg[3] = -0.1
        out.update({"weights length": dict(weights=w[:-1]), "weights negative": dict(weights=neg), "weights zero": dict(weights=0 * w)})
    for c in [k for k in ("cost", "cost_value", "cost_gradient") if k in kw]:
        one = torch.ones(10, dtype=DT)
        out.update({f"{c} length": {c: one[:-1]}, f"{c} negative": {c: -one}, f"{c} zero": {c: 0 * one}})
    if "q" in kw:
        out.update({"q zero": dict(q=0), "q too large": dict(q=11)})
    if "num_nodes" in kw:
        out.update({"num_nodes zero": dict(num_nodes=0), "num_nodes 65": dict(num_nodes=65)})
    if "gradient" in kw:
        p = 6  # (the borehole model's quantitative columns)
        out.update({"mask without a True": dict(gradient=torch.zeros(p, dtype=torch.bool)), "mask length": dict(gradient=[True] * (p + 1)),
                    "gradient False": dict(gradient=False)})
    if "gradient_noise" in kw:
        out.update({"gradient_noise without gradient": dict(gradient=None), "gradient_noise negative": dict(gradient_noise=-1.0),
                    "gradient_noise shape": dict(gradient_noise=torch.ones(3, dtype=DT))})
    if "y" in kw:
        bad = kw["y"].clone()
        bad[4] = float("nan")
        out.update({"y length": dict(y=kw["y"][:-1]), "y nan": dict(y=bad), "no observation": dict(X=kw["X"][:0], y=kw["y"][:0])})
    return out


#: (first fault, second fault) of the double faults; "nan" stands for NaN in the method's first row set
_DOUBLES = (("nan", "weights negative"), ("nan", "weights length"), ("weights negative", "mask without a True"),
            ("weights zero", "cost length"), ("weights length", "q too large"), ("cost negative", "q too large"),
            ("cost length", "q zero"), ("cost zero", "num_nodes zero"), ("q too large", "num_nodes zero"), ("q zero", "num_nodes 65"),
            ("mask without a True", "gradient_noise negative"), ("weights zero", "cost_value negative"),
            ("mask without a True", "cost_gradient zero"), ("nan", "y length"))


def _host_cases():
    cases = {}

    def add(name, call, model, kw):
        cases[name] = lambda: call(model()[0], **kw)

    for meth, (call, kw, sets) in _methods().items():
        faults = _faults(kw)
        for s in sets:
            for f, rows in _row_faults(kw[s]).items():
                faults[f"{f} in {s}"] = {s: rows}
        for f, repl in faults.items():
            add(f"{meth}: {f}", call, _borehole, dict(kw, **repl))
        faults["nan"] = faults[f"nan in {sets[0]}"]
        for a, b in _DOUBLES:
            if a in faults and b in faults:
                add(f"{meth}: {a} + {b}", call, _borehole, dict(kw, **faults[a], **faults[b]))
        add(f"{meth}: valid", call, _borehole, kw)
        # a source the model has not seen, on the multi-fidelity model (no weights, costs of its own sizes)
        _, seen, unseen, y = _wing()
        base = {k: v for k, v in kw.items() if k not in ("weights", "cost", "q", "y")}
        for s in sets:
            wkw = dict(base, **{t: seen for t in sets})
            wkw[s] = unseen
            if "y" in kw:
                wkw["y"] = y[:unseen.shape[0]]
            if "q" in kw:
                wkw["q"] = 2
            add(f"{meth}: source in {s}", call, _wing, wkw)
    return cases


HOST_CASES = _host_cases()


# ---- the three wrappers: tiny device operands ------------------------------------------------------------------------------------------
MC, MR, D, K = 3, 2, 3, 4


def _operands(transposed=False):
    """Valid operands of all three wrappers (M_c = 3, M_r = 2, D = 3, K = 4, 5 nodes, one observed direction), as keywords."""
    from gpplus_amd.backend import rows_buffer

    g = torch.Generator().manual_seed(7)

    def rnd(*shape):
        return torch.rand(*shape, dtype=DT, generator=g).to("cuda")

    def V(pts):
        buf = rows_buffer(K, pts, "cuda") if transposed else rows_buffer(pts, K, "cuda")
        return buf.copy_(0.1 * rnd(*buf.shape))

    return dict(Uc=rnd(MC, D), Ur=rnd(MR, D), w=rnd(D), sf2=rnd(1), Vc=V(MC), Vr=V(MR), K=K, out=rnd(MC), omega=rnd(MR), kind=0,
                d_split=0, transposed=transposed, A=rnd(MC, 2), d0=1, nd=1, m=rnd(MR), scale=rnd(MC), nodes=rnd(5), outQ=rnd(MC, 5))


def _call(fn, o):
    from gpplus_amd.backend import get_context

    ctx = get_context("cuda")
    tail = dict(kind=o["kind"], d_split=o["d_split"], transposed=o["transposed"])
    if fn == "sq":
        return ctx.post_cross_sq(o["Uc"], o["Ur"], o["w"], o["sf2"], o["Vc"], o["Vr"], o["K"], o["out"], omega=o["omega"], **tail)
    if fn == "lin_sq":
        return ctx.post_cross_lin_sq(o["Uc"], o["Ur"], o["w"], o["sf2"], o["A"], o["d0"], o["nd"], o["Vc"], o["Vr"], o["K"], o["out"],
                                     omega=o["omega"], **tail)
    return ctx.post_cross_min(o["Uc"], o["Ur"], o["w"], o["sf2"], o["Vc"], o["Vr"], o["K"], o["m"], o["scale"], o["nodes"], o["outQ"],
                              **tail)


def _wide(pts, cols, ld):
    """A pts x cols window of a buffer with leading dimension ``ld``."""
    return torch.zeros(pts, ld, dtype=DT, device="cuda")[:, :cols]


def _shared_faults():
    """fault name -> (transposed, function of the valid operands returning the replaced ones)."""
    def rnd(*shape):
        return torch.rand(*shape, dtype=DT).to("cuda")

    return {
        "dtype": (False, lambda o: dict(Ur=o["Ur"].float())),
        "D mismatch": (False, lambda o: dict(Ur=rnd(MR, D + 1))),
        "K zero": (False, lambda o: dict(K=0)),
        "Ur not contiguous": (False, lambda o: dict(Ur=rnd(D, MR).T)),
        "w too long": (False, lambda o: dict(w=rnd(D + 1))),
        "sf2 empty": (False, lambda o: dict(sf2=rnd(0))),
        "kind 3": (False, lambda o: dict(kind=3)),
        "d_split": (False, lambda o: dict(d_split=D + 1)),
        "V column stride": (False, lambda o: dict(Vc=torch.zeros(MC, 2 * K, dtype=DT, device="cuda")[:, ::2])),
        "V too few columns": (False, lambda o: dict(Vr=o["Vr"][:, :K - 1])),
        "V too few rows (transposed)": (True, lambda o: dict(Vc=o["Vc"][:K - 1])),
        "V point count": (False, lambda o: dict(Vc=_wide(MC + 1, K, 16))),
        "V point count (transposed)": (True, lambda o: dict(Vr=_wide(K, MR + 1, 16))),
        "odd leading dimension": (False, lambda o: dict(Vr=_wide(MR, K, 5))),
        "misaligned": (False, lambda o: dict(Vc=torch.zeros(MC * 16 + 1, dtype=DT, device="cuda")[1:].view(MC, 16)[:, :K])),
        "omega length": (False, lambda o: dict(omega=rnd(MR + 1))),
        "out too short": (False, lambda o: dict(out=rnd(MC - 1), outQ=rnd(MC - 1, 5))),
    }


_OWN_FAULTS = {
    "lin_sq": lambda rnd: {"d0 + nd > D": lambda o: dict(d0=D - 1, nd=2, A=rnd(MC, 3)), "A too narrow": lambda o: dict(A=rnd(MC, 1))},
    "min": lambda rnd: {"no nodes": lambda o: dict(nodes=rnd(0), outQ=rnd(MC, 0)), "65 nodes": lambda o: dict(nodes=rnd(65), outQ=rnd(MC, 65)),
                        "m length": lambda o: dict(m=rnd(MR + 1)), "scale length": lambda o: dict(scale=rnd(MC + 1)),
                        "out with the wrong Q": lambda o: dict(outQ=rnd(MC, 4))},
}
#: double faults that straddle the place where a wrapper's own checks sit between the shared ones
_POST_CROSS_DOUBLES = {
    "sq": (("misaligned", "omega length"), ("omega length", "out too short"), ("kind 3", "V column stride")),
    "lin_sq": (("d0 + nd > D", "misaligned"), ("kind 3", "A too narrow"), ("A too narrow", "V column stride"),
               ("d_split", "d0 + nd > D")),
    "min": (("misaligned", "65 nodes"), ("odd leading dimension", "m length"), ("scale length", "out with the wrong Q"),
            ("kind 3", "no nodes")),
}


def _post_cross_cases():
    def rnd(*shape):
        return torch.rand(*shape, dtype=DT).to("cuda")

    cases = {}

    def add(name, fn, transposed, repls):
        def case():
            o = _operands(transposed)
            for r in repls:
                o.update(r(o))
            return _call(fn, o)
        cases[name] = case

    shared = _shared_faults()
    for fn in ("sq", "lin_sq", "min"):
        own = _OWN_FAULTS.get(fn, lambda rnd: {})(rnd)
        for f, (tr, repl) in shared.items():
            if fn == "min" and f == "omega length":
                continue  # (gpp_post_cross_min takes no weights)
            add(f"post_cross_{fn}: {f}", fn, tr, [repl])
        for f, repl in own.items():
            add(f"post_cross_{fn}: {f}", fn, False, [repl])
        for a, b in _POST_CROSS_DOUBLES[fn]:
            ra, rb = (shared[f][1] if f in shared else own[f] for f in (a, b))
            add(f"post_cross_{fn}: {a} + {b}", fn, False, [ra, rb])
    return cases


POST_CROSS_CASES = _post_cross_cases()

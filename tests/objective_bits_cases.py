"""The fixed evaluations whose bits tests/golden/objective_bits.json records (tools/objective_bits.py writes it,
tests/test_gpu_objective_bits.py asserts it): every training objective, eager and batched, on the small inputs of the tests that
check their values — the host scaffold around the launches may be rearranged, the value and every gradient may not change a bit.
Each case is a function without arguments that evaluates on the GPU and returns {name: CPU tensor}."""
import hashlib
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_gek_batched as GB  # noqa: E402
from loo_reference import KIND_MATERN52, KIND_RBF, make_inputs  # noqa: E402
from test_gpu_loo_batched import _element  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objective_bits.json")
DT = torch.float64
NAMES = ("U", "w", "sf2", "tau", "mean", "y")


def source_hash():
    """The ``src`` field of the library's version string: the hash of the sources it was built from."""
    from gpplus_amd._lib import load

    return load().gpp_version().decode().split("src ")[1].split()[0].rstrip(")")


def sha256(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def digests(case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the case that needs jitter warns)
        return {k: sha256(v) for k, v in case().items()}


def _finish(val, leaves, scale):
    """Backward with a gradient that is not 1 (and differs per element); the value and every leaf's gradient."""
    torch.nansum(val * scale).backward()
    out = {"value": val.detach().cpu()}
    out.update({"d" + k: v.grad.detach().cpu() for k, v in leaves.items() if v.grad is not None})
    return out


def _cuda_leaves(t):
    return {k: v.to("cuda").requires_grad_(True) for k, v in t.items()}


def _batch_scale(nb):
    return (1.0 + 0.25 * torch.arange(nb, dtype=DT)).to("cuda")


def _eager(fn, N, D, kind, d_split, S, dU):
    def case():
        from gpplus_amd.linalg import Calibration, KernelSpec, exact_cv, exact_loo, exact_mll

        inp = make_inputs(N, D, seed=3000 + N + D, S=S)
        kw = {}
        if fn == "calibrated":  # theta stands in the last feature column of every third row
            member = (torch.arange(N) % 3 == 0).to(torch.int32)
            inp["U"][member.bool(), D - 1] = 0.4
            theta = torch.tensor([0.4], dtype=DT, device="cuda", requires_grad=True)
            kw["calib"] = Calibration(theta, member.to("cuda"), torch.tensor([D - 1], dtype=torch.int32, device="cuda"))
        lv = _cuda_leaves({k: inp[k] for k in NAMES})
        grp = None if inp["grp"] is None else inp["grp"].to("cuda")
        spec = KernelSpec(lv["w"], lv["sf2"], kind, d_split)
        args = (lv["U"], spec, lv["tau"], lv["mean"], lv["y"])
        if fn == "cv":
            val = exact_cv(*args, torch.arange(N) % 5, grp, n_grad_dims=dU)
        elif fn == "loo":
            val = exact_loo(*args, grp, n_grad_dims=dU)
        else:
            val = exact_mll(*args, grp, n_grad_dims=dU, **kw)
        if kw:
            lv["theta"] = theta
        return _finish(val, lv, 1.5)
    return case


def _eager_jitter():
    """The duplicate rows of ``test_gpu_model.test_duplicate_rows_and_jitter_policy`` without noise: factored with jitter."""
    from gpplus_amd.linalg import KernelSpec, exact_mll

    rng = np.random.default_rng(3)
    U = rng.standard_normal((200, 3))
    U[100:] = U[:100]
    lv = _cuda_leaves(dict(U=torch.tensor(U), w=torch.full((3,), 0.3, dtype=DT), sf2=torch.tensor(1.0, dtype=DT),
                           tau=torch.tensor([0.0], dtype=DT), mean=torch.zeros(200, dtype=DT), y=torch.tensor(rng.standard_normal(200))))
    val = exact_mll(lv["U"], KernelSpec(lv["w"], lv["sf2"]), lv["tau"], lv["mean"], lv["y"], n_grad_dims=0)
    return _finish(val, lv, 1.5)


def _eager_gek(shape, b, two_groups, noise_given):
    """Element b of a shape of tests/test_gpu_gek_batched.py through ``linalg.exact_gek_mll``."""
    def case():
        from gpplus_amd.linalg import KernelSpec, exact_gek_mll

        N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
        t, fixed = GB._leaves(shape)
        t = {k: (v if (k == "y" or (k == "U" and shared)) else v[b]) for k, v in t.items()}
        grp = fixed["grp"]
        if two_groups:
            t["tau"], grp = torch.tensor([0.05, 0.08], dtype=DT), (torch.arange(N) % 2).to(torch.int32)
        lv = _cuda_leaves(t)
        val = exact_gek_mll(lv["U"], lv["Ug"], KernelSpec(lv["w"], lv["sf2"], kind, d_split), lv["tau"], lv["mean"], lv["y"],
                            fixed["r_g"].to("cuda"), fixed["noise"].to("cuda") if noise_given else None, grp.to("cuda"), d0, nd,
                            n_grad_dims=dU, sel=GB._selection(GB._inputs(shape)["mask"], "cuda"))
        return _finish(val, lv, 1.5)
    return case


def _batched(fn, N, D, kind, d_split, S, dU, shared):
    def case():
        from gpplus_amd.batched import batched_loo, batched_mll

        inp = make_inputs(N, D, seed=3000 + N + D, S=S)
        elems = [_element(inp, b) for b in range(GB.B)]
        t = {k: torch.stack([e[k] for e in elems]) for k in ("w", "sf2", "tau", "mean")}
        t["U"] = inp["U"].clone() if shared else torch.stack([inp["U"] * (1.0 + 0.02 * b) for b in range(GB.B)])
        t["y"] = inp["y"].clone()
        lv = _cuda_leaves(t)
        grp = None if inp["grp"] is None else inp["grp"].to("cuda")
        val = (batched_loo if fn == "loo" else batched_mll)(lv["U"], lv["w"], lv["sf2"], lv["tau"], lv["mean"], lv["y"], grp, kind,
                                                            d_split, dU)
        return _finish(val, lv, _batch_scale(GB.B))
    return case


def _batched_gek(shape, noise_given=True, bad=None):
    def case():
        from gpplus_amd.batched import batched_gek_mll

        N, Mg, D, d0, nd, kind, d_split, dU, selection, shared = shape
        t, fixed = GB._leaves(shape, noise=0.05 if bad is None else 0.0)
        if bad is not None:  # the singular element of test_one_bad_element_returns_nan_and_leaves_the_others_alone
            t["Ug"][bad] = t["Ug"][bad][0].clone().expand(Mg, D)
            t["sf2"][bad] = 1e14
            t["tau"][bad] = 1e-8
        lv = _cuda_leaves(t)
        val = batched_gek_mll(lv["U"], lv["Ug"], lv["w"], lv["sf2"], lv["tau"], lv["mean"], lv["y"], fixed["r_g"].to("cuda"),
                              fixed["noise"].to("cuda") if noise_given else None, fixed["grp"].to("cuda"), kind, d_split, d0, nd, dU,
                              sel=GB._selection(GB._inputs(shape)["mask"], "cuda"))
        if bad is not None:
            assert bool(torch.isnan(val[bad])) and int(torch.isnan(val).sum()) == 1, val
        return _finish(val, lv, _batch_scale(GB.B))
    return case


CASES = {
    "eager-mll-63": _eager("mll", 63, 3, KIND_RBF, 0, 1, 0),
    "eager-mll-130-matern": _eager("mll", 130, 4, KIND_MATERN52, 2, 2, 4),
    "eager-loo-65-matern": _eager("loo", 65, 8, KIND_MATERN52, 3, 3, 2),
    "eager-cv-63": _eager("cv", 63, 3, KIND_RBF, 0, 1, 0),
    "eager-calibrated-40": _eager("calibrated", 40, 4, KIND_RBF, 0, 2, 1),
    "eager-mll-jitter-200": _eager_jitter,
    "batched-mll-63-shared": _batched("mll", 63, 3, KIND_RBF, 0, 1, 0, True),
    "batched-mll-130-matern": _batched("mll", 130, 4, KIND_MATERN52, 2, 2, 4, False),
    "batched-loo-63-shared": _batched("loo", 63, 3, KIND_RBF, 0, 1, 0, True),
    "batched-loo-130-matern": _batched("loo", 130, 4, KIND_MATERN52, 2, 2, 4, False),
    "batched-gek-bad-element": _batched_gek(GB.BAD_SHAPE, bad=2),
}
for _i, (_shape, _id) in enumerate(zip(GB.SHAPES, GB._IDS)):
    CASES[f"eager-gek-{_id}-noise"] = _eager_gek(_shape, 1, _i % 2 == 1, True)
    CASES[f"eager-gek-{_id}-nugget"] = _eager_gek(_shape, 3, _i % 2 == 0, False)
    CASES[f"batched-gek-{_id}-noise"] = _batched_gek(_shape)
    CASES[f"batched-gek-{_id}-nugget"] = _batched_gek(_shape, noise_given=False)

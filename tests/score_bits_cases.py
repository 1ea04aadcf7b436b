"""The fixed evaluations whose bits tests/golden/score_bits.json records (tools/objective_bits.py writes it when given this module's
name, tests/test_gpu_objective_bits.py asserts it): every candidate score — expected variance reduction, knowledge gradient, the
score of a run with gradients and the score from a gradient-enhanced posterior — at the ``linalg`` level on 2 x 2 ragged tiles and
at the model level on the multi-fidelity fixture.  The host code around the launches may be rearranged; no output may change a bit.
Each case is a function without arguments that evaluates on the GPU and returns {name: CPU tensor}."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kg_fixture import build_c4  # noqa: E402
from loo_reference import KIND_MATERN52, KIND_RBF, make_inputs  # noqa: E402
from objective_bits_cases import digests, sha256, source_hash  # noqa: E402,F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_bits.json")
DT = torch.float64
N, D, MC, MR = 150, 4, 130, 131  # (candidates and reference rows: 2 x 2 tiles, ragged on both sides)
FORMS = (("nt", False), ("tn", True))


def _cpu(**named):
    return {k: v.detach().cpu() for k, v in named.items()}


def _setup(kind, d_split):
    """(cache, Uc, tau_c, Ur, omega, cost, mean_r): a ``FactorCache`` of 150 rows with two noise groups and the row sets of a score."""
    from gpplus_amd.linalg import KernelSpec, factorize

    inp = {k: (v if v is None else v.to("cuda")) for k, v in make_inputs(N, D, seed=4100 + kind, S=2).items()}
    cache = factorize(inp["U"], KernelSpec(inp["w"], inp["sf2"], kind, d_split), inp["tau"], inp["grp"], inp["mean"], inp["y"])
    g = torch.Generator().manual_seed(4200 + kind)

    def rnd(*shape):
        return torch.rand(*shape, dtype=DT, generator=g).to("cuda")

    Uc, Ur = rnd(MC, D), rnd(MR, D)
    return cache, Uc, inp["tau"][torch.arange(MC, device="cuda") % 2], Ur, 0.1 + rnd(MR), 0.5 + rnd(MC), rnd(MR)


def _gradient_cache(cache, drop=True):
    """``cache`` bordered with the gradients at five points in the directions 1 and 2, three of the ten entries unobserved (q = 7)."""
    from gpplus_amd.backend import GradientSelection
    from gpplus_amd.linalg import append_gradients_to_cache

    g = torch.Generator().manual_seed(4300)
    Ug = torch.rand(5, D, dtype=DT, generator=g).to("cuda")
    mask = torch.ones(5, 2, dtype=torch.bool)
    mask[0, 1] = mask[2, 0] = mask[4, 1] = False
    sel = GradientSelection(mask, "cuda")
    r_g = torch.randn(sel.q, dtype=DT, generator=g).to("cuda")
    noise = torch.full((sel.q,), 1e-3, dtype=DT, device="cuda")
    return append_gradients_to_cache(cache, Ug, 1, 2, r_g, noise, sel)


def _variance_reduction(kind, d_split):
    def case():
        from gpplus_amd.linalg import variance_reduction

        cache, Uc, tau_c, Ur, omega, cost, _ = _setup(kind, d_split)
        out = {}
        for form, tr in FORMS:
            for wn, om in (("uniform", None), ("omega", omega)):
                for cn, c in (("", None), ("-cost", cost)):
                    first, picks, gains = variance_reduction(cache, Uc, tau_c, Ur, omega=om, q=3, cost=c, transposed=tr)
                    out.update(_cpu(**{f"{form}-{wn}{cn}-first": first, f"{form}-{wn}{cn}-picks": picks, f"{form}-{wn}{cn}-gains": gains}))
        return out
    return case


def _knowledge_gradient(kind, d_split):
    def case():
        from gpplus_amd import linalg

        cache, Uc, tau_c, Ur, _, _, mean_r = _setup(kind, d_split)
        out = {}
        for form, tr in FORMS:
            for mx in (False, True):
                for cap in (linalg.KG_WORKSPACE_CAP, 1):  # (1 byte: the 131 reference rows go as 128 + 3)
                    saved, linalg.KG_WORKSPACE_CAP = linalg.KG_WORKSPACE_CAP, cap
                    try:
                        first, picks, gains = linalg.knowledge_gradient(cache, Uc, tau_c, Ur, mean_r, q=3, maximize=mx, num_nodes=7,
                                                                        transposed=tr)
                    finally:
                        linalg.KG_WORKSPACE_CAP = saved
                    key = f"{form}-{'max' if mx else 'min'}{'-chunked' if cap == 1 else ''}"
                    out.update(_cpu(**{key + "-first": first, key + "-picks": picks, key + "-gains": gains}))
        return out
    return case


def _from_gradient_cache(kind, d_split):
    def case():
        from gpplus_amd.linalg import variance_reduction_from_gradient_cache

        cache, Uc, tau_c, Ur, omega, _, _ = _setup(kind, d_split)
        gcache = _gradient_cache(cache)
        assert gcache.q == 7
        return _cpu(**{f"{form}-{wn}": variance_reduction_from_gradient_cache(gcache, Uc, tau_c, Ur, omega=om, transposed=tr)
                       for form, tr in FORMS for wn, om in (("uniform", None), ("omega", omega))})
    return case


def _block(kind, d_split):
    def case():
        from gpplus_amd import linalg

        cache, Uc, tau_c, Ur, omega, _, _ = _setup(kind, d_split)
        gcache = _gradient_cache(cache)
        g = torch.Generator().manual_seed(4400)
        out = {}
        # the full range of directions and a selection of it, on both cache types
        for cn, c, dir_sets in (("factor", cache, ([1, 2], [0, 2])), ("gradient", gcache, ([1, 2], [2]))):
            for dirs in dir_sets:
                gnoise = (1e-3 + 1e-2 * torch.rand(MC, len(dirs), dtype=DT, generator=g)).to("cuda")
                for form, tr in FORMS:
                    with_g, value = linalg.variance_reduction_block(c, Uc, tau_c, gnoise, dirs, Ur, omega=omega, transposed=tr)
                    key = f"{cn}-dirs{''.join(map(str, dirs))}-{form}"
                    out.update(_cpu(**{key + "-with": with_g, key + "-value": value}))
        # nine candidates in three chunks
        dirs = [0, 1, 2, 3]
        gnoise = (1e-3 + 1e-2 * torch.rand(9, 4, dtype=DT, generator=g)).to("cuda")
        saved, linalg.ALC_GRADIENT_CHUNK_BYTES = linalg.ALC_GRADIENT_CHUNK_BYTES, 20000
        try:
            assert linalg._alc_gradient_chunk_points(N, 5) == 3
            for form, tr in FORMS:
                with_g, value = linalg.variance_reduction_block(cache, Uc[:9], tau_c[:9], gnoise, dirs, Ur, transposed=tr)
                out.update(_cpu(**{f"chunked-{form}-with": with_g, f"chunked-{form}-value": value}))
        finally:
            linalg.ALC_GRADIENT_CHUNK_BYTES = saved
        return out
    return case


def _launches(kind, d_split):
    """What the three fused launches write, unprocessed, on the V of ``predict_from_cache`` in both operand forms."""
    def case():
        from gpplus_amd.backend import rows_buffer
        from gpplus_amd.linalg import predict_from_cache

        cache, Uc, tau_c, Ur, omega, _, mean_r = _setup(kind, d_split)
        gctx, spec = cache.gctx, cache.spec
        w, sf2, kw = spec.w, spec.sf2.reshape(1), dict(kind=spec.kind, d_split=spec.d_split)
        V = {}
        for name, U in (("c", Uc), ("r", Ur)):
            _, var, Vn = predict_from_cache(cache, U, need_V=True)
            Vt = rows_buffer(N, U.shape[0], "cuda")
            gctx.transpose(Vn, Vt)
            V[name] = (Vn, Vt, var)
        scale = 1.0 / (V["c"][2].clamp_min(0.0) + tau_c).sqrt()
        nodes = torch.linspace(-2.0, 2.0, 7, dtype=DT, device="cuda")
        A = torch.rand(MC, 3, dtype=DT, generator=torch.Generator().manual_seed(4600)).to("cuda")
        out = {}

        def new(*shape):
            return torch.empty(*shape, dtype=DT, device="cuda")

        for form, tr in FORMS:
            Vc, Vr = V["c"][tr], V["r"][tr]
            out.update(_cpu(**{
                f"sq-{form}": gctx.post_cross_sq(Uc, Ur, w, sf2, Vc, Vr, N, new(MC), omega=omega, transposed=tr, **kw),
                f"sq-uniform-{form}": gctx.post_cross_sq(Uc, Ur, w, sf2, Vc, Vr, N, new(MC), transposed=tr, **kw),
                f"lin-sq-{form}": gctx.post_cross_lin_sq(Uc, Ur, w, sf2, A, 1, 2, Vc, Vr, N, new(MC), omega=omega, transposed=tr, **kw),
                f"min-{form}": gctx.post_cross_min(Uc, Ur, w, sf2, Vc, Vr, N, mean_r, scale, nodes, new(MC, 7), transposed=tr, **kw)}))
        return out
    return case


# ---- the model level: c4_wing_mf_n300 with the fixture's parameters (three sources, a noise and a mean each) ----------------------------
def _model():
    """(model on 250 rows, the other 50 rows: the candidates, those of the high-fidelity source: the reference rows, their weights,
    the candidates' costs by source, the mask of the gradient components a run returns)."""
    m, cand, ref = build_c4("cuda")
    weights = 0.5 + torch.arange(ref.shape[0], dtype=DT) / ref.shape[0]
    cost = torch.tensor([4.0, 2.0, 1.0], dtype=DT)[cand[:, 10].long()]
    mask = torch.zeros(int(m.quant_index.numel()), dtype=torch.bool)
    mask[[0, 3, 4]] = True
    return m, cand, ref, weights, cost, mask


def _m_variance_reduction():
    from gpplus_amd.bayesian_optimizations import select_by_variance_reduction

    m, cand, ref, weights, cost, _ = _model()
    picks, gains = select_by_variance_reduction(m, 3, cand, ref, cost=cost)
    return _cpu(weighted=m.variance_reduction(cand, ref, weights=weights), picks=picks, gains=gains)


def _m_knowledge_gradient():
    from gpplus_amd.bayesian_optimizations import select_by_knowledge_gradient

    m, cand, ref, _, cost, _ = _model()
    picks, gains = select_by_knowledge_gradient(m, 2, cand, ref, cost=cost)
    return _cpu(scores=m.knowledge_gradient(cand, ref), picks=picks, gains=gains)


def _m_gradient_runs():
    from gpplus_amd.bayesian_optimizations import select_run_by_variance_reduction

    m, cand, ref, weights, _, mask = _model()
    with_g, value = m.variance_reduction(cand, ref, weights=weights, gradient=mask, gradient_noise=0.02)
    j, is_g, gains = select_run_by_variance_reduction(m, cand, ref, gradient=mask, cost_value=1.0, cost_gradient=1.5)
    return _cpu(with_gradient=with_g, value=value, pick=torch.tensor([j, int(is_g)]), gains=gains)


def _m_gradient_posterior():
    m, cand, ref, weights, _, mask = _model()
    g = torch.Generator().manual_seed(4500)
    post = m.condition_on_gradients(cand[:4], torch.randn(4, mask.numel(), dtype=DT, generator=g), noise=0.05, observed=mask)
    with_g, value = post.variance_reduction(cand, ref, weights=weights, gradient=mask, gradient_noise=0.02)
    return _cpu(function=post.variance_reduction(cand, ref, weights=weights), with_gradient=with_g, value=value)


def _m_active_subspace():
    m, _, ref, weights, _, _ = _model()
    a = m.active_subspace(ref, weights=weights)
    return _cpu(matrix=a.matrix, mean_part=a.mean_part, cov_part=a.cov_part)


def _m_condition_on():
    from kg_fixture import load_c4

    m, cand, ref, _, _, _ = _model()
    rows = torch.cat([(cand[:, 10] == 0).nonzero()[:3, 0], (cand[:, 10] == 1).nonzero()[:2, 0]])
    y = torch.tensor(load_c4()["ytrain"][250:])[rows]
    child = m.condition_on(cand[rows], y)
    mean, std = child.predict(ref, return_std=True)
    return _cpu(mean=mean, std=std)


CASES = {
    "model-variance-reduction": _m_variance_reduction,
    "model-knowledge-gradient": _m_knowledge_gradient,
    "model-gradient-runs": _m_gradient_runs,
    "model-gradient-posterior": _m_gradient_posterior,
    "model-active-subspace": _m_active_subspace,
    "model-condition-on": _m_condition_on,
}
for _kn, _kind, _split in (("rbf", KIND_RBF, 0), ("matern52", KIND_MATERN52, 2)):
    CASES[f"linalg-variance-reduction-{_kn}"] = _variance_reduction(_kind, _split)
    CASES[f"linalg-knowledge-gradient-{_kn}"] = _knowledge_gradient(_kind, _split)
    CASES[f"linalg-from-gradient-cache-{_kn}"] = _from_gradient_cache(_kind, _split)
    CASES[f"linalg-block-{_kn}"] = _block(_kind, _split)
    CASES[f"linalg-launches-{_kn}"] = _launches(_kind, _split)

"""The kernels that generate covariance VALUES produce the same bits: gpp_cov_tile (through gpp_cross_kernel and through
gpp_kernel_build) and KernelGen::value (gpp_kernel_apply) stage the features as sqrt(w) u, sum the squared distances by fma in the
order of the features and form exp(-r2_rbf) h(r2_mat) with the one gpp_kernel_value of csrc/gpp_internal.h.  The error bounds of
tests/apply_reference.py and of the ALC / KG kernel tests assume exactly that; here it is asserted."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_value_sites_agree_to_the_bit(gpu_ctx, kind):
    """M = 65, N = 130: a ragged second tile in each direction; one row of Ua is a row of Ub (r = 0: sqrt(0), both factors exactly
    1).  The block of gpp_kernel_build is an off-diagonal one of the stacked points (no noise term); with C = I and beta = 0 the fma
    chain of gpp_kernel_apply adds exact zeros to the one entry it keeps."""
    from gpplus_amd.backend import square_buffer

    M, N, D, d_split = 65, 130, 3, 1
    g = torch.Generator(device="cuda").manual_seed(40 + kind)
    Ua = torch.randn(M, D, dtype=torch.float64, device="cuda", generator=g)
    Ub = torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)
    Ua[7] = Ub[100]
    w = torch.tensor([0.31, 0.07, 0.19], dtype=torch.float64, device="cuda")
    sf2 = torch.tensor([0.83], dtype=torch.float64, device="cuda")

    cross = torch.full((M, N), float("nan"), dtype=torch.float64, device="cuda")
    gpu_ctx.cross_kernel(Ua, Ub, w, sf2, cross, kind=kind, d_split=d_split)
    assert cross[7, 100].item() == sf2.item()

    full = square_buffer(M + N, "cuda")
    full.fill_(float("nan"))
    gpu_ctx.kernel_build(torch.cat([Ua, Ub]).contiguous(), w, sf2, None, None, full, kind=kind, d_split=d_split, uplo=0)
    assert torch.equal(full[:M, M:M + N], cross)

    applied = torch.zeros(M, N, dtype=torch.float64, device="cuda")
    gpu_ctx.kernel_apply(Ua, Ub, w, sf2, torch.eye(N, dtype=torch.float64, device="cuda"), applied, beta=0.0, kind=kind,
                         d_split=d_split)
    assert torch.equal(applied, cross)

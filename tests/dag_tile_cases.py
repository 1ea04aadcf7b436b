"""Shared by tests/test_gpu_dag_tile_pipeline.py and tools/dag_tile_sha.py: the sizes at which the factorisation's ticket list
(gpp_dag_f64) runs different tile forms, the matrix they factor, and the hash of a factor.

| size   | what the list does there                                                        |
|--------|---------------------------------------------------------------------------------|
| 6912   | its first size, steps not fused (f = 1)                                         |
| 7000   | ragged edge tiles: general iterations and both seams of the big tile's clean loop |
| 11 264 | two steps fused per far tile (f = 2, K = 2048)                                  |
| 14 336 | four steps fused (f = 4, K = 4096)                                              |

At all four the whole inverse is built inside the list (its XB / XA tile tasks), so ``gpp_trtri`` behind it has nothing to merge.
"""
import ctypes
import hashlib
import json
import os

import torch

SIZES = (6912, 7000, 11264, 14336)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dag_tile_pipeline_sha.json")
BLOCK = 1024  # columns hashed at a time


def inputs(n, d=6, tau=(2e-2, 5e-2), seed=0):
    """The kernel inputs of tests/test_gpu_build_potrf.py (same generator, same values)."""
    g = torch.Generator(device="cpu").manual_seed(seed + n)
    U = torch.rand(n, d, generator=g, dtype=torch.float64).cuda()
    w = (torch.rand(d, generator=g, dtype=torch.float64) * 0.5 + 0.1).cuda()
    sf2 = torch.tensor([0.9], dtype=torch.float64, device="cuda")
    tau = torch.tensor(tau, dtype=torch.float64, device="cuda")
    grp = (torch.arange(n, device="cuda") % tau.numel()).to(torch.int32)
    return U, w, sf2, tau, grp


def factor_and_inverse(ctx, n, list_on):
    """(A, Li): upper factor U (Ky = U^T U) in A's upper triangle and the inverse of L = U^T in Li (lower + mirror), through
    ``potrf`` + ``trtri`` with the ticket list on or off; NaN-filled buffers, status checked."""
    from gpplus_amd.backend import OPT_DAG_SCHED, square_buffer

    U, w, sf2, tau, grp = inputs(n)
    A, Li, T = (square_buffer(n, "cuda") for _ in range(3))
    for t in (A, Li, T):
        t.fill_(float("nan"))
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    was = ctx.dag_sched
    ctx.set_option(OPT_DAG_SCHED, int(list_on))
    try:
        ctx.kernel_build(U, w, sf2, tau, grp, A, uplo=2)
        Li.zero_()
        ctx.potrf(A, Li, info, T)
        ctx.trtri(A, Li, T)
        torch.cuda.synchronize()
    finally:
        ctx.set_option(OPT_DAG_SCHED, int(was))
    assert int(info.item()) == 0, hex(int(info.item()))  # (a time-out of the list would leave its status bits here)
    return A, Li


def list_state(ctx):
    """What the handle's most recently used ticket list looks like after a synchronisation: (rows it was planned for, rows of the
    inverse built inside it, tasks, abort word, tickets taken)."""
    lib = ctx.lib
    lib.gpp_debug_dag_info.restype, lib.gpp_debug_dag_info.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
    lib.gpp_debug_dag_counters.restype = ctypes.c_int
    lib.gpp_debug_dag_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    info = (ctypes.c_int64 * 10)()
    assert lib.gpp_debug_dag_info(ctx.h, info) == 0, "no ticket list on this handle"
    buf = (ctypes.c_int * 1024)()
    assert lib.gpp_debug_dag_counters(ctx.h, buf, 1024) >= 3
    return int(info[9]), int(info[8]), int(info[0]), int(buf[0]), int(buf[1])


def factor_sha256(A, n):
    """SHA-256 of the factor's bytes: the upper triangle of A[:n, :n], block column by block column (rows 0 .. end of the block's
    diagonal part, what lies under the diagonal zeroed), each as a contiguous row-major fp64 array."""
    h = hashlib.sha256()
    for c0 in range(0, n, BLOCK):
        c1 = min(c0 + BLOCK, n)
        blk = A[:c1, c0:c1].clone()
        blk[c0:c1] = torch.triu(blk[c0:c1])
        h.update(blk.cpu().numpy().tobytes())
    return h.hexdigest()


def golden():
    with open(GOLDEN) as f:
        return {int(k): v for k, v in json.load(f).items()}

/*
 * gpp.h — C ABI of libgpp_hip.so, the MI355X (gfx950) native back end of the GP+ exact-GP hot path.
 *
 * The reference (Bostanabad-Research-Group/GP-Plus @ 2024_08_07) has no FFI of its own: the path
 *   optim/mll_torch.py:112-117   output = model(*train_inputs); loss = -mll(output, y); loss.backward()
 * runs entirely inside gpytorch/ATen.  Each entry point below replaces the ATen/gpytorch operator(s)
 * that the named reference call site reaches (SURVEY.md §2.1 "implicit device-op inventory", rows K1-K8).
 * The Python host in gp-plus_amd/ binds these with ctypes (gp-plus_amd/_lib.py); INTEGRATION.md shows the
 * stub a GP+ maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors), except where noted "host";
 *  - matrices are row-major fp64 with an explicit leading dimension `ld` (elements).  The covariance and its Cholesky
 *    factor keep the UPPER triangle authoritative (Ky = U^T U, U row-major == L = U^T column-major, LAPACK 'L' on a
 *    column-major array); the strict lower triangle of that buffer is never read or written.  The inverse factor
 *    buffer `Linv` holds L^-1 in its lower triangle and the mirror image L^-T in its strict upper triangle; Kinv keeps
 *    its LOWER triangle authoritative.  (This mix makes every O(N^3) product a row-contiguous "TN" GEMM.)
 *  - N x N matrix pointers must be 16-byte aligned and `ld` even (the kernels use 16-byte accesses);
 *  - all work is enqueued on the handle's stream (gpp_set_stream) and is asynchronous to the host;
 *  - return value: 0 ok, <0 bad argument (-(index of the argument)), >0 HIP runtime error code + 1000;
 *    numerical failure of the factorisation is reported LAPACK-style through `info_dev` (device int32:
 *    0 = ok, k>0 = leading minor k not positive definite), which the caller reads after syncing;
 *  - the library never allocates or frees user-visible memory; scratch comes from the workspace the caller
 *    attaches with gpp_set_workspace (size from gpp_workspace_bytes).
 */
#ifndef GPP_H
#define GPP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpp_handle_s* gpp_handle_t;

/* kernel family of gpp_kernel_build / gpp_cross_kernel / gpp_grad_reduce (`kind`) */
#define GPP_KIND_RBF      0 /* sf2*exp(-sum_d w_d (u_id-u_jd)^2): gpytorch RBFKernel (models/gp_plus.py:223-253),
                               kernels/Rough_RBF.py:27-32, product of RBFs (models/gp_plus.py:297-303) */
#define GPP_KIND_MATERN32 1 /* kernels/matern.py:4-5 on the dims >= d_split, RBF on dims < d_split */
#define GPP_KIND_MATERN52 2 /* kernels/matern.py:7-8 */

#define GPP_UPLO_FULL  0
#define GPP_UPLO_LOWER 1    /* only tiles that intersect the lower triangle are written */
#define GPP_UPLO_UPPER 2    /* only tiles that intersect the upper triangle are written (what gpp_potrf reads) */

/* operation ids for gpp_workspace_bytes */
#define GPP_OP_MLL_EVAL 0   /* potrf + trtri + lauum + mll_reduce + grad_reduce for an N-point model */
#define GPP_OP_PREDICT  1   /* gpp_predict with M test points */
#define GPP_OP_PREDICT_GRAD 2 /* gpp_cross_grad with M test points, N training points, D features; S carries dB (0..D) */
#define GPP_OP_APPLY 3      /* gpp_kernel_apply / gpp_rff_apply: N = the contracted length (training points or random features),
                               M rows, S columns; 0 extra bytes up to a contracted length of 2048 */
#define GPP_OP_APPLY_GRAD 4 /* gpp_kernel_apply_grad / gpp_rff_apply_grad: N = the contracted length, M rows, D features: pieces * M * D
                               doubles above a contracted length of 2048, 0 extra bytes up to it */
#define GPP_OP_APPEND 5     /* gpp_chol_append: N cached points, M = q appended points (D and S are not read) */
#define GPP_OP_POST_CROSS 6 /* gpp_post_cross_sq: N = M_r reference points, M = M_c candidates (D and S are not read) */
#define GPP_OP_POST_CROSS_MIN 7 /* gpp_post_cross_min: N = M_r reference points, M = M_c candidates, S = Q nodes (D is not read) */
#define GPP_OP_POINT_GRAM 8 /* gpp_point_gram with a weighted sum: M points, D = nd rows per point (N and S are not read) */
#define GPP_OP_GEK_GRAD 9   /* gpp_gek_grad_reduce: N function points, M = Mg gradient points, D features, S carries dU */
#define GPP_OP_POST_CROSS_LIN 10 /* gpp_post_cross_lin_sq: N = M_r reference points, M = M_f functionals (D and S are not read) */

const char* gpp_version(void);

int gpp_create(gpp_handle_t* out, int device);
int gpp_destroy(gpp_handle_t h);
/* `stream` is a hipStream_t (passed as void* so this header needs no HIP include). */
int gpp_set_stream(gpp_handle_t h, void* stream);
/* The look-ahead factorisation inside gpp_potrf(_ws) runs on internal streams of the handle, created on first use: a
 * latency stream on 32 CUs (one per shader engine), a throughput stream and a fill stream on the other 224, and one
 * stream without a CU mask for the bulk of each trailing update once the diagonal block it ran beside is done; the
 * calling stream waits for all of them before the entry point's work is complete in stream order.
 * The first two are exposed here, with their disjoint CU sets: which = 0 the latency stream (32 CUs,
 * one per shader engine) on which gpp_potrf_ws factors diagonal blocks, which = 1 the throughput stream (the other CUs)
 * of its trailing updates, which = 2 the stream without a CU mask.  A host-side driver that overlaps its own panel
 * factorisations with its own updates (the sharded evaluation, gp-plus_amd/sharded.py) enqueues on them through
 * gpp_set_stream.  *out receives a hipStream_t. */
int gpp_internal_stream(gpp_handle_t h, int which, void** out);
/* Per-handle switches.  GPP_OPT_COOP_PANEL (default 1, or 0 with GPP_COOP_PANEL=0 in the environment): factor diagonal blocks and
 * small matrices with the cooperative panel kernel, whose work-groups wait for each other on the device and therefore must all be
 * resident together.  When several handles (threads or processes) share one GPU two such launches can each hold part of the same
 * CUs; a wait inside the kernel then gives up after GPP_OPT_PANEL_TIMEOUT_MS (default 500) milliseconds of the device's 100 MHz
 * constant clock — wall time, independent of the core clock and of how slow a poll is beside other tenants — and the factorisation
 * reports *info = GPP_INFO_PANEL_TIMEOUT + the milliseconds the abandoned wait had waited (low 20 bits) — the
 * caller switches the option off and factors again (gp-plus_amd/linalg.py does).  GPP_OPT_PANEL_FAULT (default 0): the NEXT
 * panel launch reports that time-out without running (one shot; for tests of the caller's recovery).
 * GPP_OPT_GEMM_TILE (default 0; for tests): the work-group tile of gpp_gemm and gpp_gemm_batched — 0 chosen by grid size, 1 = 32 x 32,
 * 2 = 64 x 64, 3 = 128 x 128, 4 = 128 x 32 (full output only: with c_tri the two entry points report their c_tri argument); any other
 * value returns -3.  No other entry point reads it.
 * No reference counterpart: the reference's factorisation is torch.linalg.cholesky_ex behind gpytorch (optim/mll_torch.py:116). */
#define GPP_OPT_COOP_PANEL 1
#define GPP_OPT_PANEL_FAULT 2
#define GPP_OPT_PANEL_TIMEOUT_MS 3
#define GPP_OPT_EXEC_SCHED 4 /* (round 4's statically scheduled executor, replaced by the DAG executor: an alias of GPP_OPT_DAG_SCHED) */
#define GPP_OPT_DAG_SCHED 5  /* default 1 (0 with GPP_DAG_SCHED=0): factorisation (and, for 6912 <= N <= 19456, the whole inverse
                              * beside it) as ONE list of tile tasks in topological order that persistent work-groups take by atomic
                              * ticket (gpp_dag.hip, gpp_dag_f64) — needs no co-residency of its work-groups; the diagonal blocks still
                              * run as cooperative panel launches (GPP_OPT_COOP_PANEL) */
#define GPP_OPT_GEMM_TILE 6
#define GPP_INFO_PANEL_TIMEOUT (1 << 30)
/* a wait of one of the DAG executor's work-groups (gpp_dag_f64, its gate kernels) timed out — status =
 * GPP_INFO_EXEC_TIMEOUT + milliseconds: the caller switches GPP_OPT_DAG_SCHED off and factors again; the
 * cooperative panel itself (GPP_INFO_PANEL_TIMEOUT without the second bit) stays on unless it times out on its own */
#define GPP_INFO_EXEC_TIMEOUT ((1 << 30) | (1 << 29))
int gpp_set_option(gpp_handle_t h, int option, int value);
size_t gpp_workspace_bytes(gpp_handle_t h, int op, int64_t N, int64_t M, int D, int S);
int gpp_set_workspace(gpp_handle_t h, void* ws, size_t bytes);

/*
 * K1-K4 fused (models/gp_plus.py:472-474 covar_module(x_new).evaluate();
 * gpytorch RBFKernel/ProductKernel/ScaleKernel; likelihoods_noise/multifidelity.py:63-67 K + diag(noise)):
 *   Ky[i,j] = sf2 * k(U_i, U_j; w) + (i==j) * (tau[grp[i]] + jitter)      for row0 <= i < row0+nrows
 * U: N x D row-major; w: D weights; sf2: 1 double (device); tau: S doubles or NULL; grp: N int32 or NULL
 * (NULL => group 0); d_split: number of leading dims that stay RBF when kind != RBF.
 * row0 is a multiple of 64.  A proper sub-range (row0 != 0 or nrows != N) is a range of ROWS for GPP_UPLO_FULL and
 * GPP_UPLO_LOWER; GPP_UPLO_UPPER takes only the whole matrix here (bad argument #16 otherwise).
 */
int gpp_kernel_build(gpp_handle_t h, const double* U, int64_t N, int D, const double* w, const double* sf2,
                     const double* tau, const int32_t* grp, int S, double jitter, int kind, int d_split,
                     int uplo, double* Ky, int64_t ld, int64_t row0, int64_t nrows);

/* K8 cross block (models/gpregression.py:126 self(x) -> test/train covariance): Kab[a,b] = sf2*k(Ua_a, Ub_b; w) */
int gpp_cross_kernel(gpp_handle_t h, const double* Ua, int64_t Ma, const double* Ub, int64_t Nb, int D,
                     const double* w, const double* sf2, int kind, int d_split, double* Kab, int64_t ld);

/*
 * Products with a GENERATED matrix, for pathwise posterior draws (no reference counterpart: the reference samples only vectors,
 * models/gp_plus.py:985-998).  Neither forms its M x N / M x F matrix in memory: tiles of it are generated in registers and fed
 * to the fp64 MFMA.
 *   gpp_kernel_apply:  Out[a,s] = beta Out[a,s] + sum_j sf2 k(Ua_a, Ub_j; w) C[j,s]          (kind / d_split as gpp_cross_kernel)
 *   gpp_rff_apply:     Out[a,s] = beta Out[a,s] + sum_f sqrt(2 sf2 / F) cos(Omega_f . Ua_a + phase_f) Theta[f,s]
 * Ua: M x D, Ub: N x D, Omega: F x D row-major and contiguous; phase: F; C (N x S, ldc >= S), Theta (F x S, ldt >= S) and Out
 * (M x S, ldo >= S) row-major with any leading dimension and 8-byte alignment.  M, N, F, S >= 1, D <= 64.  beta == 0 overwrites Out
 * without reading it.  Nothing outside the stated extents is read or written.  A contracted length (N or F) above 2048 is cut into
 * pieces of 2048 whose partial products go through the handle workspace (gpp_workspace_bytes(GPP_OP_APPLY, length, M, D, S);
 * GPP_NO_WORKSPACE when it is missing) and are added in a fixed order by a second launch: the count of pieces depends on the
 * contracted length only, so a row's result does not depend on the other rows of the call, and two launches agree bit for bit.
 */
int gpp_kernel_apply(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                     const double* sf2, int kind, int d_split, const double* C, int64_t ldc, int S, double beta, double* Out,
                     int64_t ldo);
int gpp_rff_apply(gpp_handle_t h, const double* Ua, int64_t M, int D, const double* Omega, const double* phase, int64_t F,
                  const double* sf2, const double* Theta, int64_t ldt, int S, double beta, double* Out, int64_t ldo);

/*
 * The gradients of the two products above with respect to Ua, for an upstream Gbar (M x S, ldg >= S): with Out = G C,
 *   g_Ua[a,d] = beta g_Ua[a,d] + sum_j (sum_s Gbar[a,s] C[j,s]) dG[a,j]/dUa[a,d]
 * in one fused launch: neither G, its derivative nor the M x N block Gbar C^T is formed in memory (gpp_cross_grad needs the latter as
 * its operand B).  Operands, checks and status codes as gpp_kernel_apply / gpp_rff_apply; g_Ua is M x D row-major, ldu >= D, and
 * beta == 0 overwrites it without reading it.  A feature with w_d == 0 gets an exact 0; a row of Ua that equals a row of Ub gets a
 * finite gradient for the Matern kinds too.  Contracted lengths above 2048 go through the handle workspace
 * (gpp_workspace_bytes(GPP_OP_APPLY_GRAD, length, M, D, S); GPP_NO_WORKSPACE when it is missing, with nothing enqueued) exactly as in
 * the forward: no float atomics, a row's gradient does not depend on the other rows of the call, two launches agree bit for bit.
 */
int gpp_kernel_apply_grad(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                          const double* sf2, int kind, int d_split, const double* C, int64_t ldc, int S, const double* Gbar,
                          int64_t ldg, double beta, double* g_Ua, int64_t ldu);
int gpp_rff_apply_grad(gpp_handle_t h, const double* Ua, int64_t M, int D, const double* Omega, const double* phase, int64_t F,
                       const double* sf2, const double* Theta, int64_t ldt, int S, const double* Gbar, int64_t ldg, double beta,
                       double* g_Ua, int64_t ldu);

/*
 * K5 (gpytorch psd_safe_cholesky -> torch.linalg.cholesky_ex reached from optim/mll_torch.py:116):
 * in-place Cholesky of A (N x N, UPPER triangle): A = U^T U.  Right-looking in steps of one 128 x 128 leaf (factored
 * AND inverted in LDS by one work-group) below 6144 rows, block rows of 1024 / 512 with look-ahead on two CU-masked
 * streams above; every product runs on the fp64 MFMA GEMM kernel.  On return the upper triangle of A holds U = L^T and
 * the 128-aligned diagonal blocks of Linv hold inv(L_bb) (lower) mirrored with inv(L_bb)^T (upper), as gpp_trtri needs
 * them.
 */
int gpp_potrf(gpp_handle_t h, double* A, int64_t N, int64_t ld, double* Linv, int64_t ldi, int32_t* info_dev);
/* Same, with an N x N scratch T (may be the Kinv buffer): the driver then also completes the inverse of every diagonal block it
 * factors and uses it to solve each block row with GEMMs; the following gpp_trtri on the same handle skips the merges that are
 * already done.  By size (round 5; gpp_api.hip):
 *   3840 <= N < 6912    look-ahead with launches on two CU-masked streams, the WHOLE inverse by bordering on a third beside it;
 *   6912 <= N <= 65536  the DAG executor (gpp_dag.hip, gpp_dag_f64): factorisation — and up to N = 19456 the whole inverse, above
 *                       that its leading 2^j x 1024-row block — as ONE list of tile tasks in topological order that persistent
 *                       work-groups take by atomic ticket, the diagonal blocks as cooperative panel launches behind gate kernels
 *                       (22.75 -> 20.6 ms per evaluation at N = 10000, 61.6 -> 59.9 at 15000, 131.0 -> 129.2 at 20000);
 *   N > 65536           look-ahead with launches (the bulk of each update on a stream without a CU mask).
 * Linv is complete on return wherever the inverse was built beside the factorisation (gpp_trtri then launches nothing). */
int gpp_potrf_ws(gpp_handle_t h, double* A, int64_t N, int64_t ld, double* Linv, int64_t ldi, double* T, int64_t ldt,
                 int32_t* info_dev);

/* gpp_kernel_build (uplo = GPP_UPLO_UPPER, all rows) + gpp_potrf_ws in one call: the same kernels on the same values, so A, Linv
 * and *info_dev are bit for bit what the two calls give.  Where the ticket list applies (6912 <= N <= 65536, the options on, a
 * scratch T) only the leading diagonal block's columns of Ky — all the first cooperative panel reads — are built on the caller's
 * stream; the rest is built on the handle's throughput stream (CU-masked to the CUs the panel does not use) in front of the
 * executor's launch, while the panel stream's 32 CUs already factor block 0.  The panel stream waits for that second build before
 * its first filler launch takes tasks from the list.  Everywhere else (small N, stream capture, the list switched off or not
 * applicable) it IS the two calls, on the caller's stream. */
int gpp_build_potrf_ws(gpp_handle_t h, const double* U, int64_t N, int D, const double* w, const double* sf2, const double* tau,
                       const int32_t* grp, int S, double jitter, int kind, int d_split, double* A, int64_t ld, double* Linv,
                       int64_t ldi, double* T, int64_t ldt, int32_t* info_dev);

/* Completes Linv = inv(L) (lower triangle, mirrored into the upper) from the diagonal-block inverses left by
 * gpp_potrf.  `U` is the factored matrix (upper).  T (N x N) is scratch. */
int gpp_trtri(gpp_handle_t h, const double* U, int64_t N, int64_t ld, double* Linv, int64_t ldi, double* T, int64_t ldt);

/* Kinv(lower) = Linv^T Linv.  With gpp_trtri this is K7's "K_y^-1" (ATen cholesky_backward, optim/mll_torch.py:117). */
int gpp_lauum(gpp_handle_t h, const double* Linv, int64_t N, int64_t ldi, double* Kinv, int64_t ldk);

/* gpp_lauum whose epilogue IS gpp_grad_reduce: the gradient sums of a training evaluation straight from the accumulators of
 * Linv^T Linv, so that Ky^-1 is neither written nor read back (1.6 GB each way at N = 20000).  With W = 0.5 (alpha alpha' - Ky^-1):
 *   g_w[d] = sum_ij W_ij dKy_ij/dw_d        g_sf2 = sum_ij W_ij K_ij / sf2        g_tau[s] = sum_{i in s} W_ii
 * exactly as gpp_grad_reduce defines them; the sums are regrouped by 128 x 128 tiles (one record per tile in the handle's
 * workspace, added in a fixed order: two calls agree bitwise; no atomics).  128-wide tiles at every N (the Python caller uses it
 * above N = 5120, where gpp_lauum does too).  Supported: kind == GPP_KIND_RBF, D <= 16, dU == 0 (no feature gradients), one
 * unsharded matrix.  Anything else returns GPP_NOT_SUPPORTED with nothing enqueued: the caller runs gpp_lauum + gpp_grad_reduce.
 * Linv: the complete inverse factor with its mirror (gpp_trtri); U: N x D row-major; grp: N int32 or NULL; the workspace of
 * GPP_OP_MLL_EVAL must be set (GPP_NO_WORKSPACE otherwise).  Reference counterpart: ATen cholesky_backward + the backward of the kernel ops, optim/mll_torch.py:117. */
#define GPP_NOT_SUPPORTED 2001
#define GPP_NO_WORKSPACE 2002 /* gpp_lauum_grad: gpp_set_workspace has not been given gpp_workspace_bytes(GPP_OP_MLL_EVAL) bytes */
int gpp_lauum_grad(gpp_handle_t h, const double* Linv, int64_t N, int64_t ldi, const double* U, int D, const double* w,
                   const double* sf2, const int32_t* grp, int S, int kind, int dU, const double* alpha, double* g_w,
                   double* g_sf2, double* g_tau);

/* Posterior covariance at the TRAINING inputs (models/gp_plus.py:985-998 sample_y: likelihood(self(train_x)).sample()), built into
 * the upper triangle of A in the layout gpp_potrf_ws factors:
 *   A[i,j] = -tau[grp[i]] Kinv[j,i] tau[grp[j]] + (i == j)(tau[grp[i]] + d[i] + jitter)      j >= i
 * from Kinv = Ky^-1 (LOWER triangle, as gpp_lauum leaves it; Ky = K + diag(tau[grp])): with that T = diag(tau[grp]),
 * K - K Ky^-1 K = T - T Ky^-1 T, and the likelihood's diagonal d on top (d = tau[grp]: 2T - T Ky^-1 T, eigenvalues in
 * [min tau, 2 max tau)).  tau: S doubles; grp: N int32 or NULL (group 0); d: N doubles or NULL (none).  Only the upper
 * triangle of A is written.  A may be Kinv itself (same ld): a tile of the upper triangle is written from the mirrored tile
 * of the lower one, and the diagonal is read before it is written, so the strict lower triangle of Kinv survives. */
int gpp_post_cov_train(gpp_handle_t h, const double* Kinv, int64_t N, int64_t ldk, const double* tau, const int32_t* grp, int S,
                       const double* d, double jitter, double* A, int64_t lda);

/* Trailing update of a block-row-cyclic sharded factorisation, one launch per rank and step:
 *   C(upper triangle of Nt x Nt) -= Urow^T Urow   on the block rows (height nb, a multiple of 128) this rank owns,
 * block row i of C (0-based) being global block row first_block + i, owned when (first_block + i) % nranks == rank.
 * Urow: K x Nt (the just-factored block row, right of its diagonal block), C: the trailing corner of the matrix. */
int gpp_syrk_rows(gpp_handle_t h, const double* Urow, int64_t ldu, double* C, int64_t ldc, int64_t Nt, int64_t K, int64_t nb,
                  int64_t first_block, int rank, int nranks);

/* One right-looking step of the sharded evaluation's BACK-substitution ("each GPU solves for its own
 * block-columns of L^-T L^-1 E_k"): C(lower triangle of M x M) = beta C + alpha A^T B on the column blocks (width nb, a multiple
 * of 128) this rank owns — column block i of C (0-based) is global block first_block + i, owned when
 * (first_block + i) % nranks == rank; other ranks' column blocks are neither read nor written.  A: K x M (rows of the factor's
 * mirror L = U^T), B: K x M (the just-solved block row of Ky^-1), both row-contiguous.  Only the rows [row0, row1) of C are produced
 * (row0 a multiple of 128): the block row the next step depends on is issued first, the rest behind it.  Replaces the broadcast of the inverse's
 * column blocks + the LAUUM share (gpp_lauum_rows_range); reference counterpart: ATen cholesky_backward, optim/mll_torch.py:117.
 * compact != 0 (here, in gpp_trmv_lower_cols and in gpp_grad_reduce_cols): B and C — there T, Kinv — hold ONLY the owned column
 * blocks, side by side (the q-th owned block, global block rank + q nranks, in columns [q nb, (q+1) nb) of the buffer, ld >= the
 * owned width): N x (N / nranks) doubles per rank and matrix instead of N x N — what lets 8 GPUs hold a problem one cannot
 * ("28.8 GB (3.6 GB/GPU sharded)"). */
int gpp_gemm_lower_cols(gpp_handle_t h, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                        int64_t M, int64_t K, double alpha, double beta, int64_t nb, int64_t first_block, int rank, int nranks,
                        int64_t row0, int64_t row1, int compact);

/*
 * The sharded evaluation's factorisation AND forward sweep of one rank as ONE ticket list of tile tasks (the executor of
 * gpp_potrf_ws, gp-plus_amd/csrc/gpp_dag.hip, with the block-cyclic ownership built into the list): the rank's panels (diagonal blocks
 * k % nranks == rank: factor in place in A, inverse + mirror into D[k]), row solves (through the scratch rows W0..W2, nb x N, ldw),
 * its share of the trailing updates, and — right-looking beside them — the rows below the diagonal of ITS column blocks of
 * X = L^-1 into Kc (compact, as in gpp_gemm_lower_cols; Lc: the running sums).  Block rows of other ranks arrive as messages the
 * CALLER moves on a stream of its own (RCCL broadcasts in gp-plus_amd/sharded.py): per block row k a head (diagonal block, D[k], the
 * columns of block k + 1) and a tail (the columns behind, in pieces: gpp_shard_piece_cols).  The owner enqueues gpp_shard_list_gate in
 * front of packing each from A; a receiver enqueues gpp_shard_list_signal behind unpacking each into A / D.  Replaces the per-step launches of
 * gp-plus_amd/sharded.py::_factor and ::_forward (reference counterpart: torch.linalg.cholesky + the solves of optim/mll_torch.py:114-117;
 * the reference has no multi-GPU evaluation).  *used = 0: not applicable here (size, block height, options) — nothing was
 * enqueued and the caller runs its launch-per-product path.  workers: work-groups of the executor (0 = two per throughput CU; tests
 * that share one GPU between ranks pass fewer).  Between _begin and _end the handle runs nothing else.  A wait that exceeds
 * GPP_SHARD_TIMEOUT_MS (default 60 000: it covers the other ranks' progress) sets GPP_INFO_EXEC_TIMEOUT in *info.
 */
int gpp_shard_list_begin(gpp_handle_t h, int64_t N, int64_t nb, int rank, int nranks, double* A, int64_t ld, double* Kc, double* Lc,
                         int64_t ldc, double* D, double* W0, double* W1, double* W2, int64_t ldw, int32_t* info, int workers,
                         int* used);
/* Messages of block row k, in the order every rank moves them on its communication stream: the HEAD (message 0), then the TAIL in
 * pieces of gpp_shard_piece_cols() columns (messages 1 + g: the columns [(k + 2) nb + g W, min((k + 2) nb + (g + 1) W, N)), while that
 * range is not empty; W = 8192, or GPP_SHARD_PIECE_COLS, a multiple of 128; 0 = the whole tail as ONE piece [(k + 2) nb, N)).  Round 6:
 * a task waits for the piece of the column tile it reads, so the owner of block row k + 1 updates, solves and sends its first piece
 * while the rest of block row k is still on the wire.  `tail` in gpp_shard_list_gate / _signal is the message number. */
int64_t gpp_shard_piece_cols(void);
int gpp_shard_list_gate(gpp_handle_t h, void* stream, int tail, int k);
int gpp_shard_list_signal(gpp_handle_t h, void* stream, int tail, int k);
int gpp_shard_list_end(gpp_handle_t h);

/* The sharded evaluation's BACK-substitution of one rank as one ticket list on the handle's stream: the owned column blocks of L^-1 in
 * Kc (compact; rows at and below each block's diagonal, destroyed) become the same column blocks of Ky^-1 = L^-T L^-1 in Lc, against
 * the factor's mirror L in the strict lower triangle of A and the diagonal blocks' inverses D — gp-plus_amd/sharded.py::_backward's
 * per-step launches (gpp_gemm_batched + gpp_gemm_lower_cols) as tile tasks in dependency order, far tiles taking several steps'
 * updates at once.  No communication (bullet 4).  *used = 0: not applicable, nothing enqueued. */
int gpp_shard_back_list(gpp_handle_t h, int64_t N, int64_t nb, int rank, int nranks, const double* A, int64_t ld, double* Kc, double* Lc,
                        int64_t ldc, const double* D, int32_t* info, int workers, int* used);

/*
 * The WHOLE sharded evaluation behind the C ABI (SURVEY.md §8(b) sketched `gpp_set_comm(handle, ncclComm_t, rank, nranks)`): what
 * gp-plus_amd/sharded.py drives from Python — build of the owned block rows, the rank's ticket list with the block rows' messages
 * around it, z / alpha, the back-substitution's list, the gradient reduction — as ONE call per rank, for C / Fortran / MPI callers.
 * The collectives are the caller's (gpp_set_comm: two callbacks, each enqueued on or ordered against the given stream; they may
 * block the host) or RCCL's own (gpp_comm_init_rccl: librccl.so is opened at run time; rank 0 creates the 128-byte id with
 * gpp_comm_unique_id and hands it to the other ranks by any means).  gpp_shard_eval (reference counterpart: `mll(output, y)` +
 * `loss.backward()`, optim/mll_torch.py:114-117) returns 0 with *info_host = the status every rank agrees on: 0, LAPACK's "leading
 * minor not positive definite" (the caller adds jitter and calls again — gpytorch's policy stays with the caller), or a time-out's
 * bits; GPP_SHARD_UNSUPPORTED when the lists do not apply (N < 4096, a block height the panel does not take, a last block of <= 256
 * rows): nothing useful was computed.  On success b->out3 = {quad, logdet, mll}, b->alpha = Ky^-1 r, and with need_grad b->flat =
 * {g_w[D], g_sf2, g_tau[S], g_U[N x dU]} summed over the ranks (the layout of gpp_grad_reduce).  The buffers are the caller's
 * (sizes: gpp_shard_buffer_doubles); b->r = y - mean on entry; the handle's scratch workspace (gpp_set_workspace,
 * GPP_OP_MLL_EVAL) must be set.
 */
enum { GPP_COMM_SUM_F64 = 0, GPP_COMM_MAX_I32 = 1 };
#define GPP_SHARD_UNSUPPORTED 2000
typedef struct gpp_comm {
  void* user;
  int (*bcast)(void* user, void* dev_buf, size_t bytes, int root, void* stream);          /* in place, from rank `root` */
  int (*allreduce)(void* user, void* dev_buf, size_t count, int kind, void* stream);      /* in place; kind: GPP_COMM_* */
} gpp_comm_t;
typedef struct gpp_shard_buffers {
  double* A; int64_t ld;                    /* N x N: the factor (upper) and its mirror (strict lower) */
  double* Kc; double* Lc; int64_t ldc;      /* N x (owned blocks x nb) each: column blocks of L^-1, then of Ky^-1 (in Lc) */
  double* D;                                /* nblk x nb x nb: the diagonal blocks' inverses */
  double* W0; double* W1; double* W2; int64_t ldw;  /* three nb x N scratch rows */
  double* msg;                              /* nb x (N + 2 nb): a message being packed / unpacked */
  double* z; double* alpha; double* r;      /* N each */
  double* flat;                             /* D + 1 + S + N dU */
  double* out3; int32_t* info;              /* 3 doubles; 2 ints */
} gpp_shard_buffers_t;
int gpp_set_comm(gpp_handle_t h, const gpp_comm_t* comm, int rank, int nranks);
int gpp_comm_unique_id(void* out128);
int gpp_comm_init_rccl(gpp_handle_t h, const void* unique_id128, int rank, int nranks);
/* which: 0 A, 1 Kc / Lc (each), 2 D, 3 W0 / W1 / W2 (each), 4 msg — with ld = ldw = N rounded up to 16, ldc = owned blocks x nb.
 * The sizes of A, Kc / Lc and W include 128 doubles of slack behind the last row: the tile kernels read (never write) up to the next
 * multiple of 128 columns past N along a row, and a buffer that ends exactly on a page boundary must not fault there.  (The same holds
 * for the N x N operands of gpp_potrf_ws & co. when a caller allocates them with hipMalloc instead of a pooling allocator.) */
size_t gpp_shard_buffer_doubles(int64_t N, int64_t nb, int rank, int nranks, int which);
int gpp_shard_eval(gpp_handle_t h, int64_t N, int64_t nb, const double* U, int D, const double* w, const double* sf2, const double* tau,
                   const int32_t* grp, int S, int kind, int d_split, double jitter, int dU, int need_grad, const gpp_shard_buffers_t* b,
                   int32_t* info_host);

/*
 * A direct one-to-all PUSH of the sharded evaluation's messages, the alternative to a broadcast collective (SURVEY.md:204, :423-425:
 * "owner pushes the same panel on all 7 links concurrently"); gp-plus_amd/csrc/gpp_push.hip has the protocol.  Every rank creates a
 * channel (two message slots of slot_bytes + a flag page, exported as a GPP_PUSH_HANDLE_BYTES record), the ranks exchange the records
 * by any means (all-gather) and connect (hipIpcOpenMemHandle of every peer's).  Messages are numbered seq = 1, 2, ... in the one order
 * in which every rank moves them.  For message seq, on every rank, in this order:
 *   its owner:   gpp_push_send  — behind what `after_stream` has enqueued so far, on one stream per peer: wait until the peer has
 *                consumed message seq - 2, copy part i (height[i] rows of width[i] bytes at src[i], row pitch spitch[i]: straight
 *                from where it lies, no packing) to byte `offset[i]` of the peer's slot with row pitch dpitch[i], then mark the slot
 *                complete; `after_stream` continues when the message has left.
 *   the others:  gpp_push_recv  — on `stream`: wait until message seq is complete in this rank's slot, then copy part i from byte
 *                offset[i] of the slot (row pitch spitch[i]) to dst[i] (row pitch dpitch[i]).
 *   every rank:  gpp_push_ack   — on `stream`, behind whatever consumed the message: tell every peer that this rank is done with seq.
 * A wait that exceeds GPP_SHARD_TIMEOUT_MS ORs `code` into *status (device memory) and gives up.  gpp_push_destroy: stage 0 drains and
 * unmaps the peers' memory, stage 1 — after every rank's stage 0 — frees this rank's; stage 2 does both.
 */
typedef struct gpp_push* gpp_push_t;
#define GPP_PUSH_HANDLE_BYTES 128
int gpp_push_create(int device, int rank, int nranks, int64_t slot_bytes, gpp_push_t* out, void* handle_out);
int gpp_push_connect(gpp_push_t p, const void* handles /* nranks x GPP_PUSH_HANDLE_BYTES, in rank order */);
int gpp_push_send(gpp_push_t p, void* after_stream, int64_t seq, int32_t* status, int code, int nparts, const void* const* src,
                  const int64_t* spitch, const int64_t* offset, const int64_t* dpitch, const int64_t* width, const int64_t* height);
int gpp_push_recv(gpp_push_t p, void* stream, int64_t seq, int32_t* status, int code, int nparts, void* const* dst, const int64_t* dpitch,
                  const int64_t* offset, const int64_t* spitch, const int64_t* width, const int64_t* height);
int gpp_push_ack(gpp_push_t p, void* stream, int64_t seq);
int gpp_push_info(gpp_push_t p, int64_t* slot_bytes, int* flag_kind /* 0 uncached, 1 fine-grained, 2 ordinary device memory */);
int gpp_push_destroy(gpp_push_t p, int stage);

/* Products with a lower-triangular T of which only the block-cyclically owned COLUMN blocks (width nb, a multiple of 64; block
 * b owned when b % nranks == rank) exist on this rank:  trans = 0: y_i = sum over owned columns k <= i of T[i][k] x_k (this
 * rank's part of z = L^-1 r);  trans = 1: y_k = sum_{i >= k} T[i][k] x_i for the owned columns k and 0 for the others (this
 * rank's entries of alpha = L^-T z).  The caller sums the results of all ranks (one all-reduce of N doubles each). */
int gpp_trmv_lower_cols(gpp_handle_t h, const double* T, int64_t ldt, int64_t N, const double* x, double* y, int64_t nb, int rank,
                        int nranks, int trans, int compact);

/* out3 = { quad = z'z, logdet = 2 sum log U_ii, mll = -0.5*(quad + logdet + N log 2pi) } from a z the caller already holds
 * (the second half of gpp_mll_reduce; optim/mll_torch.py:116). */
int gpp_mll_scalars(gpp_handle_t h, const double* U, int64_t ld, int64_t N, const double* z, double* out3);

/* The share of gpp_lauum owned by one rank of a sharded evaluation: the 128-row tile rows t of Kinv with
 * t % nranks == rank, in ONE launch (cyclic at tile granularity: every rank gets the same mix of short and long rows).
 * Linv must be complete on this rank; the other tile rows of Kinv are not touched. */
int gpp_lauum_rows(gpp_handle_t h, const double* Linv, int64_t N, int64_t ldi, double* Kinv, int64_t ldk, int rank, int nranks);

/* The part of that share inside the rows [row0, row1) of Kinv (row0 a multiple of 128): what one rank can form as soon as
 * the column blocks 0 .. row1 of the inverse have arrived — Kinv[i, j <= i] needs the columns i and j of Linv only — so the
 * product is pipelined with the broadcasts of the inverse's column blocks (gp-plus_amd/sharded.py).  The reference has no
 * counterpart (single-process ATen cholesky_backward, optim/mll_torch.py:117). */
int gpp_lauum_rows_range(gpp_handle_t h, const double* Linv, int64_t N, int64_t ldi, double* Kinv, int64_t ldk, int rank,
                         int nranks, int64_t row0, int64_t row1);

/* dst[c][r] = src[r][c] (rows x cols, out of place, 64 x 64 tiles through LDS): the mirror L^-T of a column block of the inverse
 * that arrived from another rank (gp-plus_amd/sharded.py); on the single-GPU path the mirror is written by the GEMM epilogue. */
int gpp_transpose(gpp_handle_t h, const double* src, int64_t lds, int64_t rows, int64_t cols, double* dst, int64_t ldd);

/*
 * K6 (gpytorch MultivariateNormal.log_prob -> inv_quad_logdet, optim/mll_torch.py:116):
 *   z = Linv r;  out3 = { quad = z'z, logdet = 2 sum log U_ii, mll = -0.5*(quad + logdet + N log 2pi) }
 */
int gpp_mll_reduce(gpp_handle_t h, const double* U, int64_t ld, const double* Linv, int64_t ldi, int64_t N,
                   const double* r, double* z, double* out3);

/* alpha = Linv^T z = Ky^-1 r (gpytorch prediction_strategy mean_cache; dMLL/dmean) */
int gpp_alpha(gpp_handle_t h, const double* Linv, int64_t ldi, int64_t N, const double* z, double* alpha);

/*
 * K7 reduction (autograd backward of K1-K4, optim/mll_torch.py:117), with W = 0.5*(alpha alpha' - Kinv):
 *   g_w[d]   = sum_ij W_ij dKy_ij/dw_d        g_sf2 = sum_ij W_ij K_ij / sf2
 *   g_tau[s] = sum_{i in s} W_ii              g_U[i,d] = dMLL/dU_id for d < dU (dU may be 0)
 * K_ij is recomputed from U in registers; only the lower triangle of Kinv is read.
 */
int gpp_grad_reduce(gpp_handle_t h, const double* U, int64_t N, int D, const double* w, const double* sf2,
                    const int32_t* grp, int S, int kind, int d_split, const double* alpha, const double* Kinv,
                    int64_t ldk, int dU, double* g_w, double* g_sf2, double* g_tau, double* g_U);

/*
 * Leave-one-out pseudo-likelihood (Rasmussen & Williams 5.4.2; gpytorch LeaveOneOutPseudoLikelihood).  The reference names a LOOCV
 * criterion (optim/mll_noise_continuation.py:54) and only ever computes the scalar error of :28-42; there is no call site to replace.
 * With P = Ky^-1, alpha = P (y - m) and d = diag(P):
 *   d[i] = sum_{j >= i} Linv[i][j]^2   (row i of the Linv buffer from the diagonal on: column i of L^-1 through the mirror)
 *   mu[i] = y[i] - alpha[i] / d[i]      s2[i] = 1 / d[i]                       (leave-one-out predictive mean and variance)
 *   a[i]  = -alpha[i] / d[i]            sqrtb[i] = sqrt(1 / (2 d[i]) + alpha[i]^2 / (2 d[i]^2))
 *   loo[0] = sum_i [ 0.5 log d[i] - alpha[i]^2 / (2 d[i]) ] - (N / 2) log 2 pi
 * Linv: the complete inverse factor with its mirror.  mu (with y), s2, a, sqrtb and loo may each be NULL; d is always written.
 * Deterministic: a row's sum does not depend on the launch shape, and loo is added in a fixed order (no atomics).
 */
int gpp_loo_scalars(gpp_handle_t h, const double* Linv, int64_t ldi, int64_t N, const double* alpha, const double* y, double* d,
                    double* mu, double* s2, double* a, double* sqrtb, double* loo);

/* S[i,j] = s[i] * Kinv[max(i,j), min(i,j)] for 0 <= i, j < N: the FULL square, row-scaled, from the LOWER triangle of Kinv (as the
 * LAUUM leaves it; nothing above its diagonal is read).  Out of place (S != Kinv).  With s = sqrtb the lower triangle of
 * P diag(b) P is the TN product S^T S (gpp_gemm with transA = 1, c_tri = 1).  Columns [N, lds) of S are not written. */
int gpp_sym_rowscale(gpp_handle_t h, const double* Kinv, int64_t N, int64_t ldk, const double* s, double* S, int64_t lds);

/*
 * The K7 reduction with the weights of the leave-one-out pseudo-likelihood: W_ij = -0.5 (alpha_i beta_j + beta_i alpha_j) - C_ij,
 * beta = P a and C = P diag(b) P (LOWER triangle read).  g_w, g_sf2, g_tau, g_U are defined as for gpp_grad_reduce with this W;
 * the same kinds, d_split, D, S, dU, workspace and bitwise repeatability.  dLOO/dmean = -beta, dLOO/dy = +beta.
 */
int gpp_loo_grad_reduce(gpp_handle_t h, const double* U, int64_t N, int D, const double* w, const double* sf2,
                        const int32_t* grp, int S, int kind, int d_split, const double* alpha, const double* beta,
                        const double* C, int64_t ldc, int dU, double* g_w, double* g_sf2, double* g_tau, double* g_U);

/*
 * Gradient of the MLL by calibration parameters (reference models/gp_plus.py:439-461 writes theta_k into input column k of every
 * row of the calibrated source and leaves the derivative to autograd).  With member[i] != 0 for the rows that carry theta, cols[k]
 * the feature column of theta_k (0 <= cols[k] < D, 1 <= C <= D) and W = 0.5 (alpha alpha' - Kinv):
 *   g_theta[k] = sum_ij W_ij (m_i - m_j) dK_ij/du_{i,cols[k]}  =  sum_{i: member[i] != 0} g_U[i, cols[k]] of gpp_grad_reduce
 * without an N x D block of feature gradients.  The noise diagonal does not depend on theta; pairs of one source contribute an exact
 * zero (all rows members, or none: g_theta = 0.0), and 64 x 64 tiles with one membership throughout are skipped unread.  Only the
 * LOWER triangle of Kinv is read (as gpp_lauum leaves it); all three kinds, cols[k] on either side of d_split.  One record per
 * work-group in the handle workspace (gpp_workspace_bytes(GPP_OP_MLL_EVAL) covers it), added in index order: no atomics, the result
 * depends on the sizes alone, bit for bit.
 */
int gpp_calib_grad_reduce(gpp_handle_t h, const double* U, int64_t N, int D, const double* w, const double* sf2, int kind,
                          int d_split, const double* alpha, const double* Kinv, int64_t ldk, const int32_t* member,
                          const int32_t* cols, int C, double* g_theta);

/*
 * The same reduction restricted to the block rows of Kinv this rank owns in a sharded evaluation (SURVEY.md §8(e) mode 2;
 * BASELINE config 5): rows [b*nb, (b+1)*nb) with b % nranks == rank (nb a multiple of 64).  Only those rows of Kinv are
 * read; the outputs are this rank's PARTIAL sums (the caller all-reduces them).  nranks == 1 is gpp_grad_reduce.
 */
int gpp_grad_reduce_rows(gpp_handle_t h, const double* U, int64_t N, int D, const double* w, const double* sf2,
                         const int32_t* grp, int S, int kind, int d_split, const double* alpha, const double* Kinv,
                         int64_t ldk, int dU, int64_t nb, int rank, int nranks, double* g_w, double* g_sf2, double* g_tau,
                         double* g_U);

/* The same reduction over the block-cyclically owned COLUMN blocks of Kinv's lower triangle (columns [b*nb, (b+1)*nb) with
 * b % nranks == rank): what a rank holds after the sharded back-substitution (gpp_gemm_lower_cols). */
int gpp_grad_reduce_cols(gpp_handle_t h, const double* U, int64_t N, int D, const double* w, const double* sf2,
                         const int32_t* grp, int S, int kind, int d_split, const double* alpha, const double* Kinv,
                         int64_t ldk, int dU, int64_t nb, int rank, int nranks, double* g_w, double* g_sf2, double* g_tau,
                         double* g_U, int compact);

/*
 * K8 (models/gpregression.py:122-149 predict): V = Ksn Linv^T (M x N, scratch, may be NULL to skip var),
 *   mean_out[a] = sum_j Ksn[a,j] alpha[j],   var_out[a] = kss[a] - sum_j V[a,j]^2
 */
int gpp_predict(gpp_handle_t h, const double* Linv, int64_t ldi, int64_t N, const double* alpha, const double* Ksn,
                int64_t lds, int64_t M, const double* kss, double* V, int64_t ldv, double* mean_out, double* var_out);

/* The same prediction from the TRANSPOSED cross block Kns (N x M: gpp_cross_kernel with the training points as rows) and
 * z = Linv r (gpp_mll_reduce):  V = Kns^T Linv^T as a row-contiguous TN product against the mirror in Linv's upper triangle,
 * mean_out[a] = sum_j V[a,j] z[j],  var_out[a] = kss[a] - sum_j V[a,j]^2.  The form to use when the variance is wanted (the product
 * is ~1.7x faster than gpp_predict's); for the mean alone gpp_predict with V = NULL is O(M N).  (models/gpregression.py:122-149) */
int gpp_predict_tn(gpp_handle_t h, const double* Linv, int64_t ldi, int64_t N, const double* z, const double* Kns, int64_t ldk,
                   int64_t M, const double* kss, double* V, int64_t ldv, double* mean_out, double* var_out);

/* Backward of a prediction (models/gp_plus.py predict_with_grad): with G = gmean (x) alpha + diag(gvar) B (never formed) and
 * K = sf2 k(Ua, Ub; w) recomputed in registers (kind / d_split as in gpp_cross_kernel),
 *   g_Ua[a,d] = sum_j G_aj dK_aj/dUa_ad  (d < dA),   g_Ub[j,d] = sum_a G_aj dK_aj/dUb_jd  (d < dB),
 *   g_w[d] = sum_aj G_aj dK_aj/dw_d,   g_sf2 = sum_aj G_aj K_aj / sf2.
 * Ua: M x D, Ub: N x D row-major; gmean (M) and alpha (N) may both be NULL, and so may gvar (M) and B (M x N, ldb >= N even,
 * 16-byte aligned).  Every output may be NULL (g_Ua / g_Ub with dA / dB = 0).  Deterministic: per-work-group partial sums in
 * the handle workspace (gpp_workspace_bytes(GPP_OP_PREDICT_GRAD, N, M, D, dB)), added in a fixed order; no atomics.
 * For the variance the caller passes gvar = -2 dL/dvar and B = K_*N Ky^-1, and adds sum(dL/dvar) to g_sf2 itself. */
int gpp_cross_grad(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                   const double* sf2, int kind, int d_split, const double* gmean, const double* alpha, const double* gvar,
                   const double* B, int64_t ldb, double* g_Ua, int dA, double* g_Ub, int dB, double* g_w, double* g_sf2);

/*
 * The fp64 MFMA GEMM behind all of the above, exported for the parity tests:
 *   C = beta*C + alpha*op(A)*op(B),  op(A): M x K, op(B): K x N, all row-major.
 * transA: 0 = A stored M x K, 1 = A stored K x M;  transB: 0 = B stored K x N, 1 = B stored N x K.
 * Supported (transA,transB): (0,1) "NT", (0,0) "NN", (1,0) "TN".
 * a_mask/b_mask: 0 none, 1 keep entries with k <= row, 2 keep entries with k >= row (row = m for A, n for B);
 * c_tri: 0 full output, 1 only entries with n <= m, 2 only entries with n >= m (M == N); every other entry of C is left as it is.
 * klo_mode / khi_mode: the range of k each work-group tile runs over, from the tile's own first row m0 and first column n0 and its
 * own edge (TM rows x TN columns, chosen by the launcher: 32, 64 or 128) —
 *   klo_mode: 0 -> 0, 1 -> m0, 2 -> n0, 3 -> max(m0, n0);   khi_mode: 0 -> K, 1 -> min(K, m0 + TM), 2 -> min(K, n0 + TN).
 * A mode is a HINT that saves the chunks the masks zero anyway: it is valid only where the masks already exclude every k outside
 * the range, and under that condition the result does not depend on the tile (nor, bit for bit, on the hint).  The legal pairs:
 *   khi_mode 1 needs a_mask 1,  khi_mode 2 needs b_mask 1,  klo_mode 1 needs a_mask 2,  klo_mode 2 needs b_mask 2,
 *   klo_mode 3 needs a_mask 2 and b_mask 2.
 * Any other combination drops terms of the product, differently for every tile size.  A tile whose range is empty (khi <= klo)
 * gets beta*C.  lda, ldb, ldc: even; A, B, C: 16-byte aligned; a row's last 16-byte load may read one double past an odd extent,
 * inside ld.
 */
int gpp_gemm(gpp_handle_t h, int transA, int transB, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
             int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc, int a_mask, int b_mask,
             int klo_mode, int khi_mode, int c_tri);

/* `batch` independent products of the same shape in one launch: element b uses A + b*sA, B + b*sB, C + b*sC (strides in
 * elements, even; sA = 0 shares A).  Used by the sharded inverse, whose column blocks sit at a regular column spacing. */
int gpp_gemm_batched(gpp_handle_t h, int transA, int transB, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
                     int64_t lda, int64_t sA, const double* B, int64_t ldb, int64_t sB, double beta, double* C, int64_t ldc,
                     int64_t sC, int batch, int a_mask, int b_mask, int klo_mode, int khi_mode, int c_tri);

/*
 * Batched evaluation: `batch` independent problems of the SAME size N in every launch (the restarts of a multistart
 * fit, optim/mll_torch.py:99-141, evaluated together instead of one after the other).  Element b uses the matrices at
 * base + b*s? (strides in elements, even), parameters w + b*D, sf2 + b, tau + b*S, vectors r/z/alpha + b*sv (sv >= N,
 * even), out3 + 3*b, info_dev + b, and returns g_w + b*D, g_sf2 + b, g_tau + b*S, g_U + b*N*dU.  sU = 0 shares one
 * feature matrix.  N is at most 6144 for gpp_potrf_batched (the leaf-step
 * factorisation); gpp_trtri_batched completes the inverse from the 128-blocks, so it follows gpp_potrf_batched
 * directly.  The workspace must hold batch * gpp_workspace_bytes(GPP_OP_MLL_EVAL, ...).
 */
int gpp_kernel_build_batched(gpp_handle_t h, const double* U, int64_t sU, int64_t N, int D, const double* w, const double* sf2,
                             const double* tau, const int32_t* grp, int S, double jitter, int kind, int d_split, int uplo,
                             double* Ky, int64_t ld, int64_t sK, int batch);
int gpp_potrf_batched(gpp_handle_t h, double* A, int64_t N, int64_t ld, int64_t sA, double* Linv, int64_t ldi, int64_t sLi,
                      int32_t* info_dev, int batch);
int gpp_trtri_batched(gpp_handle_t h, const double* U, int64_t N, int64_t ld, int64_t sA, double* Linv, int64_t ldi,
                      int64_t sLi, double* T, int64_t ldt, int64_t sT, int batch);
int gpp_lauum_batched(gpp_handle_t h, const double* Linv, int64_t N, int64_t ldi, int64_t sLi, double* Kinv, int64_t ldk,
                      int64_t sK, int batch);
int gpp_mll_reduce_batched(gpp_handle_t h, const double* U, int64_t ld, int64_t sA, const double* Linv, int64_t ldi,
                           int64_t sLi, int64_t N, const double* r, double* z, int64_t sv, double* out3, int batch);
int gpp_alpha_batched(gpp_handle_t h, const double* Linv, int64_t ldi, int64_t sLi, int64_t N, const double* z, double* alpha,
                      int64_t sv, int batch);
int gpp_grad_reduce_batched(gpp_handle_t h, const double* U, int64_t sU, int64_t N, int D, const double* w, const double* sf2,
                            const int32_t* grp, int S, int kind, int d_split, const double* alpha, int64_t sv,
                            const double* Kinv, int64_t ldk, int64_t sK, int dU, double* g_w, double* g_sf2, double* g_tau,
                            double* g_U, int batch);

/* The leave-one-out pseudo-likelihood in the same batched form (all restarts of an objective="loo" fit in one launch).  Element b
 * reads Linv + b*sLi and alpha / y + b*sv, writes d / mu / s2 / a / sqrtb + b*sv and loo + b; gpp_sym_rowscale_batched reads
 * Kinv + b*sK and s + b*sv and writes S + b*sS; gpp_loo_grad_reduce_batched is gpp_grad_reduce_batched with beta + b*sv and
 * C + b*sC = P_b diag(b_b) P_b (same workspace, batch * gpp_workspace_bytes(GPP_OP_MLL_EVAL, ...), same output layout).  All strides
 * even, sv >= N.  The kernels, the per-row arithmetic and the summation orders are those of gpp_loo_scalars / gpp_sym_rowscale /
 * gpp_loo_grad_reduce (which are these with batch = 1): an element's results are bitwise those of the single-problem call. */
int gpp_loo_scalars_batched(gpp_handle_t h, const double* Linv, int64_t ldi, int64_t sLi, int64_t N, const double* alpha,
                            const double* y, double* d, double* mu, double* s2, double* a, double* sqrtb, int64_t sv, double* loo,
                            int batch);
int gpp_sym_rowscale_batched(gpp_handle_t h, const double* Kinv, int64_t N, int64_t ldk, int64_t sK, const double* s, int64_t sv,
                             double* S, int64_t lds, int64_t sS, int batch);
int gpp_loo_grad_reduce_batched(gpp_handle_t h, const double* U, int64_t sU, int64_t N, int D, const double* w, const double* sf2,
                                const int32_t* grp, int S, int kind, int d_split, const double* alpha, const double* beta,
                                int64_t sv, const double* C, int64_t ldc, int64_t sC, int dU, double* g_w, double* g_sf2,
                                double* g_tau, double* g_U, int batch);

/*
 * Grouped (k-fold, leave-one-group-out) cross-validation from ONE factorisation.  With P = Ky^-1, alpha = P (y - m) and a fold F (an
 * index set of size m_F), p(y_F | y_-F) = N(y_F - P_FF^-1 alpha_F, P_FF^-1) and
 *   cv = sum_F [ -0.5 alpha_F' P_FF^-1 alpha_F + 0.5 log|P_FF| ] - (N / 2) log 2 pi
 * (folds of one point: the leave-one-out quantities above; one fold of everything: the marginal likelihood).  The reference has no
 * counterpart (optim/mll_noise_continuation.py:54 names LOOCV only).  The folds of a call are a CSR list: idx (int32, off[nfolds]
 * entries, every value in [0, N), ASCENDING inside a fold) and off (int32, nfolds + 1 entries, off[0] = 0 not required).  Both products
 * run on v_mfma_f64_16x16x4_f64 in 64 x 64 tiles, one launch for the whole list; no atomics, no workspace; a fold's output does not
 * depend on the other folds of the call and is bitwise repeatable.
 *
 * gpp_cv_blocks: for fold f the UPPER triangle of the mp x mp block at B + f*sB (m_f <= mp <= ldb, ldb and sB even):
 *   B_f[a][b] = P_FF[a][b] = sum_{j >= max(i_a, i_b)} Linv[i_a][j] Linv[i_b][j]   for a <= b < m_f,  i_a = idx[off[f] + a]
 *   B_f[a][b] = (a == b)                                                           for a <= b, m_f <= b < mp (identity padding: the
 *               block factors to diag(chol P_FF, I), its log-determinant and solves are those of P_FF)
 * Linv: the complete inverse factor with its mirror (row i from the diagonal on = column i of L^-1, as gpp_loo_scalars reads it);
 * row i is read at columns j >= i only, and a tile's chunks start at its smallest gathered index.  The strict lower triangle of a
 * block is never written.
 *
 * gpp_cv_rows: S[off[f] + a][c] = sum_{b < m_f} G_f[a][b] Psq[idx[off[f] + b]][c]   for a < m_f, c < N
 * G_f = G + f*sG: m_f x m_f, row-major with rows of ldg doubles (m_f <= ldg, and m_f * ldg <= sG when nfolds > 1; ldg, sG even); its
 * padding (rows and columns from m_f on) is never read.  Psq: the full symmetric N x N square (gpp_sym_rowscale with s = 1 gives it
 * exactly from the LAUUM's lower triangle).  With G_f'G_f = dcv/dP_FF the rows of S stack G_F P[F, :], and the lower triangle of
 * S'S (gpp_gemm, transA = 1, c_tri = 1) is the matrix C of gpp_loo_grad_reduce.  Columns [N, lds) of S are never written.
 */
int gpp_cv_blocks(gpp_handle_t h, const double* Linv, int64_t ldi, int64_t N, const int32_t* idx, const int32_t* off, int nfolds,
                  int mp, double* B, int64_t ldb, int64_t sB);
int gpp_cv_rows(gpp_handle_t h, const double* G, int64_t ldg, int64_t sG, const int32_t* idx, const int32_t* off, int nfolds,
                const double* Psq, int64_t ldp, int64_t N, double* S, int64_t lds);

/*
 * Border a cached factorisation with q new points in O(N^2 q): no refactorisation (the reference refits, and so refactorises, at every
 * step of bayesian_optimizations/BO_GP_plus.py).  A (the upper factor U = L^T) and Linv (L^-1, lower, with its mirror) hold an N x N
 * window as gpp_potrf + gpp_trtri leave it, inside buffers of at least N + q rows with ld, ldi >= N + q (even; 16-byte aligned).
 *   k:  the cross block K(X, Xq), N x q row-major (ldk >= q, even; 16-byte aligned)
 *   C:  the corner K(Xq, Xq) + noise + jitter, q x q, UPPER triangle read (ldc >= q, even; 16-byte aligned); not modified
 *   rq: the q new residuals y_q - m(Xq);   z = Linv r and alpha = Linv^T z: N entries on entry, room for N + q
 * With V = (Linv k)^T, S = C - V V^T = Ls Ls^T, W = -Ls^-1 (V Linv), zq = Ls^-1 (rq - V z), on success:
 *   A[0..N, N..N+q) = V^T,  A[N.., N..) upper = Ls^T                       (the strict lower triangle of the corner is not written)
 *   Linv[N.., 0..N) = W,  Linv[0..N, N..) = W^T (mirror),  Linv[N.., N..) = Ls^-1 with its mirror
 *   z[N..) = zq,   alpha[0..N) += W^T zq,   alpha[N..) = Ls^-T zq
 * *info_dev is what gpp_potrf reports for S (0, or k > 0: leading minor k of the Schur complement is not positive definite); then
 * the new rows and columns, z[N..) and alpha[N..) are unspecified and alpha[0..N) is left as it was, on both routes.  The N x N
 * windows are never written, whatever happens, and nothing outside the (N + q) x (N + q) extents is read or written.  q <= 16
 * runs dedicated kernels that read the N x N buffer of Linv once
 * (the lower triangle for V, the mirror for V Linv); q > 16 composes gpp_gemm, gpp_potrf and gpp_trtri.  Scratch: the handle
 * workspace, gpp_workspace_bytes(h, GPP_OP_APPEND, N, q, 0, 0) bytes; GPP_NO_WORKSPACE with nothing enqueued when it is missing.
 * Plain launches on the handle's stream, no float atomics, sums in an order fixed by (N, q): two calls agree bit for bit.
 */
int gpp_chol_append(gpp_handle_t h, double* A, int64_t ld, double* Linv, int64_t ldi, int64_t N, int64_t q, const double* k,
                    int64_t ldk, const double* C, int64_t ldc, const double* rq, double* z, double* alpha, int32_t* info_dev);

/*
 * Weighted sum of squared posterior cross-covariances, the numerator of the expected-variance-reduction (ALC / IMSE) score:
 *   out[c] = sum_r omega_r ( sf2 k(Uc_c, Ur_r; w) - sum_{n < K} Vc[c,n] Vr[r,n] )^2
 * Uc (M_c x D) and Ur (M_r x D) are row-major feature rows; kind / d_split as in gpp_cross_kernel.  vt = 0: Vc is M_c x K and Vr is
 * M_r x K, row-major, the V of gpp_predict (ldc, ldr >= K); vt = 1: the transposed operands, Vc K x M_c and Vr K x M_r (ldc >= M_c,
 * ldr >= M_r).  Leading dimensions even, buffers 16-byte aligned.  omega: M_r weights, or NULL for all ones.  out: M_c doubles.
 * K, M_c, M_r >= 1, D <= 64.  The M_c x M_r block never reaches memory: 128 x 128 tiles of Vc Vr^T on the MFMA path of gpp_gemm,
 * whose epilogue regenerates k per entry, subtracts, squares, weights and sums along the tile's columns into one record of 128 row
 * sums per tile in the handle workspace (gpp_workspace_bytes(h, GPP_OP_POST_CROSS, M_r, M_c, 0, 0) bytes; GPP_NO_WORKSPACE with
 * nothing enqueued when it is missing); a second launch adds the column tiles' records in index order.  No float atomics, the number
 * and order of the terms of out[c] depend on (M_r, K) only: two calls agree bit for bit, and a candidate's value does not depend on
 * its row or on the other candidates.  Nothing outside the stated extents is read (the columns [K, ld) may hold anything).
 */
int gpp_post_cross_sq(gpp_handle_t h, const double* Uc, int64_t Mc, const double* Ur, int64_t Mr, int D, const double* w,
                      const double* sf2, int kind, int d_split, const double* Vc, int64_t ldc, const double* Vr, int64_t ldr,
                      int64_t K, int vt, const double* omega, double* out);

/*
 * gpp_post_cross_sq for rows that observe a LINEAR functional of f, a value plus gradient components at the row's point: the
 * numerator of the expected variance reduction of a run that returns y and (part of) its gradient (linalg.py
 * variance_reduction_block; no reference counterpart):
 *   out[i] = sum_r omega_r ( g_i(r) - sum_{n < K} Vf[i,n] Vr[r,n] )^2
 *   g_i(r) = A[i,0] sf2 k(Uf_i, Ur_r; w) + sum_{j < nd} A[i,1+j] 2 w_{d0+j} (Uf[i,d0+j] - Ur[r,d0+j]) m_{f(j)}(i, r)
 * with the multipliers m_0 = -sf2 k and m_1 = sf2 e1 h' of gpp_cross_kernel_dx (h' without a division by r).  A: M_f x (1 + nd)
 * row-major, lda >= 1 + nd; its columns [1 + nd, lda) are never read.  0 <= d0, nd >= 1, d0 + nd <= D <= 64.  Uf, Ur, w, sf2, kind,
 * d_split, vt, Vf / ldf, Vr / ldr (16-byte aligned, even leading dimensions), K, omega (or NULL) and out as in gpp_post_cross_sq, and
 * so are the tiles, the records (gpp_workspace_bytes(h, GPP_OP_POST_CROSS_LIN, M_r, M_f, 0, 0) bytes; GPP_NO_WORKSPACE with nothing
 * enqueued when it is missing) and the second launch.  Per entry: one multiplier pair from one exponential (and one Matern factor),
 * one fma per observed direction on the staged difference sqrt(w_d) (Uf - Ur) with the rounded coefficient A[i,1+j] 2 sqrt(w_d), then
 * fma(A[i,0] sf2, k, -acc), fma(m_0, lin_0, .), fma(m_1, lin_1, .).  Hence: a row with A[i,:] = (1, 0, ..., 0) is bit for bit the
 * gpp_post_cross_sq value of the same operands; a feature with w_d == 0 contributes an exact 0; a row of Uf that equals a row of Ur
 * gives finite values for the Matern kinds and an exact 0 derivative part.  No float atomics, two calls agree bit for bit, and a
 * row's value does not depend on its index or on the other rows.  Nothing outside the stated extents is read or written.
 * Argument codes in the order of the arguments (-11 d0, -12 nd, -13 A, -14 lda, -15 Vf or ldf, -17 Vr or ldr, -19 K, -20 vt, -22 out).
 */
int gpp_post_cross_lin_sq(gpp_handle_t h, const double* Uf, int64_t Mf, const double* Ur, int64_t Mr, int D, const double* w,
                          const double* sf2, int kind, int d_split, int d0, int nd, const double* A, int64_t lda, const double* Vf,
                          int64_t ldf, const double* Vr, int64_t ldr, int64_t K, int vt, const double* omega, double* out);

/*
 * Minima of affine images of the posterior cross-covariance, the reduction of the knowledge gradient under a Q-node quadrature:
 *   out[c*Q + k] = min_{r < M_r} ( m_r + nodes_k scale_c ( sf2 k(Uc_c, Ur_r; w) - sum_{n < K} Vc[c,n] Vr[r,n] ) )
 * Operands, vt, alignment and extents as in gpp_post_cross_sq; m: M_r offsets, scale: M_c factors, nodes: Q values, 1 <= Q <= 64;
 * out: M_c x Q, row-major, contiguous.  The product nodes_k scale_c is rounded once and enters one fma per entry.  The same tiles
 * and the same arithmetic for the cross-covariance as gpp_post_cross_sq; the epilogue leaves Q minima per row and 64-column half of
 * a tile in the handle workspace (gpp_workspace_bytes(h, GPP_OP_POST_CROSS_MIN, M_r, M_c, 0, Q) bytes; GPP_NO_WORKSPACE with nothing
 * enqueued when it is missing) and a second launch takes the minimum of a row's records.  No atomics and no sum across entries:
 * out[c][k] does not depend on the order of the reference rows, on the candidate's row or on the other candidates, bit for bit.
 * Nothing outside the stated extents is read.
 */
int gpp_post_cross_min(gpp_handle_t h, const double* Uc, int64_t Mc, const double* Ur, int64_t Mr, int D, const double* w,
                       const double* sf2, int kind, int d_split, const double* Vc, int64_t ldc, const double* Vr, int64_t ldr,
                       int64_t K, int vt, const double* m, const double* scale, const double* nodes, int Q, double* out);

/*
 * Derivative cross block, for the posterior of the gradient (models/gp_plus.py predict_gradient; no reference counterpart):
 *   Dk[n, a nd + j] = d/du_{d0+j} ( sf2 k(u, Ub_n; w) ) at u = Ua_a = 2 w_{d0+j} (Ua[a,d0+j] - Ub[n,d0+j]) m_f(a, n)
 * with the multipliers of gpp_kernel_apply_grad: m_0 = -sf2 k on a feature of the RBF factor, m_1 = sf2 e1 h' on one of the Matern
 * factor, h' formed without a division by r.  Ua: M x D, Ub: N x D row-major and contiguous; kind / d_split as in gpp_cross_kernel;
 * D <= 64, nd >= 1, 0 <= d0, d0 + nd <= D.  Dk: N x (M nd) row-major — training points as rows, the operand Kns of gpp_predict_tn —
 * ld >= M nd, ld even, 16-byte aligned.  The multiplier (one exp, plus the Matern polynomial) is computed once per pair (a, n) and
 * serves its nd directions.  A feature with w_d == 0 gives an exact 0; a row of Ua that equals a row of Ub gives finite values for
 * the Matern kinds too, and exact zeros in that pair's entries.  The columns [M nd, ld) are never written and nothing outside the
 * stated extents is read.  One plain launch on the handle's stream, no workspace; every entry is a function of its own pair alone,
 * so two launches agree bit for bit.
 */
int gpp_cross_kernel_dx(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                        const double* sf2, int kind, int d_split, int d0, int nd, double* Dk, int64_t ld);

/*
 * Gram matrices of consecutive groups of nd rows, the explained part of the gradient's posterior covariance (Q = Dk^T Linv^T as
 * gpp_predict_tn leaves it, rows = points x directions):
 *   G[a][j][j'] = sum_{n < N} Q[a nd + j][n] Q[a nd + j'][n],          Gsum[j][j'] = sum_{a < M} omega_a G[a][j][j']
 * Q: (M nd) x N row-major, ldq >= N, ldq even, 16-byte aligned; the columns [N, ldq) are never read.  1 <= nd <= 16.  G: M x nd x nd,
 * contiguous, both triangles written and bitwise symmetric; NULL when only the sum is wanted.  Gsum: nd x nd, or NULL; omega: M
 * weights, or NULL for all ones.  G and Gsum may not both be NULL.  A point's matrix is a sum in an order fixed by (N, nd) alone:
 * bit for bit it does not depend on M, on the point's index or on the other points.  Gsum adds the points in index order in two
 * further launches (groups of 32 points, then the groups), whose partial sums — and the points' matrices when G is NULL — go
 * through the handle workspace: gpp_workspace_bytes(h, GPP_OP_POINT_GRAM, 0, M, nd, 0) bytes, needed only with Gsum;
 * GPP_NO_WORKSPACE with nothing enqueued when it is missing.  Plain launches on the handle's stream, no float atomics: two calls
 * agree bit for bit.
 */
int gpp_point_gram(gpp_handle_t h, const double* Q, int64_t ldq, int64_t M, int nd, int64_t N, const double* omega, double* G,
                   double* Gsum);

/*
 * Second-derivative block, the covariance of two gradient observations and of a gradient observation with a predicted gradient
 * (models/gp_plus.py condition_on_gradients; no reference counterpart):
 *   H[a nd + j][b nd + l] = d^2/du_{d0+j} dv_{d0+l} ( sf2 k(u, v; w) ) at u = Ua_a, v = Ub_b
 *                         = g_j g_l D_j D_l m_{f(j)+f(l)} - [j == l] g_j m_{f(j)},      g = 2 w,  D_d = Ua[a,d] - Ub[b,d],
 * f = 0 on a feature of the RBF factor and 1 on one of the Matern factor, m_0 and m_1 the multipliers of gpp_cross_kernel_dx and
 * m_2 = -sf2 e1 h'' with h'' = (25/3) e^-r (Matern 5/2) or 9 e^-r / r (Matern 3/2: the only division; |sqrt(w_j) D_j| <= r / sqrt(6)
 * bounds the term by a multiple of r, and where r == 0 the multiplier is an exact 0, so a pair of equal points keeps the finite
 * prior curvature 6 w_j sf2 e1 on its diagonal and nothing else).  Ua: Ma x D, Ub: Mb x D row-major and contiguous; kind / d_split as
 * in gpp_cross_kernel; D <= 64, nd >= 1, 0 <= d0, d0 + nd <= D.  H: (Ma nd) x (Mb nd) row-major, ld >= Mb nd, ld even, 16-byte
 * aligned.  The multipliers (one exp, plus the Matern polynomial) are computed once per pair (a, b) by the staged arithmetic of
 * gpp_cross_kernel_dx and serve its nd^2 entries; D_d comes from the raw features.  A feature with w_d == 0 gives exact zeros in its
 * whole row and column of every pair's block.  The columns [Mb nd, ld) are never written and nothing outside the stated extents is
 * read.  One plain launch on the handle's stream, no workspace, no atomics; every entry is a function of its own pair alone, so two
 * launches agree bit for bit, and the entries (a, j), (b, l) and (b, l), (a, j) are the same operations on the same numbers: with
 * Ua and Ub the same rows H is bitwise symmetric.
 */
int gpp_kernel_dxdx(gpp_handle_t h, const double* Ua, int64_t Ma, const double* Ub, int64_t Mb, int D, const double* w,
                    const double* sf2, int kind, int d_split, int d0, int nd, double* H, int64_t ld);

/*
 * Gradient of the joint log-likelihood of function values and gradient observations through the two derivative blocks of
 *   Kj = [[Kff, Kfg], [Kfg^T, Kgg]],  Kfg = gpp_cross_kernel_dx(Ua = Ug, Ub = U) (N x q),  Kgg = gpp_kernel_dxdx(Ug, Ug),  q = Mg nd
 * (linalg.py exact_gek_mll; no reference counterpart).  With W = 0.5 (alpha alpha' - Kinv), the convention of gpp_grad_reduce, the
 * call ADDS to g_w (D), g_sf2 (1) and g_U (N x dU) and WRITES g_Ug (Mg x dU):
 *   sum over the entries of Kfg (counted for both triangles) and of Kgg of W_rc dKj_rc/dtheta,   theta = w_d, sf2, U[i, d], Ug[a, d]
 * (g_sf2 as in gpp_grad_reduce: the sum of W_rc Kj_rc / sf2).  The caller adds gpp_grad_reduce on the leading N x N view (ld = n,
 * alpha[:N]) for the Kff block and its own noise terms.  alpha: n = N + q doubles; Kinv: n x n, ld >= n, ld even, 16-byte aligned,
 * LOWER triangle read (as gpp_lauum leaves it), rows N + a nd + j = the gradient observations, point-major.  kind / d_split as in
 * gpp_cross_kernel; D <= 64, nd >= 1, 0 <= d0, d0 + nd <= D; 0 <= dU <= d0, and dU <= d_split on the Matern kinds (a feature with a
 * gradient is none of the differentiated ones and belongs to the RBF factor), -16 otherwise; g_U and g_Ug may be NULL when dU == 0.
 * The Matern kinds need the third derivative of the factor, h''' = -(125/3) e^-r / r (5/2) or -27 e^-r (1/r^2 + 1/r^3) (3/2): it
 * only appears times products of features' differences that vanish faster, which are formed without a division by r == 0; pairs
 * of equal points give finite results and an exact 0 in those terms.  Tiles of 16 x 16 pairs of points, one record of sums per tile
 * and one slot per (tile, point) of the feature gradients in the handle workspace (gpp_workspace_bytes(h, GPP_OP_GEK_GRAD, N, Mg, D,
 * dU) bytes; GPP_NO_WORKSPACE with nothing enqueued when it is missing), added in index order by two finish launches: no float
 * atomics, two calls agree bit for bit.
 */
int gpp_gek_grad_reduce(gpp_handle_t h, const double* U, int64_t N, const double* Ug, int64_t Mg, int D, const double* w,
                        const double* sf2, int kind, int d_split, int d0, int nd, const double* alpha, const double* Kinv,
                        int64_t ldk, int dU, double* g_w, double* g_sf2, double* g_U, double* g_Ug);

/*
 * Partial gradients: the three calls above on a SELECTION of the (point, direction) entries (models/gp_plus.py
 * condition_on_gradients(observed=...); no reference counterpart).  A selection of M points with nd directions each is two DEVICE
 * arrays of int and a count q:
 *   first[M + 1]  first[a] = the number of selected entries of the points before a (first[0] = 0, first[M] = q, non-decreasing;
 *                 a point may have none);
 *   dir[q]        dir[first[a] + k] in [0, nd) = the direction of entry k of point a, strictly increasing within a point.
 * The selected entries are numbered point-major, 0 .. q - 1: entry first[a] + k is row (or column) N-or-0 + first[a] + k wherever the
 * dense calls have a nd + j.  A NULL pair first / dir means "dense on this side": its q must then be M nd, and with every pair NULL
 * the call IS the one above.  Checked on the host, with argument codes: a pair of which one pointer is NULL (the code of dir), q
 * outside [1, M nd] (or != M nd for a NULL pair), the leading dimension against q, the alignment, and everything the dense calls
 * check.  NOT checked — the caller's contract, backend.GradientSelection being the only producer: the arrays' contents as stated
 * above.  Every call writes the compact extents alone (the columns [q, ld) stay untouched), reads nothing outside the stated
 * extents, uses no workspace beyond the dense call's and no float atomics; two calls agree bit for bit, every entry is the dense
 * entry it selects bit for bit, and a selection of all M nd entries gives the bits of the dense call.
 *
 * gpp_cross_kernel_dx_sel: Dk[n, first_a[a] + k] = the dense Dk[n, a nd + dir_a[first_a[a] + k]].  Dk: N x qa, ld >= qa, ld even,
 * 16-byte aligned.  Two columns per lane are paired on the ABSOLUTE compact column, so the 16-byte stores stay aligned where a tile
 * of 16 points starts at an odd column; an odd head or tail is one 8-byte store.
 */
int gpp_cross_kernel_dx_sel(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                            const double* sf2, int kind, int d_split, int d0, int nd, const int* first_a, const int* dir_a, int64_t qa,
                            double* Dk, int64_t ld);

/*
 * gpp_kernel_dxdx on a selection of the rows (first_a, dir_a, qa: Ma points) and / or of the columns (first_b, dir_b, qb: Mb
 * points), as described at gpp_cross_kernel_dx_sel: H: qa x qb row-major, ld >= qb, ld even, 16-byte aligned;
 *   H[first_a[a] + k][first_b[b] + m] = the dense H[a nd + dir_a[first_a[a] + k]][b nd + dir_b[first_b[b] + m]].
 * With Ua and Ub the same rows and the same selection on both sides H is bitwise symmetric.
 */
int gpp_kernel_dxdx_sel(gpp_handle_t h, const double* Ua, int64_t Ma, const double* Ub, int64_t Mb, int D, const double* w,
                        const double* sf2, int kind, int d_split, int d0, int nd, const int* first_a, const int* dir_a, int64_t qa,
                        const int* first_b, const int* dir_b, int64_t qb, double* H, int64_t ld);

/*
 * gpp_gek_grad_reduce for q selected gradient observations (first, dir, q: Mg points; described at gpp_cross_kernel_dx_sel):
 * n = N + q, alpha: n doubles, Kinv: n x n with ld >= n, the gradient observations in the rows N + first[a] + k.  The sums of a pair
 * of points run over the selected directions of its points in the order of k; the explicit-weight terms of entry k go to
 * g_w[d0 + dir[first[a] + k]]; g_Ug of a point without an entry is an exact 0.  Workspace, finish launches and the codes from dU on
 * (moved by the three arguments) as gpp_gek_grad_reduce: gpp_workspace_bytes(h, GPP_OP_GEK_GRAD, N, Mg, D, dU) bytes.
 */
int gpp_gek_grad_reduce_sel(gpp_handle_t h, const double* U, int64_t N, const double* Ug, int64_t Mg, int D, const double* w,
                            const double* sf2, int kind, int d_split, int d0, int nd, const int* first, const int* dir, int64_t q,
                            const double* alpha, const double* Kinv, int64_t ldk, int dU, double* g_w, double* g_sf2, double* g_U,
                            double* g_Ug);

/*
 * The three calls above for `batch` problems of the same sizes in one launch each (batched.py batched_gek_mll: all restarts of an
 * objective="gek" fit evaluated together; no reference counterpart).  The tile bodies, the per-entry arithmetic and every order of
 * summation are those of the single-problem calls, the element being a further grid dimension: element b of a batched call gives
 * the bits of the single-problem call on element b's operands.  Element b reads the feature rows at base + b*s (strides in doubles;
 * 0 = one block of rows shared by every element, each side with a stride of its own), w + b*D and sf2 + b.  ONE selection serves every
 * element: first / dir / q as in the _sel calls, a NULL pair for the dense layout (q is then M nd).
 *   gpp_cross_kernel_dx_batched  writes Dk + b*sDk (N x qa, leading dimension ld);
 *   gpp_kernel_dxdx_batched      writes H + b*sH (qa x qb, leading dimension ld);
 *   gpp_gek_grad_reduce_batched  reads alpha + b*sv (n = N + q doubles) and Kinv + b*sK (n x n, leading dimension ldk, lower triangle),
 *                                ADDS to g_w + b*D, g_sf2 + b and g_U + b*N*dU and WRITES g_Ug + b*Mg*dU (contiguous over the batch).
 * A window of a larger matrix is a base, a leading dimension and the stride of that matrix: the builders write the blocks
 * A_b[:N, N:n] and A_b[N:n, N:n] of a batched joint matrix in place when N is even.  The reduction keeps each element's tile records
 * and slots in a slice of the handle workspace of its own, batch * gpp_workspace_bytes(h, GPP_OP_GEK_GRAD, N, Mg, D, dU) bytes in all
 * (GPP_NO_WORKSPACE with nothing enqueued when it is smaller); no float atomics.  Argument codes: those of the _sel call of the same
 * name for what the two share (counted in ITS argument list), and for the batch alone -30 an odd stride (every stride must be even:
 * the elements behind the first keep the 16-byte alignment of the base), -31 batch outside 1 .. 65535, -32 a stride that is neither 0
 * (feature rows only) nor at least an element's extent.
 */
int gpp_cross_kernel_dx_batched(gpp_handle_t h, const double* Ua, int64_t sUa, int64_t M, const double* Ub, int64_t sUb, int64_t N, int D,
                                const double* w, const double* sf2, int kind, int d_split, int d0, int nd, const int* first_a,
                                const int* dir_a, int64_t qa, double* Dk, int64_t ld, int64_t sDk, int batch);
int gpp_kernel_dxdx_batched(gpp_handle_t h, const double* Ua, int64_t sUa, int64_t Ma, const double* Ub, int64_t sUb, int64_t Mb, int D,
                            const double* w, const double* sf2, int kind, int d_split, int d0, int nd, const int* first_a,
                            const int* dir_a, int64_t qa, const int* first_b, const int* dir_b, int64_t qb, double* H, int64_t ld,
                            int64_t sH, int batch);
int gpp_gek_grad_reduce_batched(gpp_handle_t h, const double* U, int64_t sU, int64_t N, const double* Ug, int64_t sUg, int64_t Mg, int D,
                                const double* w, const double* sf2, int kind, int d_split, int d0, int nd, const int* first,
                                const int* dir, int64_t q, const double* alpha, int64_t sv, const double* Kinv, int64_t ldk, int64_t sK,
                                int dU, double* g_w, double* g_sf2, double* g_U, double* g_Ug, int batch);

#ifdef __cplusplus
}
#endif
#endif /* GPP_H */

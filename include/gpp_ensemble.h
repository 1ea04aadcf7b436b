/* gpp_ensemble.h — C ABI of libgpp_ensemble_hip.so: prediction for hyperparameter ensembles on the handle of libgpp_hip.so (gpp.h).
 * A library of its own, so that libgpp_hip.so — and the source signature its version string reports — is untouched by it.  The
 * handle is the one gpp_create returns; its stream (gpp_set_stream) and scratch workspace (gpp_set_workspace) are used.
 * Status codes as in gpp.h: 0, -(index of the offending argument), GPP_NO_WORKSPACE, 1000 + a HIP error. */
#ifndef GPP_ENSEMBLE_H
#define GPP_ENSEMBLE_H
#include "gpp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* "gpp_ensemble <version> (gfx950; src <hash of gpp_ensemble.hip, gpp_internal.h, gpp.h and this file>)" */
const char* gpp_ensemble_version(void);

/* bytes of handle workspace the two calls below need: batch * ceil(N / 64) * M * 2 doubles (0 for a non-positive argument) */
size_t gpp_predict_gen_workspace_bytes(int64_t N, int64_t M, int batch);

/*
 * Prediction from a GENERATED cross block, batched over parameter sets (the members of a hyperparameter ensemble; the reference's
 * multi-pass ensembles, models/gp_plus.py:387-396, 474-482, predict pass by pass).  Element b reads Ua + b*sUa (M x D test features),
 * Ub + b*sUb (N x D training features), w + b*D, sf2 + b, Linv + b*sLi and z + b*sv with z = Linv (y - m) as gpp_mll_reduce_batched
 * leaves it, and writes mean_out + b*so and var_out + b*so:
 *   mean[a] = sum_j V[a,j] z_j,   var[a] = sf2_b - sum_j V[a,j]^2,   V = K_*N L^-T,   K_*N[a,j] = sf2_b k(Ua_a, Ub_j; w_b)
 * i.e. gpp_predict_tn with kss = sf2, but neither the cross block nor V reaches memory: the kernel is gpp_kernel_apply's tile with
 * C = L^-T, the mirror in the UPPER triangle of the Linv buffer (the strictly lower triangle is never read), walking j < min(N,
 * s0 + 64) for the column tile that starts at s0, one work-group per (64 rows, column tile, element) and no split of the contracted
 * index.  Each tile reduces its rows to the pair (sum V z, sum V^2) in a fixed order and writes it to a record [b][column tile][row]
 * in the handle workspace (gpp_predict_gen_workspace_bytes(N, M, batch) bytes, attached with gpp_set_workspace; GPP_NO_WORKSPACE with nothing enqueued
 * when it is missing or smaller); a finish launch adds the column tiles in their order.  No atomics: two launches agree bit for bit, a
 * row's result does not depend on the other rows of the call, and an element's results are bitwise those of gpp_predict_gen (which
 * is the batched call with batch = 1) on its operands.  sUa = 0 / sUb = 0 share the features across elements.  M, N >= 1, D <= 64,
 * kind / d_split as gpp_cross_kernel; Linv and z 16-byte aligned, ldi even and >= N; every stride even, sv >= N, so >= M.
 */
int gpp_predict_gen(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w, const double* sf2,
                    int kind, int d_split, const double* Linv, int64_t ldi, const double* z, double* mean_out, double* var_out);
int gpp_predict_gen_batched(gpp_handle_t h, const double* Ua, int64_t sUa, int64_t M, const double* Ub, int64_t sUb, int64_t N, int D,
                            const double* w, const double* sf2, int kind, int d_split, const double* Linv, int64_t ldi, int64_t sLi,
                            const double* z, int64_t sv, double* mean_out, double* var_out, int64_t so, int batch);

#ifdef __cplusplus
}
#endif
#endif

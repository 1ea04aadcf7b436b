// gpp_reduce.hip — the O(N^2), HBM-bound reductions of the exact-GP path.
//
// Reference call sites replaced:
//   optim/mll_torch.py:116  MultivariateNormal.log_prob -> gpytorch inv_quad_logdet (triangular solve, diag log-sum)
//   optim/mll_torch.py:117  loss.backward(): the backward of exp / distance / outputscale / noise-add, i.e.
//                           dMLL/dtheta = sum_ij W_ij dKy_ij/dtheta with W = 0.5 (alpha alpha' - Ky^-1)
//   models/gpregression.py:142-147  predictive mean and variance
// Every matrix is streamed exactly once; all reductions are two-stage and deterministic (no float atomics).
#include "gpp_internal.h"

#include <algorithm>

typedef double v2d __attribute__((ext_vector_type(2)));

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// red[0] = the sum of v over the 256 threads of a work-group, through the LDS array red[256]: a fixed tree, so a sum's order never
// depends on the run.  The finish kernels' sum.  (The pointer carries the LDS address space: through a generic one the compiler forms
// the tree's last step differently.  The record loops that end gpp_grad_tiles and gpp_pgrad_tiles write the same tree out: called
// inside a loop the helper's comparisons are hoisted out of it, which changes the code of the RBF instantiations.)
typedef __attribute__((address_space(3))) double lds_double;
__device__ __forceinline__ void block_sum(int tid, double v, lds_double* red) {
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
}

// y_i = sum_{k<=i} T[i][k] x_k : one wave per row, rows interleaved over waves so long and short rows mix.
__global__ __launch_bounds__(256) void gpp_trmv_lower(const double* __restrict__ T, int64_t ldt, int64_t N,
                                                      const double* __restrict__ x, double* __restrict__ y, int64_t sT,
                                                      int64_t sv) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= N) return;
  T += (int64_t)blockIdx.y * sT;  // batch element
  x += (int64_t)blockIdx.y * sv;
  y += (int64_t)blockIdx.y * sv;
  const double* row = T + i * ldt;
  double acc = 0.0;
  const int64_t len = i + 1;
  const int64_t len2 = len & ~(int64_t)1;
  for (int64_t k = 2 * lane; k < len2; k += 128) {
    const v2d t = *reinterpret_cast<const v2d*>(row + k);
    const v2d xx = *reinterpret_cast<const v2d*>(x + k);
    acc = fma(t.x, xx.x, acc);
    acc = fma(t.y, xx.y, acc);
  }
  if (lane == 0 && (len & 1)) acc = fma(row[len - 1], x[len - 1], acc);
  acc = wave_sum(acc);
  if (lane == 0) y[i] = acc;
}

// y_j = sum_{i>=j} T[j][i] x_i for the UPPER triangle of T: one wave per row (the mirror of gpp_trmv_lower).
__global__ __launch_bounds__(256) void gpp_trmv_upper(const double* __restrict__ T, int64_t ldt, int64_t N,
                                                      const double* __restrict__ x, double* __restrict__ y, int64_t sT,
                                                      int64_t sv) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + wave;
  if (j >= N) return;
  T += (int64_t)blockIdx.y * sT;  // batch element
  x += (int64_t)blockIdx.y * sv;
  y += (int64_t)blockIdx.y * sv;
  const double* row = T + j * ldt;
  double acc = 0.0;
  int64_t k0 = j;
  if (k0 & 1) {  // align the vector loop to an even column
    if (lane == 0) acc = fma(row[k0], x[k0], acc);
    ++k0;
  }
  const int64_t nvec = (N - k0) >> 1;
  for (int64_t v = lane; v < nvec; v += 64) {
    const v2d t = *reinterpret_cast<const v2d*>(row + k0 + 2 * v);
    const v2d xx = *reinterpret_cast<const v2d*>(x + k0 + 2 * v);
    acc = fma(t.x, xx.x, acc);
    acc = fma(t.y, xx.y, acc);
  }
  if (lane == 0 && ((N - k0) & 1)) acc = fma(row[N - 1], x[N - 1], acc);
  acc = wave_sum(acc);
  if (lane == 0) y[j] = acc;
}

// Column-sharded products with a lower-triangular T of which this rank holds only the column blocks it owns (block-cyclic:
// columns [b*nb, (b+1)*nb) with b % nranks == rank): the sharded evaluation's z = L^-1 r and alpha = L^-T z from the owned
// column blocks of L^-1 (the caller all-reduces the partial results).
//   y_i = sum over owned columns k <= i of T[i][k] x_k        (one wave per row; other columns are never read)
// compact: T holds ONLY the owned column blocks, side by side (the q-th owned block, global block rank + q nranks, in columns
// [q nb, (q+1) nb)): N x (N / nranks) doubles per rank instead of N x N.
__global__ __launch_bounds__(256) void gpp_trmv_lower_cols(const double* __restrict__ T, int64_t ldt, int64_t N,
                                                           const double* __restrict__ x, double* __restrict__ y, int64_t nb,
                                                           int rank, int nranks, int compact) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= N) return;
  const double* row = T + i * ldt;
  double acc = 0.0;
  int64_t q = 0;
  for (int64_t c0 = (int64_t)rank * nb; c0 <= i; c0 += (int64_t)nranks * nb, ++q) {
    const int64_t c1 = (c0 + nb < i + 1) ? c0 + nb : i + 1;  // nb is even: c0 is, so the 16-byte loads are aligned
    const int64_t len = c1 - c0, len2 = len & ~(int64_t)1;
    const double* seg = row + (compact ? q * nb : c0);
    for (int64_t k = 2 * lane; k < len2; k += 128) {
      const v2d t = *reinterpret_cast<const v2d*>(seg + k);
      const v2d xx = *reinterpret_cast<const v2d*>(x + c0 + k);
      acc = fma(t.x, xx.x, acc);
      acc = fma(t.y, xx.y, acc);
    }
    if (lane == 0 && (len & 1)) acc = fma(seg[len - 1], x[c1 - 1], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) y[i] = acc;
}

//   y_k = sum_{i >= k} T[i][k] x_i   for the owned columns k, 0 for the others.  Work-group (g, r): 64 columns (lane = column,
//   coalesced along the row) x the r-th chunk of rows, the four waves striding over the rows with eight loads in flight each;
//   the chunks' partial sums are added in a fixed order by the second kernel (deterministic, no float atomics).
constexpr int TRT_CHUNKS = 16;
__global__ __launch_bounds__(256) void gpp_trmv_lower_t_cols(const double* __restrict__ T, int64_t ldt, int64_t N,
                                                             const double* __restrict__ x, double* __restrict__ part, int64_t nb,
                                                             int rank, int nranks, int64_t chunk, int compact) {
  __shared__ double red[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k0 = (int64_t)blockIdx.x * 64, k = k0 + lane;
  const bool owned = (int)((k0 / nb) % nranks) == rank;  // nb is a multiple of 64: a group of 64 columns has one owner
  double acc = 0.0;
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = (r0 + chunk < N) ? r0 + chunk : N;
  if (owned && k < N && r1 > k0) {
    int64_t i = (r0 > k0 ? r0 : k0) + wave;
    const double* p = T + (compact ? ((k0 / nb) / nranks) * nb + (k0 % nb) + lane : k);
    for (; i + 28 < r1; i += 32) {  // rows i, i+4, ..., i+28 of this wave: eight independent loads
      double t[8], xv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        t[u] = p[(i + 4 * u) * ldt];
        xv[u] = x[i + 4 * u];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = (i + 4 * u >= k) ? fma(t[u], xv[u], acc) : acc;
    }
    for (; i < r1; i += 4)
      if (i >= k) acc = fma(p[i * ldt], x[i], acc);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && k < N) part[(int64_t)blockIdx.y * N + k] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}
__global__ __launch_bounds__(256) void gpp_trmv_lower_t_finish(const double* __restrict__ part, int64_t N, int chunks,
                                                               double* __restrict__ y) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= N) return;
  double s = 0.0;
  for (int r = 0; r < chunks; ++r) s += part[(int64_t)r * N + k];
  y[k] = s;
}

// out3 = { quad = z'z, logdet = 2 sum log L_ii, mll = -0.5 (quad + logdet + N log 2pi) } : one work-group.
__global__ __launch_bounds__(1024) void gpp_mll_scalars(const double* __restrict__ L, int64_t ld, int64_t N,
                                                        const double* __restrict__ z, double* __restrict__ out3, int64_t sL,
                                                        int64_t sv) {
  __shared__ double sq[16], sl[16];
  L += (int64_t)blockIdx.x * sL;  // batch element
  z += (int64_t)blockIdx.x * sv;
  out3 += 3 * (int64_t)blockIdx.x;
  double q = 0.0, l = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 1024) {
    const double zi = z[i];
    q = fma(zi, zi, q);
    l += log(L[i * ld + i]);
  }
  q = wave_sum(q);
  l = wave_sum(l);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    sq[wave] = q;
    sl[wave] = l;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double qq = 0.0, ll = 0.0;
    for (int w = 0; w < 16; ++w) {
      qq += sq[w];
      ll += sl[w];
    }
    ll *= 2.0;
    out3[0] = qq;
    out3[1] = ll;
    out3[2] = -0.5 * (qq + ll + (double)N * 1.8378770664093454835606594728112);  // log(2 pi)
  }
}

// Leave-one-out quantities of an exact GP (Rasmussen & Williams, section 5.4.2; gpytorch LeaveOneOutPseudoLikelihood) from the
// inverse factor, without Ky^-1: row i of the Linv buffer from the diagonal on is column i of L^-1 (the mirror), so
//   d_i = (Ky^-1)_ii = sum_{j >= i} Linv[i][j]^2
// is one contiguous row reduction — one wave per row, 16-byte loads, a lane's terms added in index order and the lanes by the
// butterfly: a row's sum depends on N and i only, never on the grid.  Lane 0 then writes what the caller asked for:
//   mu_i = y_i - alpha_i / d_i,  s2_i = 1 / d_i,  a_i = -alpha_i / d_i,  sb_i = sqrt(b_i),  b_i = 1 / (2 d_i) + alpha_i^2 / (2 d_i^2)
// HBM-read-bound: 4 N^2 bytes.  (No reference counterpart: optim/mll_noise_continuation.py:54 names the criterion only.)
// Batch element blockIdx.y: its matrix at Linv + b*sLi, its vectors at + b*sv (a single problem is batch 1 with strides 0).
__global__ __launch_bounds__(256) void gpp_loo_rows(const double* __restrict__ Linv, int64_t ldi, int64_t N,
                                                    const double* __restrict__ alpha, const double* __restrict__ y,
                                                    double* __restrict__ d, double* __restrict__ mu, double* __restrict__ s2,
                                                    double* __restrict__ a, double* __restrict__ sb, int64_t sLi, int64_t sv) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= N) return;
  const int64_t vo = (int64_t)blockIdx.y * sv;  // this element's vectors
  const double* row = Linv + (int64_t)blockIdx.y * sLi + i * ldi;
  double acc = 0.0;
  int64_t k0 = i;
  if (k0 & 1) {  // align the vector loop to an even column
    if (lane == 0) acc = row[k0] * row[k0];
    ++k0;
  }
  const int64_t nvec = (N - k0) >> 1;
#pragma unroll 4
  for (int64_t v = lane; v < nvec; v += 64) {
    const v2d t = *reinterpret_cast<const v2d*>(row + k0 + 2 * v);
    acc = fma(t.x, t.x, acc);
    acc = fma(t.y, t.y, acc);
  }
  if (lane == 0 && ((N - k0) & 1)) acc = fma(row[N - 1], row[N - 1], acc);
  acc = wave_sum(acc);
  if (lane == 0) {
    const int64_t o = vo + i;
    const double di = acc, al = alpha[o], inv = 1.0 / di;
    d[o] = di;
    if (mu) mu[o] = y[o] - al * inv;
    if (s2) s2[o] = inv;
    if (a) a[o] = -al * inv;
    if (sb) sb[o] = sqrt(0.5 * inv + 0.5 * (al * inv) * (al * inv));
  }
}

// loo = sum_i [ 0.5 log d_i - alpha_i^2 / (2 d_i) ] - (N / 2) log 2pi : one work-group per batch element (blockIdx.x), the
// summation order of gpp_mll_scalars
__global__ __launch_bounds__(1024) void gpp_loo_value(const double* __restrict__ d, const double* __restrict__ alpha, int64_t N,
                                                      double* __restrict__ out, int64_t sv) {
  __shared__ double sp[16];
  d += (int64_t)blockIdx.x * sv;  // batch element
  alpha += (int64_t)blockIdx.x * sv;
  out += blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 1024) {
    const double di = d[i], al = alpha[i];
    s += 0.5 * log(di) - 0.5 * al * al / di;
  }
  s = wave_sum(s);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sp[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += sp[w];
    out[0] = t - 0.5 * (double)N * 1.8378770664093454835606594728112;  // log(2 pi)
  }
}

// ------------------------------------------------------------------------------------------------
// gradient reduction.  Tiles of 64x64 over the lower triangle of Kinv; 256 threads, 4x4 per thread.
// Per tile the kernel forms G_ij = mult * W_ij * sf2*k_ij  (W = 0.5(alpha_i alpha_j - Kinv_ij), mult = 2 for the
// strictly-lower entries, which stand for (i,j) and (j,i), 1 on the diagonal) and accumulates
//    g_w[d]  += G_ij * (-(u_id-u_jd)^2)          g_sf2 += mult * W_ij * k_ij          wdiag[i] = W_ii
//    g_U[i,d] += G_ij (-2 w_d)(u_id-u_jd)   and   g_U[j,d] += G_ij (-2 w_d)(u_jd-u_id)      (d < dU)
// Work-groups grid-stride over tiles; scalar sums go to one record per work-group, g_U row/column sums to the
// slot [partner tile][row] of a partial buffer (every slot is written exactly once).  Finish kernels sum both.
constexpr int GT = 64;
constexpr int GD_MAX = 64;
constexpr int GS_MAX = 64;
constexpr int G_WGS = 2048;

__device__ __forceinline__ void tile_from_index(int64_t t, int64_t& ti, int64_t& tj) {
  int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  while (r * (r + 1) / 2 > t) --r;
  ti = r;
  tj = t - r * (r + 1) / 2;
}

// kv = exp(-r2_rbf) h(r2_mat) and kd = its derivative by -r2_mat, from er = exp(-r2_rbf), for the three gradient reductions; kind 0 and
// the RBF instantiations: kv = er, kd = 0.  Their products take er first and e^-r last, (er 3) e^-r and ((er (5/3)) (1 + r)) e^-r:
// gpp_matern's dp, the rounded product -(5/3)(1 + r), cannot give the second, so -dp is written out here in that order (with dp the
// nu = 5/2 sums change in the last bit, gpp_grad_reduce with feature gradients runs 2 % slower and gpp_pgrad_tiles<8, true> takes 224
// registers instead of 220).  One call per kind, as the branches were: the code of every instantiation stays as it was.
template <bool MAT>
__device__ __forceinline__ void kernel_and_dmat(int kind, double er, double r2_mat, const GppExpConsts& ec, double& kv, double& kd) {
  kv = er;
  kd = 0.0;
  if (MAT && kind == 1) {
    const GppMatern m = gpp_matern(1, r2_mat, ec);
    kv = er * m.p * m.er;
    kd = er * 3.0 * m.er;
  } else if (MAT && kind == 2) {
    const GppMatern m = gpp_matern(2, r2_mat, ec);
    kv = er * m.p * m.er;
    kd = er * (5.0 / 3.0) * (1.0 + m.r) * m.er;
  }
}

// MAT = false: pure RBF product (kind 0): no Matern distance / derivative registers, two waves per SIMD
// HASU = false: no gradient w.r.t. feature columns (dU = 0): the 4 x 4 blocks of G are never materialised
// LOO = true: the leave-one-out pseudo-likelihood's weights W_ij = -0.5 (alpha_i beta_j + beta_i alpha_j) - C_ij (gpp_loo_grad_reduce:
//       `Kinv` is C = P diag(b) P, `beta` = P a) in place of 0.5 (alpha_i alpha_j - Kinv_ij); everything else is shared
template <int DT, bool MAT, bool HASU, bool LOO = false>
__global__ __launch_bounds__(256) void gpp_grad_tiles(const double* __restrict__ U, int64_t N, int D,
                                                      const double* __restrict__ w, const double* __restrict__ sf2p,
                                                      int kind, int d_split, const double* __restrict__ alpha, const double* __restrict__ Kinv,
                                                      int64_t ldk, int dU, int64_t ntiles, int shard_nb, int shard_rank,
                                                      int shard_nranks, int shard_cols, int64_t sU, int64_t sK, int64_t sv, int64_t ws_stride,
                                                      double* __restrict__ rec /* [gridDim.x][D+1] */,
                                                      double* __restrict__ wdiag /* [N] */,
                                                      double* __restrict__ gUpart /* [T][N][dU] */,
                                                      const double* __restrict__ beta /* [N], LOO only */) {
  {  // batch element blockIdx.y: its own parameters, matrices and slice of the workspace
    const int64_t b = blockIdx.y;
    if constexpr (LOO) beta += b * sv;
    U += b * sU;
    w += b * D;
    sf2p += b;
    alpha += b * sv;
    Kinv += b * sK;
    rec += b * ws_stride;
    wdiag += b * ws_stride;
    gUpart += b * ws_stride;
  }
  __shared__ __attribute__((aligned(16))) double sa[DT * GT];  // raw U rows of tile-row ti, [d][r]
  __shared__ __attribute__((aligned(16))) double sb[DT * GT];
  __shared__ double sal_a[GT], sal_b[GT];
  __shared__ double sbe_a[LOO ? GT : 1], sbe_b[LOO ? GT : 1];
  __shared__ double sw[DT];
  __shared__ double red[256];
  __shared__ double rowpart[GT * 16];
  const int tid = threadIdx.x;
  const int ty = tid >> 4, tx = tid & 15;
  const double sf2 = *sf2p;
  const GppExpConsts ec = gpp_exp_consts();
  if (tid < DT) sw[tid] = (tid < D) ? w[tid] : 0.0;

  // per-feature sums of this thread over all its tiles — in registers up to 16 features; beyond that (2 x DT registers, on top of
  // the 4 x 4 blocks of the feature gradients: <32,true,true> spilled 122 registers, <64,true,true> 645) every half-tile's
  // per-feature sum is reduced over the wave at once and kept in LDS, one accumulator per wave and feature
  constexpr bool WACC = (DT >= 32);
  __shared__ double wacc[WACC ? 4 * DT : 1];
  double my_sf2 = 0.0;
  double my_w[WACC ? 1 : DT];
#pragma unroll
  for (int d = 0; d < (WACC ? 1 : DT); ++d) my_w[d] = 0.0;
  if constexpr (WACC) {
    for (int e = tid; e < 4 * DT; e += 256) wacc[e] = 0.0;
  }

  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int64_t ti, tj;
    tile_from_index(t, ti, tj);
    const int64_t i0 = ti * GT, j0 = tj * GT;
    // row-sharded evaluation: this rank only holds (and reduces) the block rows of Kinv it owns (block-cyclic)
    // (shard_cols: the rank holds column blocks of Kinv instead — the back-substituted sharded evaluation)
    if (shard_nranks > 1 && (int)(((shard_cols ? j0 : i0) / shard_nb) % shard_nranks) != shard_rank) continue;
    const bool diag_tile = (ti == tj);
    __syncthreads();
    for (int e = tid; e < DT * GT; e += 256) {
      const int d = e / GT, r = e - d * GT;
      sa[e] = (d < D && i0 + r < N) ? U[(i0 + r) * D + d] : 0.0;
      sb[e] = (d < D && j0 + r < N) ? U[(j0 + r) * D + d] : 0.0;
    }
    if (tid < GT) {
      sal_a[tid] = (i0 + tid < N) ? alpha[i0 + tid] : 0.0;
      sal_b[tid] = (j0 + tid < N) ? alpha[j0 + tid] : 0.0;
      if constexpr (LOO) {
        sbe_a[tid] = (i0 + tid < N) ? beta[i0 + tid] : 0.0;
        sbe_b[tid] = (j0 + tid < N) ? beta[j0 + tid] : 0.0;
      }
    }
    __syncthreads();

    // G  = mult * W_ij * dK_ij/d(-r2_rbf)  (= mult W K for the RBF dims)
    // GM = mult * W_ij * dK_ij/d(-r2_mat)  for the Matern dims (d >= d_split), with K = sf2 e^{-r2_rbf} h(r2_mat) (gpp_matern)
    const int dsp = MAT ? d_split : DT;
    typedef double v2d __attribute__((ext_vector_type(2)));
    double G[4][4], GM[4][4];  // (GM only lives in the Matern instantiation; G / GM feed the g_U part below)
    // Two half-tiles of 2 rows x 4 columns per thread, each with its own two passes over the features: the live set stays
    // at 8 distances + 8 Kinv entries + 8 G values (two waves per SIMD), and every LDS access is a 16-byte read of
    // consecutive rows / columns of one feature.  Round 4: a thread's columns are the PAIRS {2 tx, 2 tx + 1} and {32 + 2 tx, ...}, so
    // the 16 lanes of a ds_read_b128 cover 256 contiguous bytes (every bank once); with 4 consecutive columns per thread lanes
    // k and k + 8 met in the same banks (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.36, profiles/r03_sq_counters.txt).
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      const int ra = 4 * ty + 2 * h;  // first of this half's two rows inside the tile
      double kin[2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        // the thread's columns: the pairs {2 tx, 2 tx + 1} and {32 + 2 tx, 32 + 2 tx + 1} of the tile (see the LDS reads below)
        const int64_t i = i0 + ra + a, jb = j0 + 2 * tx;
        // (shard_cols == 2: Kinv holds only the owned column blocks, side by side — see gpp_trmv_lower_cols)
        const int64_t pjb = (shard_cols == 2) ? ((j0 / shard_nb) / shard_nranks) * shard_nb + (j0 % shard_nb) + 2 * tx : jb;
        const double* src = Kinv + (i < N ? i : N - 1) * ldk + pjb;
        if (pjb + 34 <= ldk) {  // two 16-byte loads, issued before the arithmetic (entries above the diagonal are never used)
          const v2d p0 = *reinterpret_cast<const v2d*>(src), p1 = *reinterpret_cast<const v2d*>(src + 32);
          kin[a][0] = p0.x; kin[a][1] = p0.y; kin[a][2] = p1.x; kin[a][3] = p1.y;
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b) kin[a][b] = (gpp_tile_col(jb, b) < N) ? src[gpp_tile_col(0, b)] : 0.0;
        }
      }
      double r2[2][4], r2m[2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) r2[a][b] = r2m[a][b] = 0.0;
#pragma unroll 4
      for (int d = 0; d < DT; ++d) {
        const v2d ua = *reinterpret_cast<const v2d*>(sa + d * GT + ra);
        const v2d b01 = *reinterpret_cast<const v2d*>(sb + d * GT + 2 * tx), b23 = *reinterpret_cast<const v2d*>(sb + d * GT + 32 + 2 * tx);
        const double ub[4] = {b01.x, b01.y, b23.x, b23.y};
        const double wd = sw[d];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double df = (a ? ua.y : ua.x) - ub[b];
            if (!MAT || d < dsp) r2[a][b] = fma(wd * df, df, r2[a][b]);
            else r2m[a][b] = fma(wd * df, df, r2m[a][b]);
          }
      }
      // compiler barrier: without it the second pass below re-uses the first pass's LDS reads (same addresses), i.e. keeps
      // 12 registers per feature alive across the exp section (DT = 16: 398 VGPRs, DT >= 32: spills)
      __asm__ volatile("" ::: "memory");
      double g2[2][4], gm2[2][4];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int64_t i = i0 + ra + a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int cb = gpp_tile_col(2 * tx, b);
          const int64_t j = j0 + cb;
          double g = 0.0, gm = 0.0;
          if (i < N && j <= i) {
            double kv, kd;
            kernel_and_dmat<MAT>(kind, gpp_exp_nonpos(-r2[a][b], ec), r2m[a][b], ec, kv, kd);
            double Wij;
            if constexpr (LOO) Wij = -0.5 * (sal_a[ra + a] * sbe_b[cb] + sbe_a[ra + a] * sal_b[cb]) - kin[a][b];
            else Wij = 0.5 * (sal_a[ra + a] * sal_b[cb] - kin[a][b]);
            const double mult = (i == j) ? 1.0 : 2.0;
            my_sf2 = fma(mult * Wij, kv, my_sf2);
            g = mult * Wij * sf2 * kv;
            gm = mult * Wij * sf2 * kd;
            if (i == j) wdiag[i] = Wij;
          }
          g2[a][b] = g;
          gm2[a][b] = gm;
        }
      }
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        const v2d ua = *reinterpret_cast<const v2d*>(sa + d * GT + ra);
        const v2d b01 = *reinterpret_cast<const v2d*>(sb + d * GT + 2 * tx), b23 = *reinterpret_cast<const v2d*>(sb + d * GT + 32 + 2 * tx);
        const double ub[4] = {b01.x, b01.y, b23.x, b23.y};
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double df = (a ? ua.y : ua.x) - ub[b];
            s = fma(-((!MAT || d < dsp) ? g2[a][b] : gm2[a][b]) * df, df, s);
          }
        if constexpr (WACC) {
          const double t = wave_sum(s);
          if ((tid & 63) == 0) wacc[(tid >> 6) * DT + d] += t;
        } else {
          my_w[d] += s;
        }
      }
      if constexpr (HASU) {  // the manifold-gradient part below wants the whole 4 x 4 block
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if (h == 0) { G[a][b] = g2[a][b]; GM[a][b] = gm2[a][b]; }
            else { G[2 + a][b] = g2[a][b]; GM[2 + a][b] = gm2[a][b]; }
          }
      }
    }
    for (int d = 0; HASU && d < dU; ++d) {
      const double m2w = -2.0 * sw[d];
      const bool rbf_dim = !MAT || d < dsp;
      double rs[4], cs[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
          s = fma(rbf_dim ? G[a][b] : GM[a][b], sa[d * GT + 4 * ty + a] - sb[gpp_tile_col(d * GT + 2 * tx, b)], s);
        rs[a] = s;
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
          s = fma(rbf_dim ? G[a][b] : GM[a][b], sb[gpp_tile_col(d * GT + 2 * tx, b)] - sa[d * GT + 4 * ty + a], s);
        cs[b] = s;
      }
      __syncthreads();
#pragma unroll
      for (int a = 0; a < 4; ++a) rowpart[(4 * ty + a) * 16 + tx] = rs[a];
      __syncthreads();
      double rsum = 0.0;
      if (tid < GT)
        for (int q = 0; q < 16; ++q) rsum += rowpart[tid * 16 + q];
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 4; ++b) rowpart[gpp_tile_col(2 * tx, b) * 16 + ty] = cs[b];
      __syncthreads();
      if (tid < GT) {
        double csum = 0.0;
        for (int q = 0; q < 16; ++q) csum += rowpart[tid * 16 + q];
        if (diag_tile) {
          if (i0 + tid < N) gUpart[((int64_t)ti * N + (i0 + tid)) * dU + d] = m2w * (rsum + csum);
        } else {
          if (i0 + tid < N) gUpart[((int64_t)tj * N + (i0 + tid)) * dU + d] = m2w * rsum;
          if (j0 + tid < N) gUpart[((int64_t)ti * N + (j0 + tid)) * dU + d] = m2w * csum;
        }
      }
    }
  }

  const int nrec = D + 1;
  for (int q = 0; q < nrec; ++q) {
    double v = my_sf2;
    if (q < D) {
      if constexpr (WACC) {
        v = ((tid & 63) == 0) ? wacc[(tid >> 6) * DT + q] : 0.0;
      } else {
#pragma unroll
        for (int d = 0; d < DT; ++d)
          if (q == d) v = my_w[d];
      }
    }
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) rec[(int64_t)blockIdx.x * nrec + q] = red[0];
  }
}

// q < D: g_w[q]; q == D: g_sf2; q > D: g_tau[q-D-1] = sum_{i in group} wdiag[i]
__global__ __launch_bounds__(256) void gpp_grad_finish(const double* __restrict__ rec, int nwg, int D, int S,
                                                       const double* __restrict__ wdiag, const int32_t* __restrict__ grp,
                                                       int64_t N, double* __restrict__ g_w, double* __restrict__ g_sf2,
                                                       double* __restrict__ g_tau, int64_t ws_stride) {
  __shared__ double red[256];
  rec += (int64_t)blockIdx.y * ws_stride;  // batch element
  wdiag += (int64_t)blockIdx.y * ws_stride;
  g_w += (int64_t)blockIdx.y * D;
  g_sf2 += blockIdx.y;
  g_tau += (int64_t)blockIdx.y * S;
  const int q = blockIdx.x, nrec = D + 1, tid = threadIdx.x;
  double v = 0.0;
  if (q <= D) {
    for (int b = tid; b < nwg; b += 256) v += rec[(int64_t)b * nrec + q];
  } else {
    const int s = q - D - 1;
    for (int64_t i = tid; i < N; i += 256)
      if ((grp ? grp[i] : 0) == s) v += wdiag[i];
  }
  block_sum(tid, v, (lds_double*)red);
  if (tid == 0) {
    if (q < D) g_w[q] = red[0];
    else if (q == D) g_sf2[0] = red[0];
    else g_tau[q - D - 1] = red[0];
  }
}

__global__ __launch_bounds__(256) void gpp_gU_finish(const double* __restrict__ gUpart, int64_t N, int dU, int T,
                                                     double* __restrict__ g_U, int64_t ws_stride) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * dU) return;
  gUpart += (int64_t)blockIdx.y * ws_stride;  // batch element
  g_U += (int64_t)blockIdx.y * N * dU;
  double s = 0.0;
  for (int t = 0; t < T; ++t) s += gUpart[(int64_t)t * N * dU + e];
  g_U[e] = s;
}

// ------------------------------------------------------------------------------------------------
// gradient of predictions (gpp_cross_grad).  With G_aj = gmean_a alpha_j + gvar_a B_aj (never materialised) and
// K_aj = sf2 k(u_a, u_j) recomputed in registers from the staged features:
//    g_Ua[a,d] += G_aj dK_aj/du_ad = (-2 w_d) G_aj sf2 k'_aj (u_ad-u_jd)      (d < dA)
//    g_Ub[j,d] += G_aj dK_aj/du_jd = ( 2 w_d) G_aj sf2 k'_aj (u_ad-u_jd)      (d < dB)
//    g_w[d]    += G_aj dK_aj/dw_d  = -G_aj sf2 k'_aj (u_ad-u_jd)^2            g_sf2 += G_aj k_aj
// (k' = k for the RBF dims, the Matern factor's derivative for d >= d_split, as in gpp_grad_tiles).
// Work-group (c, t): row tile t (64 test rows, staged once) against the column tiles c, c + CN, c + 2 CN, ... of the
// training points, so both M and N are split over the grid (M = 1 against N = 20000: 313 work-groups; M = 8192: 128 x 16).
// Thread (ty, tx): rows 4 ty .. 4 ty + 3 and the column pairs {2 tx, 2 tx + 1}, {32 + 2 tx, 33 + 2 tx} of the tile (16-byte LDS
// reads covering every bank once, see gpp_grad_tiles).  Deterministic: the row sums of a tile are reduced over the 16 lanes that
// share a row and added, in column-tile order, to an LDS accumulator with one owner per entry, written once per work-group to
// slot [c][a]; column sums go to slot [t][j] (every slot written exactly once); scalar sums to one record per work-group.
// The finish kernels add the slots in a fixed order.  B (M x N) is the only M x N operand, read once.
constexpr int PG_WGS = 2048;

struct PgradShape {
  int64_t MT, NT;
  int CN;
};

static PgradShape pgrad_shape(int64_t M, int64_t N) {
  PgradShape s;
  s.MT = (M + GT - 1) / GT;
  s.NT = (N + GT - 1) / GT;
  const int64_t want = (PG_WGS + s.MT - 1) / (s.MT > 0 ? s.MT : 1);
  s.CN = (int)std::max<int64_t>(1, std::min<int64_t>(s.NT, want));
  return s;
}

template <int DT, bool MAT>
__global__ __launch_bounds__(256) void gpp_pgrad_tiles(const double* __restrict__ Ua, int64_t M, const double* __restrict__ Ub,
                                                       int64_t N, int D, const double* __restrict__ w,
                                                       const double* __restrict__ sf2p, int kind, int d_split,
                                                       const double* __restrict__ gmean, const double* __restrict__ alpha,
                                                       const double* __restrict__ gvar, const double* __restrict__ B, int64_t ldb,
                                                       int dA, int dB, int want_w, int CN,
                                                       double* __restrict__ rec /* [MT * CN][D+1] */,
                                                       double* __restrict__ gApart /* [CN][M][dA] */,
                                                       double* __restrict__ gBpart /* [MT][N][dB] */) {
  __shared__ __attribute__((aligned(16))) double sa[DT * GT];  // test rows of tile t, [d][r]
  __shared__ __attribute__((aligned(16))) double sb[DT * GT];  // training rows of the current column tile, [d][r]
  __shared__ double accA[DT * GT];                              // g_Ua of tile t over this work-group's column tiles, [d][r]
  __shared__ double s_gm[GT], s_gv[GT], s_al[GT];
  __shared__ double sw[DT];
  __shared__ double wacc[4 * DT];
  __shared__ double colred[4 * GT];
  __shared__ double red[256];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, wave = tid >> 6, lane = tid & 63;
  const int c = blockIdx.x;
  const int64_t t = blockIdx.y, i0 = t * GT;
  const double sf2 = *sf2p;
  const GppExpConsts ec = gpp_exp_consts();
  const int dsp = MAT ? d_split : DT;
  if (tid < DT) sw[tid] = (tid < D) ? w[tid] : 0.0;
  for (int e = tid; e < DT * GT; e += 256) {
    const int d = e / GT, r = e - d * GT;
    sa[e] = (d < D && i0 + r < M) ? Ua[(i0 + r) * D + d] : 0.0;
    accA[e] = 0.0;
  }
  for (int e = tid; e < 4 * DT; e += 256) wacc[e] = 0.0;
  if (tid < GT) {
    const bool ok = i0 + tid < M;
    s_gm[tid] = (ok && gmean) ? gmean[i0 + tid] : 0.0;
    s_gv[tid] = (ok && gvar) ? gvar[i0 + tid] : 0.0;
  }
  double my_sf2 = 0.0;
  const int64_t NT = (N + GT - 1) / GT;
  typedef double v2d __attribute__((ext_vector_type(2)));
  for (int64_t ct = c; ct < NT; ct += CN) {
    const int64_t j0 = ct * GT;
    __syncthreads();
    for (int e = tid; e < DT * GT; e += 256) {
      const int d = e / GT, r = e - d * GT;
      sb[e] = (d < D && j0 + r < N) ? Ub[(j0 + r) * D + d] : 0.0;
    }
    if (tid < GT) s_al[tid] = (alpha && j0 + tid < N) ? alpha[j0 + tid] : 0.0;
    __syncthreads();

    // this thread's 4 x 4 entries of B, two 16-byte loads per row issued before the arithmetic
    double bv[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[a][b] = 0.0;
    if (B) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int64_t i = i0 + 4 * ty + a, jb = j0 + 2 * tx;
        const double* src = B + (i < M ? i : M - 1) * ldb + jb;
        if (jb + 34 <= ldb) {
          const v2d p0 = *reinterpret_cast<const v2d*>(src), p1 = *reinterpret_cast<const v2d*>(src + 32);
          bv[a][0] = p0.x; bv[a][1] = p0.y; bv[a][2] = p1.x; bv[a][3] = p1.y;
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b) bv[a][b] = (gpp_tile_col(jb, b) < N) ? src[gpp_tile_col(0, b)] : 0.0;
        }
      }
    }

    double r2[4][4], r2m[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) r2[a][b] = r2m[a][b] = 0.0;
#pragma unroll 4
    for (int d = 0; d < DT; ++d) {
      const v2d u01 = *reinterpret_cast<const v2d*>(sa + d * GT + 4 * ty), u23 = *reinterpret_cast<const v2d*>(sa + d * GT + 4 * ty + 2);
      const v2d b01 = *reinterpret_cast<const v2d*>(sb + d * GT + 2 * tx), b23 = *reinterpret_cast<const v2d*>(sb + d * GT + 32 + 2 * tx);
      const double ua[4] = {u01.x, u01.y, u23.x, u23.y}, ub[4] = {b01.x, b01.y, b23.x, b23.y};
      const double wd = sw[d];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = ua[a] - ub[b];
          if (!MAT || d < dsp) r2[a][b] = fma(wd * df, df, r2[a][b]);
          else r2m[a][b] = fma(wd * df, df, r2m[a][b]);
        }
    }
    // compiler barrier: the feature pass below reads the same LDS addresses again instead of keeping them live (gpp_grad_tiles)
    __asm__ volatile("" ::: "memory");
    // g = G sf2 k (the RBF dims' factor of dK/d(-r2)), gm = G sf2 dm/d(-r2_mat) for the Matern dims (as in gpp_grad_tiles)
    double g[4][4], gm[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t i = i0 + 4 * ty + a;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int cb = gpp_tile_col(2 * tx, b);
        double gg = 0.0, gmm = 0.0;
        if (i < M && j0 + cb < N) {
          double kv, kd;
          kernel_and_dmat<MAT>(kind, gpp_exp_nonpos(-r2[a][b], ec), r2m[a][b], ec, kv, kd);
          const double G = fma(s_gm[4 * ty + a], s_al[cb], s_gv[4 * ty + a] * bv[a][b]);
          my_sf2 = fma(G, kv, my_sf2);
          gg = G * sf2 * kv;
          gmm = G * sf2 * kd;
        }
        g[a][b] = gg;
        gm[a][b] = gmm;
      }
    }
    // feature pass: per feature, the g_w sum (wave-reduced into one LDS accumulator per wave), the row sums (reduced over the
    // 16 lanes of a row) and the column sums (reduced over the wave, then over the four waves through LDS)
#pragma unroll 2
    for (int d = 0; d < D; ++d) {
      const v2d u01 = *reinterpret_cast<const v2d*>(sa + d * GT + 4 * ty), u23 = *reinterpret_cast<const v2d*>(sa + d * GT + 4 * ty + 2);
      const v2d b01 = *reinterpret_cast<const v2d*>(sb + d * GT + 2 * tx), b23 = *reinterpret_cast<const v2d*>(sb + d * GT + 32 + 2 * tx);
      const double ua[4] = {u01.x, u01.y, u23.x, u23.y}, ub[4] = {b01.x, b01.y, b23.x, b23.y};
      const double wd = sw[d];
      const bool rbf_dim = !MAT || d < dsp;
      double rs[4] = {0.0, 0.0, 0.0, 0.0}, cs[4] = {0.0, 0.0, 0.0, 0.0}, sw2 = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = ua[a] - ub[b];
          const double gs = rbf_dim ? g[a][b] : gm[a][b];
          const double gd = gs * df;
          rs[a] += gd;
          cs[b] += gd;
          sw2 = fma(-gd, df, sw2);
        }
      if (want_w) {
        const double s = wave_sum(sw2);
        if (lane == 0) wacc[wave * DT + d] += s;
      }
      if (d < dA) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          double v = rs[a];
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
          if (tx == 0) accA[d * GT + 4 * ty + a] += -2.0 * wd * v;
        }
      }
      if (d < dB) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          double v = cs[b];
          v += __shfl_xor(v, 16);
          v += __shfl_xor(v, 32);
          if (lane < 16) colred[gpp_tile_col(wave * GT + 2 * tx, b)] = v;
        }
        __syncthreads();
        if (tid < GT && j0 + tid < N)
          gBpart[((int64_t)t * N + j0 + tid) * dB + d] =
              2.0 * wd * ((colred[tid] + colred[GT + tid]) + (colred[2 * GT + tid] + colred[3 * GT + tid]));
        __syncthreads();
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < dA * GT; e += 256) {
    const int d = e / GT, r = e - d * GT;
    if (i0 + r < M) gApart[((int64_t)c * M + i0 + r) * dA + d] = accA[e];
  }
  const int nrec = D + 1;
  const int64_t wg = t * CN + c;
  for (int q = 0; q < nrec; ++q) {
    double v = my_sf2;
    if (q < D) v = (lane == 0) ? wacc[wave * DT + q] : 0.0;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) rec[wg * nrec + q] = red[0];
  }
}

// q < D: g_w[q]; q == D: g_sf2 — each only when asked for
__global__ __launch_bounds__(256) void gpp_pgrad_finish(const double* __restrict__ rec, int nwg, int D, double* __restrict__ g_w,
                                                        double* __restrict__ g_sf2) {
  __shared__ double red[256];
  const int q = blockIdx.x, nrec = D + 1, tid = threadIdx.x;
  double v = 0.0;
  for (int b = tid; b < nwg; b += 256) v += rec[(int64_t)b * nrec + q];
  block_sum(tid, v, (lds_double*)red);
  if (tid == 0) {
    if (q < D && g_w) g_w[q] = red[0];
    else if (q == D && g_sf2) g_sf2[0] = red[0];
  }
}

// mean_a = sum_j Ksn[a][j] alpha_j ; var_a = kss_a - sum_j V[a][j]^2 : one wave per test row.
__global__ __launch_bounds__(256) void gpp_predict_rows(const double* __restrict__ Ksn, int64_t lds, const double* __restrict__ V,
                                                        int64_t ldv, int64_t M, int64_t N, const double* __restrict__ alpha,
                                                        const double* __restrict__ kss, double* __restrict__ mean_out,
                                                        double* __restrict__ var_out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t a = (int64_t)blockIdx.x * 4 + wave;
  if (a >= M) return;
  double m = 0.0, q = 0.0;
  const double* kr = Ksn + a * lds;
  for (int64_t j = lane; j < N; j += 64) m = fma(kr[j], alpha[j], m);
  if (V) {
    const double* vr = V + a * ldv;
    for (int64_t j = lane; j < N; j += 64) q = fma(vr[j], vr[j], q);
  }
  m = wave_sum(m);
  q = wave_sum(q);
  if (lane == 0) {
    mean_out[a] = m;
    if (V && var_out) var_out[a] = kss[a] - q;
  }
}

}  // namespace

hipError_t gpp_launch_trmv_lower(hipStream_t s, const double* T, int64_t ldt, int64_t N, const double* x, double* y,
                                 int batch, int64_t sT, int64_t sv) {
  if (N <= 0 || batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(gpp_trmv_lower, dim3((unsigned)((N + 3) / 4), (unsigned)batch), dim3(256), 0, s, T, ldt, N, x, y, sT, sv);
  return hipGetLastError();
}

hipError_t gpp_launch_trmv_upper(hipStream_t s, const double* T, int64_t ldt, int64_t N, const double* x, double* y,
                                 int batch, int64_t sT, int64_t sv) {
  if (N <= 0 || batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(gpp_trmv_upper, dim3((unsigned)((N + 3) / 4), (unsigned)batch), dim3(256), 0, s, T, ldt, N, x, y, sT, sv);
  return hipGetLastError();
}

size_t gpp_trmv_t_ws_bytes(int64_t N) { return (size_t)TRT_CHUNKS * (size_t)N * sizeof(double); }

hipError_t gpp_launch_trmv_lower_cols(hipStream_t s, const double* T, int64_t ldt, int64_t N, const double* x, double* y,
                                      int64_t nb, int rank, int nranks, int trans, void* ws, size_t ws_bytes, int compact) {
  if (N <= 0) return hipSuccess;
  if (nb < 64 || nb % 64 != 0 || nranks < 1 || rank < 0 || rank >= nranks) return hipErrorInvalidValue;
  if (trans) {
    if (!ws || ws_bytes < gpp_trmv_t_ws_bytes(N)) return hipErrorInvalidValue;
    const int64_t chunk = (((N + TRT_CHUNKS - 1) / TRT_CHUNKS) + 31) / 32 * 32;
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(gpp_trmv_lower_t_cols, dim3((unsigned)((N + 63) / 64), TRT_CHUNKS), dim3(256), 0, s, T, ldt, N, x, part, nb,
                       rank, nranks, chunk, compact);
    hipLaunchKernelGGL(gpp_trmv_lower_t_finish, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, part, N, TRT_CHUNKS, y);
  } else
    hipLaunchKernelGGL(gpp_trmv_lower_cols, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, T, ldt, N, x, y, nb, rank, nranks, compact);
  return hipGetLastError();
}

hipError_t gpp_launch_mll_scalars(hipStream_t s, const double* L, int64_t ld, int64_t N, const double* z, double* out3,
                                  int batch, int64_t sL, int64_t sv) {
  if (batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(gpp_mll_scalars, dim3((unsigned)batch), dim3(1024), 0, s, L, ld, N, z, out3, sL, sv);
  return hipGetLastError();
}

hipError_t gpp_launch_loo_scalars_batched(hipStream_t s, const double* Linv, int64_t ldi, int64_t N, const double* alpha,
                                          const double* y, double* d, double* mu, double* s2, double* a, double* sb, double* loo,
                                          int batch, int64_t sLi, int64_t sv) {
  if (batch <= 0) return hipSuccess;
  if (batch > 65535) return hipErrorInvalidValue;  // gridDim.y
  if (N > 0)
    hipLaunchKernelGGL(gpp_loo_rows, dim3((unsigned)((N + 3) / 4), (unsigned)batch), dim3(256), 0, s, Linv, ldi, N, alpha, y, d, mu,
                       s2, a, sb, sLi, sv);
  if (loo) hipLaunchKernelGGL(gpp_loo_value, dim3((unsigned)batch), dim3(1024), 0, s, d, alpha, N, loo, sv);
  return hipGetLastError();
}

hipError_t gpp_launch_loo_scalars(hipStream_t s, const double* Linv, int64_t ldi, int64_t N, const double* alpha, const double* y,
                                  double* d, double* mu, double* s2, double* a, double* sb, double* loo) {
  return gpp_launch_loo_scalars_batched(s, Linv, ldi, N, alpha, y, d, mu, s2, a, sb, loo, 1, 0, 0);
}

size_t gpp_grad_ws_bytes(int64_t N, int D, int S, int dU) {
  (void)S;
  const int64_t T = (N + GT - 1) / GT;
  return (size_t)G_WGS * (D + 1) * sizeof(double) + (size_t)N * sizeof(double) +
         (size_t)T * N * (dU > 0 ? dU : 0) * sizeof(double) + 256;
}

hipError_t gpp_launch_grad_reduce(hipStream_t s, const double* U, int64_t N, int D, const double* w, const double* sf2,
                                  const int32_t* grp, int S, int kind, int d_split, const double* alpha,
                                  const double* Kinv, int64_t ldk, int dU, double* g_w, double* g_sf2, double* g_tau,
                                  double* g_U, void* ws, size_t ws_bytes, int shard_nb, int shard_rank, int shard_nranks,
                                  int batch, int64_t sU, int64_t sK, int64_t sv, int shard_cols, const double* beta) {
  if (kind < 0 || kind > 2) return hipErrorInvalidValue;
  if (batch < 1 || batch > 65535) return hipErrorInvalidValue;
  if (shard_nranks > 1 && (shard_nb < GT || shard_nb % GT != 0 || shard_rank < 0 || shard_rank >= shard_nranks))
    return hipErrorInvalidValue;
  if (D > GD_MAX || D < 1 || S > GS_MAX || S < 1 || dU > D || dU < 0) return hipErrorInvalidValue;
  if (ws_bytes < (size_t)batch * gpp_grad_ws_bytes(N, D, S, dU)) return hipErrorInvalidValue;
  const int64_t ws_stride = (int64_t)(gpp_grad_ws_bytes(N, D, S, dU) / sizeof(double));  // doubles per batch element
  const int T = (int)((N + GT - 1) / GT);
  const int64_t ntiles = (int64_t)T * (T + 1) / 2;
  const int nwg = (int)(ntiles < G_WGS ? ntiles : G_WGS);
  double* rec = reinterpret_cast<double*>(ws);
  double* wdiag = rec + (size_t)G_WGS * (D + 1);
  double* gUpart = wdiag + N;
  if (shard_nranks > 1) {  // skipped tiles leave their slots unwritten: start from zero
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)batch * ws_stride * sizeof(double), s);
    if (e != hipSuccess) return e;
  }
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(nwg, batch), dim3(256), 0, s, U, N, D, w, sf2, kind, d_split, alpha, Kinv, ldk, dU, ntiles,
                       shard_nb, shard_rank, shard_nranks, shard_cols, sU, sK, sv, ws_stride, rec, wdiag, gUpart, beta);
  };
  const bool mat = kind != 0, hasu = dU > 0, loo = beta != nullptr;  // beta: the leave-one-out weights (gpp_loo_grad_reduce)
#define GPP_GT2(DT, LOO)                                                                                             \
  (mat ? (hasu ? launch(gpp_grad_tiles<DT, true, true, LOO>) : launch(gpp_grad_tiles<DT, true, false, LOO>))         \
       : (hasu ? launch(gpp_grad_tiles<DT, false, true, LOO>) : launch(gpp_grad_tiles<DT, false, false, LOO>)))
#define GPP_GT(DT) (loo ? GPP_GT2(DT, true) : GPP_GT2(DT, false))
  if (D <= 8) GPP_GT(8);
  else if (D <= 16) GPP_GT(16);
  else if (D <= 32) GPP_GT(32);
  else GPP_GT(64);
#undef GPP_GT
#undef GPP_GT2
  hipLaunchKernelGGL(gpp_grad_finish, dim3(D + 1 + S, batch), dim3(256), 0, s, rec, nwg, D, S, wdiag, grp, N, g_w, g_sf2, g_tau,
                     ws_stride);
  if (dU > 0)
    hipLaunchKernelGGL(gpp_gU_finish, dim3((unsigned)((N * dU + 255) / 256), batch), dim3(256), 0, s, gUpart, N, dU, T, g_U,
                       ws_stride);
  return hipGetLastError();
}

// gpp_lauum_grad (gpp_gemm.hip): one record per 128 x 128 tile of the lower triangle, then wdiag
size_t gpp_lauum_grad_ws_bytes(int64_t N, int D) {
  const int64_t T = (N + 127) / 128;
  return (size_t)(T * (T + 1) / 2) * (D + 1) * sizeof(double) + (size_t)N * sizeof(double) + 256;
}
hipError_t gpp_launch_grad_finish(hipStream_t s, const double* rec, int64_t nrec, int D, int S, const double* wdiag,
                                  const int32_t* grp, int64_t N, double* g_w, double* g_sf2, double* g_tau) {
  if (nrec < 0 || nrec > INT32_MAX || D < 1 || D > GD_MAX || S < 1 || S > GS_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gpp_grad_finish, dim3(D + 1 + S, 1), dim3(256), 0, s, rec, (int)nrec, D, S, wdiag, grp, N, g_w, g_sf2, g_tau,
                     (int64_t)0);
  return hipGetLastError();
}

size_t gpp_pgrad_ws_bytes(int64_t M, int64_t N, int D, int dA, int dB) {
  const PgradShape p = pgrad_shape(M, N);
  const int64_t nwg = p.MT * p.CN;
  return ((size_t)nwg * (D + 1) + (size_t)p.CN * M * std::max(dA, 0) + (size_t)p.MT * N * std::max(dB, 0)) * sizeof(double);
}

hipError_t gpp_launch_cross_grad(hipStream_t s, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                                 const double* sf2, int kind, int d_split, const double* gmean, const double* alpha,
                                 const double* gvar, const double* B, int64_t ldb, double* g_Ua, int dA, double* g_Ub, int dB,
                                 double* g_w, double* g_sf2, void* ws, size_t ws_bytes) {
  if (kind < 0 || kind > 2 || D < 1 || D > GD_MAX) return hipErrorInvalidValue;
  if (M <= 0 || N <= 0) {  // empty sums
    if (g_w) if (hipError_t e = hipMemsetAsync(g_w, 0, (size_t)D * sizeof(double), s); e != hipSuccess) return e;
    if (g_sf2) if (hipError_t e = hipMemsetAsync(g_sf2, 0, sizeof(double), s); e != hipSuccess) return e;
    if (dA > 0 && M > 0) if (hipError_t e = hipMemsetAsync(g_Ua, 0, (size_t)M * dA * sizeof(double), s); e != hipSuccess) return e;
    if (dB > 0 && N > 0) if (hipError_t e = hipMemsetAsync(g_Ub, 0, (size_t)N * dB * sizeof(double), s); e != hipSuccess) return e;
    return hipSuccess;
  }
  const PgradShape p = pgrad_shape(M, N);
  if (p.MT > 65535) return hipErrorInvalidValue;
  if (ws_bytes < gpp_pgrad_ws_bytes(M, N, D, dA, dB)) return hipErrorInvalidValue;
  const int nwg = (int)(p.MT * p.CN);
  double* rec = reinterpret_cast<double*>(ws);
  double* gApart = rec + (size_t)nwg * (D + 1);
  double* gBpart = gApart + (size_t)p.CN * M * std::max(dA, 0);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)p.CN, (unsigned)p.MT), dim3(256), 0, s, Ua, M, Ub, N, D, w, sf2, kind, d_split, gmean,
                       alpha, gvar, B, ldb, dA, dB, g_w ? 1 : 0, p.CN, rec, gApart, gBpart);
  };
  const bool mat = kind != 0;
#define GPP_PG(DT) (mat ? launch(gpp_pgrad_tiles<DT, true>) : launch(gpp_pgrad_tiles<DT, false>))
  if (D <= 8) GPP_PG(8);
  else if (D <= 16) GPP_PG(16);
  else if (D <= 32) GPP_PG(32);
  else GPP_PG(64);
#undef GPP_PG
  if (g_w || g_sf2) hipLaunchKernelGGL(gpp_pgrad_finish, dim3(D + 1), dim3(256), 0, s, rec, nwg, D, g_w, g_sf2);
  if (dA > 0)
    hipLaunchKernelGGL(gpp_gU_finish, dim3((unsigned)((M * dA + 255) / 256), 1), dim3(256), 0, s, gApart, M, dA, p.CN, g_Ua,
                       (int64_t)0);
  if (dB > 0)
    hipLaunchKernelGGL(gpp_gU_finish, dim3((unsigned)((N * dB + 255) / 256), 1), dim3(256), 0, s, gBpart, N, dB, (int)p.MT, g_Ub,
                       (int64_t)0);
  return hipGetLastError();
}

hipError_t gpp_launch_predict_reduce(hipStream_t s, const double* Ksn, int64_t lds, const double* V, int64_t ldv,
                                     int64_t M, int64_t N, const double* alpha, const double* kss, double* mean_out,
                                     double* var_out) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(gpp_predict_rows, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, Ksn, lds, V, ldv, M, N, alpha, kss,
                     mean_out, var_out);
  return hipGetLastError();
}

// ---- out-of-place transpose (the mirror L^-T of the sharded evaluation's column blocks) --------------------------------
namespace {
__global__ __launch_bounds__(256) void gpp_transpose_tile(const double* __restrict__ src, int64_t lds, int64_t rows, int64_t cols,
                                                          double* __restrict__ dst, int64_t ldd) {
  __shared__ double tile[64][65];  // padded: the transposed read walks a column
  const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 64 x 4 threads, 16 passes
#pragma unroll 4
  for (int i = ty; i < 64; i += 4) {
    const int64_t r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < rows && c < cols) ? src[r * lds + c] : 0.0;
  }
  __syncthreads();
#pragma unroll 4
  for (int i = ty; i < 64; i += 4) {
    const int64_t c = c0 + i, r = r0 + tx;  // dst row = source column
    if (c < cols && r < rows) dst[c * ldd + r] = tile[tx][i];
  }
}
}  // namespace

hipError_t gpp_launch_transpose(hipStream_t s, const double* src, int64_t lds, int64_t rows, int64_t cols, double* dst, int64_t ldd) {
  if (rows <= 0 || cols <= 0) return hipSuccess;
  dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64));
  hipLaunchKernelGGL(gpp_transpose_tile, grid, dim3(256), 0, s, src, lds, rows, cols, dst, ldd);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// gradient by calibration parameters (gpp_calib_grad_reduce).  theta_k is written into feature column cols[k] of every row of the
// calibrated source (member[i] != 0), so with m_i the membership and W = 0.5 (alpha alpha' - Kinv)
//    g_theta[k] = sum_ij W_ij (m_i - m_j) dK_ij/du_{i,c}   =   2 sum_{i > j} (m_i - m_j) W_ij sf2 k'_ij (-2 w_c) (u_ic - u_jc),   c = cols[k]
// (k' = k on an RBF dimension, the Matern factor's derivative for c >= d_split, as in gpp_grad_tiles): the sum of gpp_grad_reduce's
// g_U[i, c] over the member rows, without the N x dU block and its T x N x dU partials.  Pairs of one source contribute an exact
// zero and are never evaluated: a 64 x 64 tile of Kinv's lower triangle whose rows and columns all share one membership is skipped
// before any of it is read, so rows sorted by source cost the cross-source rectangle only.
// Work-groups grid-stride over the tiles (the tile -> work-group map and so every sum's order depend on N alone); a thread holds
// 4 rows x the column pairs {2 tx, 2 tx + 1}, {32 + 2 tx, 33 + 2 tx} (the LDS and Kinv access shapes of gpp_grad_tiles); per tile and
// parameter the wave's sum goes to one LDS accumulator per wave, the work-group writes one record of C sums, and the finish kernel
// adds the records in index order.  No atomics.
namespace {

template <int DT, bool MAT>
__global__ __launch_bounds__(256) void gpp_calib_tiles(const double* __restrict__ U, int64_t N, int D, const double* __restrict__ w,
                                                       const double* __restrict__ sf2p, int kind, int d_split,
                                                       const double* __restrict__ alpha, const double* __restrict__ Kinv, int64_t ldk,
                                                       const int32_t* __restrict__ member, const int32_t* __restrict__ cols, int C,
                                                       int64_t ntiles, double* __restrict__ rec /* [gridDim.x][C] */) {
  __shared__ __attribute__((aligned(16))) double sa[DT * GT];  // raw U rows of tile-row ti, [d][r]
  __shared__ __attribute__((aligned(16))) double sb[DT * GT];
  __shared__ double sal_a[GT], sal_b[GT];
  __shared__ int sm_a[GT], sm_b[GT];
  __shared__ double sw[DT];
  __shared__ int scol[GD_MAX];
  __shared__ double wacc[4 * GD_MAX];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, wave = tid >> 6, lane = tid & 63;
  const double sf2 = *sf2p;
  const GppExpConsts ec = gpp_exp_consts();
  const int dsp = MAT ? d_split : DT;
  if (tid < DT) sw[tid] = (tid < D) ? w[tid] : 0.0;
  if (tid < GD_MAX) {
    const int c = (tid < C) ? cols[tid] : -1;
    scol[tid] = (c >= 0 && c < D) ? c : -1;  // (the wrappers refuse a column outside [0, D); here it would add nothing)
  }
  for (int e = tid; e < 4 * GD_MAX; e += 256) wacc[e] = 0.0;
  __syncthreads();

  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int64_t ti, tj;
    tile_from_index(t, ti, tj);
    const int64_t i0 = ti * GT, j0 = tj * GT;
    // the tile's memberships: threads 0..63 look at its rows, 64..127 at its columns
    int mine = 0, p1 = 0, p0 = 0;
    if (tid < 2 * GT) {
      const int64_t r = (tid < GT) ? i0 + tid : j0 + (tid - GT);
      if (r < N) {
        mine = member[r] != 0;
        p1 = mine;
        p0 = !mine;
      }
    }
    // (both are barriers: every thread is done with the previous tile's LDS before anything below is overwritten)
    const int any1 = __syncthreads_or(p1), any0 = __syncthreads_or(p0);
    if (!(any1 && any0)) continue;  // one membership throughout: every pair contributes an exact zero
    for (int e = tid; e < DT * GT; e += 256) {
      const int d = e / GT, r = e - d * GT;
      sa[e] = (d < D && i0 + r < N) ? U[(i0 + r) * D + d] : 0.0;
      sb[e] = (d < D && j0 + r < N) ? U[(j0 + r) * D + d] : 0.0;
    }
    if (tid < GT) {
      sal_a[tid] = (i0 + tid < N) ? alpha[i0 + tid] : 0.0;
      sm_a[tid] = mine;
    } else if (tid < 2 * GT) {
      sal_b[tid - GT] = (j0 + tid - GT < N) ? alpha[j0 + tid - GT] : 0.0;
      sm_b[tid - GT] = mine;
    }
    __syncthreads();

    // this thread's 4 x 4 entries of Kinv: two 16-byte loads per row, issued before the arithmetic (lower triangle only is used)
    double kin[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t i = i0 + 4 * ty + a, jb = j0 + 2 * tx;
      const double* src = Kinv + (i < N ? i : N - 1) * ldk + jb;
      if (jb + 34 <= ldk) {
        const v2d q0 = *reinterpret_cast<const v2d*>(src), q1 = *reinterpret_cast<const v2d*>(src + 32);
        kin[a][0] = q0.x; kin[a][1] = q0.y; kin[a][2] = q1.x; kin[a][3] = q1.y;
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) kin[a][b] = (gpp_tile_col(jb, b) < N) ? src[gpp_tile_col(0, b)] : 0.0;
      }
    }
    double r2[4][4], r2m[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) r2[a][b] = r2m[a][b] = 0.0;
#pragma unroll 4
    for (int d = 0; d < DT; ++d) {
      const v2d u01 = *reinterpret_cast<const v2d*>(sa + d * GT + 4 * ty), u23 = *reinterpret_cast<const v2d*>(sa + d * GT + 4 * ty + 2);
      const v2d b01 = *reinterpret_cast<const v2d*>(sb + d * GT + 2 * tx), b23 = *reinterpret_cast<const v2d*>(sb + d * GT + 32 + 2 * tx);
      const double ua[4] = {u01.x, u01.y, u23.x, u23.y}, ub[4] = {b01.x, b01.y, b23.x, b23.y};
      const double wd = sw[d];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const double df = ua[a] - ub[b];
          if (!MAT || d < dsp) r2[a][b] = fma(wd * df, df, r2[a][b]);
          else r2m[a][b] = fma(wd * df, df, r2m[a][b]);
        }
    }
    // g = (m_i - m_j) 2 W_ij sf2 k_ij, gm the same with the Matern factor's derivative by -r2_mat (gpp_grad_tiles); 0 where the pair
    // shares a membership, lies on or above the diagonal or outside the matrix
    double g[4][4], gm[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int64_t i = i0 + 4 * ty + a;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int cb = gpp_tile_col(2 * tx, b);
        const int64_t j = j0 + cb;
        double gg = 0.0, gmm = 0.0;
        const int sgn = sm_a[4 * ty + a] - sm_b[cb];
        if (i < N && j < i && sgn != 0) {
          double kv, kd;
          kernel_and_dmat<MAT>(kind, gpp_exp_nonpos(-r2[a][b], ec), r2m[a][b], ec, kv, kd);
          const double Wij = 0.5 * (sal_a[4 * ty + a] * sal_b[cb] - kin[a][b]);
          const double s2w = (sgn > 0 ? 2.0 : -2.0) * Wij * sf2;
          gg = s2w * kv;
          gmm = s2w * kd;
        }
        g[a][b] = gg;
        gm[a][b] = gmm;
      }
    }
    for (int k = 0; k < C; ++k) {
      const int c = scol[k];
      if (c < 0) continue;
      const bool rbf_dim = !MAT || c < dsp;
      const double* pa = sa + c * GT + 4 * ty;
      const double* pb = sb + c * GT + 2 * tx;
      const double ub[4] = {pb[0], pb[1], pb[32], pb[33]};
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) s = fma(rbf_dim ? g[a][b] : gm[a][b], pa[a] - ub[b], s);
      s = wave_sum(s);
      if (lane == 0) wacc[wave * GD_MAX + k] += -2.0 * sw[c] * s;
    }
  }
  __syncthreads();
  if (tid < C) rec[(int64_t)blockIdx.x * C + tid] = (wacc[tid] + wacc[GD_MAX + tid]) + (wacc[2 * GD_MAX + tid] + wacc[3 * GD_MAX + tid]);
}

// g_theta[k] = the records' k-th sums, added in work-group order
__global__ __launch_bounds__(256) void gpp_calib_finish(const double* __restrict__ rec, int nwg, int C, double* __restrict__ g_theta) {
  __shared__ double red[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  double v = 0.0;
  for (int b = tid; b < nwg; b += 256) v += rec[(int64_t)b * C + k];
  block_sum(tid, v, (lds_double*)red);
  if (tid == 0) g_theta[k] = red[0];
}

}  // namespace

size_t gpp_calib_ws_bytes(int C) { return (size_t)G_WGS * (size_t)(C > 0 ? C : 0) * sizeof(double); }

hipError_t gpp_launch_calib_grad_reduce(hipStream_t s, const double* U, int64_t N, int D, const double* w, const double* sf2, int kind,
                                        int d_split, const double* alpha, const double* Kinv, int64_t ldk, const int32_t* member,
                                        const int32_t* cols, int C, double* g_theta, void* ws, size_t ws_bytes) {
  if (kind < 0 || kind > 2 || D < 1 || D > GD_MAX || C < 1 || C > D) return hipErrorInvalidValue;
  if (N <= 1) return hipMemsetAsync(g_theta, 0, (size_t)C * sizeof(double), s);  // no pair of distinct rows: an empty sum
  if (!ws || ws_bytes < gpp_calib_ws_bytes(C)) return hipErrorInvalidValue;
  const int64_t T = (N + GT - 1) / GT, ntiles = T * (T + 1) / 2;
  const int nwg = (int)(ntiles < G_WGS ? ntiles : G_WGS);
  double* rec = reinterpret_cast<double*>(ws);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(nwg), dim3(256), 0, s, U, N, D, w, sf2, kind, d_split, alpha, Kinv, ldk, member, cols, C, ntiles, rec);
  };
  const bool mat = kind != 0;
#define GPP_CT(DT) (mat ? launch(gpp_calib_tiles<DT, true>) : launch(gpp_calib_tiles<DT, false>))
  if (D <= 8) GPP_CT(8);
  else if (D <= 16) GPP_CT(16);
  else if (D <= 32) GPP_CT(32);
  else GPP_CT(64);
#undef GPP_CT
  hipLaunchKernelGGL(gpp_calib_finish, dim3(C), dim3(256), 0, s, rec, nwg, C, g_theta);
  return hipGetLastError();
}

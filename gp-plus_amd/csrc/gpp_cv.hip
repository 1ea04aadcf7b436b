// gpp_cv.hip — the two gathered, ragged products of grouped (k-fold) cross-validation (gpp_cv_blocks, gpp_cv_rows in gpp.h).
//
// With P = Ky^-1 = Linv^T Linv and a fold F (an ascending index set of size m), one factorisation gives every fold's held-out
// distribution p(y_F | y_-F) = N(y_F - P_FF^-1 alpha_F, P_FF^-1).  The two products whose rows are gathered by index:
//   P_FF[a,b] = sum_{j >= max(i_a, i_b)} Lbuf[i_a][j] Lbuf[i_b][j]          (gpp_cv_blocks; Lbuf: the Linv buffer with its mirror)
//   S[o_F + a, c] = sum_{b < m} G_F[a][b] Psq[i_b][c]                        (gpp_cv_rows; the row blocks G_F P[F, :] of the gradient)
// The reference has no counterpart: it names a LOOCV criterion (optim/mll_noise_continuation.py:54) and evaluates neither it nor a
// grouped form; gpytorch offers the leave-one-out pseudo-likelihood only.
//
// Both kernels use the 64 x 64 work-group tile of gpp_apply.hip: 256 threads, wave w owns rows 16 w .. 16 w + 15 and all four
// 16-column blocks, chunks of 32 of the contracted index staged in LDS, v_mfma_f64_16x16x4_f64.  One launch covers a whole CSR list of
// folds: a work-group finds its fold and its tile from blockIdx.x alone and reads that fold's indices only.  Every output element is
// the sum of the same terms in the same order whatever else the call holds (the chunk grid of gpp_cv_blocks starts at the tile's own
// smallest gathered index, that of gpp_cv_rows at 0): no float atomics, no work-group waits for another one, a fold's output does not
// depend on the other folds of the call and two launches agree bit for bit.
#include "gpp_internal.h"

#include <type_traits>

typedef double v2d __attribute__((ext_vector_type(2)));
typedef double v4d __attribute__((ext_vector_type(4)));

namespace {

constexpr int CV_T = 64;             // work-group tile edge
constexpr int CV_BK = 32;            // chunk of the contracted index
constexpr int CV_LDK = CV_BK + 2;    // [row][k] rows of a k-contiguous operand: 272-byte rows (16-byte aligned pairs)
constexpr int CV_LDC = CV_T + 16;    // [k][col] rows of a column-contiguous operand (gpp_apply.hip AP_LDC)
constexpr int CV_NONE = 0x7fffffff;  // gathered index of a row past the fold's end: every k is below it, the row is exact zeros

struct CvBlocksArgs {
  const double* Linv;
  const int32_t* idx;
  const int32_t* off;
  double* B;
  int64_t ldi, ldb, sB;
  int N, mp, T, npairs;
};

// 64 gathered rows x 32 columns [kb, kb + 32) of the Linv buffer into s[row][k], entries left of a row's diagonal (and right of N)
// as exact zeros.  Thread (ty, tx) = (tid >> 4, tid & 15) owns rows ty + 16 q and the column pair kb + 2 tx; kb is even, so a pair is
// one 16-byte load.  Nothing strictly below the diagonal is read: a pair that straddles the diagonal loads its upper element alone.
__device__ __forceinline__ void cv_stage_rows(double* s, const double* __restrict__ Linv, int64_t ldi, int N, const int (&r)[4], int kb,
                                              int ty, int tx) {
  const int j = kb + 2 * tx;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = r[q];
    v2d v = {0.0, 0.0};
    if (i != CV_NONE) {
      const double* row = Linv + (int64_t)i * ldi;
      if (j >= i) {
        if (j + 1 < N) v = *reinterpret_cast<const v2d*>(row + j);
        else if (j < N) v.x = row[j];
      } else if (j + 1 == i) {  // (i < N)
        v.y = row[i];
      }
    }
    *reinterpret_cast<v2d*>(s + (ty + 16 * q) * CV_LDK + 2 * tx) = v;
  }
}

__global__ __launch_bounds__(256) void gpp_cv_blocks_tile(const CvBlocksArgs p) {
  __shared__ __attribute__((aligned(16))) double sa[CV_T * CV_LDK];
  __shared__ __attribute__((aligned(16))) double sb[CV_T * CV_LDK];
  const int tid = threadIdx.x;
  const int f = blockIdx.x / p.npairs;
  int pr = blockIdx.x - f * p.npairs;
  int ta = 0;  // pair -> (ta <= tb): the tiles of the upper triangle row by row (uniform)
  while (pr >= p.T - ta) {
    pr -= p.T - ta;
    ++ta;
  }
  const int tb = ta + pr;
  const int o = p.off[f], m = p.off[f + 1] - o;
  const int a0 = ta * CV_T, b0 = tb * CV_T;
  const bool diag = ta == tb;
  const double* sbp = diag ? sa : sb;  // a diagonal tile multiplies its rows with themselves

  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int ty = tid >> 4, tx = tid & 15;

  v4d acc4[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc4[b] = (v4d){0.0, 0.0, 0.0, 0.0};

  if (b0 < m) {  // (a0 <= b0: both tiles hold rows of the fold; otherwise the tile is padding only)
    int ra[4], rb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = ty + 16 * q;
      ra[q] = a0 + r < m ? p.idx[o + a0 + r] : CV_NONE;
      rb[q] = b0 + r < m ? p.idx[o + b0 + r] : CV_NONE;
    }
    // every term has j >= max(i_a, i_b) >= the column tile's first (smallest) index: the chunks start there, at an even column
    const int klo = p.idx[o + b0] & ~1;
    const double* ga = sa + (wave * 16 + li) * CV_LDK + lk;
    const double* gb = sbp + li * CV_LDK + lk;
    for (int kb = klo; kb < p.N; kb += CV_BK) {
      __syncthreads();  // the previous chunk's LDS reads are done
      cv_stage_rows(sa, p.Linv, p.ldi, p.N, ra, kb, ty, tx);
      if (!diag) cv_stage_rows(sb, p.Linv, p.ldi, p.N, rb, kb, ty, tx);
      __syncthreads();
      // lane (i = l & 15, k = l >> 4) supplies A[row i][k] and B[k][col i] = rows of the second operand (gpp_gemm.hip, NT)
#pragma unroll
      for (int kk = 0; kk < CV_BK / 4; ++kk) {
        const double af = ga[4 * kk];
        double bf[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) bf[b] = gb[16 * b * CV_LDK + 4 * kk];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc4[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf[b], acc4[b], 0, 0, 0);
      }
    }
  }

  // element v of acc4[b]: row wave * 16 + 4 v + (l >> 4), column 16 b + (l & 15).  Upper triangle only; padding = identity.
  double* __restrict__ Bf = p.B + (int64_t)f * p.sB;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int c = b0 + 16 * b + li;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = a0 + wave * 16 + 4 * v + lk;
      if (r >= p.mp || c >= p.mp || c < r) continue;
      Bf[(int64_t)r * p.ldb + c] = (c < m) ? acc4[b][v] : (c == r ? 1.0 : 0.0);  // (r <= c < m: inside the fold)
    }
  }
}

struct CvRowsArgs {
  const double* G;
  const int32_t* idx;
  const int32_t* off;
  const double* Psq;
  double* S;
  int64_t ldg, sG, ldp, lds;
  int N, Tm;
};

__global__ __launch_bounds__(256) void gpp_cv_rows_tile(const CvRowsArgs p) {
  __shared__ __attribute__((aligned(16))) double sa[CV_T * CV_LDK];   // [64 rows of G_f][32 k]
  __shared__ __attribute__((aligned(16))) double sc[CV_BK * CV_LDC];  // [32 k][64 columns of the gathered rows of Psq]
  const int tid = threadIdx.x;
  const int f = blockIdx.x / p.Tm;
  const int a0 = (blockIdx.x - f * p.Tm) * CV_T;
  const int o = p.off[f], m = p.off[f + 1] - o;
  if (a0 >= m) return;  // (uniform: the launch has a tile row for every 64 rows a fold could have)
  const int c0 = blockIdx.y * CV_T;
  const double* __restrict__ Gf = p.G + (int64_t)f * p.sG;

  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int ty = tid >> 4, tx = tid & 15;   // G: rows ty + 16 q, the k pair 2 tx
  const int cy = tid >> 5, cx = tid & 31;   // Psq: k = cy + 8 q, the column pair 2 cx
  const int nb = min(4, (p.N - c0 + 15) >> 4);  // 16-column blocks of this tile that hold a column (uniform)

  v4d acc4[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc4[b] = (v4d){0.0, 0.0, 0.0, 0.0};

  const double* ga = sa + (wave * 16 + li) * CV_LDK + lk;
  const double* cb = sc + lk * CV_LDC + li;
  for (int kb = 0; kb < m; kb += CV_BK) {
    __syncthreads();
    {  // the padding of G_f (rows and columns from m on) is never read
      const int k = kb + 2 * tx;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int r = a0 + ty + 16 * q;
        v2d v = {0.0, 0.0};
        if (r < m) {
          const double* row = Gf + (int64_t)r * p.ldg;
          if (k + 1 < m) v = *reinterpret_cast<const v2d*>(row + k);
          else if (k < m) v.x = row[k];
        }
        *reinterpret_cast<v2d*>(sa + (ty + 16 * q) * CV_LDK + 2 * tx) = v;
      }
    }
    {
      const int c = c0 + 2 * cx;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = kb + cy + 8 * q;
        v2d v = {0.0, 0.0};
        if (k < m) {
          const double* row = p.Psq + (int64_t)p.idx[o + k] * p.ldp;
          if (c + 1 < p.N) v = *reinterpret_cast<const v2d*>(row + c);
          else if (c < p.N) v.x = row[c];
        }
        *reinterpret_cast<v2d*>(sc + (cy + 8 * q) * CV_LDC + 2 * cx) = v;
      }
    }
    __syncthreads();
    // one straight-line body per count of live column blocks (gpp_apply.hip)
    auto products = [&](auto nbc) {
      constexpr int NB = decltype(nbc)::value;
#pragma unroll
      for (int kk = 0; kk < CV_BK / 4; ++kk) {
        const double af = ga[4 * kk];
        double bf[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) bf[b] = cb[4 * kk * CV_LDC + 16 * b];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc4[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf[b], acc4[b], 0, 0, 0);
      }
    };
    if (nb == 4) products(std::integral_constant<int, 4>{});
    else if (nb == 3) products(std::integral_constant<int, 3>{});
    else if (nb == 2) products(std::integral_constant<int, 2>{});
    else products(std::integral_constant<int, 1>{});
  }

#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int c = c0 + 16 * b + li;
    if (c >= p.N) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = a0 + wave * 16 + 4 * v + lk;
      if (r >= m) continue;
      p.S[(int64_t)(o + r) * p.lds + c] = acc4[b][v];
    }
  }
}

inline bool cv_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int cv_rc(hipError_t e) { return e == hipSuccess ? 0 : 1000 + (int)e; }

}  // namespace

int gpp_cv_blocks(gpp_handle_t h, const double* Linv, int64_t ldi, int64_t N, const int32_t* idx, const int32_t* off, int nfolds,
                  int mp, double* B, int64_t ldb, int64_t sB) {
  if (!h) return -1;
  if (!Linv || !cv_aligned16(Linv) || (ldi & 1) || ldi < N) return -3;
  if (N < 0 || N > 0x7ffffffe) return -4;
  if (!idx) return -5;
  if (!off) return -6;
  if (nfolds < 0) return -7;
  if (mp < 1) return -8;
  if (!B || !cv_aligned16(B)) return -9;
  if ((ldb & 1) || ldb < mp) return -10;
  if ((sB & 1) || (nfolds > 1 && sB < (int64_t)mp * ldb)) return -11;
  if (nfolds == 0) return 0;
  CvBlocksArgs a{};
  a.Linv = Linv; a.idx = idx; a.off = off; a.B = B;
  a.ldi = ldi; a.ldb = ldb; a.sB = sB;
  a.N = (int)N; a.mp = mp;
  a.T = (mp + CV_T - 1) / CV_T;
  a.npairs = a.T * (a.T + 1) / 2;
  const int64_t groups = (int64_t)nfolds * a.npairs;
  if (groups > 0x7fffffff) return -7;
  hipLaunchKernelGGL(gpp_cv_blocks_tile, dim3((unsigned)groups), dim3(256), 0, h->stream, a);
  return cv_rc(hipGetLastError());
}

int gpp_cv_rows(gpp_handle_t h, const double* G, int64_t ldg, int64_t sG, const int32_t* idx, const int32_t* off, int nfolds,
                const double* Psq, int64_t ldp, int64_t N, double* S, int64_t lds) {
  if (!h) return -1;
  if (!G || !cv_aligned16(G)) return -2;
  if ((ldg & 1) || ldg < 1) return -3;
  if ((sG & 1) || (nfolds > 1 && sG < ldg)) return -4;
  if (!idx) return -5;
  if (!off) return -6;
  if (nfolds < 0) return -7;
  if (!Psq || !cv_aligned16(Psq)) return -8;
  if ((ldp & 1) || ldp < N) return -9;
  if (N < 0 || N > 0x7ffffffe) return -10;
  if (!S || !cv_aligned16(S)) return -11;
  if ((lds & 1) || lds < N) return -12;
  if (nfolds == 0 || N == 0) return 0;
  CvRowsArgs a{};
  a.G = G; a.idx = idx; a.off = off; a.Psq = Psq; a.S = S;
  a.ldg = ldg; a.sG = sG; a.ldp = ldp; a.lds = lds;
  a.N = (int)N;
  // a fold has at most ldg rows (G_f is square inside rows of ldg doubles) and, beside other folds, at most sG / ldg
  const int64_t mmax = nfolds > 1 ? (sG / ldg < ldg ? sG / ldg : ldg) : ldg;
  a.Tm = (int)((mmax + CV_T - 1) / CV_T);
  const int64_t groups = (int64_t)nfolds * a.Tm, tiles_n = (N + CV_T - 1) / CV_T;
  if (groups > 0x7fffffff || tiles_n > 65535) return -7;
  hipLaunchKernelGGL(gpp_cv_rows_tile, dim3((unsigned)groups, (unsigned)tiles_n), dim3(256), 0, h->stream, a);
  return cv_rc(hipGetLastError());
}

// gpp_append.hip — border a cached factorisation with q new points in O(N^2 q) (gpp_chol_append in gpp.h).
//
// Ky = L L^T is cached as the upper factor U = L^T in A and as Linv = L^-1 (lower) with its mirror L^-T (upper) in the Linv buffer,
// beside z = Linv r and alpha = Linv^T z.  With the cross block k = K(X, Xq) (N x q), the corner C = K(Xq, Xq) + noise (upper) and the
// new residuals r_q:
//   V  = (Linv k)^T                       q x N     the new COLUMNS of U are V^T (rows 0 .. N-1, columns N .. N+q-1)
//   S  = C - V V^T = Ls Ls^T              q x q     the corner of U is Ls^T
//   W  = -Ls^-1 (V Linv)                  q x N     the new rows of Linv, mirrored into its new columns; corner Ls^-1 with its mirror
//   zq = Ls^-1 (r_q - V z)                          z' = [z; zq]
//   alpha' = [alpha + W^T zq ; Ls^-T zq]
// The leading N x N windows of A and Linv are neither written nor (beyond the triangles named below) read.
// The reference has no counterpart: it refits (and refactorises) at every step of its BO loop (bayesian_optimizations/BO_GP_plus.py).
//
// Two routes leave the same layout.
//  q <= 16 (sequential design; bound by reading Linv once, not by flops): five launches.
//    ap_pack        kT[a][i] = k[i][a] into the workspace (the sweeps read their q-row operand row-contiguous)
//    ap_sweep<0>    V[a][j] = sum_{i <= j} Linv[j][i] kT[a][i]: work-group = 4 rows of the LOWER triangle, 16-byte loads; writes V to
//                   the workspace and the new columns of A
//    ap_dots        S[a][b] = C[a][b] - sum_j V[a][j] V[b][j] (a <= b) and t[a] = r_q[a] - sum_j V[a][j] z[j], one work-group each
//    ap_corner      Ls, Ls^-1, zq in LDS by one work-group; the two corners, z', the tail of alpha', *info
//    ap_sweep<1>    P[a][j] = sum_{i >= j} V[a][i] Linv[i][j], read through the MIRROR (row j from the diagonal on, contiguous);
//                   W = -Ls^-1 P in the epilogue, stored as new rows and new columns of Linv; alpha[j] += sum_a W[a][j] zq[a]
//    The two sweeps together read the N x N buffer once.  They cannot share a pass: P[., j] needs V[., i] of every row i >= j.
//  q > 16: the existing entry points — V by the TN GEMM against the mirror (as gpp_predict_tn), S by the NT GEMM on the upper
//    triangle, gpp_potrf + gpp_trtri on S in the workspace, P by the NN GEMM against the lower triangle, W = -Ls^-1 P by the NN GEMM
//    straight into the new rows of Linv — and small kernels of this file for what has no counterpart: the transposed scatter of V
//    and W into the new columns (8-byte accesses: column N of a row is 16-byte aligned only for even N), the corner copies, t, zq
//    and the alpha update.
// Every kernel here is a plain launch on the caller's stream; no cooperative launch, no work-group waits for another, no float
// atomics; every sum runs in an order fixed by (N, q) alone, so two launches agree bit for bit.
#include "gpp_internal.h"

typedef double v2d __attribute__((ext_vector_type(2)));

namespace {

constexpr int AP_Q = 16;   // widest skinny append
constexpr int AP_R = 4;    // rows of Linv per work-group of a sweep
constexpr int AP_T = 256;  // threads per work-group (4 waves)

inline int64_t ap_up16(int64_t n) { return n < 16 ? 16 : (n + 15) / 16 * 16; }
inline bool ap_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int ap_rc(hipError_t e) { return e == hipSuccess ? 0 : 1000 + (int)e; }
#define AP_CHECK_LAUNCH()                                  \
  do {                                                     \
    if (hipError_t e_ = hipGetLastError(); e_ != hipSuccess) return ap_rc(e_); \
  } while (0)

// sum over the work-group in a fixed order: xor-shuffles inside a wave, then the 4 waves' sums left to right.  `red` holds 4 doubles.
__device__ __forceinline__ double ap_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // (red may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// kT[a][i] = k[i][a], a < q, i < N
__global__ __launch_bounds__(AP_T) void ap_pack(const double* __restrict__ k, int64_t ldk, int N, int q, double* __restrict__ kT,
                                                int64_t ldx) {
  const int64_t e = (int64_t)blockIdx.x * AP_T + threadIdx.x;
  if (e >= (int64_t)N * q) return;
  const int a = (int)(e / N), i = (int)(e - (int64_t)a * N);
  kT[(int64_t)a * ldx + i] = k[(int64_t)i * ldk + a];
}

struct SweepArgs {
  const double* Linv;  // the N x N window: lower triangle (sweep 0) or the mirror from the diagonal on (sweep 1)
  const double* X;     // QP rows of ldx doubles: kT (sweep 0) or V (sweep 1); rows >= q are not read
  double* V;           // sweep 0: workspace V, q rows of ldx
  double* A;           // sweep 0: the factor buffer (new columns written)
  double* Lout;        // sweep 1: the Linv buffer (new rows and new columns written)
  const double* Lsi;   // sweep 1: Ls^-1, [16][16] lower, zeros above
  const double* zq;    // sweep 1
  double* alpha;       // sweep 1: alpha[j] += sum_a W[a][j] zq[a]
  int64_t ldi, ldx, lda;
  int N, q;
};

template <int QP, int SECOND>
__global__ __launch_bounds__(AP_T) void ap_sweep(const SweepArgs p) {
  __shared__ double red[4][AP_R * QP];
  __shared__ double res[AP_R][AP_Q];
  __shared__ double wres[AP_R][AP_Q];
  const int tid = threadIdx.x;
  const int nblk = (p.N + AP_R - 1) / AP_R;
  // the longest rows first: the lower triangle's rows grow with j, the mirror's shrink
  const int j0 = (SECOND ? (int)blockIdx.x : nblk - 1 - (int)blockIdx.x) * AP_R;
  const int N = p.N;

  // Row r of the group is row j0 + r, columns [j0 + r, N) (mirror) or [0, j0 + r] (lower triangle).  A row past the window's end
  // reads the last row instead: its sums are never stored.
  const double* row[AP_R];
#pragma unroll
  for (int r = 0; r < AP_R; ++r) row[r] = p.Linv + (int64_t)min(j0 + r, N - 1) * p.ldi;
  const int cb = SECOND ? (j0 & ~1) : 0;
  const int ce = SECOND ? N : min(N, j0 + AP_R);

  double acc[AP_R][QP];
#pragma unroll
  for (int r = 0; r < AP_R; ++r)
#pragma unroll
    for (int a = 0; a < QP; ++a) acc[r][a] = 0.0;

  for (int c = cb + 2 * tid; c < ce; c += 2 * AP_T) {
    const bool pair = c + 1 < N;  // (c < N: a pair never reaches past the window's last column)
    v2d l[AP_R];
#pragma unroll
    for (int r = 0; r < AP_R; ++r) {
      v2d v;
      if (pair) v = *reinterpret_cast<const v2d*>(row[r] + c);
      else { v.x = row[r][c]; v.y = 0.0; }
      // entries outside the row's own range are exact zeros (selected, not multiplied)
      l[r].x = (SECOND ? c >= j0 + r : c <= j0 + r) ? v.x : 0.0;
      l[r].y = (SECOND ? c + 1 >= j0 + r : c + 1 <= j0 + r) ? v.y : 0.0;
    }
#pragma unroll
    for (int a = 0; a < QP; ++a) {
      v2d x = {0.0, 0.0};
      if (a < p.q) {
        const double* xr = p.X + (int64_t)a * p.ldx + c;
        if (pair) x = *reinterpret_cast<const v2d*>(xr);
        else x.x = xr[0];
      }
#pragma unroll
      for (int r = 0; r < AP_R; ++r) acc[r][a] = __builtin_fma(l[r].y, x.y, __builtin_fma(l[r].x, x.x, acc[r][a]));
    }
  }

  // work-group sums in a fixed order
#pragma unroll
  for (int r = 0; r < AP_R; ++r)
#pragma unroll
    for (int a = 0; a < QP; ++a) {
      double v = acc[r][a];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((tid & 63) == 0) red[tid >> 6][r * QP + a] = v;
    }
  __syncthreads();
  if (tid < AP_R * QP) {
    const int r = tid / QP, a = tid - r * QP;
    res[r][a] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  }
  __syncthreads();

  if (tid < AP_R * QP) {
    const int r = tid / QP, a = tid - r * QP;
    const int j = j0 + r;
    if (a < p.q && j < N) {
      if (!SECOND) {
        const double v = res[r][a];
        p.V[(int64_t)a * p.ldx + j] = v;
        p.A[(int64_t)j * p.lda + N + a] = v;
      } else {
        double w = 0.0;
        for (int b = 0; b <= a; ++b) w = __builtin_fma(p.Lsi[a * AP_Q + b], res[r][b], w);
        w = -w;
        wres[r][a] = w;
        p.Lout[(int64_t)(N + a) * p.ldi + j] = w;
        p.Lout[(int64_t)j * p.ldi + N + a] = w;
      }
    }
  }
  if (SECOND) {
    __syncthreads();
    if (tid < AP_R && j0 + tid < N) {
      double s = 0.0;
      for (int a = 0; a < p.q; ++a) s = __builtin_fma(wres[tid][a], p.zq[a], s);
      p.alpha[j0 + tid] += s;
    }
  }
}

// Work-group g < npairs: the pair (a <= b) of the upper triangle, S[a][b] = C[a][b] - sum_j V[a][j] V[b][j].
// Work-group npairs + a: t[a] = rq[a] - sum_j V[a][j] z[j].
__global__ __launch_bounds__(AP_T) void ap_dots(const double* __restrict__ V, int64_t ldv, int N, int q, int npairs,
                                                const double* __restrict__ C, int64_t ldc, double* __restrict__ S, int64_t lds,
                                                const double* __restrict__ rq, const double* __restrict__ z, double* __restrict__ t) {
  __shared__ double red[4];
  const int g = blockIdx.x;
  int a, b = -1;
  if (g < npairs) {
    a = 0;
    int pr = g;
    while (pr >= q - a) {
      pr -= q - a;
      ++a;
    }
    b = a + pr;
  } else {
    a = g - npairs;
  }
  const double* x = V + (int64_t)a * ldv;
  const double* y = b >= 0 ? V + (int64_t)b * ldv : z;
  double s = 0.0;
  for (int j = threadIdx.x; j < N; j += AP_T) s = __builtin_fma(x[j], y[j], s);
  s = ap_block_sum(s, red);
  if (threadIdx.x == 0) {
    if (b >= 0) S[(int64_t)a * lds + b] = C[(int64_t)a * ldc + b] - s;
    else t[a] = rq[a] - s;
  }
}

struct CornerArgs {
  const double* S;   // [16][16], upper triangle
  const double* t;   // r_q - V z
  double* Lsi;       // out: [16][16] Ls^-1, lower, zeros above (all zero when S is not positive definite)
  double* zq;        // out (zero when S is not positive definite)
  double* A;         // factor buffer: corner's upper triangle
  double* Linv;      // inverse-factor buffer: corner with its mirror
  double* z;
  double* alpha;
  int32_t* info;
  int64_t lda, ldi;
  int N, q;
};

// One work-group: Cholesky of the q x q Schur complement, its inverse, zq, and everything that lives in the two corners.
__global__ __launch_bounds__(AP_T) void ap_corner(const CornerArgs p) {
  __shared__ double M[AP_Q][AP_Q + 1];   // S, then Ls in the lower triangle
  __shared__ double Xi[AP_Q][AP_Q + 1];  // Ls^-1, lower
  __shared__ double zs[AP_Q];
  __shared__ int bad;
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15, q = p.q;
  if (tid == 0) bad = 0;
  if (i < q && j < q) M[i][j] = p.S[(i <= j ? i : j) * AP_Q + (i <= j ? j : i)];
  Xi[i][j] = 0.0;
  __syncthreads();
  for (int c = 0; c < q; ++c) {
    if (tid == 0) {
      const double d = M[c][c];
      if (!(d > 0.0) && !bad) bad = c + 1;  // the first non-positive or NaN pivot, as gpp_potrf reports it
      M[c][c] = sqrt(d);
    }
    __syncthreads();
    if (j == c && i > c && i < q) M[i][c] = M[i][c] / M[c][c];
    __syncthreads();
    if (i > c && i < q && j > c && j <= i) M[i][j] = __builtin_fma(-M[i][c], M[j][c], M[i][j]);
    __syncthreads();
  }
  // column c of the inverse by forward substitution, one thread per column
  if (tid < q) {
    const int c = tid;
    Xi[c][c] = 1.0 / M[c][c];
    for (int r = c + 1; r < q; ++r) {
      double s = 0.0;
      for (int k = c; k < r; ++k) s = __builtin_fma(M[r][k], Xi[k][c], s);
      Xi[r][c] = -s / M[r][r];
    }
  }
  __syncthreads();
  if (tid < q) {
    double s = 0.0;
    for (int b = 0; b <= tid; ++b) s = __builtin_fma(Xi[tid][b], p.t[b], s);
    zs[tid] = s;
  }
  __syncthreads();
  const bool ok = bad == 0;
  if (i < q && j < q) {
    p.Lsi[i * AP_Q + j] = (ok && j <= i) ? Xi[i][j] : 0.0;
    if (j >= i) p.A[(int64_t)(p.N + i) * p.lda + p.N + j] = M[j][i];  // U corner = Ls^T
    p.Linv[(int64_t)(p.N + i) * p.ldi + p.N + j] = j <= i ? Xi[i][j] : Xi[j][i];
  }
  if (tid < q) {
    p.zq[tid] = ok ? zs[tid] : 0.0;
    p.z[p.N + tid] = zs[tid];
    double s = 0.0;
    for (int b = tid; b < q; ++b) s = __builtin_fma(Xi[b][tid], zs[b], s);
    p.alpha[p.N + tid] = s;
  }
  if (tid == 0) *p.info = bad;
}

// ---- kernels of the wide route ---------------------------------------------------------------------------------------------------
// dst[r][c] = src[r][c] for r < rows, c < cols (upper != 0: only c >= r), 8-byte accesses
__global__ __launch_bounds__(AP_T) void ap_copy(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd,
                                                int rows, int cols, int upper) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int r0 = blockIdx.y * 64 + (threadIdx.x >> 6);
  if (c >= cols) return;
  for (int r = r0; r < min(rows, (int)blockIdx.y * 64 + 64); r += 4)
    if (!upper || c >= r) dst[(int64_t)r * ldd + c] = src[(int64_t)r * lds + c];
}

// dst[c][r] = src[r][c] for r < rows, c < cols through a 32 x 32 LDS tile, 8-byte accesses (dst may sit at an odd column)
__global__ __launch_bounds__(AP_T) void ap_scatter_t(const double* __restrict__ src, int64_t lds, double* __restrict__ dst, int64_t ldd,
                                                     int rows, int cols) {
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // ty 0..7
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int r = r0 + ty + 8 * s, c = c0 + tx;
    if (r < rows && c < cols) tile[ty + 8 * s][tx] = src[(int64_t)r * lds + c];
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int c = c0 + ty + 8 * s, r = r0 + tx;
    if (r < rows && c < cols) dst[(int64_t)c * ldd + r] = tile[tx][ty + 8 * s];
  }
}

// y[a] = sum_b M[a][b] x[b] over b <= a (upper == 0) or b >= a (upper != 0), one work-group per row; y2[a] = x[a] when y2 is given
__global__ __launch_bounds__(AP_T) void ap_trmv(const double* __restrict__ Mx, int64_t ld, int n, const double* __restrict__ x, int upper,
                                                double* __restrict__ y, double* __restrict__ y2) {
  __shared__ double red[4];
  const int a = blockIdx.x;
  const int b0 = upper ? a : 0, b1 = upper ? n : a + 1;
  double s = 0.0;
  for (int b = b0 + threadIdx.x; b < b1; b += AP_T) s = __builtin_fma(Mx[(int64_t)a * ld + b], x[b], s);
  s = ap_block_sum(s, red);
  if (threadIdx.x == 0) {
    y[a] = s;
    if (y2) y2[a] = x[a];
  }
}

// alpha[j] += sum_a W[a][j] zq[a], a ascending, one thread per column.  Where the Schur complement was not positive definite
// (*info != 0) alpha's head is left as it was, as the skinny route leaves it: W and zq then come from a failed factor.
__global__ __launch_bounds__(AP_T) void ap_alpha_head(const double* __restrict__ W, int64_t ldw, int N, int q, const double* __restrict__ zq,
                                                      double* __restrict__ alpha, const int32_t* __restrict__ info) {
  const int j = blockIdx.x * AP_T + threadIdx.x;
  if (j >= N || *info != 0) return;
  double s = 0.0;
  for (int a = 0; a < q; ++a) s = __builtin_fma(W[(int64_t)a * ldw + j], zq[a], s);
  alpha[j] += s;
}

template <int QP>
hipError_t ap_launch_sweeps(hipStream_t s, int second, const SweepArgs& a) {
  const unsigned blocks = (unsigned)((a.N + AP_R - 1) / AP_R);
  if (second) hipLaunchKernelGGL((ap_sweep<QP, 1>), dim3(blocks), dim3(AP_T), 0, s, a);
  else hipLaunchKernelGGL((ap_sweep<QP, 0>), dim3(blocks), dim3(AP_T), 0, s, a);
  return hipGetLastError();
}

hipError_t ap_sweep_by_q(hipStream_t s, int second, const SweepArgs& a) {
  if (a.q == 1) return ap_launch_sweeps<1>(s, second, a);
  if (a.q == 2) return ap_launch_sweeps<2>(s, second, a);
  if (a.q <= 4) return ap_launch_sweeps<4>(s, second, a);
  if (a.q <= 8) return ap_launch_sweeps<8>(s, second, a);
  return ap_launch_sweeps<16>(s, second, a);
}

}  // namespace

size_t gpp_append_ws_bytes(int64_t N, int64_t q) {
  if (N < 0 || q < 1) return 0;
  const int64_t ldn = ap_up16(N);
  if (q <= AP_Q) return (size_t)(2 * AP_Q * ldn + 2 * AP_Q * AP_Q + 2 * AP_Q) * sizeof(double);
  const int64_t ldq = ap_up16(q);
  return (size_t)(2 * q * ldn + 3 * q * ldq + 2 * ldq) * sizeof(double);
}

extern "C" int gpp_chol_append(gpp_handle_t h, double* A, int64_t ld, double* Linv, int64_t ldi, int64_t N, int64_t q, const double* k,
                               int64_t ldk, const double* C, int64_t ldc, const double* rq, double* z, double* alpha,
                               int32_t* info_dev) {
  if (!h) return -1;
  if (N < 1 || N > 0x7ffffff0) return -6;
  if (q < 1 || N + q > 0x7ffffff0) return -7;
  if (!A || !ap_aligned16(A) || (ld & 1) || ld < N + q) return -2;
  if (!Linv || !ap_aligned16(Linv) || (ldi & 1) || ldi < N + q) return -4;
  if (!k || !ap_aligned16(k) || (ldk & 1) || ldk < q) return -8;
  if (!C || !ap_aligned16(C) || (ldc & 1) || ldc < q) return -10;
  if (!rq) return -12;
  if (!z) return -13;
  if (!alpha) return -14;
  if (!info_dev) return -15;
  const size_t need = gpp_append_ws_bytes(N, q);
  if (!h->ws || h->ws_bytes < need) return GPP_NO_WORKSPACE;
  hipStream_t s = h->stream;
  double* w = reinterpret_cast<double*>(h->ws);
  const int64_t ldn = ap_up16(N);
  const int n = (int)N, qi = (int)q;

  if (q <= AP_Q) {
    double* kT = w;
    double* V = kT + AP_Q * ldn;
    double* S = V + AP_Q * ldn;
    double* Lsi = S + AP_Q * AP_Q;
    double* t = Lsi + AP_Q * AP_Q;
    double* zq = t + AP_Q;
    hipLaunchKernelGGL(ap_pack, dim3((unsigned)((N * q + AP_T - 1) / AP_T)), dim3(AP_T), 0, s, k, ldk, n, qi, kT, ldn);
    AP_CHECK_LAUNCH();
    SweepArgs a{};
    a.Linv = Linv; a.X = kT; a.V = V; a.A = A; a.ldi = ldi; a.ldx = ldn; a.lda = ld; a.N = n; a.q = qi;
    if (hipError_t e = ap_sweep_by_q(s, 0, a); e != hipSuccess) return ap_rc(e);
    const int npairs = qi * (qi + 1) / 2;
    hipLaunchKernelGGL(ap_dots, dim3((unsigned)(npairs + qi)), dim3(AP_T), 0, s, V, ldn, n, qi, npairs, C, ldc, S, (int64_t)AP_Q, rq, z, t);
    AP_CHECK_LAUNCH();
    CornerArgs c{};
    c.S = S; c.t = t; c.Lsi = Lsi; c.zq = zq; c.A = A; c.Linv = Linv; c.z = z; c.alpha = alpha; c.info = info_dev;
    c.lda = ld; c.ldi = ldi; c.N = n; c.q = qi;
    hipLaunchKernelGGL(ap_corner, dim3(1), dim3(AP_T), 0, s, c);
    AP_CHECK_LAUNCH();
    SweepArgs b{};
    b.Linv = Linv; b.X = V; b.Lout = Linv; b.Lsi = Lsi; b.zq = zq; b.alpha = alpha; b.ldi = ldi; b.ldx = ldn; b.N = n; b.q = qi;
    return ap_rc(ap_sweep_by_q(s, 1, b));
  }

  // ---- wide: the existing GEMM / potrf / trtri entry points on workspace operands -------------------------------------------------
  const int64_t ldq = ap_up16(q);
  double* V = w;
  double* P = V + q * ldn;
  double* S = P + q * ldn;
  double* Lsi = S + q * ldq;
  double* T = Lsi + q * ldq;
  double* t = T + q * ldq;
  double* zq = t + ldq;
  // gpp_potrf / gpp_trtri note on the handle which diagonal blocks the last factorisation inverted: that belongs to the caller's own
  // factorisation, not to the corner's
  const GppInvBlocks keep = gpp_inv_blocks_save(h);
  // V[a][j] = sum_{i <= j} k[i][a] Lbuf[i][j]: TN against the mirror (b_mask 1 keeps i <= j)
  if (int r = gpp_gemm(h, 1, 0, q, N, N, 1.0, k, ldk, Linv, ldi, 0.0, V, ldn, 0, 1, 0, 2, 0)) return r;
  const dim3 gq((unsigned)((q + 63) / 64), (unsigned)((q + 63) / 64));
  hipLaunchKernelGGL(ap_copy, gq, dim3(AP_T), 0, s, C, ldc, S, ldq, qi, qi, 1);
  AP_CHECK_LAUNCH();
  if (int r = gpp_gemm(h, 0, 1, q, q, N, -1.0, V, ldn, V, ldn, 1.0, S, ldq, 0, 0, 0, 0, 2)) return r;
  hipLaunchKernelGGL(ap_dots, dim3((unsigned)qi), dim3(AP_T), 0, s, V, ldn, n, qi, 0, C, ldc, S, ldq, rq, z, t);
  AP_CHECK_LAUNCH();
  int r = gpp_potrf(h, S, q, ldq, Lsi, ldq, info_dev);
  if (!r) r = gpp_trtri(h, S, q, ldq, Lsi, ldq, T, ldq);
  gpp_inv_blocks_restore(h, keep);
  if (r) return r;
  // P[a][j] = sum_{i >= j} V[a][i] Linv[i][j]: NN against the lower triangle (b_mask 2 keeps i >= j)
  if (int e = gpp_gemm(h, 0, 0, q, N, N, 1.0, V, ldn, Linv, ldi, 0.0, P, ldn, 0, 2, 2, 0, 0)) return e;
  // W = -Ls^-1 P into the new rows of Linv (a_mask 1 keeps b <= a: the corner buffer's upper triangle holds the mirror)
  double* Wrows = Linv + N * ldi;
  if (int e = gpp_gemm(h, 0, 0, q, N, q, -1.0, Lsi, ldq, P, ldn, 0.0, Wrows, ldi, 1, 0, 0, 1, 0)) return e;
  const dim3 gt((unsigned)((N + 31) / 32), (unsigned)((q + 31) / 32));
  hipLaunchKernelGGL(ap_scatter_t, gt, dim3(AP_T), 0, s, V, ldn, A + N, ld, qi, n);
  AP_CHECK_LAUNCH();
  hipLaunchKernelGGL(ap_scatter_t, gt, dim3(AP_T), 0, s, Wrows, ldi, Linv + N, ldi, qi, n);
  AP_CHECK_LAUNCH();
  hipLaunchKernelGGL(ap_copy, gq, dim3(AP_T), 0, s, S, ldq, A + N * ld + N, ld, qi, qi, 1);
  AP_CHECK_LAUNCH();
  hipLaunchKernelGGL(ap_copy, gq, dim3(AP_T), 0, s, Lsi, ldq, Linv + N * ldi + N, ldi, qi, qi, 0);
  AP_CHECK_LAUNCH();
  hipLaunchKernelGGL(ap_trmv, dim3((unsigned)qi), dim3(AP_T), 0, s, Lsi, ldq, qi, t, 0, zq, (double*)nullptr);
  AP_CHECK_LAUNCH();
  hipLaunchKernelGGL(ap_trmv, dim3((unsigned)qi), dim3(AP_T), 0, s, Lsi, ldq, qi, zq, 1, alpha + N, z + N);
  AP_CHECK_LAUNCH();
  hipLaunchKernelGGL(ap_alpha_head, dim3((unsigned)((N + AP_T - 1) / AP_T)), dim3(AP_T), 0, s, Wrows, ldi, n, qi, zq, alpha, info_dev);
  return ap_rc(hipGetLastError());
}

// gpp_dgrad.hip — the two kernels behind the posterior of the gradient (GP_Plus.predict_gradient / active_subspace) and the
// second-derivative block behind conditioning on gradient observations (GP_Plus.condition_on_gradients).
//
// gpp_cross_kernel_dx (gpp.h): the derivative cross block Dk[n, a nd + j] = d/du_{d0+j} sf2 k(Ua_a, Ub_n; w), training points as rows —
// the orientation gpp_predict_tn takes, so that Q = Dk^T Linv^T, the gradient's mean Q z and its variance diagonal come from the
// existing product.  One work-group per tile of DX_TA test points x DX_TN training points: the multipliers m_f of the file header of
// gpp_apply.hip (one exp, plus the Matern polynomial) are computed once per pair from features staged as sqrt(w) u — the arithmetic of
// KernelGen::dvalue, to which tests/pathwise_grad_reference.py's bound belongs — and left in LDS; the nd directions of a pair are then
// 2 w_d (ua_d - ub_d) m_f from the RAW features (an exact 0 where they agree, and for w_d == 0), written with 16-byte stores along the
// contiguous (a, j) axis.  Bandwidth-bound: M nd N doubles written once.
//
// gpp_point_gram (gpp.h): G[a] = Q_a Q_a^T of the nd rows of each point (nd <= 16), one work-group of 256 threads per point: thread t
// walks the columns n = 2 t, 2 t + 512, ... with 16-byte loads and keeps the nd (nd + 1) / 2 sums of the lower triangle in registers, a
// butterfly adds the 64 lanes of each wave, the four waves' sums are added in wave order, and both triangles are written from the one
// sum.  The order of a point's additions depends on (N, nd) alone.  The weighted sum over the points takes two more launches (groups
// of PG_GROUP points in index order, then the groups in index order) through the handle workspace.  No atomics.  No reference
// counterpart: the reference has no gradient posterior.
//
// gpp_kernel_dxdx (gpp.h): the second-derivative block H[a nd + j][b nd + l] = d^2/du_{d0+j} dv_{d0+l} sf2 k(Ua_a, Ub_b; w), the covariance
// of two gradient observations (GP_Plus.condition_on_gradients).  One work-group per tile of HX_TA x HX_TB pairs: the multipliers
// m_0 = -sf2 e1 h, m_1 = sf2 e1 h' and m_2 = -sf2 e1 h'' are computed once per pair by the staged arithmetic above and left in LDS; an
// entry is then (p_j p_l) m_{f(j) + f(l)} - delta_jl g_j m_{f(j)} with g = 2 w, p_j = g_j (ua_j - vb_j) from the RAW features and f = 0 on
// a feature of the RBF factor, 1 on one of the Matern factor.  The product p_j p_l and the one fused multiply-add are the same
// operations on the same numbers for the entries (a, j), (b, l) and (b, l), (a, j): with Ua = Ub the block is bitwise symmetric.
// 16-byte stores along the contiguous (b, l) axis.  Bandwidth-bound: Ma nd Mb nd doubles written once.
#include "../../include/gpp.h"
#include "gpp_internal.h"

namespace {

inline bool dg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int dg_rc(hipError_t e) { return e == hipSuccess ? 0 : 1000 + (int)e; }

// ---- gpp_cross_kernel_dx ------------------------------------------------------------------------------------------------------------
constexpr int DX_TA = 16;       // test points per tile (even: a tile's first column a0 nd is even, the 16-byte stores stay aligned)
constexpr int DX_TN = 32;       // training points per tile
constexpr int DX_TAP = DX_TA + 1;  // row stride of the multiplier tiles (odd: lanes that differ in n fall in different banks)
constexpr int DX_THREADS = 256;

struct DxArgs {
  const double* Ua;
  const double* Ub;
  const double* w;
  const double* sf2;
  double* Dk;
  int64_t ld;
  int M, N, D, kind, d_split, d0, nd, tiles_a;
};

// doubles of dynamic LDS: staged rows (odd stride D | 1), raw direction columns, 2 w and sqrt(w), the multiplier tiles
inline size_t dx_lds_doubles(int D, int nd, int nf) {
  return (size_t)(DX_TA + DX_TN) * (D | 1) + (size_t)DX_TA * nd + (size_t)DX_TN * (nd | 1) + nd + D + (size_t)nf * DX_TN * DX_TAP;
}

template <bool MAT>
__global__ __launch_bounds__(DX_THREADS) void gpp_cross_dx_f64(DxArgs p) {
  extern __shared__ __attribute__((aligned(16))) double dx_lds[];
  constexpr int NF = MAT ? 2 : 1;
  const int D = p.D, nd = p.nd, Dp = D | 1, ndp = nd | 1;
  double* sA = dx_lds;                   // [DX_TA][Dp]  sqrt(w_d) ua_d
  double* sB = sA + DX_TA * Dp;          // [DX_TN][Dp]  sqrt(w_d) ub_d
  double* rA = sB + DX_TN * Dp;          // [DX_TA][nd]  ua_{d0+j}
  double* rB = rA + DX_TA * nd;          // [DX_TN][ndp] ub_{d0+j}
  double* w2 = rB + DX_TN * ndp;         // [nd]         2 w_{d0+j}
  double* sw = w2 + nd;                  // [D]          sqrt(w_d)
  double* sM = sw + D;                   // [NF][DX_TN][DX_TAP] multipliers
  const int t = (int)threadIdx.x;
  const int ta = (int)(blockIdx.x % (unsigned)p.tiles_a), tn = (int)(blockIdx.x / (unsigned)p.tiles_a);
  const int a0 = ta * DX_TA, n0 = tn * DX_TN;
  const int na = min(DX_TA, p.M - a0), nn = min(DX_TN, p.N - n0);
  const int ds = (!MAT || p.kind == 0) ? D : p.d_split;  // dims below ds belong to the RBF factor

  for (int d = t; d < D; d += DX_THREADS) sw[d] = sqrt(p.w[d]);
  for (int j = t; j < nd; j += DX_THREADS) w2[j] = 2.0 * p.w[p.d0 + j];
  __syncthreads();
  // rows beyond the matrices' ends are staged as zeros and never read from memory; their pairs are computed and never stored
  for (int i = t; i < (DX_TA + DX_TN) * D; i += DX_THREADS) {
    const int r = i / D, d = i - r * D;
    if (r < DX_TA) {
      const double u = r < na ? p.Ua[(int64_t)(a0 + r) * D + d] : 0.0;
      sA[r * Dp + d] = sw[d] * u;
      if (d >= p.d0 && d < p.d0 + nd) rA[r * nd + (d - p.d0)] = u;
    } else {
      const int rn = r - DX_TA;
      const double u = rn < nn ? p.Ub[(int64_t)(n0 + rn) * D + d] : 0.0;
      sB[rn * Dp + d] = sw[d] * u;
      if (d >= p.d0 && d < p.d0 + nd) rB[rn * ndp + (d - p.d0)] = u;
    }
  }
  __syncthreads();

  // the multipliers, once per pair: m_0 = -(e1 h), m_1 = e1 h' from gpp_matern's pieces, as KernelGen::dvalue of gpp_apply.hip forms them
  const GppExpConsts ec = gpp_exp_consts();
  const double sf2 = *p.sf2;
  for (int pr = t; pr < DX_TA * DX_TN; pr += DX_THREADS) {
    const int nl = pr & (DX_TN - 1), al = pr / DX_TN;
    const double* ua = sA + al * Dp;
    const double* ub = sB + nl * Dp;
    double q1 = 0.0;
    for (int d = 0; d < ds; ++d) {
      const double df = ua[d] - ub[d];
      q1 = fma(df, df, q1);
    }
    const double e1 = sf2 * gpp_exp_nonpos(-q1, ec);
    if constexpr (MAT) {
      double q2 = 0.0;
      for (int d = ds; d < D; ++d) {
        const double df = ua[d] - ub[d];
        q2 = fma(df, df, q2);
      }
      // (one call per kind, the products inside the branches: with a single call the two exp chains of a pair meet in one block,
      //  the scheduler interleaves them and the kernel takes 50 registers instead of 48)
      double h, hp;
      if (p.kind == 1) {
        const GppMatern m = gpp_matern(1, q2, ec);
        h = m.p * m.er;
        hp = m.dp * m.er;
      } else {
        const GppMatern m = gpp_matern(2, q2, ec);
        h = m.p * m.er;
        hp = m.dp * m.er;
      }
      sM[nl * DX_TAP + al] = -(e1 * h);
      sM[DX_TN * DX_TAP + nl * DX_TAP + al] = e1 * hp;
    } else {
      sM[nl * DX_TAP + al] = -e1;
    }
  }
  __syncthreads();

  // the tile's nn rows of cw = na nd contiguous columns, two columns per lane: consecutive lanes write consecutive 16 bytes
  const int cw = na * nd, hp2 = (cw + 1) >> 1;
  int ct = 1;
  while (ct < hp2 && ct < DX_THREADS) ct <<= 1;
  const int rt = DX_THREADS / ct;
  double* out = p.Dk + (int64_t)n0 * p.ld + (int64_t)a0 * nd;
  for (int pc = t % ct; pc < hp2; pc += ct) {
    const int c0 = 2 * pc;
    const bool two = c0 + 1 < cw;
    const int al0 = c0 / nd, j0 = c0 - al0 * nd;
    int al1 = al0, j1 = j0 + 1;
    if (j1 == nd) { j1 = 0; al1 = al0 + 1; }
    if (!two) { al1 = al0; j1 = j0; }
    const int f0 = (NF == 2 && p.d0 + j0 >= ds) ? DX_TN * DX_TAP : 0;
    const int f1 = (NF == 2 && p.d0 + j1 >= ds) ? DX_TN * DX_TAP : 0;
    const double x0 = rA[al0 * nd + j0], x1 = rA[al1 * nd + j1];
    const double g0 = w2[j0], g1 = w2[j1];
    for (int row = t / ct; row < nn; row += rt) {
      const double v0 = (g0 * (x0 - rB[row * ndp + j0])) * sM[f0 + row * DX_TAP + al0];
      double* dst = out + (int64_t)row * p.ld + c0;
      if (two) {
        const double v1 = (g1 * (x1 - rB[row * ndp + j1])) * sM[f1 + row * DX_TAP + al1];
        *reinterpret_cast<double2*>(dst) = make_double2(v0, v1);
      } else {
        *dst = v0;
      }
    }
  }
}

// ---- gpp_point_gram -----------------------------------------------------------------------------------------------------------------
constexpr int PG_WAVES = 4;    // waves of a point's work-group: each takes every fourth run of 64 column pairs
constexpr int PG_GROUP = 32;   // points per partial sum of the weighted total

template <int ND>
__global__ __launch_bounds__(64 * PG_WAVES) void gpp_point_gram_f64(const double* __restrict__ Q, int64_t ldq, int M, int nd, int N,
                                                                    double* __restrict__ G) {
  constexpr int NT = ND * (ND + 1) / 2;
  __shared__ double sG[PG_WAVES][NT];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int a = (int)blockIdx.x;  // (always < M: one work-group per point)
  double acc[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = 0.0;
  {
    const double* q0 = Q + (int64_t)a * nd * ldq;
    const int npairs = (N + 1) >> 1;
    for (int pc = (int)threadIdx.x; pc < npairs; pc += 64 * PG_WAVES) {
      const int n = 2 * pc;
      const bool two = n + 1 < N;  // the last column of an odd N is read alone: nothing at or beyond column N is touched
      double2 q[ND];
#pragma unroll
      for (int j = 0; j < ND; ++j) {
        if (j < nd) {
          const double* src = q0 + (int64_t)j * ldq + n;
          if (two) q[j] = *reinterpret_cast<const double2*>(src);
          else q[j] = make_double2(*src, 0.0);
        } else {
          q[j] = make_double2(0.0, 0.0);
        }
      }
#pragma unroll
      for (int j = 0; j < ND; ++j)
#pragma unroll
        for (int i = 0; i <= j; ++i) {
          const int k = j * (j + 1) / 2 + i;
          acc[k] = fma(q[j].x, q[i].x, acc[k]);
          acc[k] = fma(q[j].y, q[i].y, acc[k]);
        }
    }
  }
  // butterfly over each wave (every lane ends with the same sum), then the waves' sums in wave order: an order that depends on
  // nothing but the thread count
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) sG[wave][k] = v;
  }
  __syncthreads();
  double* g = G + (int64_t)a * nd * nd;
  for (int e = (int)threadIdx.x; e < nd * nd; e += 64 * PG_WAVES) {
    const int j = e / nd, i = e - j * nd;
    const int hi = max(i, j), lo = min(i, j), k = hi * (hi + 1) / 2 + lo;
    double s = sG[0][k];
#pragma unroll
    for (int v = 1; v < PG_WAVES; ++v) s += sG[v][k];
    g[e] = s;  // both triangles from the one sum: bitwise symmetric
  }
}

// partial[g][e] = sum over the points a of group g, in index order, of omega_a G[a][e]
__global__ __launch_bounds__(256) void gpp_point_gram_group(const double* __restrict__ G, const double* __restrict__ omega, int M, int nn,
                                                            double* __restrict__ part) {
  const int e = (int)threadIdx.x;
  if (e >= nn) return;
  const int a0 = (int)blockIdx.x * PG_GROUP, a1 = min(a0 + PG_GROUP, M);
  double s = 0.0;
  for (int a = a0; a < a1; ++a) s = fma(omega ? omega[a] : 1.0, G[(int64_t)a * nn + e], s);
  part[(int64_t)blockIdx.x * nn + e] = s;
}

__global__ __launch_bounds__(256) void gpp_point_gram_total(const double* __restrict__ part, int groups, int nn, double* __restrict__ Gsum) {
  const int e = (int)threadIdx.x;
  if (e >= nn) return;
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += part[(int64_t)g * nn + e];
  Gsum[e] = s;
}

template <int ND>
void pg_launch(hipStream_t s, const double* Q, int64_t ldq, int M, int nd, int N, double* G) {
  hipLaunchKernelGGL(gpp_point_gram_f64<ND>, dim3((unsigned)M), dim3(64 * PG_WAVES), 0, s, Q, ldq, M, nd, N, G);
}

}  // namespace

size_t gpp_point_gram_ws_bytes(int64_t M, int nd) {
  if (M < 1 || nd < 1) return 0;
  return (size_t)((M + (M + PG_GROUP - 1) / PG_GROUP) * nd * nd) * sizeof(double);
}

extern "C" int gpp_cross_kernel_dx(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                                   const double* sf2, int kind, int d_split, int d0, int nd, double* Dk, int64_t ld) {
  if (!h) return -1;
  if (!Ua) return -2;
  if (M < 1 || M > 0x7ffffff0) return -3;
  if (!Ub) return -4;
  if (N < 1 || N > 0x7ffffff0) return -5;
  if (D < 1 || D > 64) return -6;
  if (!w) return -7;
  if (!sf2) return -8;
  if (kind < 0 || kind > 2) return -9;
  if (d_split < 0 || d_split > D) return -10;
  if (d0 < 0 || d0 >= D) return -11;
  if (nd < 1 || d0 + nd > D) return -12;
  if (M * nd > 0x7ffffff0) return -3;
  if (!Dk || !dg_aligned16(Dk)) return -13;
  if ((ld & 1) || ld < M * nd) return -14;
  const int64_t tiles_a = (M + DX_TA - 1) / DX_TA, tiles_n = (N + DX_TN - 1) / DX_TN;
  if (tiles_a * tiles_n >= ((int64_t)1 << 31)) return -3;
  DxArgs p{Ua, Ub, w, sf2, Dk, ld, (int)M, (int)N, D, kind, d_split, d0, nd, (int)tiles_a};
  const dim3 grid((unsigned)(tiles_a * tiles_n)), block(DX_THREADS);
  if (kind == GPP_KIND_RBF)
    hipLaunchKernelGGL(gpp_cross_dx_f64<false>, grid, block, dx_lds_doubles(D, nd, 1) * sizeof(double), h->stream, p);
  else
    hipLaunchKernelGGL(gpp_cross_dx_f64<true>, grid, block, dx_lds_doubles(D, nd, 2) * sizeof(double), h->stream, p);
  return dg_rc(hipGetLastError());
}

extern "C" int gpp_point_gram(gpp_handle_t h, const double* Q, int64_t ldq, int64_t M, int nd, int64_t N, const double* omega, double* G,
                              double* Gsum) {
  if (!h) return -1;
  if (!Q || !dg_aligned16(Q)) return -2;
  if (N < 1 || N > 0x7ffffff0) return -6;
  if ((ldq & 1) || ldq < N) return -3;
  if (nd < 1 || nd > 16) return -5;
  if (M < 1 || M * nd > 0x7ffffff0) return -4;
  if (!G && !Gsum) return -9;
  const int nn = nd * nd;
  const int groups = (int)((M + PG_GROUP - 1) / PG_GROUP);
  double* part = nullptr;
  if (Gsum) {
    if (!h->ws || h->ws_bytes < gpp_point_gram_ws_bytes(M, nd)) return GPP_NO_WORKSPACE;
    part = reinterpret_cast<double*>(h->ws);
    if (!G) G = part + (int64_t)groups * nn;  // only the sum is wanted: the points' own matrices stay in the workspace
  }
  const int m = (int)M, n = (int)N;
  if (nd == 1) pg_launch<1>(h->stream, Q, ldq, m, nd, n, G);
  else if (nd == 2) pg_launch<2>(h->stream, Q, ldq, m, nd, n, G);
  else if (nd <= 4) pg_launch<4>(h->stream, Q, ldq, m, nd, n, G);
  else if (nd <= 8) pg_launch<8>(h->stream, Q, ldq, m, nd, n, G);
  else if (nd <= 12) pg_launch<12>(h->stream, Q, ldq, m, nd, n, G);
  else pg_launch<16>(h->stream, Q, ldq, m, nd, n, G);
  if (hipError_t r = hipGetLastError(); r != hipSuccess) return dg_rc(r);
  if (Gsum) {
    hipLaunchKernelGGL(gpp_point_gram_group, dim3((unsigned)groups), dim3(256), 0, h->stream, G, omega, m, nn, part);
    hipLaunchKernelGGL(gpp_point_gram_total, dim3(1), dim3(256), 0, h->stream, part, groups, nn, Gsum);
  }
  return dg_rc(hipGetLastError());
}

// ---- gpp_kernel_dxdx ----------------------------------------------------------------------------------------------------------------
namespace {

constexpr int HX_TA = 16;          // row points per tile
constexpr int HX_TB = 16;          // column points per tile (even: a tile's first column b0 nd is even, the 16-byte stores stay aligned)
constexpr int HX_TBP = HX_TB + 1;  // row stride of the multiplier tiles
constexpr int HX_THREADS = 256;    // one pair per thread in the multiplier phase

struct HxArgs {
  const double* Ua;
  const double* Ub;
  const double* w;
  const double* sf2;
  double* H;
  int64_t ld;
  int Ma, Mb, D, kind, d_split, d0, nd, tiles_b;
};

// doubles of dynamic LDS: staged rows (odd stride D | 1), raw direction columns of both sides, 2 w and sqrt(w), the multiplier tiles
inline size_t hx_lds_doubles(int D, int nd, int nf) {
  return (size_t)(HX_TA + HX_TB) * (D | 1) + (size_t)(HX_TA + HX_TB) * (nd | 1) + nd + D + (size_t)nf * HX_TA * HX_TBP;
}

// (p_j p_l) m_F - [j == l] g_j m_f: one product, one fused multiply-add
__device__ __forceinline__ double hx_entry(double pj, double pl, double mF, bool diag, double gj, double mf) {
  return fma(pj * pl, mF, diag ? -(gj * mf) : 0.0);
}

template <bool MAT>
__global__ __launch_bounds__(HX_THREADS) void gpp_kernel_dxdx_f64(HxArgs p) {
  extern __shared__ __attribute__((aligned(16))) double hx_lds[];
  constexpr int NF = MAT ? 3 : 1;
  constexpr int MT = HX_TA * HX_TBP;  // doubles of one multiplier tile
  const int D = p.D, nd = p.nd, Dp = D | 1, ndp = nd | 1;
  double* sA = hx_lds;                   // [HX_TA][Dp]  sqrt(w_d) ua_d
  double* sB = sA + HX_TA * Dp;          // [HX_TB][Dp]  sqrt(w_d) vb_d
  double* rA = sB + HX_TB * Dp;          // [HX_TA][ndp] ua_{d0+j}
  double* rB = rA + HX_TA * ndp;         // [HX_TB][ndp] vb_{d0+j}
  double* w2 = rB + HX_TB * ndp;         // [nd]         2 w_{d0+j}
  double* sw = w2 + nd;                  // [D]          sqrt(w_d)
  double* sM = sw + D;                   // [NF][HX_TA][HX_TBP] multipliers
  const int t = (int)threadIdx.x;
  const int tb = (int)(blockIdx.x % (unsigned)p.tiles_b), ta = (int)(blockIdx.x / (unsigned)p.tiles_b);
  const int a0 = ta * HX_TA, b0 = tb * HX_TB;
  const int na = min(HX_TA, p.Ma - a0), nb = min(HX_TB, p.Mb - b0);
  const int ds = (!MAT || p.kind == 0) ? D : p.d_split;  // dims below ds belong to the RBF factor

  for (int d = t; d < D; d += HX_THREADS) sw[d] = sqrt(p.w[d]);
  for (int j = t; j < nd; j += HX_THREADS) w2[j] = 2.0 * p.w[p.d0 + j];
  __syncthreads();
  // rows beyond the matrices' ends are staged as zeros and never read from memory; their pairs are computed and never stored
  for (int i = t; i < (HX_TA + HX_TB) * D; i += HX_THREADS) {
    const int r = i / D, d = i - r * D;
    if (r < HX_TA) {
      const double u = r < na ? p.Ua[(int64_t)(a0 + r) * D + d] : 0.0;
      sA[r * Dp + d] = sw[d] * u;
      if (d >= p.d0 && d < p.d0 + nd) rA[r * ndp + (d - p.d0)] = u;
    } else {
      const int rb = r - HX_TA;
      const double u = rb < nb ? p.Ub[(int64_t)(b0 + rb) * D + d] : 0.0;
      sB[rb * Dp + d] = sw[d] * u;
      if (d >= p.d0 && d < p.d0 + nd) rB[rb * ndp + (d - p.d0)] = u;
    }
  }
  __syncthreads();

  // the multipliers, once per pair: those of gpp_cross_kernel_dx and m_2 = -(e1 h'') (gpp_matern_d2)
  {
    const GppExpConsts ec = gpp_exp_consts();
    const double sf2 = *p.sf2;
    const int bl = t & (HX_TB - 1), al = t / HX_TB;
    const double* ua = sA + al * Dp;
    const double* ub = sB + bl * Dp;
    double q1 = 0.0;
    for (int d = 0; d < ds; ++d) {
      const double df = ua[d] - ub[d];
      q1 = fma(df, df, q1);
    }
    const double e1 = sf2 * gpp_exp_nonpos(-q1, ec);
    if constexpr (MAT) {
      double q2 = 0.0;
      for (int d = ds; d < D; ++d) {
        const double df = ua[d] - ub[d];
        q2 = fma(df, df, q2);
      }
      const GppMatern h = gpp_matern(p.kind, q2, ec);
      sM[al * HX_TBP + bl] = -(e1 * (h.p * h.er));
      sM[MT + al * HX_TBP + bl] = e1 * (h.dp * h.er);
      sM[2 * MT + al * HX_TBP + bl] = -(e1 * gpp_matern_d2(p.kind, h));
    } else {
      sM[al * HX_TBP + bl] = -e1;
    }
  }
  __syncthreads();

  // the tile's na nd rows of cw = nb nd contiguous columns, two columns per lane: consecutive lanes write consecutive 16 bytes
  const int rows = na * nd, cw = nb * nd, hp2 = (cw + 1) >> 1;
  int ct = 1;
  while (ct < hp2 && ct < HX_THREADS) ct <<= 1;
  const int rt = HX_THREADS / ct;
  double* out = p.H + (int64_t)a0 * nd * p.ld + (int64_t)b0 * nd;
  for (int pc = t % ct; pc < hp2; pc += ct) {
    const int c0 = 2 * pc;
    const bool two = c0 + 1 < cw;
    const int bl0 = c0 / nd, l0 = c0 - bl0 * nd;
    int bl1 = bl0, l1 = l0 + 1;
    if (l1 == nd) { l1 = 0; bl1 = bl0 + 1; }
    if (!two) { bl1 = bl0; l1 = l0; }
    const int f0 = (NF == 3 && p.d0 + l0 >= ds) ? 1 : 0;
    const int f1 = (NF == 3 && p.d0 + l1 >= ds) ? 1 : 0;
    const double y0 = rB[bl0 * ndp + l0], y1 = rB[bl1 * ndp + l1];
    const double g0 = w2[l0], g1 = w2[l1];
    for (int row = t / ct; row < rows; row += rt) {
      const int al = row / nd, j = row - al * nd;
      const int fj = (NF == 3 && p.d0 + j >= ds) ? 1 : 0;
      const double* xa = rA + al * ndp;
      const double gj = w2[j], xj = xa[j];
      const double* m0 = sM + al * HX_TBP + bl0;
      const double v0 = hx_entry(gj * (xj - rB[bl0 * ndp + j]), g0 * (xa[l0] - y0), m0[(fj + f0) * MT], j == l0, gj, m0[fj * MT]);
      double* dst = out + (int64_t)row * p.ld + c0;
      if (two) {
        const double* m1 = sM + al * HX_TBP + bl1;
        const double v1 = hx_entry(gj * (xj - rB[bl1 * ndp + j]), g1 * (xa[l1] - y1), m1[(fj + f1) * MT], j == l1, gj, m1[fj * MT]);
        *reinterpret_cast<double2*>(dst) = make_double2(v0, v1);
      } else {
        *dst = v0;
      }
    }
  }
}

}  // namespace

extern "C" int gpp_kernel_dxdx(gpp_handle_t h, const double* Ua, int64_t Ma, const double* Ub, int64_t Mb, int D, const double* w,
                               const double* sf2, int kind, int d_split, int d0, int nd, double* H, int64_t ld) {
  if (!h) return -1;
  if (!Ua) return -2;
  if (Ma < 1 || Ma > 0x7ffffff0) return -3;
  if (!Ub) return -4;
  if (Mb < 1 || Mb > 0x7ffffff0) return -5;
  if (D < 1 || D > 64) return -6;
  if (!w) return -7;
  if (!sf2) return -8;
  if (kind < 0 || kind > 2) return -9;
  if (d_split < 0 || d_split > D) return -10;
  if (d0 < 0 || d0 >= D) return -11;
  if (nd < 1 || d0 + nd > D) return -12;
  if (Ma * nd > 0x7ffffff0) return -3;
  if (Mb * nd > 0x7ffffff0) return -5;
  if (!H || !dg_aligned16(H)) return -13;
  if ((ld & 1) || ld < Mb * nd) return -14;
  const int64_t tiles_a = (Ma + HX_TA - 1) / HX_TA, tiles_b = (Mb + HX_TB - 1) / HX_TB;
  if (tiles_a * tiles_b >= ((int64_t)1 << 31)) return -3;
  HxArgs p{Ua, Ub, w, sf2, H, ld, (int)Ma, (int)Mb, D, kind, d_split, d0, nd, (int)tiles_b};
  const dim3 grid((unsigned)(tiles_a * tiles_b)), block(HX_THREADS);
  if (kind == GPP_KIND_RBF)
    hipLaunchKernelGGL(gpp_kernel_dxdx_f64<false>, grid, block, hx_lds_doubles(D, nd, 1) * sizeof(double), h->stream, p);
  else
    hipLaunchKernelGGL(gpp_kernel_dxdx_f64<true>, grid, block, hx_lds_doubles(D, nd, 3) * sizeof(double), h->stream, p);
  return dg_rc(hipGetLastError());
}

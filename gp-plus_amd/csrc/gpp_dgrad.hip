// gpp_dgrad.hip — the two kernels behind the posterior of the gradient (GP_Plus.predict_gradient / active_subspace) and the
// second-derivative block behind conditioning on gradient observations (GP_Plus.condition_on_gradients), and the gradient of the
// joint log-likelihood through both derivative blocks (gpp_gek_grad_reduce, described in front of its code at the end of the file).
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
//
// Partial gradients (gpp.h: the three _sel entry points): the same kernels with a second instantiation (SEL) in which a tile's points
// own the compact rows / columns first[a0] .. first[a0 + na) - 1 of a selection and the map from compact index to (point, direction)
// is staged in LDS once per tile; pairs, multipliers and every entry's arithmetic are those of the dense instantiation.
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
  const int* first;  // SEL: the selection of the Ua side (gpp.h), device pointers; unread otherwise
  const int* dir;
};

// doubles of dynamic LDS: staged rows (odd stride D | 1), raw direction columns, 2 w and sqrt(w), the multiplier tiles
inline size_t dx_lds_doubles(int D, int nd, int nf) {
  return (size_t)(DX_TA + DX_TN) * (D | 1) + (size_t)DX_TA * nd + (size_t)DX_TN * (nd | 1) + nd + D + (size_t)nf * DX_TN * DX_TAP;
}
// SEL: plus the tile's column map, one int per entry of its points
inline size_t dx_sel_lds_doubles(int D, int nd, int nf) { return dx_lds_doubles(D, nd, nf) + (size_t)(DX_TA * nd + 1) / 2; }

// An entry of a selection as the tiles stage it: the point within the tile and the direction (nd <= 64)
__device__ __forceinline__ int dg_pack(int point, int dir) { return (point << 8) | dir; }

// One tile's slice of a selection into LDS: map[c - first[p0]] = (point - p0, direction) of the compact row or column c, for the
// np points from p0 on.  A NULL selection is the dense layout, point-major.  One thread per point: each slot has one writer.
__device__ __forceinline__ void dg_stage_selection(const int* __restrict__ first, const int* __restrict__ dir, int p0, int np, int nd,
                                                   int* map, int t, int threads) {
  if (first) {
    const int c0 = first[p0];
    for (int r = t; r < np; r += threads) {
      const int k1 = first[p0 + r + 1];
      for (int k = first[p0 + r]; k < k1; ++k) map[k - c0] = dg_pack(r, dir[k]);
    }
  } else {
    for (int i = t; i < np * nd; i += threads) map[i] = dg_pack(i / nd, i % nd);
  }
}

// SEL: the tile's points own the compact columns [first[a0], first[a0 + na)) and entry k of point a is the direction
// dir[first[a] + k] (gpp_cross_kernel_dx_sel); the dense instantiation is the code it was.
template <bool MAT, bool SEL>
__device__ __forceinline__ void dx_tile(const DxArgs& p) {
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
  int cb = 0, ce = 0;  // SEL: the tile's compact columns [cb, ce)
  int* cmap = reinterpret_cast<int*>(sM + NF * DX_TN * DX_TAP);  // SEL: [ce - cb] (point, direction) of each
  if constexpr (SEL) {
    cb = p.first[a0];
    ce = p.first[a0 + na];
    if (cb == ce) return;  // (the whole work-group: a tile of points without an entry owns no column)
    dg_stage_selection(p.first, p.dir, a0, na, nd, cmap, t, DX_THREADS);
  }

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

  if constexpr (SEL) {
    // the tile's nn rows of its columns [cb, ce), paired on the ABSOLUTE column: a lane takes the even column c0 and c0 + 1, so a
    // 16-byte store is aligned whatever the parity of cb; an odd head (c0 = cb - 1) and an odd tail (c0 + 1 = ce) store one double
    // and leave the neighbouring tile's column alone
    const int cs = cb & ~1, hp2 = (ce - cs + 1) >> 1;
    int ct = 1;
    while (ct < hp2 && ct < DX_THREADS) ct <<= 1;
    const int rt = DX_THREADS / ct;
    double* out = p.Dk + (int64_t)n0 * p.ld;
    for (int pc = t % ct; pc < hp2; pc += ct) {
      const int c0 = cs + 2 * pc;
      const bool h0 = c0 >= cb, h1 = c0 + 1 < ce;  // (never both false: cb < ce)
      const int e0 = cmap[(h0 ? c0 : c0 + 1) - cb], e1 = cmap[(h1 ? c0 + 1 : c0) - cb];
      const int al0 = e0 >> 8, j0 = e0 & 255, al1 = e1 >> 8, j1 = e1 & 255;
      const int f0 = (NF == 2 && p.d0 + j0 >= ds) ? DX_TN * DX_TAP : 0;
      const int f1 = (NF == 2 && p.d0 + j1 >= ds) ? DX_TN * DX_TAP : 0;
      const double x0 = rA[al0 * nd + j0], x1 = rA[al1 * nd + j1];
      const double g0 = w2[j0], g1 = w2[j1];
      for (int row = t / ct; row < nn; row += rt) {
        const double v0 = (g0 * (x0 - rB[row * ndp + j0])) * sM[f0 + row * DX_TAP + al0];
        const double v1 = (g1 * (x1 - rB[row * ndp + j1])) * sM[f1 + row * DX_TAP + al1];
        double* dst = out + (int64_t)row * p.ld + c0;
        if (h0 && h1) *reinterpret_cast<double2*>(dst) = make_double2(v0, v1);
        else if (h0) dst[0] = v0;
        else dst[1] = v1;
      }
    }
    return;
  }
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

template <bool MAT, bool SEL>
__global__ __launch_bounds__(DX_THREADS) void gpp_cross_dx_f64(DxArgs p) {
  dx_tile<MAT, SEL>(p);
}

// gpp_cross_kernel_dx_batched: the tile of element blockIdx.y, whose operands lie b strides behind the first element's
template <bool MAT, bool SEL>
__global__ __launch_bounds__(DX_THREADS) void gpp_cross_dx_batched_f64(DxArgs p, int64_t sUa, int64_t sUb, int64_t sDk) {
  const int64_t b = blockIdx.y;
  p.Ua += b * sUa;
  p.Ub += b * sUb;
  p.w += b * p.D;
  p.sf2 += b;
  p.Dk += b * sDk;
  dx_tile<MAT, SEL>(p);
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

// the checks the derivative-block entry points share; 0 or the argument code
static int dg_check_pair(gpp_handle_t h, const double* Ua, int64_t Ma, const double* Ub, int64_t Mb, int D, const double* w,
                         const double* sf2, int kind, int d_split, int d0, int nd) {
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
  return 0;
}

// a selection's pair of pointers and its count q for M points: 0, or 1 for a mismatched pair, 2 for q out of range
static int dg_check_selection(const int* first, const int* dir, int64_t q, int64_t M, int nd) {
  if ((first == nullptr) != (dir == nullptr)) return 1;
  if (first ? (q < 1 || q > M * nd) : q != M * nd) return 2;
  return 0;
}

// The batch of a _batched entry point: the element count and the strides, in doubles, between the elements' feature rows and
// outputs.  The codes of what only a batch can get wrong lie behind every single-problem code.
constexpr int DG_ODD_STRIDE = -30;    // a stride is odd: the elements behind the first would lose their 16-byte alignment
constexpr int DG_BAD_BATCH = -31;     // batch outside 1 .. 65535 (the elements are the grid's y dimension)
constexpr int DG_SHORT_STRIDE = -32;  // a stride that is negative, or neither 0 (where 0 means shared) nor an element's extent
struct DgBatch {
  int batch;
  int64_t sUa, sUb, sOut;
};

// sa / sb: the strides of Ua (ra rows) and Ub (rb rows), 0 = shared; so: that of the rows x cols output window
static int dg_check_batch(const DgBatch& bt, int64_t ra, int64_t rb, int D, int64_t rows, int64_t cols, int64_t ld) {
  if (bt.batch < 1 || bt.batch > 65535) return DG_BAD_BATCH;
  if ((bt.sUa & 1) || (bt.sUb & 1) || (bt.sOut & 1)) return DG_ODD_STRIDE;
  if (bt.sUa != 0 && bt.sUa < ra * D) return DG_SHORT_STRIDE;
  if (bt.sUb != 0 && bt.sUb < rb * D) return DG_SHORT_STRIDE;
  if (bt.batch > 1 && bt.sOut < (rows - 1) * ld + cols) return DG_SHORT_STRIDE;
  return 0;
}

// gpp_cross_kernel_dx (first == NULL, cols = M nd) and gpp_cross_kernel_dx_sel; `shift`: how far the latter's three extra arguments
// move the codes of Dk and ld.  `bt`: the batch of gpp_cross_kernel_dx_batched, NULL for the single-problem calls.
static int dx_run(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w, const double* sf2,
                  int kind, int d_split, int d0, int nd, const int* first, const int* dir, int64_t cols, double* Dk, int64_t ld,
                  int shift, const DgBatch* bt = nullptr) {
  if (int rc = dg_check_pair(h, Ua, M, Ub, N, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (M * nd > 0x7ffffff0) return -3;
  if (!Dk || !dg_aligned16(Dk)) return -13 - shift;
  if ((ld & 1) || ld < cols) return -14 - shift;
  const int64_t tiles_a = (M + DX_TA - 1) / DX_TA, tiles_n = (N + DX_TN - 1) / DX_TN;
  if (tiles_a * tiles_n >= ((int64_t)1 << 31)) return -3;
  DxArgs p{Ua, Ub, w, sf2, Dk, ld, (int)M, (int)N, D, kind, d_split, d0, nd, (int)tiles_a, first, dir};
  const dim3 block(DX_THREADS);
  const bool mat = kind != GPP_KIND_RBF;
  const int nf = mat ? 2 : 1;
  if (bt) {
    if (int rc = dg_check_batch(*bt, M, N, D, N, cols, ld)) return rc;
    const dim3 grid((unsigned)(tiles_a * tiles_n), (unsigned)bt->batch);
    const size_t lds = (first ? dx_sel_lds_doubles(D, nd, nf) : dx_lds_doubles(D, nd, nf)) * sizeof(double);
    const int64_t sa = bt->sUa, sb = bt->sUb, so = bt->sOut;
    if (!first) {
      if (!mat) hipLaunchKernelGGL((gpp_cross_dx_batched_f64<false, false>), grid, block, lds, h->stream, p, sa, sb, so);
      else hipLaunchKernelGGL((gpp_cross_dx_batched_f64<true, false>), grid, block, lds, h->stream, p, sa, sb, so);
    } else {
      if (!mat) hipLaunchKernelGGL((gpp_cross_dx_batched_f64<false, true>), grid, block, lds, h->stream, p, sa, sb, so);
      else hipLaunchKernelGGL((gpp_cross_dx_batched_f64<true, true>), grid, block, lds, h->stream, p, sa, sb, so);
    }
    return dg_rc(hipGetLastError());
  }
  const dim3 grid((unsigned)(tiles_a * tiles_n));
  if (!first) {
    const size_t lds = dx_lds_doubles(D, nd, nf) * sizeof(double);
    if (!mat) hipLaunchKernelGGL((gpp_cross_dx_f64<false, false>), grid, block, lds, h->stream, p);
    else hipLaunchKernelGGL((gpp_cross_dx_f64<true, false>), grid, block, lds, h->stream, p);
  } else {
    const size_t lds = dx_sel_lds_doubles(D, nd, nf) * sizeof(double);
    if (!mat) hipLaunchKernelGGL((gpp_cross_dx_f64<false, true>), grid, block, lds, h->stream, p);
    else hipLaunchKernelGGL((gpp_cross_dx_f64<true, true>), grid, block, lds, h->stream, p);
  }
  return dg_rc(hipGetLastError());
}

extern "C" int gpp_cross_kernel_dx(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                                   const double* sf2, int kind, int d_split, int d0, int nd, double* Dk, int64_t ld) {
  return dx_run(h, Ua, M, Ub, N, D, w, sf2, kind, d_split, d0, nd, nullptr, nullptr, M * nd, Dk, ld, 0);
}

extern "C" int gpp_cross_kernel_dx_sel(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                                       const double* sf2, int kind, int d_split, int d0, int nd, const int* first_a, const int* dir_a,
                                       int64_t qa, double* Dk, int64_t ld) {
  if (int rc = dg_check_pair(h, Ua, M, Ub, N, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (M * nd > 0x7ffffff0) return -3;
  if (int rc = dg_check_selection(first_a, dir_a, qa, M, nd)) return rc == 1 ? -14 : -15;
  return dx_run(h, Ua, M, Ub, N, D, w, sf2, kind, d_split, d0, nd, first_a, dir_a, qa, Dk, ld, 3);
}

extern "C" int gpp_cross_kernel_dx_batched(gpp_handle_t h, const double* Ua, int64_t sUa, int64_t M, const double* Ub, int64_t sUb,
                                           int64_t N, int D, const double* w, const double* sf2, int kind, int d_split, int d0, int nd,
                                           const int* first_a, const int* dir_a, int64_t qa, double* Dk, int64_t ld, int64_t sDk,
                                           int batch) {
  if (int rc = dg_check_pair(h, Ua, M, Ub, N, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (M * nd > 0x7ffffff0) return -3;
  if (int rc = dg_check_selection(first_a, dir_a, qa, M, nd)) return rc == 1 ? -14 : -15;
  const DgBatch bt{batch, sUa, sUb, sDk};
  return dx_run(h, Ua, M, Ub, N, D, w, sf2, kind, d_split, d0, nd, first_a, dir_a, qa, Dk, ld, 3, &bt);
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
  const int* first_a;  // SEL: the selections of the two sides (gpp.h), device pointers, a NULL pair for a dense side
  const int* dir_a;
  const int* first_b;
  const int* dir_b;
};

// doubles of dynamic LDS: staged rows (odd stride D | 1), raw direction columns of both sides, 2 w and sqrt(w), the multiplier tiles
inline size_t hx_lds_doubles(int D, int nd, int nf) {
  return (size_t)(HX_TA + HX_TB) * (D | 1) + (size_t)(HX_TA + HX_TB) * (nd | 1) + nd + D + (size_t)nf * HX_TA * HX_TBP;
}

// (p_j p_l) m_F - [j == l] g_j m_f: one product, one fused multiply-add
__device__ __forceinline__ double hx_entry(double pj, double pl, double mF, bool diag, double gj, double mf) {
  return fma(pj * pl, mF, diag ? -(gj * mf) : 0.0);
}

// SEL: plus the tile's row and column maps, one int per entry of its points
inline size_t hx_sel_lds_doubles(int D, int nd, int nf) { return hx_lds_doubles(D, nd, nf) + (size_t)(HX_TA + HX_TB) * nd / 2; }

// SEL: rows and columns through the selections of gpp_kernel_dxdx_sel, either side dense where its pair is NULL; the dense
// instantiation is the code it was.
template <bool MAT, bool SEL>
__device__ __forceinline__ void hx_tile(const HxArgs& p) {
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
  int rb = 0, re = 0, cb = 0, ce = 0;  // SEL: the tile's compact rows [rb, re) and columns [cb, ce)
  int* rmap = reinterpret_cast<int*>(sM + NF * MT);  // SEL: [re - rb] (point, direction) of each row
  int* cmap = rmap + HX_TA * nd;                     // SEL: [ce - cb] the same of each column
  if constexpr (SEL) {
    rb = p.first_a ? p.first_a[a0] : a0 * nd;
    re = p.first_a ? p.first_a[a0 + na] : (a0 + na) * nd;
    cb = p.first_b ? p.first_b[b0] : b0 * nd;
    ce = p.first_b ? p.first_b[b0 + nb] : (b0 + nb) * nd;
    if (rb == re || cb == ce) return;  // (the whole work-group: a tile of points without an entry owns no row or no column)
    dg_stage_selection(p.first_a, p.dir_a, a0, na, nd, rmap, t, HX_THREADS);
    dg_stage_selection(p.first_b, p.dir_b, b0, nb, nd, cmap, t, HX_THREADS);
  }

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

  if constexpr (SEL) {
    // the tile's rows [rb, re) of its columns [cb, ce), paired on the ABSOLUTE column as in gpp_cross_dx_f64: an aligned 16-byte
    // store on an even column, one double at an odd head or tail
    const int rows = re - rb, cs = cb & ~1, hp2 = (ce - cs + 1) >> 1;
    int ct = 1;
    while (ct < hp2 && ct < HX_THREADS) ct <<= 1;
    const int rt = HX_THREADS / ct;
    double* out = p.H + (int64_t)rb * p.ld;
    for (int pc = t % ct; pc < hp2; pc += ct) {
      const int c0 = cs + 2 * pc;
      const bool h0 = c0 >= cb, h1 = c0 + 1 < ce;  // (never both false: cb < ce)
      const int e0 = cmap[(h0 ? c0 : c0 + 1) - cb], e1 = cmap[(h1 ? c0 + 1 : c0) - cb];
      const int bl0 = e0 >> 8, l0 = e0 & 255, bl1 = e1 >> 8, l1 = e1 & 255;
      const int f0 = (NF == 3 && p.d0 + l0 >= ds) ? 1 : 0;
      const int f1 = (NF == 3 && p.d0 + l1 >= ds) ? 1 : 0;
      const double y0 = rB[bl0 * ndp + l0], y1 = rB[bl1 * ndp + l1];
      const double g0 = w2[l0], g1 = w2[l1];
      for (int row = t / ct; row < rows; row += rt) {
        const int er = rmap[row], al = er >> 8, j = er & 255;
        const int fj = (NF == 3 && p.d0 + j >= ds) ? 1 : 0;
        const double* xa = rA + al * ndp;
        const double gj = w2[j], xj = xa[j];
        const double* m0 = sM + al * HX_TBP + bl0;
        const double* m1 = sM + al * HX_TBP + bl1;
        const double v0 = hx_entry(gj * (xj - rB[bl0 * ndp + j]), g0 * (xa[l0] - y0), m0[(fj + f0) * MT], j == l0, gj, m0[fj * MT]);
        const double v1 = hx_entry(gj * (xj - rB[bl1 * ndp + j]), g1 * (xa[l1] - y1), m1[(fj + f1) * MT], j == l1, gj, m1[fj * MT]);
        double* dst = out + (int64_t)row * p.ld + c0;
        if (h0 && h1) *reinterpret_cast<double2*>(dst) = make_double2(v0, v1);
        else if (h0) dst[0] = v0;
        else dst[1] = v1;
      }
    }
    return;
  }
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

template <bool MAT, bool SEL>
__global__ __launch_bounds__(HX_THREADS) void gpp_kernel_dxdx_f64(HxArgs p) {
  hx_tile<MAT, SEL>(p);
}

// gpp_kernel_dxdx_batched: the tile of element blockIdx.y
template <bool MAT, bool SEL>
__global__ __launch_bounds__(HX_THREADS) void gpp_kernel_dxdx_batched_f64(HxArgs p, int64_t sUa, int64_t sUb, int64_t sH) {
  const int64_t b = blockIdx.y;
  p.Ua += b * sUa;
  p.Ub += b * sUb;
  p.w += b * p.D;
  p.sf2 += b;
  p.H += b * sH;
  hx_tile<MAT, SEL>(p);
}

}  // namespace

// gpp_kernel_dxdx (both pairs NULL, cols = Mb nd) and gpp_kernel_dxdx_sel; `shift`: how far the latter's six extra arguments move the
// codes of H and ld
static int hx_run(gpp_handle_t h, const double* Ua, int64_t Ma, const double* Ub, int64_t Mb, int D, const double* w, const double* sf2,
                  int kind, int d_split, int d0, int nd, const int* first_a, const int* dir_a, const int* first_b, const int* dir_b,
                  int64_t cols, double* H, int64_t ld, int shift, int64_t rows = 0, const DgBatch* bt = nullptr) {
  if (int rc = dg_check_pair(h, Ua, Ma, Ub, Mb, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (Ma * nd > 0x7ffffff0) return -3;
  if (Mb * nd > 0x7ffffff0) return -5;
  if (!H || !dg_aligned16(H)) return -13 - shift;
  if ((ld & 1) || ld < cols) return -14 - shift;
  const int64_t tiles_a = (Ma + HX_TA - 1) / HX_TA, tiles_b = (Mb + HX_TB - 1) / HX_TB;
  if (tiles_a * tiles_b >= ((int64_t)1 << 31)) return -3;
  HxArgs p{Ua, Ub, w, sf2, H, ld, (int)Ma, (int)Mb, D, kind, d_split, d0, nd, (int)tiles_b, first_a, dir_a, first_b, dir_b};
  const dim3 block(HX_THREADS);
  const bool mat = kind != GPP_KIND_RBF;
  const int nf = mat ? 3 : 1;
  if (bt) {
    if (int rc = dg_check_batch(*bt, Ma, Mb, D, rows, cols, ld)) return rc;
    const dim3 grid((unsigned)(tiles_a * tiles_b), (unsigned)bt->batch);
    const bool sel = first_a || first_b;
    const size_t lds = (sel ? hx_sel_lds_doubles(D, nd, nf) : hx_lds_doubles(D, nd, nf)) * sizeof(double);
    const int64_t sa = bt->sUa, sb = bt->sUb, so = bt->sOut;
    if (!sel) {
      if (!mat) hipLaunchKernelGGL((gpp_kernel_dxdx_batched_f64<false, false>), grid, block, lds, h->stream, p, sa, sb, so);
      else hipLaunchKernelGGL((gpp_kernel_dxdx_batched_f64<true, false>), grid, block, lds, h->stream, p, sa, sb, so);
    } else {
      if (!mat) hipLaunchKernelGGL((gpp_kernel_dxdx_batched_f64<false, true>), grid, block, lds, h->stream, p, sa, sb, so);
      else hipLaunchKernelGGL((gpp_kernel_dxdx_batched_f64<true, true>), grid, block, lds, h->stream, p, sa, sb, so);
    }
    return dg_rc(hipGetLastError());
  }
  const dim3 grid((unsigned)(tiles_a * tiles_b));
  if (!first_a && !first_b) {
    const size_t lds = hx_lds_doubles(D, nd, nf) * sizeof(double);
    if (!mat) hipLaunchKernelGGL((gpp_kernel_dxdx_f64<false, false>), grid, block, lds, h->stream, p);
    else hipLaunchKernelGGL((gpp_kernel_dxdx_f64<true, false>), grid, block, lds, h->stream, p);
  } else {
    const size_t lds = hx_sel_lds_doubles(D, nd, nf) * sizeof(double);
    if (!mat) hipLaunchKernelGGL((gpp_kernel_dxdx_f64<false, true>), grid, block, lds, h->stream, p);
    else hipLaunchKernelGGL((gpp_kernel_dxdx_f64<true, true>), grid, block, lds, h->stream, p);
  }
  return dg_rc(hipGetLastError());
}

extern "C" int gpp_kernel_dxdx(gpp_handle_t h, const double* Ua, int64_t Ma, const double* Ub, int64_t Mb, int D, const double* w,
                               const double* sf2, int kind, int d_split, int d0, int nd, double* H, int64_t ld) {
  return hx_run(h, Ua, Ma, Ub, Mb, D, w, sf2, kind, d_split, d0, nd, nullptr, nullptr, nullptr, nullptr, Mb * nd, H, ld, 0);
}

extern "C" int gpp_kernel_dxdx_sel(gpp_handle_t h, const double* Ua, int64_t Ma, const double* Ub, int64_t Mb, int D, const double* w,
                                   const double* sf2, int kind, int d_split, int d0, int nd, const int* first_a, const int* dir_a,
                                   int64_t qa, const int* first_b, const int* dir_b, int64_t qb, double* H, int64_t ld) {
  if (int rc = dg_check_pair(h, Ua, Ma, Ub, Mb, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (Ma * nd > 0x7ffffff0) return -3;
  if (Mb * nd > 0x7ffffff0) return -5;
  if (int rc = dg_check_selection(first_a, dir_a, qa, Ma, nd)) return rc == 1 ? -14 : -15;
  if (int rc = dg_check_selection(first_b, dir_b, qb, Mb, nd)) return rc == 1 ? -17 : -18;
  return hx_run(h, Ua, Ma, Ub, Mb, D, w, sf2, kind, d_split, d0, nd, first_a, dir_a, first_b, dir_b, qb, H, ld, 6);
}

extern "C" int gpp_kernel_dxdx_batched(gpp_handle_t h, const double* Ua, int64_t sUa, int64_t Ma, const double* Ub, int64_t sUb,
                                       int64_t Mb, int D, const double* w, const double* sf2, int kind, int d_split, int d0, int nd,
                                       const int* first_a, const int* dir_a, int64_t qa, const int* first_b, const int* dir_b,
                                       int64_t qb, double* H, int64_t ld, int64_t sH, int batch) {
  if (int rc = dg_check_pair(h, Ua, Ma, Ub, Mb, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (Ma * nd > 0x7ffffff0) return -3;
  if (Mb * nd > 0x7ffffff0) return -5;
  if (int rc = dg_check_selection(first_a, dir_a, qa, Ma, nd)) return rc == 1 ? -14 : -15;
  if (int rc = dg_check_selection(first_b, dir_b, qb, Mb, nd)) return rc == 1 ? -17 : -18;
  const DgBatch bt{batch, sUa, sUb, sH};
  return hx_run(h, Ua, Ma, Ub, Mb, D, w, sf2, kind, d_split, d0, nd, first_a, dir_a, first_b, dir_b, qb, H, ld, 6, qa, &bt);
}

// ---- gpp_gek_grad_reduce ------------------------------------------------------------------------------------------------------------
// The gradient of the joint log-likelihood of [y; grad y] through the two derivative blocks of
//   Kj = [[Kff, Kfg], [Kfg^T, Kgg]],   Kfg[i, a nd + j] = gpp_cross_kernel_dx(Ua = Ug, Ub = U),   Kgg = gpp_kernel_dxdx(Ug, Ug):
// sum over their entries of W dKj / dtheta with W = (alpha alpha^T - Kinv) / 2, the Kfg block counted for both triangles, theta in
// {w (all D), sf2, U[:, :dU], Ug[:, :dU]}.  Only the lower triangle of Kinv is read: the rows N + a nd + j against the columns i < N
// (Kfg^T) and, of Kgg, the pairs of points a >= b (twice for a > b; the block of a point with itself through max / min indices).
//
// Chain rule (tests/gek_reference.py's header one order further).  An entry is a derivative of F(q1, q2) = sf2 e^-q1 H(q2) in
// delta = u - v with dq / dw_d = delta_d^2 and dq / du_d = 2 w_d delta_d; a derivative of F by q1 is -F, so with A_k = e^-q1 H^(k)(q2) a
// partial of F of order n with k Matern indices is (-1)^(n - k) sf2 A_k.  With p_j = 2 w_j delta_j and f(j) the factor of feature j:
//   Kfg entry  E_j  = F_f(j) p_j                                      Kgg entry  E_jl = -F_f(j)f(l) p_j p_l - [j == l] 2 w_j F_f(j)
// One set of sums per PAIR of points serves all its nd or nd^2 entries:
//   Kfg:  P_k = sum_{j in k} W_j p_j;                         s0 = A_1 P_1 - A_0 P_0;                    r1 = A_2 P_1 - A_1 P_0
//   Kgg:  Q_m = sum_{f(j) + f(l) = m} W_jl p_j p_l,  D_k = sum_{j in k} W_jj 2 w_j;
//         s0 = -A_0 Q_0 + A_1 Q_1 - A_2 Q_2 + A_0 D_0 - A_1 D_1;      r1 = -A_1 Q_0 + A_2 Q_1 - A_3 Q_2 + A_1 D_0 - A_2 D_1
//   g_sf2 += s0;    g_w[d] += sf2 delta_d^2 (d in the RBF factor ? -s0 : r1);    g_u[d] -= 2 w_d delta_d sf2 s0,  g_v[d] += the same (d < dU)
// and, through the explicit weights of p_j and of the diagonal term, per differentiated feature
//   Kfg:  g_w[d0 + j] += 2 delta_j F_f(j) W_j
//   Kgg:  g_w[d0 + j] += -2 delta_j sum_l W_jl F_f(j)f(l) p_l - 2 F_f(j) W_jj        g_w[d0 + l] += -2 delta_l sum_j W_jl F_f(j)f(l) p_j
// dU <= d0 (and <= d_split on a Matern kind): a feature with a gradient is none of the differentiated ones and sits in the RBF
// factor, which is what makes its derivative the entry itself times -2 w_d delta_d.  A_3 Q_2 is gpp_matern_d3_times: Q_2 carries two
// factors delta of the Matern features, nothing divides by r = 0 and the term is an exact 0 there (as are A_2's, gpp_matern_d2).
//
// One work-group per tile of GK_T x GK_T pairs, thread (al, bl) = one pair: the A_k are computed once per pair and left in LDS; the
// pair's entries of Kinv are read once (Kfg: 16 consecutive lanes read 16 consecutive columns of one row; Kgg: nd consecutive columns
// per lane, 16 nd per row over the 16 lanes).  Every sum of a tile is added over each wave by a butterfly, the four waves' sums in
// wave order, and written as one record per tile to the handle workspace; g_U / g_Ug rows go to one slot per (tile row or column,
// point), each written exactly once.  Two finish kernels add records and slots in index order: no atomics, two calls agree bitwise.
namespace {

constexpr int GK_T = 16;            // points per tile side
constexpr int GK_TP = GK_T + 1;     // row stride of the per-pair tiles in LDS
constexpr int GK_THREADS = 256;     // one pair per thread
constexpr int GK_MT = GK_T * GK_TP;

struct GkArgs {
  const double* U;
  const double* Ug;
  const double* w;
  const double* sf2;
  const double* alpha;
  const double* Kinv;
  int64_t ldk, N, Mg, tiles_a, n_fg;
  int D, kind, d_split, d0, nd, dU;
  double* rec;    // [tiles][D + 1]
  double* partA;  // [tiles_i][Mg][dU]   g_Ug rows from the Kfg tiles, slot = the tile of function points
  double* partI;  // [tiles_a][N][dU]    g_U rows from the Kfg tiles, slot = the tile of gradient points
  double* partG;  // [tiles_a][Mg][dU]   g_Ug rows from the Kgg tiles, slot = the other tile of the pair
  const int* first;  // SEL: the selection of the gradient points (gpp.h), device pointers; unread otherwise
  const int* dir;
};

__device__ __forceinline__ double gk_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// tile t of the lower triangle in row-major order: (ti, tj), tj <= ti
__device__ __forceinline__ void gk_tile_from_index(int64_t t, int64_t& ti, int64_t& tj) {
  int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  while (r * (r + 1) / 2 > t) --r;
  ti = r;
  tj = t - r * (r + 1) / 2;
}

inline size_t gk_lds_doubles(int D, int nm) {
  return (size_t)2 * GK_T * (D | 1) + D + (size_t)(nm + 1) * GK_MT + (size_t)4 * (D + 1);
}

// SEL: plus, for the 2 GK_T points of a tile, the compact index of each of their nd directions
inline size_t gk_sel_lds_doubles(int D, int nm, int nd) { return gk_lds_doubles(D, nm) + (size_t)GK_T * nd; }

// CH: columns of a Kgg pair's block taken per pass (their column sums stay in registers)
// SEL (gpp_gek_grad_reduce_sel): the rows of a point's observed directions are first[a] .. first[a + 1] - 1 of the gradient block.
// The loops still walk the nd directions, in order and uniformly over a wave (every direction's term is summed over the wave and
// lands in its own g_w slot), and a lane skips the directions its point lacks: cix[point][j] is the compact index of direction j
// or -1, staged once per tile.  What is read of alpha and Kinv, and the sums P_k, Q_m, D_k, run over the observed directions alone,
// in the order of k; with every direction observed the operations are those of the dense instantiation, which is the code it was.
template <bool MAT, int CH, bool SEL>
__device__ __forceinline__ void gk_tile(const GkArgs& p) {
  extern __shared__ __attribute__((aligned(16))) double gk_lds[];
  constexpr int NM = MAT ? 5 : 1;
  const int D = p.D, nd = p.nd, d0 = p.d0, dU = p.dU, Dp = D | 1, nrec = D + 1;
  double* rA = gk_lds;              // [GK_T][Dp] raw rows of the gradient points a
  double* rB = rA + GK_T * Dp;      // [GK_T][Dp] raw rows of the other side: function points (Kfg) or gradient points b (Kgg)
  double* sw = rB + GK_T * Dp;      // [D]
  double* sM = sw + D;              // [NM][GK_T][GK_TP]: A_0 (, A_1, A_2, r, e^-q1 e^-r)
  double* sG = sM + NM * GK_MT;     // [GK_T][GK_TP] sf2 s0 of every pair
  double* wred = sG + GK_MT;        // [4][nrec] the waves' sums
  int* cix = reinterpret_cast<int*>(wred + 4 * nrec);  // SEL: [2 GK_T][nd], side a then side b
  const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
  const int al = t >> 4, bl = t & 15;
  const int64_t blk = blockIdx.x;
  const bool gg = blk >= p.n_fg;
  int64_t ta, tb;
  if (!gg) {
    ta = blk % p.tiles_a;
    tb = blk / p.tiles_a;
  } else {
    gk_tile_from_index(blk - p.n_fg, ta, tb);
  }
  const int64_t a0 = ta * GK_T, b0 = tb * GK_T;
  const double* Ub = gg ? p.Ug : p.U;
  const int64_t nbt = gg ? p.Mg : p.N;
  const int na = (int)min((int64_t)GK_T, p.Mg - a0), nb = (int)min((int64_t)GK_T, nbt - b0);
  const int ds = MAT ? p.d_split : D;  // features below ds belong to the RBF factor
  const double sf2 = *p.sf2;

  for (int d = t; d < D; d += GK_THREADS) sw[d] = p.w[d];
  for (int e = t; e < 4 * nrec; e += GK_THREADS) wred[e] = 0.0;
  // rows beyond the ends are staged as zeros and never read from memory; their pairs are not valid and add nothing
  for (int e = t; e < 2 * GK_T * D; e += GK_THREADS) {
    const int r = e / D, d = e - r * D;
    if (r < GK_T) {
      rA[r * Dp + d] = r < na ? p.Ug[(a0 + r) * D + d] : 0.0;
    } else {
      const int rb = r - GK_T;
      rB[rb * Dp + d] = rb < nb ? Ub[(b0 + rb) * D + d] : 0.0;
    }
  }
  if constexpr (SEL) {
    // one thread per point (the b side only in a Kgg tile): dir is increasing within a point, so one pass fills its nd slots
    if (t < (gg ? 2 * GK_T : GK_T)) {
      const int r = t & (GK_T - 1);
      const bool side_b = t >= GK_T;
      const int64_t pt = (side_b ? b0 : a0) + r;
      int k = 0, k1 = 0;
      if (r < (side_b ? nb : na)) {
        k = p.first[pt];
        k1 = p.first[pt + 1];
      }
      for (int j = 0; j < nd; ++j) {
        const bool has = k < k1 && p.dir[k] == j;
        cix[t * nd + j] = has ? k : -1;
        if (has) ++k;
      }
    }
  }
  __syncthreads();

  const double* xa = rA + al * Dp;
  const double* xb = rB + bl * Dp;
  const int64_t a = a0 + al, b = b0 + bl;
  const bool valid = al < na && bl < nb && (!gg || a >= b);
  double* mine = sM + al * GK_TP + bl;
  {
    const GppExpConsts ec = gpp_exp_consts();
    double q1 = 0.0;
    for (int d = 0; d < ds; ++d) {
      const double df = xa[d] - xb[d];
      q1 = fma(sw[d] * df, df, q1);
    }
    const double e1 = gpp_exp_nonpos(-q1, ec);
    if constexpr (MAT) {
      double q2 = 0.0;
      for (int d = ds; d < D; ++d) {
        const double df = xa[d] - xb[d];
        q2 = fma(sw[d] * df, df, q2);
      }
      const GppMatern h = gpp_matern(p.kind, q2, ec);
      mine[0] = e1 * (h.p * h.er);
      mine[GK_MT] = e1 * (h.dp * h.er);
      mine[2 * GK_MT] = e1 * gpp_matern_d2(p.kind, h);
      mine[3 * GK_MT] = h.r;
      mine[4 * GK_MT] = e1 * h.er;
    } else {
      mine[0] = e1;
    }
  }
  __syncthreads();
  const double A0 = mine[0];
  const double A1 = MAT ? mine[GK_MT] : 0.0, A2 = MAT ? mine[2 * GK_MT] : 0.0;

  const double* __restrict__ alpha = p.alpha;
  const double* __restrict__ Kinv = p.Kinv;
  const double* da = xa + d0;
  const double* db = xb + d0;
  const double* wd = sw + d0;
  const int* ca = cix + al * nd;            // SEL: compact indices of the directions of point a,
  const int* cb = cix + (GK_T + bl) * nd;   //      and in a Kgg tile of point b
  double s0 = 0.0, r1 = 0.0;  // per unit sf2
  if (!gg) {
    double P0 = 0.0, P1 = 0.0;
    const double ab = valid ? alpha[b] : 0.0;
    for (int j = 0; j < nd; ++j) {
      double dir = 0.0;
      const int ka = SEL ? ca[j] : 0;
      if (valid && (!SEL || ka >= 0)) {
        const int64_t r = SEL ? p.N + ka : p.N + a * nd + j;
        const double W = alpha[r] * ab - Kinv[r * p.ldk + b];  // both triangles: 2 x 1/2
        const double dj = da[j] - db[j];
        const double pj = (2.0 * wd[j]) * dj;
        const bool fj = MAT && d0 + j >= ds;
        if (fj) P1 = fma(W, pj, P1);
        else P0 = fma(W, pj, P0);
        dir = (2.0 * dj) * ((fj ? A1 : -A0) * W);
      }
      dir = gk_wave_sum(dir);
      if (lane == 0) wred[wave * nrec + d0 + j] += dir;
    }
    s0 = A1 * P1 - A0 * P0;
    r1 = A2 * P1 - A1 * P0;
  } else {
    double Q0 = 0.0, Q1 = 0.0, Q2 = 0.0, D0 = 0.0, D1 = 0.0;
    const bool self = a == b;
    const double hm = self ? 0.5 : 1.0;  // (1 or 2 triangles) x 1/2
    for (int l0 = 0; l0 < nd; l0 += CH) {
      double cF[CH];
#pragma unroll
      for (int ll = 0; ll < CH; ++ll) cF[ll] = 0.0;
      for (int j = 0; j < nd; ++j) {
        double dir = 0.0;
        const int ka = SEL ? ca[j] : 0;
        if (valid && (!SEL || ka >= 0)) {
          const int64_t r = SEL ? p.N + ka : p.N + a * nd + j;
          const double ar = alpha[r];
          const double dj = da[j] - db[j];
          const double wj2 = 2.0 * wd[j];
          const double pj = wj2 * dj;
          const int fj = (MAT && d0 + j >= ds) ? 1 : 0;
          double rF = 0.0;
#pragma unroll
          for (int ll = 0; ll < CH; ++ll) {
            const int l = l0 + ll;
            const int kb = (SEL && l < nd) ? cb[l] : 0;
            if (l < nd && (!SEL || kb >= 0)) {
              const int64_t c = SEL ? p.N + kb : p.N + b * nd + l;
              const bool flip = self && c > r;  // a point with itself: the block straddles the diagonal
              const double W = hm * (ar * alpha[c] - Kinv[(flip ? c : r) * p.ldk + (flip ? r : c)]);
              const double pl = (2.0 * wd[l]) * (da[l] - db[l]);
              const int m = fj + ((MAT && d0 + l >= ds) ? 1 : 0);
              const double F = m == 0 ? A0 : (m == 1 ? -A1 : A2);
              const double x = W * F;
              rF = fma(x, pl, rF);
              cF[ll] = fma(x, pj, cF[ll]);
              const double wpp = W * (pj * pl);
              if (m == 0) Q0 += wpp;
              else if (m == 1) Q1 += wpp;
              else Q2 += wpp;
              if (l == j) {
                if (fj) D1 = fma(W, wj2, D1);
                else D0 = fma(W, wj2, D0);
                dir = -2.0 * ((fj ? A1 : -A0) * W);
              }
            }
          }
          dir = fma(-2.0 * dj, rF, dir);
        }
        dir = gk_wave_sum(dir);
        if (lane == 0) wred[wave * nrec + d0 + j] += dir;
      }
#pragma unroll
      for (int ll = 0; ll < CH; ++ll) {
        const int l = l0 + ll;
        if (l < nd) {  // (wave-uniform)
          const double v = gk_wave_sum(valid ? (-2.0 * (da[l] - db[l])) * cF[ll] : 0.0);
          if (lane == 0) wred[wave * nrec + d0 + l] += v;
        }
      }
    }
    s0 = -A0 * Q0 + A1 * Q1 - A2 * Q2 + A0 * D0 - A1 * D1;
    if constexpr (MAT) {
      GppMatern h3;
      h3.r = mine[3 * GK_MT];
      h3.er = mine[4 * GK_MT];
      h3.p = h3.dp = 0.0;
      r1 = -A1 * Q0 + A2 * Q1 - gpp_matern_d3_times(p.kind, h3, Q2) + A1 * D0 - A2 * D1;
    }
  }
  if (!valid) s0 = r1 = 0.0;

  for (int d = 0; d < D; ++d) {
    const double df = xa[d] - xb[d];
    const double v = gk_wave_sum((df * df) * ((MAT && d >= ds) ? r1 : -s0));
    if (lane == 0) wred[wave * nrec + d] += v;
  }
  {
    const double v = gk_wave_sum(s0);
    if (lane == 0) wred[wave * nrec + D] += v;
  }
  sG[al * GK_TP + bl] = sf2 * s0;
  __syncthreads();
  if (t < nrec) {
    const double s = ((wred[t] + wred[nrec + t]) + wred[2 * nrec + t]) + wred[3 * nrec + t];
    p.rec[blk * nrec + t] = t < D ? sf2 * s : s;
  }
  for (int e = t; e < GK_T * dU; e += GK_THREADS) {
    const int x = e & (GK_T - 1), d = e / GK_T;
    double rs = 0.0, cs = 0.0;
    for (int k = 0; k < GK_T; ++k) {
      rs = fma(sG[x * GK_TP + k], rA[x * Dp + d] - rB[k * Dp + d], rs);
      cs = fma(sG[k * GK_TP + x], rA[k * Dp + d] - rB[x * Dp + d], cs);
    }
    const double w2 = 2.0 * sw[d];
    const double ga = -(w2 * rs), gb = w2 * cs;
    if (!gg) {
      if (x < na) p.partA[(tb * p.Mg + a0 + x) * dU + d] = ga;
      if (x < nb) p.partI[(ta * p.N + b0 + x) * dU + d] = gb;
    } else if (ta == tb) {
      if (x < na) p.partG[(ta * p.Mg + a0 + x) * dU + d] = ga + gb;
    } else {
      if (x < na) p.partG[(tb * p.Mg + a0 + x) * dU + d] = ga;
      if (x < nb) p.partG[(ta * p.Mg + b0 + x) * dU + d] = gb;
    }
  }
}

template <bool MAT, int CH, bool SEL>
__global__ __launch_bounds__(GK_THREADS) void gpp_gek_grad_tiles(GkArgs p) {
  gk_tile<MAT, CH, SEL>(p);
}

// The strides of gpp_gek_grad_reduce_batched, in doubles: element b reads U + b sU, Ug + b sUg, w + b D, sf2 + b, alpha + b sv and
// Kinv + b sK, keeps its records and slots in the slice b sWs of the workspace and returns g_w + b D, g_sf2 + b, g_U + b N dU and
// g_Ug + b Mg dU
struct GkBatch {
  int64_t sU, sUg, sv, sK, sWs;
};

// the tile of element blockIdx.y
template <bool MAT, int CH, bool SEL>
__global__ __launch_bounds__(GK_THREADS) void gpp_gek_grad_tiles_batched(GkArgs p, GkBatch s) {
  const int64_t b = blockIdx.y;
  p.U += b * s.sU;
  p.Ug += b * s.sUg;
  p.w += b * p.D;
  p.sf2 += b;
  p.alpha += b * s.sv;
  p.Kinv += b * s.sK;
  p.rec += b * s.sWs;
  p.partA += b * s.sWs;
  p.partI += b * s.sWs;
  p.partG += b * s.sWs;
  gk_tile<MAT, CH, SEL>(p);
}

// g_w[q] (q < D) or g_sf2 (q == D) += the tiles' records in index order
__device__ __forceinline__ void gk_finish(const double* __restrict__ rec, int64_t ntiles, int D, double* __restrict__ g_w,
                                          double* __restrict__ g_sf2) {
  __shared__ double red[256];
  const int q = (int)blockIdx.x, nrec = D + 1, tid = (int)threadIdx.x;
  double v = 0.0;
  for (int64_t b = tid; b < ntiles; b += 256) v += rec[b * nrec + q];
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    if (q < D) g_w[q] += red[0];
    else g_sf2[0] += red[0];
  }
}

__global__ __launch_bounds__(256) void gpp_gek_finish(const double* __restrict__ rec, int64_t ntiles, int D, double* __restrict__ g_w,
                                                      double* __restrict__ g_sf2) {
  gk_finish(rec, ntiles, D, g_w, g_sf2);
}

__global__ __launch_bounds__(256) void gpp_gek_finish_batched(const double* __restrict__ rec, int64_t sWs, int64_t ntiles, int D,
                                                              double* __restrict__ g_w, double* __restrict__ g_sf2) {
  const int64_t b = blockIdx.y;
  gk_finish(rec + b * sWs, ntiles, D, g_w + b * D, g_sf2 + b);
}

// g_Ug[e] = the slots of partA, then of partG, in slot order (written); g_U[e] += the slots of partI in slot order
__device__ __forceinline__ void gk_gU_finish(const double* __restrict__ partA, int64_t tiles_i, const double* __restrict__ partG,
                                             const double* __restrict__ partI, int64_t tiles_a, int64_t N, int64_t Mg, int dU,
                                             double* __restrict__ g_U, double* __restrict__ g_Ug) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < Mg * dU) {
    double s = 0.0;
    for (int64_t k = 0; k < tiles_i; ++k) s += partA[k * Mg * dU + e];
    for (int64_t k = 0; k < tiles_a; ++k) s += partG[k * Mg * dU + e];
    g_Ug[e] = s;
  }
  if (e < N * dU) {
    double s = 0.0;
    for (int64_t k = 0; k < tiles_a; ++k) s += partI[k * N * dU + e];
    g_U[e] += s;
  }
}

__global__ __launch_bounds__(256) void gpp_gek_gU_finish(const double* __restrict__ partA, int64_t tiles_i, const double* __restrict__ partG,
                                                         const double* __restrict__ partI, int64_t tiles_a, int64_t N, int64_t Mg, int dU,
                                                         double* __restrict__ g_U, double* __restrict__ g_Ug) {
  gk_gU_finish(partA, tiles_i, partG, partI, tiles_a, N, Mg, dU, g_U, g_Ug);
}

__global__ __launch_bounds__(256) void gpp_gek_gU_finish_batched(const double* __restrict__ partA, int64_t tiles_i,
                                                                 const double* __restrict__ partG, const double* __restrict__ partI,
                                                                 int64_t sWs, int64_t tiles_a, int64_t N, int64_t Mg, int dU,
                                                                 double* __restrict__ g_U, double* __restrict__ g_Ug) {
  const int64_t b = blockIdx.y;
  gk_gU_finish(partA + b * sWs, tiles_i, partG + b * sWs, partI + b * sWs, tiles_a, N, Mg, dU, g_U + b * N * dU, g_Ug + b * Mg * dU);
}

inline int64_t gk_tiles(int64_t n) { return (n + GK_T - 1) / GK_T; }

// one launch for every element of a batch: the same instantiations, the element on the grid's y dimension
template <bool MAT>
void gk_launch_batched(hipStream_t s, const GkArgs& p, int64_t ntiles, const GkBatch& bt, int batch) {
  const dim3 grid((unsigned)ntiles, (unsigned)batch), block(GK_THREADS);
  if (!p.first) {
    const size_t lds = gk_lds_doubles(p.D, MAT ? 5 : 1) * sizeof(double);
    if (p.nd <= 4) hipLaunchKernelGGL((gpp_gek_grad_tiles_batched<MAT, 4, false>), grid, block, lds, s, p, bt);
    else if (p.nd <= 8) hipLaunchKernelGGL((gpp_gek_grad_tiles_batched<MAT, 8, false>), grid, block, lds, s, p, bt);
    else hipLaunchKernelGGL((gpp_gek_grad_tiles_batched<MAT, 16, false>), grid, block, lds, s, p, bt);
  } else {
    const size_t lds = gk_sel_lds_doubles(p.D, MAT ? 5 : 1, p.nd) * sizeof(double);
    if (p.nd <= 4) hipLaunchKernelGGL((gpp_gek_grad_tiles_batched<MAT, 4, true>), grid, block, lds, s, p, bt);
    else if (p.nd <= 8) hipLaunchKernelGGL((gpp_gek_grad_tiles_batched<MAT, 8, true>), grid, block, lds, s, p, bt);
    else hipLaunchKernelGGL((gpp_gek_grad_tiles_batched<MAT, 16, true>), grid, block, lds, s, p, bt);
  }
}

template <bool MAT>
void gk_launch(hipStream_t s, const GkArgs& p, int64_t ntiles) {
  const dim3 grid((unsigned)ntiles), block(GK_THREADS);
  if (!p.first) {
    const size_t lds = gk_lds_doubles(p.D, MAT ? 5 : 1) * sizeof(double);
    if (p.nd <= 4) hipLaunchKernelGGL((gpp_gek_grad_tiles<MAT, 4, false>), grid, block, lds, s, p);
    else if (p.nd <= 8) hipLaunchKernelGGL((gpp_gek_grad_tiles<MAT, 8, false>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((gpp_gek_grad_tiles<MAT, 16, false>), grid, block, lds, s, p);
  } else {
    const size_t lds = gk_sel_lds_doubles(p.D, MAT ? 5 : 1, p.nd) * sizeof(double);
    if (p.nd <= 4) hipLaunchKernelGGL((gpp_gek_grad_tiles<MAT, 4, true>), grid, block, lds, s, p);
    else if (p.nd <= 8) hipLaunchKernelGGL((gpp_gek_grad_tiles<MAT, 8, true>), grid, block, lds, s, p);
    else hipLaunchKernelGGL((gpp_gek_grad_tiles<MAT, 16, true>), grid, block, lds, s, p);
  }
}

}  // namespace

size_t gpp_gek_grad_ws_bytes(int64_t N, int64_t Mg, int D, int dU) {
  if (N < 1 || Mg < 1 || D < 1 || dU < 0) return 0;
  const int64_t ta = gk_tiles(Mg), ti = gk_tiles(N);
  const int64_t ntiles = ta * ti + ta * (ta + 1) / 2;
  return (size_t)(ntiles * (D + 1) + (int64_t)dU * (ti * Mg + ta * N + ta * Mg)) * sizeof(double);
}

// gpp_gek_grad_reduce (first == NULL, q = Mg nd) and gpp_gek_grad_reduce_sel; `shift`: how far the latter's three extra arguments move
// the codes from alpha on
static int gk_run(gpp_handle_t h, const double* U, int64_t N, const double* Ug, int64_t Mg, int D, const double* w, const double* sf2,
                  int kind, int d_split, int d0, int nd, const int* first, const int* dir, int64_t q, const double* alpha,
                  const double* Kinv, int64_t ldk, int dU, double* g_w, double* g_sf2, double* g_U, double* g_Ug, int shift,
                  int batch = 0, const GkBatch* strides = nullptr) {
  if (int rc = dg_check_pair(h, U, N, Ug, Mg, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (Mg * nd > 0x7ffffff0) return -5;
  if (!alpha) return -13 - shift;
  if (!Kinv || !dg_aligned16(Kinv)) return -14 - shift;
  if ((ldk & 1) || ldk < N + q) return -15 - shift;
  // a feature with a gradient is none of the differentiated ones and, on a Matern kind, belongs to the RBF factor
  if (dU < 0 || dU > d0 || (kind != GPP_KIND_RBF && dU > d_split)) return -16 - shift;
  if (!g_w) return -17 - shift;
  if (!g_sf2) return -18 - shift;
  if (dU > 0 && !g_U) return -19 - shift;
  if (dU > 0 && !g_Ug) return -20 - shift;
  const int64_t ta = gk_tiles(Mg), ti = gk_tiles(N);
  const int64_t n_fg = ta * ti, ntiles = n_fg + ta * (ta + 1) / 2;
  if (ntiles >= ((int64_t)1 << 31)) return -3;
  const size_t ws_one = gpp_gek_grad_ws_bytes(N, Mg, D, dU);
  if (strides) {
    // gpp_gek_grad_reduce_batched: one slice of the workspace per element, every stride even (0: shared feature rows)
    if (batch < 1 || batch > 65535) return DG_BAD_BATCH;
    if ((strides->sU & 1) || (strides->sUg & 1) || (strides->sv & 1) || (strides->sK & 1)) return DG_ODD_STRIDE;
    if ((strides->sU != 0 && strides->sU < N * D) || (strides->sUg != 0 && strides->sUg < Mg * D)) return DG_SHORT_STRIDE;
    if (batch > 1 && (strides->sv < N + q || strides->sK < (N + q - 1) * ldk + N + q)) return DG_SHORT_STRIDE;
    if (!h->ws || h->ws_bytes < (size_t)batch * ws_one) return GPP_NO_WORKSPACE;
  } else if (!h->ws || h->ws_bytes < ws_one) {
    return GPP_NO_WORKSPACE;
  }
  double* rec = reinterpret_cast<double*>(h->ws);
  double* partA = rec + ntiles * (D + 1);
  double* partI = partA + (int64_t)dU * ti * Mg;
  double* partG = partI + (int64_t)dU * ta * N;
  GkArgs p{U, Ug, w, sf2, alpha, Kinv, ldk, N, Mg, ta, n_fg, D, kind, d_split, d0, nd, dU, rec, partA, partI, partG, first, dir};
  if (strides) {
    GkBatch bt = *strides;
    bt.sWs = (int64_t)(ws_one / sizeof(double));
    const unsigned nb = (unsigned)batch;
    if (kind == GPP_KIND_RBF) gk_launch_batched<false>(h->stream, p, ntiles, bt, batch);
    else gk_launch_batched<true>(h->stream, p, ntiles, bt, batch);
    if (hipError_t r = hipGetLastError(); r != hipSuccess) return dg_rc(r);
    hipLaunchKernelGGL(gpp_gek_finish_batched, dim3((unsigned)(D + 1), nb), dim3(256), 0, h->stream, rec, bt.sWs, ntiles, D, g_w, g_sf2);
    if (dU > 0) {
      const int64_t rows = (Mg > N ? Mg : N) * dU;
      hipLaunchKernelGGL(gpp_gek_gU_finish_batched, dim3((unsigned)((rows + 255) / 256), nb), dim3(256), 0, h->stream, partA, ti, partG,
                         partI, bt.sWs, ta, N, Mg, dU, g_U, g_Ug);
    }
    return dg_rc(hipGetLastError());
  }
  if (kind == GPP_KIND_RBF) gk_launch<false>(h->stream, p, ntiles);
  else gk_launch<true>(h->stream, p, ntiles);
  if (hipError_t r = hipGetLastError(); r != hipSuccess) return dg_rc(r);
  hipLaunchKernelGGL(gpp_gek_finish, dim3((unsigned)(D + 1)), dim3(256), 0, h->stream, rec, ntiles, D, g_w, g_sf2);
  if (dU > 0) {
    const int64_t rows = (Mg > N ? Mg : N) * dU;
    hipLaunchKernelGGL(gpp_gek_gU_finish, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, h->stream, partA, ti, partG, partI, ta, N, Mg,
                       dU, g_U, g_Ug);
  }
  return dg_rc(hipGetLastError());
}

extern "C" int gpp_gek_grad_reduce(gpp_handle_t h, const double* U, int64_t N, const double* Ug, int64_t Mg, int D, const double* w,
                                   const double* sf2, int kind, int d_split, int d0, int nd, const double* alpha, const double* Kinv,
                                   int64_t ldk, int dU, double* g_w, double* g_sf2, double* g_U, double* g_Ug) {
  return gk_run(h, U, N, Ug, Mg, D, w, sf2, kind, d_split, d0, nd, nullptr, nullptr, Mg * nd, alpha, Kinv, ldk, dU, g_w, g_sf2, g_U,
                g_Ug, 0);
}

extern "C" int gpp_gek_grad_reduce_sel(gpp_handle_t h, const double* U, int64_t N, const double* Ug, int64_t Mg, int D, const double* w,
                                       const double* sf2, int kind, int d_split, int d0, int nd, const int* first, const int* dir,
                                       int64_t q, const double* alpha, const double* Kinv, int64_t ldk, int dU, double* g_w,
                                       double* g_sf2, double* g_U, double* g_Ug) {
  if (int rc = dg_check_pair(h, U, N, Ug, Mg, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (Mg * nd > 0x7ffffff0) return -5;
  if (int rc = dg_check_selection(first, dir, q, Mg, nd)) return rc == 1 ? -14 : -15;
  return gk_run(h, U, N, Ug, Mg, D, w, sf2, kind, d_split, d0, nd, first, dir, q, alpha, Kinv, ldk, dU, g_w, g_sf2, g_U, g_Ug, 3);
}

extern "C" int gpp_gek_grad_reduce_batched(gpp_handle_t h, const double* U, int64_t sU, int64_t N, const double* Ug, int64_t sUg, int64_t Mg,
                                           int D, const double* w, const double* sf2, int kind, int d_split, int d0, int nd,
                                           const int* first, const int* dir, int64_t q, const double* alpha, int64_t sv,
                                           const double* Kinv, int64_t ldk, int64_t sK, int dU, double* g_w, double* g_sf2, double* g_U,
                                           double* g_Ug, int batch) {
  if (int rc = dg_check_pair(h, U, N, Ug, Mg, D, w, sf2, kind, d_split, d0, nd)) return rc;
  if (Mg * nd > 0x7ffffff0) return -5;
  if (int rc = dg_check_selection(first, dir, q, Mg, nd)) return rc == 1 ? -14 : -15;
  const GkBatch bt{sU, sUg, sv, sK, 0};
  return gk_run(h, U, N, Ug, Mg, D, w, sf2, kind, d_split, d0, nd, first, dir, q, alpha, Kinv, ldk, dU, g_w, g_sf2, g_U, g_Ug, 3, batch,
                &bt);
}

// gpp_apply.hip — generated-matrix products for pathwise posterior draws (gpp_kernel_apply, gpp_rff_apply in gpp.h).
//
//   Out[a,s] = beta Out[a,s] + sum_j G[a,j] C[j,s],     G[a,j] = sf2 k(Ua_a, Ub_j; w)                    (kernel)
//                                                       G[a,f] = sqrt(2 sf2 / F) cos(omega_f . Ua_a + b_f) (random features)
// G is never written to memory: a 64 x 32 tile of it is generated in registers from the features staged in LDS, stored to LDS in
// the A-operand layout of gemm_tile's k-contiguous operands ([row][k], padded rows) and multiplied with the staged 32 x 64 chunk of
// C by v_mfma_f64_16x16x4_f64.  No reference counterpart: the reference draws posterior samples only as vectors
// (models/gp_plus.py:985-998, likelihood(self(X)).sample), through the dense predictive covariance.
//
// One 256-thread work-group owns 64 rows of Ua and up to 64 columns of C (further column tiles on blockIdx.y) and walks its share of
// the contracted index in chunks of 32.  A contracted length above AP_SPLIT is cut into ceil(L / AP_SPLIT) pieces on blockIdx.z, each
// of which writes its partial tile to the handle workspace; a finish kernel adds the pieces in their order.  The number of pieces
// depends on the contracted length alone, every output element is the sum of the same terms in the same order wherever its row
// stands in the call, there are no float atomics and no work-group waits for another one: a row's result does not depend on the
// other rows of the call and two launches agree bit for bit.
//
// The gradient with respect to Ua (gpp_kernel_apply_grad, gpp_rff_apply_grad; gpp_apply_grad_tile below), for an upstream Gbar (M x S):
//   g_Ua[a,d] = beta g_Ua[a,d] + sum_j V[a,j] dG[a,j]/dUa[a,d],     V = Gbar C^T  (never written to memory either)
// With the staged values a = sqrt(w) ua, b = sqrt(w) ub, the distance accumulators q1 (RBF dims) and q2 (Matern dims), e1 = exp(-q1)
// and h the Matern factor, dG/dua_d = 2 sqrt(w_d) (a_d - b_d) m_f, where f is the factor feature d belongs to and
//   m_0 = -G = -sf2 e1 h,     m_1 = sf2 e1 h'(q2),     h' = -3 e^-r (Matern 3/2),  -(5/3) (1 + r) e^-r (Matern 5/2)
// (h' is dh/dq2 / 2, formed without a division by r: finite where a row of Ua equals a row of Ub).  For the random features
// dG[a,f]/dua_d = -amp sin(omega_f . ua + b_f) omega_fd.  So with W_f = V o m_f (one per factor)
//   g_Ua[a,d] = 2 sqrt(w_d) (a_d sum_j W_f[a,j] - sum_j W_f[a,j] b[j,d])         (kernel)
//   g_Ua[a,d] = sum_j W[a,j] (omega_jd / 2 pi),     W = -(2 pi amp) V o sin        (random features)
// i.e. two MFMA products per chunk, V = Gbar-tile C-chunk^T (K = S) and W [b | 1] (K = 32), with the generation between them.
#include "gpp_internal.h"

#include <atomic>
#include <type_traits>

typedef double v2d __attribute__((ext_vector_type(2)));
typedef double v4d __attribute__((ext_vector_type(4)));

namespace {

constexpr int AP_TM = 64;        // rows of Ua per work-group
constexpr int AP_TS = 64;        // columns of C per work-group
constexpr int AP_BK = 32;        // chunk of the contracted index
constexpr int AP_LDG = AP_BK + 2;   // [row][k] rows of the generated tile: 272-byte rows (16-byte aligned pairs)
constexpr int AP_LDC = AP_TS + 16;  // [k][col] rows of the staged chunk of C: the k rows of a fragment read fall in different bank halves
constexpr int AP_DMAX = 64;
constexpr int64_t AP_SPLIT = 2048;  // longest contraction one work-group walks

constexpr size_t ap_lds_bytes(int D) {
  return ((size_t)D * AP_TM + (size_t)D * AP_BK + AP_BK + 2 * AP_DMAX + (size_t)AP_TM * AP_LDG + (size_t)AP_BK * AP_LDC) * sizeof(double);
}

// ---- cos(2 pi r) for |r| <= 1/2 (r in turns) ---------------------------------------------------------------------------------
// a = |r|; above a quarter turn cos(2 pi a) = -cos(2 pi (1/2 - a)) with 1/2 - a exact, so x = 2 pi a' lies in [0, pi/2]; there the
// Taylor polynomial of degree 22 in x (11 Horner steps in x^2, truncation (pi/2)^24 / 24! = 8e-20).  No table, no branches, no
// scratch.  Absolute error <= 4 * 2^-53 (x carries 1.5 * 2^-53 relative, i.e. <= 1.5 * 2^-53 x sin x <= 2.4 * 2^-53 in the value; the
// Horner steps add less than 1.5 * 2^-53: the terms alternate and the largest is x^2 / 2 <= 1.24) — measured 2.8 * 2^-53 over
// 4 10^7 arguments against the long double library cosine in a one-off host build of this function; tests/test_pathwise_host.py
// re-evaluates the same coefficients (read from this file) with exact fused multiply-adds and holds them to the stated bound.  The coefficients stay in SGPRs like gpp_exp_consts'.
struct GppCosConsts {
  double two_pi, c[11];
};
__device__ __forceinline__ GppCosConsts gpp_cos_consts() {
  GppCosConsts k = {6.28318530717958647693e+00,
                    {-8.89679139245057328675e-22,   // -1/22!
                     4.11031762331216485648e-19,    //  1/20!
                     -1.56192069685862264546e-16,   // -1/18!
                     4.77947733238738529744e-14,    //  1/16!
                     -1.14707455977297247139e-11,   // -1/14!
                     2.08767569878680989792e-09,    //  1/12!
                     -2.75573192239858906526e-07,   // -1/10!
                     2.48015873015873015873e-05,    //  1/8!
                     -1.38888888888888888889e-03,   // -1/6!
                     4.16666666666666666667e-02,    //  1/4!
                     -0.5}};
  asm volatile("" : "+s"(k.two_pi));
#pragma unroll
  for (int i = 0; i < 10; ++i) asm volatile("" : "+s"(k.c[i]));
  return k;
}
__device__ __forceinline__ double gpp_cos_turns(double r, const GppCosConsts& k) {
  const double a = __builtin_fabs(r);
  const bool flip = a > 0.25;
  const double x = (flip ? 0.5 - a : a) * k.two_pi;
  const double z = x * x;
  double p = k.c[0];
#pragma unroll
  for (int i = 1; i < 11; ++i) p = __builtin_fma(p, z, k.c[i]);
  p = __builtin_fma(p, z, 1.0);
  return flip ? -p : p;
}

// ---- generators: what turns (a row of Ua, a row of the second operand) into an entry of G ------------------------------------
// scale_a / scale_b: the factor of feature d as it is staged in LDS;  NACC accumulators per entry, started by init(extra) where
// `extra` is the staged per-column scalar (the phase of a random feature), advanced by step() for every d, turned into G by value().
template <bool MAT>
struct KernelGen {
  static constexpr int NACC = MAT ? 2 : 1;
  static constexpr bool HAS_EXTRA = false;
  const double* w;
  double sf2;
  int kind, d_split;
  GppExpConsts ec;
  template <class A>
  __device__ __forceinline__ void setup(const A& p) {
    w = p.w;
    sf2 = *p.sf2;
    kind = p.kind;
    d_split = p.d_split;
    ec = gpp_exp_consts();
  }
  __device__ __forceinline__ double scale_a(int d) const { return sqrt(w[d]); }
  __device__ __forceinline__ double scale_b(int d) const { return sqrt(w[d]); }
  __device__ __forceinline__ double scale_extra() const { return 0.0; }
  __device__ __forceinline__ void init(double (&acc)[NACC], double) const {
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  }
  // (second == true: feature d belongs to the Matern factor; uniform in the work-group)
  __device__ __forceinline__ void step(double (&acc)[NACC], double ua, double ub, bool second) const {
    const double df = ua - ub;
    if (MAT && second) acc[NACC - 1] = fma(df, df, acc[NACC - 1]);
    else acc[0] = fma(df, df, acc[0]);
  }
  __device__ __forceinline__ bool second(int d) const { return MAT && kind != 0 && d >= d_split; }
  __device__ __forceinline__ double value(const double (&acc)[NACC]) const {
    if constexpr (MAT) return sf2 * gpp_kernel_value(kind, acc[0], acc[1], ec);
    else return sf2 * gpp_exp_nonpos(-acc[0], ec);
  }
  // gradient: one ones-column per factor gives the row sums of W_f; m_f as in the file header
  static constexpr int NROWSUM = NACC;
  __device__ __forceinline__ void dvalue(const double (&acc)[NACC], double (&m)[NACC]) const {
    const double e1 = sf2 * gpp_exp_nonpos(-acc[0], ec);
    if constexpr (MAT) {
      const GppMatern h = gpp_matern(kind, acc[1], ec);
      m[0] = -(e1 * (h.p * h.er));
      m[1] = e1 * (h.dp * h.er);
    } else {
      m[0] = -e1;
    }
  }
  // g = out_scale (a_d rowsum_f - (W_f b)[d])
  __device__ __forceinline__ double finish(double wb, double a, double rowsum, double scale_a_d) const {
    return (2.0 * scale_a_d) * fma(a, rowsum, -wb);
  }
};

struct RffGen {
  static constexpr int NACC = 1;
  static constexpr bool HAS_EXTRA = true;
  double amp;  // sqrt(2 sf2 / F)
  GppCosConsts cc;
  template <class A>
  __device__ __forceinline__ void setup(const A& p) {
    amp = sqrt(2.0 * *p.sf2 / p.nfeat);
    cc = gpp_cos_consts();
  }
  // the phase in TURNS: t = sum_d (omega_d / 2 pi) u_d + b / 2 pi, r = t - rint(t) (exact), cos(2 pi r)
  __device__ __forceinline__ double scale_a(int) const { return 1.0; }
  __device__ __forceinline__ double scale_b(int) const { return 1.59154943091895335769e-01; }
  __device__ __forceinline__ double scale_extra() const { return 1.59154943091895335769e-01; }
  __device__ __forceinline__ void init(double (&acc)[1], double phase) const { acc[0] = phase; }
  __device__ __forceinline__ void step(double (&acc)[1], double ua, double ub, bool) const { acc[0] = fma(ua, ub, acc[0]); }
  __device__ __forceinline__ bool second(int) const { return false; }
  __device__ __forceinline__ double value(const double (&acc)[1]) const {
    const double t = acc[0];
    return amp * gpp_cos_turns(t - __builtin_rint(t), cc);
  }
  // gradient: sin(2 pi r) = sign(r) cos(2 pi (|r| - 1/4)), the cosine's argument within a quarter turn (|r| - 1/4 is exact from
  // |r| = 1/8 on and errs by at most 2^-56 turns below); the staged frequencies are omega / 2 pi, so 2 pi goes into W
  static constexpr int NROWSUM = 0;
  __device__ __forceinline__ void dvalue(const double (&acc)[1], double (&m)[1]) const {
    const double t = acc[0];
    const double r = t - __builtin_rint(t);
    const double c = gpp_cos_turns(__builtin_fabs(r) - 0.25, cc);
    m[0] = -(amp * cc.two_pi) * (r < 0.0 ? -c : c);
  }
  __device__ __forceinline__ double finish(double wb, double, double, double) const { return wb; }
};

struct ApplyArgs {
  const double* Ua;     // M x D
  const double* Ub;     // L x D: training features, or Omega
  const double* extra;  // L (the phases) or null
  const double* w;      // D or null
  const double* sf2;
  const double* C;      // L x S, ldc
  double* Out;          // M x S, ldo — or the partial tiles [piece][M][S] when pieces > 1
  int64_t M, L, ldc, ldo;
  int D, S, kind, d_split, pieces;
  double beta, nfeat;
};

// (three waves per SIMD asked of the register allocator: left alone it spends 212-224 VGPRs on the eight exponential / cosine
//  chains of the generation phase, i.e. two work-groups per CU; with the request 120-124, no scratch)
template <class GEN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void gpp_apply_tile(const ApplyArgs p) {
  extern __shared__ __attribute__((aligned(16))) double ap_smem[];
  const int D = p.D;
  double* sa = ap_smem;                       // [d][64 rows of Ua], scaled
  double* sb = sa + (size_t)D * AP_TM;        // [d][32 rows of the second operand], scaled
  double* sx = sb + (size_t)D * AP_BK;        // [32] per-column scalars
  double* sw = sx + AP_BK;                    // [2][AP_DMAX] the staging factors of feature d: of Ua, of the second operand
  double* sg = sw + 2 * AP_DMAX;              // [64 rows][AP_LDG] generated tile
  double* sc = sg + (size_t)AP_TM * AP_LDG;   // [32 k][AP_LDC] chunk of C

  GEN gen;
  gen.setup(p);

  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * AP_TM;
  const int s0 = blockIdx.y * AP_TS;
  // this work-group's piece of the contracted index: [k0, k1), piece boundaries at multiples of AP_SPLIT
  const int64_t k0 = (int64_t)blockIdx.z * AP_SPLIT;
  const int64_t k1 = p.pieces > 1 ? (k0 + AP_SPLIT < p.L ? k0 + AP_SPLIT : p.L) : p.L;
  double* __restrict__ Out = p.Out + (p.pieces > 1 ? (int64_t)blockIdx.z * p.M * p.ldo : 0);
  const double beta = p.pieces > 1 ? 0.0 : p.beta;

  if (tid < D) {
    sw[tid] = gen.scale_a(tid);
    sw[AP_DMAX + tid] = gen.scale_b(tid);
  }
  __syncthreads();
  for (int e = tid; e < D * AP_TM; e += 256) {
    const int r = e / D, d = e - r * D;  // consecutive threads read consecutive addresses of a row
    sa[d * AP_TM + r] = (i0 + r < p.M) ? p.Ua[(i0 + r) * D + d] * sw[d] : 0.0;
  }

  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int ty = tid >> 4, tx = tid & 15;  // generation: rows 4 ty .. 4 ty + 3, columns 2 tx, 2 tx + 1 of the chunk
  const int nb = min(4, (p.S - s0 + 15) >> 4);  // 16-column blocks of this tile that hold a column of C (uniform)

  v4d acc4[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc4[b] = (v4d){0.0, 0.0, 0.0, 0.0};

  for (int64_t kb = k0; kb < k1; kb += AP_BK) {
    __syncthreads();  // the previous chunk's LDS reads are done (and, the first time, sa is complete)
    for (int e = tid; e < D * AP_BK; e += 256) {
      const int r = e / D, d = e - r * D;
      sb[d * AP_BK + r] = (kb + r < k1) ? p.Ub[(kb + r) * D + d] * sw[AP_DMAX + d] : 0.0;
    }
    if (GEN::HAS_EXTRA && tid < AP_BK) sx[tid] = (kb + tid < k1) ? p.extra[kb + tid] * gen.scale_extra() : 0.0;
#pragma unroll
    for (int i = 0; i < AP_BK * AP_TS / 256; ++i) {
      const int e = tid + 256 * i;
      const int k = e >> 6, c = e & 63;
      const bool ok = (kb + k < k1) & (s0 + c < p.S);
      sc[k * AP_LDC + c] = ok ? p.C[(kb + k) * p.ldc + s0 + c] : 0.0;
    }
    __syncthreads();

    {  // generate G[4 ty + a][2 tx + b]
      double acc[4][2][GEN::NACC];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const double x = GEN::HAS_EXTRA ? sx[2 * tx + b] : 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) gen.init(acc[a][b], x);
      }
      for (int d = 0; d < D; ++d) {
        const v2d a01 = reinterpret_cast<const v2d*>(sa + d * AP_TM + 4 * ty)[0];
        const v2d a23 = reinterpret_cast<const v2d*>(sa + d * AP_TM + 4 * ty)[1];
        const v2d b01 = *reinterpret_cast<const v2d*>(sb + d * AP_BK + 2 * tx);
        const double ua[4] = {a01.x, a01.y, a23.x, a23.y}, ub[2] = {b01.x, b01.y};
        const bool second = gen.second(d);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) gen.step(acc[a][b], ua[a], ub[b], second);
      }
      const bool ok0 = kb + 2 * tx < k1, ok1 = kb + 2 * tx + 1 < k1;  // entries past the contracted length are exact zeros
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double g0 = gen.value(acc[a][0]), g1 = gen.value(acc[a][1]);
        const v2d g = {ok0 ? g0 : 0.0, ok1 ? g1 : 0.0};
        *reinterpret_cast<v2d*>(sg + (4 * ty + a) * AP_LDG + 2 * tx) = g;
      }
    }
    __syncthreads();

    // the wave's 16 rows x 64 columns: lane (i = l & 15, k = l >> 4) supplies G[row i][k] and C[k][col i] (gpp_gemm.hip)
    const double* ga = sg + (wave * 16 + li) * AP_LDG + lk;
    const double* cb = sc + lk * AP_LDC + li;
    // one straight-line body per count of live column blocks (a uniform switch): a test around every MFMA puts each in a basic
    // block of its own, behind a wait for its own fragment read
    auto products = [&](auto nbc) {
      constexpr int NB = decltype(nbc)::value;
#pragma unroll
      for (int kk = 0; kk < AP_BK / 4; ++kk) {
        const double af = ga[4 * kk];
        double bf[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) bf[b] = cb[4 * kk * AP_LDC + 16 * b];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc4[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf[b], acc4[b], 0, 0, 0);
      }
    };
    if (nb == 4) products(std::integral_constant<int, 4>{});
    else if (nb == 3) products(std::integral_constant<int, 3>{});
    else if (nb == 2) products(std::integral_constant<int, 2>{});
    else products(std::integral_constant<int, 1>{});
  }

  // element v of acc4[b]: row wave * 16 + 4 v + (l >> 4), column 16 b + (l & 15)
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int s = s0 + 16 * b + li;
    if (s >= p.S) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t i = i0 + wave * 16 + 4 * v + lk;
      if (i >= p.M) continue;
      double* o = Out + i * p.ldo + s;
      double x = acc4[b][v];
      if (beta != 0.0) x = fma(beta, *o, x);
      *o = x;
    }
  }
}

// Out[i][s] = beta Out[i][s] + sum over the pieces, in their order, of part[piece][i][s]
__global__ __launch_bounds__(256) void gpp_apply_finish(const double* __restrict__ part, int pieces, int64_t M, int S, double beta,
                                                        double* __restrict__ Out, int64_t ldo) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * S) return;
  const int64_t i = e / S;
  const int s = (int)(e - i * S);
  double x = part[e];
  for (int q = 1; q < pieces; ++q) x += part[(int64_t)q * M * S + e];
  double* o = Out + i * ldo + s;
  if (beta != 0.0) x = fma(beta, *o, x);
  *o = x;
}

template <class K>
hipError_t ap_lds_optin(K kern, std::atomic<bool>* done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev >= 0 && dev < 64 && done[dev]) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ap_lds_bytes(AP_DMAX));
  if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
  return e;
}

template <class GEN>
hipError_t ap_launch(hipStream_t s, ApplyArgs a, void* ws, size_t ws_bytes) {
  static std::atomic<bool> done[64];  // more than 48 KiB of dynamic LDS (D > 19 features) needs the opt-in, once per device
  if (ap_lds_bytes(a.D) > 48 * 1024)
    if (hipError_t e = ap_lds_optin(gpp_apply_tile<GEN>, done); e != hipSuccess) return e;
  const int pieces = gpp_apply_pieces(a.L);
  const int64_t tiles_m = (a.M + AP_TM - 1) / AP_TM;
  const int tiles_s = (a.S + AP_TS - 1) / AP_TS;
  if (tiles_m > 0x7fffffff || tiles_s > 65535 || pieces > 65535) return hipErrorInvalidValue;
  a.pieces = pieces;
  double* out = a.Out;
  const int64_t ldo = a.ldo;
  if (pieces > 1) {
    if (!ws || ws_bytes < (size_t)pieces * a.M * a.S * sizeof(double)) return hipErrorInvalidValue;  // (checked by the caller)
    a.Out = static_cast<double*>(ws);
    a.ldo = a.S;
  }
  hipLaunchKernelGGL((gpp_apply_tile<GEN>), dim3((unsigned)tiles_m, (unsigned)tiles_s, (unsigned)pieces), dim3(256),
                     ap_lds_bytes(a.D), s, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (pieces > 1) {
    const int64_t n = a.M * a.S;
    hipLaunchKernelGGL(gpp_apply_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<const double*>(ws), pieces,
                       a.M, a.S, a.beta, out, ldo);
    return hipGetLastError();
  }
  return hipSuccess;
}

// ---- the gradient with respect to Ua ---------------------------------------------------------------------------------------------
constexpr int AG_LDV = AP_TS + 2;  // [row][s] rows of the staged tile of Gbar and chunk of C: 528-byte rows, as AP_LDG's 272 (A-operand reads)
constexpr int AG_NB = (AP_DMAX + 2 + 15) / 16;  // most 16-column blocks of [b | 1]

struct ApplyGradArgs {
  const double* Ua;     // M x D
  const double* Ub;     // L x D: training features, or Omega
  const double* extra;  // L (the phases) or null
  const double* w;      // D or null
  const double* sf2;
  const double* C;      // L x S, ldc
  const double* Gbar;   // M x S, ldg
  double* Out;          // M x D, ldo — or the partial tiles [piece][M][D] when pieces > 1
  int64_t M, L, ldc, ldg, ldo;
  int D, S, kind, d_split, pieces;
  double beta, nfeat;
};

template <class GEN>
constexpr size_t ag_lds_bytes(int D) {
  return ((size_t)D * AP_TM + (size_t)16 * ((D + GEN::NROWSUM + 15) / 16) * AP_LDG + AP_BK + 2 * AP_DMAX + (size_t)AP_TM * AG_LDV +
          (size_t)AP_BK * AG_LDV + (size_t)GEN::NACC * AP_TM * AP_LDG) * sizeof(double);
}

// where row r of the tile stands in sa: the four rows 16 wave + 4 v + k (v = 0..3) a lane holds of an accumulator are adjacent
__device__ __forceinline__ int ag_row_slot(int r) { return (r & 48) | ((r & 3) << 2) | ((r >> 2) & 3); }

// One 256-thread work-group owns 64 rows of Ua and all D columns of the gradient, walks all S columns of Gbar / C in blocks of 64
// inside each chunk of 32 of the contracted index, and its piece of the contracted index as gpp_apply_tile does.
template <class GEN>
__global__ __launch_bounds__(256) void gpp_apply_grad_tile(const ApplyGradArgs p) {
  extern __shared__ __attribute__((aligned(16))) double ag_smem[];
  constexpr int NF = GEN::NACC;      // factors of G: one W each
  constexpr int NRS = GEN::NROWSUM;  // ones-columns behind the D feature columns of the second operand
  constexpr bool MAT = NF > 1;
  const int D = p.D, S = p.S;
  const int nd = (D + NRS + 15) >> 4;  // 16-column blocks of [b | 1] (uniform)
  double* sa = ag_smem;                              // [d][64 rows of Ua], scaled, rows at ag_row_slot
  double* sb = sa + (size_t)D * AP_TM;               // [16 nd][AP_LDG]: rows d < D the chunk of the second operand, scaled; then the ones-rows; zeros
  double* sx = sb + (size_t)16 * nd * AP_LDG;        // [32] per-column scalars
  double* sw = sx + AP_BK;                           // [2][AP_DMAX] the staging factors of feature d
  double* sg = sw + 2 * AP_DMAX;                     // [64 rows][AG_LDV] block of Gbar's tile
  double* sc = sg + (size_t)AP_TM * AG_LDV;          // [32 j][AG_LDV] block of the chunk of C, as it lies in memory
  double* sv = sc + (size_t)AP_BK * AG_LDV;          // [NF][64 rows][AP_LDG] W_f

  GEN gen;
  gen.setup(p);

  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * AP_TM;
  const int64_t k0 = (int64_t)blockIdx.z * AP_SPLIT;
  const int64_t k1 = p.pieces > 1 ? (k0 + AP_SPLIT < p.L ? k0 + AP_SPLIT : p.L) : p.L;
  double* __restrict__ Out = p.Out + (p.pieces > 1 ? (int64_t)blockIdx.z * p.M * p.ldo : 0);
  const double beta = p.pieces > 1 ? 0.0 : p.beta;

  if (tid < D) {
    sw[tid] = gen.scale_a(tid);
    sw[AP_DMAX + tid] = gen.scale_b(tid);
  }
  for (int e = D * AP_LDG + tid; e < 16 * nd * AP_LDG; e += 256) sb[e] = (e / AP_LDG - D < NRS) ? 1.0 : 0.0;
  __syncthreads();
  for (int e = tid; e < D * AP_TM; e += 256) {
    const int r = e / D, d = e - r * D;
    sa[d * AP_TM + ag_row_slot(r)] = (i0 + r < p.M) ? p.Ua[(i0 + r) * D + d] * sw[d] : 0.0;
  }

  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;

  // does block b of [b | 1] hold a column of factor f (uniform), and is column c one (per lane)?
  auto block_has = [&](int b, int f) {
    if (!MAT) return true;
    if (f == 0) return 16 * b < p.d_split || (D >> 4) == b;
    return (16 * b + 15 >= p.d_split && 16 * b < D) || ((D + 1) >> 4) == b;
  };
  auto column_of = [&](int c, int f) {
    if (!MAT) return true;
    return c < D ? (c >= p.d_split) == (f == 1) : c == D + f;
  };

  v4d gacc[AG_NB];
#pragma unroll
  for (int b = 0; b < AG_NB; ++b) gacc[b] = (v4d){0.0, 0.0, 0.0, 0.0};

  for (int64_t kb = k0; kb < k1; kb += AP_BK) {
    // V (64 x 32) = Gbar-tile C-chunk^T: element v of vacc[b] is row wave * 16 + 4 v + (l >> 4), column 16 b + (l & 15) of the chunk
    v4d vacc[2] = {(v4d){0.0, 0.0, 0.0, 0.0}, (v4d){0.0, 0.0, 0.0, 0.0}};
    for (int s0 = 0; s0 < S; s0 += AP_TS) {
      __syncthreads();  // the reads of what is staged next are done (and, the first time, sa and sb's constant rows are complete)
      if (s0 == 0) {
        for (int e = tid; e < D * AP_BK; e += 256) {
          const int r = e / D, d = e - r * D;
          sb[d * AP_LDG + r] = (kb + r < k1) ? p.Ub[(kb + r) * D + d] * sw[AP_DMAX + d] : 0.0;
        }
        if (GEN::HAS_EXTRA && tid < AP_BK) sx[tid] = (kb + tid < k1) ? p.extra[kb + tid] * gen.scale_extra() : 0.0;
      }
      if (S > AP_TS || kb == k0) {  // Gbar's tile stays when it is one block
#pragma unroll
        for (int i = 0; i < AP_TM * AP_TS / 256; ++i) {
          const int e = tid + 256 * i;
          const int r = e >> 6, c = e & 63;
          const bool ok = (i0 + r < p.M) & (s0 + c < S);
          sg[r * AG_LDV + c] = ok ? p.Gbar[(i0 + r) * p.ldg + s0 + c] : 0.0;
        }
      }
#pragma unroll
      for (int i = 0; i < AP_BK * AP_TS / 256; ++i) {
        const int e = tid + 256 * i;
        const int k = e >> 6, c = e & 63;
        const bool ok = (kb + k < k1) & (s0 + c < S);
        sc[k * AG_LDV + c] = ok ? p.C[(kb + k) * p.ldc + s0 + c] : 0.0;
      }
      __syncthreads();
      // lane (i = l & 15, k = l >> 4) supplies Gbar[row i][s = k] and C[j = i][s = k]: both row reads of a [..][AG_LDV] image
      const int nk = (min(AP_TS, S - s0) + 3) >> 2;
      const double* ga = sg + (wave * 16 + li) * AG_LDV + lk;
      const double* cb = sc + li * AG_LDV + lk;
      for (int kk = 0; kk < nk; ++kk) {
        const double af = ga[4 * kk], b0 = cb[4 * kk], b1 = cb[16 * AG_LDV + 4 * kk];
        vacc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, b0, vacc[0], 0, 0, 0);
        vacc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, b1, vacc[1], 0, 0, 0);
      }
    }

    {  // W_f = V o m_f at the 4 x 2 entries this lane holds of V
      double acc[4][2][NF];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const double x = GEN::HAS_EXTRA ? sx[16 * b + li] : 0.0;
#pragma unroll
        for (int v = 0; v < 4; ++v) gen.init(acc[v][b], x);
      }
      for (int d = 0; d < D; ++d) {
        const v2d a01 = reinterpret_cast<const v2d*>(sa + d * AP_TM + 16 * wave + 4 * lk)[0];
        const v2d a23 = reinterpret_cast<const v2d*>(sa + d * AP_TM + 16 * wave + 4 * lk)[1];
        const double ua[4] = {a01.x, a01.y, a23.x, a23.y}, ub[2] = {sb[d * AP_LDG + li], sb[d * AP_LDG + 16 + li]};
        const bool second = gen.second(d);
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
          for (int b = 0; b < 2; ++b) gen.step(acc[v][b], ua[v], ub[b], second);
      }
      const bool ok[2] = {kb + li < k1, kb + 16 + li < k1};  // entries past the contracted length are exact zeros
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          double m[NF];
          gen.dvalue(acc[v][b], m);
#pragma unroll
          for (int f = 0; f < NF; ++f)
            sv[(f * AP_TM + wave * 16 + 4 * v + lk) * AP_LDG + 16 * b + li] = ok[b] ? vacc[b][v] * m[f] : 0.0;
        }
    }
    __syncthreads();

    // gacc (64 x 16 nd) += W_f [b | 1]: lane (i, k) supplies W_f[row i][j = k] and sb[column i][j = k]
    const double* wa = sv + (wave * 16 + li) * AP_LDG + lk;
    const double* bb = sb + li * AP_LDG + lk;
#pragma unroll
    for (int b = 0; b < AG_NB; ++b) {
      if (b >= nd) continue;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (!block_has(b, f)) continue;
        const bool mine = column_of(16 * b + li, f);
#pragma unroll
        for (int kk = 0; kk < AP_BK / 4; ++kk) {
          const double af = wa[f * AP_TM * AP_LDG + 4 * kk];
          double bf = bb[16 * b * AP_LDG + 4 * kk];
          if (MAT) bf = mine ? bf : 0.0;
          gacc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, gacc[b], 0, 0, 0);
        }
      }
    }
  }

  // element v of gacc[b]: row wave * 16 + 4 v + (l >> 4), column 16 b + (l & 15); the row sums of W_f stand in column D + f
  double rs[NRS > 0 ? NRS : 1][4];
#pragma unroll
  for (int f = 0; f < NRS; ++f)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      double x = 0.0;
#pragma unroll
      for (int b = 0; b < AG_NB; ++b) x = ((D + f) >> 4) == b ? gacc[b][v] : x;
      rs[f][v] = __shfl(x, (lane & 48) | ((D + f) & 15));
    }
#pragma unroll
  for (int b = 0; b < AG_NB; ++b) {
    const int d = 16 * b + li;
    if (d >= D) continue;
    const int f = gen.second(d) ? NF - 1 : 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int64_t i = i0 + wave * 16 + 4 * v + lk;
      if (i >= p.M) continue;
      double rowsum = 0.0;
      if constexpr (NRS > 0) rowsum = (MAT && f) ? rs[NRS - 1][v] : rs[0][v];
      double x = gen.finish(gacc[b][v], sa[d * AP_TM + 16 * wave + 4 * lk + v], rowsum, sw[d]);
      double* o = Out + i * p.ldo + d;
      if (beta != 0.0) x = fma(beta, *o, x);
      *o = x;
    }
  }
}

template <class GEN>
hipError_t ag_launch(hipStream_t s, ApplyGradArgs a, void* ws, size_t ws_bytes) {
  static std::atomic<bool> done[64];  // more than 48 KiB of dynamic LDS needs the opt-in, once per device
  if (ag_lds_bytes<GEN>(a.D) > 48 * 1024) {
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    if (!(dev >= 0 && dev < 64 && done[dev])) {
      if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gpp_apply_grad_tile<GEN>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)ag_lds_bytes<GEN>(AP_DMAX));
          e != hipSuccess)
        return e;
      if (dev >= 0 && dev < 64) done[dev] = true;
    }
  }
  const int pieces = gpp_apply_pieces(a.L);
  const int64_t tiles_m = (a.M + AP_TM - 1) / AP_TM;
  if (tiles_m > 0x7fffffff || pieces > 65535) return hipErrorInvalidValue;
  a.pieces = pieces;
  double* out = a.Out;
  const int64_t ldo = a.ldo;
  if (pieces > 1) {
    if (!ws || ws_bytes < (size_t)pieces * a.M * a.D * sizeof(double)) return hipErrorInvalidValue;  // (checked by the caller)
    a.Out = static_cast<double*>(ws);
    a.ldo = a.D;
  }
  hipLaunchKernelGGL((gpp_apply_grad_tile<GEN>), dim3((unsigned)tiles_m, 1, (unsigned)pieces), dim3(256), ag_lds_bytes<GEN>(a.D), s, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (pieces > 1) {  // the pieces in their order, as the forward's: gpp_apply_finish with S := D
    const int64_t n = a.M * a.D;
    hipLaunchKernelGGL(gpp_apply_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<const double*>(ws), pieces,
                       a.M, a.D, a.beta, out, ldo);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace

int gpp_apply_pieces(int64_t L) { return L <= AP_SPLIT ? 1 : (int)((L + AP_SPLIT - 1) / AP_SPLIT); }

size_t gpp_apply_ws_bytes(int64_t L, int64_t M, int S) {
  const int pieces = gpp_apply_pieces(L);
  return pieces > 1 ? (size_t)pieces * (size_t)M * (size_t)S * sizeof(double) : 0;
}

hipError_t gpp_launch_kernel_apply(hipStream_t s, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                                   const double* sf2, int kind, int d_split, const double* C, int64_t ldc, int S, double beta,
                                   double* Out, int64_t ldo, void* ws, size_t ws_bytes) {
  ApplyArgs a{};
  a.Ua = Ua; a.Ub = Ub; a.extra = nullptr; a.w = w; a.sf2 = sf2; a.C = C; a.Out = Out;
  a.M = M; a.L = N; a.ldc = ldc; a.ldo = ldo;
  a.D = D; a.S = S; a.kind = kind; a.d_split = d_split;
  a.beta = beta; a.nfeat = 0.0;
  if (kind == 0) return ap_launch<KernelGen<false>>(s, a, ws, ws_bytes);
  return ap_launch<KernelGen<true>>(s, a, ws, ws_bytes);
}

hipError_t gpp_launch_rff_apply(hipStream_t s, const double* Ua, int64_t M, int D, const double* Omega, const double* phase, int64_t F,
                                const double* sf2, const double* Theta, int64_t ldt, int S, double beta, double* Out, int64_t ldo,
                                void* ws, size_t ws_bytes) {
  ApplyArgs a{};
  a.Ua = Ua; a.Ub = Omega; a.extra = phase; a.w = nullptr; a.sf2 = sf2; a.C = Theta; a.Out = Out;
  a.M = M; a.L = F; a.ldc = ldt; a.ldo = ldo;
  a.D = D; a.S = S; a.kind = 0; a.d_split = 0;
  a.beta = beta; a.nfeat = (double)F;
  return ap_launch<RffGen>(s, a, ws, ws_bytes);
}

hipError_t gpp_launch_kernel_apply_grad(hipStream_t s, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w,
                                        const double* sf2, int kind, int d_split, const double* C, int64_t ldc, int S,
                                        const double* Gbar, int64_t ldg, double beta, double* g_Ua, int64_t ldu, void* ws,
                                        size_t ws_bytes) {
  ApplyGradArgs a{};
  a.Ua = Ua; a.Ub = Ub; a.extra = nullptr; a.w = w; a.sf2 = sf2; a.C = C; a.Gbar = Gbar; a.Out = g_Ua;
  a.M = M; a.L = N; a.ldc = ldc; a.ldg = ldg; a.ldo = ldu;
  a.D = D; a.S = S; a.kind = kind; a.d_split = d_split;
  a.beta = beta; a.nfeat = 0.0;
  if (kind == 0) return ag_launch<KernelGen<false>>(s, a, ws, ws_bytes);
  return ag_launch<KernelGen<true>>(s, a, ws, ws_bytes);
}

hipError_t gpp_launch_rff_apply_grad(hipStream_t s, const double* Ua, int64_t M, int D, const double* Omega, const double* phase,
                                     int64_t F, const double* sf2, const double* Theta, int64_t ldt, int S, const double* Gbar,
                                     int64_t ldg, double beta, double* g_Ua, int64_t ldu, void* ws, size_t ws_bytes) {
  ApplyGradArgs a{};
  a.Ua = Ua; a.Ub = Omega; a.extra = phase; a.w = nullptr; a.sf2 = sf2; a.C = Theta; a.Gbar = Gbar; a.Out = g_Ua;
  a.M = M; a.L = F; a.ldc = ldt; a.ldg = ldg; a.ldo = ldu;
  a.D = D; a.S = S; a.kind = 0; a.d_split = 0;
  a.beta = beta; a.nfeat = (double)F;
  return ag_launch<RffGen>(s, a, ws, ws_bytes);
}

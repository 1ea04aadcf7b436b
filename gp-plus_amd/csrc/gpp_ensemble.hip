// gpp_ensemble.hip — prediction from a generated cross block, batched over parameter sets (gpp_predict_gen, gpp_predict_gen_batched in
// include/gpp_ensemble.h): the hot path of ensemble.HyperparameterEnsemble.  Built into a library of its own, libgpp_ensemble_hip.so:
// libgpp_hip.so stays byte for byte what it was, and with it the source signature gpp_version() reports and every recorded digest of
// its arithmetic.  The two libraries share the handle (gpp_internal.h: its stream and its scratch workspace are read here) and the
// device functions of gpp_internal.h; this file calls no function of the other library.
//
// The tile is gpp_apply_tile of gpp_apply.hip (same constants, same LDS layout, same generation and MFMA phases) with another
// operand C and another epilogue; the generator below is that file's KernelGen without its gradient members.
#include "gpp_internal.h"
#include "../../include/gpp_ensemble.h"

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

constexpr size_t ap_lds_bytes(int D) {
  return ((size_t)D * AP_TM + (size_t)D * AP_BK + AP_BK + 2 * AP_DMAX + (size_t)AP_TM * AP_LDG + (size_t)AP_BK * AP_LDC) * sizeof(double);
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

// what turns (a row of Ua, a row of Ub) into an entry of the cross block: sf2 k(ua, ub; w), features staged scaled by sqrt(w)
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
};

// ---- prediction from a generated cross block (gpp_predict_gen, gpp_predict_gen_batched) ------------------------------------------
//   mean[a] = sum_s V[a,s] z_s,   var[a] = sf2 - sum_s V[a,s]^2,   V = K_*N L^-T,   K_*N[a,j] = sf2 k(Ua_a, Ub_j; w)
// gpp_apply_tile with C = L^-T, the mirror the Linv buffer keeps in its upper triangle (C[j][s] = Linv[j * ldi + s], j <= s), and
// an epilogue that reduces the tile instead of storing it.  Column s of L^-T is zero below row s, so the column tile that starts at
// s0 walks j < min(N, s0 + 64) only, and while a chunk is staged every entry with j > s becomes an exact 0: the strictly lower
// triangle (L^-1) is never read.  A sum of squares is not linear in partial products, so there are no AP_SPLIT pieces: one
// work-group walks its whole range.  blockIdx.z is the batch element.  The epilogue adds, for each of the tile's rows, V z and V^2
// over the lane's four column blocks in their order and then over the sixteen lanes of the row by a fixed butterfly, and writes the
// pair to the record [element][column tile][row]; gpp_predict_gen_finish adds the column tiles in their order.  No atomics, every
// sum has the same terms in the same order wherever the row stands in the call and whichever element it belongs to.
struct PredictGenArgs {
  const double* Ua;    // M x D (+ b * sUa)
  const double* Ub;    // N x D (+ b * sUb)
  const double* w;     // D (+ b * D)
  const double* sf2;   // (+ b)
  const double* Linv;  // N x N, ldi (+ b * sLi): the upper triangle is read
  const double* z;     // N (+ b * sv)
  double* rec;         // [batch][column tiles][M][2]
  int64_t M, N, ldi, sUa, sUb, sLi, sv;
  int D, kind, d_split, tiles_s;
};

template <class GEN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void gpp_predict_gen_tile(const PredictGenArgs p) {
  extern __shared__ __attribute__((aligned(16))) double ap_smem[];
  const int D = p.D;
  double* sa = ap_smem;                       // the layout of gpp_apply_tile (sx is not used)
  double* sb = sa + (size_t)D * AP_TM;
  double* sx = sb + (size_t)D * AP_BK;
  double* sw = sx + AP_BK;
  double* sg = sw + 2 * AP_DMAX;
  double* sc = sg + (size_t)AP_TM * AP_LDG;

  const int64_t be = blockIdx.z;
  const double* __restrict__ Ua = p.Ua + be * p.sUa;
  const double* __restrict__ Ub = p.Ub + be * p.sUb;
  const double* __restrict__ C = p.Linv + be * p.sLi;
  const double* __restrict__ z = p.z + be * p.sv;
  struct { const double* w; const double* sf2; int kind, d_split; } q{p.w + be * D, p.sf2 + be, p.kind, p.d_split};
  GEN gen;
  gen.setup(q);

  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * AP_TM;
  const int64_t s0 = (int64_t)blockIdx.y * AP_TS;
  const int64_t k1 = s0 + AP_TS < p.N ? s0 + AP_TS : p.N;  // L^-T[j][s] = 0 for j > s: nothing beyond the tile's last column

  if (tid < D) {
    sw[tid] = gen.scale_a(tid);
    sw[AP_DMAX + tid] = gen.scale_b(tid);
  }
  __syncthreads();
  for (int e = tid; e < D * AP_TM; e += 256) {
    const int r = e / D, d = e - r * D;
    sa[d * AP_TM + r] = (i0 + r < p.M) ? Ua[(i0 + r) * D + d] * sw[d] : 0.0;
  }

  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int ty = tid >> 4, tx = tid & 15;
  const int nb = (int)((k1 - s0 + 15) >> 4);  // 16-column blocks of this tile that hold a column (uniform, 1 .. 4)

  v4d acc4[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc4[b] = (v4d){0.0, 0.0, 0.0, 0.0};

  for (int64_t kb = 0; kb < k1; kb += AP_BK) {
    __syncthreads();
    for (int e = tid; e < D * AP_BK; e += 256) {
      const int r = e / D, d = e - r * D;
      sb[d * AP_BK + r] = (kb + r < k1) ? Ub[(kb + r) * D + d] * sw[AP_DMAX + d] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < AP_BK * AP_TS / 256; ++i) {
      const int e = tid + 256 * i;
      const int k = e >> 6, c = e & 63;
      const bool ok = (s0 + c < k1) & (kb + k <= s0 + c);  // the mirror only (and with it kb + k < k1)
      sc[k * AP_LDC + c] = ok ? C[(kb + k) * p.ldi + s0 + c] : 0.0;
    }
    __syncthreads();

    {  // generate K_*N[4 ty + a][2 tx + b], as gpp_apply_tile does
      double acc[4][2][GEN::NACC];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a) gen.init(acc[a][b], 0.0);
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
      const bool ok0 = kb + 2 * tx < k1, ok1 = kb + 2 * tx + 1 < k1;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double g0 = gen.value(acc[a][0]), g1 = gen.value(acc[a][1]);
        const v2d g = {ok0 ? g0 : 0.0, ok1 ? g1 : 0.0};
        *reinterpret_cast<v2d*>(sg + (4 * ty + a) * AP_LDG + 2 * tx) = g;
      }
    }
    __syncthreads();

    const double* ga = sg + (wave * 16 + li) * AP_LDG + lk;
    const double* cb = sc + lk * AP_LDC + li;
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

  // element v of acc4[b]: row wave * 16 + 4 v + (l >> 4), column 16 b + (l & 15); a column past N holds an exact 0
  double zs[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) zs[b] = (s0 + 16 * b + li < k1) ? z[s0 + 16 * b + li] : 0.0;
  double* __restrict__ rec = p.rec + ((be * p.tiles_s + blockIdx.y) * p.M) * 2;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    double m = 0.0, ss = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const double x = acc4[b][v];
      m = fma(x, zs[b], m);
      ss = fma(x, x, ss);
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {  // the sixteen lanes of the row: lane ^ o stays inside the group of sixteen
      m += __shfl_xor(m, o);
      ss += __shfl_xor(ss, o);
    }
    const int64_t i = i0 + wave * 16 + 4 * v + lk;
    if (li == 0 && i < p.M) *reinterpret_cast<v2d*>(rec + 2 * i) = (v2d){m, ss};
  }
}

// mean[b][a] = the sum over the column tiles, in their order, of the first entries of the records; var[b][a] = sf2_b - that of the second
__global__ __launch_bounds__(256) void gpp_predict_gen_finish(const double* __restrict__ rec, int tiles_s, int64_t M,
                                                              const double* __restrict__ sf2, double* __restrict__ mean_out,
                                                              double* __restrict__ var_out, int64_t so) {
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t be = blockIdx.y;
  if (a >= M) return;
  const double* r = rec + (be * tiles_s * M + a) * 2;
  double m = r[0], ss = r[1];
  for (int t = 1; t < tiles_s; ++t) {
    m += r[(int64_t)t * M * 2];
    ss += r[(int64_t)t * M * 2 + 1];
  }
  mean_out[be * so + a] = m;
  var_out[be * so + a] = sf2[be] - ss;
}

template <class GEN>
hipError_t pg_launch(hipStream_t s, PredictGenArgs a, double* mean_out, double* var_out, int64_t so, int batch) {
  static std::atomic<bool> done[64];  // more than 48 KiB of dynamic LDS (D > 19 features) needs the opt-in, once per device
  if (ap_lds_bytes(a.D) > 48 * 1024)
    if (hipError_t e = ap_lds_optin(gpp_predict_gen_tile<GEN>, done); e != hipSuccess) return e;
  const int64_t tiles_m = (a.M + AP_TM - 1) / AP_TM;
  const int64_t tiles_s = (a.N + AP_TS - 1) / AP_TS;
  if (tiles_m > 0x7fffffff || tiles_s > 65535 || batch > 65535) return hipErrorInvalidValue;
  a.tiles_s = (int)tiles_s;
  hipLaunchKernelGGL((gpp_predict_gen_tile<GEN>), dim3((unsigned)tiles_m, (unsigned)tiles_s, (unsigned)batch), dim3(256),
                     ap_lds_bytes(a.D), s, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(gpp_predict_gen_finish, dim3((unsigned)((a.M + 255) / 256), (unsigned)batch), dim3(256), 0, s, a.rec,
                     (int)tiles_s, a.M, a.sf2, mean_out, var_out, so);
  return hipGetLastError();
}


size_t pg_ws_bytes(int64_t N, int64_t M, int batch) {
  return (size_t)batch * (size_t)((N + AP_TS - 1) / AP_TS) * (size_t)M * 2 * sizeof(double);
}

hipError_t pg_launch_any(hipStream_t s, const double* Ua, int64_t sUa, int64_t M, const double* Ub, int64_t sUb, int64_t N,
                                  int D, const double* w, const double* sf2, int kind, int d_split, const double* Linv, int64_t ldi,
                                  int64_t sLi, const double* z, int64_t sv, double* mean_out, double* var_out, int64_t so, int batch,
                                  void* ws) {
  PredictGenArgs a{};
  a.Ua = Ua; a.Ub = Ub; a.w = w; a.sf2 = sf2; a.Linv = Linv; a.z = z; a.rec = static_cast<double*>(ws);
  a.M = M; a.N = N; a.ldi = ldi; a.sUa = sUa; a.sUb = sUb; a.sLi = sLi; a.sv = sv;
  a.D = D; a.kind = kind; a.d_split = d_split;
  if (kind == 0) return pg_launch<KernelGen<false>>(s, a, mean_out, var_out, so, batch);
  return pg_launch<KernelGen<true>>(s, a, mean_out, var_out, so, batch);
}


inline int rc(hipError_t e) { return e == hipSuccess ? 0 : 1000 + (int)e; }
#define GPP_TRY(expr)                   \
  do {                                  \
    hipError_t _e = (expr);             \
    if (_e != hipSuccess) return rc(_e); \
  } while (0)
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks of the two entry points; `one` says which argument list a code counts in (single-problem, batched)
static int predict_gen(gpp_handle_t h, bool one, const double* Ua, int64_t sUa, int64_t M, const double* Ub, int64_t sUb, int64_t N,
                       int D, const double* w, const double* sf2, int kind, int d_split, const double* Linv, int64_t ldi, int64_t sLi,
                       const double* z, int64_t sv, double* mean_out, double* var_out, int64_t so, int batch) {
  auto arg = [one](int single, int batched) { return -(one ? single : batched); };
  if (!h) return -1;
  if (!Ua) return arg(2, 2);
  if (M < 1) return arg(3, 4);
  if (!Ub) return arg(4, 5);
  if (N < 1) return arg(5, 7);
  if (D < 1 || D > 64) return arg(6, 8);
  if (!w) return arg(7, 9);
  if (!sf2) return arg(8, 10);
  if (kind < 0 || kind > 2) return arg(9, 11);
  if (d_split < 0 || d_split > D) return arg(10, 12);
  if (!Linv) return arg(11, 13);
  if (!aligned16(Linv) || (ldi & 1) || ldi < N) return arg(12, 14);
  if (!z || !aligned16(z)) return arg(13, 16);
  if (!mean_out) return arg(14, 18);
  if (!var_out) return arg(15, 19);
  if (!one) {
    if (sUa < 0 || (sUa & 1)) return -3;
    if (sUb < 0 || (sUb & 1)) return -6;
    if (sLi < 0 || (sLi & 1)) return -15;
    if (sv < N || (sv & 1)) return -17;
    if (so < M || (so & 1)) return -20;
    if (int q = ((batch < 1 || batch > 65535) ? -21 : 0)) return q;
  }
  if (!h->ws || h->ws_bytes < pg_ws_bytes(N, M, batch)) return GPP_NO_WORKSPACE;
  GPP_TRY(pg_launch_any(h->stream, Ua, sUa, M, Ub, sUb, N, D, w, sf2, kind, d_split, Linv, ldi, sLi, z, sv, mean_out, var_out,
                                 so, batch, h->ws));
  return 0;
}

}  // namespace

extern "C" {

#ifndef GPP_ENSEMBLE_SRC_HASH
#define GPP_ENSEMBLE_SRC_HASH "unknown"
#endif
const char* gpp_ensemble_version(void) { return "gpp_ensemble 0.1 (gfx950; src " GPP_ENSEMBLE_SRC_HASH ")"; }

size_t gpp_predict_gen_workspace_bytes(int64_t N, int64_t M, int batch) {
  return (N < 1 || M < 1 || batch < 1) ? 0 : pg_ws_bytes(N, M, batch);
}

int gpp_predict_gen(gpp_handle_t h, const double* Ua, int64_t M, const double* Ub, int64_t N, int D, const double* w, const double* sf2,
                    int kind, int d_split, const double* Linv, int64_t ldi, const double* z, double* mean_out, double* var_out) {
  return predict_gen(h, true, Ua, 0, M, Ub, 0, N, D, w, sf2, kind, d_split, Linv, ldi, 0, z, 0, mean_out, var_out, 0, 1);
}

int gpp_predict_gen_batched(gpp_handle_t h, const double* Ua, int64_t sUa, int64_t M, const double* Ub, int64_t sUb, int64_t N, int D,
                            const double* w, const double* sf2, int kind, int d_split, const double* Linv, int64_t ldi, int64_t sLi,
                            const double* z, int64_t sv, double* mean_out, double* var_out, int64_t so, int batch) {
  return predict_gen(h, false, Ua, sUa, M, Ub, sUb, N, D, w, sf2, kind, d_split, Linv, ldi, sLi, z, sv, mean_out, var_out, so, batch);
}

}  // extern "C"

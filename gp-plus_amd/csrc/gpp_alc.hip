// gpp_alc.hip — expected variance reduction of candidate observations (active learning: Cohn's ALC, IMSE over a reference set).
//
// gpp_post_cross_sq (gpp.h): out[c] = sum_r omega_r c(x_r, x_c)^2 with the posterior cross-covariance c = sf2 k - Vc Vr^T of a
// fitted model, V = K_*N Linv^T as gpp_predict leaves it.  No reference counterpart: the reference refits per candidate.
// The product and the square-and-sum run in ONE launch of gpp_post_cross_f64 (gpp_gemm.hip, beside the tile body it shares with
// gpp_gemm), which leaves one record of 128 row sums per 128 x 128 tile in the handle workspace; the finish kernel below adds the
// records of a row tile's column tiles in index order.  The M_c x M_r block is never written.
//
// gpp_post_cross_min (gpp.h): out[c][k] = min_r (m_r + nodes_k scale_c c(x_r, x_c)), the reduction of the knowledge gradient's
// Gauss-Hermite form, by the same product with PostCrossMinEpilogue (gpp_gemm.hip): Q minima per row and column half of a tile go to
// the workspace, the finish kernel below takes the minimum of a row's records.
//
// gpp_post_cross_lin_sq (gpp.h): gpp_post_cross_sq for rows that observe a linear functional of f, a value plus gradient components
// (the score of a run that returns y and its gradient), by the same product with PostCrossLinEpilogue and the same records and finish.
#include "../../include/gpp.h"
#include "gpp_internal.h"

namespace {

inline bool alc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int alc_rc(hipError_t e) { return e == hipSuccess ? 0 : 1000 + (int)e; }

// one thread per candidate: tiles_n terms, added in the order of the column tiles
__global__ __launch_bounds__(256) void gpp_post_cross_finish(const double* __restrict__ rec, int tiles_n, int Mc, double* __restrict__ out) {
  const int c = (int)(blockIdx.x * 256 + threadIdx.x);
  if (c >= Mc) return;
  const double* p = rec + ((int64_t)(c >> 7) * tiles_n) * 128 + (c & 127);
  double s = 0.0;
  for (int tn = 0; tn < tiles_n; ++tn) s += p[(int64_t)tn * 128];
  out[c] = s;
}

// one thread per (candidate, node): the minimum over the 2 tiles_n records of the candidate's row, in index order
__global__ __launch_bounds__(256) void gpp_post_cross_min_finish(const double* __restrict__ rec, int tiles_n, int64_t Mc, int Q,
                                                                 double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Mc * Q) return;
  const int64_t c = i / Q;
  const int k = (int)(i - c * Q);
  const double* p = rec + (((c >> 7) * tiles_n) * 2 * 128 + (c & 127)) * Q + k;
  double s = p[0];
  for (int j = 1; j < 2 * tiles_n; ++j) s = fmin(s, p[(int64_t)j * 128 * Q]);
  out[i] = s;
}

}  // namespace

size_t gpp_post_cross_ws_bytes(int64_t Mc, int64_t Mr) {
  if (Mc < 1 || Mr < 1) return 0;
  return (size_t)(((Mc + 127) / 128) * ((Mr + 127) / 128) * 128) * sizeof(double);
}

extern "C" int gpp_post_cross_sq(gpp_handle_t h, const double* Uc, int64_t Mc, const double* Ur, int64_t Mr, int D, const double* w,
                                 const double* sf2, int kind, int d_split, const double* Vc, int64_t ldc, const double* Vr,
                                 int64_t ldr, int64_t K, int vt, const double* omega, double* out) {
  if (!h) return -1;
  if (!Uc) return -2;
  if (Mc < 1 || Mc > 0x7ffffff0) return -3;
  if (!Ur) return -4;
  if (Mr < 1 || Mr > 0x7ffffff0) return -5;
  if (D < 1 || D > 64) return -6;
  if (!w) return -7;
  if (!sf2) return -8;
  if (kind < 0 || kind > 2) return -9;
  if (d_split < 0 || d_split > D) return -10;
  if (K < 1 || K > 0x7ffffff0) return -15;
  if (vt != 0 && vt != 1) return -16;
  if (!Vc || !alc_aligned16(Vc) || (ldc & 1) || ldc < (vt ? Mc : K)) return -11;
  if (!Vr || !alc_aligned16(Vr) || (ldr & 1) || ldr < (vt ? Mr : K)) return -13;
  if (!out) return -18;
  const int64_t tiles_m = (Mc + 127) / 128, tiles_n = (Mr + 127) / 128;
  if (tiles_m * tiles_n >= ((int64_t)1 << 31)) return -3;
  if (!h->ws || h->ws_bytes < gpp_post_cross_ws_bytes(Mc, Mr)) return GPP_NO_WORKSPACE;
  GemmArgs g{};
  g.A = Vc; g.B = Vr; g.C = nullptr;
  g.lda = ldc; g.ldb = ldr;
  g.M = (int)Mc; g.N = (int)Mr; g.K = (int)K;
  PostCrossArgs e{};
  e.Uc = Uc; e.Ur = Ur; e.w = w; e.sf2 = sf2; e.omega = omega;
  e.rec = reinterpret_cast<double*>(h->ws);
  e.dk = D | (kind << 8) | (d_split << 16);
  if (hipError_t r = gpp_launch_post_cross(h->stream, vt ? 2 : 0, g, e); r != hipSuccess) return alc_rc(r);
  hipLaunchKernelGGL(gpp_post_cross_finish, dim3((unsigned)((Mc + 255) / 256)), dim3(256), 0, h->stream, e.rec, (int)tiles_n, (int)Mc, out);
  return alc_rc(hipGetLastError());
}

// rows that are linear functionals of f (value and gradient components at Uf_i): the tiles, records and finish of gpp_post_cross_sq
extern "C" int gpp_post_cross_lin_sq(gpp_handle_t h, const double* Uf, int64_t Mf, const double* Ur, int64_t Mr, int D, const double* w,
                                     const double* sf2, int kind, int d_split, int d0, int nd, const double* A, int64_t lda,
                                     const double* Vf, int64_t ldf, const double* Vr, int64_t ldr, int64_t K, int vt,
                                     const double* omega, double* out) {
  if (!h) return -1;
  if (!Uf) return -2;
  if (Mf < 1 || Mf > 0x7ffffff0) return -3;
  if (!Ur) return -4;
  if (Mr < 1 || Mr > 0x7ffffff0) return -5;
  if (D < 1 || D > 64) return -6;
  if (!w) return -7;
  if (!sf2) return -8;
  if (kind < 0 || kind > 2) return -9;
  if (d_split < 0 || d_split > D) return -10;
  if (d0 < 0 || d0 >= D) return -11;
  if (nd < 1 || d0 + nd > D) return -12;
  if (!A) return -13;
  if (lda < 1 + nd) return -14;
  if (K < 1 || K > 0x7ffffff0) return -19;
  if (vt != 0 && vt != 1) return -20;
  if (!Vf || !alc_aligned16(Vf) || (ldf & 1) || ldf < (vt ? Mf : K)) return -15;
  if (!Vr || !alc_aligned16(Vr) || (ldr & 1) || ldr < (vt ? Mr : K)) return -17;
  if (!out) return -22;
  const int64_t tiles_m = (Mf + 127) / 128, tiles_n = (Mr + 127) / 128;
  if (tiles_m * tiles_n >= ((int64_t)1 << 31)) return -3;
  if (!h->ws || h->ws_bytes < gpp_post_cross_ws_bytes(Mf, Mr)) return GPP_NO_WORKSPACE;
  GemmArgs g{};
  g.A = Vf; g.B = Vr; g.C = nullptr;
  g.lda = ldf; g.ldb = ldr;
  g.M = (int)Mf; g.N = (int)Mr; g.K = (int)K;
  PostCrossLinArgs e{};
  e.Uf = Uf; e.Ur = Ur; e.w = w; e.sf2 = sf2; e.omega = omega; e.A = A; e.lda = lda;
  e.rec = reinterpret_cast<double*>(h->ws);
  e.dk = D | (kind << 8) | (d_split << 16);
  e.dn = d0 | (nd << 8);
  if (hipError_t r = gpp_launch_post_cross_lin(h->stream, vt ? 2 : 0, g, e); r != hipSuccess) return alc_rc(r);
  hipLaunchKernelGGL(gpp_post_cross_finish, dim3((unsigned)((Mf + 255) / 256)), dim3(256), 0, h->stream, e.rec, (int)tiles_n, (int)Mf, out);
  return alc_rc(hipGetLastError());
}

size_t gpp_post_cross_min_ws_bytes(int64_t Mc, int64_t Mr, int Q) {
  if (Mc < 1 || Mr < 1 || Q < 1) return 0;
  return (size_t)(((Mc + 127) / 128) * ((Mr + 127) / 128) * 2 * 128 * Q) * sizeof(double);
}

extern "C" int gpp_post_cross_min(gpp_handle_t h, const double* Uc, int64_t Mc, const double* Ur, int64_t Mr, int D, const double* w,
                                  const double* sf2, int kind, int d_split, const double* Vc, int64_t ldc, const double* Vr,
                                  int64_t ldr, int64_t K, int vt, const double* m, const double* scale, const double* nodes, int Q,
                                  double* out) {
  if (!h) return -1;
  if (!Uc) return -2;
  if (Mc < 1 || Mc > 0x7ffffff0) return -3;
  if (!Ur) return -4;
  if (Mr < 1 || Mr > 0x7ffffff0) return -5;
  if (D < 1 || D > 64) return -6;
  if (!w) return -7;
  if (!sf2) return -8;
  if (kind < 0 || kind > 2) return -9;
  if (d_split < 0 || d_split > D) return -10;
  if (K < 1 || K > 0x7ffffff0) return -15;
  if (vt != 0 && vt != 1) return -16;
  if (!Vc || !alc_aligned16(Vc) || (ldc & 1) || ldc < (vt ? Mc : K)) return -11;
  if (!Vr || !alc_aligned16(Vr) || (ldr & 1) || ldr < (vt ? Mr : K)) return -13;
  if (!m) return -17;
  if (!scale) return -18;
  if (!nodes) return -19;
  if (Q < 1 || Q > 64) return -20;
  if (!out) return -21;
  const int64_t tiles_m = (Mc + 127) / 128, tiles_n = (Mr + 127) / 128;
  if (tiles_m * tiles_n >= ((int64_t)1 << 31)) return -3;
  if ((Mc * Q + 255) / 256 >= ((int64_t)1 << 31)) return -3;
  if (!h->ws || h->ws_bytes < gpp_post_cross_min_ws_bytes(Mc, Mr, Q)) return GPP_NO_WORKSPACE;
  GemmArgs g{};
  g.A = Vc; g.B = Vr; g.C = nullptr;
  g.lda = ldc; g.ldb = ldr;
  g.M = (int)Mc; g.N = (int)Mr; g.K = (int)K;
  PostCrossMinArgs e{};
  e.Uc = Uc; e.Ur = Ur; e.w = w; e.sf2 = sf2; e.m = m; e.scale = scale; e.nodes = nodes;
  e.rec = reinterpret_cast<double*>(h->ws);
  e.dk = D | (kind << 8) | (d_split << 16) | (Q << 24);
  if (hipError_t r = gpp_launch_post_cross_min(h->stream, vt ? 2 : 0, g, e); r != hipSuccess) return alc_rc(r);
  hipLaunchKernelGGL(gpp_post_cross_min_finish, dim3((unsigned)((Mc * Q + 255) / 256)), dim3(256), 0, h->stream, e.rec, (int)tiles_n,
                     Mc, Q, out);
  return alc_rc(hipGetLastError());
}

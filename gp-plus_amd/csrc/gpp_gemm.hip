// gpp_gemm.hip — fp64 MFMA GEMM for gfx950 (MI355X): C = beta*C + alpha*op(A)*op(B) with triangular operand
// masks, per-tile K ranges and lower-only output.  It carries every O(N^3) flop of the exact-GP path:
//   - TRSM / SYRK / GEMM updates of the blocked Cholesky  (replaces torch.linalg.cholesky_ex reached from
//     gpytorch psd_safe_cholesky, reference call site optim/mll_torch.py:116)
//   - TRMM pair products of the bottom-up triangular inverse and the LAUUM product Linv^T Linv
//     (replace ATen cholesky_backward, reference call site optim/mll_torch.py:117)
//   - V = K_*N Linv^T of the prediction path (models/gpregression.py:122-149).
//
// Design (CDNA4, measured on MI355X): v_mfma_f64_16x16x4_f64 — lane l supplies A[row l%16][k l/16] and B[k l/16][col l%16] and
// holds D[row (l/16) + 4v][col l%16] in element v of its 4-double accumulator (tools/attic/mfma16_layout.hip).  A bare loop of the
// instruction sustains 69.6 TFLOP/s chip-wide, the rate rocBLAS's MI16x16x4 DGEMM kernels reach too (72.9); the round-1 kernel
// used the 4x4x4_4b form on the strength of a probe that had measured hipcc's AGPR copies (profiles/r02_mfma_f64_16x16x4.txt).
// A (2*WT)^2 output tile per 256-thread work-group, 2x2 waves; each wave owns WT x WT = (WT/16)^2 blocks of 16 x 16
// (WT=64: 64 accumulator doubles per lane, in VGPRs: __launch_bounds__(256, 2)).  K is consumed in chunks of 16;
// both operand chunks are staged in LDS in [k][row] order (padded strides, see ldt_*), double-buffered: the global
// loads of chunk c+1 are issued before the MFMAs of chunk c and written to the other buffer afterwards, one barrier
// per chunk (in the big tile's interior loop both run UNDER the MFMAs, see PIPE).
// WT = 32 / 16 variants (64^2 / 32^2 tiles) and a 128 x 32 tile serve the small sub-problems, where the
// grid of 128^2 tiles would leave most of the 256 CUs idle; they stage K in chunks of 64 with one LDS buffer (template
// parameters BK, NBUF below).  Work-groups are independent along two batch dimensions (grid.y, grid.z).
#include "../../include/gpp.h"
#include "gpp_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>

typedef double v2d __attribute__((ext_vector_type(2)));
typedef double v4d __attribute__((ext_vector_type(4)));
typedef const char __attribute__((address_space(1))) gchar;  // global address space, spelled out
typedef const v2d __attribute__((address_space(1))) gv2d;

namespace {

#ifndef GPP_CLEAN_SETPRIO
#define GPP_CLEAN_SETPRIO 1  // s_setprio pair around the big tile's pipelined loop in the TAG != 0 kernels (build-time A/B knob)
#endif
#ifndef GPP_DAG_CHAIN_PRIO
#define GPP_DAG_CHAIN_PRIO 2  // s_setprio level of the DAG executor's 64-tile (chain) tasks, 0 = none (build-time A/B knob)
#endif
#ifndef GPP_DAG_PIPE
#define GPP_DAG_PIPE 1  // the pipelined clean loop in the DAG executor's big tile too (0: the plain loop there; build-time A/B knob)
#endif
constexpr int BK16 = 16;  // K chunk of the big tile and of every k-contiguous ("KC") operand
// LDS layouts.  Row-contiguous operands ("MC", stored [k][row] in memory) are staged as [k][T+16]: 16-byte aligned
// rows for ds_write_b128, and the two k-rows a 32-lane ds_read_b64 group touches fall in different bank halves.
// k-contiguous operands ("KC", stored [row][k]) are staged UNtransposed as [row][18]: every thread writes its 16-byte
// vector with one ds_write_b128 (8 lanes = one 128-byte row), and with the 144-byte row stride both fragment reads
// are conflict free: A lanes (i=0..3, k, k+1) hit slots {18i + k}, B lanes (c=0..15, k, k+1) hit 18c + k mod 32,
// which enumerates all 32 8-byte slots.
constexpr int ldt_mc(int T, int BK = 16) { return BK == 16 ? T + 16 : T + 4; }
constexpr int LDK = BK16 + 2;  // [row][k] chunks of k-contiguous operands: 144-byte rows, see below

// Staging is split in two so that the global loads of chunk c+1 stay in flight across the MFMAs of chunk c:
//   load_*  : computes the keep-predicates (range + triangular mask; no loaded data involved) and issues one
//             branch-free 16-byte load per vector (from P itself when the element is out of range).  Reading one
//             double past kend/R stays inside the allocation: ld is even and >= the extent (gpp.h).
//   store_* : after the MFMAs, zeroes the dropped elements by select and writes the chunk to LDS.
__device__ __forceinline__ bool keep_elem(int mask, int k, int row) {
  // bitwise on purpose: no short-circuit branches between the loads of a chunk (a branch ends the basic block, and
  // hipcc then waits for the loads issued so far: the 20 vectors of a 128-row chunk arrived one L2 trip at a time)
  return (mask == 0) | ((mask == 1) & (k <= row)) | ((mask == 2) & (k >= row));
}

// Operand stored [row][k] (k contiguous): T rows x 16 k per chunk, T/32 16-byte vectors per thread.
template <int T>
__device__ __forceinline__ unsigned load_kc(const double* __restrict__ P, int64_t ld, int R, int r0, int kb, int kend,
                                            int mask, int tid, v2d (&reg)[T / 32]) {
  unsigned keep = 0;
  const double* ptr[T / 32];
#pragma unroll
  for (int i = 0; i < T / 32; ++i) {
    const int v = tid + 256 * i;
    const int gr = r0 + (v >> 3);
    const int gk = kb + ((v & 7) << 1);
    const bool v0 = (gr < R) & (gk < kend);
    const bool k0 = v0 & keep_elem(mask, gk, gr);
    const bool k1 = v0 & (gk + 1 < kend) & keep_elem(mask, gk + 1, gr);
    keep |= (k0 ? 1u : 0u) << (2 * i);
    keep |= (k1 ? 1u : 0u) << (2 * i + 1);
    ptr[i] = v0 ? P + (int64_t)gr * ld + gk : P;
  }
#pragma unroll
  for (int i = 0; i < T / 32; ++i) reg[i] = *reinterpret_cast<const v2d*>(ptr[i]);
  return keep;
}
template <int T, bool SEL>
__device__ __forceinline__ void store_kc(double* __restrict__ s, int tid, const v2d (&reg)[T / 32], unsigned keep) {
#pragma unroll
  for (int i = 0; i < T / 32; ++i) {
    const int v = tid + 256 * i;
    v2d t = reg[i];
    if (SEL) {
      t.x = ((keep >> (2 * i)) & 1u) ? t.x : 0.0;
      t.y = ((keep >> (2 * i + 1)) & 1u) ? t.y : 0.0;
    }
    *reinterpret_cast<v2d*>(s + (v >> 3) * LDK + ((v & 7) << 1)) = t;
  }
}

// Operand stored [k][row] (row contiguous): BK k x T rows per chunk, BK * T / 512 16-byte vectors per thread.
// (`dummy`: where the lanes of out-of-range elements read instead — any readable address; P itself unless P is a biased base,
//  see GemmArgs::compact_bc)
template <int T, int BK, int NTH = 256>
__device__ __forceinline__ unsigned load_mc(const double* __restrict__ P, int64_t ld, int R, int r0, int kb, int kend,
                                            int mask, int tid, v2d (&reg)[BK * T / (2 * NTH)], const double* __restrict__ dummy) {
  constexpr int NV = BK * T / (2 * NTH);
  unsigned keep = 0;
  const double* ptr[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = tid + NTH * i;
    const int gk = kb + v / (T / 2);
    const int gr = r0 + ((v % (T / 2)) << 1);
    const bool v0 = (gk < kend) & (gr < R);
    const bool k0 = v0 & keep_elem(mask, gk, gr);
    const bool k1 = v0 & (gr + 1 < R) & keep_elem(mask, gk, gr + 1);
    keep |= (k0 ? 1u : 0u) << (2 * i);
    keep |= (k1 ? 1u : 0u) << (2 * i + 1);
    ptr[i] = v0 ? P + (int64_t)gk * ld + gr : dummy;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) reg[i] = *reinterpret_cast<const v2d*>(ptr[i]);  // all requests back to back
  return keep;
}
template <int T, int BK, bool SEL, int NTH = 256>
__device__ __forceinline__ void store_mc(double* __restrict__ s, int tid, const v2d (&reg)[BK * T / (2 * NTH)], unsigned keep) {
#pragma unroll
  for (int i = 0; i < BK * T / (2 * NTH); ++i) {
    const int v = tid + NTH * i;
    v2d t = reg[i];
    if (SEL) {
      t.x = ((keep >> (2 * i)) & 1u) ? t.x : 0.0;
      t.y = ((keep >> (2 * i + 1)) & 1u) ? t.y : 0.0;
    }
    *reinterpret_cast<v2d*>(s + (v / (T / 2)) * ldt_mc(T, BK) + ((v % (T / 2)) << 1)) = t;
  }
}

// ---- interior fast path --------------------------------------------------------------------------------
// For a chunk whose 16 k's and T rows are all in range and untouched by the triangular mask (a work-group-uniform
// test), staging needs no predicates at all: one load per vector from  uniform_base + per-thread 32-bit byte offset
// (SGPR-base addressing), and plain LDS stores.  This removes ~3/4 of the VALU instructions that otherwise compete
// with the MFMAs for the SIMD's issue port.
template <int T, int BK>
__device__ __forceinline__ bool chunk_is_interior(int r0, int R, int kb, int kend, int mask) {
  if (r0 + T > R || kb + BK > kend) return false;
  if (mask == 1) return kb + BK - 1 <= r0;      // keep k <= row holds for every row >= r0
  if (mask == 2) return kb >= r0 + T - 1;       // keep k >= row holds for every row <  r0 + T
  return true;
}
// In-range chunk of a row-contiguous operand that the triangular mask cuts: same lean loads as an interior chunk, the
// keep bits come from the indices alone.
template <int T, int BK>
__device__ __forceinline__ bool chunk_in_range(int r0, int R, int kb, int kend) {
  return r0 + T <= R && kb + BK <= kend;
}
template <int T, int BK, int NTH = 256>
__device__ __forceinline__ unsigned mask_bits_mc(int r0, int kb, int mask, int tid) {
  unsigned keep = 0;
#pragma unroll
  for (int i = 0; i < BK * T / (2 * NTH); ++i) {
    const int v = tid + NTH * i;
    const int gk = kb + v / (T / 2);
    const int gr = r0 + ((v % (T / 2)) << 1);
    keep |= (keep_elem(mask, gk, gr) ? 1u : 0u) << (2 * i);
    keep |= (keep_elem(mask, gk, gr + 1) ? 1u : 0u) << (2 * i + 1);
  }
  return keep;
}
template <int T, bool KC, int BK, int NTH = 256>
__device__ __forceinline__ void thread_offsets(int64_t ld, int tid, unsigned (&off)[BK * T / (2 * NTH)]) {
#pragma unroll
  for (int i = 0; i < BK * T / (2 * NTH); ++i) {
    const int v = tid + NTH * i;
    if (KC) off[i] = (unsigned)(((int64_t)(v >> 3) * ld + ((v & 7) << 1)) * 8);
    else off[i] = (unsigned)(((int64_t)(v / (T / 2)) * ld + ((v % (T / 2)) << 1)) * 8);
  }
}
template <int NV>
__device__ __forceinline__ void load_fast(const double* __restrict__ ubase, const unsigned (&off)[NV], v2d (&reg)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i)
    reg[i] = *reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(ubase) + off[i]);
}

// The row-contiguous TN variant (every hot product of the evaluation) keeps 2 work-groups per CU (<= 256 VGPRs);
// variants with a k-contiguous operand are off the hot path (prediction, tests) and take the registers they need.
// TAG only changes the kernel's NAME: the single N^3/3-flop LAUUM launch runs as <2,64,64,1> so that profilers report
// it on its own line (the roofline entry of bench.py), apart from the ~1300 launches of the recursions.
// BK = K chunk, NBUF = LDS buffers per operand.  The big tile runs (16, 2): its MFMA phase (64 accumulators per lane,
// 2 work-groups per CU) covers a load round trip and one barrier per chunk suffices.  The small tiles of the recursions'
// leaves have almost no MFMA work per 16-wide chunk, so every chunk cost one full L2 round trip (~0.6 us: a K = 128
// product took 8-20 us); they run (64, 1): four times fewer round trips, the next chunk's loads in flight in
// registers during the MFMAs, two barriers per chunk.  (k-contiguous operands, VAR != 2, only exist with BK = 16.)
// WR = rows of waves in the work-group: 2 (256 threads, 2 x 2 waves: every instantiation of the evaluation) or 4 (512 threads, 4 x 2
// waves, a 256 x 128 tile on ONE work-group per CU: 25 % fewer operand bytes per flop and measured slower — LAUUM at N = 20000 41.4
// against 39.1 ms, profiles/r03_potrf_experiments.txt — so the launcher instantiates WR = 2 only).
// One output tile (tm, tn) of the product described by ``p``: the body shared by the launch-per-product kernel (gpp_gemm_f64, p in
// the kernel arguments) and the DAG executor (gpp_dag_f64, p in a device array read through the constant address
// space: scalar loads, re-materialisable like kernel arguments).  A, B, C: the batch element's operands,
// C2: its mirrored output (or null).  Ends with a work-group barrier after the last LDS read, so the caller may stage another tile at once.
struct GemmNoHook {
  static constexpr bool per_task = false;
  __device__ __forceinline__ void operator()() const {}
};
// (`epi`: anything but GemmStoreC replaces the store of C — it is handed the wave's accumulators once the main loop's LDS is free)
struct GemmStoreC {};
// (`before_epilogue`: called by every thread after the last MFMA and before the first access to C — the DAG executor issues its
//  next ticket's atomic there, so that its latency runs under the epilogue)
template <int VAR, int WTM, int WTN, int TAG, int BK, int NBUF, int WR, class P, class H = GemmNoHook, class E = GemmStoreC>
__device__ __forceinline__ void gemm_tile(const P& p, const int tm, const int tn, const double* __restrict__ A,
                                          const double* __restrict__ B, double* __restrict__ C, double* C2,
                                          double* __restrict__ smem, H before_epilogue = H(), const E& epi = E()) {
  static_assert(BK == 16 || VAR == 2, "wide K chunks are implemented for row-contiguous (TN) operands only");
  static_assert(BK % 16 == 0 && (NBUF == 1 || NBUF == 2), "bad staging parameters");
  static_assert(WR == 2 || (WR == 4 && VAR == 2 && BK == 16 && NBUF == 2 && WTM == 64 && WTN == 64), "the tall tile is TN only");
  constexpr int NTH = 128 * WR;
  constexpr bool A_KC = (VAR != 2);
  constexpr bool B_KC = (VAR == 0);
  constexpr int TM = WR * WTM, TN = 2 * WTN;  // work-group tile: TM rows x TN columns (WR x 2 waves)
  constexpr int LDA = ldt_mc(TM, BK), LDB = ldt_mc(TN, BK);  // strides of [k][row] chunks (MC operands)
  constexpr int TX = TM > TN ? TM : TN;
  // doubles per staged chunk: one size for both operands of the square tiles, the two true sizes for the tall one
  constexpr int OPSZ = (BK * ldt_mc(TX, BK) > TX * LDK) ? BK * ldt_mc(TX, BK) : TX * LDK;
  constexpr int OPA = (WR == 2) ? OPSZ : BK * LDA, OPB = (WR == 2) ? OPSZ : BK * LDB;
  constexpr int NVA = BK * TM / (2 * NTH), NVB = BK * TN / (2 * NTH);  // 16-byte vectors per thread and chunk
  constexpr int RB = WTM / 4, CB = WTN / 16;
  constexpr bool SPLIT = (VAR == 2 && RB == 16 && CB == 4 && BK == 16 && NBUF == 2 && WR == 2);  // the big row-contiguous tile
  // The pipelined form of its clean loop (below): every caller of the big tile, the DAG executor included since it stopped carrying
  // the per-thread state of all its bodies through the tile (H::per_task; 249 VGPRs, no spill — profiles/EXPERIMENTS.md).
  // GPP_DAG_PIPE = 0 gives the executor, and only it, the plain loop back.
  constexpr bool PIPE = SPLIT && !(H::per_task && !GPP_DAG_PIPE);

  int tid = threadIdx.x;
  if constexpr (H::per_task) {  // one body of several inside a task loop: nothing derived from the thread index is hoisted out of that loop
    asm volatile("" : "+v"(tid));
    tid &= NTH - 1;  // (gives the compiler the value range back: shifts, not signed divisions)
  }
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = (wave >> 1) * WTM, wn = (wave & 1) * WTN;
  const int li = lane & 15, lk = lane >> 4;
  const int row0 = tm * TM, col0 = tn * TN;
  const double* __restrict__ Bd = B;  // readable addresses for the lanes that must not touch memory (the biased bases below may
  double* __restrict__ Cd = C;        // lie in front of their buffers)
  if (p.compact_bc) {
    // B and C store only the owned column blocks, side by side: shift their bases by (physical - logical) first column of this
    // tile's block (a tile never straddles two blocks: the block width is a multiple of the tile)
    const int b = tn / p.own_bt, q = (b + p.own_off) / p.own_mod;
    const int64_t bias = (int64_t)(q - b) * p.own_bt * TN;
    B += bias;
    C += bias;
  }

  int klo = 0;
  if (p.klo_mode == 1) klo = row0;
  else if (p.klo_mode == 2) klo = col0;
  else if (p.klo_mode == 3) klo = row0 > col0 ? row0 : col0;
  int khi = p.K;
  if (p.khi_mode == 1) khi = min(p.K, row0 + TM);
  else if (p.khi_mode == 2) khi = min(p.K, col0 + TN);
  const int nch = khi > klo ? (khi - klo + BK - 1) / BK : 0;

  // accumulators: acc4[a4][b] element v is C[row0 + wm + 16 a4 + 4 v + (l>>4)][col0 + wn + 16 b + (l&15)] — the 16 x 16 result
  // block of v_mfma_f64_16x16x4_f64 (lane l, element v: row (l>>4) + 4 v, column l&15; tools/attic/mfma16_layout.hip)
  static_assert(RB % 4 == 0, "wave tile rows must be a multiple of 16");
  v4d acc4[RB / 4][CB];
#pragma unroll
  for (int a = 0; a < RB / 4; ++a)
#pragma unroll
    for (int b = 0; b < CB; ++b) acc4[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};

  v2d ra[NVA], rb[NVB];
  unsigned ka = 0, kb_ = 0;
  unsigned offa[NVA], offb[NVB];
  thread_offsets<TM, A_KC, BK, NTH>(p.lda, tid, offa);
  thread_offsets<TN, B_KC, BK, NTH>(p.ldb, tid, offb);
  // uniform bases of the tile's first chunk row/column block; advanced by a scalar per chunk
  const double* __restrict__ ubaseA = A_KC ? A + (int64_t)row0 * p.lda : A + row0;
  const double* __restrict__ ubaseB = B_KC ? B + (int64_t)col0 * p.ldb : B + col0;
  const int64_t stepA = A_KC ? 1 : p.lda, stepB = B_KC ? 1 : p.ldb;  // elements per unit of k

  // extents for the LOADS (see GemmArgs::pad_ok); the stores below always use the true M and N
  const int Mld = (VAR == 2 && p.pad_ok) ? ((p.M + TM - 1) / TM) * TM : p.M;
  const int Nld = (VAR == 2 && p.pad_ok) ? ((p.N + TN - 1) / TN) * TN : p.N;
  // Per operand and chunk, work-group uniform: 0 = edge (predicated loads, select on store), 1 = interior (lean loads,
  // plain stores), 2 = in range but cut by the triangular mask (lean loads, select on store).  The lean paths exist for
  // the row-contiguous TN variant only: with a k-contiguous operand the extra live registers push hipcc over the
  // 256-VGPR budget of 2 waves/SIMD and the spills cost more than the VALU saved.
  int pa = 0, pb = 0;
  auto stage_load = [&](int kb) {
    pa = pb = 0;
    if constexpr (VAR == 2) {
      if (chunk_in_range<TM, BK>(row0, Mld, kb, khi)) pa = chunk_is_interior<TM, BK>(row0, Mld, kb, khi, p.a_mask) ? 1 : 2;
      if (chunk_in_range<TN, BK>(col0, Nld, kb, khi)) pb = chunk_is_interior<TN, BK>(col0, Nld, kb, khi, p.b_mask) ? 1 : 2;
    }
    if constexpr (PIPE) {  // keep the offsets' zero-extension beside the loads (see the clean loop below)
#pragma unroll
      for (int i = 0; i < NVA; ++i) asm("" : "+v"(offa[i]));
#pragma unroll
      for (int i = 0; i < NVB; ++i) asm("" : "+v"(offb[i]));
    }
    if (pa) {
      load_fast<NVA>(ubaseA + (int64_t)kb * stepA, offa, ra);
      if (pa == 2) ka = mask_bits_mc<TM, BK, NTH>(row0, kb, p.a_mask, tid);
    } else {
      if constexpr (A_KC) ka = load_kc<TM>(A, p.lda, p.M, row0, kb, khi, p.a_mask, tid, ra);
      else ka = load_mc<TM, BK, NTH>(A, p.lda, p.M, row0, kb, khi, p.a_mask, tid, ra, A);
    }
    if (pb) {
      load_fast<NVB>(ubaseB + (int64_t)kb * stepB, offb, rb);
      if (pb == 2) kb_ = mask_bits_mc<TN, BK, NTH>(col0, kb, p.b_mask, tid);
    } else {
      if constexpr (B_KC) kb_ = load_kc<TN>(B, p.ldb, p.N, col0, kb, khi, p.b_mask, tid, rb);
      else kb_ = load_mc<TN, BK, NTH>(B, p.ldb, p.N, col0, kb, khi, p.b_mask, tid, rb, Bd);
    }
  };
  auto stage_store = [&](double* da, double* db) {
    if (pa == 1) {
      if constexpr (A_KC) store_kc<TM, false>(da, tid, ra, 0); else store_mc<TM, BK, false, NTH>(da, tid, ra, 0);
    } else {
      if constexpr (A_KC) store_kc<TM, true>(da, tid, ra, ka); else store_mc<TM, BK, true, NTH>(da, tid, ra, ka);
    }
    if (pb == 1) {
      if constexpr (B_KC) store_kc<TN, false>(db, tid, rb, 0); else store_mc<TN, BK, false, NTH>(db, tid, rb, 0);
    } else {
      if constexpr (B_KC) store_kc<TN, true>(db, tid, rb, kb_); else store_mc<TN, BK, true, NTH>(db, tid, rb, kb_);
    }
  };

  // chunk c covers k in [kpos(c), kpos(c)+BK).  With k_reverse the chunks run from the top of the range down, so that
  // tiles whose ranges END together (klo differs per column tile, e.g. X^T * lower-triangular) sweep the shared
  // operand in lockstep and hit in L2 instead of each streaming its own k rows.
  auto kpos = [&](int c) { return p.k_reverse ? klo + (nch - 1 - c) * BK : klo + c * BK; };
  if (nch > 0) {
    stage_load(kpos(0));
    stage_store(smem, smem + OPA);
  }
  __syncthreads();

  auto compute = [&](int cur) {
    // v_mfma_f64_16x16x4_f64: lane (i = l&15, k = l>>4) supplies A[row i][k] and B[k][col i]; one instruction yields a
    // 16 x 16 block of C.  Per k-step of 4 a 64 x 64 wave tile takes 4 + 4 fragment reads for 16 MFMAs.
    const double* sa = smem + cur * (OPA + OPB) + (A_KC ? (wm + li) * LDK + lk : wm + li + lk * LDA);
    const double* sb = smem + cur * (OPA + OPB) + OPA + (B_KC ? (wn + li) * LDK + lk : wn + li + lk * LDB);
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      double bf[CB], af[RB / 4];
#pragma unroll
      for (int b = 0; b < CB; ++b) bf[b] = B_KC ? sb[16 * b * LDK + kk * 4] : sb[kk * 4 * LDB + 16 * b];
#pragma unroll
      for (int a = 0; a < RB / 4; ++a) af[a] = A_KC ? sa[16 * a * LDK + kk * 4] : sa[kk * 4 * LDA + 16 * a];
#pragma unroll
      for (int a = 0; a < RB / 4; ++a)
#pragma unroll
        for (int b = 0; b < CB; ++b)
          acc4[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf[b], acc4[a][b], 0, 0, 0);
    }
  };

  // Chunks whose loads are interior for BOTH operands form one contiguous range of k (each operand's condition is an
  // interval in kb).  Iterations that prefetch such a chunk run a branch-free body (lean loads, plain stores): one basic
  // block, so the compiler can spread the memory instructions over the MFMAs and the wave spends no issue slots on
  // the path selection (~100 scalar instructions per chunk).
  int ca = 0, cb = 0;  // clean iterations: ca <= c < cb
  // (big tile only, SPLIT above: the small tiles run a handful of chunks per launch and lose more to the second loop's code)
  if constexpr (SPLIT) {
    if (row0 + TM <= Mld && col0 + TN <= Nld && nch > 1) {
      int k_lo = klo, k_hi = khi;  // chunk [kb, kb+BK) is interior iff k_lo <= kb and kb + BK <= k_hi
      if (p.a_mask == 1) k_hi = min(k_hi, row0 + 1);
      if (p.a_mask == 2) k_lo = max(k_lo, row0 + TM - 1);
      if (p.b_mask == 1) k_hi = min(k_hi, col0 + 1);
      if (p.b_mask == 2) k_lo = max(k_lo, col0 + TN - 1);
      // chunk positions are klo + j*BK, j = c (forward) or nch-1-c (reverse)
      int j_lo = (k_lo - klo + BK - 1) / BK, j_hi = (k_hi - klo) / BK;  // interior positions j_lo <= j < j_hi
      j_lo = max(j_lo, 0);
      j_hi = min(j_hi, nch);
      if (j_hi > j_lo) {
        const int ci_lo = p.k_reverse ? nch - j_hi : j_lo, ci_hi = p.k_reverse ? nch - j_lo : j_hi;  // chunk indices
        ca = max(ci_lo - 1, 0);          // iteration c prefetches chunk c + 1
        cb = min(ci_hi - 1, nch - 1);
        if (cb < ca) ca = cb = 0;
      }
    }
  }
  auto general_iter = [&](int c) {
    const int cur = (NBUF == 2) ? (c & 1) : 0;
    const bool more = (c + 1 < nch);
    if (more) stage_load(kpos(c + 1));
    compute(cur);
    if (NBUF == 1) __syncthreads();  // everyone has read this chunk: the single buffer may take the next one
    if (more) {
      const int nxt = (NBUF == 2) ? (cur ^ 1) : 0;
      stage_store(smem + nxt * (OPA + OPB), smem + nxt * (OPA + OPB) + OPA);
    }
    __syncthreads();
  };
  int c = 0;
  for (; c < ca; ++c) general_iter(c);
  if constexpr (SPLIT && !PIPE) {
    for (; c < cb; ++c) {
      const int cur = c & 1, nxt = cur ^ 1;
      const int kb = kpos(c + 1);
      load_fast<NVA>(ubaseA + (int64_t)kb * stepA, offa, ra);
      load_fast<NVB>(ubaseB + (int64_t)kb * stepB, offb, rb);
      compute(cur);
      store_mc<TM, BK, false, NTH>(smem + nxt * (OPA + OPB), tid, ra, 0);
      store_mc<TN, BK, false, NTH>(smem + nxt * (OPA + OPB) + OPA, tid, rb, 0);
      __syncthreads();
    }
  }
  if constexpr (PIPE) {
    if (c < cb) {
      // The clean loop is software-pipelined by hand: the staging of chunk c + 1 runs UNDER the 64 MFMAs of chunk c, so that only
      // the barrier and the first fragment reads separate two chunks' MFMAs (before, ~90 instructions, eight vmcnt waits and an
      // LDS round trip sat in series between them, once per chunk and wave, and the four waves of a work-group meet at the
      // barrier: profiles/EXPERIMENTS.md).  The body is ONE basic block; its order is pinned with sched_group_barrier:
      //   k-step 0: the 8 global loads of chunk c + 1, one per MFMA
      //   k-step 2: the 4 LDS stores of A, each behind the vmcnt that covers its own load, in the k-step's second half
      //   k-step 3: the 4 LDS stores of B in its first half; nothing but loop control between the last MFMA and the barrier
      //   every k-step but the last: the fragment reads of the next one.
      // The `nxt` buffer has been free since the barrier that ended chunk c - 1, so the stores need no barrier of their own.
      // The loads address  uniform base (two SGPR pairs, advanced by a scalar add per chunk) + the thread's 32-bit offset; the
      // empty asm keeps the offsets' zero-extension inside the loop, where instruction selection folds it into the load's
      // SGPR-base form (hoisted, it costs 8 more VGPRs and a 64-bit VALU add per load and chunk).
      // MFMA order (kk, a, b) and fragment read order are those of compute(): the same bits.
      static_assert(!SPLIT || (TM == TN && LDA == LDB && NTH % (TM / 2) == 0), "the clean loop assumes the square row-contiguous tile");
      constexpr int RPV = NTH / (TM / 2);  // LDS rows between a thread's consecutive staging vectors: (tid + NTH i) / (T/2) = tid / (T/2) + RPV i
      auto uniform_ptr = [](const double* q) {
        const uint64_t u = reinterpret_cast<uint64_t>(q);  // work-group uniform by construction (tile indices, product descriptor)
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
        return reinterpret_cast<gchar*>(((uint64_t)hi << 32) | lo);  // (an integer cast would yield a generic pointer: flat loads)
      };
      const int kb1 = kpos(c + 1);
      gchar* ua = uniform_ptr(ubaseA + (int64_t)kb1 * stepA);
      gchar* ub = uniform_ptr(ubaseB + (int64_t)kb1 * stepB);
      const int64_t dk = p.k_reverse ? -(int64_t)BK : (int64_t)BK;
      const int64_t inca = dk * stepA * 8, incb = dk * stepB * 8;  // bytes per chunk
      // one register each for the thread's LDS positions (the asm keeps hipcc from re-deriving them from wave / lane parts per chunk)
      int wofs = (tid / (TM / 2)) * LDA + ((tid % (TM / 2)) << 1);
      int rofa = wm + li + lk * LDA, rofb = OPA + wn + li + lk * LDB;
      asm("" : "+v"(wofs), "+v"(rofa), "+v"(rofb));
      for (; c < cb; ++c) {
        const int cur = c & 1;
        const double* sa = smem + cur * (OPA + OPB) + rofa;
        const double* sb = smem + cur * (OPA + OPB) + rofb;
        int wpos = (cur ^ 1) * (OPA + OPB) + wofs;
#pragma unroll
        for (int i = 0; i < NVA; ++i) asm("" : "+v"(offa[i]));
#pragma unroll
        for (int i = 0; i < NVB; ++i) asm("" : "+v"(offb[i]));
        // raised wave priority over the MFMA phase, now the whole body: worth 0.5 ms of C2's 125 in the TAG != 0 kernels (LAUUM, the
        // post_cross products; profiles/r08_ab_setprio_gemm_pipeline.txt).  TAG 0 stays without: around the plain loop it was
        // nothing for gpp_trtri's masked merges and -3 % for the look-ahead factorisation's concurrent streams.
        if constexpr (TAG != 0 && GPP_CLEAN_SETPRIO) __builtin_amdgcn_s_setprio(1);
        double af[BK / 4][RB / 4], bf[BK / 4][CB];
        auto frag_b = [&](int kk) {
#pragma unroll
          for (int b = 0; b < CB; ++b) bf[kk][b] = sb[kk * 4 * LDB + 16 * b];
        };
        auto frag_a = [&](int kk, int a0) {  // rows a0, a0 + 1
#pragma unroll
          for (int a = a0; a < a0 + 2; ++a) af[kk][a] = sa[kk * 4 * LDA + 16 * a];
        };
        auto mfma_rows = [&](int kk, int a0) {
#pragma unroll
          for (int a = a0; a < a0 + 2; ++a)
#pragma unroll
            for (int b = 0; b < CB; ++b)
              acc4[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[kk][a], bf[kk][b], acc4[a][b], 0, 0, 0);
        };
        // Each store goes through a position the compiler cannot see through (the asm), so it may alias the store before it and the
        // fragment reads around it: the source order of the LDS accesses below is the order they are scheduled in.
        auto stage = [&](int ofs, const v2d& v) {
          asm("" : "+v"(wpos));
          *reinterpret_cast<v2d*>(smem + wpos + ofs) = v;
        };
        frag_b(0);
        frag_a(0, 0);
        frag_a(0, 2);
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
          if (kk + 1 < BK / 4) frag_b(kk + 1);
          if (kk == BK / 4 - 1) {
#pragma unroll
            for (int i = 0; i < NVB; ++i) stage(OPA + i * RPV * LDB, rb[i]);
          }
          mfma_rows(kk, 0);
          if (kk == 0) {
#pragma unroll
            for (int i = 0; i < NVA; ++i) ra[i] = *reinterpret_cast<gv2d*>(ua + offa[i]);
#pragma unroll
            for (int i = 0; i < NVB; ++i) rb[i] = *reinterpret_cast<gv2d*>(ub + offb[i]);
            ua += inca;
            ub += incb;
          }
          if (kk + 1 < BK / 4) frag_a(kk + 1, 0);
          if (kk == BK / 4 - 2) {
#pragma unroll
            for (int i = 0; i < NVA; ++i) stage(i * RPV * LDA, ra[i]);
          }
          if (kk + 1 < BK / 4) frag_a(kk + 1, 2);
          mfma_rows(kk, 2);
        }
        // The pinned order (masks: 0x8 MFMA, 0x20 VMEM read, 0x100 DS read, 0x200 DS write; two fragment reads are one
        // ds_read2_b64: B pair, B pair, A pair, A pair per k-step).  The next k-step's A rows 0-1 are read once this k-step's rows
        // 0-1 are done (MFMA 8) and its rows 2-3 at the top of the next k-step, so they take over the registers of the rows they
        // replace: one and a half fragment sets live, not two (8 VGPRs, which gpp_dag_f64 does not have).
        static_assert(BK == 16 && RB / 4 * CB == 16 && NVA == 4 && NVB == 4, "the schedule below is written out for 4 k-steps of 16 MFMAs");
#define GPP_SG(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)
#define GPP_SG_NEXT_B GPP_SG(0x8, 1); GPP_SG(0x100, 1); GPP_SG(0x8, 1); GPP_SG(0x100, 1)  // 2 MFMAs, B of the next k-step
#define GPP_SG_PAIR(mask, m) GPP_SG(mask, 1); GPP_SG(0x8, m)
        GPP_SG(0x100, 4);  // k-step 0: its own fragments,
        GPP_SG_NEXT_B;
        GPP_SG_PAIR(0x20, 1); GPP_SG_PAIR(0x20, 1); GPP_SG_PAIR(0x20, 1); GPP_SG_PAIR(0x20, 1); GPP_SG_PAIR(0x20, 1); GPP_SG_PAIR(0x20, 1);
        GPP_SG(0x100, 1);  // (A rows 0-1 of k-step 1)
        GPP_SG_PAIR(0x20, 1); GPP_SG_PAIR(0x20, 1);  // the global loads of chunk c + 1, one per MFMA
        GPP_SG(0x8, 6);
        GPP_SG(0x100, 1);  // k-step 1 (its A rows 2-3)
        GPP_SG_NEXT_B;
        GPP_SG(0x8, 6);
        GPP_SG(0x100, 1);
        GPP_SG(0x8, 8);
        GPP_SG(0x100, 1);  // k-step 2
        GPP_SG_NEXT_B;
        GPP_SG(0x8, 6);
        GPP_SG(0x100, 1);
        GPP_SG_PAIR(0x200, 2); GPP_SG_PAIR(0x200, 2); GPP_SG_PAIR(0x200, 2); GPP_SG_PAIR(0x200, 2);  // the LDS stores of A
        GPP_SG(0x100, 1);  // k-step 3
        GPP_SG_PAIR(0x200, 2); GPP_SG_PAIR(0x200, 2); GPP_SG_PAIR(0x200, 2); GPP_SG_PAIR(0x200, 2);  // the LDS stores of B
        GPP_SG(0x8, 8);
#undef GPP_SG_PAIR
#undef GPP_SG_NEXT_B
#undef GPP_SG
        if constexpr (TAG != 0 && GPP_CLEAN_SETPRIO) __builtin_amdgcn_s_setprio(0);
        __syncthreads();
      }
    }
  }
  for (; c < nch; ++c) general_iter(c);
  before_epilogue();
  if constexpr (!__is_same(E, GemmStoreC)) {
    static_assert((VAR == 2 || VAR == 0) && WTM == 64 && WTN == 64 && WR == 2, "accumulator epilogues are written for the big tile");
    epi(acc4, row0, col0, p.M, smem);  // (every wave is past the barrier behind the last chunk's LDS reads)
    return;
  }

  // epilogue: slab (a,b) holds C[row0+wm+4a+(l>>4)][col0+wn+16b+(l&15)].  The beta path first issues all C loads of a
  // group of slabs (clamped addresses, no branches around loads) and only then combines and stores.
  const double alpha = p.alpha, beta = p.beta;
  constexpr int GA = RB < 4 ? RB : 4;  // slab rows per group
#pragma unroll
  for (int a0 = 0; a0 < RB; a0 += GA) {
    double cold[GA][CB];
    if (beta != 0.0) {
#pragma unroll
      for (int a = 0; a < GA; ++a) {
        const int m = row0 + wm + 4 * (a0 + a) + lk;
#pragma unroll
        for (int b = 0; b < CB; ++b) {
          const int n = col0 + wn + 16 * b + li;
          const bool ok = (m < p.M) && (n < p.N) && (p.c_lower == 0 || (p.c_lower == 1 ? n <= m : n >= m));
          const double* src = ok ? C + (int64_t)m * p.ldc + n : Cd;
          cold[a][b] = *src;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < GA; ++a) {
      const int m = row0 + wm + 4 * (a0 + a) + lk;
#pragma unroll
      for (int b = 0; b < CB; ++b) {
        const int n = col0 + wn + 16 * b + li;
        const bool ok = (m < p.M) && (n < p.N) && (p.c_lower == 0 || (p.c_lower == 1 ? n <= m : n >= m));
        double v = alpha * acc4[(a0 + a) >> 2][b][(a0 + a) & 3];
        if (beta != 0.0) v = fma(beta, cold[a][b], v);
        if (ok) {
          C[(int64_t)m * p.ldc + n] = v;
          if (C2)  // mirrored (transposed) copy
            C2[(int64_t)n * p.ldc2 + m] = v;
        }
      }
    }
  }
}

template <int VAR, int WTM, int WTN, int TAG = 0, int BK = 16, int NBUF = 2, int WR = 2>
__global__ __launch_bounds__(128 * WR, ((VAR == 2 && !(BK > 16 && WTM >= 64)) || WTM < 64) ? 2 : 1) void gpp_gemm_f64(GemmArgs p) {
  constexpr int TM = WR * WTM, TN = 2 * WTN;  // work-group tile: TM rows x TN columns (WR x 2 waves)
  extern __shared__ __attribute__((aligned(16))) double smem[];  // NBUF * 2 * OPSZ doubles (see gemm_lds_bytes)
  int tm, tn;
  if (p.swz) {
    // XCD-aware mapping (blocks are dealt round-robin to the 8 XCDs, each with a private 4 MiB L2): the 64 work-groups
    // an XCD runs concurrently (32 CUs x 2) form ONE 8 x 8 super-tile of output tiles, so every staged A chunk is
    // shared by 8 and every B chunk by 8 work-groups of that L2.  Tiles outside the matrix / triangle exit at once.
    const int b = blockIdx.x, xcd = b & 7, i = b >> 3;
    const int S = (i >> 6) * 8 + xcd, w = i & 63;
    const int super_n = (p.tiles_n + 7) >> 3;
    const int sm = S / super_n, sn = S - sm * super_n;
    tm = sm * 8 + (w >> 3);
    tn = sn * 8 + (w & 7);
    if (tm >= p.tiles_m || tn >= p.tiles_n) return;
    if ((p.c_lower == 1 && tn > tm) || (p.c_lower == 2 && tn < tm)) return;
  } else {
    const int t = (p.batch_fast ? (int)(blockIdx.x / (unsigned)p.nbatch) : (int)blockIdx.x) + (int)p.tile_base;
    if (p.c_lower == 1 && p.row_mod >= 1) {
      // owned tile rows tm = row_off + row_mod * i, row i has tm + 1 tiles: S(i) = i (row_off + 1) + row_mod i (i-1) / 2
      const float a = 0.5f * (float)p.row_mod, b = (float)p.row_off + 1.f - a;
      int i = (int)((-b + sqrtf(b * b + 4.f * a * (float)t)) / (2.f * a));
      auto S = [&](int q) { return q * (p.row_off + 1) + p.row_mod * (q * (q - 1) / 2); };
      while (S(i + 1) <= t) ++i;
      while (S(i) > t) --i;
      tm = p.row_off + p.row_mod * i;
      tn = t - S(i);
    } else if (p.c_lower == 1 && TM == 2 * TN) {
      // tall tiles, lower triangle: tile row tm (TM rows) has the column tiles 0 .. 2 tm + 1; S(tm) = tm (tm + 1) tiles precede it
      tm = (int)((sqrtf(4.f * (float)t + 1.f) - 1.f) * 0.5f);
      while ((tm + 1) * (tm + 2) <= t) ++tm;
      while (tm * (tm + 1) > t) --tm;
      tn = t - tm * (tm + 1);
      if (tn >= p.tiles_n) return;
    } else if (p.c_lower) {
      tm = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
      while ((tm + 1) * (tm + 2) / 2 <= t) ++tm;
      while (tm * (tm + 1) / 2 > t) --tm;
      tn = t - tm * (tm + 1) / 2;
      // lower triangle, column blocks owned block-cyclically (the sharded back-substitution): another rank's column block
      if (p.c_lower == 1 && p.own_mod > 1 && (tn / p.own_bt + p.own_off) % p.own_mod != 0) return;
      if (p.c_lower == 2) {  // upper triangle: same enumeration, mirrored tile
        const int q = tm;
        tm = tn;
        tn = q;
        if (p.own_mod > 1 && (tm / p.own_bt + p.own_off) % p.own_mod != 0) return;  // another rank's block row
        if ((tn + 1) * TN <= p.skip_lead) return;  // (tm <= tn) inside the leading block another launch has updated
        if (p.row_limit > 0 && tm * TM >= p.row_limit) return;  // below the trapezoid this launch produces
      }
    } else if (p.col_major) {
      // column-major tile order: consecutive work-groups share the column tile (hence the K range when it depends on
      // the column, and the B chunks) and run in lockstep
      tn = t / p.tiles_m;
      tm = t - tn * p.tiles_m;
    } else {
      tm = t / p.tiles_n;
      tn = t - tm * p.tiles_n;
      if (p.row_reverse) tm = p.tiles_m - 1 - tm;  // longest K ranges (khi grows with the row) first: short tail
    }
  }
  const int64_t bi = p.batch_fast ? (int64_t)(blockIdx.x % (unsigned)p.nbatch) : (int64_t)blockIdx.y;  // batch element
  gemm_tile<VAR, WTM, WTN, TAG, BK, NBUF, WR>(p, tm, tn, p.A + bi * p.sA + (int64_t)blockIdx.z * p.zA, p.B + bi * p.sB + (int64_t)blockIdx.z * p.zB,
                                             p.C + bi * p.sC + (int64_t)blockIdx.z * p.zC,
                                             p.C2 ? p.C2 + bi * p.sC2 + (int64_t)blockIdx.z * p.zC2 : nullptr, smem);

}

// ---- LAUUM with the gradient reduction as its epilogue (gpp_lauum_grad in gpp.h) ---------------------------------------------
// The accumulators of a lower-triangular 128 x 128 tile of Ky^-1 = Linv^T Linv never reach memory: each entry goes straight into
// the sums gpp_grad_tiles (gpp_reduce.hip) defines — W_ij = 0.5 (alpha_i alpha_j - Kinv_ij), mult = 2 below the diagonal,
//    g_w[d] += mult W_ij sf2 k_ij (-(u_id - u_jd)^2)        g_sf2 += mult W_ij k_ij        wdiag[i] = W_ii
// with k_ij = exp(-sum_d w_d (u_id - u_jd)^2) recomputed from the tile's raw feature rows / columns, which are staged with the
// alpha segments in the LDS the main loop has finished with.  A lane holds rows 16 a4 + 4 v + (l >> 4) and columns 16 b + (l & 15)
// of its wave's quadrant.  The arithmetic runs in a ROLLED loop over half-slabs of 2 rows x 4 columns per lane (fully unrolled
// over the 64 entries it is ~40 KiB of code per tile): the 16 values of slab a4 pass through lane-private LDS slots, which turns
// the accumulator index into an address (no barrier: a lane reads back only what it wrote).
// Deterministic: per-lane sums in a fixed order, a fixed butterfly over each wave, the four wave sums added in order, ONE record
// of D + 1 doubles per tile (every slot written exactly once), summed by gpp_grad_finish in a fixed order.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <int DT>
struct GradEpilogue {
  GradEpiArgs e;
  int tile;
  static constexpr int T = 128;
  static constexpr int FIXED = 2 * DT * T + 2 * T + DT + 4 * (DT + 1);  // doubles in front of the slab
  static constexpr int SLAB = (FIXED + 1) & ~1;
  static_assert((SLAB + 16 * 256) * sizeof(double) <= 2 * 2 * BK16 * ldt_mc(T) * sizeof(double), "the epilogue lives in the main loop's LDS");
  __device__ __forceinline__ void operator()(const v4d (&acc4)[4][4], int row0, int col0, int N, double* __restrict__ smem) const {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, li = lane & 15, lk = lane >> 4;
    const int D = e.D;
    double* __restrict__ sa = smem;            // raw features of the tile's rows, [d][r]
    double* __restrict__ sb = sa + DT * T;     // ... of its columns
    double* __restrict__ sal_a = sb + DT * T;  // alpha of the rows / columns
    double* __restrict__ sal_b = sal_a + T;
    double* __restrict__ sw = sal_b + T;
    double* __restrict__ red = sw + DT;        // [4 waves][DT + 1]
    double* __restrict__ slab = smem + SLAB;   // [16 values][256 lanes]
    for (int x = tid; x < DT * T; x += 256) {
      const int d = x / T, r = x - d * T;
      sa[x] = (d < D && row0 + r < N) ? e.U[(int64_t)(row0 + r) * D + d] : 0.0;
      sb[x] = (d < D && col0 + r < N) ? e.U[(int64_t)(col0 + r) * D + d] : 0.0;
    }
    if (tid < T) {
      sal_a[tid] = (row0 + tid < N) ? e.alpha[row0 + tid] : 0.0;
      sal_b[tid] = (col0 + tid < N) ? e.alpha[col0 + tid] : 0.0;
    }
    if (tid < DT) sw[tid] = (tid < D) ? e.w[tid] : 0.0;
    __syncthreads();

    const double sf2 = *e.sf2;
    const GppExpConsts ec = gpp_exp_consts();
    const bool diag_tile = (row0 == col0);
    double my_sf2 = 0.0, my_w[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) my_w[d] = 0.0;
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int b = 0; b < 4; ++b) slab[(v * 4 + b) * 256 + tid] = acc4[a4][b][v];
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const int ra = wm + 16 * a4 + 8 * h + lk;  // this half's rows inside the tile: ra and ra + 4
        const int cb = wn + li;                    // its columns: cb + 16 b
        double r2[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
#pragma unroll 2
        for (int d = 0; d < DT; ++d) {
          const double ua[2] = {sa[d * T + ra], sa[d * T + ra + 4]};
          const double wd = sw[d];
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double ub = sb[d * T + cb + 16 * b];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
              const double df = ua[a] - ub;
              r2[a][b] = fma(wd * df, df, r2[a][b]);
            }
          }
        }
        // compiler barrier: the second pass reads the features again instead of keeping them live across the exp section (gpp_grad_tiles)
        __asm__ volatile("" ::: "memory");
        double g2[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const int i = row0 + ra + 4 * a;
          const double al_i = sal_a[ra + 4 * a];
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int j = col0 + cb + 16 * b;
            const bool ok = (i < N) & (j <= i);  // as the store of C masks them: beyond N, above the diagonal
            const double kv = gpp_exp_nonpos(-r2[a][b], ec);
            const double kin = slab[((2 * h + a) * 4 + b) * 256 + tid];
            double Wij = 0.5 * (al_i * sal_b[cb + 16 * b] - kin);
            Wij = ok ? Wij : 0.0;  // (a select: whatever the accumulator of a masked entry holds never reaches a sum)
            const double mult = (i == j) ? 1.0 : 2.0;
            my_sf2 = fma(mult * Wij, kv, my_sf2);
            g2[a][b] = mult * Wij * sf2 * kv;
            if (diag_tile && ok && i == j) e.wdiag[i] = Wij;
          }
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          const double ua[2] = {sa[d * T + ra], sa[d * T + ra + 4]};
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double ub = sb[d * T + cb + 16 * b];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
              const double df = ua[a] - ub;
              s = fma(-g2[a][b] * df, df, s);
            }
          }
          my_w[d] += s;
          __builtin_amdgcn_sched_barrier(0);  // (keeps the LDS reads of later features from being hoisted: 6 registers each)
        }
      }
    }
#pragma unroll
    for (int q = 0; q <= DT; ++q) {
      const double v = wave_sum(q < DT ? my_w[q < DT ? q : 0] : my_sf2);
      if (lane == 0) red[wave * (DT + 1) + q] = v;
    }
    __syncthreads();
    if (tid <= D) {
      const int q = (tid == D) ? DT : tid;
      e.rec[(int64_t)tile * (D + 1) + tid] = ((red[q] + red[(DT + 1) + q]) + red[2 * (DT + 1) + q]) + red[3 * (DT + 1) + q];
    }
  }
};

// one work-group per lower-triangular tile, in gpp_gemm_f64's plain row-by-row enumeration
template <int DT>
__global__ __launch_bounds__(256, 2) void gpp_lauum_grad_f64(GemmArgs p, GradEpiArgs e) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = (int)blockIdx.x;
  int tm = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while ((tm + 1) * (tm + 2) / 2 <= t) ++tm;
  while (tm * (tm + 1) / 2 > t) --tm;
  const int tn = t - tm * (tm + 1) / 2;
  gemm_tile<2, 64, 64, 2, 16, 2, 2>(p, tm, tn, p.A, p.B, nullptr, nullptr, smem, GemmNoHook(), GradEpilogue<DT>{e, t});
}

// ---- Vc Vr^T with the weighted squared posterior cross-covariance as its epilogue (gpp_post_cross_sq in gpp.h) -------------------
// Entry (c, r) of a 128 x 128 tile of Vc Vr^T never reaches memory: the epilogue regenerates g = sf2 k(Uc_c, Ur_r; w) with the
// arithmetic of gpp_cov_tile (features staged times sqrt(w_d), r2 summed by fma in the order of d, gpp_kernel_value), forms
// omega_r (g - acc)^2 and sums it along the tile's columns.  The slab idiom of GradEpilogue: the 16 values of slab a4 pass through
// lane-private LDS slots, the arithmetic runs in a rolled loop over half-slabs of 2 rows x 4 columns per lane.  The features are
// staged DC dims at a time: D <= DC once for the whole tile; above, every half-slab walks the chunks (two barriers per chunk — the
// r2 sums of a half-slab stay in registers, so the tile's 64 entries per lane never need D-many staged dims at once; the re-read
// feature rows are L2-resident and ~1 MB per tile at D = 64 against the 2 x 128 x K doubles of the main loop).
// Deterministic, and the same for every row of the tile: a lane adds its 4 columns (16 b + li) in the order of b, a fixed butterfly
// adds the 16 lanes of a row, the two column halves (waves) are added in order — ONE record of 128 row sums per tile, every slot
// written exactly once, summed over the column tiles by gpp_post_cross_finish (gpp_alc.hip) in index order.
template <bool MAT>
struct PostCrossEpilogue {
  PostCrossArgs e;
  int tile, Mr;
  static constexpr int T = 128, DC = 16;
  static constexpr int SLAB = 2 * DC * T + T + 2 * T;  // doubles in front of the slab
  static_assert((SLAB & 1) == 0 && (SLAB + 16 * 256) * sizeof(double) <= 2 * 2 * BK16 * ldt_mc(T) * sizeof(double) &&
                    (SLAB + 16 * 256) * sizeof(double) <= 2 * 2 * T * LDK * sizeof(double),
                "the epilogue lives in the main loop's LDS");
  __device__ __forceinline__ void operator()(const v4d (&acc4)[4][4], int row0, int col0, int Mc, double* __restrict__ smem) const {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, li = lane & 15, lk = lane >> 4;
    const int D = e.dk & 255, kind = (e.dk >> 8) & 255;
    const int dsp = (!MAT || kind == 0) ? D : (e.dk >> 16);  // dims below go to the RBF factor, the others to the Matern factor
    double* __restrict__ sa = smem;           // staged features of the tile's rows (candidates), [d][r], times sqrt(w_d)
    double* __restrict__ sb = sa + DC * T;    // ... of its columns (reference points)
    double* __restrict__ som = sb + DC * T;   // omega of the columns, 0 beyond M_r
    double* __restrict__ rs = som + T;        // [2 column halves][T] row sums
    double* __restrict__ slab = smem + SLAB;  // [16 values][256 lanes]
    // (what the staging of a later chunk and the record need is parked in VGPRs: with the exponential's 28 constant SGPRs on top
    //  of the tile body's own, the scalar file would spill)
    const double* __restrict__ Uc = e.Uc;
    const double* __restrict__ Ur = e.Ur;
    const double* __restrict__ wp = e.w;
    double* __restrict__ rec = e.rec + (int64_t)tile * T;
    Uc += (int64_t)row0 * (e.dk & 255);
    Ur += (int64_t)col0 * (e.dk & 255);
    int rlim = Mc - row0, clim = Mr - col0;  // rows / columns of the tile inside the block
    asm volatile("" : "+v"(Uc), "+v"(Ur), "+v"(wp), "+v"(rec), "+v"(rlim), "+v"(clim));
    auto stage = [&](int d0) {
      for (int x = tid; x < DC * T; x += 256) {
        const int dd = x / T, r = x - dd * T, d = d0 + dd;
        const bool okd = d < D;
        const double sw = okd ? sqrt(wp[okd ? d : 0]) : 0.0;
        sa[x] = (okd && r < rlim) ? Uc[r * D + d] * sw : 0.0;
        sb[x] = (okd && r < clim) ? Ur[r * D + d] * sw : 0.0;
      }
    };
    if (tid < T) som[tid] = (tid < clim) ? (e.omega ? e.omega[col0 + tid] : 1.0) : 0.0;
    const bool one = (D <= DC);  // work-group uniform
    if (one) stage(0);
    __syncthreads();

    const double sf2 = *e.sf2;
    const GppExpConsts ec = gpp_exp_consts();
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int b = 0; b < 4; ++b) slab[(v * 4 + b) * 256 + tid] = acc4[a4][b][v];
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const int ra = wm + 16 * a4 + 8 * h + lk;  // this half's rows inside the tile: ra and ra + 4
        const int cb = wn + li;                    // its columns: cb + 16 b
        double r2[2][4], r2m[MAT ? 2 : 1][MAT ? 4 : 1];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            r2[a][b] = 0.0;
            if (MAT) r2m[MAT ? a : 0][MAT ? b : 0] = 0.0;
          }
#pragma unroll 1
        for (int d0 = 0; d0 < D; d0 += DC) {
          if (!one) {
            __syncthreads();  // (every wave has read the previous chunk)
            stage(d0);
            __syncthreads();
          }
          const int nd = min(DC, D - d0);
#pragma unroll 2
          for (int dd = 0; dd < nd; ++dd) {
            const double ua[2] = {sa[dd * T + ra], sa[dd * T + ra + 4]};
            const bool second = MAT && (d0 + dd >= dsp);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const double ub = sb[dd * T + cb + 16 * b];
#pragma unroll
              for (int a = 0; a < 2; ++a) {
                const double df = ua[a] - ub;
                if (MAT && second) r2m[MAT ? a : 0][MAT ? b : 0] = fma(df, df, r2m[MAT ? a : 0][MAT ? b : 0]);
                else r2[a][b] = fma(df, df, r2[a][b]);
              }
            }
          }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double kv = MAT ? gpp_kernel_value(kind, r2[a][b], r2m[MAT ? a : 0][MAT ? b : 0], ec) : gpp_exp_nonpos(-r2[a][b], ec);
            const double c = sf2 * kv - slab[((2 * h + a) * 4 + b) * 256 + tid];
            double t = c * c;
            t = (cb + 16 * b < clim) ? t : 0.0;  // (a select: whatever a column beyond M_r holds never reaches a sum)
            s = fma(som[cb + 16 * b], t, s);
          }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);  // the 16 lanes (li) that share this row
          if (li == 0) rs[(wave & 1) * T + ra + 4 * a] = s;
        }
      }
    }
    __syncthreads();
    if (tid < T) rec[tid] = rs[tid] + rs[T + tid];
  }
};

// one work-group per tile of the M_c x M_r block, row by row (consecutive work-groups share the candidates' chunks)
template <int VAR, bool MAT>
__global__ __launch_bounds__(256, VAR == 2 ? 2 : 1) void gpp_post_cross_f64(GemmArgs p, PostCrossArgs e) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = (int)blockIdx.x;
  const int tm = t / p.tiles_n, tn = t - tm * p.tiles_n;
  gemm_tile<VAR, 64, 64, 2, 16, 2, 2>(p, tm, tn, p.A, p.B, nullptr, nullptr, smem, GemmNoHook(), PostCrossEpilogue<MAT>{e, t, p.N});
}

// ---- Vf Vr^T whose rows are linear functionals of f: value and gradient components (gpp_post_cross_lin_sq in gpp.h) -------------
// PostCrossEpilogue with a richer generator: row i observes a_0 f + sum_j a_j df/du_{dlo + j} at Uf_i, a = A[i][0 .. nd], so its
// prior covariance with f(Ur_r) is a_0 sf2 k + m_0 lin_0 + m_1 lin_1 with the multipliers of gpp_cross_kernel_dx (m_0 = -(e1 h),
// m_1 = e1 h', e1 = sf2 exp(-r2_rbf), h and h' from the ONE gpp_matern call that also gives k) and, per kernel factor f,
//   lin_f = sum over the observed dims d of factor f of (a_d g_d) (sa_d - sb_d),   g_d = 2 sqrt(w_d),
// one rounded product a_d g_d per row and dim and one fma per entry, inside the loop over the staged dims that sums r2 (same
// staging, same r2 order, same slab idiom, same record).  The entry is
//   c = fma(a_0 sf2, k, -acc);  c = fma(m_0, lin_0, c);  c = fma(m_1, lin_1, c)
// in this order: with a = (1, 0, ..., 0) the product a_0 sf2 is sf2, every lin is an exact +0 and adding a zero changes no bit of
// c^2 — such a row is bit for bit PostCrossEpilogue's (which the compiler contracts to fma(sf2, k, -acc) as well).  A feature with
// w_d == 0 has g_d == 0 and staged zeros; a row of Uf equal to a row of Ur has sa == sb in every dim: lin is an exact 0 either way.
// The coefficients do not fit beside the slab (a 128 x 17 table at two work-groups per CU): g_d is staged (DC doubles), a lane
// reads its two rows' a_d from global memory as the dims come by — M_f (1 + nd) doubles, L2-resident, 16 lanes per address.
template <bool MAT>
struct PostCrossLinEpilogue {
  PostCrossLinArgs e;
  int tile, Mr;
  static constexpr int T = 128, DC = 16;
  static constexpr int SLAB = 2 * DC * T + T + 2 * T + DC;  // doubles in front of the slab
  static_assert((SLAB & 1) == 0 && (SLAB + 16 * 256) * sizeof(double) <= 2 * 2 * BK16 * ldt_mc(T) * sizeof(double) &&
                    (SLAB + 16 * 256) * sizeof(double) <= 2 * 2 * T * LDK * sizeof(double),
                "the epilogue lives in the main loop's LDS");
  __device__ __forceinline__ void operator()(const v4d (&acc4)[4][4], int row0, int col0, int Mf, double* __restrict__ smem) const {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, li = lane & 15, lk = lane >> 4;
    const int D = e.dk & 255, kind = (e.dk >> 8) & 255;
    const int dsp = (!MAT || kind == 0) ? D : (e.dk >> 16);  // dims below go to the RBF factor, the others to the Matern factor
    const int dlo = e.dn & 255, dhi = dlo + (e.dn >> 8);     // the observed directions [dlo, dhi)
    double* __restrict__ sa = smem;           // staged features of the tile's rows (functionals), [d][r], times sqrt(w_d)
    double* __restrict__ sb = sa + DC * T;    // ... of its columns (reference points)
    double* __restrict__ som = sb + DC * T;   // omega of the columns, 0 beyond M_r
    double* __restrict__ rs = som + T;        // [2 column halves][T] row sums
    double* __restrict__ sg = rs + 2 * T;     // g_d = 2 sqrt(w_d) of the staged dims
    double* __restrict__ slab = smem + SLAB;  // [16 values][256 lanes]
    // (parked in VGPRs as in PostCrossEpilogue)
    const double* __restrict__ Uf = e.Uf;
    const double* __restrict__ Ur = e.Ur;
    const double* __restrict__ wp = e.w;
    const double* __restrict__ Ap = e.A + (int64_t)row0 * e.lda;
    double* __restrict__ rec = e.rec + (int64_t)tile * T;
    Uf += (int64_t)row0 * (e.dk & 255);
    Ur += (int64_t)col0 * (e.dk & 255);
    int rlim = Mf - row0, clim = Mr - col0;  // rows / columns of the tile inside the block
    int64_t lda = e.lda;
    asm volatile("" : "+v"(Uf), "+v"(Ur), "+v"(wp), "+v"(Ap), "+v"(lda), "+v"(rec), "+v"(rlim), "+v"(clim));
    auto stage = [&](int d0) {
      for (int x = tid; x < DC * T; x += 256) {
        const int dd = x / T, r = x - dd * T, d = d0 + dd;
        const bool okd = d < D;
        const double sw = okd ? sqrt(wp[okd ? d : 0]) : 0.0;
        sa[x] = (okd && r < rlim) ? Uf[r * D + d] * sw : 0.0;
        sb[x] = (okd && r < clim) ? Ur[r * D + d] * sw : 0.0;
        if (r == 0) sg[dd] = 2.0 * sw;
      }
    };
    if (tid < T) som[tid] = (tid < clim) ? (e.omega ? e.omega[col0 + tid] : 1.0) : 0.0;
    const bool one = (D <= DC);  // work-group uniform
    if (one) stage(0);
    __syncthreads();

    const double sf2 = *e.sf2;
    const GppExpConsts ec = gpp_exp_consts();
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int b = 0; b < 4; ++b) slab[(v * 4 + b) * 256 + tid] = acc4[a4][b][v];
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const int ra = wm + 16 * a4 + 8 * h + lk;  // this half's rows inside the tile: ra and ra + 4
        const int cb = wn + li;                    // its columns: cb + 16 b
        // the two rows' coefficients; a row beyond M_f has none (never read) and counts as all zeros
        const bool okr[2] = {ra < rlim, ra + 4 < rlim};
        const double* __restrict__ pa[2] = {Ap + (okr[0] ? ra : 0) * lda, Ap + (okr[1] ? ra + 4 : 0) * lda};
        double r2[2][4], r2m[MAT ? 2 : 1][MAT ? 4 : 1], lin[2][4], linm[MAT ? 2 : 1][MAT ? 4 : 1];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            r2[a][b] = 0.0;
            lin[a][b] = 0.0;
            if (MAT) r2m[MAT ? a : 0][MAT ? b : 0] = 0.0;
            if (MAT) linm[MAT ? a : 0][MAT ? b : 0] = 0.0;
          }
#pragma unroll 1
        for (int d0 = 0; d0 < D; d0 += DC) {
          if (!one) {
            __syncthreads();  // (every wave has read the previous chunk)
            stage(d0);
            __syncthreads();
          }
          const int nd = min(DC, D - d0);
#pragma unroll 1
          for (int dd = 0; dd < nd; ++dd) {
            const int d = d0 + dd;
            const double ua[2] = {sa[dd * T + ra], sa[dd * T + ra + 4]};
            const bool second = MAT && (d >= dsp);
            const bool obs = d >= dlo && d < dhi;  // (uniform)
            double t[2] = {0.0, 0.0};
            if (obs) {
              const double g = sg[dd];
#pragma unroll
              for (int a = 0; a < 2; ++a) t[a] = okr[a] ? pa[a][1 + d - dlo] * g : 0.0;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const double ub = sb[dd * T + cb + 16 * b];
#pragma unroll
              for (int a = 0; a < 2; ++a) {
                const double df = ua[a] - ub;
                if (MAT && second) r2m[MAT ? a : 0][MAT ? b : 0] = fma(df, df, r2m[MAT ? a : 0][MAT ? b : 0]);
                else r2[a][b] = fma(df, df, r2[a][b]);
                if (obs) {
                  if (MAT && second) linm[MAT ? a : 0][MAT ? b : 0] = fma(t[a], df, linm[MAT ? a : 0][MAT ? b : 0]);
                  else lin[a][b] = fma(t[a], df, lin[a][b]);
                }
              }
            }
          }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const double a0s = (okr[a] ? pa[a][0] : 0.0) * sf2;
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double ex = gpp_exp_nonpos(-r2[a][b], ec);
            const double e1 = sf2 * ex;
            double kv = ex, m0, m1 = 0.0;
            if (MAT) {
              const GppMatern m = gpp_matern(kind, r2m[MAT ? a : 0][MAT ? b : 0], ec);
              const double hm = m.p * m.er;
              kv = ex * hm;
              m0 = -(e1 * hm);
              m1 = e1 * (m.dp * m.er);
            } else {
              m0 = -e1;
            }
            double c = __builtin_fma(a0s, kv, -slab[((2 * h + a) * 4 + b) * 256 + tid]);
            c = __builtin_fma(m0, lin[a][b], c);
            if (MAT) c = __builtin_fma(m1, linm[MAT ? a : 0][MAT ? b : 0], c);
            double t = c * c;
            t = (cb + 16 * b < clim) ? t : 0.0;  // (a select: whatever a column beyond M_r holds never reaches a sum)
            s = fma(som[cb + 16 * b], t, s);
          }
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);  // the 16 lanes (li) that share this row
          if (li == 0) rs[(wave & 1) * T + ra + 4 * a] = s;
        }
      }
    }
    __syncthreads();
    if (tid < T) rec[tid] = rs[tid] + rs[T + tid];
  }
};

template <int VAR, bool MAT>
__global__ __launch_bounds__(256, VAR == 2 ? 2 : 1) void gpp_post_cross_lin_f64(GemmArgs p, PostCrossLinArgs e) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = (int)blockIdx.x;
  const int tm = t / p.tiles_n, tn = t - tm * p.tiles_n;
  gemm_tile<VAR, 64, 64, 2, 16, 2, 2>(p, tm, tn, p.A, p.B, nullptr, nullptr, smem, GemmNoHook(), PostCrossLinEpilogue<MAT>{e, t, p.N});
}

// ---- Vc Vr^T with the minima of affine images of the posterior cross-covariance as its epilogue (gpp_post_cross_min in gpp.h) -----
// The knowledge gradient's reduction: for every node k < Q, min_r (m_r + t_ck c_cr) with c = g - acc as in PostCrossEpilogue (the
// same staging, r2 order, exponential and Matern factors) and t_ck = nodes[k] * scale[c], one rounded product per row and node.
// The 8 entries of a half-slab (2 rows x 4 columns per lane) stay in registers while a rolled loop walks the nodes: per node and
// row 4 fma + min, then the 16-lane butterfly, after which every lane of the row holds the half-slab's final minimum — nothing is
// collected in LDS.  Lane li keeps node 16 j + li, so each group of 16 nodes leaves as one 128-byte store per row.  A column beyond
// M_r enters with c = 0 and m = +inf (selects): it yields +inf, never m_r + 0.  The two column halves (waves) record separately:
// rec[((tile 2 + half) 128 + row) Q + k], every slot written exactly once (rows beyond M_c too: they are never read);
// gpp_post_cross_min_finish (gpp_alc.hip) takes the minimum over a row's records in index order.  Minima are exact and
// order-independent, so no rounding depends on the tiling.
// (the scalar-file remark in PostCrossEpilogue holds here as well: the nodes sit in LDS, not behind a uniform pointer)
template <bool MAT>
struct PostCrossMinEpilogue {
  PostCrossMinArgs e;
  int tile, Mr;
  static constexpr int T = 128, DC = 16, QMAX = 64;
  static constexpr int SLAB = 2 * DC * T + 2 * T + QMAX;  // doubles in front of the slab
  static_assert((SLAB & 1) == 0 && (SLAB + 16 * 256) * sizeof(double) <= 2 * 2 * BK16 * ldt_mc(T) * sizeof(double) &&
                    (SLAB + 16 * 256) * sizeof(double) <= 2 * 2 * T * LDK * sizeof(double),
                "the epilogue lives in the main loop's LDS");
  __device__ __forceinline__ void operator()(const v4d (&acc4)[4][4], int row0, int col0, int Mc, double* __restrict__ smem) const {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, li = lane & 15, lk = lane >> 4;
    const int D = e.dk & 255, kind = (e.dk >> 8) & 255;
    const int dsp = (!MAT || kind == 0) ? D : ((e.dk >> 16) & 255);
    const int Q = e.dk >> 24;
    double* __restrict__ sa = smem;           // staged features of the tile's rows (candidates), [d][r], times sqrt(w_d)
    double* __restrict__ sb = sa + DC * T;    // ... of its columns (reference points)
    double* __restrict__ sm = sb + DC * T;    // m of the columns, +inf beyond M_r
    double* __restrict__ ss = sm + T;         // scale of the rows, 0 beyond M_c
    double* __restrict__ sz = ss + T;         // the nodes
    double* __restrict__ slab = smem + SLAB;  // [16 values][256 lanes]
    const double* __restrict__ Uc = e.Uc;
    const double* __restrict__ Ur = e.Ur;
    const double* __restrict__ wp = e.w;
    // this wave's records: column half (wave & 1) of the tile
    double* __restrict__ rec = e.rec + ((int64_t)tile * 2 + (wave & 1)) * T * Q;
    Uc += (int64_t)row0 * (e.dk & 255);
    Ur += (int64_t)col0 * (e.dk & 255);
    int rlim = Mc - row0, clim = Mr - col0;  // rows / columns of the tile inside the block
    asm volatile("" : "+v"(Uc), "+v"(Ur), "+v"(wp), "+v"(rec), "+v"(rlim), "+v"(clim));
    auto stage = [&](int d0) {
      for (int x = tid; x < DC * T; x += 256) {
        const int dd = x / T, r = x - dd * T, d = d0 + dd;
        const bool okd = d < D;
        const double sw = okd ? sqrt(wp[okd ? d : 0]) : 0.0;
        sa[x] = (okd && r < rlim) ? Uc[r * D + d] * sw : 0.0;
        sb[x] = (okd && r < clim) ? Ur[r * D + d] * sw : 0.0;
      }
    };
    if (tid < T) sm[tid] = (tid < clim) ? e.m[col0 + tid] : __builtin_huge_val();
    else ss[tid - T] = (tid - T < rlim) ? e.scale[row0 + tid - T] : 0.0;
    if (tid < Q) sz[tid] = e.nodes[tid];
    const bool one = (D <= DC);  // work-group uniform
    if (one) stage(0);
    __syncthreads();

    const double sf2 = *e.sf2;
    const GppExpConsts ec = gpp_exp_consts();
#pragma unroll
    for (int a4 = 0; a4 < 4; ++a4) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int b = 0; b < 4; ++b) slab[(v * 4 + b) * 256 + tid] = acc4[a4][b][v];
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const int ra = wm + 16 * a4 + 8 * h + lk;  // this half's rows inside the tile: ra and ra + 4
        const int cb = wn + li;                    // its columns: cb + 16 b
        double r2[2][4], r2m[MAT ? 2 : 1][MAT ? 4 : 1];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            r2[a][b] = 0.0;
            if (MAT) r2m[MAT ? a : 0][MAT ? b : 0] = 0.0;
          }
#pragma unroll 1
        for (int d0 = 0; d0 < D; d0 += DC) {
          if (!one) {
            __syncthreads();  // (every wave has read the previous chunk)
            stage(d0);
            __syncthreads();
          }
          const int nd = min(DC, D - d0);
#pragma unroll 2
          for (int dd = 0; dd < nd; ++dd) {
            const double ua[2] = {sa[dd * T + ra], sa[dd * T + ra + 4]};
            const bool second = MAT && (d0 + dd >= dsp);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              const double ub = sb[dd * T + cb + 16 * b];
#pragma unroll
              for (int a = 0; a < 2; ++a) {
                const double df = ua[a] - ub;
                if (MAT && second) r2m[MAT ? a : 0][MAT ? b : 0] = fma(df, df, r2m[MAT ? a : 0][MAT ? b : 0]);
                else r2[a][b] = fma(df, df, r2[a][b]);
              }
            }
          }
        }
        double cv[2][4], mb[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) mb[b] = sm[cb + 16 * b];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double kv = MAT ? gpp_kernel_value(kind, r2[a][b], r2m[MAT ? a : 0][MAT ? b : 0], ec) : gpp_exp_nonpos(-r2[a][b], ec);
            const double c = sf2 * kv - slab[((2 * h + a) * 4 + b) * 256 + tid];
            cv[a][b] = (cb + 16 * b < clim) ? c : 0.0;  // (a select: whatever a column beyond M_r holds never reaches a minimum)
          }
        const double sc[2] = {ss[ra], ss[ra + 4]};
        double keep[2] = {0.0, 0.0};
#pragma unroll 1
        for (int k = 0; k < Q; ++k) {
          const double z = sz[k];
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            const double t = z * sc[a];
            double s = fma(cv[a][0], t, mb[0]);
#pragma unroll
            for (int b = 1; b < 4; ++b) s = fmin(s, fma(cv[a][b], t, mb[b]));
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) s = fmin(s, __shfl_xor(s, o));  // the 16 lanes (li) that share this row
            keep[a] = (li == (k & 15)) ? s : keep[a];
          }
          if ((k & 15) == 15 || k + 1 == Q) {  // (uniform) nodes (k & ~15) .. k leave, one per lane
            const int kn = (k & ~15) + li;
            if (kn <= k) {
              rec[(int64_t)ra * Q + kn] = keep[0];
              rec[(int64_t)(ra + 4) * Q + kn] = keep[1];
            }
          }
        }
      }
    }
    __syncthreads();  // (the caller may stage another tile at once)
  }
};

template <int VAR, bool MAT>
__global__ __launch_bounds__(256, VAR == 2 ? 2 : 1) void gpp_post_cross_min_f64(GemmArgs p, PostCrossMinArgs e) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = (int)blockIdx.x;
  const int tm = t / p.tiles_n, tn = t - tm * p.tiles_n;
  gemm_tile<VAR, 64, 64, 2, 16, 2, 2>(p, tm, tn, p.A, p.B, nullptr, nullptr, smem, GemmNoHook(), PostCrossMinEpilogue<MAT>{e, t, p.N});
}

// LDS bytes of an instantiation (dynamic: the wide-chunk variants exceed the 64 KiB static limit)
constexpr size_t gemm_lds_bytes(int var, int tm, int tn, int bk, int nbuf) {
  const int tx = tm > tn ? tm : tn;
  const int mc = bk * ldt_mc(tx, bk), kc = tx * LDK;
  return (size_t)nbuf * 2 * ((var != 2 && kc > mc) ? kc : mc) * sizeof(double);
}
template <int VAR, int WTM, int WTN, int TAG, int BK, int NBUF>
hipError_t launch_inst(hipStream_t s, dim3 grid, const GemmArgs& a) {
  constexpr size_t bytes = gemm_lds_bytes(VAR, 2 * WTM, 2 * WTN, BK, NBUF);
  auto* fn = gpp_gemm_f64<VAR, WTM, WTN, TAG, BK, NBUF>;
  if (bytes > 48 * 1024) {
    static std::atomic<bool> attr_set[64];  // per instantiation and device (function attributes are per device)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
  }
  hipLaunchKernelGGL(fn, grid, dim3(256), bytes, s, a);
  return hipGetLastError();
}
// small tiles: wide K chunks for the row-contiguous variant, the classic staging otherwise
#ifndef GPP_SMALL_BK
#define GPP_SMALL_BK 64
#endif
template <int VAR>
hipError_t launch_var(hipStream_t s, int tm, int tn, dim3 grid, const GemmArgs& a) {
  constexpr int SBK = (VAR == 2) ? GPP_SMALL_BK : 16;
  constexpr int SNB = (VAR == 2 && GPP_SMALL_BK > 16) ? 1 : 2;
  if (tm == 128 && tn == 128 && a.tag == 1 && VAR == 2) return launch_inst<2, 64, 64, 1, 16, 2>(s, grid, a);
  if (tm == 128 && tn == 128) return launch_inst<VAR, 64, 64, 0, 16, 2>(s, grid, a);
  if (tm == 64 && tn == 64) return launch_inst<VAR, 32, 32, 0, SBK, SNB>(s, grid, a);
  if (tm == 32 && tn == 32) return launch_inst<VAR, 16, 16, 0, SBK, SNB>(s, grid, a);
  if (tm == 128 && tn == 32) return launch_inst<VAR, 64, 16, 0, SBK, SNB>(s, grid, a);
  return hipErrorInvalidValue;
}


// ---- DAG executor: device side ----------------------------------------------------------------------------------------------
// (see gpp_internal.h.)  The task list and the product descriptors are read through the CONSTANT address space: scalar loads the
// compiler may repeat at will, exactly like kernel arguments — the tile body compiles to the code of the launch-per-product kernel.
#define GPP_AS4 __attribute__((address_space(4)))
typedef const GemmArgs GPP_AS4 CGemmArgs;

__device__ __forceinline__ int exec_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// thread 0 polls until both counters have reached their values; false: the launch is being abandoned (time-out or abort word)
__device__ __forceinline__ bool exec_poll(int* counters, int w0, int v0, int w1, int v1, long long budget, int32_t* info,
                                          int status = GPP_INFO_EXEC_TIMEOUT) {
  long long t0 = 0;
  bool timed = false;
  for (;;) {
    const bool r0 = w0 < 0 || exec_load(counters + w0) >= v0;
    const bool r1 = w1 < 0 || exec_load(counters + w1) >= v1;
    if (r0 & r1) return true;
    if (!timed) {
      t0 = (long long)wall_clock64();
      timed = true;
    }
    const long long waited = (long long)wall_clock64() - t0;
    if (exec_load(counters) != 0) return false;
    if (waited > budget) {
      const long long ms = waited / 100000;
      __hip_atomic_store(counters, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicCAS(info, 0, status | (int)(ms > 0xFFFFF ? 0xFFFFF : ms));
      return false;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

typedef const DagTask GPP_AS4 CDagTask;
// Plans are independent of the operands' addresses (GemmArgs::buf + byte offsets); this one-wave-per-64-groups kernel writes the
// absolute copy the executor reads, stream-ordered in front of it (the tile body then finds its operands as re-loadable scalars of a
// constant-address-space struct, as kernel arguments would be — computing them per task cost spilled VGPRs).
__global__ __launch_bounds__(64) void gpp_dag_bind(const GemmArgs* rel, GemmArgs* abs, int n, DagBases bases) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= n) return;
  GemmArgs a = rel[g];
  auto base = [&](int b) {
    return b == 0 ? bases.p[0] : b == 1 ? bases.p[1] : b == 2 ? bases.p[2] : b == 3 ? bases.p[3] : b == 4 ? bases.p[4] : b == 5 ? bases.p[5]
                                                                                                     : b == 6 ? bases.p[6] : bases.p[7];
  };
  a.A = reinterpret_cast<const double*>(base(a.buf[0]) + reinterpret_cast<uintptr_t>(a.A));
  a.B = reinterpret_cast<const double*>(base(a.buf[1]) + reinterpret_cast<uintptr_t>(a.B));
  a.C = reinterpret_cast<double*>(base(a.buf[2]) + reinterpret_cast<uintptr_t>(a.C));
  a.C2 = a.buf[3] >= 0 ? reinterpret_cast<double*>(base(a.buf[3]) + reinterpret_cast<uintptr_t>(a.C2)) : nullptr;
  abs[g] = a;
}
// The executor's tile hooks.  per_task: the tile is one of many bodies inside the task loop, so gemm_tile derives its per-thread
// positions afresh per tile (else hipcc hoists the positions of EVERY body to kernel entry and carries them through every K loop).
struct DagPlainTile {
  static constexpr bool per_task = true;
  __device__ __forceinline__ void operator()() const {}
};
template <class T>
struct DagAhead {  // thread 0 takes the next ticket after the last MFMA and parks it in LDS
  static constexpr bool per_task = true;
  const T& take;
  int* s_pre;
  int done_after;
  __device__ __forceinline__ void operator()() const {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));  // (see tid_now in gpp_dag_f64)
    if (t == 0) *s_pre = take(done_after);
  }
};
__global__ __launch_bounds__(256, 2) void gpp_dag_f64(DagLaunch e) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int s_idx, s_ok, s_pre;
  const int tid = threadIdx.x;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
  CDagTask* tasks = (CDagTask*)e.tasks;
  CGemmArgs* groups = (CGemmArgs*)e.groups;
#pragma clang diagnostic pop
  // The ticket of the NEXT task is taken just before the current tile's epilogue (thread 0; the value is consumed after the task's
  // increments), so the atomic's round trip runs under the epilogue's own memory traffic.  A work-group then holds two tickets for
  // those few microseconds, its current one always the smaller: the earliest unfinished task is still some work-group's CURRENT
  // task, so progress is as before.  (Earlier than the epilogue the next task — possibly a chain task — would sit behind a whole tile.)
  // s_pre (thread 0 only, in LDS so that it costs no VGPR across the tile): -2 nothing taken ahead, -1 stop, >= 0 ticket
  auto take = [&](int done_after) -> int {  // thread 0 only
    // (main workers: no budget, no quit flag, no limit — nothing but the atomic; the abort word is seen by the waits)
    // (the launch's switches pass through an asm: compared afresh per call, not as flags and addresses held from kernel entry on — six
    //  SGPRs that were spilled around every tile)
    int max_tasks = e.max_tasks, quit_id = e.quit_id, ticket_limit = e.ticket_limit;
    asm volatile("" : "+s"(max_tasks), "+s"(quit_id), "+s"(ticket_limit));
    if (max_tasks > 0 && done_after >= max_tasks) return -1;
    if (quit_id >= 0 && (exec_load(e.counters) != 0 || exec_load(e.counters + quit_id) >= e.quit_val)) return -1;
    if (ticket_limit <= 0) return __hip_atomic_fetch_add(e.counters + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // a filler launch in front of a panel never takes a task that needs that panel: the launch could not end (gpp_dag.hip)
    int old = exec_load(e.counters + 1);
    while (old < ticket_limit &&
           !__hip_atomic_compare_exchange_strong(e.counters + 1, &old, old + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
    }
    return old < ticket_limit ? old : -1;
  };
  // The thread index is read afresh at every use inside the task loop (an asm the compiler cannot merge or hoist): derived once,
  // "thread 0" masks and per-thread positions are loop invariants, which hipcc computes at kernel entry and then holds in registers
  // (or spill slots) through every tile's K loop.
  auto tid_now = []() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
  };
  auto first = [&]() { return tid_now() == 0; };
  if (tid == 0) s_pre = -2;
  for (int done = 0;; ++done) {
    if (first()) {
      const int pre = s_pre;
      s_idx = pre != -2 ? pre : take(done);
      s_pre = -2;
    }
    __syncthreads();
    const int idx = __builtin_amdgcn_readfirstlane(s_idx);
    __syncthreads();  // (thread 0 rewrites s_idx at the top of the next iteration; the copy tasks have no barrier of their own)
    if (idx < 0 || idx >= e.ntasks) break;
    if (e.trace && first()) {
      e.trace[4 * (size_t)idx] = wall_clock64();
      e.trace[4 * (size_t)idx + 3] = (unsigned long long)blockIdx.x | ((unsigned long long)(unsigned)e.tag << 32);
    }
    const int w0 = tasks[idx].wait_id[0], w1 = tasks[idx].wait_id[1], w2 = tasks[idx].wait_id[2];
    if (w0 >= 0 || w1 >= 0 || w2 >= 0) {
      if (first()) {
        // (fast path: all three counters' loads in flight together; the polling loop only when one of them is not there yet)
        const int v0 = tasks[idx].wait_val[0], v1 = tasks[idx].wait_val[1], v2 = tasks[idx].wait_val[2];
        const int c0 = w0 >= 0 ? exec_load(e.counters + w0) : v0, c1 = w1 >= 0 ? exec_load(e.counters + w1) : v1,
                  c2 = w2 >= 0 ? exec_load(e.counters + w2) : v2;
        bool ok = (c0 >= v0) & (c1 >= v1) & (c2 >= v2);
        if (!ok) {
          ok = exec_poll(e.counters, w0, v0, w1, v1, e.budget, e.info, GPP_INFO_EXEC_TIMEOUT);
          if (ok && w2 >= 0) ok = exec_poll(e.counters, w2, v2, -1, 0, e.budget, e.info, GPP_INFO_EXEC_TIMEOUT);
        }
        s_ok = ok ? 1 : 0;
      }
      __syncthreads();
      const int ok = s_ok;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // what the publishers wrote before their increments is visible from here
      __syncthreads();
      if (!ok) break;
    }
    if (e.trace && first()) e.trace[4 * (size_t)idx + 1] = wall_clock64();
    const CGemmArgs& p = groups[tasks[idx].group];
    const int tm = tasks[idx].tm, tn = tasks[idx].tn;
    if (p.op == 0) {
      if (p.etile == 64) {
        // The 64-tile tasks are the chain between two panels: few, short, latency-bound and on the list's critical path, and they
        // share their SIMDs with another work-group's big tile, whose pipelined loop leaves hardly an issue slot free (beside it they
        // ran 20 % longer and the panels started later: profiles/r19_dag_traces.txt).  They run at raised wave priority.
        if constexpr (GPP_DAG_CHAIN_PRIO != 0) __builtin_amdgcn_s_setprio(GPP_DAG_CHAIN_PRIO);
        gemm_tile<2, 32, 32, 0, 64, 1, 2>(p, tm, tn, p.A, p.B, p.C, p.C2, smem, DagPlainTile());
        if constexpr (GPP_DAG_CHAIN_PRIO != 0) __builtin_amdgcn_s_setprio(0);
      } else gemm_tile<2, 64, 64, 0, 16, 2, 2>(p, tm, tn, p.A, p.B, p.C, p.C2, smem, DagAhead<decltype(take)>{take, &s_pre, done + 1});
    } else {
      // copy the M x 128 strip tn of B into C: 64 16-byte vectors per row, 4 rows per pass, 8 passes in flight
      const int t = tid_now() & 255;
      const int c = tn * 128 + ((t & 63) << 1), r4 = t >> 6;
      if (c < p.N) {
        const bool pair = c + 1 < p.N;
        for (int r0 = 0; r0 < p.M; r0 += 32) {
          v2d v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int r = r0 + 4 * q + r4;
            const double* src = p.B + (int64_t)(r < p.M ? r : 0) * p.ldb + c;
            if (pair) v[q] = *reinterpret_cast<const v2d*>(src);
            else v[q] = (v2d){*src, 0.0};
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int r = r0 + 4 * q + r4;
            if (r < p.M) {
              double* dst = p.C + (int64_t)r * p.ldc + c;
              if (pair) *reinterpret_cast<v2d*>(dst) = v[q];
              else *dst = v[q].x;
            }
          }
        }
      }
    }
    const int i0 = tasks[idx].inc_id[0], i1 = tasks[idx].inc_id[1];
    if (i0 >= 0 || i1 >= 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have left the CU
      __syncthreads();
      if (first()) {
        // (the explicit wait between the write-back and the increments is REQUIRED: see panel_publish in gpp_leaf.hip)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (i0 >= 0) __hip_atomic_fetch_add(e.counters + i0, (int)tasks[idx].inc_val[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (i1 >= 0) __hip_atomic_fetch_add(e.counters + i1, (int)tasks[idx].inc_val[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (e.trace) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (first()) e.trace[4 * (size_t)idx + 2] = wall_clock64();
    }
  }
}

__global__ __launch_bounds__(64) void gpp_exec_gate(int* counters, int id, int target, int32_t* info, long long budget) {
  if (threadIdx.x == 0) (void)exec_poll(counters, id, target, -1, 0, budget, info);
}
__global__ __launch_bounds__(64) void gpp_exec_signal(int* counters, int id) {
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(counters + id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

// tile_m/tile_n: 0 = pick a square tile by grid size; else the work-group tile (128x128, 64x64, 32x32 or 128x32).
hipError_t gpp_launch_gemm(hipStream_t s, int variant, const GemmArgs& a_in, int batch, int tile_m, int tile_n) {
  GemmArgs a = a_in;
  if (a.M <= 0 || a.N <= 0 || batch <= 0) return hipSuccess;
  auto ntiles = [&](int T) -> int64_t {
    const int64_t tm = (a.M + T - 1) / T, tn = (a.N + T - 1) / T;
    return (a.c_lower ? tm * (tm + 1) / 2 : tm * tn) * batch * (a.batch2 > 1 ? a.batch2 : 1);  // triangular: M == N
  };
  if (tile_m == 0) {
    // enough 128^2 tiles to give every CU a work-group -> big tile; otherwise shrink until the chip is covered
    constexpr int64_t t128 = 256, t64 = 192;
    // (a launch on the panel stream has 32 CUs to fill, not 256: the thresholds scale with the stream's CU count)
    const int64_t cus = a.cu_hint > 0 ? a.cu_hint : 256;
    if (ntiles(128) * 256 >= t128 * cus) tile_m = 128;
    else if (ntiles(64) * 256 >= t64 * cus) tile_m = 64;
    else tile_m = 32;
    tile_n = tile_m;
  }
  if (a.c_lower && tile_m != tile_n) return hipErrorInvalidValue;
  a.tiles_m = (a.M + tile_m - 1) / tile_m;
  a.tiles_n = (a.N + tile_n - 1) / tile_n;
  int64_t nt = a.c_lower ? (int64_t)a.tiles_m * (a.tiles_m + 1) / 2 : (int64_t)a.tiles_m * a.tiles_n;
  a.tile_base = 0;
  if (a.c_lower == 1 && (a.row_mod > 1 || a.row_i1 > 0)) {
    if (a.row_mod < 1) { a.row_mod = 1; a.row_off = 0; }
    if (a.row_off < 0 || a.row_off >= a.row_mod) return hipErrorInvalidValue;
    const int64_t rows = a.tiles_m > a.row_off ? (a.tiles_m - a.row_off + a.row_mod - 1) / a.row_mod : 0;
    // tiles before owned row i: S(i) = i (row_off + 1) + row_mod i (i - 1) / 2
    auto S = [&](int64_t i) { return i * (a.row_off + 1) + (int64_t)a.row_mod * (i * (i - 1) / 2); };
    const int64_t i0 = std::min<int64_t>(std::max(a.row_i0, 0), rows), i1 = a.row_i1 > 0 ? std::min<int64_t>(a.row_i1, rows) : rows;
    if (i1 <= i0) return hipSuccess;
    a.tile_base = S(i0);
    nt = S(i1) - S(i0);
  } else {
    a.row_mod = 0;  // plain enumeration
    if (a.c_lower == 1 && a.row_t1 > 0) {
      // a band of tile rows [row_t0, row_t1): the row-by-row enumeration of the lower triangle makes it a contiguous range
      const int64_t t0 = std::min<int64_t>(std::max(a.row_t0, 0), a.tiles_m), t1 = std::min<int64_t>(a.row_t1, a.tiles_m);
      if (t1 <= t0) return hipSuccess;
      a.tile_base = t0 * (t0 + 1) / 2;
      nt = t1 * (t1 + 1) / 2 - a.tile_base;
    }
  }
  a.swz = 0;
  // Measured on MI355X (N = 20000): the super-tile mapping LOSES 10-20 % against plain row-major order (row-major
  // already shares each A chunk among 16 and each B chunk among 4 work-groups of an XCD, and the triangular launches
  // waste whole super-tiles), so it stays off; kept for experiments with GPP_SWZ-style builds.
  if (false && nt >= 1024) {
    const int64_t n_super = (int64_t)((a.tiles_m + 7) / 8) * ((a.tiles_n + 7) / 8);
    nt = ((n_super + 7) / 8) * 8 * 64;
    a.swz = 1;
  }
  const int batch2 = a.batch2 > 1 ? a.batch2 : 1;
  dim3 grid((unsigned)nt, (unsigned)batch, (unsigned)batch2);
  if (a.batch_fast && batch > 1 && !a.swz && nt * batch < (int64_t)1 << 31) {
    a.nbatch = batch;
    grid = dim3((unsigned)(nt * batch), 1u, (unsigned)batch2);
  } else {
    a.batch_fast = 0;
  }
  switch (variant) {
    case 0: return launch_var<0>(s, tile_m, tile_n, grid, a);
    case 1: return launch_var<1>(s, tile_m, tile_n, grid, a);
    case 2: return launch_var<2>(s, tile_m, tile_n, grid, a);
    default: return hipErrorInvalidValue;
  }
}

// a: gpp_lauum's product (TN, both masks 2, klo_mode 3, c_lower 1; C unused).  e.rec holds one record per 128 x 128 tile.
hipError_t gpp_launch_lauum_grad(hipStream_t s, const GemmArgs& a_in, const GradEpiArgs& e) {
  GemmArgs a = a_in;
  if (a.M <= 0) return hipSuccess;
  if (a.M != a.N || a.c_lower != 1 || e.D < 1 || e.D > 16) return hipErrorInvalidValue;
  a.tiles_m = a.tiles_n = (a.M + 127) / 128;
  a.row_mod = 0;
  a.swz = 0;
  a.batch_fast = 0;
  a.tile_base = 0;
  const int64_t nt = (int64_t)a.tiles_m * (a.tiles_m + 1) / 2;
  constexpr size_t bytes = gemm_lds_bytes(2, 128, 128, 16, 2);
  auto* fn = e.D <= 8 ? gpp_lauum_grad_f64<8> : gpp_lauum_grad_f64<16>;
  static std::atomic<bool> attr_set[2][64];  // per instantiation and device
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  const int which = e.D <= 8 ? 0 : 1;
  if (dev < 0 || dev >= 64 || !attr_set[which][dev]) {
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    if (dev >= 0 && dev < 64) attr_set[which][dev] = true;
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)nt), dim3(256), bytes, s, a, e);
  return hipGetLastError();
}

// a: M = M_c, N = M_r, K, the operands' leading dimensions; everything else is set here
hipError_t gpp_launch_post_cross(hipStream_t s, int variant, const GemmArgs& a_in, const PostCrossArgs& e) {
  GemmArgs a = a_in;
  if (a.M <= 0 || a.N <= 0 || a.K <= 0 || (variant != 0 && variant != 2)) return hipErrorInvalidValue;
  a.tiles_m = (a.M + 127) / 128;
  a.tiles_n = (a.N + 127) / 128;
  const int64_t nt = (int64_t)a.tiles_m * a.tiles_n;
  if (nt >= (int64_t)1 << 31) return hipErrorInvalidValue;
  const bool mat = ((e.dk >> 8) & 255) != 0;
  const size_t bytes = gemm_lds_bytes(variant, 128, 128, 16, 2);
  auto* fn = variant == 2 ? (mat ? gpp_post_cross_f64<2, true> : gpp_post_cross_f64<2, false>)
                          : (mat ? gpp_post_cross_f64<0, true> : gpp_post_cross_f64<0, false>);
  static std::atomic<bool> attr_set[4][64];  // per instantiation and device
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  const int which = (variant == 2 ? 2 : 0) + (mat ? 1 : 0);
  if (dev < 0 || dev >= 64 || !attr_set[which][dev]) {
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    if (dev >= 0 && dev < 64) attr_set[which][dev] = true;
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)nt), dim3(256), bytes, s, a, e);
  return hipGetLastError();
}

// as gpp_launch_post_cross; e.dn carries the observed directions
hipError_t gpp_launch_post_cross_lin(hipStream_t s, int variant, const GemmArgs& a_in, const PostCrossLinArgs& e) {
  GemmArgs a = a_in;
  const int D = e.dk & 255, dlo = e.dn & 255, dnum = e.dn >> 8;
  if (a.M <= 0 || a.N <= 0 || a.K <= 0 || (variant != 0 && variant != 2) || dnum < 1 || dlo + dnum > D || e.lda < 1 + dnum)
    return hipErrorInvalidValue;
  a.tiles_m = (a.M + 127) / 128;
  a.tiles_n = (a.N + 127) / 128;
  const int64_t nt = (int64_t)a.tiles_m * a.tiles_n;
  if (nt >= (int64_t)1 << 31) return hipErrorInvalidValue;
  const bool mat = ((e.dk >> 8) & 255) != 0;
  const size_t bytes = gemm_lds_bytes(variant, 128, 128, 16, 2);
  auto* fn = variant == 2 ? (mat ? gpp_post_cross_lin_f64<2, true> : gpp_post_cross_lin_f64<2, false>)
                          : (mat ? gpp_post_cross_lin_f64<0, true> : gpp_post_cross_lin_f64<0, false>);
  static std::atomic<bool> attr_set[4][64];  // per instantiation and device
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  const int which = (variant == 2 ? 2 : 0) + (mat ? 1 : 0);
  if (dev < 0 || dev >= 64 || !attr_set[which][dev]) {
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    if (dev >= 0 && dev < 64) attr_set[which][dev] = true;
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)nt), dim3(256), bytes, s, a, e);
  return hipGetLastError();
}

// as gpp_launch_post_cross; e.dk carries Q
hipError_t gpp_launch_post_cross_min(hipStream_t s, int variant, const GemmArgs& a_in, const PostCrossMinArgs& e) {
  GemmArgs a = a_in;
  const int Q = e.dk >> 24;
  if (a.M <= 0 || a.N <= 0 || a.K <= 0 || (variant != 0 && variant != 2) || Q < 1 || Q > 64) return hipErrorInvalidValue;
  a.tiles_m = (a.M + 127) / 128;
  a.tiles_n = (a.N + 127) / 128;
  const int64_t nt = (int64_t)a.tiles_m * a.tiles_n;
  if (nt >= (int64_t)1 << 31) return hipErrorInvalidValue;
  const bool mat = ((e.dk >> 8) & 255) != 0;
  const size_t bytes = gemm_lds_bytes(variant, 128, 128, 16, 2);
  auto* fn = variant == 2 ? (mat ? gpp_post_cross_min_f64<2, true> : gpp_post_cross_min_f64<2, false>)
                          : (mat ? gpp_post_cross_min_f64<0, true> : gpp_post_cross_min_f64<0, false>);
  static std::atomic<bool> attr_set[4][64];  // per instantiation and device
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  const int which = (variant == 2 ? 2 : 0) + (mat ? 1 : 0);
  if (dev < 0 || dev >= 64 || !attr_set[which][dev]) {
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    if (dev >= 0 && dev < 64) attr_set[which][dev] = true;
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)nt), dim3(256), bytes, s, a, e);
  return hipGetLastError();
}

hipError_t gpp_launch_dag_bind(hipStream_t s, const GemmArgs* rel, GemmArgs* abs, int n, const DagBases& bases) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(gpp_dag_bind, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, rel, abs, n, bases);
  return hipGetLastError();
}
hipError_t gpp_launch_dag(hipStream_t s, int nworkers, const DagLaunch& e) {
  if (nworkers <= 0) return hipSuccess;
  constexpr size_t b128 = gemm_lds_bytes(2, 128, 128, 16, 2), b64 = gemm_lds_bytes(2, 64, 64, 64, 1);
  constexpr size_t bytes = b128 > b64 ? b128 : b64;
  static std::atomic<bool> attr_set[64];
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(gpp_dag_f64), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (err != hipSuccess) return err;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  hipLaunchKernelGGL(gpp_dag_f64, dim3((unsigned)nworkers), dim3(256), bytes, s, e);
  return hipGetLastError();
}
hipError_t gpp_launch_exec_gate(hipStream_t s, int* counters, int id, int target, int32_t* info, long long budget) {
  hipLaunchKernelGGL(gpp_exec_gate, dim3(1), dim3(64), 0, s, counters, id, target, info, budget);
  return hipGetLastError();
}
hipError_t gpp_launch_exec_signal(hipStream_t s, int* counters, int id) {
  hipLaunchKernelGGL(gpp_exec_signal, dim3(1), dim3(64), 0, s, counters, id);
  return hipGetLastError();
}

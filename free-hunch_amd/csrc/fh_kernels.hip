// Free Hunch covariance / DCT / operator / CG kernels for gfx950 (CDNA4, wave64), float64.
//
// Everything on this side of the path is HBM- or latency-bound vector work on d = 3*S*S elements
// plus the d x m factor base; the kernels are organised around coalesced 16-byte row-pair accesses,
// wave shuffles + LDS for reductions, and deterministic two-stage sums (no float atomics on this side, so a
// solve is bitwise reproducible).  Every kernel that runs inside the CG loop takes a device `done` flag and
// returns at once when it is set, which lets the host enqueue iterations in chunks without changing
// the reference's stopping rule.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "fh_common.h"

using namespace fh;

// Kernels inside the CG loop are gated per image: `states` is the array of device-resident CG control blocks (null
// outside the loop) and a workgroup returns at once when its image has met its stopping rule.
#define IMG_GUARD(states, img) \
  if ((states) != nullptr && (states)[(img)].done != 0) return

struct RtolArr {
  double v[FH_MAX_BATCH];
};

// Per-image pointer table of a lock-step batch (passed by value in the kernel arguments; the image is a grid dimension).
// The covariance-update kernels below take their per-image operands this way, so that ONE launch sequence updates all
// images of a batch; the single-image entry points pass a table with one entry (same kernels, same arithmetic).
struct PtrTab {
  double* p[FH_MAX_BATCH];
};
static inline PtrTab tab1(const double* q) {
  PtrTab t;
  memset(&t, 0, sizeof(t));
  t.p[0] = const_cast<double*>(q);
  return t;
}

// ------------------------------------------------------------------------------------------------
// float64 GEMM for the two DCT passes on the matrix cores (v_mfma_f64_16x16x4_f64):
//   C = A * op(B),  A [M][K] (lda), C [M][N] (ldc),  BT ? B [N][K] : B [K][N]  (ldb).
// 32x32 output tile per workgroup, one 16x16 MFMA tile per wave, K staged through LDS in chunks of
// 32 with both operands k-contiguous (row stride 34 doubles: conflict-free ds_read_b64 for the
// A[i=l&15][k=l>>4] / B[k=l>>4][j=l&15] operand maps).  f64 C/D map: col = l&15, row = (l>>4) + 4*reg.
// ------------------------------------------------------------------------------------------------
typedef double double4_t __attribute__((ext_vector_type(4)));

// PPI: planes per image (3 colour planes; 1 for the one-plane measurement of the colorization operator) - only the
// image a workgroup asks the `done` flag of depends on it
template <bool BT, int TM, int TN = TM, int PPI = 3>  // TM x TN MFMA tiles (16x16) per wave: workgroup tile 32 TM x 32 TN
__global__ __launch_bounds__(256) void k_gemm_f64(const double* __restrict__ A, const double* __restrict__ B,
                                                  double* __restrict__ C, int M, int N, int K, int lda, int ldb,
                                                  int ldc, int64_t sA, int64_t sB, int64_t sC,
                                                  const fh_cg_state* __restrict__ states, int rows_per_plane,
                                                  const double* __restrict__ add, double add_scale) {
  constexpr int BM = 32 * TM, BN = 32 * TN, BK = 32, LD = BK + 2;
  if (states != nullptr) {
    // Pass 1 runs over the rows of all planes at once, so where the rows of an image (PPI * S) are no multiple of BM a tile
    // holds rows of several images: it is skipped only when every one of them has met its stopping rule (uniform).
    const int row_hi = (int)(blockIdx.y * BM) + BM - 1 < M ? (int)(blockIdx.y * BM) + BM - 1 : M - 1;
    int img = ((int)blockIdx.z + (int)(blockIdx.y * BM) / rows_per_plane) / PPI;
    const int img_hi = ((int)blockIdx.z + row_hi / rows_per_plane) / PPI;
    bool live = false;
    for (; img <= img_hi; ++img) live = live || states[img].done == 0;
    if (!live) return;
  }
  __shared__ __align__(16) double As[2][BM][LD];
  __shared__ __align__(16) double Bs[2][BN][LD];
  A += sA * blockIdx.z;
  B += sB * blockIdx.z;
  C += sC * blockIdx.z;
  if (add != nullptr) add += sC * blockIdx.z;  // epilogue C = acc + add_scale * add, same layout as C
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 16 * TM, wn = (wave & 1) * 16 * TN;
  const int li = lane & 15, lk = lane >> 4;
  double4_t acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = double4_t{0.0, 0.0, 0.0, 0.0};
  // staging: BM rows x 32 k per operand = 4*T doubles per thread: row = (tid >> 3) + 32 * q, k segment (tid & 7) * 4
  const int srow = tid >> 3, sseg = (tid & 7) * 4;
  double ra[TM][4], rb[TN][4];
  // full tiles (every DCT size that is a multiple of 64/32) take 16-byte loads; ragged edges fall back to guarded scalars
  const bool full = (m0 + BM <= M) && (n0 + BN <= N) && (K % BK == 0) && ((lda | ldb) % 2 == 0);
  auto load_chunk = [&](int k0) {  // global -> registers (issued one chunk ahead of its use)
#pragma unroll
    for (int q = 0; q < TM; ++q) {
      const int gm = m0 + srow + 32 * q;
      if (full) {
        const double2* pa = reinterpret_cast<const double2*>(A + (int64_t)gm * lda + k0 + sseg);
        const double2 a0 = pa[0], a1 = pa[1];
        ra[q][0] = a0.x, ra[q][1] = a0.y, ra[q][2] = a1.x, ra[q][3] = a1.y;
        continue;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int gk = k0 + sseg + e;
        ra[q][e] = (gm < M && gk < K) ? A[(int64_t)gm * lda + gk] : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < TN; ++q) {
      if (full) {
        const double2* pb = BT ? reinterpret_cast<const double2*>(B + (int64_t)(n0 + srow + 32 * q) * ldb + k0 + sseg)
                               : reinterpret_cast<const double2*>(B + (int64_t)(k0 + srow) * ldb + n0 + sseg + 32 * q);
        const double2 b0 = pb[0], b1 = pb[1];
        rb[q][0] = b0.x, rb[q][1] = b0.y, rb[q][2] = b1.x, rb[q][3] = b1.y;
        continue;
      }
      if (BT) {
        const int gn = n0 + srow + 32 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int gk = k0 + sseg + e;
          rb[q][e] = (gn < N && gk < K) ? B[(int64_t)gn * ldb + gk] : 0.0;
        }
      } else {
        const int gk = k0 + srow;  // srow indexes k here, (sseg + 32 q) the n segment
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int gn = n0 + sseg + 32 * q + e;
          rb[q][e] = (gn < N && gk < K) ? B[(int64_t)gk * ldb + gn] : 0.0;
        }
      }
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int q = 0; q < TM; ++q) {
      *reinterpret_cast<double2*>(&As[buf][srow + 32 * q][sseg]) = make_double2(ra[q][0], ra[q][1]);
      *reinterpret_cast<double2*>(&As[buf][srow + 32 * q][sseg + 2]) = make_double2(ra[q][2], ra[q][3]);
    }
#pragma unroll
    for (int q = 0; q < TN; ++q) {
      if (BT) {
        *reinterpret_cast<double2*>(&Bs[buf][srow + 32 * q][sseg]) = make_double2(rb[q][0], rb[q][1]);
        *reinterpret_cast<double2*>(&Bs[buf][srow + 32 * q][sseg + 2]) = make_double2(rb[q][2], rb[q][3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[buf][sseg + 32 * q + e][srow] = rb[q][e];
      }
    }
  };
  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += BK, buf ^= 1) {
    const bool more = k0 + BK < K;
    if (more) load_chunk(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      double a[TM], b[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = As[buf][wm + 16 * i + li][kk + lk];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = Bs[buf][wn + 16 * j + li][kk + lk];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) store_chunk(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int gn = n0 + wn + 16 * j + li;
    if (gn >= N) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gm = m0 + wm + 16 * i + lk + 4 * r;
        if (gm < M) {
          const int64_t o = (int64_t)gm * ldc + gn;
          C[o] = add != nullptr ? fma(add_scale, add[o], acc[i][j][r]) : acc[i][j][r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Symmetric-basis form of the DCT passes (k_dct_sym).  Both dense passes are written as the SAME per-plane product with a
// transposed result,  out[k][r] = sum_n P[k][n] in[r][n]:  pass A gives (X P_w^T)^T, pass B applied to that gives
// P_h X P_w^T in the natural orientation.  The DCT basis - and a symmetric blur folded into it - satisfies
// P[k][S-1-n] = (-1)^k P[k][n], so with the butterflies s = x_n + x_{S-1-n}, d = x_n - x_{S-1-n}
//     forward  (INV = 0):  out[2j][r] = sum_{n<S/2} Pe[j][n] s[r][n],   out[2j+1][r] = sum_{n<S/2} Po[j][n] d[r][n]
//     inverse  (INV = 1, basis Q = P^T, mirror symmetry in k):  E = sum_j Qe[k][j] x[r][2j],  O = sum_j Qo[k][j] x[r][2j+1],
//                          out[k][r] = E + O,  out[S-1-k][r] = E - O          (k < S/2)
// half the multiply-adds of the dense pass.  A workgroup owns 32 (j or k) x 32 (r) outputs of each parity, keeps its two
// half-basis slices (2 x 32 x S/2 doubles, 66 KB at S = 256) RESIDENT in LDS and walks over its share of the planes, so per
// output tile it pulls 85 KB from L2 instead of the 192 KB of the 64 x 32 dense tile (the dense kernel is bound by the
// ~12 B/clk a CU pulls from L2, not by the f64 matrix cores).  Same MFMA (v_mfma_f64_16x16x4_f64), same LDS row pitch rule.
// ------------------------------------------------------------------------------------------------
// per-image diagonal applied to the result of a pass (the m = 0 covariance apply C z = D .* z folded into the forward DCT)
struct fh_diag_tab {
  const double* D[FH_MAX_BATCH];  // null table (D[0] == nullptr): no scaling
};

// NS: plane streams per workgroup.  NS = 2 is a 512-thread workgroup whose two 4-wave halves share the resident half-basis
// slices and each walk a plane list of their own with their own staging buffers and accumulators: two waves per SIMD, so
// one half's MFMAs run under the other half's load waits, and 12 planes at S = 256 are one task per half on 192 workgroups
// instead of two tasks back to back on half of 256 (profiles/dct_streams.md).  tid = threadIdx.x & 255 drives the same
// staging map, wave tile and epilogue in either half; every output keeps its chain of MFMA accumulations (k ascending in
// steps of 4, parities apart), so the result does not depend on NS.
template <bool INV, int PPI = 3, int NS = 1>  // PPI: planes per image (3, or 1 for the colorization operator's measurement plane)
__global__ __launch_bounds__(256 * NS) void k_dct_sym(const double* __restrict__ Ah, const double* __restrict__ X,
                                                      double* __restrict__ C, int S, int planes,
                                                      const fh_cg_state* __restrict__ states, const double* __restrict__ add,
                                                      double add_scale, fh_diag_tab dg, double* __restrict__ dot_part,
                                                      int dot_stride) {
  // dot_part != null (with add): the workgroup also leaves sum(add .* out) of every (plane, tile) it completes in
  // dot_part[image * dot_stride + (plane % PPI) * tiles + tile] - the p.Ap reduction of the CG iteration rides in the pass
  // that produces Ap (A p = sigma_y^2 p + ..., add = p), summed later in a fixed order
  // NS = 1: K chunks of 64 (two per plane at S = 256): the per-chunk cost besides the 16 MFMA pairs - LDS stores, the
  // barrier, the wait for the prefetched rows - was ~65 % of a 32-wide chunk's time (measured 14.4 us per pass at BK = 32,
  // 36 % of the f64 MFMA rate); halving the chunk count halves it.  Two LDS buffers, the next chunk prefetched into registers.
  // NS = 2: two streams of double buffers do not fit beside the basis (201 728 B).  One 64-wide buffer per stream does
  // (134 144 B) at the price of a second barrier per chunk, and measured faster than double-buffered chunks of 32
  // (136 192 B): 22.0 against 23.1 us for the two passes over 12 planes (profiles/dct_streams.md).
  constexpr int TJ = 32, TR = 32, BK = 64, LDB = BK + 2, NBUF = NS == 2 ? 1 : 2, NP8 = BK / 32;  // NP8 pieces of 8 doubles per thread
  extern __shared__ __align__(16) double smem[];
  const int H = S >> 1, LDA = H + 2;
  const int half = NS == 2 ? (int)(threadIdx.x >> 8) : 0;
  double* As_e = smem;                      // [TJ][LDA] resident half-basis slices (shared by the halves)
  double* As_o = As_e + TJ * LDA;           // [TJ][LDA]
  double* Bs = As_o + TJ * LDA + half * (NBUF * 2 * TR * LDB);  // per half: [NBUF buffers][2 parities][TR][LDB]
  const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;  // wave: within the half
  const int li = lane & 15, lk = lane >> 4;
  const int jw = (wave >> 1) * 16, rw = (wave & 1) * 16;
  const int j0 = blockIdx.y * TJ, r0 = blockIdx.x * TR;
  for (int i = threadIdx.x; i < TJ * (H / 2); i += 256 * NS) {
    const int row = i / (H / 2), c2 = (i % (H / 2)) * 2;
    const double2 ve = *reinterpret_cast<const double2*>(Ah + (int64_t)(j0 + row) * H + c2);
    const double2 vo = *reinterpret_cast<const double2*>(Ah + (int64_t)H * H + (int64_t)(j0 + row) * H + c2);
    *reinterpret_cast<double2*>(&As_e[row * LDA + c2]) = ve;
    *reinterpret_cast<double2*>(&As_o[row * LDA + c2]) = vo;
  }
  const int srow = tid >> 3, sq = tid & 7;  // staging: row of the r tile, lane within the row's 8-thread group
  const int nkc = H / BK;
  // planes of this half's stream s: p = s, s + streams, ...  (finished images of a CG batch are skipped).  Both halves
  // take every barrier, so the loop runs the longer half's trip count: each thread counts the other half's planes too.
  const int nstreams = (int)gridDim.z * NS;
  int pl[8], npl = 0, npl_other = 0;
  // Half h of workgroup z is stream h * gridDim.z + z: where the streams are uneven (24 planes on 16 streams) every
  // workgroup pairs a long stream with a short one; pairing neighbours (2 z + h) left half the workgroups with two long
  // streams and measured 37.5 against 34.2 us for the two passes over 24 planes (profiles/dct_streams.md).
  for (int p = half * (int)gridDim.z + (int)blockIdx.z; p < planes && npl < 8; p += nstreams)
    if (states == nullptr || states[p / PPI].done == 0) pl[npl++] = p;
  if (NS == 2)
    for (int p = (1 - half) * (int)gridDim.z + (int)blockIdx.z; p < planes && npl_other < 8; p += nstreams)
      if (states == nullptr || states[p / PPI].done == 0) ++npl_other;
  const int total = npl * nkc, trips = (npl > npl_other ? npl : npl_other) * nkc;
  if (trips == 0) return;  // (uniform over the workgroup)
  double ra[NP8][8];
  auto load_chunk = [&](int t) {
    const double* row = X + (int64_t)pl[t / nkc] * S * S + (int64_t)(r0 + srow) * S;
    const int n0 = (t % nkc) * BK;
#pragma unroll
    for (int h = 0; h < NP8; ++h) {
      if (INV) {  // (even, odd) sample pairs j = n0 + 32 h + 8 e + sq: 8 lanes of a row read 128 contiguous bytes per load
        const double2* p2 = reinterpret_cast<const double2*>(row + 2 * (n0 + 32 * h)) + sq;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double2 v = p2[8 * e];
          ra[h][2 * e] = v.x, ra[h][2 * e + 1] = v.y;
        }
      } else {    // 4 samples at n = n0 + 32 h + 4 sq + i and their mirror images S - 1 - n
        const int nb = n0 + 32 * h + 4 * sq;
        const double2* lo = reinterpret_cast<const double2*>(row + nb);
        const double2* hi = reinterpret_cast<const double2*>(row + S - 4 - nb);
        const double2 l0 = lo[0], l1 = lo[1], h0 = hi[0], h1 = hi[1];
        ra[h][0] = l0.x, ra[h][1] = l0.y, ra[h][2] = l1.x, ra[h][3] = l1.y;
        ra[h][4] = h1.y, ra[h][5] = h1.x, ra[h][6] = h0.y, ra[h][7] = h0.x;  // mirrors of samples 0 .. 3
      }
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int h = 0; h < NP8; ++h) {
      if (INV) {  // pair j = 32 h + 8 e + sq of the chunk: even sample to parity 0, odd sample to parity 1
        double* c0 = Bs + (buf * 2 + 0) * TR * LDB + srow * LDB + 32 * h + sq;
        double* c1 = Bs + (buf * 2 + 1) * TR * LDB + srow * LDB + 32 * h + sq;
#pragma unroll
        for (int e = 0; e < 4; ++e) c0[8 * e] = ra[h][2 * e], c1[8 * e] = ra[h][2 * e + 1];
      } else {
        double* b0 = Bs + (buf * 2 + 0) * TR * LDB + srow * LDB + 32 * h + 4 * sq;
        double* b1 = Bs + (buf * 2 + 1) * TR * LDB + srow * LDB + 32 * h + 4 * sq;
        *reinterpret_cast<double2*>(b0) = make_double2(ra[h][0] + ra[h][4], ra[h][1] + ra[h][5]);
        *reinterpret_cast<double2*>(b0 + 2) = make_double2(ra[h][2] + ra[h][6], ra[h][3] + ra[h][7]);
        *reinterpret_cast<double2*>(b1) = make_double2(ra[h][0] - ra[h][4], ra[h][1] - ra[h][5]);
        *reinterpret_cast<double2*>(b1 + 2) = make_double2(ra[h][2] - ra[h][6], ra[h][3] - ra[h][7]);
      }
    }
  };
  if (NS == 1 || total > 0) {
    load_chunk(0);
    store_chunk(0);
  }
  __syncthreads();
  double4_t acc_e = {0.0, 0.0, 0.0, 0.0}, acc_o = {0.0, 0.0, 0.0, 0.0};
  int buf = 0;
  for (int t = 0; t < trips; ++t, buf ^= NBUF - 1) {
    // a half past its own plane list does no loads, MFMAs or stores and only arrives at the barriers
    const bool active = NS == 1 || t < total, more = t + 1 < total;
    if (more) load_chunk(t + 1);
    const int kc = t % nkc;
    if (active) {
      const double* be = Bs + (buf * 2 + 0) * TR * LDB + (rw + li) * LDB + lk;
      const double* bo = Bs + (buf * 2 + 1) * TR * LDB + (rw + li) * LDB + lk;
      const double* ae = As_e + (jw + li) * LDA + kc * BK + lk;
      const double* ao = As_o + (jw + li) * LDA + kc * BK + lk;
#pragma unroll
      for (int kk = 0; kk < BK; kk += 4) {
        acc_e = __builtin_amdgcn_mfma_f64_16x16x4f64(ae[kk], be[kk], acc_e, 0, 0, 0);
        acc_o = __builtin_amdgcn_mfma_f64_16x16x4f64(ao[kk], bo[kk], acc_o, 0, 0, 0);
      }
    }
    if (kc == nkc - 1) {  // the active halves complete a plane (kc is uniform): write its two output row families
      const int plane = active ? pl[t / nkc] : 0;
      double dsum = 0.0;
      if (active) {
        double* Cp = C + (int64_t)plane * S * S;
        const double* Ap = add != nullptr ? add + (int64_t)plane * S * S : nullptr;
        const double* Dp = dg.D[0] != nullptr ? dg.D[plane / PPI] + (int64_t)(plane % PPI) * S * S : nullptr;
        const int col = r0 + rw + li;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jj = j0 + jw + lk + 4 * q;
          int64_t o0, o1;
          double v0, v1;
          if (INV) {
            o0 = (int64_t)jj * S + col, o1 = (int64_t)(S - 1 - jj) * S + col;
            v0 = acc_e[q] + acc_o[q], v1 = acc_e[q] - acc_o[q];
          } else {
            o0 = (int64_t)(2 * jj) * S + col, o1 = o0 + S;
            v0 = acc_e[q], v1 = acc_o[q];
          }
          if (Dp != nullptr) v0 = Dp[o0] * v0, v1 = Dp[o1] * v1;  // same product as k_rep_apply2 forms for m = 0
          if (Ap != nullptr) {
            const double a0 = Ap[o0], a1 = Ap[o1];
            v0 = fma(add_scale, a0, v0), v1 = fma(add_scale, a1, v1);
            dsum = fma(a0, v0, fma(a1, v1, dsum));
          }
          Cp[o0] = v0;
          Cp[o1] = v1;
        }
        acc_e = double4_t{0.0, 0.0, 0.0, 0.0};
        acc_o = double4_t{0.0, 0.0, 0.0, 0.0};
      }
      if (dot_part != nullptr) {  // (uniform: every thread takes these barriers on every plane-completing trip)
        // block_sum_256 per half: each half sums its own four wave partials, in the same order, from its own four slots
        __shared__ double dred[4 * NS];
        dsum = wave_sum(dsum);
        __syncthreads();
        if (lane == 0) dred[4 * half + wave] = dsum;
        __syncthreads();
        if (active && tid == 0)
          dot_part[(int64_t)(plane / PPI) * dot_stride + (plane % PPI) * (int)(gridDim.x * gridDim.y) + blockIdx.y * gridDim.x +
                   blockIdx.x] = dred[4 * half] + dred[4 * half + 1] + dred[4 * half + 2] + dred[4 * half + 3];
      }
    }
    if (NBUF == 1) __syncthreads();  // every wave is done reading the one buffer
    if (more) store_chunk(buf ^ (NBUF - 1));
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// Rectangular form of the transposed-result pass (k_dct_rect): per plane  out[k][r] = sum_n P[k][n] in[r][n]  with
// P [KO][KI], in [R][KI], out [KO][R].  Blur + decimation by s of a rank-1 PSF fold into the DCT bases as the stride-1 blur
// does (fh_problem.op = 7): G[k][j] = P[k][j s] is [S][So], So = S / s, and
//     dct2(A^T u) = G_col u G_row^T :  pass A  P = G_row,   in u [So][So] -> [S][So];   pass B  P = G_col,   -> [S][S]
//     A(idct2(v)) = G_col^T v G_row :  pass A  P = G_row^T, in v [S][S]   -> [So][S];   pass B  P = G_col^T, -> [So][So]
// The subsampled bases have no mirror symmetry, so these are dense products - but of S S So (S + So) multiply-adds per
// plane pair instead of S^3.  A workgroup owns 32 (k) x 32 (r) outputs, keeps its 32-row slice of P (zero padded to whole
// K chunks of 32, at most 32 x 258 doubles) RESIDENT in LDS and walks over its share of the planes (z, z + gridDim.z, ...),
// the next chunk of `in` prefetched into registers while the current one is multiplied.  Same MFMA
// (v_mfma_f64_16x16x4_f64), operand maps and row pitch rule (pitch = 2 mod 32 doubles) as k_gemm_f64 / k_dct_sym.  Ragged
// KO, KI and R are zero padded under guards; zero terms leave an accumulator as it is, so every output is ONE chain of
// accumulations with k ascending in steps of 4 and does not depend on the planes, the batch or the launch.
// Epilogue operands as in k_dct_sym: the per-image done flag, the per-image table dg (forward pass B: C z = D .* z for
// m = 0), add / add_scale and the p.Ap block partials dot_part (inverse pass B).
// ------------------------------------------------------------------------------------------------
template <int PPI = 3>
__global__ __launch_bounds__(256) void k_dct_rect(const double* __restrict__ P, const double* __restrict__ X,
                                                  double* __restrict__ C, int KO, int KI, int R, int planes,
                                                  const fh_cg_state* __restrict__ states, const double* __restrict__ add,
                                                  double add_scale, fh_diag_tab dg, double* __restrict__ dot_part,
                                                  int dot_stride) {
  constexpr int TJ = 32, TR = 32, BK = 32, LDB = BK + 2;
  extern __shared__ __align__(16) double smem[];
  const int nkc = (KI + BK - 1) / BK, KP = nkc * BK, LDA = KP + 2;
  double* As = smem;             // [TJ][LDA] resident slice of P, zero beyond KO / KI
  double* Bs = As + TJ * LDA;    // [2 buffers][TR][LDB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int jw = (wave >> 1) * 16, rw = (wave & 1) * 16;
  const int j0 = blockIdx.y * TJ, r0 = blockIdx.x * TR;
  const int gz = (int)gridDim.z;
  // the next plane of this workgroup's list at or after p whose image is still running (uniform: scalar loads)
  auto live = [&](int p) {
    while (p < planes && states != nullptr && states[p / PPI].done != 0) p += gz;
    return p;
  };
  int p = live((int)blockIdx.z);
  if (p >= planes) return;  // (uniform over the workgroup)
  const bool pvec = (KI & 1) == 0 && ((uintptr_t)P & 15) == 0, xvec = (KI & 1) == 0 && ((uintptr_t)X & 15) == 0;
  for (int i = tid; i < TJ * (KP / 2); i += 256) {
    const int row = i / (KP / 2), c2 = (i % (KP / 2)) * 2;
    const bool in_row = j0 + row < KO;
    const double* src = P + (int64_t)(j0 + row) * KI + c2;
    double2 v = make_double2(0.0, 0.0);
    if (in_row && pvec && c2 + 2 <= KI) {
      v = *reinterpret_cast<const double2*>(src);
    } else if (in_row) {
      if (c2 < KI) v.x = src[0];
      if (c2 + 1 < KI) v.y = src[1];
    }
    *reinterpret_cast<double2*>(&As[row * LDA + c2]) = v;
  }
  // staging: 32 rows x 32 k per chunk = 4 doubles per thread: row tid >> 3 of the r tile, k segment (tid & 7) * 4
  const int srow = tid >> 3, sseg = (tid & 7) * 4;
  double ra[4];
  auto load_chunk = [&](int pp, int kc) {
    const int gr = r0 + srow, gk = kc * BK + sseg;
    const double* row = X + (int64_t)pp * R * KI + (int64_t)gr * KI + gk;
    if (gr < R && xvec && gk + 4 <= KI) {
      const double2 a0 = reinterpret_cast<const double2*>(row)[0], a1 = reinterpret_cast<const double2*>(row)[1];
      ra[0] = a0.x, ra[1] = a0.y, ra[2] = a1.x, ra[3] = a1.y;
      return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) ra[e] = (gr < R && gk + e < KI) ? row[e] : 0.0;
  };
  auto store_chunk = [&](int buf) {
    double* dst = Bs + (buf * TR + srow) * LDB + sseg;
    *reinterpret_cast<double2*>(dst) = make_double2(ra[0], ra[1]);
    *reinterpret_cast<double2*>(dst + 2) = make_double2(ra[2], ra[3]);
  };
  load_chunk(p, 0);
  store_chunk(0);
  __syncthreads();
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  const int tiles = (int)(gridDim.x * gridDim.y), tile = (int)(blockIdx.y * gridDim.x + blockIdx.x);
  int buf = 0, kc = 0;
  while (true) {
    int np = p, nk = kc + 1;
    if (nk == nkc) nk = 0, np = live(p + gz);
    const bool more = np < planes;
    if (more) load_chunk(np, nk);
    const double* a = As + (jw + li) * LDA + kc * BK + lk;
    const double* b = Bs + (buf * TR + rw + li) * LDB + lk;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc, 0, 0, 0);
    if (kc == nkc - 1) {  // plane p is complete (kc and p are uniform)
      double* Cp = C + (int64_t)p * KO * R;
      const double* Ap = add != nullptr ? add + (int64_t)p * KO * R : nullptr;
      const double* Dp = dg.D[0] != nullptr ? dg.D[p / PPI] + (int64_t)(p % PPI) * KO * R : nullptr;
      const int col = r0 + rw + li;
      double dsum = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int jj = j0 + jw + lk + 4 * q;
        if (jj < KO && col < R) {
          const int64_t o = (int64_t)jj * R + col;
          double v = acc[q];
          if (Dp != nullptr) v = Dp[o] * v;  // same product as k_rep_apply2 forms for m = 0
          if (Ap != nullptr) {
            const double a0 = Ap[o];
            v = fma(add_scale, a0, v);
            dsum = fma(a0, v, dsum);
          }
          Cp[o] = v;
        }
      }
      acc = double4_t{0.0, 0.0, 0.0, 0.0};
      if (dot_part != nullptr) {  // (uniform) sum(add .* out) of this (plane, tile), as k_dct_sym leaves it
        __shared__ double dred[4];
        dsum = wave_sum(dsum);
        __syncthreads();
        if (lane == 0) dred[wave] = dsum;
        __syncthreads();
        if (tid == 0)
          dot_part[(int64_t)(p / PPI) * dot_stride + (p % PPI) * tiles + tile] = dred[0] + dred[1] + dred[2] + dred[3];
      }
    }
    if (more) store_chunk(buf ^ 1);
    __syncthreads();
    if (!more) break;
    p = np, kc = nk, buf ^= 1;
  }
}

// ------------------------------------------------------------------------------------------------
// DCT-variance prior (fh_dct_moments_u8): ingest and moments around the DCT passes.  Both are streaming kernels over a
// few MB; the tool they serve is bound by image decoding, so nothing here goes beyond coalesced 16-byte accesses.
// ------------------------------------------------------------------------------------------------
// x = u8 / 127.5 - 1 over `quads` groups of four pixels: one 4-byte load, two 16-byte stores per thread
__global__ __launch_bounds__(256) void k_u8_to_f64(const uint8_t* __restrict__ in, double* __restrict__ out, int64_t quads) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const uchar4 u = reinterpret_cast<const uchar4*>(in)[q];
  double2* o = reinterpret_cast<double2*>(out + 4 * q);
  o[0] = make_double2((double)u.x / 127.5 - 1.0, (double)u.y / 127.5 - 1.0);
  o[1] = make_double2((double)u.z / 127.5 - 1.0, (double)u.w / 127.5 - 1.0);
}

// sum[k] += z_i[k], sumsq[k] += z_i[k]^2 for i = 0 .. n-1 in index order, z [n][per].  One thread owns two coefficients
// and carries both running sums in registers from the values already in `sum` / `sumsq`: no atomics, no reduction across
// threads, so a coefficient sees the same chain of additions however the images were split into calls.
__global__ __launch_bounds__(256) void k_dct_moments(const double* __restrict__ z, double* __restrict__ sum,
                                                     double* __restrict__ sumsq, int per, int n) {
  const int k = 2 * ((int)blockIdx.x * 256 + (int)threadIdx.x);
  if (k >= per) return;  // per is even: k + 1 < per
  double2 s = *reinterpret_cast<const double2*>(sum + k);
  double2 q = *reinterpret_cast<const double2*>(sumsq + k);
  for (int i = 0; i < n; ++i) {
    const double2 v = *reinterpret_cast<const double2*>(z + (int64_t)i * per + k);
    s.x += v.x, s.y += v.y;
    q.x = fma(v.x, v.x, q.x), q.y = fma(v.y, v.y, q.y);
  }
  *reinterpret_cast<double2*>(sum + k) = s;
  *reinterpret_cast<double2*>(sumsq + k) = q;
}

// the two dense launches at one tile size (32 TM x 32 TN per workgroup): pass 1 along W over all planes at once,
// T[r][k] = sum_n X[r][n] * b1[k][n];  pass 2 along H per plane, Y[k][w] = sum_n b2[k][n] * T[n][w] (+ add_scale * add)
template <int TM, int TN, int PPI>
static void dct_bases_pair(fh_context* ctx, hipStream_t st, const double* b1, const double* b2, const double* in, double* out,
                           int planes, const fh_cg_state* states, const double* add, double add_scale) {
  const int S = ctx->S;
  const unsigned gx = (S + 32 * TN - 1) / (32 * TN);
  hipLaunchKernelGGL((k_gemm_f64<true, TM, TN, PPI>), dim3(gx, (planes * S + 32 * TM - 1) / (32 * TM), 1), dim3(256), 0, st, in, b1,
                     ctx->tmp_img, planes * S, S, S, S, S, S, (int64_t)0, (int64_t)0, (int64_t)0, states, S,
                     (const double*)nullptr, 0.0);
  hipLaunchKernelGGL((k_gemm_f64<false, TM, TN, PPI>), dim3(gx, (S + 32 * TM - 1) / (32 * TM), planes), dim3(256), 0, st, b2,
                     (const double*)ctx->tmp_img, out, S, S, S, S, S, S, (int64_t)0, (int64_t)S * S, (int64_t)S * S, states,
                     1 << 30, add, add_scale);
}

// Two dense S x S passes over `planes` images: T = X b1^T (along W), out = b2 T (along H) [+ add_scale * add].
// b1 = b2 = the DCT basis (or its transpose) gives the 2-D DCT-II / DCT-III; a separable blur folded into the bases
// (fh_problem.fold_*) makes the same two passes compute dct2(A^T x) or A(idct2(x)).
static int dct2d_launch_bases(fh_context* ctx, const double* in, double* out, int planes, const double* b1, const double* b2,
                              const double* add, double add_scale, const fh_cg_state* states, hipStream_t st, int ppi = 3) {
  const int S = ctx->S;
  if (planes > ctx->planes_max) return FH_ESIZE;
  if (ppi != 1 && ppi != 3) return FH_EINVAL;
  // Tile choice by workgroup count (256 CUs, the GEMMs are MFMA-bound: what matters is an even number of tile-units per
  // CU).  64x64 tiles halve the LDS/global traffic per flop but S = 256, 24 planes gives 384 of them = 1.5 per CU
  // (half the CUs carry two: 24 us); 64x32 tiles give 768 = exactly 3 half-size units per CU.
  // One plane per image (colorization): the 32 x 32 tiles (the smallest: a batch has few planes here; not tuned).
  const int64_t n64 = (int64_t)((S + 63) / 64) * ((S + 63) / 64) * planes;
  const int tile = ppi == 1 ? 0 : (n64 >= 1024 ? 1 : ((int64_t)((S + 31) / 32) * ((S + 63) / 64) * planes >= 512 ? 2 : 3));
  switch (tile) {
    case 0: dct_bases_pair<1, 1, 1>(ctx, st, b1, b2, in, out, planes, states, add, add_scale); break;
    case 1: dct_bases_pair<2, 2, 3>(ctx, st, b1, b2, in, out, planes, states, add, add_scale); break;
    case 2: dct_bases_pair<2, 1, 3>(ctx, st, b1, b2, in, out, planes, states, add, add_scale); break;
    default: dct_bases_pair<1, 1, 3>(ctx, st, b1, b2, in, out, planes, states, add, add_scale);
  }
  FH_LAUNCH_CHECK();
  return 0;
}

// whether the 2-D DCT of this context runs on the symmetric half-basis passes (k_dct_sym); FH_DCT_NOSYM=1 keeps the dense
// passes (A/B switch, read once per process)
static bool sym_dct(const fh_context* ctx) {
  static const bool no_sym = getenv("FH_DCT_NOSYM") != nullptr;
  return ctx->sym_fwd != nullptr && !no_sym;
}

// Launch plan of a symmetric pass over `planes` planes of side S (host arithmetic only).  One (plane, 32 x 32 tile) task
// is a fixed amount of work and a workgroup owns a CU (its LDS), so with more tasks than the 256 CUs a workgroup would run
// tasks back to back: then it runs two plane streams side by side (ns = 2, k_dct_sym<.., 2>), gz = ceil(planes / 2) capped
// at 256 workgroups.  Otherwise one stream per workgroup, the z extent filling the CUs.  A stream holds at most 8 planes.
// FH_DCT_STREAMS=1 keeps one stream per workgroup at every size (A/B switch, read once per process).
struct dct_sym_plan_t {
  int gx, gy, gz, ns;
  int64_t lds_bytes;
};
static dct_sym_plan_t dct_sym_plan(int S, int planes) {
  static const bool one_stream = getenv("FH_DCT_STREAMS") != nullptr && atoi(getenv("FH_DCT_STREAMS")) == 1;
  const int H = S / 2;
  dct_sym_plan_t pn;
  pn.gx = S / 32, pn.gy = H / 32;
  const int tiles = pn.gx * pn.gy, cap = 256 / tiles;
  pn.ns = (int64_t)planes * tiles > 256 && !one_stream ? 2 : 1;
  pn.gz = pn.ns == 2 ? ((planes + 1) / 2 < cap ? (planes + 1) / 2 : cap) : cap;
  const int need = (planes + 8 * pn.ns - 1) / (8 * pn.ns);  // streams of at most 8 planes
  if (pn.gz < need) pn.gz = need;
  if (pn.ns == 1 && pn.gz > planes) pn.gz = planes;
  if (pn.gz < 1) pn.gz = 1;
  // doubles: the resident slices, then [2 parities][32][66] staging buffers - two of one stream, or one of each of two
  pn.lds_bytes = ((int64_t)2 * 32 * (H + 2) + (int64_t)2 * 2 * 32 * 66) * (int64_t)sizeof(double);
  return pn;
}

// the two launches of a symmetric 2-D pass: along W into the context's intermediate, then along H with the epilogue operands
template <bool INV, int PPI, int NS>
static void dct_sym_pair(fh_context* ctx, dim3 grid, size_t lds, hipStream_t st, const double* sym_w, const double* sym_h,
                         const double* in, double* out, int planes, const fh_cg_state* states, const double* add,
                         double add_scale, const fh_diag_tab& dg, double* dot_part, int dot_stride) {
  fh_diag_tab none;
  memset(&none, 0, sizeof(none));
  hipLaunchKernelGGL((k_dct_sym<INV, PPI, NS>), grid, dim3(256 * NS), lds, st, sym_w, in, ctx->tmp_img, ctx->S, planes, states,
                     (const double*)nullptr, 0.0, none, (double*)nullptr, 0);
  hipLaunchKernelGGL((k_dct_sym<INV, PPI, NS>), grid, dim3(256 * NS), lds, st, sym_h, (const double*)ctx->tmp_img, out, ctx->S,
                     planes, states, add, add_scale, dg, dot_part, dot_stride);
}

// the two symmetric passes: tmp = (X P_w^T)^T, out = P_h X P_w^T (+ add_scale * add); sym_* = packed half bases [2][S/2][S/2]
static int dct2d_launch_sym(fh_context* ctx, const double* in, double* out, int planes, const double* sym_w,
                            const double* sym_h, int inverse, const double* add, double add_scale,
                            const fh_cg_state* states, hipStream_t st, const fh_batch* diag = nullptr,
                            double* dot_part = nullptr, int dot_stride = 0, int* dot_nparts = nullptr, int ppi = 3) {
  // ppi: planes per image (3; 1 = the one-plane measurement of the colorization operator: `planes` images, diag->D[i] one plane)
  const int S = ctx->S, H = S / 2;
  if (planes > ctx->planes_max || S % 128 != 0) return FH_ESIZE;
  if (ppi != 1 && ppi != 3) return FH_EINVAL;
  if (H % 64 != 0) return FH_ESIZE;  // K chunks of 64
  const dct_sym_plan_t pn = dct_sym_plan(S, planes);
  if (pn.lds_bytes > 140 * 1024) return FH_ESIZE;  // (the opt-in of set_kernel_attributes)
  const int gx = pn.gx, gy = pn.gy;
  const dim3 grid(gx, gy, pn.gz);
  fh_diag_tab dg;
  memset(&dg, 0, sizeof(dg));
  if (diag != nullptr)
    for (int i = 0; i < diag->nimg && i < FH_MAX_BATCH; ++i) dg.D[i] = diag->D[i];
  if (add == nullptr || ppi * gx * gy > 256) dot_part = nullptr;  // (the consumer sums <= 256 partials per image)
  if (dot_nparts != nullptr) *dot_nparts = dot_part != nullptr ? ppi * gx * gy : 0;
  const auto pair = pn.ns == 2
                        ? (ppi == 1 ? (inverse ? dct_sym_pair<true, 1, 2> : dct_sym_pair<false, 1, 2>)
                                    : (inverse ? dct_sym_pair<true, 3, 2> : dct_sym_pair<false, 3, 2>))
                        : (ppi == 1 ? (inverse ? dct_sym_pair<true, 1, 1> : dct_sym_pair<false, 1, 1>)  // (one plane per image)
                                    : (inverse ? dct_sym_pair<true, 3, 1> : dct_sym_pair<false, 3, 1>));
  pair(ctx, grid, (size_t)pn.lds_bytes, st, sym_w, sym_h, in, out, planes, states, add, add_scale, dg, dot_part, dot_stride);
  FH_LAUNCH_CHECK();
  return 0;
}

static int dct2d_launch(fh_context* ctx, const double* in, double* out, int planes, int inverse,
                        const fh_cg_state* states, hipStream_t st, int ppi = 3, const double* add = nullptr,
                        double add_scale = 0.0, double* dot_part = nullptr, int dot_stride = 0, int* dot_nparts = nullptr) {
  if (sym_dct(ctx)) {
    const double* sb = inverse ? ctx->sym_inv : ctx->sym_fwd;
    return dct2d_launch_sym(ctx, in, out, planes, sb, sb, inverse, add, add_scale, states, st, nullptr, dot_part, dot_stride,
                            dot_nparts, ppi);
  }
  const double* b1 = inverse ? ctx->basis_t : ctx->basis;
  return dct2d_launch_bases(ctx, in, out, planes, b1, b1, add, add_scale, states, st, ppi);
}

// Launch plan of one rectangular pass (host arithmetic only): 32 x 32 output tiles, and over z as few workgroups as walk the
// planes in the same number of trips as one workgroup per CU would (24 planes on 16 tiles: 12 x 2 planes, not 16 x 1 or 2).
struct dct_rect_plan_t {
  int gx, gy, gz;
  int64_t lds_bytes;
};
static dct_rect_plan_t dct_rect_plan(int KO, int KI, int R, int planes) {
  dct_rect_plan_t pn;
  pn.gx = (R + 31) / 32, pn.gy = (KO + 31) / 32;
  int cap = 256 / (pn.gx * pn.gy);
  if (cap < 1) cap = 1;
  if (cap > planes) cap = planes;
  const int trips = (planes + cap - 1) / cap;
  pn.gz = (planes + trips - 1) / trips;
  // doubles: the resident slice [32][KI padded to chunks of 32, + 2], then two [32][34] staging buffers
  pn.lds_bytes = ((int64_t)32 * ((KI + 31) / 32 * 32 + 2) + (int64_t)2 * 32 * 34) * (int64_t)sizeof(double);
  return pn;
}
constexpr int64_t kLdsRect = 140 * 1024;  // the opt-in of set_kernel_attributes (k_dct_sym's)

// (KO, KI, R) of pass A and pass B of a rectangular pair at image side S and measurement side So
static void dct_rect_shapes(int S, int So, int inverse, int shp[2][3]) {
  const int a[3] = {inverse ? So : S, inverse ? S : So, inverse ? S : So};
  const int b[3] = {inverse ? So : S, inverse ? S : So, inverse ? So : S};
  memcpy(shp[0], a, sizeof(a));
  memcpy(shp[1], b, sizeof(b));
}

static bool dct_rect_sizes_ok(int S, int So, int planes) {
  return S >= 2 && S <= 256 && (S & 1) == 0 && So >= 1 && So <= S && planes >= 1 && planes <= 65535;
}

// the two rectangular passes: forward  out [S][S] = P_h u P_w^T of u [So][So] (P_w, P_h [S][So]), inverse
// out [So][So] = P_h v P_w^T of v [S][S] (P_w, P_h [So][S]), (+ add_scale * add); tmp = the transposed result of pass A
static int dct_rect_launch(fh_context* ctx, const double* in, double* out, int planes, const double* P_w, const double* P_h,
                           int So, int inverse, const double* add, double add_scale, const fh_cg_state* states, hipStream_t st,
                           const fh_batch* diag = nullptr, double* dot_part = nullptr, int dot_stride = 0,
                           int* dot_nparts = nullptr) {
  const int S = ctx->S;
  if (dot_nparts != nullptr) *dot_nparts = 0;
  if (!dct_rect_sizes_ok(S, So, planes)) return FH_EINVAL;
  if (planes > ctx->planes_max) return FH_ESIZE;
  int shp[2][3];
  dct_rect_shapes(S, So, inverse, shp);
  const dct_rect_plan_t pa = dct_rect_plan(shp[0][0], shp[0][1], shp[0][2], planes);
  const dct_rect_plan_t pb = dct_rect_plan(shp[1][0], shp[1][1], shp[1][2], planes);
  if (pa.lds_bytes > kLdsRect || pb.lds_bytes > kLdsRect) return FH_ESIZE;
  fh_diag_tab none, dg;
  memset(&none, 0, sizeof(none));
  memset(&dg, 0, sizeof(dg));
  if (diag != nullptr)
    for (int i = 0; i < diag->nimg && i < FH_MAX_BATCH; ++i) dg.D[i] = diag->D[i];
  if (add == nullptr || 3 * pb.gx * pb.gy > 256) dot_part = nullptr;  // (the consumer sums <= 256 partials per image)
  if (dot_nparts != nullptr) *dot_nparts = dot_part != nullptr ? 3 * pb.gx * pb.gy : 0;
  hipLaunchKernelGGL(k_dct_rect<3>, dim3(pa.gx, pa.gy, pa.gz), dim3(256), (size_t)pa.lds_bytes, st, P_w, in, ctx->tmp_img,
                     shp[0][0], shp[0][1], shp[0][2], planes, states, (const double*)nullptr, 0.0, none, (double*)nullptr, 0);
  hipLaunchKernelGGL(k_dct_rect<3>, dim3(pb.gx, pb.gy, pb.gz), dim3(256), (size_t)pb.lds_bytes, st, P_h,
                     (const double*)ctx->tmp_img, out, shp[1][0], shp[1][1], shp[1][2], planes, states, add, add_scale, dg,
                     dot_part, dot_stride);
  FH_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Representation apply:  out = D.*z + r.*(B (M (B^T (r.*z))))
//   pass 1  k_rep_dots   : block partials of t = B^T (r.*z)
//   pass 1b k_rep_coef   : t = sum of partials (fixed order), c = M t        (one workgroup)
//   pass 2  k_rep_apply2 : out = D.*z + r.*(B c)
// B is read twice; pass 2 walks the rows in the opposite order so that the tail of pass 1 is still
// in the Infinity Cache / L2 when it is needed again.
// ------------------------------------------------------------------------------------------------
typedef double d2v_t __attribute__((ext_vector_type(2)));  // native vector type: usable with the nontemporal builtins
constexpr int kDotRows = 768;   // rows per workgroup (d = 196608 -> 256 workgroups, one per CU)
constexpr int kColChunk = 4;    // columns held in registers per wave and sweep

// pass 1: the 4 waves of a workgroup split the columns (wave w owns columns w, w+4, ...), lanes run along the
// rows with 16-byte loads.  The column loads are branch-free (out-of-range columns re-read column m-1 and are
// dropped at the end) so that a wave has (768/128) x 4 independent 1-KiB loads in flight (8 per wave cost 248 VGPRs,
// two waves per SIMD and 71 us per 403 MB sweep at 8 images; 4 -> four waves per SIMD, 66 us; a pure streaming read of
// the same bytes with this access pattern takes 61 us, profiles/r02_cov_apply_single_sweep.md).  Each wave writes its sums as block
// partials; k_rep_coef (one 1024-thread workgroup) adds them in a fixed order and forms c = M t.  (float64 atomics
// into a shared m-vector were measured 2x SLOWER than this: 8192 same-address adds serialise at the memory side.)
// NT: non-temporal loads of B.  A base that does not fit the 256 MB Infinity Cache anyway (8 images x 32 columns = 403 MB)
// streams 1-4 % faster without allocating there; a smaller one (8 x 16 columns = 201 MB) is re-read from the cache by pass 2
// and by the next CG iteration, and non-temporal loads cost 15-20 % (measured 97 vs 81 us per batched apply at m = 16).
template <bool NT>
__device__ __forceinline__ d2v_t ld_base(const double* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const d2v_t*>(p));
  return *reinterpret_cast<const d2v_t*>(p);
}

template <bool NT>
__device__ __forceinline__ double ld_base1(const double* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}

template <bool NT>
__global__ __launch_bounds__(256) void k_rep_dots(fh_batch per, const double* __restrict__ z,
                                                  double* __restrict__ partial, int64_t d, int m,
                                                  const fh_cg_state* __restrict__ states) {
  const int img = blockIdx.z;
  IMG_GUARD(states, img);
  const double* __restrict__ B = per.B[img];
  const double* __restrict__ r = per.r[img];
  z += (int64_t)img * d;
  partial += (int64_t)img * kPartialRows * FH_MAX_COLS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kDotRows;
  constexpr int kIter = kDotRows / 128;  // row pairs per lane
  double2 rz[kIter];
  int64_t row[kIter];
#pragma unroll
  for (int it = 0; it < kIter; ++it) {
    int64_t i = r0 + it * 128 + 2 * lane;
    const bool ok = i + 1 < d;
    i = ok ? i : 0;  // clamped rows contribute zero
    row[it] = i;
    const double2 zz = *reinterpret_cast<const double2*>(z + i);
    const double2 rr = *reinterpret_cast<const double2*>(r + i);
    rz[it] = ok ? make_double2(zz.x * rr.x, zz.y * rr.y) : make_double2(0.0, 0.0);
  }
  for (int q0 = 0; w + 4 * q0 < m; q0 += kColChunk) {
    double acc[kColChunk];
#pragma unroll
    for (int q = 0; q < kColChunk; ++q) acc[q] = 0.0;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
#pragma unroll
      for (int q = 0; q < kColChunk; ++q) {
        const int j = w + 4 * (q0 + q);
        const int jc = j < m ? j : m - 1;
        const d2v_t b = ld_base<NT>(B + (int64_t)jc * d + row[it]);
        acc[q] = fma(b.x, rz[it].x, fma(b.y, rz[it].y, acc[q]));
      }
    }
#pragma unroll
    for (int q = 0; q < kColChunk; ++q) {
      const double v = wave_sum(acc[q]);
      const int j = w + 4 * (q0 + q);
      if (lane == 0 && j < m) partial[(int64_t)blockIdx.x * FH_MAX_COLS + j] = v;
    }
  }
}

// pass 1b: t[j] = sum_b partial[b][j] (fixed order -> deterministic), c = M t.  One workgroup of 1024 threads:
// 32 row-groups x 32 columns keep nparts/32 coalesced loads per thread in flight.
__global__ __launch_bounds__(1024) void k_rep_coef(fh_batch per, const double* __restrict__ partial, int nparts,
                                                   int ldm, int m, double* __restrict__ coef,
                                                   const fh_cg_state* __restrict__ states) {
  const int img = blockIdx.z;
  IMG_GUARD(states, img);
  const double* __restrict__ M = per.M[img];
  partial += (int64_t)img * kPartialRows * FH_MAX_COLS;
  coef += (int64_t)img * 2 * FH_MAX_COLS;
  __shared__ double t[FH_MAX_COLS];
  __shared__ double red[32][33];
  const int tid = threadIdx.x, jj = tid & 31, rg = tid >> 5;
  for (int j0 = 0; j0 < m; j0 += 32) {
    const int j = j0 + jj;
    double s0 = 0.0, s1 = 0.0;
    if (j < m) {
      int b = rg;
      for (; b + 32 < nparts; b += 64) {
        s0 += partial[(int64_t)b * FH_MAX_COLS + j];
        s1 += partial[(int64_t)(b + 32) * FH_MAX_COLS + j];
      }
      for (; b < nparts; b += 32) s0 += partial[(int64_t)b * FH_MAX_COLS + j];
    }
    red[rg][jj] = s0 + s1;
    __syncthreads();
    if (rg == 0 && j < m) {
      double sum = 0.0;
#pragma unroll
      for (int g = 0; g < 32; ++g) sum += red[g][jj];
      t[j] = sum;
      coef[FH_MAX_COLS + j] = sum;  // t = B^T (r.*z) itself (read by the closed-form BFGS inverse of the space update)
    }
    __syncthreads();
  }
  // c = M t : 32 threads per output row (rows in groups of 32), shuffle-reduced
  for (int r0 = 0; r0 < m; r0 += 32) {
    const int rowi = r0 + rg;
    double sum = 0.0;
    if (rowi < m)
      for (int l = jj; l < m; l += 32) sum = fma(M[(int64_t)rowi * ldm + l], t[l], sum);
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    sum += __shfl_xor(sum, 8, 64);
    sum += __shfl_xor(sum, 16, 64);
    if (rowi < m && jj == 0) coef[rowi] = sum;
  }
}

// pass 2: out = D.*z + r.*(B c), rows swept in the opposite order of pass 1 (Infinity-Cache reuse).
template <bool NT>
__global__ __launch_bounds__(256) void k_rep_apply2(fh_batch per, const double* __restrict__ coef,
                                                    const double* __restrict__ z, double* __restrict__ out,
                                                    int64_t d, int m, const fh_cg_state* __restrict__ states) {
  const int img = (int)gridDim.z - 1 - (int)blockIdx.z;  // images too in reverse: the last bases of pass 1 are still in the 256 MB Infinity Cache
  IMG_GUARD(states, img);
  const double* __restrict__ D = per.D[img];
  const double* __restrict__ r = per.r[img];
  const double* __restrict__ B = per.B[img];
  coef += (int64_t)img * 2 * FH_MAX_COLS;
  z += (int64_t)img * d;
  out += (int64_t)img * d;
  const int tid = threadIdx.x;
  __shared__ double c[FH_MAX_COLS];
  for (int j = tid; j < m; j += 256) c[j] = coef[j];
  __syncthreads();
  const int64_t blk = (int64_t)gridDim.x - 1 - blockIdx.x;  // reverse sweep
  // every thread owns three rows of the block (row = block start + 256 q + tid: coalesced 8-byte loads): equal work for the
  // 256 threads, any d (the former row-pair mapping needed an even d and left half of the lanes idle in a second trip)
  constexpr int kR = kDotRows / 256;
  int64_t row[kR];
  bool ok[kR];
#pragma unroll
  for (int q = 0; q < kR; ++q) {
    const int64_t i = blk * kDotRows + 256 * q + tid;
    ok[q] = i < d;
    row[q] = ok[q] ? i : 0;
  }
  // canonical summation order of (B c)_i, shared with the single-sweep kernel k_rep_fused (whose 8 waves each own the
  // columns j = w (mod 8)): eight chains over j = w, w + 8, ... then the chains added in the order w = 0 .. 7
  double ch[8][kR];
#pragma unroll
  for (int w8 = 0; w8 < 8; ++w8)
#pragma unroll
    for (int q = 0; q < kR; ++q) ch[w8][q] = 0.0;
  // the three per-row vectors are requested before the base: their latency hides behind the sweep instead of its tail
  double zq[kR], dq[kR], rq[kR];
#pragma unroll
  for (int q = 0; q < kR; ++q) zq[q] = z[row[q]], dq[q] = D[row[q]], rq[q] = m > 0 ? r[row[q]] : 0.0;
  const int mfull = m & ~7;
  for (int j0 = 0; j0 < mfull; j0 += 8) {  // 24 independent streaming loads per step
    double b[8][kR];
#pragma unroll
    for (int w8 = 0; w8 < 8; ++w8)
#pragma unroll
      for (int q = 0; q < kR; ++q) b[w8][q] = ld_base1<NT>(B + (int64_t)(j0 + w8) * d + row[q]);
#pragma unroll
    for (int w8 = 0; w8 < 8; ++w8) {
      const double cj = c[j0 + w8];
#pragma unroll
      for (int q = 0; q < kR; ++q) ch[w8][q] = fma(b[w8][q], cj, ch[w8][q]);
    }
  }
#pragma unroll
  for (int w8 = 0; w8 < 8; ++w8) {
    const int j = mfull + w8;
    if (j < m) {
      const double cj = c[j];
#pragma unroll
      for (int q = 0; q < kR; ++q) ch[w8][q] = fma(ld_base1<NT>(B + (int64_t)j * d + row[q]), cj, ch[w8][q]);
    }
  }
#pragma unroll
  for (int q = 0; q < kR; ++q) {
    double acc = ch[0][q];
#pragma unroll
    for (int w8 = 1; w8 < 8; ++w8) acc += ch[w8][q];
    const double o = m > 0 ? fma(rq[q], acc, dq[q] * zq[q]) : dq[q] * zq[q];
    if (ok[q]) out[row[q]] = o;
  }
}

// ------------------------------------------------------------------------------------------------
// Single-sweep representation apply (k_rep_fused): B is read ONCE.
// The two-pass form above is bound by its second sweep of the factor base (2 x 8 d m bytes; the base of 8 lock-step
// images, 400 MB, does not fit the 256 MB Infinity Cache).  Here a 512-thread workgroup keeps its 768-row x m slice of
// B in REGISTERS (wave w owns the columns j = w (mod 8): 6 row pairs x MC columns = 48 / 96 doubles per lane at
// m <= 32 / 64) between the reduction t = B^T (r.*z) and the product B (M t):
//   phase 1  slice -> registers, block partials of t (same per-column arithmetic as k_rep_dots), sc1 stores
//   arrive   every wave drains its stores, workgroup barrier, one relaxed agent-scope add on the image's counter
//   wait     thread 0 polls the counter with relaxed sc1 loads + s_sleep (BOUNDED: on time-out the error word of the
//            context is set and the workgroup leaves - every wave reaches its exit)
//   phase 2  every workgroup re-reduces the nb x m partials with sc1 loads (64 KB from L2 / fabric; same fixed order
//            as k_rep_coef), forms c = M t, multiplies its register slice, adds the 8 per-wave chains through LDS in the
//            canonical order and writes out = D.*z + r.*(B c)
//   depart   the last workgroup to finish reading the partials resets the image's two counters
// The hand-off follows the MI355X guide's measured counter form: sc1 (write-through) stores -> s_waitcnt vmcnt(0) in
// every storing wave -> workgroup barrier -> one lane's agent-scope atomic add; consumer: relaxed sc1 poll by one wave,
// workgroup barrier, sc1 loads of every handed-off byte.  No fence, no placement assumption.
// Residency: images are dispatched in order (blockIdx.z slowest), an image's nb <= #CU workgroups fit the chip at once
// (1 or 2 workgroups per CU by register budget) and finished workgroups never wait on later images, so every counter
// completes PROVIDED no other grid-synchronising kernel runs concurrently - the launcher takes this path only on a
// context the caller declared exclusive (fh_context_set_exclusive); everything else keeps the two-pass kernels.
// ------------------------------------------------------------------------------------------------
constexpr int kFusedSpinLimit = 1 << 21;  // x s_sleep(2) ~ 64 clocks: ~ 0.1 s before a workgroup gives up
constexpr int kSyncStride = 64;           // uint32 per image: arrive counter at +0, depart counter at +32 (own 128-B lines)

template <int MC>
__global__ __launch_bounds__(512, MC <= 4 ? 4 : 2) void k_rep_fused(fh_batch per, const double* __restrict__ z,
                                                                    double* __restrict__ out, double* __restrict__ partial,
                                                                    unsigned int* __restrict__ sync, int64_t d, int m,
                                                                    int ldm, const fh_cg_state* __restrict__ states,
                                                                    unsigned long long* __restrict__ dbg) {
  const int img = blockIdx.z;
  IMG_GUARD(states, img);
  // dbg != null (profiling builds of the launcher only): thread 0 records the 100 MHz wall clock at the phase boundaries
#define FUSED_STAMP(k)                                                                                          \
  if (dbg != nullptr && threadIdx.x == 0)                                                                       \
  dbg[((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * 8 + (k)] = __builtin_amdgcn_s_memrealtime()
  FUSED_STAMP(0);
  const double* __restrict__ B = per.B[img];
  const double* __restrict__ r = per.r[img];
  const double* __restrict__ D = per.D[img];
  const double* __restrict__ M = per.M[img];
  z += (int64_t)img * d;
  out += (int64_t)img * d;
  partial += (int64_t)img * kPartialRows * FH_MAX_COLS;
  unsigned int* arrive = sync + img * kSyncStride;
  unsigned int* depart = arrive + 32;
  unsigned int* err = sync + FH_MAX_BATCH * kSyncStride;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nb = gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * kDotRows + 2 * lane;  // d is a multiple of kDotRows on this path
  constexpr int kIter = kDotRows / 128;

  constexpr int MS = 8 * MC;                          // columns this instantiation can hold
  __shared__ __align__(16) double psum[8][kDotRows];  // phase 1: r.*z; phase 2a: reduction scratch; 2c: per-wave chains of (B c)
  __shared__ __align__(16) double dzs[kDotRows], rrs[kDotRows];  // D.*z and r of the workgroup's rows (read before the barrier)
  __shared__ double Msh[MS][MS + 1];                  // the inner matrix, staged before the barrier as well
  __shared__ double tsh[64], csh[64];
  __shared__ int ok_s;
  double(*red)[33] = reinterpret_cast<double(*)[33]>(&psum[1][0]);  // [32][33] doubles inside psum (free in phase 2a)

  // ---- phase 1: r.*z of the workgroup's rows goes through LDS (every wave needs all of it; holding it in registers next
  // to the slice would spill at the 128-VGPR budget of two workgroups per CU)
  double* rzs = &psum[0][0];
  if (tid < kDotRows / 2) {
    const int64_t i0 = (int64_t)blockIdx.x * kDotRows + 2 * tid;
    const double2 zz = *reinterpret_cast<const double2*>(z + i0);
    const double2 rr = *reinterpret_cast<const double2*>(r + i0);
    const double2 dd = *reinterpret_cast<const double2*>(D + i0);
    *reinterpret_cast<double2*>(rzs + 2 * tid) = make_double2(zz.x * rr.x, zz.y * rr.y);
    *reinterpret_cast<double2*>(dzs + 2 * tid) = make_double2(dd.x * zz.x, dd.y * zz.y);
    *reinterpret_cast<double2*>(rrs + 2 * tid) = rr;
  } else {
    // the other two waves stage M (everything the latency chain after the barrier would otherwise have to fetch)
    for (int i = tid - kDotRows / 2; i < m * m; i += 512 - kDotRows / 2) Msh[i / m][i % m] = M[(int64_t)(i / m) * ldm + i % m];
  }
  double2 breg[MC][kIter];
#pragma unroll
  for (int q = 0; q < MC; ++q) {
    const int j = w + 8 * q;  // wave-uniform
    if (j < m) {
      const double* bp = B + (int64_t)j * d + r0;
#pragma unroll
      for (int it = 0; it < kIter; ++it) breg[q][it] = *reinterpret_cast<const double2*>(bp + it * 128);
    } else {
#pragma unroll
      for (int it = 0; it < kIter; ++it) breg[q][it] = make_double2(0.0, 0.0);
    }
  }
  __syncthreads();  // r.*z, D.*z, r and M are in LDS
#pragma unroll
  for (int q = 0; q < MC; ++q) {
    double acc = 0.0;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
      const double2 rz = *reinterpret_cast<const double2*>(rzs + it * 128 + 2 * lane);
      acc = fma(breg[q][it].x, rz.x, fma(breg[q][it].y, rz.y, acc));
    }
    const double v = wave_sum(acc);
    const int j = w + 8 * q;
    if (lane == 0 && j < m)
      __hip_atomic_store(partial + (int64_t)blockIdx.x * FH_MAX_COLS + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::: "memory");  // re-read r.*z from LDS for the next column instead of keeping it live
  }
  // ---- arrive + wait
  FUSED_STAMP(1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  FUSED_STAMP(2);
  if (tid == 0) {
    __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int ok = 1, spins = 0;
    while (__hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)nb) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > kFusedSpinLimit) {
        ok = 0;
        break;
      }
    }
    if (!ok) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ok_s = ok;
  }
  __syncthreads();
  if (!ok_s) return;  // uniform: every wave of the workgroup leaves
  FUSED_STAMP(3);

  // ---- phase 2a: t = sum of the block partials, in k_rep_coef's order: row group rg = 0..31 adds the blocks
  // rg, rg + 64, ... into one chain and rg + 32, rg + 96, ... into a second one.  The 16 sc1 loads of a thread are issued
  // back to back (inline asm: the compiler would wait after every atomic load) and drained by ONE s_waitcnt that the
  // results are tied to.
  const int jj = tid & 31, rg2 = tid >> 5;
  for (int j0 = 0; j0 < m; j0 += 32) {
    const int j = j0 + jj;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // scalar base + 32-bit lane offset: one address VGPR per load keeps the batch inside the 128-VGPR budget
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int b = rg2 + 16 * h + 32 * i;
        v[i] = 0.0;
        if (j < m && b < nb) {
          const unsigned int off = (unsigned int)((b * FH_MAX_COLS + j) * (int)sizeof(double));
          asm volatile("global_load_dwordx2 %0, %1, %2 sc1" : "=v"(v[i]) : "v"(off), "s"(partial) : "memory");
        }
      }
      asm volatile("s_waitcnt vmcnt(0)"
                   : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
                   :
                   : "memory");
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int i = 0; i < 8; i += 2) s0 += v[i], s1 += v[i + 1];
      red[rg2 + 16 * h][jj] = s0 + s1;
    }
    __syncthreads();
    if (rg2 == 0 && j < m) {
      double sum = 0.0;
#pragma unroll
      for (int g = 0; g < 32; ++g) sum += red[g][jj];
      tsh[j] = sum;
    }
    __syncthreads();
  }
  FUSED_STAMP(4);
  // every partial this workgroup needs has been read: depart; the last one re-arms the image's counters for the next launch
  if (tid == 0) {
    const unsigned int prev = __hip_atomic_fetch_add(depart, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == (unsigned)nb - 1u) {
      __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(depart, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // ---- phase 2b: c = M t (32 threads per row, as k_rep_coef)
  for (int q0 = 0; q0 < m; q0 += 16) {
    const int rowi = q0 + rg2;
    double sum = 0.0;
    if (rowi < m)
      for (int l = jj; l < m; l += 32) sum = fma(Msh[rowi][l], tsh[l], sum);
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    sum += __shfl_xor(sum, 8, 64);
    sum += __shfl_xor(sum, 16, 64);
    if (rowi < m && jj == 0) csh[rowi] = sum;
  }
  __syncthreads();
  // ---- phase 2c: this wave's chain over its columns, from registers
  {
    double cq[MC];
#pragma unroll
    for (int q = 0; q < MC; ++q) cq[q] = (w + 8 * q < m) ? csh[w + 8 * q] : 0.0;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
      double2 p = make_double2(0.0, 0.0);
#pragma unroll
      for (int q = 0; q < MC; ++q) {
        p.x = fma(breg[q][it].x, cq[q], p.x);
        p.y = fma(breg[q][it].y, cq[q], p.y);
      }
      *reinterpret_cast<double2*>(&psum[w][it * 128 + 2 * lane]) = p;
    }
  }
  __syncthreads();
  FUSED_STAMP(5);
  // ---- phase 2d: out = D.*z + r.*(chains added in the order w = 0 .. 7)
  if (tid < kDotRows / 2) {
    double2 acc = *reinterpret_cast<const double2*>(&psum[0][2 * tid]);
#pragma unroll
    for (int w8 = 1; w8 < 8; ++w8) {
      const double2 p = *reinterpret_cast<const double2*>(&psum[w8][2 * tid]);
      acc.x += p.x, acc.y += p.y;
    }
    const int64_t i0 = (int64_t)blockIdx.x * kDotRows + 2 * tid;
    const double2 dz = *reinterpret_cast<const double2*>(dzs + 2 * tid);
    const double2 rr = *reinterpret_cast<const double2*>(rrs + 2 * tid);
    *reinterpret_cast<double2*>(out + i0) = make_double2(fma(rr.x, acc.x, dz.x), fma(rr.y, acc.y, dz.y));
  }
  FUSED_STAMP(6);
#undef FUSED_STAMP
}

static int rep_apply_launch(fh_context* ctx, const fh_batch& per, int ldm, const double* z, double* out, int64_t d,
                            int m, const fh_cg_state* states, hipStream_t st) {
  if (m < 0 || m > FH_MAX_COLS || (d & 1) || per.nimg < 1 || per.nimg > ctx->nimg_max) return FH_ESIZE;
  const int nb = (int)((d + kDotRows - 1) / kDotRows);
  if (nb > kPartialRows) return FH_ESIZE;
  // All images of a batch go through pass 1, then pass 2 in reverse image (and row) order, so that the bases read last
  // are re-read first while they are still in the 256 MB Infinity Cache.  Measured at 8 images, m = 32 (algorithmic
  // TB/s): same order 2.75, reverse order 2.97; splitting the batch into cache-sized groups of 4 (each group both
  // passes back to back) 2.80 - the extra dependent launches cost more than the additional hits return.
  const unsigned Z = (unsigned)per.nimg;
  // Single-sweep kernel: only on explicit request (fh_context_set_exclusive(ctx, 2): tests, profiling).  It reads the base once
  // and is bitwise equal, but since the two sweeps run at the per-CU ingest limit it is no longer faster anywhere: one image
  // per launch 26.0-27.0 us vs 25.5 us, eight images 161-177 us vs 139.5 us (the hand-off of one image goes through the same
  // per-CU memory queues as the next image's streaming loads and stretches from 13 us to 19 us, see
  // profiles/r02_cov_apply_single_sweep.md).
  if (out != nullptr && m > 0 && m <= 64 && ctx->exclusive >= 2 && !ctx->fused_disabled && d % kDotRows == 0 &&
      nb <= ctx->num_cus && nb <= 256) {
    unsigned long long* dbg = getenv("FH_FUSED_DEBUG") ? (unsigned long long*)ctx->gpartial : nullptr;  // profiling only
    if (m <= 32)
      hipLaunchKernelGGL((k_rep_fused<4>), dim3(nb, 1, Z), dim3(512), 0, st, per, z, out, ctx->partial, ctx->sync, d, m, ldm,
                         states, dbg);
    else
      hipLaunchKernelGGL((k_rep_fused<8>), dim3(nb, 1, Z), dim3(512), 0, st, per, z, out, ctx->partial, ctx->sync, d, m, ldm,
                         states, dbg);
    FH_LAUNCH_CHECK();
    return 0;
  }
  const bool nt = (int64_t)per.nimg * m * d * (int64_t)sizeof(double) > ((int64_t)220 << 20);  // beyond the Infinity Cache
  if (m > 0) {
    if (nt)
      hipLaunchKernelGGL(k_rep_dots<true>, dim3(nb, 1, Z), dim3(256), 0, st, per, z, ctx->partial, d, m, states);
    else
      hipLaunchKernelGGL(k_rep_dots<false>, dim3(nb, 1, Z), dim3(256), 0, st, per, z, ctx->partial, d, m, states);
    hipLaunchKernelGGL(k_rep_coef, dim3(1, 1, Z), dim3(1024), 0, st, per, (const double*)ctx->partial, nb, ldm, m,
                       ctx->coef, states);
  }
  if (out != nullptr) {  // out == null: only t = B^T (r.*z) and c = M t are wanted (left in ctx->coef[FH_MAX_COLS..] / [0..])
    if (nt)
      hipLaunchKernelGGL(k_rep_apply2<true>, dim3(nb, 1, Z), dim3(256), 0, st, per, (const double*)ctx->coef, z, out, d, m,
                         states);
    else
      hipLaunchKernelGGL(k_rep_apply2<false>, dim3(nb, 1, Z), dim3(256), 0, st, per, (const double*)ctx->coef, z, out, d, m,
                         states);
  }
  FH_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Representation inverse (Woodbury) - diagonal part + weighted Gram  G = B^T diag(rx^2/Dx) B.
//   k_invert_diag : Dx += shift, Dy = 1/Dx, ry = rx/Dx
//   k_gram        : grid (row blocks, 64x64 tile pairs ta<=tb); each workgroup streams its rows in chunks of 64
//                   through LDS; wave w accumulates the 16-row strip w of the pair on v_mfma_f64_16x16x4_f64
//                   (one LDS read per operand per 1024 FMAs; sub-tiles beyond column m are skipped)
//   k_gram_reduce : sums the row-block partials, writes both triangles
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_invert_diag(PtrTab Dxt, PtrTab rxt, double shift, PtrTab Dyt, PtrTab ryt,
                                                     int64_t d) {
  double* __restrict__ Dx = Dxt.p[blockIdx.z];
  const double* __restrict__ rx = rxt.p[blockIdx.z];
  double* __restrict__ Dy = Dyt.p[blockIdx.z];
  double* __restrict__ ry = ryt.p[blockIdx.z];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= d) return;
  const double v = Dx[i] + shift;
  Dx[i] = v;
  Dy[i] = 1.0 / v;
  if (rx != nullptr) ry[i] = rx[i] / v;
}

// forward time shift of a representation and of its inverse: D <- D / (1 + s D), r <- r / (1 + s D), Dinv <- Dinv + s
__global__ __launch_bounds__(256) void k_forward_diag(PtrTab Dt, PtrTab rt_, PtrTab Dinvt, double s, int64_t d) {
  double* __restrict__ D = Dt.p[blockIdx.z];
  double* __restrict__ r = rt_.p[blockIdx.z];
  double* __restrict__ Dinv = Dinvt.p[blockIdx.z];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= d) return;
  const double e = 1.0 / fma(s, D[i], 1.0);
  D[i] *= e;
  r[i] *= e;
  Dinv[i] += s;
}

constexpr int kGramRowBlocks = 512;  // 384 rows each at d = 196608: two workgroups per CU
constexpr int kGT = 64;  // Gram tile edge and row-chunk length

// fwd = 0: weights rx^2 / Dx (Woodbury inverse of the representation); fwd = 1: rx^2 / (1 + fshift Dx) (forward time
// shift of the representation itself, see cov_shift_forward)
__global__ __launch_bounds__(256) void k_gram(PtrTab Bt, PtrTab rxt, PtrTab Dxt, double* __restrict__ gpartial,
                                              int64_t gstride, int64_t d, int m, int ntiles, int fwd, double fshift) {
  const double* __restrict__ B = Bt.p[blockIdx.z];   // grid z = image
  const double* __restrict__ rx = rxt.p[blockIdx.z];
  const double* __restrict__ Dx = Dxt.p[blockIdx.z];
  gpartial += (int64_t)blockIdx.z * gstride;
  __shared__ double As[kGT][kGT + 1];  // [row i][col of tile a], weighted
  __shared__ double Bs[kGT][kGT + 1];  // [row i][col of tile b]
  // decode tile pair
  int ta = 0, tb = 0, p = blockIdx.y;
  for (ta = 0; ta < ntiles; ++ta) {
    const int cnt = ntiles - ta;
    if (p < cnt) {
      tb = ta + p;
      break;
    }
    p -= cnt;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  // 16 x 16 sub-tiles of the 64 x 64 pair that hold columns < m; wave w owns sub-tile row w (f64 MFMA 16x16x4:
  // a = A[i = l & 15][k = l >> 4], b = B[k = l >> 4][j = l & 15], C: col = l & 15, row = (l >> 4) + 4 reg)
  const int ma = m - ta * kGT < kGT ? m - ta * kGT : kGT, mb = m - tb * kGT < kGT ? m - tb * kGT : kGT;
  const int na = (ma + 15) / 16, nbt = (mb + 15) / 16;
  const bool active = wave < na;
  const int64_t rows_per = ((d + gridDim.x - 1) / gridDim.x + kGT - 1) / kGT * kGT;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per;
  const int64_t r1 = r0 + rows_per < d ? r0 + rows_per : d;
  double4_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (double4_t){0.0, 0.0, 0.0, 0.0};
  // On the diagonal pair only sub-tiles on or above the diagonal are formed (G is symmetric; k_gram_reduce mirrors).
  const int j_lo = ta == tb ? wave : 0;
  const int row = tid & 63;
  for (int64_t c0 = r0; c0 < r1; c0 += kGT) {
    // all loads of the chunk are issued before the first LDS store; columns beyond the last live sub-tile are not
    // fetched and the diagonal pair loads its columns once.  (Prefetching chunk c + 1 into registers across the MFMA
    // phase was measured slower: the allocator then needs > 256 VGPRs and the kernel drops to one workgroup per CU.)
    const int64_t gi = c0 + row;
    const bool rok = gi < r1;
    const double wgt = rok ? rx[gi] * rx[gi] / (fwd ? fma(fshift, Dx[gi], 1.0) : Dx[gi]) : 0.0;
    double va[16], vb[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int col = e * 4 + (tid >> 6);
      const int ja = ta * kGT + col, jb = tb * kGT + col;
      vb[e] = (col < 16 * nbt && rok && jb < m) ? B[(int64_t)jb * d + gi] : 0.0;
      va[e] = ta == tb ? vb[e] : ((col < 16 * na && rok && ja < m) ? B[(int64_t)ja * d + gi] : 0.0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int col = e * 4 + (tid >> 6);
      if (col < 16 * na) As[row][col] = va[e] * wgt;
      if (col < 16 * nbt) Bs[row][col] = vb[e];
    }
    __syncthreads();
    if (active) {
#pragma unroll 4
      for (int kk = 0; kk < kGT; kk += 4) {
        const double av = As[kk + lk][16 * wave + li];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j >= j_lo && j < nbt)
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bs[kk + lk][16 * j + li], acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!active) return;
  double* dst = gpartial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (kGT * kGT);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < j_lo || j >= nbt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(16 * wave + lk + 4 * r) * kGT + 16 * j + li] = acc[j][r];
  }
}
__global__ __launch_bounds__(256) void k_gram_reduce(const double* __restrict__ gpartial, int64_t gstride, int nrb,
                                                     int ntiles, int m, PtrTab Gt, int ldg) {
  double* __restrict__ G = Gt.p[blockIdx.z];
  gpartial += (int64_t)blockIdx.z * gstride;
  // grid (tile pairs, 64): a workgroup owns 64 consecutive tile outputs; its 4 waves each sum a quarter of the nrb
  // row-block partials (coalesced 512-byte rows, 4 independent chains), then the quarters are added in a fixed order.
  int ta = 0, tb = 0, p = blockIdx.x;
  for (ta = 0; ta < ntiles; ++ta) {
    const int cnt = ntiles - ta;
    if (p < cnt) {
      tb = ta + p;
      break;
    }
    p -= cnt;
  }
  __shared__ double red[4][64];
  const double* src = gpartial + (int64_t)blockIdx.x * nrb * (kGT * kGT);
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int o_out = blockIdx.y * 64 + lane;
  const int a = ta * kGT + o_out / kGT, c = tb * kGT + o_out % kGT;
  const bool live = a < m && c < m;  // k_gram writes only sub-tiles that hold columns < m
  // diagonal pair: sub-tiles below the diagonal were not formed - read the mirrored entry
  const bool mirror = ta == tb && (o_out / kGT) / 16 > (o_out % kGT) / 16;
  const int o = mirror ? (o_out % kGT) * kGT + o_out / kGT : o_out;
  const int per = (nrb + 3) / 4;
  const int b0 = q * per, b1 = b0 + per < nrb ? b0 + per : nrb;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (live) {
    int b = b0;
    for (; b + 3 < b1; b += 4) {
      s0 += src[(int64_t)b * (kGT * kGT) + o];
      s1 += src[(int64_t)(b + 1) * (kGT * kGT) + o];
      s2 += src[(int64_t)(b + 2) * (kGT * kGT) + o];
      s3 += src[(int64_t)(b + 3) * (kGT * kGT) + o];
    }
    for (; b < b1; ++b) s0 += src[(int64_t)b * (kGT * kGT) + o];
  }
  red[q][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (q == 0 && live) {
    const double s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    G[(int64_t)a * ldg + c] = s;
    if (ta != tb) G[(int64_t)c * ldg + a] = s;
  }
}

// ------------------------------------------------------------------------------------------------
// Elementwise helpers and scalar reductions
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_axpby(double alpha, const double* __restrict__ a, double beta,
                                               const double* __restrict__ b, double* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double v = alpha * a[i];
    if (b != nullptr) v = fma(beta, b[i], v);
    out[i] = v;
  }
}

// out = mask .* in  (add == null)   |   out = add_scale*add + mask .* in      (grid z = image)
__global__ __launch_bounds__(256) void k_mask(fh_batch per, const double* __restrict__ in,
                                              const double* __restrict__ add, double add_scale,
                                              double* __restrict__ out, int64_t n,
                                              const fh_cg_state* __restrict__ states) {
  const int img = blockIdx.z;
  IMG_GUARD(states, img);
  const double* __restrict__ mask = per.mask[img];
  in += (int64_t)img * n;
  out += (int64_t)img * n;
  if (add != nullptr) add += (int64_t)img * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double v = mask[i] * in[i];
    if (add != nullptr) v = fma(add_scale, add[i], v);
    out[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// Hartley butterfly (fh_hartley_fix, fh_hartley2d, fh_problem.op = 15).  With Hc[u][n] = (cos + sin)(2 pi u n / S) / sqrt(S) the
// separable transform T = Hc X Hc is NOT the 2-D discrete Hartley transform H X = Re F X - Im F X; the butterfly
//   R(T)[u][v] = 1/2 ((T[u][v] + T[-u][v]) + (T[u][-v] - T[-u][-v])),        -u = (S - u) % S
// turns one into the other (cas(a + b) = 1/2 (cas a cas b + cas(-a) cas b + cas a cas(-b) - cas(-a) cas(-b))), and R R = I.
// A work unit is a row pair (u, -u), u = 0 .. S/2 (rows 0 and S/2 are their own reflections): the workgroup stages both rows
// (times the input weights, the product rounded) in LDS with 16-byte loads, then every thread forms a 16-byte pair of outputs
// of either row, reading the two staged rows at the mirrored columns in reverse.  Block x of the grid owns units x, x + gridDim.x,
// ... of every plane it visits, grid y walks the planes (p, p + gridDim.y, ...): which elements a block sums for the p.Ap
// partial of (image, channel, block x), and in what order, depends on S alone - a batched solve repeats the single one.
//   value = 1/2 ((a + b) + (c - d)) in that order;  with output weights w * value (rounded);  with add fma(add_scale, add, .)
// Weights: plane p reads table[image] + (p % 3) S S (`wshared`: table[0] for every image, the entry point's one map).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hartley_fix(const double* __restrict__ in, double* __restrict__ out, int S, int planes,
                                                     fh_diag_tab win, fh_diag_tab wout, int wshared,
                                                     const double* __restrict__ add, double add_scale,
                                                     const fh_cg_state* __restrict__ states, double* __restrict__ dot_part,
                                                     int dot_stride) {
#pragma clang fp contract(off)  // the sums and the weight products are rounded one by one; fma() below stays an fma
  extern __shared__ __align__(16) double hrows[];  // [2][S]: row u, row -u (weighted)
  __shared__ double red[4];
  const int tid = threadIdx.x, H = S / 2, units = H + 1;
  const int64_t SS = (int64_t)S * S;
  for (int p = (int)blockIdx.y; p < planes; p += (int)gridDim.y) {
    const int img = p / 3, c = p % 3;
    if (states != nullptr && states[img].done != 0) continue;  // (uniform over the workgroup)
    const double* X = in + p * SS;
    double* Y = out + p * SS;
    const double* Wi = win.D[0] != nullptr ? win.D[wshared ? 0 : img] + c * SS : nullptr;
    const double* Wo = wout.D[0] != nullptr ? wout.D[wshared ? 0 : img] + c * SS : nullptr;
    const double* Ad = add != nullptr ? add + p * SS : nullptr;
    double dsum = 0.0;
    for (int u = (int)blockIdx.x; u < units; u += (int)gridDim.x) {
      const int ur = (S - u) % S;
      __syncthreads();  // the rows of the previous unit have been read
      for (int i = tid; i < S; i += 256) {
        const int r = i / H, j = i % H;
        const int64_t o = (int64_t)(r ? ur : u) * S + 2 * j;
        double2 v = *reinterpret_cast<const double2*>(X + o);
        if (Wi != nullptr) {
          const double2 w = *reinterpret_cast<const double2*>(Wi + o);
          v = make_double2(w.x * v.x, w.y * v.y);
        }
        *reinterpret_cast<double2*>(hrows + r * S + 2 * j) = v;
      }
      __syncthreads();
      for (int i = tid; i < S; i += 256) {
        const int r = i / H, j = i % H;
        if (r == 1 && ur == u) continue;  // a self-reflected row is written once
        const double* A = hrows + r * S;        // this row
        const double* B = hrows + (1 - r) * S;  // its reflection
        const int v0 = 2 * j, v1 = v0 + 1, m0 = (S - v0) % S, m1 = S - v1;
        double2 y = make_double2(0.5 * ((A[v0] + B[v0]) + (A[m0] - B[m0])), 0.5 * ((A[v1] + B[v1]) + (A[m1] - B[m1])));
        const int64_t o = (int64_t)(r ? ur : u) * S + v0;
        if (Wo != nullptr) {
          const double2 w = *reinterpret_cast<const double2*>(Wo + o);
          y = make_double2(w.x * y.x, w.y * y.y);
        }
        if (Ad != nullptr) {
          const double2 a = *reinterpret_cast<const double2*>(Ad + o);
          y = make_double2(fma(add_scale, a.x, y.x), fma(add_scale, a.y, y.y));
          dsum = fma(a.x, y.x, dsum);
          dsum = fma(a.y, y.y, dsum);
        }
        *reinterpret_cast<double2*>(Y + o) = y;
      }
    }
    if (dot_part != nullptr) {  // (uniform) sum(add .* out) over this block's units of plane p
      dsum = block_sum_256(dsum, red);
      if (tid == 0) dot_part[(int64_t)img * dot_stride + c * (int)gridDim.x + (int)blockIdx.x] = dsum;
    }
  }
}

// Launch plan of the butterfly (host arithmetic only): S / 2 + 1 row pairs per plane over as few blocks x as walk them in the
// same number of trips as 85 would (3 x 85 <= 256 partials per image; S = 256: 65 blocks of two pairs), and at most 48 planes -
// the 3 FH_MAX_BATCH of a full batch - in grid y; more planes take further trips.  LDS: the two staged rows.
struct hartley_plan_t {
  int gx, gy;
  int64_t lds_bytes;
};
static hartley_plan_t hartley_plan(int S, int planes) {
  hartley_plan_t pn;
  const int units = S / 2 + 1, trips = (units + 84) / 85;
  pn.gx = (units + trips - 1) / trips;
  pn.gy = planes < 3 * FH_MAX_BATCH ? planes : 3 * FH_MAX_BATCH;
  pn.lds_bytes = (int64_t)2 * S * (int64_t)sizeof(double);
  return pn;
}

static bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

// out = wout .* R(win .* in) (+ add_scale * add) over `planes` planes at the context's side; win / wout: per-image weight tables
// (null: none), `wshared`: entry 0 serves every image.  in != out; every pointer 16-byte aligned (the callers check).
static int hartley_launch(fh_context* ctx, const double* in, double* out, int planes, const fh_batch* win, const fh_batch* wout,
                          int wshared, const double* add, double add_scale, const fh_cg_state* states, hipStream_t st,
                          double* dot_part = nullptr, int dot_stride = 0, int* dot_nparts = nullptr) {
  const int S = ctx->S;
  if (dot_nparts != nullptr) *dot_nparts = 0;
  if (planes < 1 || planes > 65535 || in == out) return FH_EINVAL;
  if (planes > ctx->planes_max) return FH_ESIZE;
  const hartley_plan_t pn = hartley_plan(S, planes);
  fh_diag_tab ti, to;
  memset(&ti, 0, sizeof(ti));
  memset(&to, 0, sizeof(to));
  for (int i = 0; win != nullptr && i < win->nimg && i < FH_MAX_BATCH; ++i) ti.D[i] = win->mask[i];
  for (int i = 0; wout != nullptr && i < wout->nimg && i < FH_MAX_BATCH; ++i) to.D[i] = wout->mask[i];
  if (add == nullptr) dot_part = nullptr;
  if (dot_nparts != nullptr) *dot_nparts = dot_part != nullptr ? 3 * pn.gx : 0;
  hipLaunchKernelGGL(k_hartley_fix, dim3(pn.gx, pn.gy), dim3(256), (size_t)pn.lds_bytes, st, in, out, S, planes, ti, to, wshared,
                     add, add_scale, states, dot_part, dot_stride);
  FH_LAUNCH_CHECK();
  return 0;
}

// Channel mix of the colorization operator (grid z = image, one 16-byte pixel pair per thread, `pairs` = S*S/2 per plane):
//   ADJ = 0:  out[img] = sum_c w[c] * in[img][c]  (+ add_scale * add[img])        in [nimg][3][S][S] -> out [nimg][S][S]
//   ADJ = 1:  out[img][c] = w[c] * in[img]                                          in [nimg][S][S] -> out [nimg][3][S][S]
// w: three device doubles, the same for every image.  The sum runs c = 0, 1, 2 in one fma chain.
template <bool ADJ>
__global__ __launch_bounds__(256) void k_channel_mix(const double* __restrict__ in, double* __restrict__ out,
                                                     const double* __restrict__ w, int64_t pairs,
                                                     const double* __restrict__ add, double add_scale,
                                                     const fh_cg_state* __restrict__ states) {
  const int img = blockIdx.z;
  IMG_GUARD(states, img);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pairs) return;
  const double w0 = w[0], w1 = w[1], w2 = w[2];
  if (ADJ) {
    const double2 v = reinterpret_cast<const double2*>(in + (int64_t)img * 2 * pairs)[i];
    double2* o = reinterpret_cast<double2*>(out + (int64_t)img * 6 * pairs);
    o[i] = make_double2(w0 * v.x, w0 * v.y);
    o[pairs + i] = make_double2(w1 * v.x, w1 * v.y);
    o[2 * pairs + i] = make_double2(w2 * v.x, w2 * v.y);
  } else {
    const double2* x = reinterpret_cast<const double2*>(in + (int64_t)img * 6 * pairs);
    const double2 a = x[i], b = x[pairs + i], c = x[2 * pairs + i];
    double2 v = make_double2(fma(w2, c.x, fma(w1, b.x, w0 * a.x)), fma(w2, c.y, fma(w1, b.y, w0 * a.y)));
    if (add != nullptr) {
      const double2 ad = reinterpret_cast<const double2*>(add + (int64_t)img * 2 * pairs)[i];
      v = make_double2(fma(add_scale, ad.x, v.x), fma(add_scale, ad.y, v.y));
    }
    reinterpret_cast<double2*>(out + (int64_t)img * 2 * pairs)[i] = v;
  }
}

// D_eff[img] = sum_c w[c]^2 D_c[img]: the diagonal of A C A^T in the DCT basis while the covariance has no factor columns
// (the 2-D DCT acts per plane, so dct2 commutes with the channel mix: A C A^T u = idct2(D_eff .* dct2(u)))
__global__ __launch_bounds__(256) void k_channel_deff(fh_batch per, const double* __restrict__ w, double* __restrict__ deff,
                                                      int64_t pairs) {
  const int img = blockIdx.z;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pairs) return;
  const double w0 = w[0], w1 = w[1], w2 = w[2];
  const double2* D = reinterpret_cast<const double2*>(per.D[img]);
  const double2 a = D[i], b = D[pairs + i], c = D[2 * pairs + i];
  reinterpret_cast<double2*>(deff + (int64_t)img * 2 * pairs)[i] =
      make_double2(fma(w2 * w2, c.x, fma(w1 * w1, b.x, w0 * w0 * a.x)), fma(w2 * w2, c.y, fma(w1 * w1, b.y, w0 * w0 * a.y)));
}

constexpr int kDotBlocks = 256;
constexpr int kCgBlocks = 192;
constexpr int kCgScratch = 4 * kDotBlocks + 16;  // doubles of w2 per image: [pAp | b.b | r.r | - | rzbuf[2]]

// partial[b] = sum over block b of a.*b ; optional second product a2.*b2 -> partial[kDotBlocks + b]   (grid z = image)
__global__ __launch_bounds__(256) void k_dot_partial(const double* __restrict__ a, const double* __restrict__ b,
                                                     const double* __restrict__ a2, const double* __restrict__ b2,
                                                     double* __restrict__ part, int64_t n, int part_stride,
                                                     const fh_cg_state* __restrict__ states) {
  const int img = blockIdx.z;
  IMG_GUARD(states, img);
  a += (int64_t)img * n;
  b += (int64_t)img * n;
  part += (int64_t)img * part_stride;
  __shared__ double red[4];
  double s = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    s = fma(a[i], b[i], s);
    if (a2 != nullptr) s2 = fma(a2[i], b2[i], s2);
  }
  s = block_sum_256(s, red);
  if (a2 != nullptr) s2 = block_sum_256(s2, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s;
    if (a2 != nullptr) part[kDotBlocks + blockIdx.x] = s2;
  }
}

// grid x = image: dst[img][slot] = sum of that image's partials
__global__ __launch_bounds__(256) void k_scalar_reduce(const double* __restrict__ part, int64_t part_stride, int nparts,
                                                       PtrTab dst, int slot) {
  __shared__ double red[4];
  part += (int64_t)blockIdx.x * part_stride;
  double s = threadIdx.x < nparts ? part[threadIdx.x] : 0.0;
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) dst.p[blockIdx.x][slot] = s;
}

__global__ __launch_bounds__(256) void k_space_prep(const double* __restrict__ dm, double s2,
                                                    const double* __restrict__ dx, double* __restrict__ de,
                                                    double* __restrict__ part, int64_t part_stride, int64_t n) {
  __shared__ double red[4];
  dm += (int64_t)blockIdx.z * n;  // grid z = image: the vectors of a batch are contiguous [image][n]
  dx += (int64_t)blockIdx.z * n;
  de += (int64_t)blockIdx.z * n;
  part += (int64_t)blockIdx.z * part_stride;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double e = s2 * dm[i];
    de[i] = e;
    s = fma(dx[i], e, s);
  }
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// scal != null: gamma = 1 / scal[0] (dx.de) and q = scal[1] (dx.C dx) are read on the device, and workgroup 0 appends the
// pair to the inner matrices: Mc gets diag(gamma, -1/q) at (mc, mc+1) unless projected, Mh diag(gamma, -1/q) / s2^2 at
// (mh, mh+1); the new rows / columns are cleared first.  No scalar returns to the host.
__global__ __launch_bounds__(256) void k_space_commit(const double* __restrict__ de, const double* __restrict__ cdx,
                                                      double gamma, double q, double s2, PtrTab Dct, PtrTab rct, PtrTab bc0t,
                                                      PtrTab bc1t, PtrTab Dht, PtrTab rht, PtrTab bh0t, PtrTab bh1t,
                                                      int project, int64_t n, int use_scal, PtrTab scalt, PtrTab Mct, int ldc,
                                                      int mc, PtrTab Mht, int ldh, int mh) {
  const int img = blockIdx.z;  // grid z = image; de, cdx contiguous [image][n]
  de += (int64_t)img * n;
  cdx += (int64_t)img * n;
  double* __restrict__ Dc = Dct.p[img];
  const double* __restrict__ rc = rct.p[img];
  double* __restrict__ bc0 = bc0t.p[img];
  double* __restrict__ bc1 = bc1t.p[img];
  double* __restrict__ Dh = Dht.p[img];
  const double* __restrict__ rh = rht.p[img];
  double* __restrict__ bh0 = bh0t.p[img];
  double* __restrict__ bh1 = bh1t.p[img];
  if (use_scal) {
    const double* __restrict__ scal = scalt.p[img];
    double* __restrict__ Mc = Mct.p[img];
    double* __restrict__ Mh = Mht.p[img];
    gamma = 1.0 / scal[0];
    q = scal[1];
    if (blockIdx.x == 0) {
      const int t = threadIdx.x;
      if (!project && Mc != nullptr) {
        for (int i = t; i < mc + 2; i += 256)
          for (int e = 0; e < 2; ++e) Mc[(int64_t)(mc + e) * ldc + i] = 0.0, Mc[(int64_t)i * ldc + mc + e] = 0.0;
      }
      if (Mh != nullptr) {
        for (int i = t; i < mh + 2; i += 256)
          for (int e = 0; e < 2; ++e) Mh[(int64_t)(mh + e) * ldh + i] = 0.0, Mh[(int64_t)i * ldh + mh + e] = 0.0;
      }
      __syncthreads();
      if (t == 0) {
        if (!project && Mc != nullptr) {
          Mc[(int64_t)mc * ldc + mc] = gamma;
          Mc[(int64_t)(mc + 1) * ldc + mc + 1] = -1.0 / q;
        }
        if (Mh != nullptr) {
          Mh[(int64_t)mh * ldh + mh] = gamma / (s2 * s2);
          Mh[(int64_t)(mh + 1) * ldh + mh + 1] = -1.0 / (q * s2 * s2);
        }
      }
    }
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double e = de[i], c = cdx[i];
    double dc = Dc[i];
    if (project) {
      dc = dc + gamma * e * e - c * c / q;
      Dc[i] = dc;
    } else {
      const double s = (rc != nullptr) ? rc[i] : 1.0;
      bc0[i] = e / s;
      bc1[i] = c / s;
    }
    Dh[i] = (dc / s2 - 1.0) / s2;
    const double sh = (rh != nullptr) ? rh[i] : 1.0;
    bh0[i] = e / sh;
    bh1[i] = c / sh;
  }
}

constexpr int kWbMaxCols = 64;  // = kWbMax below: the device-side m x m algebra handles up to 64 columns

// part[b] = sum over block b of a^2 .* w   (de^T D^-1 de of the closed-form BFGS inverse)
__global__ __launch_bounds__(256) void k_wnorm_partial(const double* __restrict__ a, PtrTab wt,
                                                       double* __restrict__ part, int64_t part_stride, int64_t n) {
  __shared__ double red[4];
  const double* __restrict__ w = wt.p[blockIdx.z];  // grid z = image; a contiguous [image][n]
  a += (int64_t)blockIdx.z * n;
  part += (int64_t)blockIdx.z * part_stride;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s = fma(a[i] * a[i], w[i], s);
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_copy_small(const double* __restrict__ src, int64_t src_stride, PtrTab dstt, int n) {
  src += (int64_t)blockIdx.x * src_stride;  // grid x = image
  double* __restrict__ dst = dstt.p[blockIdx.x];
  for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

// Inverse covariance after a BFGS pair, in closed form (no inversion, no Gram):
//   C'^-1 = (I - g dx de^T) C^-1 (I - g de dx^T) + g dx dx^T,   g = 1 / (dx.de)
// In the coordinates of the shared base (columns 0..mc-1 old, mc = de / r, mc+1 = C dx / r; C^-1 = 1/D + Wi Mi Wi^T with
// Wi = (r / D) .* B):  dx = Wi' a,  C^-1 de = Wi' b  with  a = [-M t; 0; 1],  b = [Mi s; 1; 0],  t = W^T dx,  s = Wi^T de, so
//   Mi' = pad(Mi) - g (a b^T + b a^T) + (g^2 rho + g) a a^T,   rho = de^T C^-1 de = de^T D^-1 de + s^T Mi s.
// The generic Woodbury route passes through the singular matrix C - v v^T (v = C dx / sqrt(dx^T C dx)) and loses
// cond(I + G M) ~ 1e9 of the 1e16 at d = 196608 with the DCT prior; this form has no cancellation.
// scal: [0] dx.de, [2] de^T D^-1 de;  cC = M t (mc);  sCi = s, cCi = Mi s (mc).  One workgroup.
__global__ __launch_bounds__(256) void k_bfgs_inverse_commit(PtrTab scalt, PtrTab cCt, const double* __restrict__ coef,
                                                             int64_t coef_stride, PtrTab Mit, int ld, int mc) {
  const double* __restrict__ scal = scalt.p[blockIdx.x];  // grid x = image
  const double* __restrict__ cC = cCt.p[blockIdx.x];
  const double* __restrict__ cCi = coef + (int64_t)blockIdx.x * coef_stride;  // c = Mi s of the dots pass ...
  const double* __restrict__ sCi = cCi + FH_MAX_COLS;                         // ... and s = Wi^T de itself
  double* __restrict__ Mi = Mit.p[blockIdx.x];
  __shared__ double a[kWbMaxCols + 2], b[kWbMaxCols + 2];
  __shared__ double rho_s;
  const int tid = threadIdx.x, n = mc + 2;
  for (int j = tid; j < n; j += 256) {
    a[j] = j < mc ? -cC[j] : (j == mc ? 0.0 : 1.0);
    b[j] = j < mc ? cCi[j] : (j == mc ? 1.0 : 0.0);
  }
  if (tid == 0) {
    double rho = scal[2];
    for (int j = 0; j < mc; ++j) rho = fma(sCi[j], cCi[j], rho);  // fixed order
    rho_s = rho;
  }
  __syncthreads();
  const double g = 1.0 / scal[0], k2 = fma(g * g, rho_s, g);
  for (int i = tid; i < n * n; i += 256) {
    const int r = i / n, c = i % n;
    const double old = (r < mc && c < mc) ? Mi[(int64_t)r * ld + c] : 0.0;
    Mi[(int64_t)r * ld + c] = old - g * (a[r] * b[c] + b[r] * a[c]) + k2 * a[r] * a[c];
  }
}

// ------------------------------------------------------------------------------------------------
// Circular convolution with a sparse tap list.  conv_plan (after the kernels) is the one place that chooses among the seven
// kernels - k_conv1d<0/1>, k_conv_tile8, k_conv_tile, k_conv_dec, k_conv_up, k_conv_direct - and sizes their launches.
//   k_conv_tile   : stride-1 output grid (blur, blur^T, and blur^T of a zero-inserted LR image):
//                   16x32 output tile + halo staged in LDS (<= 56 KiB at halo 30), 2 outputs per
//                   thread, taps read through the scalar path (uniform index).
//   k_conv_direct : decimated forward (SR: out[i][j] sampled at (i*stride, j*stride)).
// Epilogue: out = acc + add_scale * add  when add != null  (the sigma_y^2 u term of A_mm).
// The dynamic LDS of each kernel is laid out by ONE *_lds struct: the kernel carves its regions from it and conv_plan sizes
// the launch from the same constructor (extents and offsets in doubles, `bytes` = the whole allocation).
// ------------------------------------------------------------------------------------------------
constexpr int kMaxTaps = 1024;
constexpr int kT8W = 32, kT8H = 64;  // k_conv_tile8's output tile
constexpr int k1dR = 8;              // k_conv1d: outputs per thread along the filter axis
constexpr int k1dTB = 16;            //           taps per register block
constexpr int k1dAcross = 64;        //           lanes across the filter axis
constexpr int k1dAlong = 32;         //           outputs along the filter axis per workgroup (4 waves x 8)

struct conv_tile_lds {  // [sh][sw] tile | [ntaps] weights | [ntaps] int offsets;  hy = rows (dy extent), hx = columns (dx extent)
  int sw, sh, w_off;
  size_t bytes;
  __host__ __device__ conv_tile_lds(int hy, int hx, int ntaps)
      : sw(32 + 2 * hx), sh(16 + 2 * hy), w_off(sw * sh), bytes((size_t)w_off * sizeof(double) + (size_t)ntaps * 12) {}
};
struct conv_tile8_lds {  // [sh][sw] tile (+1 to an even count) | [ntaps] (weight, offset) pairs
  int sw, sh, tap_off;
  size_t bytes;
  __host__ __device__ conv_tile8_lds(int hy, int hx, int ntaps)
      : sw(kT8W + 2 * hx), sh(kT8H + 2 * hy), tap_off((sw * sh + 1) & ~1), bytes((size_t)tap_off * sizeof(double) + (size_t)ntaps * 16) {}
};
struct conv_dec_lds {  // [s][R][Wp] input tile by column phase | [ntaps] (weight, offset) pairs
  int hq, R, Wp, tap_off;
  size_t bytes;
  __host__ __device__ conv_dec_lds(int s, int hy, int hx, int ntaps)
      : hq((hx + s - 1) / s), R(15 * s + 1 + 2 * hy), Wp(16 + 2 * hq + 1), tap_off((s * R * Wp + 1) & ~1),
        bytes((size_t)tap_off * sizeof(double) + (size_t)ntaps * 16) {}
};
struct conv_up_lds {  // [s*s][cap] (weight, offset) | [Hu][Wu] tile of u | [T][SW] outputs;  cap >= taps of one phase (cap_for)
  int hqy, hqx, Hu, Wu, T, SW, utile_off, utile_len;
  size_t bytes;
  static int cap_for(int s, int hy, int hx) { return ((2 * hy + s) / s + 1) * ((2 * hx + s) / s + 1); }
  __host__ __device__ conv_up_lds(int s, int hy, int hx, int cap)
      : hqy((hy + s - 1) / s), hqx((hx + s - 1) / s), Hu(16 + 2 * hqy), Wu(16 + 2 * hqx + 1), T(16 * s), SW(T + 1),
        utile_off(2 * s * s * cap), utile_len((Hu * Wu + 1) & ~1), bytes(((size_t)utile_off + utile_len + (size_t)T * SW) * sizeof(double)) {}
};
// [span][ld] tile | [nblk * 16 + 8] dense coefficients, zero padded.  (k_conv1d<1> turns its results through the dead tile as
// [64][33] doubles, which fits from h = 1 on: conv_plan sends h = 0 to k_conv1d<0>, which stores straight from registers.)
struct conv1d_lds {
  int span, ld, nblk, e_off;
  size_t bytes;
  __host__ __device__ explicit conv1d_lds(int h)
      : span(k1dAlong + 2 * h), ld(k1dAcross + 1), nblk((2 * h + 1 + k1dTB - 1) / k1dTB), e_off(span * ld),
        bytes(((size_t)e_off + nblk * k1dTB + k1dR) * sizeof(double)) {}
};
// k_conv_window: [sx][ld] tile, transposed (a column of the image is contiguous), ld odd | [kh][wp] window, rows zero padded to
// whole tap blocks.  At hy = hx = 32: 96 x 129 + 65 x 80 doubles = 137.4 KiB (one workgroup per CU; a 31 x 31 window: 54 KiB).
constexpr int kWinW = 32, kWinH = 64;  // k_conv_window's output tile
constexpr int kWinR = 8;               //   outputs per thread along a window row
constexpr int kWinTB = 16;             //   taps per register block
struct conv_window_lds {
  int sx, sy, ld, kh, kw, nblk, wp, w_off;
  size_t bytes;
  __host__ __device__ constexpr conv_window_lds(int hy, int hx)
      : sx(kWinW + 2 * hx), sy(kWinH + 2 * hy), ld(sy | 1), kh(2 * hy + 1), kw(2 * hx + 1), nblk((kw + kWinTB - 1) / kWinTB),
        wp(nblk * kWinTB), w_off((sx * ld + 1) & ~1), bytes(((size_t)w_off + (size_t)kh * wp) * sizeof(double)) {}
};
constexpr size_t kLdsWindow = conv_window_lds(32, 32).bytes;  // the opt-in of set_kernel_attributes: the largest window

__global__ __launch_bounds__(256) void k_conv_tile(const double* __restrict__ in, double* __restrict__ out,
                                                   const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                   const double* __restrict__ tw, int ntaps, int S, int halo,
                                                   int halo_x, int adjoint, int up, const double* __restrict__ add,
                                                   double add_scale, const fh_cg_state* __restrict__ states) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double tile[];
  const conv_tile_lds L(halo, halo_x, ntaps);
  const int sw = L.sw, sh = L.sh;
  double* s_w = tile + L.w_off;
  int* s_off = reinterpret_cast<int*>(s_w + ntaps);
  const int plane = blockIdx.z;
  const int oy0 = blockIdx.y * 16, ox0 = blockIdx.x * 32;
  const int Sin = S / up;
  const double* src = in + (int64_t)plane * Sin * Sin;
  const int sgn = adjoint ? 1 : -1;
  for (int t = threadIdx.x; t < ntaps; t += 256) {  // taps -> LDS: the inner loop then needs no scalar-memory waits
    s_w[t] = tw[t];
    s_off[t] = sgn * (tdy[t] * sw + tdx[t]);
  }
  for (int idx = threadIdx.x; idx < sw * sh; idx += 256) {
    const int ly = idx / sw, lx = idx % sw;
    int gy = (oy0 + ly - halo) % S, gx = (ox0 + lx - halo_x) % S;
    gy += gy < 0 ? S : 0;
    gx += gx < 0 ? S : 0;
    double v;
    if (up == 1) {
      v = src[(int64_t)gy * S + gx];
    } else {
      v = ((gy % up) == 0 && (gx % up) == 0) ? src[(int64_t)(gy / up) * Sin + gx / up] : 0.0;
    }
    tile[idx] = v;
  }
  __syncthreads();
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;  // ly in [0,8): rows ly, ly+8
  double a0 = 0, a1 = 0;
  const double* q0 = tile + (ly + halo) * sw + lx + halo_x;
  const double* q1 = q0 + 8 * sw;
  int t = 0;
  for (; t + 3 < ntaps; t += 4) {
    const int o0 = s_off[t], o1 = s_off[t + 1], o2 = s_off[t + 2], o3 = s_off[t + 3];
    const double w0 = s_w[t], w1 = s_w[t + 1], w2 = s_w[t + 2], w3 = s_w[t + 3];
    a0 = fma(w0, q0[o0], a0);
    a1 = fma(w0, q1[o0], a1);
    a0 = fma(w1, q0[o1], a0);
    a1 = fma(w1, q1[o1], a1);
    a0 = fma(w2, q0[o2], a0);
    a1 = fma(w2, q1[o2], a1);
    a0 = fma(w3, q0[o3], a0);
    a1 = fma(w3, q1[o3], a1);
  }
  for (; t < ntaps; ++t) {
    a0 = fma(s_w[t], q0[s_off[t]], a0);
    a1 = fma(s_w[t], q1[s_off[t]], a1);
  }
  const int ox = ox0 + lx;
  if (ox >= S) return;
  double acc[2] = {a0, a1};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int oy = oy0 + ly + 8 * e;
    if (oy < S) {
      const int64_t o = (int64_t)plane * S * S + (int64_t)oy * S + ox;
      double v = acc[e];
      if (add != nullptr) v = fma(add_scale, add[o], v);
      out[o] = v;
    }
  }
}

// k_conv_tile8: the stride-1 case with 8 outputs per thread - a 64 x 32 output tile, thread = 2 columns (16 apart) x 4 rows
// (16 apart).  k_conv_tile issues 4 LDS instructions per 2 multiply-adds (offset, weight, two inputs) and is bound by
// the LDS instruction rate (10 % of the f64 FMA rate on the 217-tap motion PSF); here a tap costs one 16-byte broadcast
// read (weight + offset packed) and four two-address reads for 8 multiply-adds, and the halo is amortised over 4x the
// outputs (2.9x the tile instead of 6.9x at the motion PSF's 58 x 16 extent).  Same tap order per output: same result.
// MASKED (here and in k_conv1d / k_conv_window): the epilogue multiplies the convolution's result by the 0/1 mask of its
// pixel before the `add` term, out = fma(add_scale, add, mask * t) - the expression of k_mask, so an all-ones mask gives the
// bits of the unmasked kernel.  The mask of plane p is mk.D[p / 3] + (p % 3) S S (fh_batch.mask).  MASKED = false never touches
// `mk`: the unmasked kernels are the code they were before the variant existed.
template <bool MASKED>
__device__ __forceinline__ const double* mask_plane(const fh_diag_tab& mk, int plane, int S) {
  return MASKED ? mk.D[plane / 3] + (int64_t)(plane % 3) * S * S : nullptr;
}

template <bool MASKED>
__device__ __forceinline__ void conv_tile8_body(const double* __restrict__ in, double* __restrict__ out,
                                                const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                const double* __restrict__ tw, int ntaps, int S, int halo, int halo_x,
                                                int adjoint, const double* __restrict__ add, double add_scale,
                                                const fh_cg_state* __restrict__ states, const fh_diag_tab& mk) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double tile[];
  const conv_tile8_lds L(halo, halo_x, ntaps);
  const int sw = L.sw, sh = L.sh;
  double2* s_tap = reinterpret_cast<double2*>(tile + L.tap_off);
  const int plane = blockIdx.z;
  const int oy0 = blockIdx.y * kT8H, ox0 = blockIdx.x * kT8W;
  const double* src = in + (int64_t)plane * S * S;
  const int sgn = adjoint ? 1 : -1;
  for (int t = threadIdx.x; t < ntaps; t += 256)
    s_tap[t] = make_double2(tw[t], __longlong_as_double((long long)(sgn * (tdy[t] * sw + tdx[t]))));
  for (int ly = threadIdx.x >> 6; ly < sh; ly += 4) {  // a wave per tile row: no division by the run-time row pitch
    int gy = (oy0 + ly - halo) % S;
    gy += gy < 0 ? S : 0;
    const double* srow = src + (int64_t)gy * S;
    for (int lx = threadIdx.x & 63; lx < sw; lx += 64) {
      int gx = (ox0 + lx - halo_x) % S;
      gx += gx < 0 ? S : 0;
      tile[ly * sw + lx] = srow[gx];
    }
  }
  __syncthreads();
  // thread = columns tx and tx + 16, rows ty + 16 r: 16 lanes read 16 consecutive doubles (all 32 banks of a half), the next
  // 16 lanes the next tile row - adjacent column PAIRS per lane would leave half of the banks idle in every pass
  const double* mplane = mask_plane<MASKED>(mk, plane, S);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const double* q = tile + (ty + halo) * sw + tx + halo_x;
  const int rstep = 16 * sw;
  double a[4][2];
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r][0] = a[r][1] = 0.0;
#pragma unroll 2
  for (int t = 0; t < ntaps; ++t) {
    const double2 tp = s_tap[t];
    const double* p = q + (int)__double_as_longlong(tp.y);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      a[r][0] = fma(tp.x, p[r * rstep], a[r][0]);
      a[r][1] = fma(tp.x, p[r * rstep + 16], a[r][1]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oy = oy0 + ty + 16 * r;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int ox = ox0 + tx + 16 * e;
      if (oy < S && ox < S) {
        const int64_t o = (int64_t)plane * S * S + (int64_t)oy * S + ox;
        double v = a[r][e];
        if (MASKED) v = mplane[(int64_t)oy * S + ox] * v;
        if (add != nullptr) v = fma(add_scale, add[o], v);
        out[o] = v;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_conv_tile8(const double* __restrict__ in, double* __restrict__ out,
                                                    const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                    const double* __restrict__ tw, int ntaps, int S, int halo,
                                                    int halo_x, int adjoint, const double* __restrict__ add,
                                                    double add_scale, const fh_cg_state* __restrict__ states) {
  conv_tile8_body<false>(in, out, tdy, tdx, tw, ntaps, S, halo, halo_x, adjoint, add, add_scale, states, fh_diag_tab{});
}

__global__ __launch_bounds__(256) void k_conv_tile8_masked(const double* __restrict__ in, double* __restrict__ out,
                                                           const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                           const double* __restrict__ tw, int ntaps, int S, int halo,
                                                           int halo_x, int adjoint, const double* __restrict__ add,
                                                           double add_scale, const fh_cg_state* __restrict__ states,
                                                           fh_diag_tab mk) {
  conv_tile8_body<true>(in, out, tdy, tdx, tw, ntaps, S, halo, halo_x, adjoint, add, add_scale, states, mk);
}

// ------------------------------------------------------------------------------------------------
// k_conv_window: circular convolution with a DENSE window W[2 hy + 1][2 hx + 1] (a measured PSF, a defocus disk: more
// non-zeros than a tap list may hold), stride 1.  A dense window needs no offset table: the tap at (a, b) multiplies the
// input at a fixed distance, so a thread that owns 8 consecutive outputs ALONG a window row reads an input once for up to 8
// multiply-adds and keeps the 16 weights of a block of taps in registers (k_conv1d's scheme, one window row after another):
// per 128 multiply-adds 23 conflict-free 8-byte tile reads and 16 broadcast weight reads, where k_conv_tile8 issues 80.
// Output tile 64 rows x 32 columns: lane = row, wave = 8 columns.  Lanes run ACROSS the window rows' axis, so the tile is
// staged transposed ([x][y], odd pitch: the 16 lanes of a store group hit 32 different banks).
// Both directions are one correlation out(py, px) = sum_{a, b} W[a][b] T[py + a][px + b] with a, b ascending from 0 - one fma
// chain per output in the window's row-major order: the adjoint stages T = in[oy0 - hy + ly][ox0 - hx + lx], the forward
// operator stages the tile, and stores its outputs, mirrored in both axes (T = in[oy0 + 63 + hy - ly][ox0 + 31 + hx - lx]).
// Window rows are zero padded to whole blocks of 16 taps (fma(0, v, acc) = acc); reads past the staged columns are 0.
// ------------------------------------------------------------------------------------------------
// one block of 16 taps of one window row: e = the block's weights, ca = the first column it reads, 23 columns for 8 outputs.
// output r multiplies tap t with the column r + t, so column jj feeds the outputs r = jj - t.  GUARD: columns from `ncol` on
// lie past the staged tile (the zero-padded taps of the row's last block) and read as 0.
template <bool GUARD>
__device__ __forceinline__ void window_block(const double* e, const double* ca, int ld, int ncol, double (&acc)[kWinR]) {
  double wreg[kWinTB];
#pragma unroll
  for (int t = 0; t < kWinTB; ++t) wreg[t] = e[t];
  // all 23 reads are issued before the first multiply-add: with one or two workgroups per CU nothing else hides their latency
  double v[kWinTB + kWinR - 1];
#pragma unroll
  for (int jj = 0; jj < kWinTB + kWinR - 1; ++jj) {
    v[jj] = ca[(GUARD && jj >= ncol ? ncol - 1 : jj) * ld];  // (ncol >= 8: the load stays inside the tile)
    if (GUARD && jj >= ncol) v[jj] = 0.0;
  }
#pragma unroll
  for (int jj = 0; jj < kWinTB + kWinR - 1; ++jj) {
#pragma unroll
    for (int r = 0; r < kWinR; ++r) {
      const int t = jj - r;
      if (t >= 0 && t < kWinTB) acc[r] = fma(wreg[t], v[jj], acc[r]);
    }
  }
}

template <bool MASKED>
__device__ __forceinline__ void conv_window_body(const double* __restrict__ in, double* __restrict__ out,
                                                 const double* __restrict__ win, int S, int hy, int hx, int adjoint,
                                                 const double* __restrict__ add, double add_scale,
                                                 const fh_cg_state* __restrict__ states, const fh_diag_tab& mk) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double lds_win[];
  const conv_window_lds L(hy, hx);
  const int sx = L.sx, sy = L.sy, ld = L.ld, wp = L.wp;
  double* tile = lds_win;
  double* e = lds_win + L.w_off;
  const int tid = threadIdx.x;
  const int plane = blockIdx.z;
  const int oy0 = blockIdx.y * kWinH, ox0 = blockIdx.x * kWinW;
  const double* src = in + (int64_t)plane * S * S;
  for (int t = tid; t < L.kh * wp; t += 256) {
    const int a = t / wp, b = t % wp;
    e[t] = b < L.kw ? win[a * L.kw + b] : 0.0;
  }
  for (int ly = tid >> 6; ly < sy; ly += 4) {  // a wave per tile row: coalesced loads along x, transposed LDS stores
    int gy = (adjoint ? oy0 - hy + ly : oy0 + kWinH - 1 + hy - ly) % S;
    gy += gy < 0 ? S : 0;
    const double* srow = src + (int64_t)gy * S;
    for (int lx = tid & 63; lx < sx; lx += 64) {
      int gx = (adjoint ? ox0 - hx + lx : ox0 + kWinW - 1 + hx - lx) % S;
      gx += gx < 0 ? S : 0;
      tile[lx * ld + ly] = srow[gx];
    }
  }
  __syncthreads();
  const int py = tid & 63, g = __builtin_amdgcn_readfirstlane(tid >> 6);  // lane = tile row, wave = group of 8 columns
  double acc[kWinR];
#pragma unroll
  for (int r = 0; r < kWinR; ++r) acc[r] = 0.0;
  const double* col = tile + (g * kWinR) * ld + py;
  const int ncol = sx - g * kWinR;  // staged columns from this wave's first one on (wave-uniform)
  for (int a = 0; a < L.kh; ++a) {
    const double* ea = e + a * wp;
    const double* ca = col + a;
    // every block but the last of a window row ends inside the staged columns (16 tb + 22 < 16 nblk - 8 <= ncol)
    for (int tb = 0; tb + 1 < L.nblk; ++tb) window_block<false>(ea + tb * kWinTB, ca + tb * kWinTB * ld, ld, 0, acc);
    window_block<true>(ea + (L.nblk - 1) * kWinTB, ca + (L.nblk - 1) * kWinTB * ld, ld, ncol - (L.nblk - 1) * kWinTB, acc);
  }
  const int oy = adjoint ? oy0 + py : oy0 + kWinH - 1 - py;
  if (oy >= S) return;
  const double* mplane = mask_plane<MASKED>(mk, plane, S);
#pragma unroll
  for (int r = 0; r < kWinR; ++r) {
    const int px = g * kWinR + r;
    const int ox = adjoint ? ox0 + px : ox0 + kWinW - 1 - px;
    if (ox < S) {
      const int64_t o = (int64_t)plane * S * S + (int64_t)oy * S + ox;
      double v = acc[r];
      if (MASKED) v = mplane[(int64_t)oy * S + ox] * v;
      if (add != nullptr) v = fma(add_scale, add[o], v);
      out[o] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_conv_window(const double* __restrict__ in, double* __restrict__ out,
                                                     const double* __restrict__ win, int S, int hy, int hx, int adjoint,
                                                     const double* __restrict__ add, double add_scale,
                                                     const fh_cg_state* __restrict__ states) {
  conv_window_body<false>(in, out, win, S, hy, hx, adjoint, add, add_scale, states, fh_diag_tab{});
}

__global__ __launch_bounds__(256) void k_conv_window_masked(const double* __restrict__ in, double* __restrict__ out,
                                                            const double* __restrict__ win, int S, int hy, int hx,
                                                            int adjoint, const double* __restrict__ add, double add_scale,
                                                            const fh_cg_state* __restrict__ states, fh_diag_tab mk) {
  conv_window_body<true>(in, out, win, S, hy, hx, adjoint, add, add_scale, states, mk);
}

__global__ __launch_bounds__(256) void k_conv_direct(const double* __restrict__ in, double* __restrict__ out,
                                                     const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                     const double* __restrict__ tw, int ntaps, int S, int stride,
                                                     int planes, const double* __restrict__ add, double add_scale,
                                                     const fh_cg_state* __restrict__ states) {
  const int So = S / stride;
  const int64_t total = (int64_t)planes * So * So;
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const int plane = (int)(o / ((int64_t)So * So));
  IMG_GUARD(states, plane / 3);
  const int rem = (int)(o % ((int64_t)So * So));
  const int oy = (rem / So) * stride, ox = (rem % So) * stride;
  const double* src = in + (int64_t)plane * S * S;
  double acc = 0.0;
  for (int t = 0; t < ntaps; ++t) {
    int gy = (oy - tdy[t]) % S, gx = (ox - tdx[t]) % S;
    gy += gy < 0 ? S : 0;
    gx += gx < 0 ? S : 0;
    acc = fma(tw[t], src[(int64_t)gy * S + gx], acc);
  }
  if (add != nullptr) acc = fma(add_scale, add[o], acc);
  out[o] = acc;
}

// ------------------------------------------------------------------------------------------------
// Super-resolution operator pair at full rate (stride s = scale factor, 25 x 25 bicubic PSF, not separable):
//   k_conv_dec : out[i][j] = sum_t w_t in[s i - dy_t][s j - dx_t]          (blur, then keep every s-th sample)
//   k_conv_up  : out[y][x] = sum_t w_t z[y + dy_t][x + dx_t],  z = u with s - 1 zeros inserted   (its adjoint)
// k_conv_direct fetched every operand of its 625 taps per output through the vector memory path (131 us per call over 24
// planes), and k_conv_tile with `up` multiplied the inserted zeros (15 of 16 taps at s = 4; 107 us).  Here the input tile
// of k_conv_dec sits in LDS de-interleaved by column phase (x = s X + px), so that 16 neighbouring outputs read 16
// consecutive doubles for every tap; k_conv_up sorts the taps by output phase (py, px) = (-dy mod s, -dx mod s) once per
// workgroup - one wave, ballots + prefix counts, list order preserved - and every output then visits only the ~ 1/s^2 of
// the taps that meet a sample of u.  Both keep the tap order of the kernels they replace (skipping exact zeros): the
// results are bitwise the same.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_conv_dec(const double* __restrict__ in, double* __restrict__ out,
                                                  const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                  const double* __restrict__ tw, int ntaps, int S, int s, int hy, int hx,
                                                  const double* __restrict__ add, double add_scale,
                                                  const fh_cg_state* __restrict__ states) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double tile[];
  const int So = S / s;
  const conv_dec_lds L(s, hy, hx, ntaps);
  const int hq = L.hq, hx4 = hq * s;
  const int R = L.R, Wp = L.Wp;
  double2* s_tap = reinterpret_cast<double2*>(tile + L.tap_off);
  const int plane = blockIdx.z, oy0 = blockIdx.y * 16, ox0 = blockIdx.x * 16;
  const double* src = in + (int64_t)plane * S * S;
  for (int t = threadIdx.x; t < ntaps; t += 256) {
    const int c = hx4 - tdx[t];  // column of the tap's operand for output column 0, >= 0
    s_tap[t] = make_double2(tw[t], __longlong_as_double((long long)(((c % s) * R + hy - tdy[t]) * Wp + c / s)));
  }
  const int gy0 = oy0 * s - hy, gx0 = ox0 * s - hx4, ncol = s * (16 + 2 * hq);
  for (int r = threadIdx.x >> 6; r < R; r += 4) {
    int gy = (gy0 + r) % S;
    gy += gy < 0 ? S : 0;
    const double* srow = src + (int64_t)gy * S;
    for (int c = threadIdx.x & 63; c < ncol; c += 64) {
      int gx = (gx0 + c) % S;
      gx += gx < 0 ? S : 0;
      tile[((c % s) * R + r) * Wp + c / s] = srow[gx];
    }
  }
  __syncthreads();
  const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
  const double* q = tile + (s * ti) * Wp + tj;
  double acc = 0.0;
#pragma unroll 4
  for (int t = 0; t < ntaps; ++t) {
    const double2 tp = s_tap[t];
    acc = fma(tp.x, q[(int)__double_as_longlong(tp.y)], acc);
  }
  const int oy = oy0 + ti, ox = ox0 + tj;
  if (oy < So && ox < So) {
    const int64_t o = (int64_t)plane * So * So + (int64_t)oy * So + ox;
    if (add != nullptr) acc = fma(add_scale, add[o], acc);
    out[o] = acc;
  }
}

constexpr int kUpMaxPhases = 16;  // s <= 4

__global__ __launch_bounds__(256) void k_conv_up(const double* __restrict__ in, double* __restrict__ out,
                                                 const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                 const double* __restrict__ tw, int ntaps, int S, int s, int hy, int hx,
                                                 int cap, const double* __restrict__ add, double add_scale,
                                                 const fh_cg_state* __restrict__ states) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double lds_up[];
  const int Sin = S / s;
  const conv_up_lds L(s, hy, hx, cap);
  const int hqy = L.hqy, hqx = L.hqx;
  const int Hu = L.Hu, Wu = L.Wu, T = L.T, SW = L.SW;
  double2* lists = reinterpret_cast<double2*>(lds_up);
  double* utile = lds_up + L.utile_off;
  double* stage = utile + L.utile_len;
  __shared__ int cnt_s[kUpMaxPhases];
  const int plane = blockIdx.z, tid = threadIdx.x;
  const double* src = in + (int64_t)plane * Sin * Sin;
  const int a0 = blockIdx.y * 16 - hqy, b0 = blockIdx.x * 16 - hqx;
  for (int idx = tid; idx < Hu * (Wu - 1); idx += 256) {
    const int r = idx / (Wu - 1), c = idx % (Wu - 1);
    int ga = (a0 + r) % Sin, gb = (b0 + c) % Sin;
    ga += ga < 0 ? Sin : 0;
    gb += gb < 0 ? Sin : 0;
    utile[r * Wu + c] = src[(int64_t)ga * Sin + gb];
  }
  if (tid < 64) {  // one wave sorts the taps by phase, keeping the list order inside every phase
    const int lane = tid;
    int cnt[kUpMaxPhases];
#pragma unroll
    for (int p = 0; p < kUpMaxPhases; ++p) cnt[p] = 0;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int t0 = 0; t0 < ntaps; t0 += 64) {
      const int t = t0 + lane;
      const bool valid = t < ntaps;
      const int dy = valid ? tdy[t] : 0, dx = valid ? tdx[t] : 0;
      const int py = ((-dy) % s + s) % s, px = ((-dx) % s + s) % s;
      const int ph = valid ? py * s + px : -1;
      const double2 item = make_double2(valid ? tw[t] : 0.0,
                                        __longlong_as_double((long long)(((py + dy) / s) * Wu + (px + dx) / s)));
#pragma unroll
      for (int p = 0; p < kUpMaxPhases; ++p) {
        const unsigned long long mask = __ballot(ph == p);
        if (ph == p) {
          const int pos = cnt[p] + __popcll(mask & lt);
          if (pos < cap) lists[p * cap + pos] = item;
        }
        cnt[p] += __popcll(mask);
      }
    }
    if (lane < kUpMaxPhases) {
      int c = 0;
#pragma unroll
      for (int p = 0; p < kUpMaxPhases; ++p) c = lane == p ? cnt[p] : c;
      cnt_s[lane] = c < cap ? c : cap;
    }
  }
  __syncthreads();
  const int la = tid >> 4, lb = tid & 15;
  const double* q = utile + (la + hqy) * Wu + lb + hqx;
  for (int p = 0; p < s * s; ++p) {
    const int n = cnt_s[p];
    const double2* lp = lists + p * cap;
    double acc = 0.0;
    for (int t = 0; t < n; ++t) {
      const double2 tp = lp[t];
      acc = fma(tp.x, q[(int)__double_as_longlong(tp.y)], acc);
    }
    stage[(s * la + p / s) * SW + s * lb + p % s] = acc;
  }
  __syncthreads();
  const int oy0 = blockIdx.y * T, ox0 = blockIdx.x * T;
  for (int idx = tid; idx < T * T; idx += 256) {
    const int r = idx / T, c = idx % T;
    const int oy = oy0 + r, ox = ox0 + c;
    if (oy < S && ox < S) {
      const int64_t o = (int64_t)plane * S * S + (int64_t)oy * S + ox;
      double v = stage[r * SW + c];
      if (add != nullptr) v = fma(add_scale, add[o], v);
      out[o] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Multi-frame super-resolution (fh_problem.op = 12, fh_conv_frames): K frames of one scene, A = [A_0; ..; A_{K-1}] with
// A_k = Dec_s B_k, the tap lists of all frames concatenated and foff[K + 1] their offsets.  The measurement is frame-major,
// [nimg][K][3][So][So]: plane (image i, channel c) of frame k is plane (i K + k) 3 + c of the low-resolution side.
//   k_conv_dec_frames : k_conv_dec with the input tile staged ONCE, for the union of the frames' extents; the frames then take
//                       turns in the tap staging (cap_taps pairs) and each thread runs one fma chain from 0 per frame, in list
//                       order - the bits of K k_conv_dec / k_conv_direct launches.
//   k_conv_up_frames  : k_conv_up per frame (low-resolution tile + phase-sorted lists re-staged, per-phase sums from 0) with the
//                       frames' sums added in frame order into the thread's own slots of the output staging, one rounding
//                       each - the bits of K k_conv_up launches chained through add (add_scale = 1).  One coalesced store.
// Both read their frame's taps inside [0, ntaps) and at most cap_taps / cap of them whatever foff holds (the host has checked
// foff before the launch, frames_prepare); the tile indices trust hy / hx like the single-frame kernels.  No atomics.
// WEIGHTED (op 13, k_conv_dec_frames_w): the epilogue multiplies the frame's sum by the weight of its output, wt.D[image] at the
// output's offset inside the image ([K][3][So][So], the measurement's own layout), rounds, and then adds: k_mask's expression,
// fma(add_scale, add, w * t).  A compile-time flag, as MASKED in the convolution kernels: k_conv_dec_frames instantiates
// `false` and never touches wt.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void frame_range(const int* __restrict__ foff, int k, int ntaps, int* t0, int* n) {
  int a = foff[k], b = foff[k + 1];
  a = a < 0 ? 0 : (a > ntaps ? ntaps : a);
  b = b < a ? a : (b > ntaps ? ntaps : b);
  *t0 = a, *n = b - a;
}

template <bool WEIGHTED>
__device__ __forceinline__ void conv_dec_frames_body(const double* __restrict__ in, double* __restrict__ out,
                                                     const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                     const double* __restrict__ tw, const int* __restrict__ foff,
                                                     int K, int ntaps, int cap_taps, int S, int s, int hy, int hx,
                                                     const double* __restrict__ add, double add_scale,
                                                     const fh_cg_state* __restrict__ states, const fh_diag_tab& wt) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double tile[];
  const int So = S / s;
  const conv_dec_lds L(s, hy, hx, cap_taps);
  const int hq = L.hq, hx4 = hq * s;
  const int R = L.R, Wp = L.Wp;
  double2* s_tap = reinterpret_cast<double2*>(tile + L.tap_off);
  const int plane = blockIdx.z, oy0 = blockIdx.y * 16, ox0 = blockIdx.x * 16;
  const double* src = in + (int64_t)plane * S * S;
  const int gy0 = oy0 * s - hy, gx0 = ox0 * s - hx4, ncol = s * (16 + 2 * hq);
  for (int r = threadIdx.x >> 6; r < R; r += 4) {
    int gy = (gy0 + r) % S;
    gy += gy < 0 ? S : 0;
    const double* srow = src + (int64_t)gy * S;
    for (int c = threadIdx.x & 63; c < ncol; c += 64) {
      int gx = (gx0 + c) % S;
      gx += gx < 0 ? S : 0;
      tile[((c % s) * R + r) * Wp + c / s] = srow[gx];
    }
  }
  const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
  const double* q = tile + (s * ti) * Wp + tj;
  const int oy = oy0 + ti, ox = ox0 + tj;
  const int img = plane / 3, ch = plane % 3;
  for (int k = 0; k < K; ++k) {
    int t0, n;
    frame_range(foff, k, ntaps, &t0, &n);
    n = n < cap_taps ? n : cap_taps;
    if (k > 0) __syncthreads();  // the previous frame's pairs have been read
    for (int t = threadIdx.x; t < n; t += 256) {
      const int c = hx4 - tdx[t0 + t];  // column of the tap's operand for output column 0, >= 0
      s_tap[t] = make_double2(tw[t0 + t], __longlong_as_double((long long)(((c % s) * R + hy - tdy[t0 + t]) * Wp + c / s)));
    }
    __syncthreads();  // (k = 0: the tile as well)
    double acc = 0.0;
#pragma unroll 4
    for (int t = 0; t < n; ++t) {
      const double2 tp = s_tap[t];
      acc = fma(tp.x, q[(int)__double_as_longlong(tp.y)], acc);
    }
    if (oy < So && ox < So) {
      const int64_t o = ((int64_t)(img * K + k) * 3 + ch) * So * So + (int64_t)oy * So + ox;
      if (WEIGHTED) acc = wt.D[img][(int64_t)(k * 3 + ch) * So * So + (int64_t)oy * So + ox] * acc;
      if (add != nullptr) acc = fma(add_scale, add[o], acc);
      out[o] = acc;
    }
  }
}

__global__ __launch_bounds__(256) void k_conv_dec_frames(const double* __restrict__ in, double* __restrict__ out,
                                                         const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                         const double* __restrict__ tw, const int* __restrict__ foff,
                                                         int K, int ntaps, int cap_taps, int S, int s, int hy, int hx,
                                                         const double* __restrict__ add, double add_scale,
                                                         const fh_cg_state* __restrict__ states) {
  conv_dec_frames_body<false>(in, out, tdy, tdx, tw, foff, K, ntaps, cap_taps, S, s, hy, hx, add, add_scale, states,
                              fh_diag_tab{});
}

__global__ __launch_bounds__(256) void k_conv_dec_frames_w(const double* __restrict__ in, double* __restrict__ out,
                                                           const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                           const double* __restrict__ tw, const int* __restrict__ foff,
                                                           int K, int ntaps, int cap_taps, int S, int s, int hy, int hx,
                                                           const double* __restrict__ add, double add_scale,
                                                           const fh_cg_state* __restrict__ states, fh_diag_tab wt) {
  conv_dec_frames_body<true>(in, out, tdy, tdx, tw, foff, K, ntaps, cap_taps, S, s, hy, hx, add, add_scale, states, wt);
}

__global__ __launch_bounds__(256) void k_conv_up_frames(const double* __restrict__ in, double* __restrict__ out,
                                                        const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                        const double* __restrict__ tw, const int* __restrict__ foff,
                                                        int K, int ntaps, int S, int s, int hy, int hx, int cap,
                                                        const fh_cg_state* __restrict__ states) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double lds_up[];
  const int Sin = S / s;
  const conv_up_lds L(s, hy, hx, cap);
  const int hqy = L.hqy, hqx = L.hqx;
  const int Hu = L.Hu, Wu = L.Wu, T = L.T, SW = L.SW;
  double2* lists = reinterpret_cast<double2*>(lds_up);
  double* utile = lds_up + L.utile_off;
  double* stage = utile + L.utile_len;
  __shared__ int cnt_s[kUpMaxPhases];
  const int plane = blockIdx.z, tid = threadIdx.x;
  const int img = plane / 3, ch = plane % 3;
  const int a0 = blockIdx.y * 16 - hqy, b0 = blockIdx.x * 16 - hqx;
  const int la = tid >> 4, lb = tid & 15;
  const double* q = utile + (la + hqy) * Wu + lb + hqx;
  for (int k = 0; k < K; ++k) {
    int t0, n_k;
    frame_range(foff, k, ntaps, &t0, &n_k);
    if (k > 0) __syncthreads();  // the previous frame's tile and lists have been read
    const double* src = in + ((int64_t)(img * K + k) * 3 + ch) * Sin * Sin;
    for (int idx = tid; idx < Hu * (Wu - 1); idx += 256) {
      const int r = idx / (Wu - 1), c = idx % (Wu - 1);
      int ga = (a0 + r) % Sin, gb = (b0 + c) % Sin;
      ga += ga < 0 ? Sin : 0;
      gb += gb < 0 ? Sin : 0;
      utile[r * Wu + c] = src[(int64_t)ga * Sin + gb];
    }
    if (tid < 64) {  // one wave sorts the frame's taps by phase, keeping the list order inside every phase (as k_conv_up)
      const int lane = tid;
      int cnt[kUpMaxPhases];
#pragma unroll
      for (int p = 0; p < kUpMaxPhases; ++p) cnt[p] = 0;
      const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
      for (int b = 0; b < n_k; b += 64) {
        const int t = b + lane;
        const bool valid = t < n_k;
        const int dy = valid ? tdy[t0 + t] : 0, dx = valid ? tdx[t0 + t] : 0;
        const int py = ((-dy) % s + s) % s, px = ((-dx) % s + s) % s;
        const int ph = valid ? py * s + px : -1;
        const double2 item = make_double2(valid ? tw[t0 + t] : 0.0,
                                          __longlong_as_double((long long)(((py + dy) / s) * Wu + (px + dx) / s)));
#pragma unroll
        for (int p = 0; p < kUpMaxPhases; ++p) {
          const unsigned long long mask = __ballot(ph == p);
          if (ph == p) {
            const int pos = cnt[p] + __popcll(mask & lt);
            if (pos < cap) lists[p * cap + pos] = item;
          }
          cnt[p] += __popcll(mask);
        }
      }
      if (lane < kUpMaxPhases) {
        int c = 0;
#pragma unroll
        for (int p = 0; p < kUpMaxPhases; ++p) c = lane == p ? cnt[p] : c;
        cnt_s[lane] = c < cap ? c : cap;
      }
    }
    __syncthreads();
    for (int p = 0; p < s * s; ++p) {
      const int n = cnt_s[p];
      const double2* lp = lists + p * cap;
      double acc = 0.0;
      for (int t = 0; t < n; ++t) {
        const double2 tp = lp[t];
        acc = fma(tp.x, q[(int)__double_as_longlong(tp.y)], acc);
      }
      double* slot = stage + (s * la + p / s) * SW + s * lb + p % s;  // this thread's own: no other thread touches it before the store
      *slot = k == 0 ? acc : fma(1.0, *slot, acc);
    }
  }
  __syncthreads();
  const int oy0 = blockIdx.y * T, ox0 = blockIdx.x * T;
  for (int idx = tid; idx < T * T; idx += 256) {
    const int r = idx / T, c = idx % T;
    const int oy = oy0 + r, ox = ox0 + c;
    if (oy < S && ox < S) out[(int64_t)plane * S * S + (int64_t)oy * S + ox] = stage[r * SW + c];
  }
}

// ------------------------------------------------------------------------------------------------
// Spatially varying blur (fh_problem.op = 14, fh_conv_blend): the Nagy-O'Leary interpolation of K shift-invariant blurs,
//   A = sum_k diag(U_k) B_k,   A^T = sum_k B_k^T diag(U_k),
// B_k the stride-1 circular blur of tap list k (lists concatenated, foff[K + 1] their offsets, as for op 12) and U_k a
// per-pixel blend map, blend[K][3][S][S], shared by every image (the map of frame k for plane p at (3 k + p % 3) S S).
// One kernel, k_conv_blend<NR, ADJ>, on a 32 x 8 NR output tile, a thread = NR outputs 8 rows apart (k_conv_tile's layout at
// NR = 2, k_conv_tile8's footprint at NR = 8); the frames take turns in the tap staging (cap_taps pairs), as in
// conv_dec_frames_body:
//   ADJ = 0 : the input tile is staged ONCE for the union of the extents; per frame t_k = one fma chain from 0 in list order,
//             then the epilogue blends in frame order, tot = fma(add_scale, add, U_0 t_0) (U_0 t_0 without add), then
//             tot = fma(1, tot, U_k t_k), every product U_k t_k rounded - the bits of K conv_launch + k_mask passes.
//   ADJ = 1 : the tile is re-staged per frame as the rounded product U_k .* in (the input itself comes through L2, so the
//             LDS holds one tile, not two); per frame one fma chain from 0, the frames added in index order, one rounding
//             each - the bits of K k_mask + conv_launch passes chained through add (add_scale = 1).
// Edge guards as k_conv_tile: any even S tiles.  A frame's taps are read inside [0, ntaps) and at most cap_taps of them
// whatever foff holds (the host has checked foff, frames_prepare); the tile indices trust hy / hx.  No atomics.
// ------------------------------------------------------------------------------------------------
struct conv_blend_lds {  // [sh][sw] tile (+1 to an even count) | [cap_taps] (weight, offset) pairs
  int sw, sh, tap_off;
  size_t bytes;
  __host__ __device__ conv_blend_lds(int nr, int hy, int hx, int cap_taps)
      : sw(32 + 2 * hx), sh(8 * nr + 2 * hy), tap_off((sw * sh + 1) & ~1),
        bytes((size_t)tap_off * sizeof(double) + (size_t)cap_taps * 16) {}
};

// a product that stays a product: rounded before whatever adds to it (no contraction into the blend's fma)
__device__ __forceinline__ double mul_rounded(double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return p;
}

template <int NR, bool ADJ>
__global__ __launch_bounds__(256) void k_conv_blend(const double* __restrict__ in, double* __restrict__ out,
                                                    const int* __restrict__ tdy, const int* __restrict__ tdx,
                                                    const double* __restrict__ tw, const int* __restrict__ foff, int K,
                                                    int ntaps, int cap_taps, int S, int hy, int hx,
                                                    const double* __restrict__ blend, const double* __restrict__ add,
                                                    double add_scale, const fh_cg_state* __restrict__ states) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double tile[];
  const conv_blend_lds L(NR, hy, hx, cap_taps);
  const int sw = L.sw, sh = L.sh;
  double2* s_tap = reinterpret_cast<double2*>(tile + L.tap_off);
  const int plane = blockIdx.z, ch = plane % 3;
  const int oy0 = blockIdx.y * (8 * NR), ox0 = blockIdx.x * 32;
  const int64_t SS = (int64_t)S * S;
  const double* src = in + (int64_t)plane * SS;
  const int sgn = ADJ ? 1 : -1;
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;  // rows ly + 8 r
  const double* q = tile + (ly + hy) * sw + lx + hx;
  const int ox = ox0 + lx;
  double tot[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) tot[r] = 0.0;
  for (int k = 0; k < K; ++k) {
    int t0, n;
    frame_range(foff, k, ntaps, &t0, &n);
    n = n < cap_taps ? n : cap_taps;
    const double* uk = blend + (int64_t)(3 * k + ch) * SS;
    if (k > 0) __syncthreads();  // the previous frame's pairs (and, ADJ, its tile) have been read
    for (int t = threadIdx.x; t < n; t += 256)
      s_tap[t] = make_double2(tw[t0 + t], __longlong_as_double((long long)(sgn * (tdy[t0 + t] * sw + tdx[t0 + t]))));
    if (ADJ || k == 0) {
      for (int ty = threadIdx.x >> 6; ty < sh; ty += 4) {  // a wave per tile row: no division by the run-time row pitch
        int gy = (oy0 + ty - hy) % S;
        gy += gy < 0 ? S : 0;
        const double* srow = src + (int64_t)gy * S;
        const double* urow = uk + (int64_t)gy * S;
        for (int tx = threadIdx.x & 63; tx < sw; tx += 64) {
          int gx = (ox0 + tx - hx) % S;
          gx += gx < 0 ? S : 0;
          tile[ty * sw + tx] = ADJ ? mul_rounded(urow[gx], srow[gx]) : srow[gx];
        }
      }
    }
    __syncthreads();
    double acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;
#pragma unroll 2
    for (int t = 0; t < n; ++t) {
      const double2 tp = s_tap[t];
      const double* p = q + (int)__double_as_longlong(tp.y);
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[r] = fma(tp.x, p[r * 8 * sw], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int oy = oy0 + ly + 8 * r;
      if (ADJ) {
        tot[r] = k == 0 ? acc[r] : fma(1.0, tot[r], acc[r]);
      } else if (oy < S && ox < S) {
        const double t = mul_rounded(uk[(int64_t)oy * S + ox], acc[r]);
        if (k > 0) tot[r] = fma(1.0, tot[r], t);
        else tot[r] = add != nullptr ? fma(add_scale, add[(int64_t)plane * SS + (int64_t)oy * S + ox], t) : t;
      }
    }
  }
  if (ox >= S) return;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int oy = oy0 + ly + 8 * r;
    if (oy < S) out[(int64_t)plane * SS + (int64_t)oy * S + ox] = tot[r];
  }
}

// ------------------------------------------------------------------------------------------------
// The m x m part of a Woodbury step / forward time shift on the device (online_update_bfgs.py:87-119 in the real form of
// this build):   Mdst = sym( sign * Msrc (I + alpha G Msrc)^-1 ),   (alpha, sign) = (1, -1): Woodbury inverse; (s, +1): shift.
// One workgroup, matrices in LDS.  A = I + alpha G Msrc is NOT well conditioned: the factor columns of a trajectory are
// nearly dependent (balanced Gram matrices with eigenvalues 1e-10 .. 7 at k = 8) and G Msrc is far from normal - measured
// cond(A) ~ 1e12 at 256 x 256, i.e. a plain float64 elimination leaves 1e-4 in Mdst and 1e-6 .. 1e-4 in the covariance at
// sigma < 0.2.  So: A^-1 by Gauss-Jordan with partial pivoting in float64, X0 = sign Msrc A^-1, then up to kWbRefine steps of
// iterative refinement  X <- X + (sign Msrc - X A) A^-1  with A = I + alpha G Msrc and the residual accumulated in
// double-double (error-free products by fma, two-sum accumulation): converges to the float64 rounding of the exact
// m x m result (contraction ~ cond(A) x 1e-16 per step), 3e-6 -> 6e-9 in the covariance on the measured states.
// No host round trip: the covariance updates of a guidance call stay on the device.
// ------------------------------------------------------------------------------------------------
constexpr int kWbMax = 64;
constexpr int kWbRefine = 12;
constexpr int kWbLdsMax = 48;  // (m (2m+1) + 2 m (m+1) + 3 m^2) doubles = 129 KB at m = 48

struct dd_acc {
  double hi, lo;
};
// s += a * b, exactly up to the final rounding of hi + lo (Ogita-Rump-Oishi Dot2 step)
__device__ __forceinline__ void dd_fma(dd_acc& s, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  const double ep = __builtin_fma(a, b, -p);
  const double t = s.hi + p;
  const double z = t - s.hi;
  const double es = (s.hi - (t - z)) + (p - z);
  s.hi = t;
  s.lo += es + ep;
}

// scratch: 4 m^2 doubles of global memory (A as hi / lo pairs, the residual, the last correction), private to this launch
__global__ __launch_bounds__(256) void k_woodbury_inner(PtrTab Msrct, int lds_, PtrTab Gt, int ldg, PtrTab Mdstt, int ldd, int m,
                                                        double alpha, double sign, double* __restrict__ scratch,
                                                        int64_t scratch_stride) {
  const double* __restrict__ Msrc = Msrct.p[blockIdx.x];  // grid x = image (one workgroup each)
  const double* __restrict__ G = Gt.p[blockIdx.x];
  double* __restrict__ Mdst = Mdstt.p[blockIdx.x];
  scratch += (int64_t)blockIdx.x * scratch_stride;
  extern __shared__ __align__(16) double wb[];
  const int w = 2 * m + 1;          // row pitch of the augmented matrix (odd: conflict-free column walks)
  const int q = m + 1;
  double* aug = wb;                 // [m][w]   left: A^T, later X;  right: I, later A^-T
  double* Ms = wb + m * w;          // [m][m+1] Msrc
  double* Gs = Ms + m * q;          // [m][m+1] alpha G
  // A (hi / lo) and the residual live in LDS while they fit beside the elimination (m <= kWbLdsMax), else in the scratch
  double* extra = Gs + m * q;
  double* Ahi = m <= kWbLdsMax ? extra : scratch;  // [m][m]
  double* Alo = m <= kWbLdsMax ? extra + m * m : scratch + m * m;
  double* Rs = m <= kWbLdsMax ? extra + 2 * m * m : scratch + 2 * m * m;
  double* Dl = scratch + 3 * m * m;  // the last applied correction
  __shared__ int piv;
  __shared__ double pval;
  __shared__ double rnorm[4];
  const int tid = threadIdx.x;
  for (int i = tid; i < m * m; i += 256) {
    const int r = i / m, c = i % m;
    Ms[r * q + c] = Msrc[(int64_t)r * lds_ + c];
    Gs[r * q + c] = alpha * G[(int64_t)r * ldg + c];
  }
  __syncthreads();
  // A = I + G Msrc in double-double;  aug[r][c] = A^T[r][c] = A[c][r] (rounded);  aug[r][m + c] = I
  for (int i = tid; i < m * m; i += 256) {
    const int r = i / m, c = i % m;  // element A[r][c]
    dd_acc a{r == c ? 1.0 : 0.0, 0.0};
    for (int k = 0; k < m; ++k) dd_fma(a, Gs[r * q + k], Ms[k * q + c]);
    const double hi = a.hi + a.lo;
    Ahi[r * m + c] = hi;
    Alo[r * m + c] = (a.hi - hi) + a.lo;
    aug[c * w + r] = hi;
    aug[r * w + m + c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int k = 0; k < m; ++k) {
    // pivot search in column k, rows k..m-1 (one wave, deterministic: the first maximum wins)
    if (tid < 64) {
      double best = -1.0;
      int bi = k;
      for (int r = k + tid; r < m; r += 64) {
        const double v = fabs(aug[r * w + k]);
        if (v > best) best = v, bi = r;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(best, o, 64);
        const int oi = __shfl_down(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
      }
      if (tid == 0) piv = bi;
    }
    __syncthreads();
    const int p = piv;
    if (p != k)
      for (int c = tid; c < 2 * m; c += 256) {
        const double t = aug[k * w + c];
        aug[k * w + c] = aug[p * w + c];
        aug[p * w + c] = t;
      }
    __syncthreads();
    if (tid == 0) pval = aug[k * w + k];
    __syncthreads();
    const double inv = 1.0 / pval;
    for (int c = tid; c < 2 * m; c += 256) aug[k * w + c] *= inv;
    __syncthreads();
    // eliminate column k from every other row: thread -> (row, column slice)
    for (int i = tid; i < m * 2 * m; i += 256) {
      const int r = i / (2 * m), c = i % (2 * m);
      if (r == k || c == k) continue;  // column k itself is cleared after the sweep (its old value is the multiplier)
      aug[r * w + c] = fma(-aug[r * w + k], aug[k * w + c], aug[r * w + c]);
    }
    __syncthreads();
    for (int r = tid; r < m; r += 256)
      if (r != k) aug[r * w + k] = 0.0;
    __syncthreads();
  }
  // right half = A^-T, i.e. Ainv[k][c] = aug[c][m + k].  X0 = sign Msrc Ainv into the left half
  for (int i = tid; i < m * m; i += 256) {
    const int r = i / m, c = i % m;
    double x = 0.0;
    for (int k = 0; k < m; ++k) x = fma(Ms[r * q + k], aug[c * w + m + k], x);
    aug[r * w + c] = sign * x;
  }
  __syncthreads();
  // refinement until the residual stops shrinking (contraction ~ cond(A) x 1e-16 per step: 2 steps at cond 1e12, more
  // towards 1e15), at most kWbRefine steps; a step after which the residual grew is taken back
  double prev = 1.0e300;
  for (int it = 0; it < kWbRefine; ++it) {
    // R = sign Msrc - X A  (double-double accumulation, A as hi + lo)
    double rmax = 0.0;
    for (int i = tid; i < m * m; i += 256) {
      const int r = i / m, c = i % m;
      dd_acc a{sign * Ms[r * q + c], 0.0};
      double lo = 0.0;
      for (int k = 0; k < m; ++k) {
        const double x = -aug[r * w + k];
        dd_fma(a, x, Ahi[k * m + c]);
        lo = fma(x, Alo[k * m + c], lo);
      }
      const double rv = a.hi + (a.lo + lo);
      Rs[r * m + c] = rv;
      rmax = fmax(rmax, fabs(rv));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rmax = fmax(rmax, __shfl_down(rmax, o, 64));
    if ((tid & 63) == 0) rnorm[tid >> 6] = rmax;
    __syncthreads();
    const double cur = fmax(fmax(rnorm[0], rnorm[1]), fmax(rnorm[2], rnorm[3]));
    __syncthreads();
    if (!(cur < prev)) {  // uniform: every thread read the same four values.  The last step did not help: take it back
      for (int i = tid; i < m * m; i += 256) aug[(i / m) * w + i % m] -= Dl[i];
      __syncthreads();
      break;
    }
    // X += R Ainv
    for (int i = tid; i < m * m; i += 256) {
      const int r = i / m, c = i % m;
      double dlt = 0.0;
      for (int k = 0; k < m; ++k) dlt = fma(Rs[r * m + k], aug[c * w + m + k], dlt);
      Dl[i] = dlt;
      aug[r * w + c] += dlt;
    }
    __syncthreads();
    if (cur == 0.0) break;
    prev = cur;
  }
  // Mdst = 0.5 (X + X^T)
  for (int i = tid; i < m * m; i += 256) {
    const int r = i / m, c = i % m;
    Mdst[(int64_t)r * ldd + c] = 0.5 * (aug[r * w + c] + aug[c * w + r]);
  }
}

// ------------------------------------------------------------------------------------------------
// 1-D pass of a separable PSF (column kernel: AXIS 0, row kernel: AXIS 1), stride 1, circular.
// k_conv_tile spends two LDS reads per FMA; here a thread owns 8 consecutive outputs ALONG the filter axis, so one LDS
// read of an input feeds up to 8 FMAs and the weights of a 16-tap block sit in registers: 0.3 LDS reads per FMA.
// Lanes always run ACROSS the filter axis (conflict-free LDS reads of consecutive doubles); for the row kernel the tile
// is therefore staged transposed ([x][y], row pad 1) and the result goes back through LDS for coalesced stores.
// The tap list (ascending offsets, possibly with gaps) is expanded to a dense, zero-padded coefficient array in LDS:
// e[k + h] multiplies in[p + k]; forward uses k = -offset, adjoint k = +offset (as k_conv_tile).
// ------------------------------------------------------------------------------------------------
template <int AXIS, bool MASKED>
__device__ __forceinline__ void conv1d_body(const double* __restrict__ in, double* __restrict__ out,
                                            const int* __restrict__ toff, const double* __restrict__ tw, int ntaps, int S,
                                            int h, int adjoint, const double* __restrict__ add, double add_scale,
                                            const fh_cg_state* __restrict__ states, const fh_diag_tab& mk) {
  IMG_GUARD(states, blockIdx.z / 3);
  extern __shared__ __align__(16) double lds1d[];
  const conv1d_lds L(h);
  const int span = L.span;  // staged extent along the filter axis
  const int ld = L.ld;      // row pitch (doubles)
  const int nblk = L.nblk;
  double* tile = lds1d;
  double* e = tile + L.e_off;
  const int tid = threadIdx.x;
  const int plane = blockIdx.z;
  const double* src = in + (int64_t)plane * S * S;
  // block origin: `a0` along the filter axis, `c0` across it
  const int a0 = (AXIS == 0 ? blockIdx.y : blockIdx.x) * k1dAlong;
  const int c0 = (AXIS == 0 ? blockIdx.x : blockIdx.y) * k1dAcross;
  for (int t = tid; t < nblk * k1dTB + k1dR; t += 256) e[t] = 0.0;
  __syncthreads();
  for (int t = tid; t < ntaps; t += 256) e[(adjoint ? toff[t] : -toff[t]) + h] = tw[t];
  // stage: tile[a][c] = in at (along = a0 - h + a, across = c0 + c), circular.  All loads of a batch of 8 elements per
  // thread are issued before the first LDS store (the staging is latency-bound otherwise); the wrap is a compare + add
  // wherever one step of S brings every staged index a0 - h .. a0 + 31 + h into range (uniform over the workgroup; every
  // S >= 64 with h <= 32), and a remainder where it does not: an image narrower than the tile, a list longer than the
  // image.
  const int total = span * k1dAcross;
  const bool wrap1 = a0 - h >= -S && a0 + k1dAlong - 1 + h < 2 * S;
  for (int base = 0; base < total; base += 256 * 8) {
    double v[8];
    int dst[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = base + q * 256 + tid;
      int a, c;
      if (AXIS == 0) a = idx / k1dAcross, c = idx % k1dAcross;  // consecutive lanes: consecutive x = across (coalesced)
      else c = idx / span, a = idx % span;                       // consecutive lanes: consecutive x = along (coalesced)
      int ga = a0 - h + a;
      if (!wrap1) ga %= S;
      ga += ga < 0 ? S : 0;
      ga -= ga >= S ? S : 0;
      const int gc = c0 + c;
      const bool ok = idx < total && gc < S;
      const int64_t off = AXIS == 0 ? (int64_t)ga * S + gc : (int64_t)gc * S + ga;
      v[q] = ok ? src[off] : 0.0;
      dst[q] = idx < total ? a * ld + c : -1;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (dst[q] >= 0) tile[dst[q]] = v[q];
  }
  __syncthreads();
  const int lc = tid & 63, g = tid >> 6;  // lane across, wave = group of 8 outputs along
  double acc[k1dR];
#pragma unroll
  for (int r = 0; r < k1dR; ++r) acc[r] = 0.0;
  const double* col = tile + (g * k1dR) * ld + lc;
  for (int tb = 0; tb < nblk; ++tb) {
    double wreg[k1dTB];
#pragma unroll
    for (int t = 0; t < k1dTB; ++t) wreg[t] = e[tb * k1dTB + t];
    // output r uses input index (r + k) with k = tap index in [0, 2h]; within this block taps 16 tb .. 16 tb + 15
#pragma unroll
    for (int jj = 0; jj < k1dTB + k1dR - 1; ++jj) {
      const int a = tb * k1dTB + jj;
      const double v = a < span - g * k1dR ? col[a * ld] : 0.0;
#pragma unroll
      for (int r = 0; r < k1dR; ++r) {
        const int t = jj - r;
        if (t >= 0 && t < k1dTB) acc[r] = fma(wreg[t], v, acc[r]);
      }
    }
  }
  __syncthreads();  // tile is dead: reuse it to turn the results so that stores are coalesced along x
  const double* mplane = mask_plane<MASKED>(mk, plane, S);
  if (AXIS == 0) {
    const int gx = c0 + lc;
#pragma unroll
    for (int r = 0; r < k1dR; ++r) {
      const int gy = a0 + g * k1dR + r;
      if (gx < S && gy < S) {
        const int64_t o = (int64_t)plane * S * S + (int64_t)gy * S + gx;
        double v = acc[r];
        if (MASKED) v = mplane[(int64_t)gy * S + gx] * v;
        if (add != nullptr) v = fma(add_scale, add[o], v);
        out[o] = v;
      }
    }
  } else {
    double* turn = tile;  // [64 rows y][33]
#pragma unroll
    for (int r = 0; r < k1dR; ++r) turn[lc * (k1dAlong + 1) + g * k1dR + r] = acc[r];
    __syncthreads();
    for (int idx = tid; idx < k1dAcross * k1dAlong; idx += 256) {
      const int yy = idx / k1dAlong, xx = idx % k1dAlong;
      const int gy = c0 + yy, gx = a0 + xx;
      if (gx < S && gy < S) {
        const int64_t o = (int64_t)plane * S * S + (int64_t)gy * S + gx;
        double v = turn[yy * (k1dAlong + 1) + xx];
        if (MASKED) v = mplane[(int64_t)gy * S + gx] * v;
        if (add != nullptr) v = fma(add_scale, add[o], v);
        out[o] = v;
      }
    }
  }
}

template <int AXIS>
__global__ __launch_bounds__(256) void k_conv1d(const double* __restrict__ in, double* __restrict__ out,
                                                const int* __restrict__ toff, const double* __restrict__ tw,
                                                int ntaps, int S, int h, int adjoint, const double* __restrict__ add,
                                                double add_scale, const fh_cg_state* __restrict__ states) {
  conv1d_body<AXIS, false>(in, out, toff, tw, ntaps, S, h, adjoint, add, add_scale, states, fh_diag_tab{});
}

template <int AXIS>
__global__ __launch_bounds__(256) void k_conv1d_masked(const double* __restrict__ in, double* __restrict__ out,
                                                       const int* __restrict__ toff, const double* __restrict__ tw,
                                                       int ntaps, int S, int h, int adjoint, const double* __restrict__ add,
                                                       double add_scale, const fh_cg_state* __restrict__ states,
                                                       fh_diag_tab mk) {
  conv1d_body<AXIS, true>(in, out, toff, tw, ntaps, S, h, adjoint, add, add_scale, states, mk);
}

// ------------------------------------------------------------------------------------------------
// The launch plan of fh_conv_circ: decode the ABI's halo code, choose the kernel, size its grid and LDS.  Pure host
// arithmetic (fh_conv_circ_plan answers from it without a device); conv_launch below only executes the plan.
// ------------------------------------------------------------------------------------------------
struct conv_extent {
  int hy, hx;  // max |dy|, max |dx| the kernel stages
  int axis;    // -1: 2-D tap list, 0: column list (all dx = 0), 1: row list (all dy = 0)
};

// halo codes: h = max(|dy|,|dx|) in 0..32;  -(h+1), h <= 99: column list;  -(h+101), h <= 32: row list;
// 1000 + 64 hy + hx, both <= 32: both extents
static int conv_decode(int halo, conv_extent* e) {
  if (halo >= 1000) {
    *e = {(halo - 1000) / 64, (halo - 1000) % 64, -1};
    return e->hy > 32 || e->hx > 32 ? FH_EINVAL : 0;
  }
  if (halo < -133 || halo > 32) return FH_EINVAL;
  if (halo >= 0) *e = {halo, halo, -1};
  else if (halo > -101) *e = {-halo - 1, 0, 0};
  else *e = {0, -halo - 101, 1};
  return 0;
}

enum conv_kernel { kConv1dCol = 0, kConv1dRow, kConvTile8, kConvTile, kConvDec, kConvUp, kConvDirect };  // = fh_conv_circ_plan ids

struct conv_choice {
  int kernel;
  dim3 grid;  // blocks of 256 threads
  size_t lds;
  int hy, hx, h, cap, up;  // the scalar arguments the chosen kernel takes besides the caller's
};

constexpr size_t kLdsDefault = 64 * 1024, kLdsOptIn = 100 * 1024;  // without / with the opt-in of set_kernel_attributes

static int conv_plan(int S, int ntaps, conv_extent e, int planes, int stride, int adjoint, conv_choice* c) {
  if (stride < 1 || S % stride != 0 || ntaps > kMaxTaps) return FH_EINVAL;
  *c = {kConvDirect, dim3(1), 0, e.hy, e.hx, e.hy + e.hx, 0, adjoint ? stride : 1};
  const auto tiles = [](int n, int t) { return (unsigned)((n + t - 1) / t); };
  const auto pick = [c](int kernel, dim3 grid) { return c->kernel = kernel, c->grid = grid, 0; };
  if (stride > 1 && stride <= 4 && e.axis < 0) {  // SR pair on the LDS-tiled kernels when the sizes allow
    if (!adjoint && (S / stride) % 16 == 0) {
      c->lds = conv_dec_lds(stride, e.hy, e.hx, ntaps).bytes;
      if (c->lds <= kLdsOptIn) return pick(kConvDec, dim3(S / stride / 16, S / stride / 16, planes));
    }
    if (adjoint && S % (16 * stride) == 0) {
      c->cap = conv_up_lds::cap_for(stride, e.hy, e.hx);
      c->lds = conv_up_lds(stride, e.hy, e.hx, c->cap).bytes;
      if (c->lds <= kLdsOptIn) return pick(kConvUp, dim3(S / (16 * stride), S / (16 * stride), planes));
    }
  }
  if (!adjoint && stride > 1) {
    const int64_t total = (int64_t)planes * (S / stride) * (S / stride);
    c->lds = 0;
    return pick(kConvDirect, dim3((unsigned)((total + 255) / 256)));
  }
  if (e.axis >= 0 && stride == 1 && S % 2 == 0) {  // 1-D pass at full resolution: register-blocked kernel
    c->lds = conv1d_lds(c->h).bytes;
    if (c->lds <= kLdsDefault) {
      // (by extent, not by axis: a row list of extent 0 is also a column list, and k_conv1d<1> needs h >= 1, see conv1d_lds)
      if (e.hx == 0) return pick(kConv1dCol, dim3(tiles(S, k1dAcross), tiles(S, k1dAlong), planes));
      return pick(kConv1dRow, dim3(tiles(S, k1dAlong), tiles(S, k1dAcross), planes));
    }
  }
  if (stride == 1) {  // 8 outputs per thread when the 64 x 32 tile with its halo fits
    c->lds = conv_tile8_lds(e.hy, e.hx, ntaps).bytes;
    if (c->lds <= kLdsDefault) return pick(kConvTile8, dim3(tiles(S, kT8W), tiles(S, kT8H), planes));
  }
  c->lds = conv_tile_lds(e.hy, e.hx, ntaps).bytes;
  if (c->lds > kLdsDefault) return FH_ESIZE;
  return pick(kConvTile, dim3(tiles(S, 32), tiles(S, 16), planes));
}

static int conv_plan_halo(int S, int ntaps, int halo, int planes, int stride, int adjoint, conv_choice* c) {
  conv_extent e;
  const int rc = conv_decode(halo, &e);
  return rc ? rc : conv_plan(S, ntaps, e, planes, stride, adjoint, c);
}

static int conv_launch(fh_context* ctx, const double* in, double* out, const int32_t* dy, const int32_t* dx,
                       const double* w, int ntaps, int halo, int planes, int stride, int adjoint, const double* add,
                       double add_scale, const fh_cg_state* done, hipStream_t st, const fh_batch* masks = nullptr,
                       double* spare = nullptr) {
  // masks (ops 5 / 6 and the weights of ops 8 / 9 / 10, the pass that finishes B w): out = add_scale * add + mask .* conv(in).
  // k_conv1d and k_conv_tile8 do it in their epilogue; the other kernels - every decimating pass of op 10 among them - write
  // conv(in) to `spare` (a work vector of the caller's, not in / out / add) and k_mask finishes: one more streaming pass, the
  // same bits.  Behind a decimating pass (adjoint = 0) the table is [3][S / stride][S / stride] per image.
  const int S = ctx->S;
  conv_choice c;
  const int rc = conv_plan_halo(S, ntaps, halo, planes, stride, adjoint, &c);
  if (rc) return rc;
  const dim3 b(256);
  if (masks != nullptr) {
    if ((stride != 1 && adjoint) || spare == nullptr || planes != 3 * masks->nimg) return FH_EINVAL;
    const int So = S / stride;
    fh_diag_tab mk;
    memset(&mk, 0, sizeof(mk));
    for (int i = 0; i < masks->nimg && i < FH_MAX_BATCH; ++i) mk.D[i] = masks->mask[i];
    switch (stride == 1 ? c.kernel : (int)kConvDirect) {
      case kConv1dCol: hipLaunchKernelGGL(k_conv1d_masked<0>, c.grid, b, c.lds, st, in, out, dy, w, ntaps, S, c.h, adjoint, add, add_scale, done, mk); break;
      case kConv1dRow: hipLaunchKernelGGL(k_conv1d_masked<1>, c.grid, b, c.lds, st, in, out, dx, w, ntaps, S, c.h, adjoint, add, add_scale, done, mk); break;
      case kConvTile8: hipLaunchKernelGGL(k_conv_tile8_masked, c.grid, b, c.lds, st, in, out, dy, dx, w, ntaps, S, c.hy, c.hx, adjoint, add, add_scale, done, mk); break;
      default: {
        const int rc2 = conv_launch(ctx, in, spare, dy, dx, w, ntaps, halo, planes, stride, adjoint, nullptr, 0.0, done, st);
        if (rc2) return rc2;
        hipLaunchKernelGGL(k_mask, dim3(512, 1, (unsigned)masks->nimg), b, 0, st, *masks, (const double*)spare, add, add_scale,
                           out, (int64_t)3 * So * So, done);
      }
    }
    FH_LAUNCH_CHECK();
    return 0;
  }
  switch (c.kernel) {
    case kConv1dCol: hipLaunchKernelGGL(k_conv1d<0>, c.grid, b, c.lds, st, in, out, dy, w, ntaps, S, c.h, adjoint, add, add_scale, done); break;
    case kConv1dRow: hipLaunchKernelGGL(k_conv1d<1>, c.grid, b, c.lds, st, in, out, dx, w, ntaps, S, c.h, adjoint, add, add_scale, done); break;
    case kConvTile8: hipLaunchKernelGGL(k_conv_tile8, c.grid, b, c.lds, st, in, out, dy, dx, w, ntaps, S, c.hy, c.hx, adjoint, add, add_scale, done); break;
    case kConvTile: hipLaunchKernelGGL(k_conv_tile, c.grid, b, c.lds, st, in, out, dy, dx, w, ntaps, S, c.hy, c.hx, adjoint, c.up, add, add_scale, done); break;
    case kConvDec: hipLaunchKernelGGL(k_conv_dec, c.grid, b, c.lds, st, in, out, dy, dx, w, ntaps, S, stride, c.hy, c.hx, add, add_scale, done); break;
    case kConvUp: hipLaunchKernelGGL(k_conv_up, c.grid, b, c.lds, st, in, out, dy, dx, w, ntaps, S, stride, c.hy, c.hx, c.cap, add, add_scale, done); break;
    default: hipLaunchKernelGGL(k_conv_direct, c.grid, b, 0, st, in, out, dy, dx, w, ntaps, S, stride, planes, add, add_scale, done);
  }
  FH_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The launch plan of fh_conv_frames (fh_conv_frames_plan reports it), pure host arithmetic like conv_plan.  Two routes:
//   fused : ONE k_conv_dec_frames / k_conv_up_frames launch over all frames and planes, where the single-frame kernel of that
//           direction tiles the image (So % 16 == 0 forward, S % 16 s == 0 adjoint) and the LDS for the union extents - with
//           the tap staging sized for the longest frame - fits the opt-in;
//   chain : conv_launch per frame (and, for the frame-major layout, per image), which fixes the arithmetic: every frame's sum
//           is one fma chain from 0 in list order, the adjoint adds the frames in index order through add (add_scale = 1).
// The chain's plan fields describe one of its launches (3 planes, the longest frame).  Nothing here depends on the frame count.
// ------------------------------------------------------------------------------------------------
struct frames_choice {
  int fused;
  dim3 grid;
  size_t lds;
  int hy, hx, cap;
};

static int frames_plan(int S, int nframes, int max_frame_taps, int halo, int planes, int stride, int adjoint,
                       frames_choice* c) {
  if (S < 2 || S > 256 || (S & 1) || stride < 2 || stride > 4 || S % stride != 0) return FH_EINVAL;
  if (nframes < 1 || nframes > stride * stride || max_frame_taps < 1 || max_frame_taps > kMaxTaps) return FH_EINVAL;
  if (planes < 3 || planes % 3 != 0 || halo < 1000 || (adjoint != 0 && adjoint != 1)) return FH_EINVAL;
  conv_extent e;
  int rc = conv_decode(halo, &e);
  if (rc) return rc;
  *c = {0, dim3(1), 0, e.hy, e.hx, 0};
  if (planes > 65535) return FH_ESIZE;  // (the plane is grid dimension z)
  if (!adjoint && (S / stride) % 16 == 0) {
    c->lds = conv_dec_lds(stride, e.hy, e.hx, max_frame_taps).bytes;
    if (c->lds <= kLdsOptIn) return c->fused = 1, c->grid = dim3(S / stride / 16, S / stride / 16, planes), 0;
  }
  if (adjoint && S % (16 * stride) == 0) {
    c->cap = conv_up_lds::cap_for(stride, e.hy, e.hx);
    c->lds = conv_up_lds(stride, e.hy, e.hx, c->cap).bytes;
    if (c->lds <= kLdsOptIn) return c->fused = 1, c->grid = dim3(S / (16 * stride), S / (16 * stride), planes), 0;
  }
  conv_choice one;
  rc = conv_plan(S, max_frame_taps, e, 3, stride, adjoint, &one);
  if (rc) return rc;
  c->grid = one.grid, c->lds = one.lds, c->cap = one.cap;
  return 0;
}

// FH_FRAMES_FUSED=0: the chain also where the fused kernels fit (A/B switch, like FH_CG_NO_DOT_FUSE).  Read at every op 12 / 13
// call (and by no other op), so one process can time both routes; the CG graph cache keys on it for ops 12 / 13
// (fh_graph_entry.frames_fused).
static bool frames_fused_on() {
  const char* v = getenv("FH_FRAMES_FUSED");
  return v == nullptr || atoi(v) != 0;
}

// Host copy of the device frame offsets into ctx->frame_off (the unused tail zeroed), checked: 0 = off[0] < off[1] < .. <
// off[K] = *ntaps, no frame longer than max_frame_taps.  *ntaps < 0 (fh_conv_frames, which is not told the total): the last
// offset is the total, returned there.  ONE copy and one synchronisation of `st`; never inside a stream capture (fh_amm,
// fh_conv_frames and the head of a solve).
static int frames_prepare(fh_context* ctx, const int32_t* frame_off, int nframes, int* ntaps, int max_frame_taps, hipStream_t st) {
  if (frame_off == nullptr || nframes < 1 || nframes > 16) return FH_EINVAL;
  FH_CHECK(hipMemcpyAsync(ctx->h_scal, frame_off, sizeof(int32_t) * (nframes + 1), hipMemcpyDeviceToHost, st));
  FH_CHECK(hipStreamSynchronize(st));
  memset(ctx->frame_off, 0, sizeof(ctx->frame_off));
  memcpy(ctx->frame_off, ctx->h_scal, sizeof(int32_t) * (nframes + 1));
  const int32_t* o = ctx->frame_off;
  if (*ntaps < 0) *ntaps = o[nframes];
  if (o[0] != 0 || o[nframes] != *ntaps || *ntaps < nframes || *ntaps > nframes * max_frame_taps) return FH_EINVAL;
  for (int k = 0; k < nframes; ++k)
    if (o[k + 1] <= o[k] || o[k + 1] - o[k] > max_frame_taps) return FH_EINVAL;
  return 0;
}

// the weights of ops 8 .. 11 and 13 as the per-image table of k_cg_init_w / k_cg_step2_w and of k_conv_dec_frames_w
static fh_diag_tab weights_tab(const fh_batch& per) {
  fh_diag_tab wt;
  memset(&wt, 0, sizeof(wt));
  for (int i = 0; i < per.nimg && i < FH_MAX_BATCH; ++i) wt.D[i] = per.mask[i];
  return wt;
}

// in [planes][S][S] -> out [nimg][K][3][So][So] (+ add_scale * add in that layout), or with `adjoint` back (no add).
// frames_prepare has run for these offsets.
// masks (op 13, forward only): the weights, masks->mask[i] = [K][3][So][So] of image i, multiplied in as k_mask does,
// out = add_scale * add + w .* conv(in): the fused kernel in its epilogue; the chain through conv_launch's masks / spare path,
// one one-image table per (image, frame) whose entry is that frame's three planes, with the frame's own slice of `spare` (a
// work vector of the caller's in the output's layout, not in / out / add) between the decimating pass and k_mask.
static int frames_launch(fh_context* ctx, const double* in, double* out, const int32_t* dy, const int32_t* dx,
                         const double* w, const int32_t* frame_off, int ntaps, int nframes, int max_frame_taps, int halo,
                         int planes, int stride, int adjoint, const double* add, double add_scale, const fh_cg_state* done,
                         hipStream_t st, const fh_batch* masks = nullptr, double* spare = nullptr) {
  const int S = ctx->S;
  frames_choice c;
  const int rc = frames_plan(S, nframes, max_frame_taps, halo, planes, stride, adjoint, &c);
  if (rc) return rc;
  if (planes > ctx->planes_max) return FH_ESIZE;
  if (masks != nullptr && (adjoint || spare == nullptr || planes != 3 * masks->nimg || masks->nimg > FH_MAX_BATCH))
    return FH_EINVAL;
  if (c.fused && frames_fused_on()) {
    if (adjoint)
      hipLaunchKernelGGL(k_conv_up_frames, c.grid, dim3(256), c.lds, st, in, out, dy, dx, w, frame_off, nframes, ntaps, S, stride,
                         c.hy, c.hx, c.cap, done);
    else if (masks != nullptr)
      hipLaunchKernelGGL(k_conv_dec_frames_w, c.grid, dim3(256), c.lds, st, in, out, dy, dx, w, frame_off, nframes, ntaps,
                         max_frame_taps, S, stride, c.hy, c.hx, add, add_scale, done, weights_tab(*masks));
    else
      hipLaunchKernelGGL(k_conv_dec_frames, c.grid, dim3(256), c.lds, st, in, out, dy, dx, w, frame_off, nframes, ntaps,
                         max_frame_taps, S, stride, c.hy, c.hx, add, add_scale, done);
    FH_LAUNCH_CHECK();
    return 0;
  }
  const int So = S / stride;
  const int64_t hi = (int64_t)3 * S * S, lo = (int64_t)3 * So * So;  // one image's planes at either side
  for (int i = 0; i < planes / 3; ++i) {
    const fh_cg_state* di = done != nullptr ? done + i : nullptr;  // (the launch carries one image: its own control block)
    for (int k = 0; k < nframes; ++k) {
      const int t0 = ctx->frame_off[k], n = ctx->frame_off[k + 1] - t0;
      const int64_t f = ((int64_t)i * nframes + k) * lo;
      int rc2;
      if (adjoint)
        rc2 = conv_launch(ctx, in + f, out + i * hi, dy + t0, dx + t0, w + t0, n, halo, 3, stride, 1,
                          k > 0 ? out + i * hi : nullptr, 1.0, di, st);
      else if (masks != nullptr) {
        fh_batch one;  // k_mask of an nimg = 1 launch reads mask[0], in, out and add from their bases: all four at this frame
        memset(&one, 0, sizeof(one));
        one.nimg = 1;
        one.mask[0] = masks->mask[i] + (int64_t)k * lo;
        rc2 = conv_launch(ctx, in + i * hi, out + f, dy + t0, dx + t0, w + t0, n, halo, 3, stride, 0,
                          add != nullptr ? add + f : nullptr, add_scale, di, st, &one, spare + f);
      } else
        rc2 = conv_launch(ctx, in + i * hi, out + f, dy + t0, dx + t0, w + t0, n, halo, 3, stride, 0,
                          add != nullptr ? add + f : nullptr, add_scale, di, st);
      if (rc2) return rc2;
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The launch plan of fh_conv_blend (fh_conv_blend_plan reports it), pure host arithmetic like frames_plan.  Two routes:
//   fused : ONE k_conv_blend launch over all frames and planes: the 32 x 64 tile (NR = 8) where its LDS for the union extents,
//           with the tap staging sized for the longest frame, fits the default 64 KiB, else the 32 x 16 tile (NR = 2) inside
//           the opt-in (76 KiB at hy = hx = 32 with 1024 taps: it always fits, so the plan never refuses by LDS size);
//   chain : per frame one conv_launch over all planes and one k_mask over all images (the blend maps are shared by the images)
//           through a spare work vector, which fixes the arithmetic (see k_conv_blend).  Its kernels hold at most 64 KiB, so
//           at wide extents with long lists only the fused route exists, and it then runs whatever the switch says.
// The plan reports the fused launch: it exists for every legal argument, and it is the default by measurement
// (profiles/varying_blur.md).
// ------------------------------------------------------------------------------------------------
struct blend_choice {  // the fused launch, and whether the chain exists beside it
  int chain_ok, nr;
  dim3 grid;
  size_t lds;
  int hy, hx;
};

static int blend_plan(int S, int nframes, int max_frame_taps, int halo, int planes, int adjoint, blend_choice* c) {
  if (S < 2 || S > 256 || (S & 1) || nframes < 1 || nframes > 16) return FH_EINVAL;
  if (max_frame_taps < 1 || max_frame_taps > kMaxTaps) return FH_EINVAL;
  if (planes < 3 || planes % 3 != 0 || halo < 1000 || (adjoint != 0 && adjoint != 1)) return FH_EINVAL;
  conv_extent e;
  const int rc = conv_decode(halo, &e);
  if (rc) return rc;
  *c = {0, 0, dim3(1), 0, e.hy, e.hx};
  if (planes > 65535) return FH_ESIZE;  // (the plane is grid dimension z)
  conv_choice one;
  c->chain_ok = conv_plan(S, max_frame_taps, e, planes, 1, adjoint, &one) == 0;
  // the largest NR = 2 layout (extents 32, kMaxTaps pairs) is 76 KiB: the fused kernel has a launch for every legal argument
  static_assert(96 * 80 * sizeof(double) + kMaxTaps * 16 <= kLdsOptIn, "k_conv_blend<2> must fit the opt-in at the widest extents");
  c->nr = conv_blend_lds(8, e.hy, e.hx, max_frame_taps).bytes <= kLdsDefault ? 8 : 2;
  c->lds = conv_blend_lds(c->nr, e.hy, e.hx, max_frame_taps).bytes;
  c->grid = dim3((unsigned)((S + 31) / 32), (unsigned)((S + 8 * c->nr - 1) / (8 * c->nr)), (unsigned)planes);
  return 0;
}

// FH_BLEND_FUSED=0: the chain also where the fused kernel fits (A/B switch, like FH_FRAMES_FUSED).  Read at every op 14 /
// fh_conv_blend call (and by no other op); the CG graph cache keys on it for op 14.
static bool blend_fused_on() {
  const char* v = getenv("FH_BLEND_FUSED");
  return v == nullptr || atoi(v) != 0;
}
// the route a launch takes: the switch decides only where both routes exist
static bool blend_route_fused(const blend_choice& c) { return blend_fused_on() || !c.chain_ok; }

// in [planes][S][S] -> out [planes][S][S]: out = add_scale * add + sum_k U_k .* conv(in; list k), or with `adjoint`
// out = sum_k conv^T(U_k .* in; list k) (no add).  frames_prepare has run for these offsets.  `spare`: a work vector of the
// caller's ([planes][S][S], not in / out / add) for the chain.
static int blend_launch(fh_context* ctx, const double* in, double* out, const int32_t* dy, const int32_t* dx, const double* w,
                        const int32_t* frame_off, int ntaps, int nframes, int max_frame_taps, int halo, int planes,
                        int adjoint, const double* blend, const double* add, double add_scale, const fh_cg_state* done,
                        hipStream_t st, double* spare) {
  const int S = ctx->S;
  blend_choice c;
  const int rc = blend_plan(S, nframes, max_frame_taps, halo, planes, adjoint, &c);
  if (rc) return rc;
  if (planes > ctx->planes_max) return FH_ESIZE;
  if (blend == nullptr || spare == nullptr || planes / 3 > FH_MAX_BATCH) return FH_EINVAL;
  if (blend_route_fused(c)) {
    const auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, c.grid, dim3(256), c.lds, st, in, out, dy, dx, w, frame_off, nframes, ntaps, max_frame_taps, S,
                         c.hy, c.hx, blend, adjoint ? (const double*)nullptr : add, add_scale, done);
    };
    if (c.nr == 8) adjoint ? go(k_conv_blend<8, true>) : go(k_conv_blend<8, false>);
    else adjoint ? go(k_conv_blend<2, true>) : go(k_conv_blend<2, false>);
    FH_LAUNCH_CHECK();
    return 0;
  }
  const int nimg = planes / 3;
  const int64_t n = (int64_t)3 * S * S;
  const dim3 mgrid(512, 1, (unsigned)nimg);
  for (int k = 0; k < nframes; ++k) {
    const int t0 = ctx->frame_off[k], nk = ctx->frame_off[k + 1] - t0;
    fh_batch uk;  // the maps of frame k as k_mask's per-image table: every image reads the same three planes
    memset(&uk, 0, sizeof(uk));
    uk.nimg = nimg;
    for (int i = 0; i < nimg; ++i) uk.mask[i] = blend + (int64_t)k * n;
    int rc2;
    if (adjoint) {
      hipLaunchKernelGGL(k_mask, mgrid, dim3(256), 0, st, uk, in, (const double*)nullptr, 0.0, spare, n, done);
      rc2 = conv_launch(ctx, spare, out, dy + t0, dx + t0, w + t0, nk, halo, planes, 1, 1, k > 0 ? out : nullptr, 1.0, done, st);
    } else {
      rc2 = conv_launch(ctx, in, spare, dy + t0, dx + t0, w + t0, nk, halo, planes, 1, 0, nullptr, 0.0, done, st);
      if (rc2) return rc2;
      hipLaunchKernelGGL(k_mask, mgrid, dim3(256), 0, st, uk, (const double*)spare, k > 0 ? (const double*)out : add,
                         k > 0 ? 1.0 : add_scale, out, n, done);
    }
    if (rc2) return rc2;
  }
  FH_LAUNCH_CHECK();
  return 0;
}

// The launch plan of fh_conv_window (fh_conv_window_plan reports it): one kernel, its grid and its LDS from conv_window_lds.
static int window_plan(int S, int hy, int hx, int planes, dim3* grid, size_t* lds) {
  if (S < 2 || S > 256 || (S & 1) || hy < 0 || hy > 32 || hx < 0 || hx > 32 || planes < 1) return FH_EINVAL;
  *lds = conv_window_lds(hy, hx).bytes;
  if (*lds > kLdsWindow || planes > 65535) return FH_ESIZE;  // (the plane is grid dimension z)
  *grid = dim3((unsigned)((S + kWinW - 1) / kWinW), (unsigned)((S + kWinH - 1) / kWinH), (unsigned)planes);
  return 0;
}

static int window_launch(fh_context* ctx, const double* in, double* out, const double* win, int hy, int hx, int planes,
                         int adjoint, const double* add, double add_scale, const fh_cg_state* done, hipStream_t st,
                         const fh_batch* masks = nullptr) {
  dim3 grid;
  size_t lds;
  const int rc = window_plan(ctx->S, hy, hx, planes, &grid, &lds);
  if (rc) return rc;
  if (masks != nullptr) {  // op 6: out = add_scale * add + mask .* conv(in) in the epilogue
    if (planes != 3 * masks->nimg) return FH_EINVAL;
    fh_diag_tab mk;
    memset(&mk, 0, sizeof(mk));
    for (int i = 0; i < masks->nimg && i < FH_MAX_BATCH; ++i) mk.D[i] = masks->mask[i];
    hipLaunchKernelGGL(k_conv_window_masked, grid, dim3(256), lds, st, in, out, win, ctx->S, hy, hx, adjoint, add, add_scale,
                       done, mk);
    FH_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(k_conv_window, grid, dim3(256), lds, st, in, out, win, ctx->S, hy, hx, adjoint, add, add_scale, done);
  FH_LAUNCH_CHECK();
  return 0;
}

// What the solver knows about an operator code, once: kOps[fh_problem.op].  A new operator is one row here, one arm of
// problem_check and one case of op_apply_launch (or a folded route of its own in amm_launch).
enum op_apply {      // how A is applied
  APPLY_MASK,        // A = a 0/1 mask (k_mask; the mask field is the operator itself)
  APPLY_TAPS,        // tap list through conv_launch; a second list (ntaps2 > 0) is the other factor of a separable PSF
  APPLY_WINDOW,      // dense window (window_launch): tap_w is the window, halo = 64 hy + hx
  APPLY_MIX,         // channel mix, one measurement plane per image; commutes with the DCT (its own route)
  APPLY_RECT,        // rank-1 PSF + decimation folded into rectangular DCT bases (its own route)
  APPLY_FRAMES,      // K decimated frames (frames_launch): ntaps2 counts frames, tap2_dy holds their offsets
  APPLY_BLEND,       // K blended PSFs (blend_launch): the same two fields and the maps in tap2_w; nothing decimates
  APPLY_HARTLEY      // Fourier sampling on folded Hartley bases (its own route)
};
enum op_mask {        // what the mask field (and per.mask[i] of a batch) means
  MASK_IGNORED,       // no check reads it (op 0 reads it as its operator)
  MASK_NULL,          // refused unless null: no mask on a low-resolution measurement, none on the varying blur
  MASK_VALID,         // 0/1 validity mask, one per image: idempotent, so only the first apply needs the input side
  MASK_WEIGHTS_WP,    // noise map w = 1 / sigma in the measurement's own layout ([3][n][n] per image at its side n, op 13:
                      // [K][3][So][So], frame-major); the operator reads W p, which the CG keeps beside p (cg_wp)
  MASK_WEIGHTS_SELF   // weights on the [3][S][S] frequency grid that the head butterfly reads itself: the CG keeps no W p
};
enum op_meas { MEAS_ONE_PLANE, MEAS_IMAGE, MEAS_PER_FRAME };  // measurement planes per image: 1, 3, 3 K (K = ntaps2 frames)
struct op_facts {
  op_apply apply;
  op_mask mask;           // (MASK_NULL: problem_check refuses p->mask, masks_check every per.mask[i])
  bool decimated;        // the measurement's side is S / stride
  op_meas meas;
  bool foldable;          // a separable blur that the DCT bases can absorb (fold_* set, use_dct)
  bool dot_partials;      // a route of this op hands the p.Ap block partials back from its last pass
  bool align16;           // the op's kernels read u and write out with 16-byte accesses
  bool unchecked;         // ops 0 .. 3 predate problem_check: their launch plans refuse what they cannot run
  bool (*graph_route)();  // non-null: a chain route bakes host-read offsets into a captured graph; its A/B switch (cg_graph_for)
};
constexpr int kNumOps = 16;
static const op_facts kOps[kNumOps] = {
    // apply         mask               decim. meas            fold   dot    al16   unchk  graph_route
    {APPLY_MASK,    MASK_IGNORED,      false, MEAS_IMAGE,     false, false, false, true,  nullptr},          //  0 inpainting, denoising
    {APPLY_TAPS,    MASK_IGNORED,      false, MEAS_IMAGE,     true,  true,  false, true,  nullptr},          //  1 blur
    {APPLY_TAPS,    MASK_IGNORED,      true,  MEAS_IMAGE,     false, false, false, true,  nullptr},          //  2 super-resolution
    {APPLY_MIX,     MASK_IGNORED,      false, MEAS_ONE_PLANE, false, true,  true,  true,  nullptr},          //  3 colorization
    {APPLY_WINDOW,  MASK_IGNORED,      false, MEAS_IMAGE,     false, false, false, false, nullptr},          //  4 dense-window blur
    {APPLY_TAPS,    MASK_VALID,        false, MEAS_IMAGE,     true,  true,  false, false, nullptr},          //  5 masked op 1
    {APPLY_WINDOW,  MASK_VALID,        false, MEAS_IMAGE,     false, false, false, false, nullptr},          //  6 masked op 4
    {APPLY_RECT,    MASK_NULL,         true,  MEAS_IMAGE,     false, true,  false, false, nullptr},          //  7 folded SR
    {APPLY_TAPS,    MASK_WEIGHTS_WP,   false, MEAS_IMAGE,     true,  true,  false, false, nullptr},          //  8 op 1 + noise map
    {APPLY_WINDOW,  MASK_WEIGHTS_WP,   false, MEAS_IMAGE,     false, false, false, false, nullptr},          //  9 op 4 + noise map
    {APPLY_TAPS,    MASK_WEIGHTS_WP,   true,  MEAS_IMAGE,     false, false, false, false, nullptr},          // 10 op 2 + noise map
    {APPLY_RECT,    MASK_WEIGHTS_WP,   true,  MEAS_IMAGE,     false, true,  false, false, nullptr},          // 11 op 7 + noise map
    {APPLY_FRAMES,  MASK_NULL,         true,  MEAS_PER_FRAME, false, false, false, false, frames_fused_on},  // 12 multi-frame SR
    {APPLY_FRAMES,  MASK_WEIGHTS_WP,   true,  MEAS_PER_FRAME, false, false, false, false, frames_fused_on},  // 13 op 12 + noise map
    {APPLY_BLEND,   MASK_NULL,         false, MEAS_IMAGE,     false, false, false, false, blend_fused_on},   // 14 varying blur
    {APPLY_HARTLEY, MASK_WEIGHTS_SELF, false, MEAS_IMAGE,     false, true,  true,  false, nullptr},          // 15 Fourier sampling
};
// (after problem_check has found the op in range)
static const op_facts& facts(const fh_problem* p) { return kOps[p->op]; }
// the one choice between k_cg_init_w / k_cg_step2_w, which write W p beside p, and the plain k_cg_init / k_cg_step2
static bool cg_keeps_wp(const fh_problem* p) { return facts(p).mask == MASK_WEIGHTS_WP; }

// what fh_amm / fh_cg_solve[_batched] refuse before anything is launched: one arm per field layout
// (the masks of a batched solve are per->mask[i]: masks_check);  S: the context's image side
static int problem_check(const fh_problem* p, int S) {
  if (p->op < 0 || p->op >= kNumOps) return FH_EINVAL;
  const op_facts& f = kOps[p->op];
  if (f.unchecked) return 0;
  if (f.mask == MASK_NULL && p->mask != nullptr) return FH_EINVAL;
  const bool no_folds = !p->fold_fwd_w && !p->fold_fwd_h && !p->fold_inv_w && !p->fold_inv_h;
  const bool all_folds = p->fold_fwd_w && p->fold_fwd_h && p->fold_inv_w && p->fold_inv_h;
  switch (f.apply) {
    case APPLY_HARTLEY:  // the four [S][S] folded Hartley bases and the weights, nothing of the tap-list operators
      if (p->stride != 1 || (p->use_dct != 0 && p->use_dct != 1) || p->fold_sym != 0 || p->mask == nullptr) return FH_EINVAL;
      if (!all_folds || p->ntaps != 0 || p->ntaps2 != 0 || p->halo != 0 || p->halo2 != 0) return FH_EINVAL;
      return p->tap_dy || p->tap_dx || p->tap_w || p->tap2_dy || p->tap2_dx || p->tap2_w ? FH_EINVAL : 0;
    case APPLY_BLEND: {  // ntaps2 = K PSFs, tap2_dy = their offsets, halo2 = the longest list, tap2_w = the blend maps
      const int K = p->ntaps2;
      conv_extent e;
      if (p->stride != 1 || K < 1 || K > 16 || (p->use_dct != 0 && p->use_dct != 1)) return FH_EINVAL;
      if (p->halo2 < 1 || p->halo2 > kMaxTaps || p->ntaps < K || p->ntaps > K * p->halo2) return FH_EINVAL;
      if (p->halo < 1000 || conv_decode(p->halo, &e) != 0) return FH_EINVAL;
      if (!p->tap2_dy || !p->tap2_w || !p->tap_dy || !p->tap_dx || !p->tap_w) return FH_EINVAL;
      return p->tap2_dx || p->fold_sym != 0 || !no_folds ? FH_EINVAL : 0;
    }
    case APPLY_FRAMES: {  // stride = s, ntaps2 = K frames, tap2_dy = their offsets, halo2 = the longest frame
      const int s = p->stride, K = p->ntaps2;
      if (s < 2 || s > 4 || S % s != 0 || K < 1 || K > s * s) return FH_EINVAL;
      if (p->halo2 < 1 || p->halo2 > kMaxTaps || p->ntaps < K || p->ntaps > K * p->halo2) return FH_EINVAL;
      if (p->halo < 1000 || p->tap2_dy == nullptr || !p->tap_dy || !p->tap_dx || !p->tap_w) return FH_EINVAL;
      return p->tap2_dx || p->tap2_w || p->fold_sym != 0 || !no_folds ? FH_EINVAL : 0;
    }
    case APPLY_RECT:  // the four [S][S / stride] / [S / stride][S] bases; the tap fields are not read
      return p->stride < 2 || S % p->stride != 0 || !p->use_dct || p->fold_sym != 0 || !all_folds ? FH_EINVAL : 0;
    case APPLY_WINDOW: {  // tap_w is the window, halo = 64 hy + hx, and nothing of the tap-list operators is set
      const int hy = p->halo / 64, hx = p->halo % 64;
      if (p->halo < 0 || hy > 32 || hx > 32 || p->ntaps != (2 * hy + 1) * (2 * hx + 1) || p->stride != 1) return FH_EINVAL;
      if (p->tap_w == nullptr || p->tap_dy || p->tap_dx || p->ntaps2 != 0 || p->tap2_dy || p->tap2_dx || p->tap2_w) return FH_EINVAL;
      return no_folds ? 0 : FH_EINVAL;
    }
    case APPLY_TAPS:  // stride 1, or a true decimation (op 10: the tap list of op 2)
      return (f.decimated ? p->stride < 2 || S % p->stride != 0 : p->stride != 1) ? FH_EINVAL : 0;
    default: return 0;
  }
}

// per.mask[i] of every image of the batch against the op's rule (fh_amm: the one mask of the problem)
static int masks_check(const fh_problem* p, const fh_batch& per) {
  const op_mask rule = facts(p).mask;
  if (rule == MASK_IGNORED) return 0;
  const bool want = rule != MASK_NULL;  // every image with a mask, or (MASK_NULL) every image without one
  // (weights also come in p->mask; a batch of masked blurs brings its masks in per alone)
  if (want && ((rule != MASK_VALID && p->mask == nullptr) || per.nimg < 1 || per.nimg > FH_MAX_BATCH)) return FH_EINVAL;
  for (int i = 0; i < per.nimg && i < FH_MAX_BATCH; ++i)
    if ((per.mask[i] != nullptr) != want) return FH_EINVAL;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// A_mm(u) = sigma_y^2 u + A C A^T u      (conditioning_mechanisms.py:395-400, 505-511, 653-659)
// ------------------------------------------------------------------------------------------------
// dot_part / dot_nparts (CG only): where the operator's last pass can also reduce u . (A u) per image it writes *dot_nparts
// block partials per image to dot_part (stride kCgScratch) - the caller then skips its own dot kernel; else *dot_nparts = 0
// serialises hipGraph captures (cg_graph_for) against the legacy-stream work of context creation / destruction, see there
static std::mutex g_capture_mu;

// colorization with no factor columns on the symmetric DCT passes: A C A^T is diagonal in the DCT basis (D_eff)
static bool colorize_deff_route(const fh_context* ctx, const fh_problem* p) {
  return facts(p).apply == APPLY_MIX && p->use_dct && p->m == 0 && sym_dct(ctx);
}

// once per solve (and per fh_amm call): D_eff of every image into the context's scratch, before the first apply
static int colorize_prepare(fh_context* ctx, const fh_problem* p, const fh_batch& per, hipStream_t st) {
  if (!colorize_deff_route(ctx, p)) return 0;
  if (p->tap_w == nullptr || per.nimg < 1 || per.nimg > ctx->nimg_max) return FH_EINVAL;
  for (int i = 0; i < per.nimg; ++i)
    if (per.D[i] == nullptr) return FH_EINVAL;
  if (ctx->deff == nullptr) {  // first colorization solve of this context (allocation under the capture lock, as context creation)
    std::lock_guard<std::mutex> capture_lock(g_capture_mu);
    FH_CHECK(hipMalloc(&ctx->deff, sizeof(double) * ctx->S * ctx->S * ctx->nimg_max));
  }
  const int64_t pairs = (int64_t)ctx->S * ctx->S / 2;
  hipLaunchKernelGGL(k_channel_deff, dim3((unsigned)((pairs + 255) / 256), 1, (unsigned)per.nimg), dim3(256), 0, st, per,
                     p->tap_w, ctx->deff, pairs);
  FH_LAUNCH_CHECK();
  return 0;
}

// One application of the operator, for the kinds that have kernels of their own: out = A^T in (`adjoint`; no add, no masks),
// or out = add_scale * add + A in, with the mask / weights of `masks` (null: none) multiplied into A in by the pass that
// finishes it.  spare: a work vector that is neither in nor out nor add.  The first pass of a separable PSF writes it, the
// chains of ops 12 .. 14 go through it, and so does every pass that has no masked epilogue.  Forward, `in` is a work vector
// as well and is free once it has been read.
static int op_apply_launch(fh_context* ctx, const fh_problem* p, const fh_batch& per, int adjoint, const double* in,
                           double* out, double* spare, const double* add, double add_scale, const fh_batch* masks,
                           const fh_cg_state* states, hipStream_t st) {
  const int planes = p->planes * per.nimg, halo = p->halo;
  switch (facts(p).apply) {
    case APPLY_MASK:
      hipLaunchKernelGGL(k_mask, dim3(512, 1, (unsigned)per.nimg), dim3(256), 0, st, per, in, add, add_scale, out, p->d, states);
      FH_LAUNCH_CHECK();
      return 0;
    case APPLY_WINDOW:
      return window_launch(ctx, in, out, p->tap_w, halo / 64, halo % 64, planes, adjoint, add, add_scale, states, st, masks);
    case APPLY_FRAMES:
      return frames_launch(ctx, in, out, p->tap_dy, p->tap_dx, p->tap_w, p->tap2_dy, p->ntaps, p->ntaps2, p->halo2, halo, planes,
                           p->stride, adjoint, add, add_scale, states, st, masks, spare);
    case APPLY_BLEND:
      return blend_launch(ctx, in, out, p->tap_dy, p->tap_dx, p->tap_w, p->tap2_dy, p->ntaps, p->ntaps2, p->halo2, halo, planes,
                          adjoint, p->tap2_w, add, add_scale, states, st, spare);
    case APPLY_TAPS: {
      if (p->ntaps2 <= 0)  // one list, at any stride
        return conv_launch(ctx, in, out, p->tap_dy, p->tap_dx, p->tap_w, p->ntaps, halo, planes, p->stride, adjoint, add,
                           add_scale, states, st, masks, spare);
      // separable PSF: two 1-D passes through `spare` (blur only, stride 1: amm_launch refuses another), the second list first
      // on the way back; the pass that finishes takes the add, the masks and - `in` has been read - in as its own spare
      const auto pass = [&](bool second, const double* i, double* o, const double* a, double as, const fh_batch* mk, double* sp) {
        return second ? conv_launch(ctx, i, o, p->tap2_dy, p->tap2_dx, p->tap2_w, p->ntaps2, p->halo2, planes, 1, adjoint, a, as,
                                    states, st, mk, sp)
                      : conv_launch(ctx, i, o, p->tap_dy, p->tap_dx, p->tap_w, p->ntaps, halo, planes, 1, adjoint, a, as, states, st,
                                    mk, sp);
      };
      const int rc = pass(adjoint, in, spare, nullptr, 0.0, nullptr, nullptr);
      return rc ? rc : pass(!adjoint, spare, out, add, add_scale, masks, const_cast<double*>(in));
    }
    default: return FH_EINVAL;  // the mix and the folded operators have routes of their own (amm_launch)
  }
}

// The covariance inside a folded forward pass (the folded symmetric blur on k_dct_sym: `sym`; ops 7 / 11 and op 15 on
// k_dct_rect):  w0 = C dct2(A^T in).  With no factor columns (every call above sigma = 10, i.e. three quarters of all CG
// iterations of a Heun-30 run) C z = D .* z rides in the epilogue of the forward pass - two kernels instead of three; else
// the plain pass goes to w1 (in place where in is w1) and rep_apply_launch brings it to w0.
static int cov_in_dct_launch(fh_context* ctx, const fh_problem* p, const fh_batch& per, const double* in, bool sym,
                             const fh_cg_state* states, hipStream_t st) {
  const int planes = p->planes * per.nimg;
  const auto forward = [&](double* out, const fh_batch* diag) {
    if (sym) return dct2d_launch_sym(ctx, in, out, planes, p->fold_fwd_w, p->fold_fwd_h, 0, nullptr, 0.0, states, st, diag);
    return dct_rect_launch(ctx, in, out, planes, p->fold_fwd_w, p->fold_fwd_h, ctx->S / p->stride, 0, nullptr, 0.0, states, st,
                           diag);
  };
  if (p->m == 0) return forward(ctx->w0, &per);
  const int rc = forward(ctx->w1, nullptr);
  return rc ? rc : rep_apply_launch(ctx, per, p->ldm, ctx->w1, ctx->w0, p->d, p->m, states, st);
}

// The covariance of the generic route, through the DCT basis when it lives there:  *w1 = C *w0.  The symmetric passes carry
// the diagonal-only covariance in the forward pass's epilogue and come back into the vector they started from: the two
// pointers then swap, so that the caller finds the result in *w1 and a free vector in *w0 on every route.
static int cov_apply_launch(fh_context* ctx, const fh_problem* p, const fh_batch& per, double** w0, double** w1,
                            const fh_cg_state* states, hipStream_t st) {
  const int planes = p->planes * per.nimg;
  if (!p->use_dct) return rep_apply_launch(ctx, per, p->ldm, *w0, *w1, p->d, p->m, states, st);  // identity basis
  if (p->m == 0 && sym_dct(ctx)) {
    int rc = dct2d_launch_sym(ctx, *w0, *w1, planes, ctx->sym_fwd, ctx->sym_fwd, 0, nullptr, 0.0, states, st, &per);
    if (rc) return rc;
    rc = dct2d_launch_sym(ctx, *w1, *w0, planes, ctx->sym_inv, ctx->sym_inv, 1, nullptr, 0.0, states, st);
    std::swap(*w0, *w1);
    return rc;
  }
  int rc = dct2d_launch(ctx, *w0, *w1, planes, 0, states, st);
  if (rc) return rc;
  rc = rep_apply_launch(ctx, per, p->ldm, *w1, *w0, p->d, p->m, states, st);
  return rc ? rc : dct2d_launch(ctx, *w0, *w1, planes, 1, states, st);
}

// Masked blur (op = 5: the fields of op 1, op = 6: those of op 4, both with per.mask): A = M B, so
//   A_mm(u) = sigma_y^2 u + M B C B^T M u.
// The output-side M is applied by whichever pass finishes B w, as out = fma(sigma_y^2, u, mask * t): the table of the inverse
// k_dct_sym pass, the masked epilogues of k_conv1d / k_conv_tile8 / k_conv_window, or a k_mask pass behind the kernels that
// have no such epilogue (k_conv_tile, k_conv_direct, the dense folded passes on k_gemm_f64).
// The input-side M is NOT applied here: the blur passes read `uin` (default u), and fh_amm hands in uin = M u.  The CG
// leaves uin null, and that is exact, not approximate: fh_cg_solve_batched starts from x0 = M b, so r0 = M b - A_mm(M b) is
// supported on the mask (off the mask A_mm(v) = sigma_y^2 v + 0 * t = 0 where v = 0), p0 = r0, and every later
// r = r - alpha A p, p = r + beta p keeps that support; M p is then the product of every entry with exactly 1 or of a zero
// with 0 - p itself, bit for bit.  So every iterate equals the one the fully masked operator would give.
//
// Per-pixel noise map (ops 8 / 9 / 10 / 11: the fields of ops 1 / 4 / 2 / 7 with the weights w = 1 / sigma in per.mask): the
// whitened system  A_mm(u) = sigma_y^2 u + W A0 C A0^T W u,  W = diag(w).  The output-side W takes the place of M above, in the
// same expression fma(sigma_y^2, u, w * t); op 11 hands the weights to inverse pass B of k_dct_rect as its table, op 10 runs a
// k_mask pass over the 3 So^2 measurements behind its decimating kernel.  W is not idempotent, so the input side cannot be
// skipped: every caller hands in uin = W u - fh_amm from a k_mask pass, the CG from the direction update that writes p
// (k_cg_init_w / k_cg_step2_w keep W p beside p).  u itself stays the add / dot operand: the partials are p . A_mm(p).
// Op 13 is op 12 in the same way: the adjoint frame kernels read uin = W u, and the forward ones finish with the weights
// (frames_launch: the WEIGHTED epilogue of the fused kernel, or k_mask per frame on the chain) - the same expression, so
// the two routes agree bit for bit, all-ones weights with sigma_y^2 = s^2 give op 12 and K = 1 gives op 10.
// (amm_prologue has checked p and per for the entry point that calls this)
static int amm_launch(fh_context* ctx, const fh_problem* p, const fh_batch& per, const double* u, double* out,
                      const fh_cg_state* states, hipStream_t st, double* dot_part = nullptr, int* dot_nparts = nullptr,
                      const double* uin = nullptr) {
  if (uin == nullptr) uin = u;
  if (dot_nparts != nullptr) *dot_nparts = 0;
  static const bool no_dot_fuse = getenv("FH_CG_NO_DOT_FUSE") != nullptr;  // A/B switch
  const op_facts& f = facts(p);
  if (no_dot_fuse || !f.dot_partials) dot_part = nullptr;
  const int S = ctx->S, nimg = per.nimg, planes = p->planes * nimg;
  const int64_t d = p->d;  // per image
  if (d != (int64_t)p->planes * S * S || p->planes != 3 || nimg < 1 || nimg > ctx->nimg_max) return FH_EINVAL;
  int rc;
  const fh_batch* masks = f.mask == MASK_VALID || f.mask == MASK_WEIGHTS_WP ? &per : nullptr;
  fh_batch mdiag;  // the masks as the per-image table of k_dct_sym's epilogue (indexed by the natural output pixel)
  memset(&mdiag, 0, sizeof(mdiag));
  mdiag.nimg = nimg;
  for (int i = 0; masks != nullptr && i < nimg; ++i) mdiag.D[i] = per.mask[i];
  const fh_batch* mtab = masks != nullptr ? &mdiag : nullptr;
  double *w0 = ctx->w0, *w1 = ctx->w1;
  if (f.apply == APPLY_MIX) {
    // colorization: u, out are ONE plane per image, A = channel mix with the three weights in tap_w.  The 2-D DCT acts per
    // plane, so it commutes with the mix: A C A^T u = idct2( sum_c w_c (C_dct (w_c dct2(u)))_c ) - one forward and one
    // inverse DCT over nimg planes instead of 3 nimg
    if (p->ntaps != 3 || p->tap_w == nullptr || p->stride != 1 || (S & 1)) return FH_EINVAL;
    if (3 * nimg > ctx->planes_max) return FH_ESIZE;  // the work vectors hold three planes per image
    const int64_t pairs = (int64_t)S * S / 2;
    const dim3 cgrid((unsigned)((pairs + 255) / 256), 1, (unsigned)nimg);
    const double* cw = p->tap_w;
    if (!p->use_dct) {  // identity basis: broadcast, apply, reduce (+ sigma_y^2 u)
      hipLaunchKernelGGL(k_channel_mix<true>, cgrid, dim3(256), 0, st, u, w0, cw, pairs, (const double*)nullptr, 0.0, states);
      rc = rep_apply_launch(ctx, per, p->ldm, w0, w1, d, p->m, states, st);
      if (rc) return rc;
      hipLaunchKernelGGL(k_channel_mix<false>, cgrid, dim3(256), 0, st, (const double*)w1, out, cw, pairs, u, p->sigma_y2,
                         states);
      FH_LAUNCH_CHECK();
      return 0;
    }
    if (colorize_deff_route(ctx, p)) {
      // no factor columns: D_eff = sum_c w_c^2 D_c (colorize_prepare, once per solve) rides in the forward pass's epilogue
      fh_batch de;
      memset(&de, 0, sizeof(de));
      de.nimg = nimg;
      for (int i = 0; i < nimg; ++i) de.D[i] = ctx->deff + (int64_t)i * S * S;
      rc = dct2d_launch_sym(ctx, u, w0, nimg, ctx->sym_fwd, ctx->sym_fwd, 0, nullptr, 0.0, states, st, &de, nullptr, 0, nullptr,
                            1);
      if (rc) return rc;
      return dct2d_launch_sym(ctx, w0, out, nimg, ctx->sym_inv, ctx->sym_inv, 1, u, p->sigma_y2, states, st, nullptr, dot_part,
                              kCgScratch, dot_nparts, 1);
    }
    rc = dct2d_launch(ctx, u, w1, nimg, 0, states, st, 1);
    if (rc) return rc;
    hipLaunchKernelGGL(k_channel_mix<true>, cgrid, dim3(256), 0, st, (const double*)w1, w0, cw, pairs, (const double*)nullptr,
                       0.0, states);
    rc = rep_apply_launch(ctx, per, p->ldm, w0, w1, d, p->m, states, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_channel_mix<false>, cgrid, dim3(256), 0, st, (const double*)w1, w0, cw, pairs, (const double*)nullptr,
                       0.0, states);
    return dct2d_launch(ctx, w0, out, nimg, 1, states, st, 1, u, p->sigma_y2, dot_part, kCgScratch, dot_nparts);
  }
  if (f.apply == APPLY_RECT) {
    // rank-1 PSF + decimation folded into rectangular DCT bases: out = sigma_y^2 u + A idct2( C dct2(A^T u) ) in four small
    // dense passes + the apply; u, out are [3][So][So] per image.
    // op 11: the first pass reads uin = W u, and inverse pass B carries the weights as its table, out = fma(sigma_y^2, u, w * t)
    rc = cov_in_dct_launch(ctx, p, per, uin, false, states, st);
    if (rc) return rc;
    return dct_rect_launch(ctx, w0, out, planes, p->fold_inv_w, p->fold_inv_h, S / p->stride, 1, u, p->sigma_y2, states, st, mtab,
                           dot_part, kCgScratch, dot_nparts);
  }
  if (f.apply == APPLY_HARTLEY) {
    // Fourier sampling, A0 = H = R o (Hc . Hc) with Hc folded into the DCT bases (P = C_dct Hc, or Hc itself on the identity
    // basis):  out = sigma_y^2 u + W R( P^T (C (P R(W u) P^T)) P ).  The head butterfly reads u and the weights itself (uin is
    // not used: the CG keeps no W p vector for this op), the tail one finishes fma(sigma_y^2, u, w * R(t)) and the p.Ap partials.
    // (16-byte accesses, and the tail butterfly reads u while it writes out: amm_prologue has refused other operands)
    rc = hartley_launch(ctx, u, w1, planes, &per, nullptr, 0, nullptr, 0.0, states, st);
    if (rc) return rc;
    rc = cov_in_dct_launch(ctx, p, per, w1, false, states, st);
    if (rc) return rc;
    rc = dct_rect_launch(ctx, w0, w1, planes, p->fold_inv_w, p->fold_inv_h, S, 1, nullptr, 0.0, states, st);
    if (rc) return rc;
    return hartley_launch(ctx, w1, out, planes, nullptr, &per, 0, u, p->sigma_y2, states, st, dot_part, kCgScratch, dot_nparts);
  }
  // a second tap list outside ops 12 .. 14 (which count frames there) is the other factor of a separable PSF: stride 1 only
  if (f.apply != APPLY_FRAMES && f.apply != APPLY_BLEND && p->ntaps2 > 0 && p->stride != 1) return FH_EINVAL;
  if (f.foldable && p->use_dct && p->fold_fwd_w != nullptr) {
    // separable blur folded into the DCT bases: out = sigma_y^2 u + A idct2( C dct2(A^T u) ) in 4 dense passes + the
    // apply, instead of 4 blur passes + 4 DCT passes + the apply + an axpy epilogue
    if (!p->fold_fwd_h || !p->fold_inv_w || !p->fold_inv_h) return FH_EINVAL;
    if (p->fold_sym) {  // symmetric PSF: the fold pointers are packed half bases (k_dct_sym)
      rc = cov_in_dct_launch(ctx, p, per, uin, true, states, st);
      if (rc) return rc;
      return dct2d_launch_sym(ctx, w0, out, planes, p->fold_inv_w, p->fold_inv_h, 1, u, p->sigma_y2, states, st, mtab,
                              dot_part, kCgScratch, dot_nparts);
    }
    rc = dct2d_launch_bases(ctx, uin, w1, planes, p->fold_fwd_w, p->fold_fwd_h, nullptr, 0.0, states, st);
    if (rc) return rc;
    rc = rep_apply_launch(ctx, per, p->ldm, w1, w0, d, p->m, states, st);
    if (rc) return rc;
    if (masks == nullptr) return dct2d_launch_bases(ctx, w0, out, planes, p->fold_inv_w, p->fold_inv_h, u, p->sigma_y2, states, st);
    // k_gemm_f64 has no masked epilogue: B w to w1, then out = sigma_y^2 u + mask .* w1
    rc = dct2d_launch_bases(ctx, w0, w1, planes, p->fold_inv_w, p->fold_inv_h, nullptr, 0.0, states, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mask, dim3(512, 1, (unsigned)nimg), dim3(256), 0, st, per, (const double*)w1, u, p->sigma_y2, out, d, states);
    FH_LAUNCH_CHECK();
    return 0;
  }
  // w0 = A^T u  (w1 is free until the covariance apply: the spare)
  rc = op_apply_launch(ctx, p, per, 1, uin, w0, w1, nullptr, 0.0, nullptr, states, st);
  if (rc) return rc;
  // w1 = C w0  (the two may have swapped)
  rc = cov_apply_launch(ctx, p, per, &w0, &w1, states, st);
  if (rc) return rc;
  // out = sigma_y^2 u + A w1  (w0 has been read: the spare)
  return op_apply_launch(ctx, p, per, 0, w1, out, w0, u, p->sigma_y2, masks, states, st);
}

// What fh_amm and fh_cg_solve_batched do once, before the first apply: every refusal that needs no launch, D_eff of the
// colorization route, the host copy of the frame offsets, the CG's W p vector, and the input side of the first apply.
// in / io: the entry point's measurement-space operands (u / out, b / x).  *n: the measurement's length per image.
// *uin: null, or `in` times the op's mask / weights (amm_launch: the input-side M or W), left in a CG vector.
enum amm_entry { ENTRY_AMM, ENTRY_SOLVE };  // where the two have always answered differently, each keeps its answer
static int amm_prologue(fh_context* ctx, const fh_problem* p, const fh_batch& per, amm_entry entry, const double* in,
                        const double* io, hipStream_t st, int64_t* n, const double** uin) {
  const int S = ctx->S, nimg = per.nimg;
  *uin = nullptr;
  if (problem_check(p, S) || masks_check(p, per)) return FH_EINVAL;
  const op_facts& f = facts(p);
  if (f.decimated && p->stride < 1) return FH_EINVAL;  // (op 2, whose stride problem_check leaves to conv_plan)
  const int So = S / (f.decimated ? p->stride : 1);
  // per image: one plane for colorization, 3 K for the K frames of ops 12 / 13, else 3
  *n = (int64_t)(f.meas == MEAS_ONE_PLANE ? 1 : (f.meas == MEAS_PER_FRAME ? p->ntaps2 : 1) * p->planes) * So * So;
  const bool maps = f.mask == MASK_VALID || f.mask == MASK_WEIGHTS_WP || f.mask == MASK_WEIGHTS_SELF;
  if (maps || f.graph_route != nullptr) {  // sizes, before the offsets are read and before the first launch
    if (p->planes != 3 || p->d != (int64_t)3 * S * S) return FH_EINVAL;
    if (entry == ENTRY_SOLVE && *n * nimg > (int64_t)ctx->planes_max * S * S) return FH_EINVAL;  // the CG vectors hold the batch
    if (entry == ENTRY_AMM && maps && ctx->planes_max < 3) return FH_ESIZE;
  }
  if (f.align16 && !aligned16(in, io)) return FH_EINVAL;  // k_channel_mix, k_hartley_fix: 16-byte accesses
  const bool self = f.mask == MASK_WEIGHTS_SELF;
  if (self && entry == ENTRY_AMM && in == io) return FH_EINVAL;  // the tail butterfly reads u while it writes out
  for (int i = 0; self && i < nimg; ++i)  // (the weights: masks_check found them non-null)
    if (!aligned16(per.mask[i])) return FH_EINVAL;
  int rc = colorize_prepare(ctx, p, per, st);
  if (rc) return rc;
  int total = p->ntaps;  // the offsets, read and checked once (the chain route launches from the host copy)
  rc = f.graph_route != nullptr ? frames_prepare(ctx, p->tap2_dy, p->ntaps2, &total, p->halo2, st) : 0;
  if (rc) return rc;
  if (f.mask != MASK_VALID && f.mask != MASK_WEIGHTS_WP) return 0;
  // The input-side mask / weights of the first apply (amm_launch: uin), one k_mask pass into a CG vector.  fh_amm: cg_p (idle).
  // Solve of a masked blur: the system is solved for M b - the one masking of a solve; the iteration then needs no input-side
  // mask.  M b goes to cg_x for the first apply (and, once that has released the work vectors, to w0 for k_cg_init).
  // Solve with a noise map: b is the caller's whitened right-hand side and is solved for as given.  W p of every iteration
  // lives in one more CG vector, allocated by the first such solve of this context (under the capture lock, as
  // colorize_prepare's scratch; never inside a capture); W b for the x0 = b apply goes there (cg_scipy: x0 = 0, no such apply).
  if (entry == ENTRY_SOLVE && f.mask == MASK_WEIGHTS_WP) {
    if (ctx->cg_wp == nullptr) {
      std::lock_guard<std::mutex> capture_lock(g_capture_mu);
      FH_CHECK(hipMalloc(&ctx->cg_wp, sizeof(double) * ctx->nimg_max * 3 * S * S));
    }
    if (p->cg_scipy) return 0;
  }
  double* dst = entry == ENTRY_AMM ? ctx->cg_p : (f.mask == MASK_VALID ? ctx->cg_x : ctx->cg_wp);
  hipLaunchKernelGGL(k_mask, dim3(512, 1, (unsigned)nimg), dim3(256), 0, st, per, in, (const double*)nullptr, 0.0, dst, *n,
                     (const fh_cg_state*)nullptr);
  *uin = dst;
  return 0;
}

static fh_batch batch_of(const fh_problem* p) {
  fh_batch per;
  memset(&per, 0, sizeof(per));
  per.nimg = 1;
  per.D[0] = p->D, per.r[0] = p->r, per.B[0] = p->B, per.M[0] = p->M, per.mask[0] = p->mask;
  return per;
}

// ------------------------------------------------------------------------------------------------
// Conjugate gradients, conditioning_utils/cg.py:232-282 (M = I, x0 = b).  Scalars stay on the device;
// the two reductions per iteration are block partials re-summed by every workgroup of the next kernel.
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int n, double* red) {
  double s = threadIdx.x < n ? part[threadIdx.x] : 0.0;
  return block_sum_256(s, red);
}

// r = b - Ab ; p = r ; x = b ; partial r.r and b.b
// WEIGHTED (here and in cg_step2_body; ops 8 .. 11): the kernel that writes the direction p also writes wp = w .* p, the input
// of the next operator apply (amm_launch: uin), from the weights wt.D[image] ([n] per image).  A compile-time flag, as MASKED
// in the convolution kernels: the unweighted entry points instantiate `false` and never touch wt / wp.
template <bool WEIGHTED>
__device__ __forceinline__ void cg_init_body(const double* __restrict__ b, const double* __restrict__ Ab,
                                             double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                             double* __restrict__ part, int64_t n, const fh_diag_tab& wt,
                                             double* __restrict__ wp) {
  const double* __restrict__ w = nullptr;
  {
    const int64_t off = (int64_t)blockIdx.z * n;
    b += off, x += off, r += off, p += off;
    if (Ab != nullptr) Ab += off;
    part += (int64_t)blockIdx.z * kCgScratch;
    if (WEIGHTED) w = wt.D[blockIdx.z], wp += off;
  }
  __shared__ double red[4];
  double srr = 0.0, sbb = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double bi = b[i], ri = Ab != nullptr ? bi - Ab[i] : bi;  // Ab == null: x0 = 0 (scipy's start), r = b
    x[i] = Ab != nullptr ? bi : 0.0;
    r[i] = ri;
    p[i] = ri;
    if (WEIGHTED) wp[i] = w[i] * ri;
    srr = fma(ri, ri, srr);
    sbb = fma(bi, bi, sbb);
  }
  srr = block_sum_256(srr, red);
  sbb = block_sum_256(sbb, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = srr;
    part[kDotBlocks + blockIdx.x] = sbb;
  }
}

__global__ __launch_bounds__(256) void k_cg_init(const double* __restrict__ b, const double* __restrict__ Ab,
                                                 double* __restrict__ x, double* __restrict__ r,
                                                 double* __restrict__ p, double* __restrict__ part, int64_t n) {
  cg_init_body<false>(b, Ab, x, r, p, part, n, fh_diag_tab{}, nullptr);
}

__global__ __launch_bounds__(256) void k_cg_init_w(const double* __restrict__ b, const double* __restrict__ Ab,
                                                   double* __restrict__ x, double* __restrict__ r,
                                                   double* __restrict__ p, double* __restrict__ part, int64_t n,
                                                   fh_diag_tab wt, double* __restrict__ wp) {
  cg_init_body<true>(b, Ab, x, r, p, part, n, wt, wp);
}

__global__ __launch_bounds__(256) void k_cg_init_fin(const double* __restrict__ part, int nparts, RtolArr rtols,
                                                     double atol, int maxiter, fh_cg_state* __restrict__ stt,
                                                     double* __restrict__ rzbuf, int scipy_mode) {
  const double rtol = rtols.v[blockIdx.z];
  part += (int64_t)blockIdx.z * kCgScratch;
  rzbuf += (int64_t)blockIdx.z * kCgScratch;
  stt += blockIdx.z;
  __shared__ double red[4];
  const double srr = sum_partials(part, nparts, red);
  const double sbb = sum_partials(part + kDotBlocks, nparts, red);
  if (threadIdx.x == 0) {
    rzbuf[0] = srr;
    stt->rz = srr;
    stt->rnorm = sqrt(srr);
    stt->bnorm = sqrt(sbb);
    const double s = rtol * sqrt(sbb);
    stt->stop = s > atol ? s : atol;
    stt->done = 0;
    stt->niter = 0;
    stt->optimal = 0;
    stt->it = 0;
    stt->k_cur = 0;
    stt->maxiter = maxiter;
    stt->scipy_mode = scipy_mode;
    if (scipy_mode && sqrt(srr) <= stt->stop) {  // scipy tests the initial residual before the first iteration
      stt->optimal = 1;
      stt->done = 1;
    }
  }
}

// iteration k, first half: pAp check, x += alpha p, r -= alpha Ap, partial r.r
__global__ __launch_bounds__(256) void k_cg_step1(const double* __restrict__ p, const double* __restrict__ ap,
                                                  double* __restrict__ x, double* __restrict__ r,
                                                  const double* __restrict__ part_pap, int nparts,
                                                  double* __restrict__ part_rr, const double* __restrict__ rzbuf,
                                                  fh_cg_state* __restrict__ stt, int64_t n) {
  {
    const int64_t off = (int64_t)blockIdx.z * n, so = (int64_t)blockIdx.z * kCgScratch;
    p += off, ap += off, x += off, r += off;
    part_pap += so, part_rr += so, rzbuf += so;
    stt += blockIdx.z;
  }
  if (stt->done) return;
  const int it = stt->it, k = it + 1;
  if (it >= stt->maxiter) {  // cg.py:245 loop bound; the host reports niter = maxiter
    if (blockIdx.x == 0 && threadIdx.x == 0) stt->done = 3;
    return;
  }
  __shared__ double red[4];
  const double pAp = sum_partials(part_pap, nparts, red);
  if (stt->scipy_mode ? pAp == 0.0 : pAp <= 1e-16) {  // cg.py:250 (scipy has no such test: only an exact zero stops it here)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      stt->pAp = pAp;
      stt->niter = k;
      stt->done = 2;
    }
    return;
  }
  const double alpha = rzbuf[(k - 1) & 1] / pAp;
  double srr = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    x[i] = fma(alpha, p[i], x[i]);
    const double ri = fma(-alpha, ap[i], r[i]);
    r[i] = ri;
    srr = fma(ri, ri, srr);
  }
  srr = block_sum_256(srr, red);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = srr;
  if (blockIdx.x == 0 && threadIdx.x == 0) stt->k_cur = k;
}

// iteration k, second half: stopping test, p = r + beta p  (WEIGHTED: and wp = w .* p, see cg_init_body; an image that is
// done leaves wp as it leaves p)
template <bool WEIGHTED>
__device__ __forceinline__ void cg_step2_body(const double* __restrict__ r, double* __restrict__ p,
                                              const double* __restrict__ part_rr, int nparts, double* __restrict__ rzbuf,
                                              fh_cg_state* __restrict__ stt, int64_t n, const fh_diag_tab& wt,
                                              double* __restrict__ wp) {
  const double* __restrict__ w = nullptr;
  {
    const int64_t off = (int64_t)blockIdx.z * n, so = (int64_t)blockIdx.z * kCgScratch;
    r += off, p += off;
    part_rr += so, rzbuf += so;
    stt += blockIdx.z;
    if (WEIGHTED) w = wt.D[blockIdx.z], wp += off;
  }
  if (stt->done) return;
  const int k = stt->k_cur;
  __shared__ double red[4];
  const double rz_new = sum_partials(part_rr, nparts, red);
  const double rnorm = sqrt(rz_new);
  if (rnorm <= stt->stop) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      stt->rnorm = rnorm;
      stt->niter = k;
      stt->optimal = 1;
      stt->done = 1;
    }
    return;
  }
  const double beta = rz_new / rzbuf[(k - 1) & 1];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double pi = fma(beta, p[i], r[i]);
    p[i] = pi;
    if (WEIGHTED) wp[i] = w[i] * pi;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rzbuf[k & 1] = rz_new;
    stt->rnorm = rnorm;
    stt->niter = k;
    stt->it = k;
  }
}

__global__ __launch_bounds__(256) void k_cg_step2(const double* __restrict__ r, double* __restrict__ p,
                                                  const double* __restrict__ part_rr, int nparts,
                                                  double* __restrict__ rzbuf, fh_cg_state* __restrict__ stt,
                                                  int64_t n) {
  cg_step2_body<false>(r, p, part_rr, nparts, rzbuf, stt, n, fh_diag_tab{}, nullptr);
}

__global__ __launch_bounds__(256) void k_cg_step2_w(const double* __restrict__ r, double* __restrict__ p,
                                                    const double* __restrict__ part_rr, int nparts,
                                                    double* __restrict__ rzbuf, fh_cg_state* __restrict__ stt, int64_t n,
                                                    fh_diag_tab wt, double* __restrict__ wp) {
  cg_step2_body<true>(r, p, part_rr, nparts, rzbuf, stt, n, wt, wp);
}

// ================================================================================================
// C ABI
// ================================================================================================
// Every kernel of this file that needs more than 64 KiB of dynamic LDS gets its opt-in here, from fh_context_create (under
// g_capture_mu, before any launch and outside any capture): no kernel of this file launches without a context.
static int set_kernel_attributes() {
  const void* const at_140k[] = {(const void*)k_dct_sym<false, 3>,    (const void*)k_dct_sym<true, 3>,
                                 (const void*)k_dct_sym<false, 1>,    (const void*)k_dct_sym<true, 1>,
                                 (const void*)k_dct_sym<false, 3, 2>, (const void*)k_dct_sym<true, 3, 2>,
                                 (const void*)k_dct_sym<false, 1, 2>, (const void*)k_dct_sym<true, 1, 2>,
                                 (const void*)k_woodbury_inner,       (const void*)k_dct_rect<3>};
  for (const void* fn : at_140k) FH_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
  for (const void* fn : {(const void*)k_conv_dec, (const void*)k_conv_up, (const void*)k_conv_dec_frames,
                         (const void*)k_conv_dec_frames_w, (const void*)k_conv_up_frames,
                         (const void*)k_conv_blend<8, false>, (const void*)k_conv_blend<8, true>,
                         (const void*)k_conv_blend<2, false>, (const void*)k_conv_blend<2, true>})
    FH_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsOptIn));
  for (const void* fn : {(const void*)k_conv_window, (const void*)k_conv_window_masked})
    FH_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsWindow));
  return 0;
}

extern "C" {

int fh_version(void) { return 100; }

int fh_context_create(fh_context** out, int S, int planes_max, int m_cap) {
  if (out == nullptr || S < 2 || S > 256 || (S & 1) || planes_max < 1 || m_cap < 0 || m_cap > FH_MAX_COLS)
    return FH_EINVAL;
  std::lock_guard<std::mutex> capture_lock(g_capture_mu);
  const int rc_attr = set_kernel_attributes();
  if (rc_attr) return rc_attr;
  fh_context* c = new fh_context();
  memset(c, 0, sizeof(*c));
  c->S = S;
  c->planes_max = planes_max;
  c->nimg_max = planes_max / 3 > 0 ? planes_max / 3 : 1;
  if (c->nimg_max > FH_MAX_BATCH) c->nimg_max = FH_MAX_BATCH;
  c->m_cap = m_cap;
  const size_t nimg = (size_t)planes_max * S * S;
  std::vector<double> bas((size_t)S * S), bast((size_t)S * S);
  for (int k = 0; k < S; ++k) {
    const long double sk = k == 0 ? sqrtl(1.0L / S) : sqrtl(2.0L / S);
    for (int n = 0; n < S; ++n) {
      const long double v = sk * cosl(M_PIl * (2 * n + 1) * k / (2.0L * S));
      bas[(size_t)k * S + n] = (double)v;
      bast[(size_t)n * S + k] = (double)v;
    }
  }
  const int ntiles = (m_cap + kGT - 1) / kGT;
  const int npairs = ntiles * (ntiles + 1) / 2;
  // Gram partials: one image at the context's column capacity, or (batched covariance updates, <= 64 columns: one tile
  // pair) every image of a batch side by side
  const int pairs_batched = m_cap > 0 ? c->nimg_max : 0;
  const int pairs = npairs > pairs_batched ? npairs : pairs_batched;
  c->gpartial_elems = (int64_t)(pairs > 0 ? pairs : 1) * kGramRowBlocks * kGT * kGT;
  FH_CHECK(hipMalloc(&c->basis, sizeof(double) * S * S));
  FH_CHECK(hipMalloc(&c->basis_t, sizeof(double) * S * S));
  FH_CHECK(hipMemcpy(c->basis, bas.data(), sizeof(double) * S * S, hipMemcpyHostToDevice));
  FH_CHECK(hipMemcpy(c->basis_t, bast.data(), sizeof(double) * S * S, hipMemcpyHostToDevice));
  if (S % 128 == 0) {  // packed half bases of the symmetric passes: forward [Pe; Po], inverse [Qe; Qo] (k_dct_sym)
    const int H = S / 2;
    std::vector<double> sf((size_t)2 * H * H), si((size_t)2 * H * H);
    for (int j = 0; j < H; ++j)
      for (int n = 0; n < H; ++n) {
        sf[(size_t)j * H + n] = bas[(size_t)(2 * j) * S + n];                      // Pe[j][n] = C[2j][n]
        sf[(size_t)H * H + (size_t)j * H + n] = bas[(size_t)(2 * j + 1) * S + n];  // Po[j][n] = C[2j+1][n]
        si[(size_t)j * H + n] = bas[(size_t)(2 * n) * S + j];                      // Qe[k][j'] = C[2j'][k]  (here k = j, j' = n)
        si[(size_t)H * H + (size_t)j * H + n] = bas[(size_t)(2 * n + 1) * S + j];  // Qo[k][j'] = C[2j'+1][k]
      }
    FH_CHECK(hipMalloc(&c->sym_fwd, sizeof(double) * 2 * H * H));
    FH_CHECK(hipMalloc(&c->sym_inv, sizeof(double) * 2 * H * H));
    FH_CHECK(hipMemcpy(c->sym_fwd, sf.data(), sizeof(double) * 2 * H * H, hipMemcpyHostToDevice));
    FH_CHECK(hipMemcpy(c->sym_inv, si.data(), sizeof(double) * 2 * H * H, hipMemcpyHostToDevice));
  }
  FH_CHECK(hipMalloc(&c->tmp_img, sizeof(double) * nimg));
  FH_CHECK(hipMalloc(&c->partial, sizeof(double) * kPartialRows * FH_MAX_COLS * c->nimg_max));
  FH_CHECK(hipMalloc(&c->gpartial, sizeof(double) * c->gpartial_elems));
  FH_CHECK(hipMalloc(&c->sync, sizeof(unsigned int) * (FH_MAX_BATCH * kSyncStride + 32)));
  FH_CHECK(hipMemset(c->sync, 0, sizeof(unsigned int) * (FH_MAX_BATCH * kSyncStride + 32)));
  {
    int dev = 0, cus = 0;
    FH_CHECK(hipGetDevice(&dev));
    FH_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    c->num_cus = cus;
  }
  FH_CHECK(hipMalloc(&c->coef, sizeof(double) * 2 * FH_MAX_COLS * c->nimg_max));
  FH_CHECK(hipMemset(c->coef, 0, sizeof(double) * 2 * FH_MAX_COLS));
  FH_CHECK(hipMalloc(&c->cg_r, sizeof(double) * nimg));
  FH_CHECK(hipMalloc(&c->cg_p, sizeof(double) * nimg));
  FH_CHECK(hipMalloc(&c->cg_ap, sizeof(double) * nimg));
  FH_CHECK(hipMalloc(&c->cg_x, sizeof(double) * nimg));
  FH_CHECK(hipMalloc(&c->w0, sizeof(double) * nimg));
  FH_CHECK(hipMalloc(&c->w1, sizeof(double) * nimg));
  FH_CHECK(hipMalloc(&c->w2, sizeof(double) * kCgScratch * c->nimg_max));
  FH_CHECK(hipMalloc(&c->cg_state, sizeof(fh_cg_state) * c->nimg_max));
  FH_CHECK(hipMemset(c->cg_state, 0, sizeof(fh_cg_state) * c->nimg_max));
  FH_CHECK(hipHostMalloc((void**)&c->h_state, sizeof(fh_cg_state) * c->nimg_max, hipHostMallocDefault));
  FH_CHECK(hipHostMalloc((void**)&c->h_scal, sizeof(double) * 64, hipHostMallocDefault));
  *out = c;
  return 0;
}

int fh_context_destroy(fh_context* c) {
  if (c == nullptr) return 0;
  std::lock_guard<std::mutex> capture_lock(g_capture_mu);
  void* bufs[] = {c->basis, c->basis_t, c->tmp_img, c->partial, c->gpartial, c->coef, c->cg_r,
                  c->cg_p,  c->cg_ap,   c->w0,      c->w1,      c->w2,       c->cg_state, c->sync,
                  c->sym_fwd, c->sym_inv, c->deff, c->cg_wp};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  for (auto& g : c->graphs)
    if (g.exec) {
      (void)hipGraphExecDestroy(g.exec);
      (void)hipGraphDestroy(g.graph);
    }
  if (c->cg_x) (void)hipFree(c->cg_x);
  if (c->h_state) (void)hipHostFree(c->h_state);
  if (c->h_scal) (void)hipHostFree(c->h_scal);
  delete c;
  return 0;
}

// a captured CG chunk bakes in the apply kernel that `exclusive` / `fused_disabled` selected at capture time: drop the cached
// graphs whenever that selection can change, so a graph never replays the single-sweep kernel on a context that has since
// lost its exclusivity (or had a time-out reported)
static void drop_graphs(fh_context* ctx) {
  for (auto& g : ctx->graphs) {
    if (g.exec != nullptr) {
      (void)hipGraphExecDestroy(g.exec);
      (void)hipGraphDestroy(g.graph);
      g.exec = nullptr;
      g.graph = nullptr;
    }
  }
}

int fh_context_set_exclusive(fh_context* ctx, int exclusive) {
  if (!ctx) return FH_EINVAL;
  const int e = exclusive < 0 ? 0 : (exclusive > 2 ? 2 : exclusive);
  if ((e >= 2) != (ctx->exclusive >= 2)) drop_graphs(ctx);  // (levels 0 and 1 select the same kernels)
  ctx->exclusive = e;
  return 0;
}

int fh_debug_read_stamps(fh_context* ctx, unsigned long long* out_host, int count, void* stream) {
  if (!ctx || !out_host || count < 1 || (int64_t)count > ctx->gpartial_elems) return FH_EINVAL;
  FH_CHECK(hipMemcpyAsync(out_host, ctx->gpartial, sizeof(unsigned long long) * count, hipMemcpyDeviceToHost, (hipStream_t)stream));
  FH_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int fh_context_status(fh_context* ctx, void* stream) {
  if (!ctx) return FH_EINVAL;
  unsigned int flag = 0;
  FH_CHECK(hipMemcpyAsync(&flag, ctx->sync + FH_MAX_BATCH * kSyncStride, sizeof(flag), hipMemcpyDeviceToHost,
                          (hipStream_t)stream));
  FH_CHECK(hipStreamSynchronize((hipStream_t)stream));
  if (flag == 0) return 0;
  // a single-sweep apply timed out waiting for its peers (another grid-synchronising kernel shared the GPU): its output
  // is invalid.  Re-arm the counters, keep this context on the two-pass kernels and report.
  ctx->fused_disabled = 1;
  drop_graphs(ctx);
  FH_CHECK(hipMemsetAsync(ctx->sync, 0, sizeof(unsigned int) * (FH_MAX_BATCH * kSyncStride + 32), (hipStream_t)stream));
  FH_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return FH_ESYNC;
}

int fh_dct_sym_plan(int S, int planes, int* gx, int* gy, int* gz, int* ns, int64_t* lds_bytes) {
  if (S < 128 || S % 128 != 0 || planes < 1 || !gx || !gy || !gz || !ns || !lds_bytes) return FH_EINVAL;
  const dct_sym_plan_t pn = dct_sym_plan(S, planes);
  *gx = pn.gx, *gy = pn.gy, *gz = pn.gz, *ns = pn.ns, *lds_bytes = pn.lds_bytes;
  return 0;
}

int fh_dct_rect_plan(int S, int So, int planes, int inverse, int32_t out[10]) {
  if (out == nullptr) return FH_EINVAL;
  memset(out, 0, sizeof(int32_t) * 10);
  if (!dct_rect_sizes_ok(S, So, planes)) return FH_EINVAL;
  int shp[2][3];
  dct_rect_shapes(S, So, inverse != 0, shp);
  for (int i = 0; i < 2; ++i) {
    const dct_rect_plan_t pn = dct_rect_plan(shp[i][0], shp[i][1], shp[i][2], planes);
    if (pn.lds_bytes > kLdsRect) {
      memset(out, 0, sizeof(int32_t) * 10);
      return FH_ESIZE;
    }
    out[5 * i] = pn.gx, out[5 * i + 1] = pn.gy, out[5 * i + 2] = pn.gz, out[5 * i + 3] = 256, out[5 * i + 4] = (int32_t)pn.lds_bytes;
  }
  return 0;
}

int fh_dct_rect(fh_context* ctx, const double* in, double* out, const double* P_w, const double* P_h, int So, int planes,
                int inverse, void* stream) {
  if (!ctx || !in || !out || !P_w || !P_h) return FH_EINVAL;
  return dct_rect_launch(ctx, in, out, planes, P_w, P_h, So, inverse != 0, nullptr, 0.0, nullptr, (hipStream_t)stream);
}

int fh_hartley_fix(fh_context* ctx, const double* in, double* out, const double* w, const double* add, double add_scale,
                   int planes, void* stream) {
  if (!ctx || !in || !out || in == out || planes < 1 || planes > 65535) return FH_EINVAL;
  if (add == out || w == out) return FH_EINVAL;  // (the kernel's operands are __restrict__)
  if (!aligned16(in, out) || !aligned16(w, add)) return FH_EINVAL;  // 16-byte accesses
  fh_batch wt;
  memset(&wt, 0, sizeof(wt));
  wt.nimg = 1, wt.mask[0] = w;
  return hartley_launch(ctx, in, out, planes, nullptr, w != nullptr ? &wt : nullptr, 1, add, add_scale, nullptr,
                        (hipStream_t)stream);
}

int fh_hartley2d(fh_context* ctx, const double* in, double* out, const double* Hc, int planes, void* stream) {
  if (!ctx || !in || !out || !Hc || planes < 1 || planes > 65535) return FH_EINVAL;
  if (!aligned16(out)) return FH_EINVAL;
  if (planes > ctx->planes_max) return FH_ESIZE;
  const int rc = dct_rect_launch(ctx, in, ctx->w0, planes, Hc, Hc, ctx->S, 0, nullptr, 0.0, nullptr, (hipStream_t)stream);
  if (rc) return rc;
  return hartley_launch(ctx, ctx->w0, out, planes, nullptr, nullptr, 0, nullptr, 0.0, nullptr, (hipStream_t)stream);
}

int fh_hartley2d_plan(int S, int planes, int32_t out[15]) {
  if (out == nullptr) return FH_EINVAL;
  memset(out, 0, sizeof(int32_t) * 15);
  const int rc = fh_dct_rect_plan(S, S, planes, 0, out);
  if (rc) return rc;
  const hartley_plan_t pn = hartley_plan(S, planes);
  out[10] = pn.gx, out[11] = pn.gy, out[12] = 1, out[13] = 256, out[14] = (int32_t)pn.lds_bytes;
  return 0;
}

int fh_dct2d(fh_context* ctx, const double* in, double* out, int planes, int inverse, void* stream) {
  if (!ctx || !in || !out || planes < 1) return FH_EINVAL;
  return dct2d_launch(ctx, in, out, planes, inverse, nullptr, (hipStream_t)stream);
}

int fh_dct_moments_u8(fh_context* ctx, const uint8_t* imgs, int n, double* work, double* sum, double* sumsq, void* stream) {
  if (!ctx || !imgs || !work || !sum || !sumsq || n < 1) return FH_EINVAL;
  if (((uintptr_t)imgs & 3) || (((uintptr_t)work | (uintptr_t)sum | (uintptr_t)sumsq) & 15)) return FH_EINVAL;  // vector accesses
  if ((int64_t)3 * n > ctx->planes_max) return FH_ESIZE;
  const hipStream_t st = (hipStream_t)stream;
  const int per = 3 * ctx->S * ctx->S;  // S is even (fh_context_create): per % 4 == 0
  const int64_t quads = (int64_t)n * per / 4;
  hipLaunchKernelGGL(k_u8_to_f64, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, imgs, work, quads);
  FH_LAUNCH_CHECK();
  const int rc = dct2d_launch(ctx, work, work, 3 * n, 0, nullptr, st);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(k_dct_moments, dim3((unsigned)((per / 2 + 255) / 256)), dim3(256), 0, st, (const double*)work, sum, sumsq,
                     per, n);
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_rep_apply(fh_context* ctx, const double* D, const double* r, const double* B, const double* M, int ldm,
                 const double* z, double* out, int64_t d, int m, void* stream) {
  if (!ctx || !D || !z || !out || d < 2) return FH_EINVAL;
  if (m > 0 && (!r || !B || !M || ldm < m)) return FH_EINVAL;
  fh_batch per;
  memset(&per, 0, sizeof(per));
  per.nimg = 1;
  per.D[0] = D, per.r[0] = r, per.B[0] = B, per.M[0] = M;
  return rep_apply_launch(ctx, per, ldm, z, out, d, m, nullptr, (hipStream_t)stream);
}

int fh_rep_apply_batched(fh_context* ctx, const fh_batch* per, int ldm, const double* z, double* out, int64_t d,
                         int m, void* stream) {
  if (!ctx || !per || !z || !out || d < 2 || per->nimg < 1 || per->nimg > FH_MAX_BATCH) return FH_EINVAL;
  for (int i = 0; i < per->nimg; ++i) {
    if (!per->D[i]) return FH_EINVAL;
    if (m > 0 && (!per->r[i] || !per->B[i] || !per->M[i] || ldm < m)) return FH_EINVAL;
  }
  return rep_apply_launch(ctx, *per, ldm, z, out, d, m, nullptr, (hipStream_t)stream);
}

// ---- batched internals: every per-image operand arrives as a PtrTab, vectors of a batch are contiguous [image][d] ----
static inline int gram_pairs(int m) {
  const int ntiles = (m + kGT - 1) / kGT;
  return ntiles * (ntiles + 1) / 2;
}

static int rep_invert_b(fh_context* ctx, int nimg, PtrTab Dx, PtrTab rx, PtrTab B, double shift, PtrTab Dy, PtrTab ry,
                        PtrTab G, int ldg, int64_t d, int m, hipStream_t st) {
  const unsigned Z = (unsigned)nimg;
  // Gram uses the shifted diagonal: apply the shift first, then read Dx
  hipLaunchKernelGGL(k_invert_diag, dim3((unsigned)((d + 255) / 256), 1, Z), dim3(256), 0, st, Dx, rx, shift, Dy, ry, d);
  if (m > 0) {
    const int ntiles = (m + kGT - 1) / kGT;
    const int npairs = gram_pairs(m);
    const int64_t gstride = (int64_t)npairs * kGramRowBlocks * kGT * kGT;
    if (gstride * nimg > ctx->gpartial_elems) return FH_ESIZE;
    hipLaunchKernelGGL(k_gram, dim3(kGramRowBlocks, npairs, Z), dim3(256), 0, st, B, rx, Dx, ctx->gpartial, gstride, d, m, ntiles, 0,
                       0.0);
    hipLaunchKernelGGL(k_gram_reduce, dim3(npairs, kGT * kGT / 64, Z), dim3(256), 0, st, (const double*)ctx->gpartial, gstride,
                       kGramRowBlocks, ntiles, m, G, ldg);
  }
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_rep_invert(fh_context* ctx, double* Dx, const double* rx, const double* B, double shift, double* Dy,
                  double* ry, double* G, int ldg, int64_t d, int m, void* stream) {
  if (!ctx || !Dx || !Dy || d < 1 || m < 0 || m > ctx->m_cap) return FH_EINVAL;
  if (m > 0 && (!rx || !ry || !B || !G || ldg < m)) return FH_EINVAL;
  return rep_invert_b(ctx, 1, tab1(Dx), tab1(rx), tab1(B), shift, tab1(Dy), tab1(ry), tab1(G), ldg, d, m, (hipStream_t)stream);
}

// de <- s2 dm; scal[img][0] = dx.de
static int space_prep_b(fh_context* ctx, int nimg, const double* dm, double s2, const double* dx, double* de, PtrTab scal,
                        int64_t d, hipStream_t st) {
  hipLaunchKernelGGL(k_space_prep, dim3(kDotBlocks, 1, (unsigned)nimg), dim3(256), 0, st, dm, s2, dx, de, ctx->w2,
                     (int64_t)kCgScratch, d);
  hipLaunchKernelGGL(k_scalar_reduce, dim3((unsigned)nimg), dim3(256), 0, st, (const double*)ctx->w2, (int64_t)kCgScratch,
                     kDotBlocks, scal, 0);
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_space_prep(fh_context* ctx, const double* dm, double s2, const double* dx, double* de, double* scal,
                  int64_t d, void* stream) {
  if (!ctx || !dm || !dx || !de || !scal) return FH_EINVAL;
  return space_prep_b(ctx, 1, dm, s2, dx, de, tab1(scal), d, (hipStream_t)stream);
}

// scal[img][slot] = a[img] . b[img]
static int dot_b(fh_context* ctx, int nimg, const double* a, const double* b, PtrTab scal, int slot, int64_t d, hipStream_t st) {
  hipLaunchKernelGGL(k_dot_partial, dim3(kDotBlocks, 1, (unsigned)nimg), dim3(256), 0, st, a, b, (const double*)nullptr,
                     (const double*)nullptr, ctx->w2, d, kCgScratch, (const fh_cg_state*)nullptr);
  hipLaunchKernelGGL(k_scalar_reduce, dim3((unsigned)nimg), dim3(256), 0, st, (const double*)ctx->w2, (int64_t)kCgScratch,
                     kDotBlocks, scal, slot);
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_dot(fh_context* ctx, const double* a, const double* b, double* scal, int slot, int64_t d, void* stream) {
  if (!ctx || !a || !b || !scal || slot < 0) return FH_EINVAL;
  return dot_b(ctx, 1, a, b, tab1(scal), slot, d, (hipStream_t)stream);
}

int fh_space_commit(fh_context* ctx, const double* de, const double* cdx, double gamma, double q, double s2,
                    double* Dc, const double* rc, double* Bc_col0, double* Bc_col1, double* Dh, const double* rh,
                    double* Bh_col0, double* Bh_col1, int project, int64_t d, void* stream) {
  if (!ctx || !de || !cdx || !Dc || !Dh || !Bh_col0 || !Bh_col1) return FH_EINVAL;
  if (!project && (!Bc_col0 || !Bc_col1)) return FH_EINVAL;
  const PtrTab none = tab1(nullptr);
  hipLaunchKernelGGL(k_space_commit, dim3(512), dim3(256), 0, (hipStream_t)stream, de, cdx, gamma, q, s2, tab1(Dc), tab1(rc),
                     tab1(Bc_col0), tab1(Bc_col1), tab1(Dh), tab1(rh), tab1(Bh_col0), tab1(Bh_col1), project, d, 0, none, none, 0,
                     0, none, 0, 0);
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_space_commit_dev(fh_context* ctx, const double* de, const double* cdx, const double* scal, double s2, double* Dc,
                        const double* rc, double* Bc_col0, double* Bc_col1, double* Dh, const double* rh,
                        double* Bh_col0, double* Bh_col1, double* Mc, int ldc, int mc, double* Mh, int ldh, int mh,
                        int project, int64_t d, void* stream) {
  if (!ctx || !de || !cdx || !scal || !Dc || !Dh || !Bh_col0 || !Bh_col1 || !Mh || mh < 0 || ldh < mh + 2) return FH_EINVAL;
  if (!project && (!Bc_col0 || !Bc_col1 || !Mc || mc < 0 || ldc < mc + 2)) return FH_EINVAL;
  hipLaunchKernelGGL(k_space_commit, dim3(512), dim3(256), 0, (hipStream_t)stream, de, cdx, 0.0, 0.0, s2, tab1(Dc), tab1(rc),
                     tab1(Bc_col0), tab1(Bc_col1), tab1(Dh), tab1(rh), tab1(Bh_col0), tab1(Bh_col1), project, d, 1, tab1(scal),
                     tab1(Mc), ldc, mc, tab1(Mh), ldh, mh);
  FH_LAUNCH_CHECK();
  return 0;
}

static int inner_update_b(fh_context* ctx, int nimg, PtrTab Msrc, int ld_src, PtrTab G, int ldg, PtrTab Mdst, int ld_dst, int m,
                          double alpha, double sign, hipStream_t st) {
  if (m == 0) return 0;
  if (m > kWbMax) return FH_ESIZE;  // the caller falls back to its host path
  const size_t lds = ((size_t)m * (2 * m + 1) + 2 * (size_t)m * (m + 1) + (m <= kWbLdsMax ? 3 * (size_t)m * m : 0)) * sizeof(double);
  const int64_t sstride = (int64_t)4 * kWbMax * kWbMax;
  if (ctx->gpartial_elems < sstride * nimg) return FH_ESIZE;
  // ctx->gpartial: the Gram partials were reduced into G before this launch (stream order); free until the next k_gram
  hipLaunchKernelGGL(k_woodbury_inner, dim3((unsigned)nimg), dim3(256), lds, st, Msrc, ld_src, G, ldg, Mdst, ld_dst, m, alpha, sign,
                     ctx->gpartial, sstride);
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_woodbury_inner(fh_context* ctx, const double* Msrc, int ld_src, const double* G, int ldg, double* Mdst, int ld_dst,
                      int m, void* stream) {
  if (!ctx || m < 0 || (m > 0 && (!Msrc || !G || !Mdst || ld_src < m || ldg < m || ld_dst < m))) return FH_EINVAL;
  return inner_update_b(ctx, 1, tab1(Msrc), ld_src, tab1(G), ldg, tab1(Mdst), ld_dst, m, 1.0, -1.0, (hipStream_t)stream);
}

int fh_axpby(double alpha, const double* a, double beta, const double* b, double* out, int64_t n, void* stream) {
  if (!a || !out || n < 1) return FH_EINVAL;
  hipLaunchKernelGGL(k_axpby, dim3(512), dim3(256), 0, (hipStream_t)stream, alpha, a, beta, b, out, n);
  FH_LAUNCH_CHECK();
  return 0;
}

// ---- whole covariance updates (see fh_hip.h): the step-by-step entry points, enqueued from C in covariance.py's order, for
// ONE image (fh_cov_time_update / fh_cov_space_update) or for all images of a lock-step batch in one launch sequence
// (fh_cov_*_update_batched: same kernels with grid z = image, so an image's result does not depend on the batch it is in).
struct CovB {
  int nimg;
  const fh_cov_state* st[FH_MAX_BATCH];
};
enum CovField { F_D, F_R, F_M, F_BC, F_BH, F_G, F_SCAL };
static PtrTab cov_tab(const CovB& cb, CovField f, int rep = 0, int64_t offset = 0) {
  PtrTab t;
  memset(&t, 0, sizeof(t));
  for (int i = 0; i < cb.nimg; ++i) {
    const fh_cov_state* s = cb.st[i];
    double* q = f == F_D ? s->D[rep] : f == F_R ? s->r[rep] : f == F_M ? s->M[rep] : f == F_BC ? s->Bc : f == F_BH ? s->Bh
                : f == F_G ? s->G : s->scal;
    t.p[i] = q ? q + offset : nullptr;
  }
  return t;
}

static int cov_invert_b(fh_context* ctx, const CovB& cb, int src, int dst, CovField base, int m, double shift, hipStream_t sq) {
  const fh_cov_state* s0 = cb.st[0];
  if (m > 0 && s0->ldg < m) return FH_ESIZE;
  int rc = rep_invert_b(ctx, cb.nimg, cov_tab(cb, F_D, src), cov_tab(cb, F_R, src), cov_tab(cb, base), shift, cov_tab(cb, F_D, dst),
                        cov_tab(cb, F_R, dst), cov_tab(cb, F_G), s0->ldg, s0->d, m, sq);
  if (rc) return rc;
  return inner_update_b(ctx, cb.nimg, cov_tab(cb, F_M, src), s0->ldm, cov_tab(cb, F_G), s0->ldg, cov_tab(cb, F_M, dst), s0->ldm, m,
                        1.0, -1.0, sq);
}

// Forward time shift  X <- (X^-1 + s I)^-1  computed from X's OWN representation (online_update_bfgs.py:166-167, 172-173):
//   D' = D / (1 + s D),  r' = r / (1 + s D),  M' = M (I + s G M)^-1  with  G = B^T diag(r^2 / (1 + s D)) B,
// while the inverse representation only moves its diagonal (Dinv += s; its row scale r / D and inner matrix are unchanged).
// Equal to inverting the shifted inverse representation (what the reference does), but I + s G M has the eigenvalues of
// I + s X restricted to the factor span - in [1, (sigma / sigma')^2] for the covariance, [1, 2) for the Hessian - whereas
// the inverse route weights the Gram by 1 / D (1e-4 .. 1e4 with the DCT prior) and loses up to 1e9 of the 1e16.
static int cov_shift_forward_b(fh_context* ctx, const CovB& cb, int fwd, int inv, CovField base, int m, double s, hipStream_t sq) {
  const fh_cov_state* s0 = cb.st[0];
  const int64_t d = s0->d;
  const unsigned Z = (unsigned)cb.nimg;
  if (m > 0) {
    const int ntiles = (m + kGT - 1) / kGT;
    const int npairs = gram_pairs(m);
    const int64_t gstride = (int64_t)npairs * kGramRowBlocks * kGT * kGT;
    if (gstride * cb.nimg > ctx->gpartial_elems || s0->ldg < m) return FH_ESIZE;
    hipLaunchKernelGGL(k_gram, dim3(kGramRowBlocks, npairs, Z), dim3(256), 0, sq, cov_tab(cb, base), cov_tab(cb, F_R, fwd),
                       cov_tab(cb, F_D, fwd), ctx->gpartial, gstride, d, m, ntiles, 1, s);
    hipLaunchKernelGGL(k_gram_reduce, dim3(npairs, kGT * kGT / 64, Z), dim3(256), 0, sq, (const double*)ctx->gpartial, gstride,
                       kGramRowBlocks, ntiles, m, cov_tab(cb, F_G), s0->ldg);
  }
  hipLaunchKernelGGL(k_forward_diag, dim3((unsigned)((d + 255) / 256), 1, Z), dim3(256), 0, sq, cov_tab(cb, F_D, fwd),
                     cov_tab(cb, F_R, fwd), cov_tab(cb, F_D, inv), s, d);
  FH_LAUNCH_CHECK();
  if (m == 0) return 0;
  return inner_update_b(ctx, cb.nimg, cov_tab(cb, F_M, fwd), s0->ldm, cov_tab(cb, F_G), s0->ldg, cov_tab(cb, F_M, fwd), s0->ldm, m, s,
                        1.0, sq);
}

static int cov_fwd_b(fh_context* ctx, const CovB& cb, const double* in, double* out, int inverse, hipStream_t sq) {
  if (cb.st[0]->use_dct) return dct2d_launch(ctx, in, out, 3 * cb.nimg, inverse, nullptr, sq);
  if (in != out) return fh_axpby(1.0, in, 0.0, nullptr, out, cb.st[0]->d * cb.nimg, sq);
  return 0;
}

static fh_batch rep_batch(const CovB& cb, int rep, CovField base) {
  fh_batch per;
  memset(&per, 0, sizeof(per));
  per.nimg = cb.nimg;
  for (int i = 0; i < cb.nimg; ++i) {
    const fh_cov_state* s = cb.st[i];
    per.D[i] = s->D[rep], per.r[i] = s->r[rep], per.B[i] = base == F_BC ? s->Bc : s->Bh, per.M[i] = s->M[rep];
  }
  return per;
}

// the images of a batch must agree on everything that shapes the launch
static int cov_batch_check(fh_context* ctx, const CovB& cb) {
  if (cb.nimg < 1 || cb.nimg > FH_MAX_BATCH || cb.nimg > ctx->nimg_max || 3 * cb.nimg > ctx->planes_max) return FH_ESIZE;
  const fh_cov_state* a = cb.st[0];
  for (int i = 0; i < cb.nimg; ++i) {
    const fh_cov_state* s = cb.st[i];
    if (!s || s->d != a->d || s->m_c != a->m_c || s->m_h != a->m_h || s->ldm != a->ldm || s->ldg != a->ldg ||
        s->project != a->project || s->use_dct != a->use_dct)
      return FH_EINVAL;
  }
  return 0;
}

// x, score, wx, ws, t0, mean_out, score_out: [nimg][d] contiguous
static int time_update_b(fh_context* ctx, const CovB& cb, const double* x, const double* score, double shift_c, double shift_h,
                         double sigma_next2, int only_covariance, double* wx, double* ws, double* t0, double* mean_out,
                         double* score_out, hipStream_t sq) {
  const fh_cov_state* s0 = cb.st[0];
  if (s0->m_c > kWbMax || s0->m_h > kWbMax) return FH_ESIZE;
  const int64_t d = s0->d, dn = d * cb.nimg;
  int rc = cov_shift_forward_b(ctx, cb, 0, 1, F_BC, s0->m_c, shift_c, sq);  // C <- (C^-1 + shift)^-1, C^-1 += shift
  if (rc || only_covariance) return rc;
  if (!x || !score || !wx || !ws || !t0 || !mean_out || !score_out) return FH_EINVAL;
  if ((rc = cov_fwd_b(ctx, cb, x, wx, 0, sq))) return rc;
  if ((rc = cov_fwd_b(ctx, cb, score, ws, 0, sq))) return rc;
  // t0 = H^-1 score with the OLD Hessian, then H <- (H^-1 + shift)^-1, new score = H t0
  if ((rc = rep_apply_launch(ctx, rep_batch(cb, 3, F_BH), s0->ldm, ws, t0, d, s0->m_h, nullptr, sq))) return rc;
  if ((rc = cov_shift_forward_b(ctx, cb, 2, 3, F_BH, s0->m_h, shift_h, sq))) return rc;
  if ((rc = rep_apply_launch(ctx, rep_batch(cb, 2, F_BH), s0->ldm, t0, ws, d, s0->m_h, nullptr, sq))) return rc;
  if ((rc = fh_axpby(1.0, wx, sigma_next2, ws, wx, dn, sq))) return rc;  // mean' = x + s'^2 score'
  if ((rc = cov_fwd_b(ctx, cb, wx, mean_out, 1, sq))) return rc;
  return cov_fwd_b(ctx, cb, ws, score_out, 1, sq);
}

// mean_x, mean_xn, x, xn, dx, de, cdx: [nimg][d] contiguous (dx, de, cdx: scratch)
static int space_update_b(fh_context* ctx, const CovB& cb, const double* mean_x, const double* mean_xn, double s2, const double* x,
                          const double* xn, double* dx, double* de, double* cdx, hipStream_t sq) {
  const fh_cov_state* s0 = cb.st[0];
  if (s0->m_c + 2 > kWbMax || s0->m_h + 2 > kWbMax) return FH_ESIZE;
  const int mc = s0->m_c, mh = s0->m_h, nimg = cb.nimg;
  const int64_t d = s0->d, dn = d * nimg;
  if (s0->ldm < (s0->project ? mc : mc + 2) || s0->ldm < mh + 2) return FH_EINVAL;
  int rc;
  if ((rc = fh_axpby(1.0, xn, -1.0, x, dx, dn, sq))) return rc;
  if ((rc = cov_fwd_b(ctx, cb, dx, dx, 0, sq))) return rc;
  if ((rc = fh_axpby(1.0, mean_xn, -1.0, mean_x, de, dn, sq))) return rc;
  if ((rc = cov_fwd_b(ctx, cb, de, de, 0, sq))) return rc;
  const PtrTab scal = cov_tab(cb, F_SCAL);
  if ((rc = space_prep_b(ctx, nimg, de, s2, dx, de, scal, d, sq))) return rc;  // de <- s2 dm; scal[0] = dx.de
  // two-pass apply also on an exclusive context: the single-sweep kernel keeps c = M t in registers, and the closed-form
  // C^-1 below reads it from ctx->coef
  const int fused_was = ctx->fused_disabled;
  ctx->fused_disabled = 1;
  rc = rep_apply_launch(ctx, rep_batch(cb, 0, F_BC), s0->ldm, dx, cdx, d, mc, nullptr, sq);
  ctx->fused_disabled = fused_was;
  if (rc) return rc;
  if ((rc = dot_b(ctx, nimg, cdx, dx, scal, 1, d, sq))) return rc;  // scal[1] = dx.(C dx)
  if (!s0->project && mc > 0)  // c = M t of that apply (ctx->coef) is needed after the next dots pass overwrites it
    hipLaunchKernelGGL(k_copy_small, dim3((unsigned)nimg), dim3(256), 0, sq, (const double*)ctx->coef, (int64_t)2 * FH_MAX_COLS,
                       cov_tab(cb, F_G), mc);
  const PtrTab none = tab1(nullptr);
  hipLaunchKernelGGL(k_space_commit, dim3(512, 1, (unsigned)nimg), dim3(256), 0, sq, (const double*)de, (const double*)cdx, 0.0, 0.0,
                     s2, cov_tab(cb, F_D, 0), cov_tab(cb, F_R, 0), s0->project ? none : cov_tab(cb, F_BC, 0, (int64_t)mc * d),
                     s0->project ? none : cov_tab(cb, F_BC, 0, (int64_t)(mc + 1) * d), cov_tab(cb, F_D, 2), cov_tab(cb, F_R, 2),
                     cov_tab(cb, F_BH, 0, (int64_t)mh * d), cov_tab(cb, F_BH, 0, (int64_t)(mh + 1) * d), s0->project, d, 1, scal,
                     cov_tab(cb, F_M, 0), s0->ldm, mc, cov_tab(cb, F_M, 2), s0->ldm, mh);
  FH_LAUNCH_CHECK();
  const int mh2 = mh + 2;
  if (s0->project) {
    // the pair went into the diagonal: C^-1 over the unchanged columns by Woodbury
    if ((rc = cov_invert_b(ctx, cb, 0, 1, F_BC, mc, 0.0, sq))) return rc;
  } else {
    // C^-1 in closed form (k_bfgs_inverse_commit): cC = M t saved above; s = Wi^T de and Mi s from a dots pass over the
    // old columns with the inverse representation's row scale; de^T D^-1 de from one more reduction
    if (mc > 0 && (rc = rep_apply_launch(ctx, rep_batch(cb, 1, F_BC), s0->ldm, de, nullptr, d, mc, nullptr, sq))) return rc;
    hipLaunchKernelGGL(k_wnorm_partial, dim3(kDotBlocks, 1, (unsigned)nimg), dim3(256), 0, sq, (const double*)de, cov_tab(cb, F_D, 1),
                       ctx->w2, (int64_t)kCgScratch, d);
    hipLaunchKernelGGL(k_scalar_reduce, dim3((unsigned)nimg), dim3(256), 0, sq, (const double*)ctx->w2, (int64_t)kCgScratch,
                       kDotBlocks, scal, 2);
    hipLaunchKernelGGL(k_bfgs_inverse_commit, dim3((unsigned)nimg), dim3(256), 0, sq, scal, cov_tab(cb, F_G), (const double*)ctx->coef,
                       (int64_t)2 * FH_MAX_COLS, cov_tab(cb, F_M, 1), s0->ldm, mc);
    FH_LAUNCH_CHECK();
  }
  return cov_invert_b(ctx, cb, 2, 3, F_BH, mh2, 0.0, sq);  // H^-1 (its diagonal was re-derived from C: full Woodbury)
}

int fh_cov_time_update(fh_context* ctx, const fh_cov_state* st, const double* x, const double* score, double shift_c,
                       double shift_h, double sigma_next2, int only_covariance, double* wx, double* ws,
                       double* mean_out, double* score_out, void* stream) {
  if (!ctx || !st) return FH_EINVAL;
  CovB cb;
  cb.nimg = 1, cb.st[0] = st;
  return time_update_b(ctx, cb, x, score, shift_c, shift_h, sigma_next2, only_covariance, wx, ws, st->t0, mean_out, score_out,
                       (hipStream_t)stream);
}

int fh_cov_space_update(fh_context* ctx, const fh_cov_state* st, const double* mean_x, const double* mean_xn, double s2,
                        const double* x, const double* xn, void* stream) {
  if (!ctx || !st || !mean_x || !mean_xn || !x || !xn) return FH_EINVAL;
  CovB cb;
  cb.nimg = 1, cb.st[0] = st;
  return space_update_b(ctx, cb, mean_x, mean_xn, s2, x, xn, st->t0, st->t1, st->t2, (hipStream_t)stream);
}

int fh_cov_time_update_batched(fh_context* ctx, int nimg, const fh_cov_state* sts, const double* x, const double* score,
                               double shift_c, double shift_h, double sigma_next2, double* work, double* mean_out,
                               double* score_out, void* stream) {
  if (!ctx || !sts || !x || !score || !work || !mean_out || !score_out || nimg < 1 || nimg > FH_MAX_BATCH) return FH_EINVAL;
  CovB cb;
  cb.nimg = nimg;
  for (int i = 0; i < nimg; ++i) cb.st[i] = sts + i;
  int rc = cov_batch_check(ctx, cb);
  if (rc) return rc;
  const int64_t dn = sts[0].d * nimg;
  return time_update_b(ctx, cb, x, score, shift_c, shift_h, sigma_next2, 0, work, work + dn, work + 2 * dn, mean_out, score_out,
                       (hipStream_t)stream);
}

int fh_cov_space_update_batched(fh_context* ctx, int nimg, const fh_cov_state* sts, const double* mean_x, const double* mean_xn,
                                double s2, const double* x, const double* xn, double* work, void* stream) {
  if (!ctx || !sts || !mean_x || !mean_xn || !x || !xn || !work || nimg < 1 || nimg > FH_MAX_BATCH) return FH_EINVAL;
  CovB cb;
  cb.nimg = nimg;
  for (int i = 0; i < nimg; ++i) cb.st[i] = sts + i;
  int rc = cov_batch_check(ctx, cb);
  if (rc) return rc;
  const int64_t dn = sts[0].d * nimg;
  return space_update_b(ctx, cb, mean_x, mean_xn, s2, x, xn, work, work + dn, work + 2 * dn, (hipStream_t)stream);
}

int fh_read_scalars(fh_context* ctx, const double* scal, double* out_host, int k, void* stream) {
  if (!ctx || !scal || !out_host || k < 1 || k > 64) return FH_EINVAL;
  FH_CHECK(hipMemcpyAsync(ctx->h_scal, scal, sizeof(double) * k, hipMemcpyDeviceToHost, (hipStream_t)stream));
  FH_CHECK(hipStreamSynchronize((hipStream_t)stream));
  memcpy(out_host, ctx->h_scal, sizeof(double) * k);
  return 0;
}

int fh_conv_circ(fh_context* ctx, const double* in, double* out, const int32_t* dy, const int32_t* dx,
                 const double* w, int ntaps, int halo, int planes, int stride, int adjoint, void* stream) {
  if (!ctx || !in || !out || !dy || !dx || !w || ntaps < 1 || planes < 1) return FH_EINVAL;
  return conv_launch(ctx, in, out, dy, dx, w, ntaps, halo, planes, stride, adjoint, nullptr, 0.0, nullptr,
                     (hipStream_t)stream);
}

int fh_conv_circ_plan(int S, int ntaps, int halo, int planes, int stride, int adjoint, int32_t out[6]) {
  if (out == nullptr) return FH_EINVAL;
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (S < 2 || S > 256 || (S & 1) || ntaps < 1 || planes < 1) return FH_EINVAL;  // as fh_context_create / fh_conv_circ
  conv_choice c;
  const int rc = conv_plan_halo(S, ntaps, halo, planes, stride, adjoint, &c);
  if (rc) return rc;
  const int32_t v[6] = {c.kernel, (int32_t)c.grid.x, (int32_t)c.grid.y, (int32_t)c.grid.z, 256, (int32_t)c.lds};
  memcpy(out, v, sizeof(v));
  return 0;
}

int fh_conv_frames(fh_context* ctx, const double* in, double* out, const int32_t* dy, const int32_t* dx, const double* w,
                   const int32_t* frame_off, int nframes, int max_frame_taps, int halo, int planes, int stride, int adjoint,
                   void* stream) {
  if (!ctx || !in || !out || !dy || !dx || !w || !frame_off || in == out) return FH_EINVAL;
  frames_choice c;
  int rc = frames_plan(ctx->S, nframes, max_frame_taps, halo, planes, stride, adjoint, &c);  // every argument, before the copy below
  if (rc) return rc;
  if (planes > ctx->planes_max) return FH_ESIZE;
  int ntaps = -1;  // the total tap count is the last offset: one read of all K + 1
  rc = frames_prepare(ctx, frame_off, nframes, &ntaps, max_frame_taps, (hipStream_t)stream);
  if (rc) return rc;
  return frames_launch(ctx, in, out, dy, dx, w, frame_off, ntaps, nframes, max_frame_taps, halo, planes, stride, adjoint, nullptr,
                       0.0, nullptr, (hipStream_t)stream);
}

int fh_conv_frames_plan(int S, int nframes, int max_frame_taps, int halo, int planes, int stride, int adjoint, int32_t out[6]) {
  if (out == nullptr) return FH_EINVAL;
  for (int i = 0; i < 6; ++i) out[i] = 0;
  frames_choice c;
  const int rc = frames_plan(S, nframes, max_frame_taps, halo, planes, stride, adjoint, &c);
  if (rc) return rc;
  const int32_t v[6] = {c.fused, (int32_t)c.grid.x, (int32_t)c.grid.y, (int32_t)c.grid.z, 256, (int32_t)c.lds};
  memcpy(out, v, sizeof(v));
  return 0;
}

int fh_conv_blend(fh_context* ctx, const double* in, double* out, const int32_t* dy, const int32_t* dx, const double* w,
                  const int32_t* frame_off, int nframes, int max_frame_taps, int halo, const double* blend, int planes,
                  int adjoint, void* stream) {
  if (!ctx || !in || !out || !dy || !dx || !w || !frame_off || !blend || in == out) return FH_EINVAL;
  blend_choice c;
  int rc = blend_plan(ctx->S, nframes, max_frame_taps, halo, planes, adjoint, &c);  // every argument, before the copy below
  if (rc) return rc;
  if (planes > ctx->planes_max) return FH_ESIZE;
  if (planes / 3 > FH_MAX_BATCH) return FH_EINVAL;
  int ntaps = -1;  // the total tap count is the last offset: one read of all K + 1
  rc = frames_prepare(ctx, frame_off, nframes, &ntaps, max_frame_taps, (hipStream_t)stream);
  if (rc) return rc;
  return blend_launch(ctx, in, out, dy, dx, w, frame_off, ntaps, nframes, max_frame_taps, halo, planes, adjoint, blend, nullptr,
                      0.0, nullptr, (hipStream_t)stream, ctx->w0);  // (a work vector, idle outside fh_amm / a solve)
}

int fh_conv_blend_plan(int S, int nframes, int max_frame_taps, int halo, int planes, int adjoint, int32_t out[6]) {
  if (out == nullptr) return FH_EINVAL;
  for (int i = 0; i < 6; ++i) out[i] = 0;
  blend_choice c;
  const int rc = blend_plan(S, nframes, max_frame_taps, halo, planes, adjoint, &c);
  if (rc) return rc;
  const int32_t v[6] = {1, (int32_t)c.grid.x, (int32_t)c.grid.y, (int32_t)c.grid.z, 256, (int32_t)c.lds};
  memcpy(out, v, sizeof(v));
  return 0;
}

int fh_conv_window(fh_context* ctx, const double* in, double* out, const double* win, int hy, int hx, int planes, int adjoint,
                   void* stream) {
  if (!ctx || !in || !out || !win || in == out) return FH_EINVAL;
  return window_launch(ctx, in, out, win, hy, hx, planes, adjoint, nullptr, 0.0, nullptr, (hipStream_t)stream);
}

int fh_conv_window_plan(int S, int hy, int hx, int planes, int32_t out[5]) {
  if (out == nullptr) return FH_EINVAL;
  for (int i = 0; i < 5; ++i) out[i] = 0;
  dim3 grid;
  size_t lds;
  const int rc = window_plan(S, hy, hx, planes, &grid, &lds);
  if (rc) return rc;
  const int32_t v[5] = {(int32_t)grid.x, (int32_t)grid.y, (int32_t)grid.z, 256, (int32_t)lds};
  memcpy(out, v, sizeof(v));
  return 0;
}

int fh_channel_mix(fh_context* ctx, const double* in, double* out, const double* w, int nimg, int adjoint, void* stream) {
  if (!ctx || !in || !out || !w || nimg < 1 || (ctx->S & 1)) return FH_EINVAL;
  if (((uintptr_t)in | (uintptr_t)out) & 15) return FH_EINVAL;  // 16-byte accesses
  if (nimg > 65535) return FH_ESIZE;                            // the image is grid dimension z
  const int64_t pairs = (int64_t)ctx->S * ctx->S / 2;
  const dim3 grid((unsigned)((pairs + 255) / 256), 1, (unsigned)nimg);
  if (adjoint)
    hipLaunchKernelGGL(k_channel_mix<true>, grid, dim3(256), 0, (hipStream_t)stream, in, out, w, pairs, (const double*)nullptr,
                       0.0, (const fh_cg_state*)nullptr);
  else
    hipLaunchKernelGGL(k_channel_mix<false>, grid, dim3(256), 0, (hipStream_t)stream, in, out, w, pairs, (const double*)nullptr,
                       0.0, (const fh_cg_state*)nullptr);
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_amm(fh_context* ctx, const fh_problem* p, const double* u, double* out, void* stream) {
  if (!ctx || !p || !u || !out) return FH_EINVAL;
  const fh_batch per = batch_of(p);
  int64_t n;          // (the measurement's length: not needed here)
  const double* uin;  // u times the op's mask / weights, or null
  const int rc = amm_prologue(ctx, p, per, ENTRY_AMM, u, out, (hipStream_t)stream, &n, &uin);
  if (rc) return rc;
  return amm_launch(ctx, p, per, u, out, nullptr, (hipStream_t)stream, nullptr, nullptr, uin);
}

// One chunk of CG iterations for all images of the batch, enqueued on `st` (eagerly, or while the stream is being
// captured into a graph).
static int cg_enqueue_chunk(fh_context* ctx, const fh_problem* p, const fh_batch& per, int64_t n, int count,
                            hipStream_t st) {
  double *x = ctx->cg_x, *r = ctx->cg_r, *pk = ctx->cg_p, *ap = ctx->cg_ap;
  double* part = ctx->w2;
  double* rzbuf = ctx->w2 + 4 * kDotBlocks;
  fh_cg_state* stt = ctx->cg_state;
  const dim3 grid(kCgBlocks, 1, (unsigned)per.nimg);
  const bool weighted = cg_keeps_wp(p);  // the operator reads W p, which k_cg_step2_w leaves in cg_wp beside p
  const fh_diag_tab wt = weights_tab(per);
  for (int i = 0; i < count; ++i) {
    int dot_n = 0;  // > 0: the operator's last pass already left the p.Ap block partials
    int rc = amm_launch(ctx, p, per, pk, ap, stt, st, part, &dot_n, weighted ? ctx->cg_wp : nullptr);
    if (rc) return rc;
    if (dot_n == 0) {
      hipLaunchKernelGGL(k_dot_partial, grid, dim3(256), 0, st, (const double*)pk, (const double*)ap,
                         (const double*)nullptr, (const double*)nullptr, part, n, kCgScratch, (const fh_cg_state*)stt);
      dot_n = kCgBlocks;
    }
    hipLaunchKernelGGL(k_cg_step1, grid, dim3(256), 0, st, (const double*)pk, (const double*)ap, x, r,
                       (const double*)part, dot_n, part + 2 * kDotBlocks, (const double*)rzbuf, stt, n);
    if (weighted)
      hipLaunchKernelGGL(k_cg_step2_w, grid, dim3(256), 0, st, (const double*)r, pk, (const double*)(part + 2 * kDotBlocks),
                         kCgBlocks, rzbuf, stt, n, wt, ctx->cg_wp);
    else
      hipLaunchKernelGGL(k_cg_step2, grid, dim3(256), 0, st, (const double*)r, pk,
                         (const double*)(part + 2 * kDotBlocks), kCgBlocks, rzbuf, stt, n);
  }
  return 0;
}

// The iteration body depends on device state only (counter, scalars, done flag), so a chunk is captured once per
// (problem, pointers, m) into a hipGraph and replayed: one host call per 8 iterations instead of ~110 launches.
static hipGraphExec_t cg_graph_for(fh_context* ctx, const fh_problem* p, const fh_batch& per, int64_t n, int chunk,
                                   hipStream_t st) {
  if (ctx->graphs_disabled) return nullptr;
  if (getenv("FH_NO_GRAPH") != nullptr) return nullptr;  // A/B switch for profiling
  ++ctx->graph_clock;
  // ops 12 / 13: the chain route bakes host-sliced tap pointers and counts into the graph, so the route switch and the offsets
  // that frames_prepare has just checked (ctx->frame_off) belong to the key; other ops never read the switch.  (The weights'
  // pointers of op 13 are part of bkey, like those of ops 8 .. 11; their values are read by the kernels at every replay.)
  bool (*const route)() = facts(p).graph_route;  // op 14: the same, with its own switch (FH_BLEND_FUSED)
  const bool offsets_op = route != nullptr;
  const int frames_route = offsets_op ? (int)route() : 0;
  fh_graph_entry* slot = &ctx->graphs[0];
  for (auto& g : ctx->graphs) {
    if (g.exec != nullptr && g.n == n && memcmp(&g.key, p, sizeof(fh_problem)) == 0 &&
        (!offsets_op || (g.frames_fused == frames_route && memcmp(g.frame_off, ctx->frame_off, sizeof(g.frame_off)) == 0)) &&
        memcmp(&g.bkey, &per, sizeof(fh_batch)) == 0) {
      g.stamp = ctx->graph_clock;
      return g.exec;
    }
    if (g.stamp < slot->stamp) slot = &g;
  }
  if (slot->exec != nullptr) {
    (void)hipGraphExecDestroy(slot->exec);
    (void)hipGraphDestroy(slot->graph);
    slot->exec = nullptr;
  }
  // A capture is short (80 launches) but must not overlap, in another host thread of the process, with the legacy-stream
  // copies and allocations of fh_context_create / fh_context_destroy (a second lock-step group creating its contexts):
  // the capture is invalidated (hipErrorStreamCaptureInvalidated in this thread) or the other call fails
  // (hipErrorStreamCaptureImplicit).  g_capture_mu serialises the two.
  std::lock_guard<std::mutex> capture_lock(g_capture_mu);
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    ctx->graphs_disabled = 1;  // e.g. the legacy null stream: stay on eager launches
    return nullptr;
  }
  const int rc = cg_enqueue_chunk(ctx, p, per, n, chunk, st);
  hipGraph_t graph = nullptr;
  const hipError_t e = hipStreamEndCapture(st, &graph);
  if (rc != 0 || e != hipSuccess || graph == nullptr) {
    (void)hipGetLastError();
    if (graph) (void)hipGraphDestroy(graph);
    ctx->graphs_disabled = 1;
    return nullptr;
  }
  hipGraphExec_t exec = nullptr;
  if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipGraphDestroy(graph);
    ctx->graphs_disabled = 1;
    return nullptr;
  }
  memcpy(&slot->key, p, sizeof(fh_problem));
  memcpy(&slot->bkey, &per, sizeof(fh_batch));
  slot->n = n;
  slot->frames_fused = frames_route;
  memcpy(slot->frame_off, ctx->frame_off, sizeof(slot->frame_off));
  slot->exec = exec;
  slot->graph = graph;
  slot->stamp = ctx->graph_clock;
  return exec;
}

int fh_cg_solve_batched(fh_context* ctx, const fh_problem* p, const fh_batch* perp, const double* b, double* x,
                        const double* rtol_host, double atol, int maxiter, fh_cg_info* info, void* stream) {
  if (!ctx || !p || !perp || !b || !x || !rtol_host || !info || maxiter < 1) return FH_EINVAL;
  const fh_batch& per = *perp;
  const int nimg = per.nimg;
  if (nimg < 1 || nimg > ctx->nimg_max || nimg > FH_MAX_BATCH) return FH_ESIZE;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < nimg; ++i)
    if (!(rtol_host[i] > 0 || atol > 0)) return FH_EINVAL;
  int64_t n;  // per image (colorization: one plane, ops 12 / 13: 3 K)
  const double* uin;
  int rc = amm_prologue(ctx, p, per, ENTRY_SOLVE, b, x, st, &n, &uin);
  if (rc) return rc;
  double *r = ctx->cg_r, *pk = ctx->cg_p, *ap = ctx->cg_ap;
  double* part = ctx->w2;                      // per image: [0,256) pAp / init r.r ; [256,512) init b.b ; [512,768) r.r
  double* rzbuf = ctx->w2 + 4 * kDotBlocks;    // per image: [2]
  fh_cg_state* stt = ctx->cg_state;
  RtolArr rt;
  for (int i = 0; i < FH_MAX_BATCH; ++i) rt.v[i] = i < nimg ? rtol_host[i] : 1.0;
  const bool masked = facts(p).mask == MASK_VALID;  // the system is solved for M b, which amm_prologue has left in cg_x
  if (!p->cg_scipy) {  // A x0 with x0 = b
    rc = masked ? amm_launch(ctx, p, per, uin, ap, nullptr, st)
                : amm_launch(ctx, p, per, b, ap, nullptr, st, nullptr, nullptr, uin);
    if (rc) return rc;
  }
  if (masked) {  // (the first apply has released the work vectors)
    hipLaunchKernelGGL(k_mask, dim3(512, 1, (unsigned)nimg), dim3(256), 0, st, per, b, (const double*)nullptr, 0.0, ctx->w0, n,
                       (const fh_cg_state*)nullptr);
    b = ctx->w0;
  }
  const dim3 grid(kCgBlocks, 1, (unsigned)nimg);
  if (cg_keeps_wp(p))
    hipLaunchKernelGGL(k_cg_init_w, grid, dim3(256), 0, st, b, p->cg_scipy ? (const double*)nullptr : (const double*)ap,
                       ctx->cg_x, r, pk, part, n, weights_tab(per), ctx->cg_wp);
  else
    hipLaunchKernelGGL(k_cg_init, grid, dim3(256), 0, st, b, p->cg_scipy ? (const double*)nullptr : (const double*)ap, ctx->cg_x,
                       r, pk, part, n);
  hipLaunchKernelGGL(k_cg_init_fin, dim3(1, 1, (unsigned)nimg), dim3(256), 0, st, (const double*)part, kCgBlocks, rt,
                     atol, maxiter, stt, rzbuf, (int)p->cg_scipy);
  const int chunk = 8;
  hipGraphExec_t exec = cg_graph_for(ctx, p, per, n, chunk, st);
  fh_cg_state* h = ctx->h_state;  // pinned: the periodic read-back is a true async copy
  memset(h, 0, sizeof(fh_cg_state) * nimg);
  bool all_done = false;
  for (int launched = 0; launched < maxiter + chunk && !all_done; launched += chunk) {
    if (exec != nullptr) {
      FH_CHECK(hipGraphLaunch(exec, st));
    } else {
      rc = cg_enqueue_chunk(ctx, p, per, n, chunk, st);
      if (rc) return rc;
    }
    FH_CHECK(hipMemcpyAsync(h, stt, sizeof(fh_cg_state) * nimg, hipMemcpyDeviceToHost, st));
    FH_CHECK(hipStreamSynchronize(st));
    all_done = true;
    for (int i = 0; i < nimg; ++i) all_done = all_done && h[i].done != 0;
  }
  FH_CHECK(hipMemcpyAsync(x, ctx->cg_x, sizeof(double) * n * nimg, hipMemcpyDeviceToDevice, st));
  FH_LAUNCH_CHECK();
  for (int i = 0; i < nimg; ++i) {
    info[i].niter = (h[i].done == 1 || h[i].done == 2) ? h[i].niter : maxiter;
    info[i].optimal = h[i].optimal;
    info[i].residual_norm = h[i].rnorm;
    info[i].b_norm = h[i].bnorm;
  }
  return 0;
}

int fh_cg_solve(fh_context* ctx, const fh_problem* p, const double* b, double* x, double rtol, double atol,
                int maxiter, fh_cg_info* info, void* stream) {
  if (!p) return FH_EINVAL;
  const fh_batch per = batch_of(p);
  return fh_cg_solve_batched(ctx, p, &per, b, x, &rtol, atol, maxiter, info, stream);
}

}  // extern "C"

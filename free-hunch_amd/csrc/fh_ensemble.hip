// Posterior ensembles (free-hunch_amd/ensemble.py): K samples of ONE measurement -> mean image, per-pixel standard deviation and
// the calibration sums.  x [N][K][n] float64 in the sampler's units; everything below is in 8-bit units.
//   k_ensemble_stats : per element v_k = clip(127.5 x_k + 127.5, 0, 255); m = (((v_0 + v_1) + v_2) + ...) / K and, in a second
//                      pass over the members, SS = sum_k (v_k - m)^2, both in member order; mean_u8 = floor(m + 0.5),
//                      std = fl32(sqrt(SS / (K - 1))).  With a truth image t: d2 = (t - m)^2, and the element is covered at c
//                      sigma when d2 K (K - 1) <= c^2 SS (K + 1) - the truth as a (K + 1)-th draw has variance s^2 (1 + 1/K);
//                      no division, no square root.  A workgroup owns a fixed chunk of kChunk elements of ONE ensemble and
//                      writes (sum SS / (K - 1), sum d2, covered at 1 sigma, covered at 2 sigma) into slot [ensemble][chunk];
//                      the chunking depends on n only.  A thread owns pairs of neighbouring elements: with n even (and x 16-byte
//                      aligned) a pair is one 16-byte load per member, else two scalar loads - the same elements in the same
//                      order either way, so both routes give the same bits.
//   k_ensemble_final : per ensemble, the chunk partials in index order -> out[e] = (mean SS / (K - 1), mean d2, covered
//                      fractions at 1 and 2 sigma), the last three -1 without a truth.  No atomics anywhere: an ensemble's
//                      numbers are bitwise the same at any N and at any position in the batch.
// No contraction: the numpy restatement (tests/_ensemble_restatement.py) rounds every product before the sum it feeds.
#include "fh_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPairsPerThread = 4;
constexpr int kChunk = 256 * 2 * kPairsPerThread;  // elements per workgroup
constexpr int kMaxMembers = 64;

__device__ __forceinline__ double to_u8_units(double x) {
  const double t = 127.5 * x;
  return fmin(fmax(t + 127.5, 0.0), 255.0);
}

struct Acc {
  double spread, skill, c1, c2;
};

// W neighbouring elements from `at` on: W = 2 reads a member's pair with one 16-byte load, W = 1 with a scalar load
template <int W>
__device__ __forceinline__ void elements(const double* __restrict__ xe, int K, int n, const uint8_t* __restrict__ te, int64_t at,
                                         uint8_t* __restrict__ mean_u8, float* __restrict__ sd, Acc& a) {
  auto load = [&](int k, double v[W]) {
    const double* src = xe + (int64_t)k * n + at;
    if (W == 2) {
      const double2 t = *reinterpret_cast<const double2*>(src);
      v[0] = to_u8_units(t.x), v[W - 1] = to_u8_units(t.y);
    } else {
      v[0] = to_u8_units(*src);
    }
  };
  double s[W], v[W], m[W], ss[W];
  load(0, s);
  for (int k = 1; k < K; ++k) {
    load(k, v);
#pragma unroll
    for (int i = 0; i < W; ++i) s[i] = s[i] + v[i];
  }
  const double Kd = (double)K, Km1 = (double)(K - 1), Kp1 = (double)(K + 1);
#pragma unroll
  for (int i = 0; i < W; ++i) m[i] = s[i] / Kd, ss[i] = 0.0;
  for (int k = 0; k < K; ++k) {  // second pass over the members (they come from the cache)
    load(k, v);
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const double d = v[i] - m[i];
      const double q = d * d;
      ss[i] = ss[i] + q;
    }
  }
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const double var = ss[i] / Km1;
    mean_u8[at + i] = (uint8_t)floor(m[i] + 0.5);
    sd[at + i] = (float)sqrt(var);
    a.spread = a.spread + var;
    if (te) {
      const double e = (double)te[at + i] - m[i];
      const double d2 = e * e;
      const double lhs = (d2 * Kd) * Km1;
      a.skill = a.skill + d2;
      a.c1 = a.c1 + (lhs <= (1.0 * ss[i]) * Kp1 ? 1.0 : 0.0);
      a.c2 = a.c2 + (lhs <= (4.0 * ss[i]) * Kp1 ? 1.0 : 0.0);
    }
  }
}

// grid (chunks, N); partial [N][chunks][4].  VEC: n even and x 16-byte aligned, so every pair is whole and aligned
template <bool VEC>
__global__ __launch_bounds__(256) void k_ensemble_stats(const double* __restrict__ x, const uint8_t* __restrict__ truth, int K,
                                                        int n, uint8_t* __restrict__ mean_u8, float* __restrict__ sd,
                                                        double* __restrict__ partial) {
  __shared__ double red[4];
  const int64_t e = blockIdx.y;
  const double* xe = x + e * K * (int64_t)n;
  const int64_t img = e * (int64_t)n;
  const uint8_t* te = truth ? truth + img : nullptr;
  const int64_t base = (int64_t)blockIdx.x * kChunk;
  Acc a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int j = 0; j < kPairsPerThread; ++j) {
    const int64_t p = base + (int64_t)j * 512 + 2 * threadIdx.x;  // first element of the pair
    if (p >= n) continue;
    if (VEC) {
      elements<2>(xe, K, n, te, p, mean_u8 + img, sd + img, a);
    } else {
      elements<1>(xe, K, n, te, p, mean_u8 + img, sd + img, a);
      if (p + 1 < n) elements<1>(xe, K, n, te, p + 1, mean_u8 + img, sd + img, a);
    }
  }
  a.spread = fh::block_sum_256(a.spread, red);
  a.skill = fh::block_sum_256(a.skill, red);
  a.c1 = fh::block_sum_256(a.c1, red);
  a.c2 = fh::block_sum_256(a.c2, red);
  if (threadIdx.x == 0) {
    double* dst = partial + (e * gridDim.x + blockIdx.x) * 4;
    dst[0] = a.spread, dst[1] = a.skill, dst[2] = a.c1, dst[3] = a.c2;
  }
}

// grid (N); thread t adds chunks t, t + 256, ... in that order, then the fixed block tree
__global__ __launch_bounds__(256) void k_ensemble_final(const double* __restrict__ partial, int chunks, int n, int has_truth,
                                                        double* __restrict__ out) {
  __shared__ double red[4];
  const int64_t e = blockIdx.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = threadIdx.x; c < chunks; c += 256) {
    const double* p = partial + (e * chunks + c) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = s[i] + p[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = fh::block_sum_256(s[i], red);
  if (threadIdx.x == 0) {
    const double nd = (double)n;
    out[e * 4 + 0] = s[0] / nd;
#pragma unroll
    for (int i = 1; i < 4; ++i) out[e * 4 + i] = has_truth ? s[i] / nd : -1.0;
  }
}

inline int64_t chunks_of(int n) { return ((int64_t)n + kChunk - 1) / kChunk; }

}  // namespace

extern "C" {

int64_t fh_ensemble_scratch_doubles(int N, int n) { return N < 1 || n < 1 ? 0 : (int64_t)N * chunks_of(n) * 4; }

int fh_ensemble_stats(const double* x, const uint8_t* truth, int N, int K, int n, uint8_t* mean_u8, float* std, double* scratch,
                      double* out, void* stream) {
  if (!x || !mean_u8 || !std || !scratch || !out || N < 1 || n < 1 || K < 2 || K > kMaxMembers) return FH_EINVAL;
  if (N > 65535) return FH_ESIZE;  // the ensemble is grid dimension y (the chunks of an int n always fit dimension x)
  const int chunks = (int)chunks_of(n);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = n % 2 == 0 && ((uintptr_t)x & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(k_ensemble_stats<true>, dim3(chunks, N), dim3(256), 0, st, x, truth, K, n, mean_u8, std, scratch);
  else
    hipLaunchKernelGGL(k_ensemble_stats<false>, dim3(chunks, N), dim3(256), 0, st, x, truth, K, n, mean_u8, std, scratch);
  FH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ensemble_final, dim3(N), dim3(256), 0, st, (const double*)scratch, chunks, n, truth ? 1 : 0, out);
  FH_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

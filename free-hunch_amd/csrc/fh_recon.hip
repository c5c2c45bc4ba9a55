// The per-sigma denoiser-error table (free-hunch_amd/recon_mse.py): the two streaming kernels around the UNet call.
//   k_noisy_u8     : uint8 NCHW -> float32 x_t = fl32((double)x32 + sigma * eps), x32 = u8 / 127.5 - 1 in float32 (the sampler's
//                    StandardRGBEncoder).  eps is Philox4x32-10 keyed by the seed, counter (quad inside the image, image index
//                    in the listing, level, 0), mapped to four normals by Box-Muller in float64: the noise of one
//                    (seed, image, level, element) does not depend on the batch, the call order or the world size.  One thread
//                    owns four consecutive elements: one 4-byte load, one 16-byte store.
//   k_sqerr_u8     : sum ((double)D - (double)x32)^2 per image.  A workgroup owns a fixed chunk of kChunkQuads quads of ONE
//                    image and writes one partial into slot [image][chunk]; the chunking depends on S only.
//   k_sqerr_final  : per image, the chunk partials in index order.  No atomics anywhere: an image's sum is bitwise the same at
//                    any batch size and any position in the batch.
#include "fh_common.h"

namespace {

constexpr int kNoisyImgs = 16;                 // images per launch of k_noisy_u8 (their indices travel as kernel arguments)
constexpr int kQuadsPerThread = 4;
constexpr int kChunkQuads = 256 * kQuadsPerThread;  // quads (of 4 elements) per workgroup of k_sqerr_u8

struct NoisyIdx {
  uint32_t v[kNoisyImgs];
};

__device__ __forceinline__ float x32_of(uint32_t u8) { return (float)u8 / 127.5f - 1.0f; }

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t r[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, double& z0, double& z1) {
  const double ua = ((double)ra + 0.5) * 0x1p-32, ub = ((double)rb + 0.5) * 0x1p-32;  // in (0, 1): the logarithm is finite
  const double rad = sqrt(-2.0 * log(ua));
  double s, c;
  sincos(6.283185307179586 * ub, &s, &c);
  z0 = rad * c;
  z1 = rad * s;
}

// the sum in float64 with the product rounded first, then ONE rounding to float32 (no fused multiply-add: the host
// restatement rounds sigma * eps)
__device__ __forceinline__ float noisy(float x, double sigma, double eps) {
#pragma clang fp contract(off)
  const double t = sigma * eps;
  return (float)((double)x + t);
}

// imgs [n][Q] packed quads, out [n][Q] float4; blockIdx.y = image of this launch
__global__ __launch_bounds__(256) void k_noisy_u8(const uint32_t* __restrict__ imgs, NoisyIdx idx, int64_t Q, double sigma,
                                                  uint32_t level, uint32_t k0, uint32_t k1, float4* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const int b = blockIdx.y;
  const uint32_t px = imgs[(int64_t)b * Q + q];
  uint32_t r[4];
  philox4x32_10((uint32_t)q, idx.v[b], level, 0u, k0, k1, r);
  double z0, z1, z2, z3;
  box_muller(r[0], r[1], z0, z1);
  box_muller(r[2], r[3], z2, z3);
  float4 o;
  o.x = noisy(x32_of(px & 0xffu), sigma, z0);
  o.y = noisy(x32_of((px >> 8) & 0xffu), sigma, z1);
  o.z = noisy(x32_of((px >> 16) & 0xffu), sigma, z2);
  o.w = noisy(x32_of(px >> 24), sigma, z3);
  out[(int64_t)b * Q + q] = o;
}

// grid (chunks, n); partial [n][chunks]
__global__ __launch_bounds__(256) void k_sqerr_u8(const float4* __restrict__ D, const uint32_t* __restrict__ imgs, int64_t Q,
                                                  double* __restrict__ partial) {
  __shared__ double red[4];
  const int b = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * kChunkQuads;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kQuadsPerThread; ++j) {
    const int64_t q = base + j * 256 + threadIdx.x;
    if (q < Q) {
      const float4 d = D[(int64_t)b * Q + q];
      const uint32_t px = imgs[(int64_t)b * Q + q];
      const double e0 = (double)d.x - (double)x32_of(px & 0xffu), e1 = (double)d.y - (double)x32_of((px >> 8) & 0xffu);
      const double e2 = (double)d.z - (double)x32_of((px >> 16) & 0xffu), e3 = (double)d.w - (double)x32_of(px >> 24);
      acc += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
    }
  }
  acc = fh::block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = acc;
}

// grid (n); thread t adds chunks t, t + 256, ... in that order, then the fixed block tree
__global__ __launch_bounds__(256) void k_sqerr_final(const double* __restrict__ partial, int chunks, double* __restrict__ out) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  double s = 0.0;
  for (int c = threadIdx.x; c < chunks; c += 256) s += partial[(int64_t)b * chunks + c];
  s = fh::block_sum_256(s, red);
  if (threadIdx.x == 0) out[b] = s;
}

inline int64_t quads_of(int S) { return (int64_t)3 * S * S / 4; }
inline int64_t chunks_of(int S) { return (quads_of(S) + kChunkQuads - 1) / kChunkQuads; }
inline bool side_ok(int S) { return S >= 2 && S % 2 == 0 && S <= 16384; }  // 3 S^2 / 4 quads: whole, and chunks fit a grid

}  // namespace

extern "C" {

int fh_noisy_u8(const uint8_t* imgs, const int64_t* img_index, int n, int S, double sigma, int level, uint64_t seed, float* out,
                void* stream) {
  if (!imgs || !img_index || !out || n < 1 || !side_ok(S) || level < 0 || !(sigma >= 0.0) || ((uintptr_t)imgs & 3) ||
      ((uintptr_t)out & 15))
    return FH_EINVAL;
  for (int b = 0; b < n; ++b)
    if (img_index[b] < 0 || img_index[b] > (int64_t)0xffffffffLL) return FH_EINVAL;
  const int64_t Q = quads_of(S);
  const unsigned gx = (unsigned)((Q + 255) / 256);
  for (int s = 0; s < n; s += kNoisyImgs) {
    const int m = n - s < kNoisyImgs ? n - s : kNoisyImgs;
    NoisyIdx idx = {};
    for (int b = 0; b < m; ++b) idx.v[b] = (uint32_t)img_index[s + b];
    hipLaunchKernelGGL(k_noisy_u8, dim3(gx, m), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t*>(imgs) + (int64_t)s * Q, idx, Q, sigma, (uint32_t)level, (uint32_t)seed,
                       (uint32_t)(seed >> 32), reinterpret_cast<float4*>(out) + (int64_t)s * Q);
    FH_LAUNCH_CHECK();
  }
  return 0;
}

int64_t fh_sqerr_u8_scratch_doubles(int n, int S) { return n < 1 || !side_ok(S) ? 0 : (int64_t)n * chunks_of(S); }

int fh_sqerr_u8(const float* D, const uint8_t* imgs, int n, int S, double* scratch, double* out, void* stream) {
  if (!D || !imgs || !scratch || !out || n < 1 || n > 65535 || !side_ok(S) || ((uintptr_t)D & 15) || ((uintptr_t)imgs & 3))
    return FH_EINVAL;
  const int64_t Q = quads_of(S);
  const int chunks = (int)chunks_of(S);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sqerr_u8, dim3(chunks, n), dim3(256), 0, st, reinterpret_cast<const float4*>(D),
                     reinterpret_cast<const uint32_t*>(imgs), Q, scratch);
  FH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sqerr_final, dim3(n), dim3(256), 0, st, (const double*)scratch, chunks, out);
  FH_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

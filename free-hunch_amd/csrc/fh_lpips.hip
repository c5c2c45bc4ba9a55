// LPIPS (v0.1, VGG16 backbone) on the device - the streaming kernels around the thirteen 3 x 3 convolutions, which are the
// UNet's own entry points (fh_conv2d_x6_nhwc / fh_conv2d_nhwc).  Reference: generate_conditional.py:499-583,
// lpips.LPIPS(net='vgg') on (x / 255 - 0.5) * 2.  Activations are float32 NHWC; both images of a pair travel in ONE batch of
// 2N (first N = image a, last N = image b).
//   k_lpips_prep     : uint8 NCHW pair -> float32 NHWC [2N][H][W][32] through a 3 x 256 table (scaling layer folded in),
//                      channels 3..31 zero.  One thread per (pixel, 4-channel group): 16-byte stores, 128 B per pixel.
//   k_relu           : in place, 16-byte accesses.
//   k_relu_maxpool2  : ReLU + 2 x 2 / stride 2 max-pool (floor semantics) in one pass, 16-byte accesses.
//   k_lpips_tap<C>   : one tap.  L = min(C / 4, 64) lanes share a pixel, each lane holds C / (4 L) float4 of both halves in
//                      registers: the channel norms are a butterfly sum over the L lanes (every lane ends with the same
//                      value), then each lane forms sum_c w_c (a_c / (|a| + eps) - b_c / (|b| + eps))^2 over ITS channels
//                      and keeps adding over the pixels it visits.  float64 throughout; ReLU on read.  One block partial per
//                      workgroup, written to a fixed slot.
//   k_lpips_tap_final: per image, the partials of its workgroups in a fixed order, divided by H W.  No atomics anywhere:
//                      results are bitwise reproducible and do not depend on the image's position in the batch.
#include "fh_common.h"

namespace {

constexpr int kTapBlocksMax = 256;  // workgroups per image of k_lpips_tap (= threads of k_lpips_tap_final)
constexpr int kPrepC = 32;          // channels of the prepared input (K granularity of the convolutions)

__global__ __launch_bounds__(256) void k_lpips_prep(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                    const float* __restrict__ table, float* __restrict__ out, int N,
                                                    int64_t P) {
  constexpr int G = kPrepC / 4;
  const int64_t total = (int64_t)2 * N * P * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i % G == 0) {
      const int64_t pix = i / G, p = pix % P;
      const int n = (int)(pix / P);
      const uint8_t* src = (n < N ? a + (int64_t)n * 3 * P : b + (int64_t)(n - N) * 3 * P) + p;
      v.x = table[src[0]];
      v.y = table[256 + src[P]];
      v.z = table[512 + src[2 * P]];
    }
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

__device__ __forceinline__ float4 relu4(float4 v) {
  return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}

__global__ __launch_bounds__(256) void k_relu(float* __restrict__ x, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
    reinterpret_cast<float4*>(x)[i] = relu4(reinterpret_cast<const float4*>(x)[i]);
}

__global__ __launch_bounds__(256) void k_relu_maxpool2(const float* __restrict__ in, float* __restrict__ out, int N, int H,
                                                       int W, int C) {
  const int C4 = C / 4, Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)N * Ho * Wo * C4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    const int64_t p = i / C4;
    const int w = (int)(p % Wo), h = (int)((p / Wo) % Ho), n = (int)(p / ((int64_t)Wo * Ho));
    const float4* src = reinterpret_cast<const float4*>(in) + (((int64_t)n * H + 2 * h) * W + 2 * w) * C4 + c4;
    const float4 q = src[0], r = src[C4], s = src[(int64_t)W * C4], t = src[(int64_t)W * C4 + C4];
    const float4 m = make_float4(fmaxf(fmaxf(q.x, r.x), fmaxf(s.x, t.x)), fmaxf(fmaxf(q.y, r.y), fmaxf(s.y, t.y)),
                                 fmaxf(fmaxf(q.z, r.z), fmaxf(s.z, t.z)), fmaxf(fmaxf(q.w, r.w), fmaxf(s.w, t.w)));
    reinterpret_cast<float4*>(out)[i] = relu4(m);
  }
}

// a ra - b rb with both products rounded: a fused multiply-add would keep one product exact, and two identical images would
// then differ by that product's rounding error instead of by exactly 0
__device__ __forceinline__ double unit_diff(float a, double ra, float b, double rb) {
#pragma clang fp contract(off)
  const double x = a * ra, y = b * rb;
  return x - y;
}

// feat [2N][P][C]; blockIdx.y = image, blockIdx.x = one of gridDim.x workgroups that stride over the image's pixels
template <int C>
__global__ __launch_bounds__(256) void k_lpips_tap(const float* __restrict__ feat, const float* __restrict__ lin, int N,
                                                   int64_t P, double* __restrict__ partial) {
  constexpr int C4 = C / 4;
  constexpr int L = C4 < 64 ? C4 : 64;  // lanes per pixel
  constexpr int V = C4 / L;             // float4 per lane and half
  constexpr int PB = 256 / L;           // pixels per workgroup step
  __shared__ double red[4];
  const int n = blockIdx.y;
  const int l = threadIdx.x % L, g = threadIdx.x / L;
  const float4* A = reinterpret_cast<const float4*>(feat) + (int64_t)n * P * C4;
  const float4* B = reinterpret_cast<const float4*>(feat) + (int64_t)(n + N) * P * C4;
  float4 w[V];
#pragma unroll
  for (int v = 0; v < V; ++v) w[v] = reinterpret_cast<const float4*>(lin)[v * L + l];
  double acc = 0.0;
  // every lane of a group of L runs the same trip count, so the shuffles below always see a full group
  for (int64_t p = (int64_t)blockIdx.x * PB + g; p < P; p += (int64_t)gridDim.x * PB) {
    float4 fa[V], fb[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      fa[v] = relu4(A[p * C4 + v * L + l]);
      fb[v] = relu4(B[p * C4 + v * L + l]);
    }
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      sa += (double)fa[v].x * fa[v].x + (double)fa[v].y * fa[v].y + (double)fa[v].z * fa[v].z + (double)fa[v].w * fa[v].w;
      sb += (double)fb[v].x * fb[v].x + (double)fb[v].y * fb[v].y + (double)fb[v].z * fb[v].z + (double)fb[v].w * fb[v].w;
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) {  // butterfly: a + b == b + a, so all L lanes hold bitwise the same sums
      sa += __shfl_xor(sa, o, fh::kWave);
      sb += __shfl_xor(sb, o, fh::kWave);
    }
    const double ra = 1.0 / (sqrt(sa) + 1e-10), rb = 1.0 / (sqrt(sb) + 1e-10);  // guard OUTSIDE the square root
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const double dx = unit_diff(fa[v].x, ra, fb[v].x, rb), dy = unit_diff(fa[v].y, ra, fb[v].y, rb);
      const double dz = unit_diff(fa[v].z, ra, fb[v].z, rb), dw = unit_diff(fa[v].w, ra, fb[v].w, rb);
      acc += (double)w[v].x * dx * dx + (double)w[v].y * dy * dy + (double)w[v].z * dz * dz + (double)w[v].w * dw * dw;
    }
  }
  acc = fh::block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[(int64_t)n * kTapBlocksMax + blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void k_lpips_tap_final(const double* __restrict__ partial, int blocks, int64_t P,
                                                         double* __restrict__ out, int out_stride) {
  __shared__ double red[4];
  const int n = blockIdx.x;
  double s = (int)threadIdx.x < blocks ? partial[(int64_t)n * kTapBlocksMax + threadIdx.x] : 0.0;
  s = fh::block_sum_256(s, red);
  if (threadIdx.x == 0) out[(int64_t)n * out_stride] = s / (double)P;
}

inline unsigned grid_for(int64_t work_items, int cap = 4096) {
  const int64_t b = (work_items + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

inline int tap_blocks(int64_t P, int C) {
  const int L = C / 4 < 64 ? C / 4 : 64;
  const int64_t steps = (P + 256 / L - 1) / (256 / L);
  return (int)(steps < kTapBlocksMax ? steps : kTapBlocksMax);
}

}  // namespace

extern "C" {

int fh_lpips_prep_u8(const uint8_t* a, const uint8_t* b, const float* table, float* out, int N, int H, int W, void* stream) {
  if (!a || !b || !table || !out || N < 1 || H < 1 || W < 1 || ((uintptr_t)out & 15)) return FH_EINVAL;
  const int64_t P = (int64_t)H * W;
  hipLaunchKernelGGL(k_lpips_prep, dim3(grid_for(2 * N * P * (kPrepC / 4))), dim3(256), 0, (hipStream_t)stream, a, b, table, out,
                     N, P);
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_relu_f32(float* x, int64_t n, void* stream) {
  if (n < 0 || n % 4 != 0 || (n > 0 && !x) || ((uintptr_t)x & 15)) return FH_EINVAL;
  if (n > 0) hipLaunchKernelGGL(k_relu, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, x, n / 4);
  FH_LAUNCH_CHECK();
  return 0;
}

int fh_relu_maxpool2_nhwc(const float* in, float* out, int N, int H, int W, int C, void* stream) {
  if (!in || !out || N < 1 || H < 2 || W < 2 || C < 4 || C % 4 != 0 || ((uintptr_t)in & 15) || ((uintptr_t)out & 15))
    return FH_EINVAL;
  hipLaunchKernelGGL(k_relu_maxpool2, dim3(grid_for((int64_t)N * (H / 2) * (W / 2) * (C / 4))), dim3(256), 0,
                     (hipStream_t)stream, in, out, N, H, W, C);
  FH_LAUNCH_CHECK();
  return 0;
}

int64_t fh_lpips_tap_scratch_doubles(int N) { return (int64_t)(N < 0 ? 0 : N) * kTapBlocksMax; }

int fh_lpips_tap(const float* feat, const float* lin, int N, int H, int W, int C, double* scratch, double* out,
                 int out_stride, void* stream) {
  if (!feat || !lin || !scratch || !out || N < 1 || N > 65535 || H < 1 || W < 1 || out_stride < 1 || ((uintptr_t)feat & 15) ||
      ((uintptr_t)lin & 15))
    return FH_EINVAL;
  if (C != 64 && C != 128 && C != 256 && C != 512) return FH_ESIZE;
  const int64_t P = (int64_t)H * W;
  const int blocks = tap_blocks(P, C);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks, N);
  if (C == 64)
    hipLaunchKernelGGL(k_lpips_tap<64>, grid, dim3(256), 0, st, feat, lin, N, P, scratch);
  else if (C == 128)
    hipLaunchKernelGGL(k_lpips_tap<128>, grid, dim3(256), 0, st, feat, lin, N, P, scratch);
  else if (C == 256)
    hipLaunchKernelGGL(k_lpips_tap<256>, grid, dim3(256), 0, st, feat, lin, N, P, scratch);
  else
    hipLaunchKernelGGL(k_lpips_tap<512>, grid, dim3(256), 0, st, feat, lin, N, P, scratch);
  FH_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_lpips_tap_final, dim3(N), dim3(256), 0, st, (const double*)scratch, blocks, P, out, out_stride);
  FH_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"

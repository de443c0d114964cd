// clip.hip -- global-norm gradient clipping over the training loop's flat gradient tensor (include/trajsde_hip_clip.h):
// torch.nn.utils.clip_grad_norm_ + AdamW as three launches.  2 MB of gradient is a launch-latency problem, not a bandwidth one:
// the sum of squares is spread over up to 512 workgroups that each read 8 KB, a single wave adds their partials, and the scaling
// rides inside the AdamW launch.  A unit of its own: k_adamw (optim.hip) keeps its listing.
#include "adamw.hpp"
#include "common.hpp"
#include "../../include/trajsde_hip_clip.h"

namespace tsde {

typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int CLIP_THREADS = 256;
constexpr int CLIP_WG_FLOATS = 2 * 4 * CLIP_THREADS;   // one workgroup, one pass: two 16-byte chunks a thread
constexpr int CLIP_MAX_WGS = 512;                      // one pass of the full grid: 1 M elements

inline int clip_wgs(int64_t n) {
  const int64_t w = (n + CLIP_WG_FLOATS - 1) / CLIP_WG_FLOATS;
  return int(w > CLIP_MAX_WGS ? CLIP_MAX_WGS : w);
}

// sum over one wave, fixed order (lane l ends with x_l + x_{l+32} + ... as a tree; lane 0 holds the total)
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}

// partial[b] = sum of grad[i]^2 over workgroup b's elements, in float64.  Element i always belongs to the same thread of the same
// workgroup and is added in the same place of that thread's sequence, whatever the pointer's alignment: thread t of workgroup b takes
// the 4-element chunks at b * 2048 + u * 1024 + 4 t (u = 0, 1) of every pass, in order.  Alignment only decides how a chunk is LOADED:
// A = the pointer's offset in floats from a 16-byte boundary (one instantiation each, picked by the host); a chunk is then
// lo[A..3] ++ hi[0..A-1] of the two aligned 16-byte words around it.  Chunks whose aligned words would reach outside
// [grad, grad + n) -- the first, when A != 0, and the last one or two -- are read element by element.
__device__ __forceinline__ void add_square(double& acc, float x) {
#pragma clang fp contract(off)
  const double d = double(x);
  acc = acc + d * d;                                        // the square is exact in float64
}
template <int A>
__global__ __launch_bounds__(CLIP_THREADS) void k_grad_sumsq(const float* __restrict__ grad, int64_t n, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double sh[CLIP_THREADS / 64];
  double acc = 0.0;
  const int64_t stride = int64_t(gridDim.x) * CLIP_WG_FLOATS;
  for (int64_t b = int64_t(blockIdx.x) * CLIP_WG_FLOATS; b < n; b += stride) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t e = b + u * (4 * CLIP_THREADS) + 4 * int(threadIdx.x);
      if (e + 4 <= n && (A == 0 || (e >= 4 && e + 8 - A <= n))) {
        const f4* __restrict__ words = reinterpret_cast<const f4*>(grad + (e - A));   // 16-byte aligned; e - A >= 0 here
        const f4 lo = words[0];
        if (A == 0) {
          add_square(acc, lo[0]); add_square(acc, lo[1]); add_square(acc, lo[2]); add_square(acc, lo[3]);
        } else {
          const f4 hi = words[1];
#pragma unroll
          for (int k = 0; k < 4; ++k) add_square(acc, A + k < 4 ? lo[(A + k) & 3] : hi[(A + k) & 3]);
        }
      } else {
        for (int k = 0; k < 4; ++k)
          if (e + k < n) add_square(acc, grad[e + k]);
      }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one wave: lane l adds partial[l], partial[l + 64], ... in order, the lanes are added as a tree; lane 0 forms the norm and the
// coefficient the way torch.nn.utils.clip_grad_norm_ does -- total_norm + 1e-6 in fp32, `max_norm / t` = t.reciprocal() * max_norm
// (torch/_tensor.py __rdiv__), torch.clamp(max=1.0), which keeps a NaN where fminf would not
__global__ __launch_bounds__(64) void k_grad_norm_finish(const double* __restrict__ partial, int wgs, float max_norm, float* __restrict__ out) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int i = threadIdx.x; i < wgs; i += 64) acc = acc + partial[i];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) {
    const float norm = float(sqrt(acc));
    const float t = norm + 1e-6f;
    const float r = 1.0f / t;
    const float c = r * max_norm;
    out[0] = norm;
    out[1] = c > 1.0f ? 1.0f : c;
  }
}

// k_adamw (optim.hip) with g = grad[i] * coef[0] in front, rounded on its own and stored back
template <bool DIVIDE>
__global__ __launch_bounds__(256) void k_adamw_clipped(float* __restrict__ param, float* __restrict__ grad, float* __restrict__ exp_avg,
                                                       float* __restrict__ exp_avg_sq, int64_t n, AdamScalars c,
                                                       const float* __restrict__ coef, int vec) {
#pragma clang fp contract(off)
  const float cf = coef[0];
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (vec) {
    const int64_t i = 4 * t;
    if (i + 3 < n) {
      f4 p = *reinterpret_cast<const f4*>(param + i), m = *reinterpret_cast<const f4*>(exp_avg + i), v = *reinterpret_cast<const f4*>(exp_avg_sq + i);
      f4 g = *reinterpret_cast<const f4*>(grad + i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = p[k], mk = m[k], vk = v[k];
        const float gk = g[k] * cf;
        adamw_one<DIVIDE>(pk, gk, mk, vk, c);
        p[k] = pk; m[k] = mk; v[k] = vk; g[k] = gk;
      }
      *reinterpret_cast<f4*>(param + i) = p;
      *reinterpret_cast<f4*>(grad + i) = g;
      *reinterpret_cast<f4*>(exp_avg + i) = m;
      *reinterpret_cast<f4*>(exp_avg_sq + i) = v;
    } else {
      for (int64_t j = i; j < n; ++j) {
        const float gj = grad[j] * cf;
        grad[j] = gj;
        adamw_one<DIVIDE>(param[j], gj, exp_avg[j], exp_avg_sq[j], c);
      }
    }
  } else if (t < n) {
    const float gt = grad[t] * cf;
    grad[t] = gt;
    adamw_one<DIVIDE>(param[t], gt, exp_avg[t], exp_avg_sq[t], c);
  }
}

}  // namespace tsde

using namespace tsde;

extern "C" {

int64_t trajsde_grad_norm_ws_bytes(int64_t n) {
  if (n <= 0) return fail(TRAJSDE_ERR_INVALID, "grad_norm_clip: need n > 0");
  return int64_t(sizeof(double)) * clip_wgs(n);
}

int trajsde_grad_norm_clip(const float* grad, int64_t n, float max_norm, void* ws, int64_t ws_bytes, float* out, void* stream) {
  TS_REQUIRE(grad && ws && out, "grad_norm_clip: null pointer");
  TS_REQUIRE(n > 0, "grad_norm_clip: need n > 0");
  TS_REQUIRE(max_norm > 0.f, "grad_norm_clip: max_norm must be positive (and not NaN)");
  TS_REQUIRE((reinterpret_cast<uintptr_t>(grad) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
             "grad_norm_clip: grad and out must be 4-byte aligned");
  TS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "grad_norm_clip: the workspace must be 8-byte aligned");
  const int wgs = clip_wgs(n);
  if (ws_bytes < int64_t(sizeof(double)) * wgs) return fail(TRAJSDE_ERR_WORKSPACE, "grad_norm_clip: workspace below trajsde_grad_norm_ws_bytes");
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* partial = static_cast<double*>(ws);
  switch ((reinterpret_cast<uintptr_t>(grad) >> 2) & 3) {
    case 0: TS_LAUNCH(k_grad_sumsq<0>, dim3(unsigned(wgs)), CLIP_THREADS, 0, st, grad, n, partial); break;
    case 1: TS_LAUNCH(k_grad_sumsq<1>, dim3(unsigned(wgs)), CLIP_THREADS, 0, st, grad, n, partial); break;
    case 2: TS_LAUNCH(k_grad_sumsq<2>, dim3(unsigned(wgs)), CLIP_THREADS, 0, st, grad, n, partial); break;
    default: TS_LAUNCH(k_grad_sumsq<3>, dim3(unsigned(wgs)), CLIP_THREADS, 0, st, grad, n, partial); break;
  }
  TS_LAUNCH(k_grad_norm_finish, dim3(1), 64, 0, st, partial, wgs, max_norm, out);
  return TRAJSDE_OK;
}

int trajsde_adamw_step_clipped(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float decay, float w1,
                               float beta2, float w2, float bias2, int divide, float eps, float neg_step, const float* coef,
                               void* stream) {
  TS_REQUIRE(param && grad && exp_avg && exp_avg_sq && coef, "adamw_step_clipped: null pointer");
  TS_REQUIRE(n >= 0, "adamw_step_clipped: negative length");
  TS_REQUIRE(bias2 > 0.f && bias2 < 3.0e38f, "adamw_step_clipped: the bias-correction scalar must be positive and finite (step >= 1)");
  if (n == 0) return TRAJSDE_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uintptr_t all = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
                        reinterpret_cast<uintptr_t>(exp_avg_sq);
  const int vec = (all & 15) == 0;
  const int64_t threads = vec ? (n + 3) / 4 : n;
  const AdamScalars c{decay, w1, beta2, w2, bias2, eps, neg_step};
  const dim3 grid(unsigned((threads + 255) / 256));
  if (divide) TS_LAUNCH(k_adamw_clipped<true>, grid, 256, 0, st, param, grad, exp_avg, exp_avg_sq, n, c, coef, vec);
  else TS_LAUNCH(k_adamw_clipped<false>, grid, 256, 0, st, param, grad, exp_avg, exp_avg_sq, n, c, coef, vec);
  return TRAJSDE_OK;
}

}  // extern "C"

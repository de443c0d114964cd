// head_cot.hpp -- one head of the SDE decoder (loc or scale: Linear LN ReLU Linear(64,2)) forward + backward on an interpolated state
// from a caller-supplied gradient of its two outputs: the body shared by the cotangent head kernels, k_head_bwd_cot over all K * N
// paths (decoder_cot_bwd.hip) and k_head_bwd_cot_sel over each actor's supported mode (decoder_cot_sel_bwd.hip).
#pragma once
#include "layouts.hpp"
#include "tile.hpp"
#include "tile_bwd.hpp"
#include "bwd.hpp"

namespace tsde {

// one head (image H = HeadL fields, W0T behind it) on the interpolated state s with the upstream gradient (gx, gy) of its two outputs:
// du := gradient at the first layer's output (the weight gradient's delta row), ds += W0^T du; accumulates the head's vector gradients
struct HeadAcc {
  f4 dgam[4], dbet[4], dw3x[4], dw3y[4];
  float db3x, db3y;
};
__device__ __forceinline__ void head_cot_pass(const float* img, const f4 (&s)[4], float gx, float gy, HeadAcc& A, f4 (&du)[4], f4 (&ds)[4],
                                              const Lane& L) {
  const float* H = img + HeadBwdL::FWD;
  f4 u[4], v[4];
  linear<4, 4>(u, s, H + HeadL::W0, H + HeadL::B0, L);
  const float rstd = ln_normalize(u);                       // u = x_hat
  bool pos[16];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const f4 ga = *reinterpret_cast<const f4*>(H + HeadL::G + 16 * jt + 4 * L.g);
    const f4 be = *reinterpret_cast<const f4*>(H + HeadL::E + 16 * jt + 4 * L.g);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float pre = u[jt][c] * ga[c] + be[c];
      pos[jt * 4 + c] = pre > 0.f;
      v[jt][c] = fmaxf(pre, 0.f);
    }
  }
  A.db3x += gx;
  A.db3y += gy;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const f4 wx = *reinterpret_cast<const f4*>(H + HeadL::W3 + 16 * jt + 4 * L.g);
    const f4 wy = *reinterpret_cast<const f4*>(H + HeadL::W3 + 64 + 16 * jt + 4 * L.g);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      A.dw3x[jt][c] = fmaf(gx, v[jt][c], A.dw3x[jt][c]);
      A.dw3y[jt][c] = fmaf(gy, v[jt][c], A.dw3y[jt][c]);
      du[jt][c] = pos[jt * 4 + c] ? fmaf(gx, wx[c], gy * wy[c]) : 0.f;
    }
  }
  ln_backward(du, u, rstd, H + HeadL::G, L.g, A.dgam, A.dbet);
  linear_adj<4, 4>(ds, du, img + HeadBwdL::W0T, L);
}
__device__ __forceinline__ void head_acc_zero(HeadAcc& A) {
  zero4(A.dgam); zero4(A.dbet); zero4(A.dw3x); zero4(A.dw3y);
  A.db3x = A.db3y = 0.f;
}
__device__ __forceinline__ void head_acc_flush(const HeadAcc& A, float* vp, const Lane& L) {
  flush_vec(A.dgam, vp + CotHeadV::DGAM, L);
  flush_vec(A.dbet, vp + CotHeadV::DBET, L);
  flush_vec(A.dw3x, vp + CotHeadV::DW3X, L);
  flush_vec(A.dw3y, vp + CotHeadV::DW3Y, L);
  flush_scalar(A.db3x, vp + CotHeadV::DB3, L);
  flush_scalar(A.db3y, vp + CotHeadV::DB3 + 1, L);
}

}  // namespace tsde

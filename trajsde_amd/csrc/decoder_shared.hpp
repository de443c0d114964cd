// decoder_shared.hpp -- what the decode kernels of decoder.hip and decoder_mc.hip have in common: the loc / scale heads on an
// interpolated state, the C noise struct as a kernel argument, and the launches of decoder.hip that decoder_mc.hip reuses.
#pragma once
#include "common.hpp"
#include "layouts.hpp"
#include "philox.hpp"
#include "tile.hpp"

namespace tsde {

// Linear(64,64)-LN-ReLU-Linear(64,2) head on state s -> (o0, o1)
__device__ __forceinline__ void head_eval(float& o0, float& o1, const f4 (&s)[4], const float* img, const Lane& L) {
  f4 h[4];
  linear<4, 4>(h, s, img + HeadL::W0, img + HeadL::B0, L);
  layer_norm<4>(h, img + HeadL::G, img + HeadL::E, L.g);
  relu<4>(h);
  o0 = row_dot(h, img + HeadL::W3, L.g) + img[HeadL::B3];
  o1 = row_dot(h, img + HeadL::W3 + 64, L.g) + img[HeadL::B3 + 1];
}

#if TSDE_SPLIT_H3
// both heads of the fused kernel on one split of s: stacked first layers (HeadPairL6), fp16x3 matrix products
__device__ __forceinline__ void head_pair_eval(float& lx, float& ly, float& sx, float& sy, const f4 (&s)[4], const float* img,
                                               const Lane& L) {
  using HP = HeadPairL6;
  f4 h[8];
  linear_x6<8, 4>(h, s, img + HP::W0, img + HP::B0, L);
  f4 a[4] = {h[0], h[1], h[2], h[3]}, b[4] = {h[4], h[5], h[6], h[7]};
  layer_norm<4>(a, img + HP::G_LOC, img + HP::E_LOC, L.g);
  relu<4>(a);
  lx = row_dot(a, img + HP::W3_LOC, L.g) + img[HP::B3_LOC];
  ly = row_dot(a, img + HP::W3_LOC + 64, L.g) + img[HP::B3_LOC + 1];
  layer_norm<4>(b, img + HP::G_SC, img + HP::E_SC, L.g);
  relu<4>(b);
  sx = row_dot(b, img + HP::W3_SC, L.g) + img[HP::B3_SC];
  sy = row_dot(b, img + HP::W3_SC + 64, L.g) + img[HP::B3_SC + 1];
}
#endif

inline NoiseArg to_arg(const trajsde_noise* n) {
  NoiseArg a{0, nullptr, nullptr};
  if (n) { a.seed = n->seed; a.z = n->z; a.row_ids = n->row_ids; a.seed_dev = n->seed_dev; }
  return a;
}

// decoder.hip
int pick_grid(int64_t ntiles, int waves_per_wg);
int decoder_init(int32_t N, int num_modes, const float* blob, const float* local_embed, const float* global_embed, float* y0, float* pi,
                 hipStream_t stream);

}  // namespace tsde

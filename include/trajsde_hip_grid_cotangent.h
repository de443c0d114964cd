/* trajsde_hip_grid_cotangent.h -- extension of the trajsde-mi355x C-ABI (trajsde_hip.h, same library, same ABI version): the vanilla
 * HiVT variant's MLPDecoder backward from caller-supplied cotangents.  trajsde_mlp_decoder_l2_backward / _nll_backward fuse a loss into
 * the backward and differentiate the winning mode only; this one takes dL/dloc and dL/dpi of ANY loss and differentiates all K modes
 * and the three-layer pi head, so `scale.*` and `pi.*` are trained too.  (The SDE decoder's twin is trajsde_hip_cotangent.h.) */
#ifndef TRAJSDE_HIP_GRID_COTANGENT_H
#define TRAJSDE_HIP_GRID_COTANGENT_H

#include "trajsde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Added at ABI 10: the vector-Jacobian product of MLPDecoder.forward (dec_hivt_nusargo_grid.py:47-63).  No loss is formed inside:
 * `d_loc` [K,N,T,4] is dL/dloc of ANY loss over all K modes (channels 0-1 the locations, 2-3 the scales) and `d_pi` [N,K] is dL/dpi.
 * The scale channels pass through ELU + 1 + min_scale, whose derivative min(1, scale - min_scale) is read off `loc`, the forward's
 * output.  `grads` follow trajsde_param_name(TRAJSDE_STAGE_DECODER_MLP_COT_BWD, i, future_steps, num_modes): the DECODER_MLP_NLL_BWD
 * table (16 names), then pi.0 / .1 / .3 / .4 / .6 weight and bias (26 in all); `blob_bwd` is that stage's image.  Overwritten in full:
 * every `grads[i]`, `d_local` (the sum over the modes of the aggr_embed and the pi path, modes added in order 0..K-1: no atomics,
 * identical calls give identical words) and `d_global`.  Inputs are only read.  The workspace holds the saved rows of all K * N (mode,
 * actor) pairs, 3.75 KB per pair. Refused with a message: null pointers, n_grads other than 26, a workspace below the query,
 * future_steps outside 1..64, an empty problem or one whose K * N overflows the kernels' 32-bit row indices. */
int64_t trajsde_mlp_decoder_cotangent_backward_ws_bytes(int32_t N, int num_modes, int future_steps);
int trajsde_mlp_decoder_cotangent_backward(int32_t N, int num_modes, int future_steps, const float* blob_bwd,
                                           const float* local_embed /*[N,64]*/, const float* global_embed /*[K,N,64]*/,
                                           const float* loc /*[K,N,T,4] forward output*/, float min_scale,
                                           const float* d_loc /*[K,N,T,4]*/, const float* d_pi /*[N,K]*/, void* ws, int64_t ws_bytes,
                                           float* const* grads, int n_grads, float* d_local /*[N,64]*/, float* d_global /*[K,N,64]*/,
                                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJSDE_HIP_GRID_COTANGENT_H */

/* trajsde_hip_cotangent.h -- extension of the trajsde-mi355x C-ABI (trajsde_hip.h, same library, same ABI version): the SDE decoder
 * stage's backward from caller-supplied cotangents.  The entry points of trajsde_hip.h fuse a loss (winner-takes-all L2, Laplace NLL)
 * into the decoder backward and replay the winning mode only; this one takes dL/dloc and dL/dpi of ANY loss and differentiates all
 * K modes, so the scale and pi heads are trained too. */
#ifndef TRAJSDE_HIP_COTANGENT_H
#define TRAJSDE_HIP_COTANGENT_H

#include "trajsde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Added at ABI 10, Euler-Maruyama only: the vector-Jacobian product of
 * SDEDecoder.forward (DEC:77-105) at the forward's noise.  No loss is formed inside: `d_loc` [K,N,T,4] is dL/dloc of ANY loss over all
 * K modes (channels 0-1 the locations, 2-3 the scales) and `d_pi` [N,K] is dL/dpi.  All K * N paths are replayed with the forward's
 * Philox counters (global row id k * N + n; noise->row_ids honoured; injected `z` is [n_euler][K*N][64]) and swept in reverse; the
 * scale channels pass through ELU + 1 + min_scale (DEC:97-98), whose derivative min(1, scale - min_scale) is read off `loc`, the
 * forward's output.  `grads` follow trajsde_param_name(TRAJSDE_STAGE_DECODER_COT_BWD, i): the DECODER_NLL_BWD table, then pi.0 / .1 /
 * .3 weight and bias; `blob_bwd` is that stage's image, `blob_fwd` the TRAJSDE_STAGE_DECODER one.  Overwritten in full: every
 * `grads[i]`, `d_local` (the sum over the modes of the aggr_embed and the pi path, modes added in order 0..K-1: no atomics, identical
 * calls give identical words) and `d_global`.  Inputs are only read.  The tape covers K * N rows, so the workspace is about K times
 * trajsde_decoder_nll_backward_ws_bytes.  Refused with a message: null pointers, n_grads other than the table's length, a workspace
 * below the query, trajsde_state_storage(1) (the replayed states would not be the forward's). */
int64_t trajsde_decoder_cotangent_backward_ws_bytes(int32_t N, int num_modes, int future_steps, int n_euler);
int trajsde_decoder_cotangent_backward(int32_t N, int num_modes, int future_steps, const float* blob_fwd, const float* blob_bwd,
                                       const float* local_embed /*[N,64]*/, const float* global_embed /*[K,N,64]*/,
                                       const float* step_table /*[n_euler,8]*/, int n_euler, const float* out_table /*[T,4]*/,
                                       const trajsde_noise* noise, const float* loc /*[K,N,T,4] forward output*/, float min_scale,
                                       const float* d_loc /*[K,N,T,4]*/, const float* d_pi /*[N,K]*/, void* ws, int64_t ws_bytes,
                                       float* const* grads, int n_grads, float* d_local /*[N,64]*/, float* d_global /*[K,N,64]*/,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJSDE_HIP_COTANGENT_H */

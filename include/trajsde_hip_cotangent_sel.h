/* trajsde_hip_cotangent_sel.h -- extension of the trajsde-mi355x C-ABI (trajsde_hip.h, same library, same ABI version): the SDE decoder
 * stage's backward from caller-supplied cotangents when dL/dloc is non-zero in at most ONE mode per actor -- any winner-takes-all
 * regression loss, next to any loss on pi.  trajsde_decoder_cotangent_backward (trajsde_hip_cotangent.h) replays and sweeps all K * N
 * paths; this one finds each actor's supported mode from `d_loc` on the device and replays that path only, like the welded entry points
 * of trajsde_hip.h.  The pi head does not depend on the SDE solution and is differentiated over all K modes as before. */
#ifndef TRAJSDE_HIP_COTANGENT_SEL_H
#define TRAJSDE_HIP_COTANGENT_SEL_H

#include "trajsde_hip_cotangent.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Added at ABI 10, Euler-Maruyama only.  The arguments, the blobs (TRAJSDE_STAGE_DECODER, TRAJSDE_STAGE_DECODER_COT_BWD), the gradient
 * table, the noise contract (global row id k * N + n; injected `z` is [n_euler][K*N][64], of which the selected rows are read) and the
 * refusals are those of trajsde_decoder_cotangent_backward, plus `status`: two device words.
 *   Support: mode k supports actor n when any word of d_loc[k, n, :, :] compares != 0.0f (a NaN does).  sel[n] is the LOWEST supported
 * mode, or 0 when there is none (that actor's SDE and head gradients are then zero, as its cotangent is).  Path sel[n] * N + n is
 * replayed and swept; row sel[n] of d_global[:, n] gets the aggr_embed gradient, the other modes' rows zeros, then the pi head adds its
 * part to all K.  On return status[0] = the number of actors with MORE than one supported mode, status[1] = the number of supported
 * actors, and the first N int32 words of `ws` hold sel.
 *   Premise: status[0] == 0.  When it is violated the call still completes and returns 0, touches nothing outside the caller's buffers,
 * and the gradients are those of the selected mode alone: the further modes' cotangent rows are ignored.  Detecting that is the caller's
 * business -- read `status` where the host waits anyway; nothing faults or asserts on the device.
 *   Overwritten in full: every `grads[i]`, `d_local`, `d_global`, `status`.  Inputs are only read; the workspace may hold anything on
 * entry.  No atomics: identical calls give identical words.  The workspace is trajsde_decoder_nll_backward_ws_bytes' carve over N rows
 * plus the pi head's K * N delta rows: strictly below trajsde_decoder_cotangent_backward_ws_bytes for K >= 2, and the SDE tape does not
 * grow with K. */
int64_t trajsde_decoder_cotangent_backward_sel_ws_bytes(int32_t N, int num_modes, int future_steps, int n_euler);
int trajsde_decoder_cotangent_backward_sel(int32_t N, int num_modes, int future_steps, const float* blob_fwd, const float* blob_bwd,
                                           const float* local_embed /*[N,64]*/, const float* global_embed /*[K,N,64]*/,
                                           const float* step_table /*[n_euler,8]*/, int n_euler, const float* out_table /*[T,4]*/,
                                           const trajsde_noise* noise, const float* loc /*[K,N,T,4] forward output*/, float min_scale,
                                           const float* d_loc /*[K,N,T,4]*/, const float* d_pi /*[N,K]*/, void* ws, int64_t ws_bytes,
                                           float* const* grads, int n_grads, float* d_local /*[N,64]*/, float* d_global /*[K,N,64]*/,
                                           int32_t* status /*[2]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJSDE_HIP_COTANGENT_SEL_H */

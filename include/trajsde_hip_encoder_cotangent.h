/* trajsde_hip_encoder_cotangent.h -- extension of the trajsde-mi355x C-ABI (trajsde_hip.h, same library, same ABI version): the SDE
 * encoder stage's backward from caller-supplied cotangents of ALL THREE of its differentiable outputs.  trajsde_encoder_backward of
 * trajsde_hip.h takes dL/d local_embed and welds the one loss on the diffusion outputs it knows, DiffBCE, in through `diff_weight`;
 * this one forms no loss: it is the stage's vector-Jacobian product, which is what a torch.autograd node of the stage needs. */
#ifndef TRAJSDE_HIP_ENCODER_COTANGENT_H
#define TRAJSDE_HIP_ENCODER_COTANGENT_H

#include "trajsde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Added at ABI 10: the vector-Jacobian product of LocalEncoderSDESepPara2.forward (ENC:66-202) at the forward's noise and dropout.
 * The arguments are those of trajsde_encoder_backward with `diff_weight` and `diff_loss` replaced by two optional, read-only
 * cotangents: `d_diff_in` = dL/d diff_in [A,64] and `d_diff_out` = dL/d diff_out [A,64] (the two halves of the forward's `diff_pick`
 * [2A,64]); a null pointer stands for zeros.  A diffusion output row is ONE sigmoid value repeated over its 64 channels (ENC:191-194),
 * so the row's cotangent enters as the sum of its 64 channels, added in a fixed order (no atomics: identical calls give identical
 * words).  With both null the call is trajsde_encoder_backward at diff_weight = 0, word for word.
 * Carried over unchanged: `noise` / `dropout` must be the forward's; the tape / scratch split (`ws` = the tape of
 * trajsde_encoder_tape_bytes with `scratch` = a buffer of trajsde_encoder_backward_scratch_bytes, or both in one `ws` of
 * trajsde_encoder_backward_ws_bytes with scratch = null -- there is no size query of its own); `tape_valid`; the optional outputs
 * `d_latent` [N,64] / `d_aa_out` [H,Nt,64]; `grads[i]` shaped like parameter trajsde_param_name(TRAJSDE_STAGE_ENCODER_BWD, i),
 * pre-zeroed by the caller and overwritten where the batch reaches the parameter; `blob_bwd` is that stage's image.  Refused with a
 * message: null pointers among the required arguments, a graph without the fake-agent rows (A = 0), n_grads other than the table's
 * length, a workspace below the query, trajsde_state_storage(1). */
int trajsde_encoder_cotangent_backward(const trajsde_batch* b, const trajsde_graph* g, const float* rotate_mat, const float* blob_fwd,
                                       const float* blob_bwd, const float* enc_step_table /*HOST [H,8]*/,
                                       const float* enc_step_table_dev /*device [H,8]*/, const trajsde_noise* noise,
                                       const float* d_local /*[N,64]*/, const float* d_diff_in /*[A,64] or null*/,
                                       const float* d_diff_out /*[A,64] or null*/, void* ws, int64_t ws_bytes, float* const* grads,
                                       int n_grads, float* d_latent, float* d_aa_out,
                                       const trajsde_dropout* dropout /* the forward's, or null */,
                                       int tape_valid /* 1: `ws` still holds the tape trajsde_encoder_forward_train left in it */,
                                       void* scratch /* or null: scratch follows the tape inside `ws` */, int64_t scratch_bytes,
                                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJSDE_HIP_ENCODER_COTANGENT_H */

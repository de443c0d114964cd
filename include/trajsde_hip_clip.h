/* trajsde_hip_clip.h -- extension of the trajsde-mi355x C-ABI (trajsde_hip.h, same library, same ABI version): global-norm gradient
 * clipping for the flat training loop, i.e. torch.nn.utils.clip_grad_norm_ (norm type 2, error_if_nonfinite=False) over ONE fp32
 * tensor followed by trajsde_adamw_step, in three launches and without a host synchronisation. */
#ifndef TRAJSDE_HIP_CLIP_H
#define TRAJSDE_HIP_CLIP_H

#include "trajsde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Added at ABI 10.  out[0] = ||grad||_2, out[1] = the clip coefficient; both fp32, on the device, overwritten in full.
 * Every grad[i] is squared in float64 (exact) and the squares are summed in float64 in an order that depends on `n` alone -- not on
 * the pointer's alignment, the workspace's contents or the dispatch: identical calls give identical words, and no atomics touch
 * floating-point data.  Two launches: workgroups of 256 threads take 2048 consecutive elements a pass (grid: ceil(n / 2048)
 * workgroups, at most 512, grid-stride beyond that) and leave one float64 partial each in `ws`; one wave adds the partials in a fixed
 * order and forms, as torch forms them (torch/nn/utils/clip_grad.py; `max_norm / tensor` is torch's reciprocal-times-scalar):
 *     norm = (float)sqrt(sum)
 *     coef = (1.0f / (norm + 1e-6f)) * max_norm, clamped to at most 1.0f      (fp32 operations, each rounded on its own)
 * A NaN norm gives a NaN coefficient (torch.clamp keeps it), an infinite norm gives 0.  `grad` need only be 4-byte aligned (a slice
 * of a flat buffer): aligned 16-byte loads in the body, single elements at the two ends, nothing read outside [grad, grad + n).
 * `ws` (8-byte aligned, >= trajsde_grad_norm_ws_bytes(n) = 8 bytes per workgroup) may hold anything on entry.
 * Refused with TRAJSDE_ERR_INVALID and a message: null pointers, n <= 0, max_norm <= 0 or NaN, a misaligned `ws`;
 * TRAJSDE_ERR_WORKSPACE: `ws_bytes` below the query.  The query returns a negative value for n <= 0. */
int64_t trajsde_grad_norm_ws_bytes(int64_t n);
int trajsde_grad_norm_clip(const float* grad, int64_t n, float max_norm, void* ws, int64_t ws_bytes, float* out /*[2]*/, void* stream);

/* Added at ABI 10.  trajsde_adamw_step with g = grad[i] * coef[0] in front: the product is rounded to fp32 on its own (torch
 * multiplies the gradient in place before the optimizer reads it), stored back to grad[i], and the update of trajsde_adamw_step --
 * same operations, same order, same scalars, both `divide` forms -- runs on g.  `coef` is a device pointer (out + 1 of the call
 * above); with coef[0] == 1.0f the parameters and both moments end on the bits of trajsde_adamw_step.  Written: param, grad, exp_avg,
 * exp_avg_sq, n elements each; `coef` is only read.  n == 0 is a no-op. */
int trajsde_adamw_step_clipped(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float decay, float w1,
                               float beta2, float w2, float bias2, int divide, float eps, float neg_step, const float* coef,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJSDE_HIP_CLIP_H */

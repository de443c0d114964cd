// adamw.hpp -- one element of torch.optim.AdamW's update, shared by k_adamw (optim.hip) and k_adamw_clipped (clip.hip): the two kernels
// live in units of their own and must end on the same bits, so the operation sequence exists once.
#pragma once
#include <hip/hip_runtime.h>

namespace tsde {

// torch.optim.AdamW's single-tensor update, operation by operation (torch/optim/adamw.py _single_tensor_adamw, amsgrad = maximize =
// False), with its scalars formed by the caller the way torch forms them (Python floats, rounded to fp32 where a tensor op takes them):
//   param.mul_(1 - lr * weight_decay)                                    decay
//   exp_avg.lerp_(grad, 1 - beta1)                                       w1   (|w| < 0.5: a + w (b - a), ATen/native/Lerp.h)
//   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)         beta2, w2
//   denom = (exp_avg_sq.sqrt() / sqrt(1 - beta2^step)).add_(eps)         bias2, eps  (torch divides a tensor by a host scalar as a
//                                                                        product with the scalar's reciprocal, formed in double and
//                                                                        rounded to fp32: `divide` = 0, bias2 = that reciprocal)
// The multi-tensor form (`foreach=True`, what AdamW(model.parameters()) runs on a GPU: MODEL:205) differs in ONE operation: its
// _foreach_div_ by the scalar list is a true division (`divide` = 1, bias2 = sqrt(1 - beta2^step) itself).  Measured on this torch,
// element by element over 2e5 values: both forms reproduced exactly (tests/test_gpu_step_launches.py).
//   param.addcdiv_(exp_avg, denom, value=-(lr / (1 - beta1^step)))       neg_step
struct AdamScalars {
  float decay, w1, beta2, w2, bias2, eps, neg_step;
};
// (each torch op rounds its result to fp32; inside one op the multiply-add is fused, as hipcc contracts it in torch's kernels.  Written
//  with contraction OFF and the fused operations spelled out: the __f*_rn spellings are plain operators to this compiler and were
//  contracted across the op boundaries; __fsqrt_rn is the bare 1-ulp v_sqrt_f32, sqrtf the correctly rounded sequence torch uses)
template <bool DIVIDE>
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamScalars& c) {
#pragma clang fp contract(off)
  p = p * c.decay;
  const float diff = g - m;
  m = c.w1 < 0.5f ? __builtin_fmaf(c.w1, diff, m) : __builtin_fmaf(-diff, 1.f - c.w1, g);
  v = v * c.beta2;
  const float gg = g * g;
  v = __builtin_fmaf(c.w2, gg, v);                                     // addcmul: a + value * (b * c)
  float denom = DIVIDE ? sqrtf(v) / c.bias2 : sqrtf(v) * c.bias2;
  denom = denom + c.eps;
  const float q = m / denom;
  p = __builtin_fmaf(c.neg_step, q, p);
}

}  // namespace tsde

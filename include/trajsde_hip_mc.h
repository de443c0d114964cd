/* trajsde_hip_mc.h -- extension of the trajsde-mi355x C-ABI (trajsde_hip.h, same library, same ABI version): Monte-Carlo decoding.
 * The SDE decoder draws ONE sample path per (mode, actor); this entry point solves R of them for every path in one launch, from
 * one y0 and one set of embeddings, and reduces them on the device (csrc/decoder_mc.hip; runtime.StageRuntime.decoder_forward_mc;
 * DESIGN.md section 7). */
#ifndef TRAJSDE_HIP_MC_H
#define TRAJSDE_HIP_MC_H

#include "trajsde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRAJSDE_MC_MAX_SAMPLES 65536

/* Added at ABI 10.  Sample s (0 <= s < R = n_samples) of path r = k * N + n is the solve of trajsde_decoder_forward (milstein == 0,
 * `blob` the TRAJSDE_STAGE_DECODER image) or trajsde_decoder_forward_milstein (milstein != 0, the TRAJSDE_STAGE_DECODER_MILSTEIN
 * image) with ONE change: the Philox counter row is  rid(r) + s * D  in uint32 arithmetic, D = sample_stride, where rid(r) is
 * noise->row_ids[r] if row ids are given and r otherwise.  Stream, step word, quad word and key (noise->seed or *noise->seed_dev)
 * are unchanged.  So sample 0 is bit for bit what the plain entry point draws, and sample s is what it draws under row ids
 * shifted by s * D.  The natural D is num_modes * N; a sharded caller passes the global row count.  Refused: D < 1, and any D with
 * (R - 1) * D + num_modes * N > 2^32 -- with local ids that is the 32-bit counter row overflowing.  Caller-supplied row ids live on
 * the device and are not read by the host: a caller whose largest id is M must itself keep M + (R - 1) * D < 2^32.
 * With injected normals (noise->z) the layout is [n_euler, R * num_modes * N, 64], row s * num_modes * N + r.
 * Outputs, all written in full by every call:
 *   loc_mean [K,N,T,4]  sample mean of (x, y, scale_x, scale_y)
 *   loc_cov  [K,N,T,3]  unbiased (/ (R - 1)) sample covariance of (x, y): var_x, var_y, cov_xy
 *   samples  [R,K,N,T,4] every sample; may be null (nothing is written)
 *   loc0     [K,N,T,4]  sample 0 alone -- the plain entry point's `loc`; may be null
 *   pi       [N,K]      as the plain entry point (it does not depend on the noise)
 * The reduction forms no sum of squares of the samples (deviations are taken from a mean first), uses no atomics and adds in a
 * fixed order: identical calls give identical words.  A wave's 16-row tile holds 16 samples of one path, or, for n_samples <= 8, the
 * samples of 8, 4 or 2 paths: the cost per sample-path is that of the plain solve from n_samples = 2 on (exactly at 2, 4, 8 and
 * multiples of 16; rows left over in a group or in the last tile compute and are dropped).  2 <= n_samples <= TRAJSDE_MC_MAX_SAMPLES.  The workspace query returns -1
 * (reason in trajsde_last_error) for sizes it refuses.  The decoder state is noted at range-guard site 0 and the embedding rows at
 * site 1, like the plain solve (tests/test_gpu_mc.py).  The launch returns a trajsde_status as int32_t. */
int64_t trajsde_decoder_mc_ws_bytes(int32_t N, int num_modes, int future_steps, int n_samples);
int32_t trajsde_decoder_forward_mc(int32_t N, int num_modes, int future_steps, int milstein, const float* blob,
                                   const float* local_embed /*[N,64]*/, const float* global_embed /*[K,N,64]*/,
                                   const float* step_table /*[n_euler,8]*/, int n_euler, const float* out_table /*[T,4]*/,
                                   float min_scale, const trajsde_noise* noise, int n_samples, int64_t sample_stride, void* ws,
                                   int64_t ws_bytes, float* loc_mean, float* loc_cov, float* samples /*or NULL*/,
                                   float* loc0 /*or NULL*/, float* pi, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJSDE_HIP_MC_H */

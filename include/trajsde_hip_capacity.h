/* trajsde_hip_capacity.h -- extension of the trajsde-mi355x C-ABI (trajsde_hip.h, same library, same ABI version): a batch of any
 * shape staged into capacity-sized static buffers with inert padding: the inference forward then runs on tensors of ONE shape at fixed
 * addresses whatever batch arrives (runtime.CapacityBuffers; host twin runtime.pad_batch_host). */
#ifndef TRAJSDE_HIP_CAPACITY_H
#define TRAJSDE_HIP_CAPACITY_H

#include "trajsde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Added at ABI 10.  `dst` describes the static buffers: its sizes are the user-visible capacity PLUS the permanent reserve,
 *     dst->N = actors + 2,  dst->A = scenes + 1,  dst->E = edges,  dst->L = lanes + 1,  dst->E_al = lane_edges,
 * and its pointers are WRITTEN (the struct is shared with the entry points that read a batch, hence the const members).  With
 * N, S, E, L, E_al the sizes of `src` (S = src->A scenes, one agent each) the call copies the real rows and writes
 *   pad actors  [N, dst->N)    padding_mask 1 at every slot, bos_mask 0, x / positions / rotate_angles / y 0
 *   pad scenes  [S, dst->A)    one pad actor each, in ascending order (agent_index[S + j] = N + j, source 0); the LAST pad scene is the
 *                              permanent one and takes every pad actor that is left -- at least two, the reserve
 *   pad edges   [E, dst->E)    between two different actors of the permanent pad scene, dealt round-robin over its actors (never valid at
 *                              any step: dropped by the snapshot lists and by the t = H - 1 filter of the global list)
 *   pad lanes   [L, dst->L)    positions 0, paddings 0
 *   pad lane-actor edges       lane dst->L - 1 to an actor of the permanent pad scene, vector (200 r, 200 r) with r = `local_radius`:
 *                              dropped by the radius filter (ENC:198)
 * and the three row-id tables under which the forward of `dst` draws, for the real rows, the noise the forward of `src` draws from
 * its local row indices (trajsde_noise.row_ids):
 *   fake_row_ids [dst->A]             a -> a
 *   enc_row_ids  [dst->N + dst->A]    actor i < N -> i, fake row dst->N + a (a < S) -> N + a; pad actor i -> S + i, pad fake row stays
 *   dec_row_ids  [num_modes * dst->N] k * dst->N + n (n < N) -> k * N + n; pad rows -> num_modes * N + k * (dst->N - N) + (n - N)
 * `y` [N,F,2] may be null (zeros are written); `dst_y` [dst->N,F,2] may be null (nothing is written).  EVERY element of every
 * destination tensor and table is overwritten by every call, in one launch of plain vector loads and stores: a smaller batch after a
 * larger one leaves nothing behind.  Sources are read only inside their tensors.
 * Everything is validated before the launch.  trajsde_batch_pad_fits is that validation alone: TRAJSDE_OK, or TRAJSDE_ERR_INVALID
 * with a message that names the dimension -- a batch fits when  S <= scenes,  N + (scenes - S) <= actors  (every pad scene needs an
 * actor),  E <= edges,  L <= lanes,  E_al <= lane_edges, and H, TT and lane_pts agree. */
/* Both return a trajsde_status as int32_t.  The launch copies tensors and computes indices (the compiler expands its integer `/` and `%`
 * through fp32 reciprocals, nothing more): it forms no split-precision product, so the fp16 range guard (csrc/range.hpp) has no site in
 * it -- tests/test_capacity_cpu.py holds the unit to including neither csrc/tile.hpp nor csrc/range.hpp and to a listing without a
 * matrix instruction. */
int32_t trajsde_batch_pad_fits(const trajsde_batch* src, const trajsde_batch* dst);
int32_t trajsde_batch_pad(const trajsde_batch* src, const float* y, int32_t F, const trajsde_batch* dst, float* dst_y, int num_modes,
                          float local_radius, int32_t* fake_row_ids, int32_t* enc_row_ids, int32_t* dec_row_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRAJSDE_HIP_CAPACITY_H */

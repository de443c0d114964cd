// encoder_cot_bwd.hip -- trajsde_encoder_cotangent_backward (the kernel, then the entry point): the LocalEncoderSDESepPara2 stage's
// backward from caller-supplied cotangents of local_embed, diff_in and diff_out, with no loss formed inside
// (include/trajsde_hip_encoder_cotangent.h).  Everything behind the row vector DLDG[Nt] is the welded entry point's
// (encoder_bwd.hip encoder_backward_run: same launches, same arguments); this unit only produces DLDG from the two cotangents
// where trajsde_encoder_backward produces it from DiffBCE (k_diffbce).
//
//   k_diff_cot   DLDG[r] = sum over the 64 channels of the cotangent row of r's slot: the encoder's diffusion output is one sigmoid
//                value repeated over 64 channels (ENC:191-194), so its cotangent is the channel sum.  pick_slot[r] < 0: 0;
//                < A: row `slot` of d_diff_in; otherwise row `slot - A` of d_diff_out; a null side is zeros.
// No atomics: identical calls give identical words.  A separate unit so that the kernels of encoder_bwd.hip keep their listings.
#include "common.hpp"
#include "encoder_bwd_host.hpp"
#include "../../include/trajsde_hip_encoder_cotangent.h"

namespace tsde {

constexpr int DIFF_COT_THREADS = 256;

// A wave owns 64 consecutive rows, lane l the row r0 + l.  The rows that have a slot (2 A of the Nt) are taken one at a time, lowest
// lane first: the 64 lanes read the 64 channels of that slot's cotangent row -- one 256-byte line -- and add them up in an
// exclusive-or butterfly.  Partners exchange and add the same two words, and a + b = b + a holds exactly, so after the six levels
// every lane holds the same sum of the same fixed tree; the lane that owns the row keeps it.  Slots are validated against A, so
// neither a batch without fake agents (A = 0) nor a stray slot reads anything.
__global__ __launch_bounds__(DIFF_COT_THREADS) void k_diff_cot(const float* __restrict__ d_diff_in, const float* __restrict__ d_diff_out,
                                                               const int32_t* __restrict__ pick_slot, int Nt, int A,
                                                               float* __restrict__ DLDG) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = (int64_t(blockIdx.x) * (DIFF_COT_THREADS / 64) + (threadIdx.x >> 6)) * 64;
  if (r0 >= Nt) return;                                    // (whole waves leave: no barrier below)
  const int64_t r = r0 + lane;
  const int slot = r < Nt ? pick_slot[r] : -1;
  float mine = 0.f;
  unsigned long long todo = __ballot(slot >= 0);
  while (todo) {                                           // wave-uniform
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int s = __shfl(slot, src);
    const float* row = nullptr;
    if (s < A) {
      if (d_diff_in) row = d_diff_in + int64_t(s) * 64;
    } else if (s - A < A) {
      if (d_diff_out) row = d_diff_out + int64_t(s - A) * 64;
    }
    float v = row ? row[lane] : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == src) mine = v;
  }
  if (r < Nt) DLDG[r] = mine;
}

}  // namespace tsde

using namespace tsde;

extern "C" {

int trajsde_encoder_cotangent_backward(const trajsde_batch* b, const trajsde_graph* g, const float* rot, const float* blob_fwd,
                                       const float* blob_bwd, const float* step_tab /*HOST [H,8]*/, const float* step_tab_dev,
                                       const trajsde_noise* noise, const float* d_local, const float* d_diff_in, const float* d_diff_out,
                                       void* ws, int64_t ws_bytes, float* const* grads, int n_grads, float* d_latent, float* d_aa_out,
                                       const trajsde_dropout* dropout, int tape_valid, void* scratch, int64_t scratch_bytes, void* stream_) {
  if (int rc = refuse_retired_switches()) return rc;
  TS_REQUIRE(b && g && rot && blob_fwd && blob_bwd && step_tab && step_tab_dev && d_local && ws && grads,
             "encoder_cotangent_backward: null pointer");
  const DldgProducer cot = [&](const float*, float* DLDG, float*, hipStream_t st) -> int {
    TS_LAUNCH(k_diff_cot, cdiv(g->Nt, DIFF_COT_THREADS), DIFF_COT_THREADS, 0, st, d_diff_in, d_diff_out, g->pick_slot, g->Nt, b->A, DLDG);
    return TRAJSDE_OK;
  };
  return encoder_backward_run("encoder_cotangent_backward", b, g, rot, blob_fwd, blob_bwd, step_tab, step_tab_dev, noise, d_local, ws,
                              ws_bytes, grads, n_grads, d_latent, d_aa_out, dropout, tape_valid, scratch, scratch_bytes, stream_, cot);
}

}  // extern "C"

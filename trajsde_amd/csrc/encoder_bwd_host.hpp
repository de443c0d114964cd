// encoder_bwd_host.hpp -- the host side of the encoder backward that its two entry points share: trajsde_encoder_backward
// (encoder_bwd.hip: DiffBCE welded in) and trajsde_encoder_cotangent_backward (encoder_cot_bwd.hip: caller-supplied cotangents of
// diff_in / diff_out).  They differ in ONE launch, the producer of DLDG[Nt] = dL/d(picked diffusion value) per row; every launch behind
// it is issued by encoder_backward_run (encoder_bwd.hip) with the same arguments for both.  No device code in this header.
#pragma once
#include <functional>

#include "common.hpp"

namespace tsde {

// enqueues on `st` what fills DLDG[Nt] (0 for the rows without a slot).  GS: the tape's diffusion values [H][Nt]; scal: 64 floats of
// the backward's scratch.  Returns a TRAJSDE_* status.
using DldgProducer = std::function<int(const float* GS, float* DLDG, float* scal, hipStream_t st)>;

// the body of trajsde_encoder_backward (same arguments without diff_weight / diff_loss): argument checks (null pointers apart: the
// entry point's), tape (re)computation, ALEncoder chain, `dldg`, recurrence sweep, AAEncoder chain, the deferred sums.  `who` names
// the entry point in the refusals.
int encoder_backward_run(const char* who, const trajsde_batch* b, const trajsde_graph* g, const float* rot, const float* blob_fwd,
                         const float* blob_bwd, const float* step_tab /*HOST [H,8]*/, const float* step_tab_dev, const trajsde_noise* noise,
                         const float* d_local, void* ws, int64_t ws_bytes, float* const* grads, int n_grads, float* d_latent,
                         float* d_aa_out, const trajsde_dropout* dropout, int tape_valid, void* scratch, int64_t scratch_bytes,
                         void* stream, const DldgProducer& dldg);

}  // namespace tsde

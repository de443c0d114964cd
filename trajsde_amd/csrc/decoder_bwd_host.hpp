// decoder_bwd_host.hpp -- host side of the SDE decoder backward shared by its entry points: the welded ones (decoder_bwd.hip, where
// everything declared here is defined) and trajsde_decoder_cotangent_backward (decoder_cot_bwd.hip).  Declarations only.
#pragma once
#include "bwd.hpp"
#include "kernels.hpp"
#include "philox.hpp"

namespace tsde {

// gradient slots, in the order of trajsde_param_name(TRAJSDE_STAGE_DECODER_BWD, i)  (pack.hip recipe_decoder_bwd)
enum GradSlot {
  F0W = 0, F2W, F4W, G0W, G2W, G4W, D0W, D0B, D1W, D1B, D3W, D3B, A0W, A0B, A1W, A1B, F0B, F2B, F4B, G0B, G2B, G4B, N_GRADS,
  // TRAJSDE_STAGE_DECODER_NLL_BWD: the same table followed by the scale head (pack.hip recipe_decoder_nll_bwd)
  S0W = N_GRADS, S0B, S1W, S1B, S3W, S3B, N_GRADS_NLL,
  // TRAJSDE_STAGE_DECODER_COT_BWD: the NLL table followed by the pi head (pack.hip recipe_decoder_cot_bwd)
  P0W = N_GRADS_NLL, P0B, P1W, P1B, P3W, P3B, N_GRADS_COT
};
constexpr int BWD_THREADS = 128;
constexpr int64_t SHARED_VPART_FLOATS = int64_t(256) * (BWD_THREADS / 64) * 512;       // BwdWs: w.vpart

struct BwdWs {
  int32_t *best, *cnt;
  float *minsum, *scal, *states, *H1, *H2, *G1, *G2, *GS, *DH1, *DH2, *DF, *DG1, *DG2, *S_in, *DU, *DS, *gsel, *DA, *DY0, *part, *cs,
      *vpart, *DU2, *varena;
  MilRows mil;                                             // Milstein only: the sweep's extra rows (k_sde_bwd_mil)
  float *MW2, *MW0;                                        // ... and their two 64 x 64 weight-gradient blocks
  int64_t bytes, parts, varena_floats;
};
BwdWs carve_bwd(void* ws, int64_t ws_bytes, int N, int T, int n_euler, bool& ok, bool nll = false, bool mil = false);
int bwd_grid(int ntiles);
NoiseArg noise_arg(const trajsde_noise* noise);

// over the row domain (rows, K): path best[i] * rows + i of rows * K for every i < rows
int launch_replay(hipStream_t st, const float* blob_fwd, const BwdWs& w, int rows, int K, int n_euler, const float* step_table,
                  const NoiseArg& na, bool milstein);
int launch_sweep(hipStream_t st, const float* blob_bwd, const float* tan_img /* Milstein: the TanL image */, const BwdWs& w, int rows, int K,
                 int T, int n_euler, const float* step_table, const float* out_table, const NoiseArg& na, float* const* grads);
void head_colsums(ColsumBatch& cb, const float* v, float* const* head /* grads + D1W or grads + S1W */);
int sde_wgrads(const WgradCtx& wc, const BwdWs& w, int rows, int n_euler, float* const* grads, bool milstein);

}  // namespace tsde

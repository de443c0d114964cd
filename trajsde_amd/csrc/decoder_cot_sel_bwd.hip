// decoder_cot_sel_bwd.hip -- trajsde_decoder_cotangent_backward_sel (kernels, then the entry point at the end): the SDEDecoder's backward
// from caller-supplied cotangents dL/dloc [K,N,T,4] and dL/dpi [N,K] when dL/dloc is non-zero in at most ONE mode per actor -- any
// winner-takes-all regression loss next to a loss on pi.  The pi head does not depend on the SDE solution (DEC:93-94), so only the
// supported mode of each actor is replayed and swept: the welded entry points' row domain (N, K) with the selection read off the
// cotangent itself, instead of trajsde_decoder_cotangent_backward's (K * N, 1).
//
//   k_cot_support        per actor the modes whose dL/dloc rows hold a non-zero (or NaN) word: sel[n] = the lowest one (0 when there is
//                        none), per-wave counts of the actors with support / with more than one supported mode
//   k_cot_support_sum    the counts' sums in a fixed order -> status[0] (more than one mode), status[1] (supported)
//   k_head_bwd_cot_sel   the cotangent head pass (head_cot.hpp) over N rows: row n reads loc / d_loc at path sel[n] * N + n and the saved
//                        states of the selected replay at row n
// Everything else is shared: k_init_sel / k_dec_init_bwd of the welded route (decoder_bwd.hip), the replay, the sweep and the SDE weight
// gradients over (N, K, sel) (decoder_bwd_host.hpp), k_pi_head_bwd over all K modes (decoder_cot_bwd.hip).  No atomics: identical calls
// give identical words.  A separate unit so that the kernels of the other decoder-backward units keep their listings.
#include "common.hpp"
#include "layouts.hpp"
#include "tile.hpp"
#include "tile_bwd.hpp"
#include "bwd.hpp"
#include "decoder_bwd_host.hpp"
#include "head_cot.hpp"
#include "../../include/trajsde_hip_cotangent_sel.h"

namespace tsde {

constexpr int SUP_ACTORS = 16;             // actors one wave of k_cot_support scans: the row tile of the kernels that read sel
constexpr int SUP_THREADS = 256;

// d_loc is [K][N][T] records of four floats.  A wave owns SUP_ACTORS consecutive actors: in mode k their records are one contiguous run of
// (actors x T) x 16 bytes, which the lanes walk 64 records at a time.  A lane keeps one bit per actor of the group; the bits are OR-ed
// over the wave (order does not matter to an OR), then lane a < SUP_ACTORS tracks actor a over the modes.  part is [groups][2].
__global__ __launch_bounds__(SUP_THREADS) void k_cot_support(const float* __restrict__ d_loc, int N, int K, int T, int32_t* __restrict__ sel,
                                                             int32_t* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int group = blockIdx.x * (SUP_THREADS / 64) + (threadIdx.x >> 6);
  const int groups = (N + SUP_ACTORS - 1) / SUP_ACTORS;
  if (group >= groups) return;                             // (whole waves leave: no barrier below)
  const int n0 = group * SUP_ACTORS;
  const int actors = N - n0 < SUP_ACTORS ? N - n0 : SUP_ACTORS;
  const int recs = actors * T;
  int first = -1, count = 0;                               // lane a: lowest supported mode of actor n0 + a, number of supported modes
  for (int k = 0; k < K; ++k) {
    const f4* run = reinterpret_cast<const f4*>(d_loc) + (int64_t(k) * N + n0) * T;
    int bits = 0;
    for (int r = lane; r < recs; r += 64) {
      const f4 v = run[r];
      // NaN != 0.0f holds too: a NaN cotangent is support, and reaches the gradients as it does on the dense route
      if (v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f || v[3] != 0.0f) bits |= 1 << (r / T);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off);
    if ((bits >> (lane & (SUP_ACTORS - 1))) & 1) {
      if (first < 0) first = k;
      ++count;
    }
  }
  const bool mine = lane < actors;
  if (mine) sel[n0 + lane] = first < 0 ? 0 : first;
  const int many = __popcll(__ballot(mine && count > 1)), some = __popcll(__ballot(mine && count > 0));
  if (lane < 2) part[int64_t(group) * 2 + lane] = lane == 0 ? many : some;
}

// status[c] = sum over the groups of part[g][c]: every thread a strided run in group order, then a tree over the workgroup
__global__ __launch_bounds__(SUP_THREADS) void k_cot_support_sum(const int32_t* __restrict__ part, int groups, int32_t* __restrict__ status) {
  __shared__ int32_t red[2][SUP_THREADS];
  int32_t many = 0, some = 0;
  for (int g = threadIdx.x; g < groups; g += SUP_THREADS) {
    many += part[int64_t(g) * 2];
    some += part[int64_t(g) * 2 + 1];
  }
  red[0][threadIdx.x] = many;
  red[1][threadIdx.x] = some;
  __syncthreads();
  for (int w = SUP_THREADS / 2; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) status[threadIdx.x] = red[threadIdx.x][0];
}

// k_head_bwd_cot (decoder_cot_bwd.hip) over the row domain N: rows are (o, n), o = output step, n = actor.  states / S_in / DU / DU2 / DS
// are the selected replay's [.][N][64]; loc / d_loc are [K * N][T][4], read at path sel[n] * N + n
__global__ __launch_bounds__(128) void k_head_bwd_cot_sel(const float* __restrict__ img_loc, const float* __restrict__ img_sc,
                                                          const float* __restrict__ states, const float* __restrict__ out_tab,
                                                          const float* __restrict__ loc, const float* __restrict__ d_loc,
                                                          const int32_t* __restrict__ sel, float min_scale, int N, int T,
                                                          float* __restrict__ S_in, float* __restrict__ DU, float* __restrict__ DU2,
                                                          float* __restrict__ DS, float* __restrict__ vpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_copy(lds, img_loc, HeadBwdL::SIZE);
  stage_copy(lds + HeadBwdL::SIZE, img_sc, HeadBwdL::SIZE);
  __syncthreads();
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int tiles_per_o = (N + 15) / 16;
  const int ntiles = tiles_per_o * T;
  const int64_t slab = int64_t(N) * D;
  HeadAcc AL, AS;
  head_acc_zero(AL);
  head_acc_zero(AS);
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    keep_lds_reads_here();
    const int o = tile / tiles_per_o;
    const int row = (tile - o * tiles_per_o) * 16 + L.n;
    const int i = row < N ? row : N - 1;
    const int ko = int(out_tab[o * 4]);
    const float w0 = out_tab[o * 4 + 1], w1 = out_tab[o * 4 + 2];
    f4 g = f4{0.f, 0.f, 0.f, 0.f};
    if (row < N) {
      const int64_t rec = ((int64_t(sel[i]) * N + i) * T + o) * 4;
      g = *reinterpret_cast<const f4*>(d_loc + rec);
      const f4 fw = *reinterpret_cast<const f4*>(loc + rec);
      // scale = ELU(raw) + 1 + min_scale (DEC:97-98): d scale / d raw = 1 for raw > 0, else exp(raw) = scale - min_scale (< = 1)
      g[2] *= fminf(1.0f, fw[2] - min_scale);
      g[3] *= fminf(1.0f, fw[3] - min_scale);
    }
    f4 s[4];
    {
      f4 a[4], b[4];
      load_row(a, states + (ko - 1) * slab, i, L.g);
      load_row(b, states + ko * slab, i, L.g);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[jt][c] = w0 * a[jt][c] + w1 * b[jt][c];
    }
    f4 du[4], ds[4];
    zero4(ds);
    head_cot_pass(lds, s, g[0], g[1], AL, du, ds, L);
    if (row < N) {
      store_row(s, S_in + o * slab, row, L.g);
      store_row(du, DU + o * slab, row, L.g);
    }
    head_cot_pass(lds + HeadBwdL::SIZE, s, g[2], g[3], AS, du, ds, L);
    if (row < N) {
      store_row(du, DU2 + o * slab, row, L.g);
      store_row(ds, DS + o * slab, row, L.g);
    }
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * CotHeadV::SIZE;
  head_acc_flush(AL, vp + CotHeadV::LOC, L);
  head_acc_flush(AS, vp + CotHeadV::SCALE, L);
}

// ------------------------------------------------------------------ host side
// the Laplace NLL workspace over N rows (the selection is its `best`, the first words of the workspace), then the pi head's delta rows
// over all K * N paths, their mode sums and the support counts of k_cot_support
struct CotSelWs {
  BwdWs w;
  float *DP, *DPS;
  int32_t* sup;
  int64_t bytes;
};
static CotSelWs carve_cot_sel(void* ws, int64_t ws_bytes, int N, int K, int T, int n_euler, bool& ok) {
  CotSelWs c;
  c.w = carve_bwd(ws, ws_bytes, N, T, n_euler, ok, true);
  Carver cv(ws ? reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(ws) + uintptr_t(c.w.bytes)) : nullptr, ws_bytes - c.w.bytes);
  c.DP = cv.take<float>(int64_t(N) * K * 64);
  c.DPS = cv.take<float>(int64_t(N) * 64);
  c.sup = cv.take<int32_t>(int64_t(cdiv(N, SUP_ACTORS)) * 2);
  c.bytes = c.w.bytes + cv.off + 256;
  ok = ok && cv.ok;
  return c;
}

// the dense entry point's bound: the pi head and its weight gradient walk K * N rows with 32-bit row indices
static bool cot_sel_rows_ok(int32_t N, int K, int T, int n_euler) {
  return N > 0 && K > 0 && T > 0 && n_euler > 0 && int64_t(N) * K * (T > n_euler ? T : n_euler) < (int64_t(1) << 31) - 64;
}

}  // namespace tsde

using namespace tsde;

extern "C" {

int64_t trajsde_decoder_cotangent_backward_sel_ws_bytes(int32_t N, int num_modes, int future_steps, int n_euler) {
  if (!cot_sel_rows_ok(N, num_modes, future_steps, n_euler))
    return fail(TRAJSDE_ERR_INVALID, "decoder_cotangent_backward_sel: empty or oversized problem");
  bool ok;
  return carve_cot_sel(nullptr, 0, N, num_modes, future_steps, n_euler, ok).bytes;
}

int trajsde_decoder_cotangent_backward_sel(int32_t N, int num_modes, int future_steps, const float* blob_fwd, const float* blob_bwd,
                                           const float* local_embed, const float* global_embed, const float* step_table, int n_euler,
                                           const float* out_table, const trajsde_noise* noise, const float* loc, float min_scale,
                                           const float* d_loc, const float* d_pi, void* ws, int64_t ws_bytes, float* const* grads,
                                           int n_grads, float* d_local, float* d_global, int32_t* status, void* stream_) {
  TS_REQUIRE(blob_fwd && blob_bwd && local_embed && global_embed && step_table && out_table && loc && d_loc && d_pi && ws && grads &&
                 d_local && d_global && status,
             "decoder_cotangent_backward_sel: null pointer");
  TS_REQUIRE(cot_sel_rows_ok(N, num_modes, future_steps, n_euler), "decoder_cotangent_backward_sel: empty or oversized problem");
  TS_REQUIRE(n_grads == int(N_GRADS_COT),
             "decoder_cotangent_backward_sel: gradient count does not match trajsde_param_count(TRAJSDE_STAGE_DECODER_COT_BWD)");
  for (int i = 0; i < int(N_GRADS_COT); ++i) TS_REQUIRE(grads[i] != nullptr, "decoder_cotangent_backward_sel: null gradient buffer");
  if (state_bf16())
    return fail(TRAJSDE_ERR_UNSUPPORTED,
                "decoder_cotangent_backward_sel: trajsde_state_storage(1) is not supported (the replay keeps fp32 states)");
  if (ws_bytes < trajsde_decoder_cotangent_backward_sel_ws_bytes(N, num_modes, future_steps, n_euler))
    return fail(TRAJSDE_ERR_WORKSPACE, "decoder_cotangent_backward_sel: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  bool ok;
  const int K = num_modes, T = future_steps, NN = N * K;
  const CotSelWs cw = carve_cot_sel(ws, ws_bytes, N, K, T, n_euler, ok);
  const BwdWs& w = cw.w;
  DeferredSums sums(st, w.part, w.cs, w.parts, step_table, w.varena, w.varena_floats);
  const NoiseArg na = noise_arg(noise);
  const int ntiles = (N + 15) / 16;
  const int waves = BWD_THREADS / 64;
  int rc;

  // ---- the supported mode of every actor, read off the cotangent
  const int groups = cdiv(N, SUP_ACTORS);
  TS_LAUNCH(k_cot_support, cdiv(groups, SUP_THREADS / 64), SUP_THREADS, 0, st, d_loc, N, K, T, w.best, cw.sup);
  TS_LAUNCH(k_cot_support_sum, 1, SUP_THREADS, 0, st, cw.sup, groups, status);

  // ---- replay of the selected paths: the welded route's domain (path sel[n] * N + n of N * K: the forward's Philox counter)
  const float* init_img = blob_bwd + DecBwdBlob::INIT;
  TS_LAUNCH(k_init_sel, bwd_grid(ntiles), BWD_THREADS, InitBwdL::AE_END * 4, st, init_img, local_embed, global_embed, w.best, N, w.states,
            w.gsel);
  if ((rc = launch_replay(st, blob_fwd, w, N, K, n_euler, step_table, na, false))) return rc;

  // ---- both heads from the selected mode's cotangent, one pass over the saved states
  int head_grid = bwd_grid(ntiles * T);
  if (int64_t(head_grid) * waves * CotHeadV::SIZE > SHARED_VPART_FLOATS) head_grid = int(SHARED_VPART_FLOATS / (waves * CotHeadV::SIZE));
  const int head_waves = head_grid * waves;
  float* vp = vpart_slab(w.vpart, head_waves, CotHeadV::SIZE);
  TS_LAUNCH(k_head_bwd_cot_sel, head_grid, BWD_THREADS, 2 * HeadBwdL::SIZE * 4, st, blob_bwd + DecBwdBlob::HEAD,
            blob_bwd + DecNllBwdBlob::HEAD_SC, w.states, out_table, loc, d_loc, w.best, min_scale, N, T, w.S_in, w.DU, w.DU2, w.DS, vp);
  {
    ColsumBatch cb(st, head_waves, CotHeadV::SIZE);
    head_colsums(cb, vp + CotHeadV::LOC, grads + D1W);
    head_colsums(cb, vp + CotHeadV::SCALE, grads + S1W);
    if ((rc = cb.flush())) return rc;
  }

  // ---- reverse sweep of the selected paths
  if ((rc = launch_sweep(st, blob_bwd, nullptr, w, N, K, T, n_euler, step_table, out_table, na, grads))) return rc;

  // ---- aggr_embed of the selected mode (overwrites d_local and, over zeros, row sel[n] * N + n of d_global), then the pi head over all
  //      K modes (adds to both)
  const int init_grid = bwd_grid(ntiles);
  TS_HIP(hipMemsetAsync(d_global, 0, size_t(NN) * 64 * sizeof(float), st));
  vp = vpart_slab(w.vpart, int64_t(init_grid) * waves, InitV::SIZE);
  TS_LAUNCH(k_dec_init_bwd, init_grid, BWD_THREADS, InitBwdL::SIZE * 4, st, init_img, local_embed, w.gsel, w.DY0, w.best, N, w.DA, d_local,
            d_global, vp);
  {
    ColsumBatch cb(st, init_grid * waves, InitV::SIZE);
    cb.add(vp + InitV::DGAM, 64, grads[A1W]);
    cb.add(vp + InitV::DBET, 64, grads[A1B]);
    if ((rc = cb.flush())) return rc;
  }
  vp = vpart_slab(w.vpart, int64_t(init_grid) * waves, PiV::SIZE);
  TS_LAUNCH(k_pi_head_bwd, init_grid, BWD_THREADS, PiBwdL::SIZE * 4, st, blob_bwd + DecCotBwdBlob::PI, local_embed, global_embed, d_pi, N, K,
            cw.DP, cw.DPS, d_local, d_global, vp);
  {
    ColsumBatch cb(st, init_grid * waves, PiV::SIZE);
    cb.add(vp + PiV::DGAM, 64, grads[P1W]);
    cb.add(vp + PiV::DBET, 64, grads[P1B]);
    cb.add(vp + PiV::DW3, 64, grads[P3W]);
    cb.add(vp + PiV::DB3, 1, grads[P3B]);
    if ((rc = cb.flush())) return rc;
  }

  // ---- weight gradients
  const WgradCtx wc{st, w.part, w.cs, step_table, w.parts};
  const int64_t RT = int64_t(N) * T;
  if ((rc = sde_wgrads(wc, w, N, n_euler, grads, false))) return rc;
  {
    WgradBatch heads(wc, RT, RT);                           // the two heads' first layers over the same (output step, actor) rows
    if ((rc = heads.add(w.DU, 64, w.S_in, 64, grads[D0W], 64, 0, grads[D0B], 0))) return rc;
    if ((rc = heads.add(w.DU2, 64, w.S_in, 64, grads[S0W], 64, 0, grads[S0B], 0))) return rc;
    if ((rc = heads.flush())) return rc;
  }
  {
    WgradBatch rows(wc, N, N);                              // aggr_embed.0 = cat(global, local) on the selected rows; pi.0's local half
    if ((rc = rows.add(w.DA, 64, w.gsel, 64, grads[A0W], 128, 0, grads[A0B], 0))) return rc;
    if ((rc = rows.add(w.DA, 64, local_embed, 64, grads[A0W], 128, 64, nullptr, 0))) return rc;
    if ((rc = rows.add(cw.DPS, 64, local_embed, 64, grads[P0W], 128, 0, nullptr, 0))) return rc;
    if ((rc = rows.flush())) return rc;
  }
  if ((rc = run_wgrad(wc, cw.DP, 64, global_embed, 64, NN, NN, grads[P0W], 128, 64, grads[P0B], 0))) return rc;   // pi.0's global half
  return sums.finish();
}

}  // extern "C"

// decoder_cot_bwd.hip -- trajsde_decoder_cotangent_backward (kernels, then the entry point at the end), the SDEDecoder's backward from
// caller-supplied cotangents dL/dloc [K,N,T,4] and dL/dpi [N,K] for gfx950.  Every one of the K * N paths carries gradient, so the
// replay and the reverse sweep of decoder_bwd.hip / recur.hip run over a row domain of K * N with the identity selection (row
// r = k * N + n is path r: the forward's Philox counter); what is new here is what the welded entry points fuse with their loss or
// restrict to the winning mode:
//
//   k_init_all           y0 of all K * N paths                                   (aggr_embed, DEC:82; local row n = r % N)
//   k_head_bwd_cot       loc AND scale head, forward + backward per (row, output step) in one pass over the saved states: the upstream
//                        gradient is read from d_loc instead of formed against y; the scale channels pass through ELU + 1 + min_scale
//   k_dec_init_bwd_all   aggr_embed backward over all modes; d local_embed = the modes' sum in mode order
//   k_pi_head_bwd        pi head Linear(128,64) LN ReLU Linear(64,1) on [local | global] rows (DEC:93-94), forward + backward; ADDS its
//                        input gradients to d_local / d_global
//
// The mode sums into d_local run inside ONE wave per 16 actors, modes 0..K-1 in order: no atomics, identical calls give identical words.
// A separate unit so that the kernels of decoder_bwd.hip keep their listings.  The host side shares the replay, the sweep and the SDE
// weight gradients with the welded entry points (decoder_bwd_host.hpp, defined in decoder_bwd.hip).
#include "common.hpp"
#include "layouts.hpp"
#include "range.hpp"
#include "tile.hpp"
#include "tile_bwd.hpp"
#include "bwd.hpp"
#include "decoder_bwd_host.hpp"
#include "head_cot.hpp"

namespace tsde {

__global__ __launch_bounds__(128) void k_init_all(const float* __restrict__ img, const float* __restrict__ local,
                                                  const float* __restrict__ global, int N, int K, float* __restrict__ y0) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, InitBwdL::AE_END);
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int NN = N * K;
  const int ntiles = (NN + 15) / 16;
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    keep_lds_reads_here();
    const int row = tile * 16 + L.n;
    const int r = row < NN ? row : NN - 1;
    f4 gl[4], lo[4], a[4];
    load_row(gl, global, r, L.g);
    load_row(lo, local, r % N, L.g);
    range_note(fmaxf(absmax<4>(gl), absmax<4>(lo)), RS_DEC_INPUT);   // the caller's rows: no forward call has to precede a backward one
    load_vec<4>(a, lds + InitBwdL::BA, L.g);
    linear_acc<4, 4>(a, gl, lds + InitBwdL::WA_G, L.lane);
    linear_acc<4, 4>(a, lo, lds + InitBwdL::WA_L, L.lane);
    layer_norm<4>(a, lds + InitBwdL::AG, lds + InitBwdL::AE, L.g);
    relu<4>(a);
    if (row < NN) store_row(a, y0, row, L.g);
  }
}

// rows are (o, r): o = output step, r = path (k * N + n) of NN = K * N.  S_in / DU / DU2 / DS are [T][NN][64]; loc / d_loc are [NN][T][4]
__global__ __launch_bounds__(128) void k_head_bwd_cot(const float* __restrict__ img_loc, const float* __restrict__ img_sc,
                                                      const float* __restrict__ states, const float* __restrict__ out_tab,
                                                      const float* __restrict__ loc, const float* __restrict__ d_loc, float min_scale, int NN,
                                                      int T, float* __restrict__ S_in, float* __restrict__ DU, float* __restrict__ DU2,
                                                      float* __restrict__ DS, float* __restrict__ vpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_copy(lds, img_loc, HeadBwdL::SIZE);
  stage_copy(lds + HeadBwdL::SIZE, img_sc, HeadBwdL::SIZE);
  __syncthreads();
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int tiles_per_o = (NN + 15) / 16;
  const int ntiles = tiles_per_o * T;
  const int64_t slab = int64_t(NN) * D;
  HeadAcc AL, AS;
  head_acc_zero(AL);
  head_acc_zero(AS);
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    keep_lds_reads_here();
    const int o = tile / tiles_per_o;
    const int row = (tile - o * tiles_per_o) * 16 + L.n;
    const int i = row < NN ? row : NN - 1;
    const int ko = int(out_tab[o * 4]);
    const float w0 = out_tab[o * 4 + 1], w1 = out_tab[o * 4 + 2];
    f4 g = f4{0.f, 0.f, 0.f, 0.f};
    if (row < NN) {
      g = *reinterpret_cast<const f4*>(d_loc + (int64_t(i) * T + o) * 4);
      const f4 fw = *reinterpret_cast<const f4*>(loc + (int64_t(i) * T + o) * 4);
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
    if (row < NN) {
      store_row(s, S_in + o * slab, row, L.g);
      store_row(du, DU + o * slab, row, L.g);
    }
    head_cot_pass(lds + HeadBwdL::SIZE, s, g[2], g[3], AS, du, ds, L);
    if (row < NN) {
      store_row(du, DU2 + o * slab, row, L.g);
      store_row(ds, DS + o * slab, row, L.g);
    }
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * CotHeadV::SIZE;
  head_acc_flush(AL, vp + CotHeadV::LOC, L);
  head_acc_flush(AS, vp + CotHeadV::SCALE, L);
}

// aggr_embed backward over all modes: one wave per 16 actors walks the modes in order.  DY0 / DA / d_global are [K][N][64]; DAS [N][64] is
// the modes' sum of DA (the delta rows of the weight's local half, whose input row does not depend on the mode)
__global__ __launch_bounds__(128) void k_dec_init_bwd_all(const float* __restrict__ img, const float* __restrict__ local,
                                                          const float* __restrict__ global, const float* __restrict__ DY0, int N, int K,
                                                          float* __restrict__ DA, float* __restrict__ DAS, float* __restrict__ d_local,
                                                          float* __restrict__ d_global, float* __restrict__ vpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, InitBwdL::SIZE);
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int ntiles = (N + 15) / 16;
  f4 dgam[4], dbet[4];
  zero4(dgam); zero4(dbet);
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    const int row = tile * 16 + L.n;
    const int i = row < N ? row : N - 1;
    f4 lo[4], das[4];
    load_row(lo, local, i, L.g);
    zero4(das);
    for (int k = 0; k < K; ++k) {
      keep_lds_reads_here();
      const int64_t r = int64_t(k) * N + i;
      f4 gl[4], a[4], d[4];
      load_row(gl, global, r, L.g);
      load_vec<4>(a, lds + InitBwdL::BA, L.g);
      linear_acc<4, 4>(a, gl, lds + InitBwdL::WA_G, L.lane);
      linear_acc<4, 4>(a, lo, lds + InitBwdL::WA_L, L.lane);
      const float rstd = ln_normalize(a);
      load_row(d, DY0, r, L.g);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f4 ga = *reinterpret_cast<const f4*>(lds + InitBwdL::AG + 16 * jt + 4 * L.g);
        const f4 be = *reinterpret_cast<const f4*>(lds + InitBwdL::AE + 16 * jt + 4 * L.g);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (!(a[jt][c] * ga[c] + be[c] > 0.f) || row >= N) d[jt][c] = 0.f;
      }
      ln_backward(d, a, rstd, lds + InitBwdL::AG, L.g, dgam, dbet);   // d := d a_pre
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) das[jt] += d[jt];
      f4 t[4];
      linear_t(t, d, lds + InitBwdL::WA_GT, L);
      if (row < N) {
        store_row(d, DA, r, L.g);
        store_row(t, d_global, r, L.g);
      }
    }
    f4 t[4];
    linear_t(t, das, lds + InitBwdL::WA_LT, L);
    if (row < N) {
      store_row(das, DAS, row, L.g);
      store_row(t, d_local, row, L.g);
    }
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * InitV::SIZE;
  flush_vec(dgam, vp + InitV::DGAM, L);
  flush_vec(dbet, vp + InitV::DBET, L);
}

// pi head forward + backward, after k_dec_init_bwd_all on the same stream: d_global rows and d_local rows are read, added to and written
// back by the one wave that owns the actor.  d_pi is [N][K] (the forward's transposed layout, DEC:94); DP [K][N][64] are the delta rows
// of pi.0's global half, DPS [N][64] their sum over the modes (the local half)
__global__ __launch_bounds__(128) void k_pi_head_bwd(const float* __restrict__ img, const float* __restrict__ local,
                                                     const float* __restrict__ global, const float* __restrict__ d_pi, int N, int K,
                                                     float* __restrict__ DP, float* __restrict__ DPS, float* __restrict__ d_local,
                                                     float* __restrict__ d_global, float* __restrict__ vpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, PiBwdL::SIZE);
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int ntiles = (N + 15) / 16;
  f4 dgam[4], dbet[4], dw3[4];
  zero4(dgam); zero4(dbet); zero4(dw3);
  float db3 = 0.f;
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    const int row = tile * 16 + L.n;
    const int i = row < N ? row : N - 1;
    f4 lo[4], dps[4];
    load_row(lo, local, i, L.g);
    zero4(dps);
    for (int k = 0; k < K; ++k) {
      keep_lds_reads_here();
      const int64_t r = int64_t(k) * N + i;
      const float g = row < N ? d_pi[int64_t(i) * K + k] : 0.f;
      f4 gl[4], a[4], d[4];
      load_row(gl, global, r, L.g);
      load_vec<4>(a, lds + PiBwdL::BP, L.g);
      linear_acc<4, 4>(a, lo, lds + PiBwdL::WP_L, L.lane);
      linear_acc<4, 4>(a, gl, lds + PiBwdL::WP_G, L.lane);
      const float rstd = ln_normalize(a);
      db3 += g;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f4 ga = *reinterpret_cast<const f4*>(lds + PiBwdL::PG + 16 * jt + 4 * L.g);
        const f4 be = *reinterpret_cast<const f4*>(lds + PiBwdL::PE + 16 * jt + 4 * L.g);
        const f4 w3 = *reinterpret_cast<const f4*>(lds + PiBwdL::WP3 + 16 * jt + 4 * L.g);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float pre = a[jt][c] * ga[c] + be[c];
          dw3[jt][c] = fmaf(g, fmaxf(pre, 0.f), dw3[jt][c]);
          d[jt][c] = pre > 0.f ? g * w3[c] : 0.f;
        }
      }
      ln_backward(d, a, rstd, lds + PiBwdL::PG, L.g, dgam, dbet);     // d := gradient at pi.0's output
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) dps[jt] += d[jt];
      f4 t[4];
      if (row < N) load_row(t, d_global, r, L.g);
      else zero4(t);
      linear_adj<4, 4>(t, d, lds + PiBwdL::WP_GT, L);
      if (row < N) {
        store_row(d, DP, r, L.g);
        store_row(t, d_global, r, L.g);
      }
    }
    f4 t[4];
    if (row < N) load_row(t, d_local, row, L.g);
    else zero4(t);
    linear_adj<4, 4>(t, dps, lds + PiBwdL::WP_LT, L);
    if (row < N) {
      store_row(dps, DPS, row, L.g);
      store_row(t, d_local, row, L.g);
    }
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * PiV::SIZE;
  flush_vec(dgam, vp + PiV::DGAM, L);
  flush_vec(dbet, vp + PiV::DBET, L);
  flush_vec(dw3, vp + PiV::DW3, L);
  flush_scalar(db3, vp + PiV::DB3, L);
}

// ------------------------------------------------------------------ host side
// trajsde_decoder_cotangent_backward: the Laplace NLL workspace over a row domain of K * N (every path is replayed and swept), then the
// pi head's delta rows and the two mode sums of delta rows whose input row is the actor's local embedding
struct CotWs {
  BwdWs w;
  float *DP, *DAS, *DPS;
  int64_t bytes;
};
static CotWs carve_cot(void* ws, int64_t ws_bytes, int N, int K, int T, int n_euler, bool& ok) {
  CotWs c;
  const int NN = N * K;
  c.w = carve_bwd(ws, ws_bytes, NN, T, n_euler, ok, true);
  Carver cv(ws ? reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(ws) + uintptr_t(c.w.bytes)) : nullptr, ws_bytes - c.w.bytes);
  c.DP = cv.take<float>(int64_t(NN) * 64);
  c.DAS = cv.take<float>(int64_t(N) * 64);
  c.DPS = cv.take<float>(int64_t(N) * 64);
  c.bytes = c.w.bytes + cv.off + 256;
  ok = ok && cv.ok;
  return c;
}

// the largest K * N * max(T, n_euler) the row indices of the kernels hold (tiles and rows are 32-bit there, offsets 64-bit)
static bool cot_rows_ok(int32_t N, int K, int T, int n_euler) {
  return N > 0 && K > 0 && T > 0 && n_euler > 0 && int64_t(N) * K * (T > n_euler ? T : n_euler) < (int64_t(1) << 31) - 64;
}

}  // namespace tsde

using namespace tsde;

extern "C" {

int64_t trajsde_decoder_cotangent_backward_ws_bytes(int32_t N, int num_modes, int future_steps, int n_euler) {
  if (!cot_rows_ok(N, num_modes, future_steps, n_euler)) return fail(TRAJSDE_ERR_INVALID, "decoder_cotangent_backward: empty or oversized problem");
  bool ok;
  return carve_cot(nullptr, 0, N, num_modes, future_steps, n_euler, ok).bytes;
}

int trajsde_decoder_cotangent_backward(int32_t N, int num_modes, int future_steps, const float* blob_fwd, const float* blob_bwd,
                                       const float* local_embed, const float* global_embed, const float* step_table, int n_euler,
                                       const float* out_table, const trajsde_noise* noise, const float* loc, float min_scale,
                                       const float* d_loc, const float* d_pi, void* ws, int64_t ws_bytes, float* const* grads, int n_grads,
                                       float* d_local, float* d_global, void* stream_) {
  TS_REQUIRE(blob_fwd && blob_bwd && local_embed && global_embed && step_table && out_table && loc && d_loc && d_pi && ws && grads &&
                 d_local && d_global,
             "decoder_cotangent_backward: null pointer");
  TS_REQUIRE(cot_rows_ok(N, num_modes, future_steps, n_euler), "decoder_cotangent_backward: empty or oversized problem");
  TS_REQUIRE(n_grads == int(N_GRADS_COT),
             "decoder_cotangent_backward: gradient count does not match trajsde_param_count(TRAJSDE_STAGE_DECODER_COT_BWD)");
  for (int i = 0; i < int(N_GRADS_COT); ++i) TS_REQUIRE(grads[i] != nullptr, "decoder_cotangent_backward: null gradient buffer");
  if (state_bf16())
    return fail(TRAJSDE_ERR_UNSUPPORTED, "decoder_cotangent_backward: trajsde_state_storage(1) is not supported (the replay keeps fp32 states)");
  if (ws_bytes < trajsde_decoder_cotangent_backward_ws_bytes(N, num_modes, future_steps, n_euler))
    return fail(TRAJSDE_ERR_WORKSPACE, "decoder_cotangent_backward: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  bool ok;
  const int K = num_modes, T = future_steps, NN = N * K;
  const CotWs cw = carve_cot(ws, ws_bytes, N, K, T, n_euler, ok);
  const BwdWs& w = cw.w;
  DeferredSums sums(st, w.part, w.cs, w.parts, step_table, w.varena, w.varena_floats);
  const NoiseArg na = noise_arg(noise);
  const int ntiles = (NN + 15) / 16, atiles = (N + 15) / 16;
  const int waves = BWD_THREADS / 64;
  int rc;

  // ---- replay of every path: the replay and sweep kernels select path best[i] * N' + i of N' * K' -- the identity over N' = K * N, K' = 1
  TS_HIP(hipMemsetAsync(w.best, 0, sizeof(int32_t) * NN, st));
  const float* init_img = blob_bwd + DecBwdBlob::INIT;
  TS_LAUNCH(k_init_all, bwd_grid(ntiles), BWD_THREADS, InitBwdL::AE_END * 4, st, init_img, local_embed, global_embed, N, K, w.states);
  if ((rc = launch_replay(st, blob_fwd, w, NN, 1, n_euler, step_table, na, false))) return rc;

  // ---- both heads from the cotangent, one pass over the saved states
  int head_grid = bwd_grid(ntiles * T);
  if (int64_t(head_grid) * waves * CotHeadV::SIZE > SHARED_VPART_FLOATS) head_grid = int(SHARED_VPART_FLOATS / (waves * CotHeadV::SIZE));
  const int head_waves = head_grid * waves;
  float* vp = vpart_slab(w.vpart, head_waves, CotHeadV::SIZE);
  TS_LAUNCH(k_head_bwd_cot, head_grid, BWD_THREADS, 2 * HeadBwdL::SIZE * 4, st, blob_bwd + DecBwdBlob::HEAD, blob_bwd + DecNllBwdBlob::HEAD_SC,
            w.states, out_table, loc, d_loc, min_scale, NN, T, w.S_in, w.DU, w.DU2, w.DS, vp);
  {
    ColsumBatch cb(st, head_waves, CotHeadV::SIZE);
    head_colsums(cb, vp + CotHeadV::LOC, grads + D1W);
    head_colsums(cb, vp + CotHeadV::SCALE, grads + S1W);
    if ((rc = cb.flush())) return rc;
  }

  // ---- reverse sweep of every path
  if ((rc = launch_sweep(st, blob_bwd, nullptr, w, NN, 1, T, n_euler, step_table, out_table, na, grads))) return rc;

  // ---- aggr_embed over all modes (overwrites d_local, d_global), then the pi head (adds to both)
  const int init_grid = bwd_grid(atiles);
  vp = vpart_slab(w.vpart, int64_t(init_grid) * waves, InitV::SIZE);
  TS_LAUNCH(k_dec_init_bwd_all, init_grid, BWD_THREADS, InitBwdL::SIZE * 4, st, init_img, local_embed, global_embed, w.DY0, N, K, w.DA, cw.DAS,
            d_local, d_global, vp);
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
  const int64_t RT = int64_t(NN) * T;
  if ((rc = sde_wgrads(wc, w, NN, n_euler, grads, false))) return rc;
  {
    WgradBatch heads(wc, RT, RT);                           // the two heads' first layers over the same (output step, path) rows
    if ((rc = heads.add(w.DU, 64, w.S_in, 64, grads[D0W], 64, 0, grads[D0B], 0))) return rc;
    if ((rc = heads.add(w.DU2, 64, w.S_in, 64, grads[S0W], 64, 0, grads[S0B], 0))) return rc;
    if ((rc = heads.flush())) return rc;
  }
  {
    WgradBatch glob(wc, NN, NN);                            // the global halves: aggr_embed.0 = cat(global, local), pi.0 = cat(local, global)
    if ((rc = glob.add(w.DA, 64, global_embed, 64, grads[A0W], 128, 0, grads[A0B], 0))) return rc;
    if ((rc = glob.add(cw.DP, 64, global_embed, 64, grads[P0W], 128, 64, grads[P0B], 0))) return rc;
    if ((rc = glob.flush())) return rc;
  }
  {
    WgradBatch loc_(wc, N, N);                              // the local halves: the mode-summed delta rows against the actors' rows
    if ((rc = loc_.add(cw.DAS, 64, local_embed, 64, grads[A0W], 128, 64, nullptr, 0))) return rc;
    if ((rc = loc_.add(cw.DPS, 64, local_embed, 64, grads[P0W], 128, 0, nullptr, 0))) return rc;
    if ((rc = loc_.flush())) return rc;
  }
  return sums.finish();
}

}  // extern "C"

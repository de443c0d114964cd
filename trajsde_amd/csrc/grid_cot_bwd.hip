// grid_cot_bwd.hip -- trajsde_mlp_decoder_cotangent_backward: the vanilla HiVT variant's MLPDecoder (GDEC:47-63) differentiated from
// caller-supplied cotangents dL/dloc [K,N,T,4] and dL/dpi [N,K] for gfx950.  No loss is formed inside and every one of the K * N rows
// (r = k * N + n) carries gradient, where grid_bwd.hip fuses L2 / the Laplace NLL and differentiates the winning mode's N rows only.
//
//   k_init_all            (decoder_cot_bwd.hip) out = aggr_embed(cat(global, local)) of all K * N rows: the same InitBwdL image
//   k_mlp_heads_bwd_cot   one head, forward (recompute of u = W0 out, LayerNorm, ReLU) + backward per row; the upstream gradient of output
//                         2t + c is d_loc[k,n,t,c] (loc head) or d_loc[k,n,t,2+c] * ELU' (scale head, ELU' = min(1, scale - min_scale)
//                         read off the forward's output).  Two launches: two MlpHeadBwdL images do not fit LDS together; the scale
//                         launch writes DOUT = DOUT_loc + its own
//   k_dec_init_bwd_all    (decoder_cot_bwd.hip) aggr_embed backward over all modes: d_global, d_local = the modes' sum in mode order
//   k_mlp_pi_bwd          the three-layer pi head Linear(128,64) LN ReLU Linear(64,64) LN ReLU Linear(64,1) on cat(local, global[k])
//                         (GDEC:37-44, 50), forward + backward; ADDS its input gradients to d_local / d_global
//
// The mode sums run inside ONE wave per 16 actors, modes 0..K-1 in order: no atomics, identical calls give identical words.
// A separate unit so that the kernels of grid_bwd.hip and decoder_cot_bwd.hip keep their listings.
#include "bwd.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "layouts.hpp"
#include "tile.hpp"
#include "tile_bwd.hpp"

namespace tsde {

// rows r = k * N + n of NN = K * N.  out / H / DU / DOUT are [NN][64], DL [NN][128] (zero beyond 2T), loc / d_loc [NN][T][4];
// per-wave (dgamma | dbeta) of .1 -> vpart[wave][128]
template <bool SCALE>
__global__ __launch_bounds__(256) void k_mlp_heads_bwd_cot(const float* __restrict__ img, const float* __restrict__ out,
                                                           const float* __restrict__ loc, const float* __restrict__ d_loc, float min_scale,
                                                           int NN, int T, float* __restrict__ H, float* __restrict__ DL,
                                                           float* __restrict__ DU, float* __restrict__ DOUT, float* __restrict__ vpart,
                                                           const float* __restrict__ DOUT_LOC) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, MlpHeadBwdL::SIZE);
  using M = MlpHeadBwdL;
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int ntiles = (NN + 15) / 16;
  f4 dgam[4], dbet[4];
  zero4(dgam); zero4(dbet);
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    keep_lds_reads_here();
    const int row = tile * 16 + L.n, i = row < NN ? row : NN - 1;
    f4 a[4], u[4], h[4], dl[8];
    load_row(a, out, i, L.g);
    linear<4, 4>(u, a, lds + M::W0, lds + M::B0, L);
    const float rstd = ln_normalize(u);
    bool pos[16];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const f4 ga = *reinterpret_cast<const f4*>(lds + M::G + 16 * jt + 4 * L.g);
      const f4 be = *reinterpret_cast<const f4*>(lds + M::E + 16 * jt + 4 * L.g);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float pre = u[jt][c] * ga[c] + be[c];
        pos[4 * jt + c] = pre > 0.f;
        h[jt][c] = fmaxf(pre, 0.f);
      }
    }
    // lane (n, g) holds outputs 16jt + 4g + c: steps t0 = 8jt + 2g (c = 0,1 -> x,y) and t0 + 1 (c = 2,3); the head's own output values
    // are not needed: the upstream gradient is the caller's, and ELU' is read off the forward's scale
#pragma unroll
    for (int jt = 0; jt < 8; ++jt) {
      dl[jt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u2 = 0; u2 < 2; ++u2) {
        const int t = 8 * jt + 2 * L.g + u2;
        if (row < NN && t < T) {
          const int64_t e = (int64_t(i) * T + t) * 4 + (SCALE ? 2 : 0);
          const float2 g = *reinterpret_cast<const float2*>(d_loc + e);
          if (SCALE) {
            // scale = ELU(raw) + 1 + min_scale (GDEC:55-56): d scale / d raw = 1 for raw > 0, else exp(raw) = scale - 1 - min_scale + 1
            const float2 fw = *reinterpret_cast<const float2*>(loc + e);
            dl[jt][2 * u2] = g.x * fminf(1.0f, fw.x - min_scale);
            dl[jt][2 * u2 + 1] = g.y * fminf(1.0f, fw.y - min_scale);
          } else {
            dl[jt][2 * u2] = g.x;
            dl[jt][2 * u2 + 1] = g.y;
          }
        }
      }
    }
    f4 dh[4];
    zero4(dh);
    linear_adj<4, 8>(dh, dl, lds + M::W3T, L);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (!pos[4 * jt + c]) dh[jt][c] = 0.f;
    ln_backward(dh, u, rstd, lds + M::G, L.g, dgam, dbet);       // dh := d u
    f4 dout[4];
    linear_t(dout, dh, lds + M::W0T, L);
    if (row < NN) {
      if (SCALE) {
        f4 prev[4];
        load_row(prev, DOUT_LOC, row, L.g);
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) dout[jt] = prev[jt] + dout[jt];
      }
      store_row(h, H, row, L.g);
      store_row(dh, DU, row, L.g);
      store_row(dout, DOUT, row, L.g);
      float* p = DL + int64_t(row) * 128 + 4 * L.g;
#pragma unroll
      for (int jt = 0; jt < 8; ++jt) *reinterpret_cast<f4*>(p + 16 * jt) = dl[jt];
    }
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * 128;
  flush_vec(dgam, vp, L);
  flush_vec(dbet, vp + 64, L);
}
template __global__ void k_mlp_heads_bwd_cot<false>(const float*, const float*, const float*, const float*, float, int, int, float*, float*,
                                                    float*, float*, float*, const float*);
template __global__ void k_mlp_heads_bwd_cot<true>(const float*, const float*, const float*, const float*, float, int, int, float*, float*,
                                                   float*, float*, float*, const float*);

// pi head forward + backward, after k_dec_init_bwd_all on the same stream: d_global rows and d_local rows are read, added to and written
// back by the one wave that owns the actor.  d_pi is [N][K] (the forward's transposed layout, GDEC:50).  Saved for the weight-gradient
// products, all [K][N][64]: DP0 the delta rows of pi.0 (its global half's; DPS [N][64] their sum over the modes, the local half's),
// H1 the input rows of pi.3 and DP3 its delta rows.  Per-wave vector partials -> vpart[wave][MlpPiV::SIZE]
__global__ __launch_bounds__(128) void k_mlp_pi_bwd(const float* __restrict__ img, const float* __restrict__ local,
                                                    const float* __restrict__ global, const float* __restrict__ d_pi, int N, int K,
                                                    float* __restrict__ DP0, float* __restrict__ DPS, float* __restrict__ H1,
                                                    float* __restrict__ DP3, float* __restrict__ d_local, float* __restrict__ d_global,
                                                    float* __restrict__ vpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, MlpPiBwdL::SIZE);
  using P = MlpPiBwdL;
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int ntiles = (N + 15) / 16;
  f4 dgam1[4], dbet1[4], dgam4[4], dbet4[4], dw6[4];
  zero4(dgam1); zero4(dbet1); zero4(dgam4); zero4(dbet4); zero4(dw6);
  float db6 = 0.f;
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
      f4 gl[4], a[4], h1[4], b[4], d[4];
      load_row(gl, global, r, L.g);
      load_vec<4>(a, lds + P::BP, L.g);
      linear_acc<4, 4>(a, lo, lds + P::WP_L, L.lane);
      linear_acc<4, 4>(a, gl, lds + P::WP_G, L.lane);
      const float rstd1 = ln_normalize(a);                       // a = x_hat of pi.1
      bool pos1[16];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f4 ga = *reinterpret_cast<const f4*>(lds + P::PG + 16 * jt + 4 * L.g);
        const f4 be = *reinterpret_cast<const f4*>(lds + P::PE + 16 * jt + 4 * L.g);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float pre = a[jt][c] * ga[c] + be[c];
          pos1[4 * jt + c] = pre > 0.f;
          h1[jt][c] = fmaxf(pre, 0.f);
        }
      }
      linear<4, 4>(b, h1, lds + P::WP3, lds + P::BP3, L);
      const float rstd4 = ln_normalize(b);                       // b = x_hat of pi.4
      db6 += g;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f4 ga = *reinterpret_cast<const f4*>(lds + P::PG4 + 16 * jt + 4 * L.g);
        const f4 be = *reinterpret_cast<const f4*>(lds + P::PE4 + 16 * jt + 4 * L.g);
        const f4 w6 = *reinterpret_cast<const f4*>(lds + P::WP6 + 16 * jt + 4 * L.g);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float pre = b[jt][c] * ga[c] + be[c];
          dw6[jt][c] = fmaf(g, fmaxf(pre, 0.f), dw6[jt][c]);
          d[jt][c] = pre > 0.f ? g * w6[c] : 0.f;
        }
      }
      ln_backward(d, b, rstd4, lds + P::PG4, L.g, dgam4, dbet4);      // d := gradient at pi.3's output
      if (row < N) {
        store_row(h1, H1, r, L.g);
        store_row(d, DP3, r, L.g);
      }
      f4 e[4];
      linear_t(e, d, lds + P::WP3T, L);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (!pos1[4 * jt + c]) e[jt][c] = 0.f;
      ln_backward(e, a, rstd1, lds + P::PG, L.g, dgam1, dbet1);       // e := gradient at pi.0's output
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) dps[jt] += e[jt];
      f4 t[4];
      if (row < N) load_row(t, d_global, r, L.g);
      else zero4(t);
      linear_adj<4, 4>(t, e, lds + P::WP_GT, L);
      if (row < N) {
        store_row(e, DP0, r, L.g);
        store_row(t, d_global, r, L.g);
      }
    }
    f4 t[4];
    if (row < N) load_row(t, d_local, row, L.g);
    else zero4(t);
    linear_adj<4, 4>(t, dps, lds + P::WP_LT, L);
    if (row < N) {
      store_row(dps, DPS, row, L.g);
      store_row(t, d_local, row, L.g);
    }
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * MlpPiV::SIZE;
  flush_vec(dgam1, vp + MlpPiV::DGAM1, L);
  flush_vec(dbet1, vp + MlpPiV::DBET1, L);
  flush_vec(dgam4, vp + MlpPiV::DGAM4, L);
  flush_vec(dbet4, vp + MlpPiV::DBET4, L);
  flush_vec(dw6, vp + MlpPiV::DW6, L);
  flush_scalar(db6, vp + MlpPiV::DB6, L);
}

}  // namespace tsde

using namespace tsde;

namespace {
// gradient slots, in the order of trajsde_param_name(TRAJSDE_STAGE_DECODER_MLP_COT_BWD, i): the DECODER_MLP_NLL_BWD table, then the pi
// head (pack.hip recipe_decoder_mlp_cot_bwd)
enum MlpCotGradSlot {
  L0W = 0, L0B, L1W, L1B, L3W, L3B, A0W, A0B, A1W, A1B, S0W, S0B, S1W, S1B, S3W, S3B,
  P0W, P0B, P1W, P1B, P3W, P3B, P4W, P4B, P6W, P6B, N_MLP_GRADS_COT
};
constexpr int INIT_THREADS = 128, HEAD_THREADS = 256;
constexpr int VPART_ROWS = 512 * 4;                       // vec_grid caps a grid at 512 workgroups of at most 4 waves

struct MlpCotWs {
  float *out, *H, *DL, *DU, *DOUT, *H2, *DL2, *DU2, *DOUT2, *DA, *DAS, *DP0, *DPS, *H1, *DP3, *w3tmp, *b3tmp, *part, *cs, *vpart;
  int64_t bytes, parts;
  bool ok;
  MlpCotWs(void* ws, int64_t n, int N, int K) {
    Carver c(ws, n);
    const int64_t slab = int64_t(N) * K * 64, nslab = int64_t(N) * 64;
    out = c.take<float>(slab);
    H = c.take<float>(slab); DL = c.take<float>(slab * 2); DU = c.take<float>(slab); DOUT = c.take<float>(slab);
    H2 = c.take<float>(slab); DL2 = c.take<float>(slab * 2); DU2 = c.take<float>(slab); DOUT2 = c.take<float>(slab);
    DA = c.take<float>(slab); DAS = c.take<float>(nslab);
    DP0 = c.take<float>(slab); DPS = c.take<float>(nslab); H1 = c.take<float>(slab); DP3 = c.take<float>(slab);
    w3tmp = c.take<float>(128 * 64); b3tmp = c.take<float>(128);
    parts = wgrad_max_parts(int64_t(N) * K, 1);
    part = c.take<float>(parts * 4096); cs = c.take<float>(parts * 64);
    vpart = c.take<float>(int64_t(VPART_ROWS) * MlpPiV::SIZE);
    bytes = c.off + 256;
    ok = c.ok;
  }
};

// the largest K * N the 32-bit row and tile indices of the kernels hold (offsets are 64-bit), and the 2T <= 128 outputs of a head
bool mlp_cot_rows_ok(int32_t N, int K) { return N > 0 && K > 0 && int64_t(N) * K < (int64_t(1) << 31) - 64; }
bool mlp_cot_steps_ok(int T) { return T >= 1 && T <= 64; }

// the .3 layer of a head [2T, 64] over R rows: two 64-row blocks into a 128-row scratch, the first 2T rows are the gradient
int head3_wgrad_rows(const WgradCtx& wc, const MlpCotWs& w, const float* DL, const float* H, int64_t R, int T, float* W3, float* B3) {
  for (int b = 0; b < 2; ++b)
    if (int rc = run_wgrad(wc, DL + 64 * b, 128, H, 64, R, R, w.w3tmp + b * MAT64, 64, 0, w.b3tmp + 64 * b, 0)) return rc;
  TS_HIP(hipMemcpyAsync(W3, w.w3tmp, size_t(2 * T) * 64 * sizeof(float), hipMemcpyDeviceToDevice, wc.st));
  TS_HIP(hipMemcpyAsync(B3, w.b3tmp, size_t(2 * T) * sizeof(float), hipMemcpyDeviceToDevice, wc.st));
  return 0;
}
}  // namespace

extern "C" {

int64_t trajsde_mlp_decoder_cotangent_backward_ws_bytes(int32_t N, int num_modes, int future_steps) {
  if (!mlp_cot_rows_ok(N, num_modes)) return fail(TRAJSDE_ERR_INVALID, "mlp_decoder_cotangent_backward: empty or oversized problem");
  if (!mlp_cot_steps_ok(future_steps)) return fail(TRAJSDE_ERR_INVALID, "mlp_decoder_cotangent_backward: need 0 < future_steps <= 64");
  return MlpCotWs(nullptr, 0, N, num_modes).bytes;
}

int trajsde_mlp_decoder_cotangent_backward(int32_t N, int num_modes, int future_steps, const float* blob_bwd, const float* local_embed,
                                           const float* global_embed, const float* loc, float min_scale, const float* d_loc,
                                           const float* d_pi, void* ws, int64_t ws_bytes, float* const* grads, int n_grads,
                                           float* d_local, float* d_global, void* stream_) {
  TS_REQUIRE(blob_bwd && local_embed && global_embed && loc && d_loc && d_pi && ws && grads && d_local && d_global,
             "mlp_decoder_cotangent_backward: null pointer");
  TS_REQUIRE(mlp_cot_rows_ok(N, num_modes), "mlp_decoder_cotangent_backward: empty or oversized problem");
  TS_REQUIRE(mlp_cot_steps_ok(future_steps), "mlp_decoder_cotangent_backward: need 0 < future_steps <= 64");
  TS_REQUIRE(n_grads == int(N_MLP_GRADS_COT),
             "mlp_decoder_cotangent_backward: gradient count does not match trajsde_param_count(TRAJSDE_STAGE_DECODER_MLP_COT_BWD)");
  for (int i = 0; i < int(N_MLP_GRADS_COT); ++i) TS_REQUIRE(grads[i] != nullptr, "mlp_decoder_cotangent_backward: null gradient buffer");
  const int K = num_modes, T = future_steps, NN = N * K;
  MlpCotWs w(ws, ws_bytes, N, K);
  if (!w.ok || ws_bytes < w.bytes) return fail(TRAJSDE_ERR_WORKSPACE, "mlp_decoder_cotangent_backward: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const int ntiles = (NN + 15) / 16, atiles = (N + 15) / 16;
  const float* init_img = blob_bwd + MlpDecBwdBlob::INIT;
  const WgradCtx wc{st, w.part, w.cs, nullptr, w.parts};

  // ---- out = aggr_embed of every (mode, actor) row
  TS_LAUNCH(k_init_all, vec_grid(ntiles, INIT_THREADS, InitBwdL::SIZE * 4), INIT_THREADS, InitBwdL::AE_END * 4, st, init_img, local_embed,
            global_embed, N, K, w.out);

  // ---- the two heads from the cotangent: loc, then scale (its d out = the loc head's + its own)
  const int gh = vec_grid(ntiles, HEAD_THREADS, MlpHeadBwdL::SIZE * 4);
  TS_LAUNCH(k_mlp_heads_bwd_cot<false>, gh, HEAD_THREADS, MlpHeadBwdL::SIZE * 4, st, blob_bwd + MlpDecBwdBlob::HEAD, w.out, loc, d_loc,
            min_scale, NN, T, w.H, w.DL, w.DU, w.DOUT, w.vpart, nullptr);
  {
    ColsumBatch cb(st, gh * (HEAD_THREADS / 64), 128);
    cb.add(w.vpart, 64, grads[L1W]);
    cb.add(w.vpart + 64, 64, grads[L1B]);
    if (int rc = cb.flush()) return rc;
  }
  TS_LAUNCH(k_mlp_heads_bwd_cot<true>, gh, HEAD_THREADS, MlpHeadBwdL::SIZE * 4, st, blob_bwd + MlpDecNllBwdBlob::HEAD_SC, w.out, loc, d_loc,
            min_scale, NN, T, w.H2, w.DL2, w.DU2, w.DOUT2, w.vpart, w.DOUT);
  {
    ColsumBatch cb(st, gh * (HEAD_THREADS / 64), 128);
    cb.add(w.vpart, 64, grads[S1W]);
    cb.add(w.vpart + 64, 64, grads[S1B]);
    if (int rc = cb.flush()) return rc;
  }

  // ---- aggr_embed over all modes (overwrites d_local, d_global), then the pi head (adds to both)
  const int gi = vec_grid(atiles, INIT_THREADS, InitBwdL::SIZE * 4);
  TS_LAUNCH(k_dec_init_bwd_all, gi, INIT_THREADS, InitBwdL::SIZE * 4, st, init_img, local_embed, global_embed, w.DOUT2, N, K, w.DA, w.DAS,
            d_local, d_global, w.vpart);
  {
    ColsumBatch cb(st, gi * (INIT_THREADS / 64), InitV::SIZE);
    cb.add(w.vpart + InitV::DGAM, 64, grads[A1W]);
    cb.add(w.vpart + InitV::DBET, 64, grads[A1B]);
    if (int rc = cb.flush()) return rc;
  }
  const int gp = vec_grid(atiles, INIT_THREADS, MlpPiBwdL::SIZE * 4);
  TS_LAUNCH(k_mlp_pi_bwd, gp, INIT_THREADS, MlpPiBwdL::SIZE * 4, st, blob_bwd + MlpDecCotBwdBlob::PI, local_embed, global_embed, d_pi, N, K,
            w.DP0, w.DPS, w.H1, w.DP3, d_local, d_global, w.vpart);
  {
    ColsumBatch cb(st, gp * (INIT_THREADS / 64), MlpPiV::SIZE);
    cb.add(w.vpart + MlpPiV::DGAM1, 64, grads[P1W]);
    cb.add(w.vpart + MlpPiV::DBET1, 64, grads[P1B]);
    cb.add(w.vpart + MlpPiV::DGAM4, 64, grads[P4W]);
    cb.add(w.vpart + MlpPiV::DBET4, 64, grads[P4B]);
    cb.add(w.vpart + MlpPiV::DW6, 64, grads[P6W]);
    cb.add(w.vpart + MlpPiV::DB6, 1, grads[P6B]);
    if (int rc = cb.flush()) return rc;
  }

  // ---- weight gradients
  int rc;
  if ((rc = head3_wgrad_rows(wc, w, w.DL, w.H, NN, T, grads[L3W], grads[L3B]))) return rc;
  if ((rc = head3_wgrad_rows(wc, w, w.DL2, w.H2, NN, T, grads[S3W], grads[S3B]))) return rc;
  {
    WgradBatch rows(wc, NN, NN);                            // every 64 x 64 problem over the K * N rows
    if ((rc = rows.add(w.DU, 64, w.out, 64, grads[L0W], 64, 0, grads[L0B], 0))) return rc;
    if ((rc = rows.add(w.DU2, 64, w.out, 64, grads[S0W], 64, 0, grads[S0B], 0))) return rc;
    if ((rc = rows.add(w.DP3, 64, w.H1, 64, grads[P3W], 64, 0, grads[P3B], 0))) return rc;
    // the global halves: aggr_embed.0 = cat(global, local), pi.0 = cat(local, global)
    if ((rc = rows.add(w.DA, 64, global_embed, 64, grads[A0W], 128, 0, grads[A0B], 0))) return rc;
    if ((rc = rows.add(w.DP0, 64, global_embed, 64, grads[P0W], 128, 64, grads[P0B], 0))) return rc;
    if ((rc = rows.flush())) return rc;
  }
  {
    WgradBatch loc_(wc, N, N);                              // the local halves: the mode-summed delta rows against the actors' rows
    if ((rc = loc_.add(w.DAS, 64, local_embed, 64, grads[A0W], 128, 64, nullptr, 0))) return rc;
    if ((rc = loc_.add(w.DPS, 64, local_embed, 64, grads[P0W], 128, 0, nullptr, 0))) return rc;
    if ((rc = loc_.flush())) return rc;
  }
  return TRAJSDE_OK;
}

}  // extern "C"

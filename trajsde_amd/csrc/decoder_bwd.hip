// decoder_bwd.hip -- winner-takes-all L2 regression loss (reference losses/L2.py:10-27) and the backward pass of the
// SDEDecoder stage (DEC:77-105) for gfx950: gradients w.r.t. the decoder's parameters and w.r.t. its two inputs
// (local_embed, global_embed).  First family of SURVEY.md 8(f) rank 1.
//
// Only the winning mode of each actor carries gradient, so everything below runs on N rows (path r_i = best_i*N + i),
// not K*N.  The Euler-Maruyama solve is differentiated "discretise-then-optimise": the forward trajectory of the
// N winning paths is replayed once (same Philox counters, so the same noise) keeping every state and hidden
// activation, then a reverse sweep propagates dL/dy_k through the step map y' = y + f(y,t) dt + g(y,t) z sqrt(h).
//
//   k_l2_wta / k_l2_finalize   best mode per actor, loss value, 1/count
//   k_init_sel                 y0 of the winning paths                      (aggr_embed, DEC:82)
//   k_sde_replay               forward replay, keeps y_k, tanh activations and g  [step][row][64]
//   k_head_bwd                 loc head forward + backward per (row, output step): dL/ds_o, saves (s, du)
//   k_sde_bwd                  the reverse sweep; saves the pre-activation gradients of the five linears
//   k_dec_init_bwd             aggr_embed backward: d local_embed, d global_embed, saves (input, da)
// The weight gradients (dW = sum_rows delta^T a over the saved rows) and every column sum go through the engine of wgrad.hip.
// trajsde_decoder_cotangent_backward (decoder_cot_bwd.hip, through the host helpers at the end of this file: decoder_bwd_host.hpp) runs
// the replay and the sweep over ALL K * N paths from caller-supplied dL/dloc and dL/dpi: no loss inside, scale and pi heads included.
// `method: milstein` (trajsde_decoder_*_backward_milstein) runs the same host code with the replay and the sweep of
// decoder_mil_bwd.hip (the Milstein step and its gdg term) and two more weight-gradient products.
//
// Matrix products run on transposed images (layouts.hpp SweepL / HeadBwdL / InitBwdL): dX^T = W^T dY^T has the same
// "row on lane" operand/result layout as the forward.  tile.hpp linear_adj: row-scaled split precision in the fp16x3
// build, the exact fp32 instruction in the bf16x6 build; the weight gradients (wgrad.hip k_wgrad) are always exact fp32.
#include <cstdlib>

#include "common.hpp"
#include "layouts.hpp"
#include "philox.hpp"
#include "range.hpp"
#include "sde_funcs.hpp"
#include "tile.hpp"
#include "tile_bwd.hpp"
#include "bwd.hpp"
#include "kernels.hpp"
#include "decoder_bwd_host.hpp"

namespace tsde {

// ------------------------------------------------------------------ loss
// masked L2 per (actor, mode), first minimum wins (L2.py:19-22).  One thread per (actor, mode): the T steps' mask bytes, targets and
// predictions are requested eight steps at a time and summed in step order -- the same sums, bit for bit, as the one-thread-per-actor
// loop this replaces, which walked K x T dependent loads per thread (0.29 ms at 128 x 48 agents, K = 10, T = 60: 4 % of that step).
// The argmin over the modes of an actor goes through LDS: 256 / KP actors a workgroup (KP = K rounded up to a power of two).
__global__ __launch_bounds__(256) void k_l2_wta(const float* __restrict__ loc, const float* __restrict__ y, const uint8_t* __restrict__ mask, int N, int K,
                                                int T, int32_t* __restrict__ best, float* __restrict__ minsum, int32_t* __restrict__ cnt, int KP) {
  __shared__ float s_sum[256];
  __shared__ int s_cnt[256];
  const int per = 256 / KP, a = threadIdx.x / KP, k = threadIdx.x - a * KP;
  const int i = blockIdx.x * per + a;
  const bool live = a < per && i < N && k < K;
  float s = 0.f;
  int c = 0;
  if (live) {
    const uint8_t* mk = mask + int64_t(i) * T;
    const float2* yy = reinterpret_cast<const float2*>(y) + int64_t(i) * T;
    const f4* ll = reinterpret_cast<const f4*>(loc) + (int64_t(k) * N + i) * T;
    for (int t0 = 0; t0 < T; t0 += 8) {
      uint8_t m[8];
      float2 yv[8];
      f4 lv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = t0 + u < T ? t0 + u : T - 1;
        m[u] = mk[t];
        yv[u] = yy[t];
        lv[u] = ll[t];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (t0 + u >= T || !m[u]) continue;
        const float dx = yv[u].x - lv[u][0], dy = yv[u].y - lv[u][1];
        s += sqrtf(dx * dx + dy * dy);
        ++c;
      }
    }
  }
  s_sum[threadIdx.x] = s;
  s_cnt[threadIdx.x] = c;
  __syncthreads();
  if (live && k == 0) {
    int bk = 0;
    float bs = s;
    for (int kk = 1; kk < K; ++kk) {
      const float v = s_sum[a * KP + kk];
      if (v < bs) {
        bs = v;
        bk = kk;
      }
    }
    best[i] = bk;
    minsum[i] = bs;
    cnt[i] = c;
  }
}

__device__ __forceinline__ void k_loss_finalize_body(const float* __restrict__ minsum, const int32_t* __restrict__ cnt, int N,
                                                      float* __restrict__ scal, int per_step);
// Laplace NLL of the winning mode (losses/laplace_nll_loss.py:29-44): per actor the sum over its valid steps of
// log(2 s) + |y - l| / s for both coordinates, s = max(scale, eps); overwrites minsum (the winner is already chosen)
__global__ void k_nll_value(const float* __restrict__ loc, const float* __restrict__ y, const uint8_t* __restrict__ mask,
                            const int32_t* __restrict__ best, int N, int T, float eps, float* __restrict__ minsum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float s = 0.f;
  const uint8_t* mk = mask + int64_t(i) * T;
  const float2* yy = reinterpret_cast<const float2*>(y) + int64_t(i) * T;
  const f4* ll = reinterpret_cast<const f4*>(loc) + (int64_t(best[i]) * N + i) * T;
  for (int t0 = 0; t0 < T; t0 += 8) {                    // eight steps' loads in flight, summed in step order
    uint8_t m[8];
    float2 yv[8];
    f4 lv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = t0 + u < T ? t0 + u : T - 1;
      m[u] = mk[t];
      yv[u] = yy[t];
      lv[u] = ll[t];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (t0 + u >= T || !m[u]) continue;
      const f4 l = lv[u];
      const float sx = fmaxf(l[2], eps), sy = fmaxf(l[3], eps);
      s += logf(2.f * sx) + fabsf(yv[u].x - l[0]) / sx;
      s += logf(2.f * sy) + fabsf(yv[u].y - l[1]) / sy;
    }
  }
  minsum[i] = s;
}

// scal[0] = loss = sum(minsum) / count, scal[1] = 1/count (0 when nothing is valid); fixed summation order
__global__ __launch_bounds__(1024) void k_l2_finalize(const float* __restrict__ minsum, const int32_t* __restrict__ cnt, int N,
                                                      float* __restrict__ scal) {
  k_loss_finalize_body(minsum, cnt, N, scal, 1);
}
// the same with `per_step` loss elements per valid step (the Laplace NLL averages over the x and the y term: 2)
__global__ __launch_bounds__(1024) void k_nll_finalize(const float* __restrict__ minsum, const int32_t* __restrict__ cnt, int N,
                                                       float* __restrict__ scal) {
  k_loss_finalize_body(minsum, cnt, N, scal, 2);
}
__device__ __forceinline__ void k_loss_finalize_body(const float* __restrict__ minsum, const int32_t* __restrict__ cnt, int N,
                                                      float* __restrict__ scal, int per_step) {
  __shared__ double ssum[1024];
  __shared__ long long scnt[1024];
  double s = 0.0;
  long long c = 0;
  for (int i = threadIdx.x; i < N; i += 1024) {
    s += double(minsum[i]);
    c += cnt[i];
  }
  ssum[threadIdx.x] = s;
  scnt[threadIdx.x] = c;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (int(threadIdx.x) < w) {
      ssum[threadIdx.x] += ssum[threadIdx.x + w];
      scnt[threadIdx.x] += scnt[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double denom = double(scnt[0]) * per_step;
    scal[0] = scnt[0] > 0 ? float(ssum[0] / denom) : 0.f;
    scal[1] = scnt[0] > 0 ? float(1.0 / denom) : 0.f;
  }
}

// ------------------------------------------------------------------ forward replay of the winning paths
__global__ __launch_bounds__(128) void k_init_sel(const float* __restrict__ img, const float* __restrict__ local,
                                                  const float* __restrict__ global, const int32_t* __restrict__ best, int N,
                                                  float* __restrict__ y0, float* __restrict__ gsel) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, InitBwdL::AE_END);
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int ntiles = (N + 15) / 16;
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    keep_lds_reads_here();
    const int row = tile * 16 + L.n;
    const int i = row < N ? row : N - 1;
    f4 gl[4], lo[4], a[4];
    load_row(gl, global, int64_t(best[i]) * N + i, L.g);
    load_row(lo, local, i, L.g);
    range_note(fmaxf(absmax<4>(gl), absmax<4>(lo)), RS_DEC_INPUT);   // the caller's rows: no forward call has to precede a backward one
    load_vec<4>(a, lds + InitBwdL::BA, L.g);
    linear_acc<4, 4>(a, gl, lds + InitBwdL::WA_G, L.lane);
    linear_acc<4, 4>(a, lo, lds + InitBwdL::WA_L, L.lane);
    layer_norm<4>(a, lds + InitBwdL::AG, lds + InitBwdL::AE, L.g);
    relu<4>(a);
    if (row < N) {
      store_row(a, y0, row, L.g);
      store_row(gl, gsel, row, L.g);
    }
  }
}

// states [n_euler+1][N][64] (slab 0 = y0 on entry); H1,H2,G1,G2 [n_euler][N][64]; GS [n_euler][N]
__global__ __launch_bounds__(128) void k_sde_replay(const float* __restrict__ img, const int32_t* __restrict__ best, int N, int K,
                                                    int n_euler, const float* __restrict__ step_tab, NoiseArg na,
                                                    float* __restrict__ states, float* __restrict__ H1, float* __restrict__ H2,
                                                    float* __restrict__ G1, float* __restrict__ G2, float* __restrict__ GS) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, DecSdeL::LOC);                      // drift + diffusion images
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int ntiles = (N + 15) / 16;
  const int64_t slab = int64_t(N) * D;
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    const int row = tile * 16 + L.n;
    const int i = row < N ? row : N - 1;
    const int64_t r = int64_t(best[i]) * N + i;
    f4 y[4];
    load_row(y, states, i, L.g);
    for (int k = 0; k < n_euler; ++k) {
      keep_lds_reads_here();
      const float dt = step_tab[k * 8 + 1], sq = step_tab[k * 8 + 2], sn = step_tab[k * 8 + 3], cs = step_tab[k * 8 + 4];
      const float* F = lds + DecSdeL::F;
      const float* G = lds + DecSdeL::G;
      f4 h1[4], h2[4], f[4], z[4];
      sde_layer0(h1, y, F, DriftL::W0, DriftL::WS, DriftL::WC, DriftL::B0, sn, cs, L);
      tanh_<4>(h1);
      linear<4, 4>(h2, h1, F + DriftL::W2, F + DriftL::B2, L);
      tanh_<4>(h2);
      linear<4, 4>(f, h2, F + DriftL::W4, F + DriftL::B4, L);
      if (row < N) {
        store_row(h1, H1 + k * slab, row, L.g);
        store_row(h2, H2 + k * slab, row, L.g);
      }
      sde_layer0(h1, y, G, DiffL::W0, DiffL::WS, DiffL::WC, DiffL::B0, sn, cs, L);
      tanh_<4>(h1);
      linear<4, 4>(h2, h1, G + DiffL::W2, G + DiffL::B2, L);
      tanh_<4>(h2);
      const float gs = fast_sigmoid(row_dot(h2, G + DiffL::W4, L.g) + G[DiffL::B4]);
      if (row < N) {
        store_row(h1, G1 + k * slab, row, L.g);
        store_row(h2, G2 + k * slab, row, L.g);
        if (L.g == 0) GS[int64_t(k) * N + row] = gs;
      }
      noise_row(z, na, STREAM_DECODER, k, r, int64_t(N) * K, L.g);
      em_update(y, f, gs, z, dt, sq);
      range_note(absmax<4>(y), RS_DEC_STATE);                 // as the forward (decoder.hip k_sde_decode): the next step's split operand
      if (row < N) store_row(y, states + (k + 1) * slab, row, L.g);
    }
  }
}

// ------------------------------------------------------------------ loc head: forward + backward per (row, output)
// vector-gradient slots of one wave in `vpart` (floats)
struct HeadV { enum : int { DGAM = 0, DBET = 64, DW3X = 128, DW3Y = 192, DB3 = 256, SIZE = 264 }; };

// rows are (o, i): o = output step, i = actor.  S_in / DU / DS are [T][N][64]
// MODE 0: the loc head under the winner-takes-all L2 loss.  MODE 1 / 2: the loc / the scale head under the Laplace NLL
// (losses/laplace_nll_loss.py): `nll` (bwd.hpp NllArg) carries the forward's outputs of the winning mode (the other head's value
// enters each head's upstream gradient); the scale head's launch ADDS its state gradient to the loc head's (DS) and writes its own
// delta rows.
template <int MODE>
__global__ __launch_bounds__(128) void k_head_bwd(const float* __restrict__ img, const float* __restrict__ states,
                                                  const float* __restrict__ out_tab, const float* __restrict__ y,
                                                  const uint8_t* __restrict__ mask, const float* __restrict__ scal, int N, int T,
                                                  float* __restrict__ S_in, float* __restrict__ DU, float* __restrict__ DS,
                                                  float* __restrict__ vpart, NllArg nll) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, HeadBwdL::SIZE);
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int tiles_per_o = (N + 15) / 16;
  const int ntiles = tiles_per_o * T;
  const int64_t slab = int64_t(N) * D;
  const float inv_count = scal[1];
  const float* H = lds + HeadBwdL::FWD;
  f4 dgam[4], dbet[4], dw3x[4], dw3y[4];
  zero4(dgam); zero4(dbet); zero4(dw3x); zero4(dw3y);
  float db3x = 0.f, db3y = 0.f;
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    keep_lds_reads_here();
    const int o = tile / tiles_per_o;
    const int row = (tile - o * tiles_per_o) * 16 + L.n;
    const int i = row < N ? row : N - 1;
    const int ko = int(out_tab[o * 4]);
    const float w0 = out_tab[o * 4 + 1], w1 = out_tab[o * 4 + 2];
    f4 s[4], u[4], v[4];
    {
      f4 a[4], b[4];
      load_row(a, states + (ko - 1) * slab, i, L.g);
      load_row(b, states + ko * slab, i, L.g);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[jt][c] = w0 * a[jt][c] + w1 * b[jt][c];
    }
    linear<4, 4>(u, s, H + HeadL::W0, H + HeadL::B0, L);
    const float rstd = ln_normalize(u);                     // u = x_hat
    bool pos[16];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const f4 ga = *reinterpret_cast<const f4*>(H + HeadL::G + 16 * jt + 4 * L.g);
      const f4 be = *reinterpret_cast<const f4*>(H + HeadL::E + 16 * jt + 4 * L.g);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float pre = u[jt][c] * ga[c] + be[c];
        pos[jt * 4 + c] = pre > 0.f;
        v[jt][c] = fmaxf(pre, 0.f);
      }
    }
    const float lx = row_dot(v, H + HeadL::W3, L.g) + H[HeadL::B3];
    const float ly = row_dot(v, H + HeadL::W3 + 64, L.g) + H[HeadL::B3 + 1];
    float gx = 0.f, gy = 0.f;
    if (row < N && mask[int64_t(i) * T + o]) {
      const float yx = y[(int64_t(i) * T + o) * 2], yy = y[(int64_t(i) * T + o) * 2 + 1];
      if (MODE == 0) {
        // dL/dl = (l - y) / |l - y| / count on valid steps (L2.py:16,25)
        const float dx = lx - yx, dy = ly - yy;
        const float nrm = sqrtf(dx * dx + dy * dy);
        if (nrm > 0.f) {
          gx = dx / nrm * inv_count;
          gy = dy / nrm * inv_count;
        }
      } else {
        const f4 fw = *reinterpret_cast<const f4*>(nll.loc + ((int64_t(nll.best[i]) * N + i) * T + o) * 4);
        if (MODE == 1) {
          // d/dl [ |y - l| / s ] = -sign(y - l) / s, s = max(scale, eps) of the forward (no gradient through the clamp's value)
          const float sx = fmaxf(fw[2], nll.eps), sy = fmaxf(fw[3], nll.eps);
          const float ex = yx - lx, ey = yy - ly;
          gx = (ex > 0.f ? -1.f : ex < 0.f ? 1.f : 0.f) / sx * inv_count;
          gy = (ey > 0.f ? -1.f : ey < 0.f ? 1.f : 0.f) / sy * inv_count;
        } else {
          // this head's two outputs are the raw scales: s = ELU(raw) + 1 + min_scale (DEC:97-98), clamped at eps in place, the
          // gradient passing through (laplace_nll_loss.py:38-40); d/ds [ log 2s + |y - l| / s ] = 1/s - |y - l| / s^2
          const float sxr = (lx > 0.f ? lx : fast_exp(lx) - 1.0f) + 1.0f + nll.min_scale;
          const float syr = (ly > 0.f ? ly : fast_exp(ly) - 1.0f) + 1.0f + nll.min_scale;
          const float sx = fmaxf(sxr, nll.eps), sy = fmaxf(syr, nll.eps);
          const float ax = fabsf(yx - fw[0]), ay = fabsf(yy - fw[1]);
          gx = (1.0f / sx - ax / (sx * sx)) * inv_count * (lx > 0.f ? 1.0f : fast_exp(lx));
          gy = (1.0f / sy - ay / (sy * sy)) * inv_count * (ly > 0.f ? 1.0f : fast_exp(ly));
        }
      }
    }
    db3x += gx;
    db3y += gy;
    f4 dv[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const f4 wx = *reinterpret_cast<const f4*>(H + HeadL::W3 + 16 * jt + 4 * L.g);
      const f4 wy = *reinterpret_cast<const f4*>(H + HeadL::W3 + 64 + 16 * jt + 4 * L.g);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        dw3x[jt][c] = fmaf(gx, v[jt][c], dw3x[jt][c]);
        dw3y[jt][c] = fmaf(gy, v[jt][c], dw3y[jt][c]);
        dv[jt][c] = pos[jt * 4 + c] ? fmaf(gx, wx[c], gy * wy[c]) : 0.f;
      }
    }
    ln_backward(dv, u, rstd, H + HeadL::G, L.g, dgam, dbet);      // dv := du
    f4 ds[4];
    linear_t(ds, dv, lds + HeadBwdL::W0T, L);
    if (row < N) {
      if (MODE == 2) {                                       // the second head of the step: its state gradient joins the first's
        f4 prev[4];
        load_row(prev, DS + o * slab, row, L.g);
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) ds[jt] += prev[jt];
      } else {
        store_row(s, S_in + o * slab, row, L.g);
      }
      store_row(dv, DU + o * slab, row, L.g);
      store_row(ds, DS + o * slab, row, L.g);
    }
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * HeadV::SIZE;
  flush_vec(dgam, vp + HeadV::DGAM, L);
  flush_vec(dbet, vp + HeadV::DBET, L);
  flush_vec(dw3x, vp + HeadV::DW3X, L);
  flush_vec(dw3y, vp + HeadV::DW3Y, L);
  flush_scalar(db3x, vp + HeadV::DB3, L);
  flush_scalar(db3y, vp + HeadV::DB3 + 1, L);
}

// ------------------------------------------------------------------ reverse sweep through the Euler-Maruyama steps
struct SweepV { enum : int { DV4 = 0, DC4 = 64, SIZE = 68 }; };

__global__ __launch_bounds__(128, 2) void k_sde_bwd(const float* __restrict__ img, const int32_t* __restrict__ best, int N, int K, int T,
                                                 int n_euler, const float* __restrict__ step_tab, const float* __restrict__ out_tab,
                                                 NoiseArg na, const float* __restrict__ H1, const float* __restrict__ H2,
                                                 const float* __restrict__ G1, const float* __restrict__ G2,
                                                 const float* __restrict__ GS, const float* __restrict__ DS,
                                                 float* __restrict__ DH1, float* __restrict__ DH2, float* __restrict__ DF,
                                                 float* __restrict__ DG1, float* __restrict__ DG2, float* __restrict__ DY0,
                                                 float* __restrict__ vpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, SweepL::SIZE);
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int ntiles = (N + 15) / 16;
  const int64_t slab = int64_t(N) * D;
  f4 dv4[4];
  zero4(dv4);
  float dc4 = 0.f;
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    const int row = tile * 16 + L.n;
    const int i = row < N ? row : N - 1;
    const bool live = row < N;
    const int64_t r = int64_t(best[i]) * N + i;
    f4 dy[4];                                             // dL/dy_{k+1} on entry of iteration k
    zero4(dy);
    int o = T - 1;
    // The saved activation tiles of an iteration used to be loaded right where they are consumed, behind a matrix product they do
    // not depend on: four exposed round trips to HBM per iteration of a kernel that runs one wave per SIMD on a third of the chip (384
    // tiles at 128 x 48 agents).  Now the two that are consumed FIRST (the last layers' activations) and the diffusion value are
    // requested one iteration ahead (32 registers), the other two at the top of their iteration, a matrix product ahead of their use.
    f4 nh2[4], ng2[4];
    float ngs;
    {
      const int k0 = n_euler - 1;
      load_row(nh2, H2 + k0 * slab, i, L.g);
      load_row(ng2, G2 + k0 * slab, i, L.g);
      ngs = GS[int64_t(k0) * N + i];
    }
    for (int k = n_euler - 1; k >= 0; --k) {
      keep_lds_reads_here();
      const float dt = step_tab[k * 8 + 1], sq = step_tab[k * 8 + 2];
      f4 ah2[4], ah1[4], ag2[4], ag1[4];
      load_row(ah1, H1 + k * slab, i, L.g);
      load_row(ag1, G1 + k * slab, i, L.g);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) { ah2[jt] = nh2[jt]; ag2[jt] = ng2[jt]; }
      const float gs = ngs;
      if (k > 0) {
        load_row(nh2, H2 + (k - 1) * slab, i, L.g);
        load_row(ng2, G2 + (k - 1) * slab, i, L.g);
        ngs = GS[int64_t(k - 1) * N + i];
      }
      // outputs interpolated between y_k and y_{k+1}: s_o = w0 y_k + w1 y_{k+1}
      f4 dprev[4];
      zero4(dprev);
      while (o >= 0 && int(out_tab[o * 4]) == k + 1) {
        const float w0 = out_tab[o * 4 + 1], w1 = out_tab[o * 4 + 2];
        f4 ds[4];
        load_row(ds, DS + o * slab, i, L.g);
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            dy[jt][c] = fmaf(w1, ds[jt][c], dy[jt][c]);
            dprev[jt][c] = fmaf(w0, ds[jt][c], dprev[jt][c]);
          }
        --o;
      }
      f4 d[4], t[4];
      // ---- drift net: y' gets f*dt
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) d[jt][c] = dt * dy[jt][c];
      if (live) store_row(d, DF + k * slab, row, L.g);
      linear_t(t, d, lds + SweepL::F_W4T, L);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) d[jt][c] = t[jt][c] * (1.0f - ah2[jt][c] * ah2[jt][c]);
      if (live) store_row(d, DH2 + k * slab, row, L.g);
      linear_t(t, d, lds + SweepL::F_W2T, L);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) d[jt][c] = t[jt][c] * (1.0f - ah1[jt][c] * ah1[jt][c]);
      if (live) store_row(d, DH1 + k * slab, row, L.g);
      f4 dyn[4];                                          // dL/dy_k being assembled
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) dyn[jt] = dy[jt] + dprev[jt];
      linear_adj<4, 4>(dyn, d, lds + SweepL::F_W0T, L);
      // ---- diffusion net: y' gets g * (z sqrt(h)), g one scalar per row
      f4 z[4];
      noise_row(z, na, STREAM_DECODER, k, r, int64_t(N) * K, L.g);
      float cdot = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) cdot = fmaf(z[jt][c] * sq, dy[jt][c], cdot);
      const float dgp = row_sum(cdot) * gs * (1.0f - gs);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f4 w4 = *reinterpret_cast<const f4*>(lds + SweepL::G_W4 + 16 * jt + 4 * L.g);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (live) dv4[jt][c] = fmaf(dgp, ag2[jt][c], dv4[jt][c]);
          d[jt][c] = dgp * w4[c] * (1.0f - ag2[jt][c] * ag2[jt][c]);
        }
      }
      if (live) {
        dc4 += dgp;
        store_row(d, DG2 + k * slab, row, L.g);
      }
      linear_t(t, d, lds + SweepL::G_W2T, L);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) d[jt][c] = t[jt][c] * (1.0f - ag1[jt][c] * ag1[jt][c]);
      if (live) store_row(d, DG1 + k * slab, row, L.g);
      linear_adj<4, 4>(dyn, d, lds + SweepL::G_W0T, L);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) dy[jt] = dyn[jt];
    }
    if (live) store_row(dy, DY0, row, L.g);
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * SweepV::SIZE;
  flush_vec(dv4, vp + SweepV::DV4, L);
  flush_scalar(dc4, vp + SweepV::DC4, L);
}

// ------------------------------------------------------------------ aggr_embed backward

__global__ __launch_bounds__(128) void k_dec_init_bwd(const float* __restrict__ img, const float* __restrict__ local,
                                                      const float* __restrict__ gsel, const float* __restrict__ DY0,
                                                      const int32_t* __restrict__ best, int N, float* __restrict__ DA,
                                                      float* __restrict__ d_local, float* __restrict__ d_global,
                                                      float* __restrict__ vpart) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_blob(lds, img, InitBwdL::SIZE);
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int ntiles = (N + 15) / 16;
  f4 dgam[4], dbet[4];
  zero4(dgam); zero4(dbet);
  for (int tile = blockIdx.x * waves + wave; tile < ntiles; tile += gridDim.x * waves) {
    keep_lds_reads_here();
    const int row = tile * 16 + L.n;
    const int i = row < N ? row : N - 1;
    f4 gl[4], lo[4], a[4], d[4];
    load_row(gl, gsel, i, L.g);
    load_row(lo, local, i, L.g);
    load_vec<4>(a, lds + InitBwdL::BA, L.g);
    linear_acc<4, 4>(a, gl, lds + InitBwdL::WA_G, L.lane);
    linear_acc<4, 4>(a, lo, lds + InitBwdL::WA_L, L.lane);
    const float rstd = ln_normalize(a);
    load_row(d, DY0, i, L.g);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const f4 ga = *reinterpret_cast<const f4*>(lds + InitBwdL::AG + 16 * jt + 4 * L.g);
      const f4 be = *reinterpret_cast<const f4*>(lds + InitBwdL::AE + 16 * jt + 4 * L.g);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (!(a[jt][c] * ga[c] + be[c] > 0.f) || row >= N) d[jt][c] = 0.f;
    }
    ln_backward(d, a, rstd, lds + InitBwdL::AG, L.g, dgam, dbet);   // d := d a_pre
    f4 t[4];
    if (row < N) store_row(d, DA, row, L.g);
    linear_t(t, d, lds + InitBwdL::WA_GT, L);
    if (row < N) store_row(t, d_global, int64_t(best[i]) * N + i, L.g);
    linear_t(t, d, lds + InitBwdL::WA_LT, L);
    if (row < N) store_row(t, d_local, row, L.g);
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * InitV::SIZE;
  flush_vec(dgam, vp + InitV::DGAM, L);
  flush_vec(dbet, vp + InitV::DBET, L);
}

// ------------------------------------------------------------------ host side (declared in decoder_bwd_host.hpp)
// Shared by the welded entry points below and by trajsde_decoder_cotangent_backward (decoder_cot_bwd.hip).  The replay, the sweep and
// the weight gradients run over a row domain (rows, K'): the kernels walk `rows` rows and take path best[i] * rows + i of rows * K'.
// The welded entry points pass (N, K) -- the winning mode of every actor; the cotangent one passes (K * N, 1) with best = 0, the
// identity over all paths.

BwdWs carve_bwd(void* ws, int64_t ws_bytes, int N, int T, int n_euler, bool& ok, bool nll, bool mil) {
  Carver cv(ws, ws_bytes);
  BwdWs w;
  const int64_t slab = int64_t(N) * 64;
  w.best = cv.take<int32_t>(N);
  w.cnt = cv.take<int32_t>(N);
  w.minsum = cv.take<float>(N);
  w.scal = cv.take<float>(4);
  w.states = cv.take<float>(slab * (n_euler + 1));
  w.H1 = cv.take<float>(slab * n_euler);
  w.H2 = cv.take<float>(slab * n_euler);
  w.G1 = cv.take<float>(slab * n_euler);
  w.G2 = cv.take<float>(slab * n_euler);
  w.GS = cv.take<float>(int64_t(N) * n_euler);
  w.DH1 = cv.take<float>(slab * n_euler);
  w.DH2 = cv.take<float>(slab * n_euler);
  w.DF = cv.take<float>(slab * n_euler);
  w.DG1 = cv.take<float>(slab * n_euler);
  w.DG2 = cv.take<float>(slab * n_euler);
  w.S_in = cv.take<float>(slab * T);
  w.DU = cv.take<float>(slab * T);
  w.DS = cv.take<float>(slab * T);
  w.gsel = cv.take<float>(slab);
  w.DA = cv.take<float>(slab);
  w.DY0 = cv.take<float>(slab);
  const int64_t max_rows = int64_t(N) * (n_euler > T ? n_euler : T);
  const int64_t max_parts = w.parts = wgrad_max_parts(max_rows, n_euler > T ? n_euler : T);
  w.part = cv.take<float>(max_parts * 4096);
  w.cs = cv.take<float>(max_parts * 64);
  w.vpart = cv.take<float>(SHARED_VPART_FLOATS);
  w.varena_floats = VPART_ARENA_SLABS * SHARED_VPART_FLOATS;
  w.varena = cv.take<float>(w.varena_floats);
  w.DU2 = nll ? cv.take<float>(slab * T) : nullptr;        // the scale head's delta rows (Laplace NLL)
  w.mil = MilRows{nullptr, nullptr, nullptr, nullptr};
  w.MW2 = w.MW0 = nullptr;
  if (mil) {
    w.mil.g2b = cv.take<float>(slab * n_euler);
    w.mil.h1t = cv.take<float>(slab * n_euler);
    w.mil.g1b = cv.take<float>(slab * n_euler);
    w.mil.u = cv.take<float>(slab * n_euler);
    w.MW2 = cv.take<float>(4096);
    w.MW0 = cv.take<float>(4096);
  }
  w.bytes = cv.off + 256;
  ok = cv.ok;
  return w;
}

int bwd_grid(int ntiles) {
  const int waves = BWD_THREADS / 64;
  const int g = (ntiles + waves - 1) / waves;
  return g < 1 ? 1 : (g > 256 ? 256 : g);
}

NoiseArg noise_arg(const trajsde_noise* noise) {
  NoiseArg na{0, nullptr, nullptr};
  if (noise) { na.seed = noise->seed; na.z = noise->z; na.row_ids = noise->row_ids; na.seed_dev = noise->seed_dev; }
  return na;
}

// Forward replay of the selected paths.  Milstein (blob_fwd a TRAJSDE_STAGE_DECODER_MILSTEIN image): the one-wave kernel of
// decoder_mil_bwd.hip, MilL staged behind the plain images.  Otherwise the cooperative form (recur.hip k_sde_replay_coop: four waves a
// tile, the fused forward kernel's own image; fp16x3 build), or with TRAJSDE_REPLAY_COOP=0 the one-wave kernel of this file.
int launch_replay(hipStream_t st, const float* blob_fwd, const BwdWs& w, int rows, int K, int n_euler, const float* step_table,
                  const NoiseArg& na, bool milstein) {
  const int ntiles = (rows + 15) / 16;
  if (milstein) {
    TS_LAUNCH(k_sde_replay_mil, bwd_grid(ntiles), BWD_THREADS, (DecSdeL::LOC + MilL::SIZE) * 4, st, blob_fwd + DecBlob::SDE,
              blob_fwd + DecMilBlob::MIL, w.best, rows, K, n_euler, step_table, na, w.states, w.H1, w.H2, w.G1, w.G2, w.GS);
    return TRAJSDE_OK;
  }
#if TSDE_SPLIT_H3
  static const bool replay_coop = []() { const char* e = getenv("TRAJSDE_REPLAY_COOP"); return !(e && e[0] == '0'); }();
  if (replay_coop) {
    TS_LAUNCH_TAG("k_sde_replay", false, k_sde_replay_coop, ntiles < 8192 ? ntiles : 8192, 256, SDE_REPLAY_COOP_LDS_BYTES, st,
                  blob_fwd + DecBlob::SDE6, w.best, rows, K, n_euler, step_table, na, w.states, w.H1, w.H2, w.G1, w.G2, w.GS);
    return TRAJSDE_OK;
  }
#endif
  TS_LAUNCH(k_sde_replay, bwd_grid(ntiles), BWD_THREADS, DecSdeL::LOC * 4, st, blob_fwd + DecBlob::SDE, w.best, rows, K, n_euler,
            step_table, na, w.states, w.H1, w.H2, w.G1, w.G2, w.GS);
  return TRAJSDE_OK;
}

// Reverse sweep of the selected paths, then the column sums of its per-wave partials (d diffusion.4.weight, its bias).  Milstein
// (tan_img = the blob's TanL image): the one-wave kernel of decoder_mil_bwd.hip.  Otherwise the cooperative form (recur.hip
// k_sde_bwd_coop: four waves a tile; fp16x3 build), or with TRAJSDE_SWEEP_COOP=0 the one-wave kernel of this file.
int launch_sweep(hipStream_t st, const float* blob_bwd, const float* tan_img, const BwdWs& w, int rows, int K, int T, int n_euler,
                 const float* step_table, const float* out_table, const NoiseArg& na, float* const* grads) {
  static_assert(SweepV::SIZE == SDE_SWEEP_V_FLOATS && SweepV::DV4 == 0 && SweepV::DC4 == 64, "recur.hip k_sde_bwd_coop writes this row");
  const bool milstein = tan_img != nullptr;
  const int ntiles = (rows + 15) / 16, waves = BWD_THREADS / 64;
  const int sweep_grid = bwd_grid(ntiles);
#if TSDE_SPLIT_H3
  static const bool sweep_coop_env = []() { const char* e = getenv("TRAJSDE_SWEEP_COOP"); return !(e && e[0] == '0'); }();
  bool sweep_coop = sweep_coop_env && !milstein;
#else
  bool sweep_coop = false;
#endif
  // (the cooperative kernel writes one SweepV row per workgroup: when vpart_slab() falls back to the workspace's shared slab -- no
  //  deferred sums active, or the arena full -- that slab bounds the rows; and its tables live in dynamic LDS, so a schedule too long
  //  for it takes the one-wave kernel, whose tables stay in global memory)
  constexpr int64_t SWEEP_ROWS_MAX = SHARED_VPART_FLOATS / SweepV::SIZE < 8192 ? SHARED_VPART_FLOATS / SweepV::SIZE : 8192;
  const int64_t coop_lds = int64_t(SDE_BWD_COOP_LDS_BYTES) + int64_t(8 * n_euler + 4 * T) * 4;
  if (sweep_coop && coop_lds > 150 * 1024) sweep_coop = false;
  const int sweep_rows = sweep_coop ? int(ntiles < SWEEP_ROWS_MAX ? ntiles : SWEEP_ROWS_MAX) : sweep_grid * waves;
  // Holds for every row domain, so it cannot fire on either route: the cooperative form writes at most SWEEP_ROWS_MAX =
  // min(262 144 / 68, 8 192) = 3 855 rows of 68 floats = 262 140 <= 262 144; the one-wave forms at most 256 workgroups x 2 waves =
  // 512 rows = 34 816 floats.  It guards a later change of SweepV, BWD_THREADS or bwd_grid().
  TS_REQUIRE(int64_t(sweep_rows) * SweepV::SIZE <= SHARED_VPART_FLOATS, "decoder backward: the sweep's partial rows exceed the shared slab");
  float* vp = vpart_slab(w.vpart, sweep_rows, SweepV::SIZE);
  if (sweep_coop) {
    const SdeBwdCoopArgs ca{blob_bwd + DecBwdBlob::SWEEP, w.best, rows, K, T, n_euler, step_table, out_table, na, w.H1, w.H2, w.G1, w.G2, w.GS,
                            w.DS, w.DH1, w.DH2, w.DF, w.DG1, w.DG2, w.DY0, vp};
    TS_LAUNCH_TAG("k_sde_bwd", false, k_sde_bwd_coop, sweep_rows, 256, int(coop_lds), st, ca);
  } else if (milstein) {
    TS_LAUNCH(k_sde_bwd_mil, sweep_grid, BWD_THREADS, (SweepL::SIZE + TanL::SIZE) * 4, st, blob_bwd + DecBwdBlob::SWEEP, tan_img, w.best, rows, K,
              T, n_euler, step_table, out_table, na, w.H1, w.H2, w.G1, w.G2, w.GS, w.DS, w.DH1, w.DH2, w.DF, w.DG1, w.DG2, w.DY0, vp, w.mil);
  } else {
    TS_LAUNCH(k_sde_bwd, sweep_grid, BWD_THREADS, SweepL::SIZE * 4, st, blob_bwd + DecBwdBlob::SWEEP, w.best, rows, K, T, n_euler, step_table,
              out_table, na, w.H1, w.H2, w.G1, w.G2, w.GS, w.DS, w.DH1, w.DH2, w.DF, w.DG1, w.DG2, w.DY0, vp);
  }
  ColsumBatch cb(st, sweep_rows, SweepV::SIZE);
  cb.add(vp + SweepV::DV4, 64, grads[G4W]);
  cb.add(vp + SweepV::DC4, 1, grads[G4B]);
  return cb.flush();
}

// the vector gradients of one head (LayerNorm weight / bias, last layer's weight / bias) from its per-wave partials at `v`:
// `head` = grads + D1W (loc head) or grads + S1W (scale head)
static_assert(D1B == D1W + 1 && D3W == D1W + 2 && D3B == D1W + 3 && S1B == S1W + 1 && S3W == S1W + 2 && S3B == S1W + 3, "head_colsums");
static_assert(int(HeadV::DGAM) == int(CotHeadV::DGAM) && int(HeadV::DBET) == int(CotHeadV::DBET) && int(HeadV::DW3X) == int(CotHeadV::DW3X) &&
                  int(HeadV::DB3) == int(CotHeadV::DB3),
              "k_head_bwd and k_head_bwd_cot flush a head's vectors at the same offsets");
void head_colsums(ColsumBatch& cb, const float* v, float* const* head) {
  cb.add(v + HeadV::DGAM, 64, head[0]);
  cb.add(v + HeadV::DBET, 64, head[1]);
  cb.add(v + HeadV::DW3X, 128, head[2]);      // rows x, y of decoder.3.weight [2,64]
  cb.add(v + HeadV::DB3, 2, head[3]);
}

// the five SDE matrices over the same (step, path) rows: one launch pair
int sde_wgrads(const WgradCtx& wc, const BwdWs& w, int rows, int n_euler, float* const* grads, bool milstein) {
  int rc;
  WgradBatch sde(wc, int64_t(rows) * n_euler, rows);
  if ((rc = sde.add(w.DH1, 64, w.states, 64, grads[F0W], 66, 0, grads[F0B], 1))) return rc;
  if ((rc = sde.add(w.DH2, 64, w.H1, 64, grads[F2W], 64, 0, grads[F2B], 0))) return rc;
  if ((rc = sde.add(w.DF, 64, w.H2, 64, grads[F4W], 64, 0, grads[F4B], 0))) return rc;
  if ((rc = sde.add(w.DG1, 64, w.states, 64, grads[G0W], 66, 0, grads[G0B], 1))) return rc;
  if ((rc = sde.add(w.DG2, 64, w.G1, 64, grads[G2W], 64, 0, grads[G2B], 0))) return rc;
  if (milstein) {                                           // the gdg term's products, into blocks of their own (k_add_mil_wgrad)
    if ((rc = sde.add(w.mil.g2b, 64, w.mil.h1t, 64, w.MW2, 64, 0, nullptr, 0))) return rc;
    if ((rc = sde.add(w.mil.g1b, 64, w.mil.u, 64, w.MW0, 64, 0, nullptr, 0))) return rc;
  }
  return sde.flush();
}

}  // namespace tsde

using namespace tsde;

extern "C" {

int64_t trajsde_decoder_backward_ws_bytes(int32_t N, int num_modes, int future_steps, int n_euler) {
  (void)num_modes;
  bool ok;
  return carve_bwd(nullptr, 0, N, future_steps, n_euler, ok).bytes;
}

int64_t trajsde_decoder_nll_backward_ws_bytes(int32_t N, int num_modes, int future_steps, int n_euler) {
  (void)num_modes;
  bool ok;
  return carve_bwd(nullptr, 0, N, future_steps, n_euler, ok, true).bytes;
}

int64_t trajsde_decoder_milstein_backward_ws_bytes(int32_t N, int num_modes, int future_steps, int n_euler) {
  (void)num_modes;
  bool ok;
  return carve_bwd(nullptr, 0, N, future_steps, n_euler, ok, true, true).bytes;      // (either loss)
}

// milstein: blob_fwd is a TRAJSDE_STAGE_DECODER_MILSTEIN image, blob_bwd a _MILSTEIN_BWD / _MILSTEIN_NLL_BWD one; the replay and the
// sweep take their one-wave Milstein kernels (the cooperative forms are Euler-only), two more weight-gradient products join the batch
static int decoder_backward_impl(bool nll, float eps, float min_scale, int32_t N, int num_modes, int future_steps, const float* blob_fwd,
                                 const float* blob_bwd, const float* local_embed, const float* global_embed, const float* step_table,
                                 int n_euler, const float* out_table, const trajsde_noise* noise, const float* loc, const float* y,
                                 const uint8_t* reg_mask, void* ws, int64_t ws_bytes, float* loss, int32_t* best_mode, float* const* grads,
                                 int n_grads, float* d_local, float* d_global, void* stream_, bool milstein = false) {
  TS_REQUIRE(blob_fwd && blob_bwd && local_embed && global_embed && step_table && out_table && loc && y && reg_mask && ws && loss &&
                 grads && d_local && d_global,
             "decoder backward: null pointer");
  TS_REQUIRE(N > 0 && num_modes > 0 && future_steps > 0 && n_euler > 0, "decoder backward: empty problem");
  const int want_grads = nll ? int(N_GRADS_NLL) : int(N_GRADS);
  TS_REQUIRE(n_grads == want_grads, "decoder backward: gradient count does not match trajsde_param_count of the backward stage");
  for (int i = 0; i < want_grads; ++i) TS_REQUIRE(grads[i] != nullptr, "decoder backward: null gradient buffer");
  if (ws_bytes < (milstein ? trajsde_decoder_milstein_backward_ws_bytes(N, num_modes, future_steps, n_euler)
                  : nll    ? trajsde_decoder_nll_backward_ws_bytes(N, num_modes, future_steps, n_euler)
                           : trajsde_decoder_backward_ws_bytes(N, num_modes, future_steps, n_euler)))
    return fail(TRAJSDE_ERR_WORKSPACE, "decoder backward: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  bool ok;
  const int K = num_modes, T = future_steps;
  BwdWs w = carve_bwd(ws, ws_bytes, N, T, n_euler, ok, nll || milstein, milstein);
  DeferredSums sums(st, w.part, w.cs, w.parts, step_table, w.varena, w.varena_floats);      // every reduction of this call: at the end
  const NoiseArg na = noise_arg(noise);
  const int ntiles = (N + 15) / 16;
  const int waves = BWD_THREADS / 64;
  int rc;

  // ---- loss, winner per actor
  {
    TS_REQUIRE(K >= 1 && K <= 256, "decoder backward: 1 <= num_modes <= 256");
    int KP = 1;
    while (KP < K) KP <<= 1;
    TS_LAUNCH(k_l2_wta, cdiv(N, 256 / KP), 256, 0, st, loc, y, reg_mask, N, K, T, w.best, w.minsum, w.cnt, KP);     // the winner is the L2 one in both losses
  }
  if (nll) {
    TS_LAUNCH(k_nll_value, cdiv(N, 256), 256, 0, st, loc, y, reg_mask, w.best, N, T, eps, w.minsum);
    TS_LAUNCH(k_nll_finalize, 1, 1024, 0, st, w.minsum, w.cnt, N, w.scal);
  } else {
    TS_LAUNCH(k_l2_finalize, 1, 1024, 0, st, w.minsum, w.cnt, N, w.scal);
  }
  TS_HIP(hipMemcpyAsync(loss, w.scal, sizeof(float), hipMemcpyDeviceToDevice, st));
  if (best_mode) TS_HIP(hipMemcpyAsync(best_mode, w.best, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, st));

  // ---- replay of the winning paths
  const float* init_img = blob_bwd + DecBwdBlob::INIT;
  TS_LAUNCH(k_init_sel, bwd_grid(ntiles), BWD_THREADS, InitBwdL::AE_END * 4, st, init_img, local_embed, global_embed, w.best, N,
            w.states, w.gsel);
  if ((rc = launch_replay(st, blob_fwd, w, N, K, n_euler, step_table, na, milstein))) return rc;

  // ---- backward: head, sweep, init
  const int head_grid = bwd_grid(ntiles * T);
  const NllArg na_nll{loc, w.best, eps, min_scale};
  const int head_waves = head_grid * waves;
  float* vp = vpart_slab(w.vpart, head_waves, HeadV::SIZE);
  if (nll)
    TS_LAUNCH(k_head_bwd<1>, head_grid, BWD_THREADS, HeadBwdL::SIZE * 4, st, blob_bwd + DecBwdBlob::HEAD, w.states, out_table, y, reg_mask,
              w.scal, N, T, w.S_in, w.DU, w.DS, vp, na_nll);
  else
    TS_LAUNCH(k_head_bwd<0>, head_grid, BWD_THREADS, HeadBwdL::SIZE * 4, st, blob_bwd + DecBwdBlob::HEAD, w.states, out_table, y, reg_mask,
              w.scal, N, T, w.S_in, w.DU, w.DS, vp, na_nll);
  {
    ColsumBatch cb(st, head_waves, HeadV::SIZE);
    head_colsums(cb, vp, grads + D1W);
    if ((rc = cb.flush())) return rc;
  }
  if (nll) {                                               // the scale head (its images follow the L2 blob: DecNllBwdBlob)
    vp = vpart_slab(w.vpart, head_waves, HeadV::SIZE);
    TS_LAUNCH(k_head_bwd<2>, head_grid, BWD_THREADS, HeadBwdL::SIZE * 4, st, blob_bwd + DecNllBwdBlob::HEAD_SC, w.states, out_table, y,
              reg_mask, w.scal, N, T, w.S_in, w.DU2, w.DS, vp, na_nll);
    ColsumBatch cb(st, head_waves, HeadV::SIZE);
    head_colsums(cb, vp, grads + S1W);
    if ((rc = cb.flush())) return rc;
  }

  const float* tan_img = milstein ? blob_bwd + (nll ? int(DecMilNllBwdBlob::TAN) : int(DecMilBwdBlob::TAN)) : nullptr;
  if ((rc = launch_sweep(st, blob_bwd, tan_img, w, N, K, T, n_euler, step_table, out_table, na, grads))) return rc;

  const int init_grid = bwd_grid(ntiles);
  TS_HIP(hipMemsetAsync(d_global, 0, size_t(K) * N * 64 * sizeof(float), st));
  vp = vpart_slab(w.vpart, int64_t(init_grid) * waves, InitV::SIZE);
  TS_LAUNCH(k_dec_init_bwd, init_grid, BWD_THREADS, InitBwdL::SIZE * 4, st, init_img, local_embed, w.gsel, w.DY0, w.best, N, w.DA, d_local,
            d_global, vp);
  {
    ColsumBatch cb(st, init_grid * waves, InitV::SIZE);
    cb.add(vp + InitV::DGAM, 64, grads[A1W]);
    cb.add(vp + InitV::DBET, 64, grads[A1B]);
    if ((rc = cb.flush())) return rc;
  }

  // ---- weight gradients: (delta rows, input rows, rows, rows per step) -> W (+ column offset), bias, time columns
  const WgradCtx wc{st, w.part, w.cs, step_table, w.parts};
  const int64_t RT = int64_t(N) * T;
  if ((rc = sde_wgrads(wc, w, N, n_euler, grads, milstein))) return rc;
  if ((rc = run_wgrad(wc, w.DU, 64, w.S_in, 64, RT, RT, grads[D0W], 64, 0, grads[D0B], 0))) return rc;
  if (nll && (rc = run_wgrad(wc, w.DU2, 64, w.S_in, 64, RT, RT, grads[S0W], 64, 0, grads[S0B], 0))) return rc;
  {
    WgradBatch init(wc, N, N);                              // aggr_embed.0 [64,128] = cat(global, local): DEC:82
    if ((rc = init.add(w.DA, 64, w.gsel, 64, grads[A0W], 128, 0, grads[A0B], 0))) return rc;
    if ((rc = init.add(w.DA, 64, local_embed, 64, grads[A0W], 128, 64, nullptr, 0))) return rc;
    if ((rc = init.flush())) return rc;
  }
  if ((rc = sums.finish())) return rc;
  if (milstein) TS_LAUNCH(k_add_mil_wgrad, 32, 256, 0, st, grads[G2W], grads[G0W], w.MW2, w.MW0);
  return TRAJSDE_OK;
}

int trajsde_decoder_l2_backward(int32_t N, int num_modes, int future_steps, const float* blob_fwd, const float* blob_bwd,
                                const float* local_embed, const float* global_embed, const float* step_table, int n_euler,
                                const float* out_table, const trajsde_noise* noise, const float* loc, const float* y,
                                const uint8_t* reg_mask, void* ws, int64_t ws_bytes, float* loss, int32_t* best_mode,
                                float* const* grads, int n_grads, float* d_local, float* d_global, void* stream_) {
  return decoder_backward_impl(false, 0.f, 0.f, N, num_modes, future_steps, blob_fwd, blob_bwd, local_embed, global_embed, step_table, n_euler,
                               out_table, noise, loc, y, reg_mask, ws, ws_bytes, loss, best_mode, grads, n_grads, d_local, d_global, stream_);
}

int trajsde_decoder_nll_backward(int32_t N, int num_modes, int future_steps, const float* blob_fwd, const float* blob_bwd,
                                 const float* local_embed, const float* global_embed, const float* step_table, int n_euler,
                                 const float* out_table, const trajsde_noise* noise, const float* loc, const float* y,
                                 const uint8_t* reg_mask, float eps, float min_scale, void* ws, int64_t ws_bytes, float* loss,
                                 int32_t* best_mode, float* const* grads, int n_grads, float* d_local, float* d_global, void* stream_) {
  TS_REQUIRE(eps > 0.f, "decoder_nll_backward: eps must be positive");
  return decoder_backward_impl(true, eps, min_scale, N, num_modes, future_steps, blob_fwd, blob_bwd, local_embed, global_embed, step_table,
                               n_euler, out_table, noise, loc, y, reg_mask, ws, ws_bytes, loss, best_mode, grads, n_grads, d_local, d_global,
                               stream_);
}

int trajsde_decoder_l2_backward_milstein(int32_t N, int num_modes, int future_steps, const float* blob_fwd, const float* blob_bwd,
                                         const float* local_embed, const float* global_embed, const float* step_table, int n_euler,
                                         const float* out_table, const trajsde_noise* noise, const float* loc, const float* y,
                                         const uint8_t* reg_mask, void* ws, int64_t ws_bytes, float* loss, int32_t* best_mode,
                                         float* const* grads, int n_grads, float* d_local, float* d_global, void* stream_) {
  return decoder_backward_impl(false, 0.f, 0.f, N, num_modes, future_steps, blob_fwd, blob_bwd, local_embed, global_embed, step_table, n_euler,
                               out_table, noise, loc, y, reg_mask, ws, ws_bytes, loss, best_mode, grads, n_grads, d_local, d_global, stream_,
                               true);
}

int trajsde_decoder_nll_backward_milstein(int32_t N, int num_modes, int future_steps, const float* blob_fwd, const float* blob_bwd,
                                          const float* local_embed, const float* global_embed, const float* step_table, int n_euler,
                                          const float* out_table, const trajsde_noise* noise, const float* loc, const float* y,
                                          const uint8_t* reg_mask, float eps, float min_scale, void* ws, int64_t ws_bytes, float* loss,
                                          int32_t* best_mode, float* const* grads, int n_grads, float* d_local, float* d_global,
                                          void* stream_) {
  TS_REQUIRE(eps > 0.f, "decoder_nll_backward: eps must be positive");
  return decoder_backward_impl(true, eps, min_scale, N, num_modes, future_steps, blob_fwd, blob_bwd, local_embed, global_embed, step_table,
                               n_euler, out_table, noise, loc, y, reg_mask, ws, ws_bytes, loss, best_mode, grads, n_grads, d_local, d_global,
                               stream_, true);
}

}  // extern "C"

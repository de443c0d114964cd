// decoder_mil_bwd.hip -- the decoder backward's kernels for `method: milstein` (trajsde_decoder_l2_backward_milstein /
// trajsde_decoder_nll_backward_milstein, host code in decoder_bwd.hip decoder_backward_impl): the forward replay with the Milstein step,
// the reverse sweep through it, and the join of its two extra weight-gradient blocks.  One-wave kernels in both builds (the cooperative
// four-wave forms of recur.hip are Euler-only).
#include "common.hpp"
#include "layouts.hpp"
#include "philox.hpp"
#include "range.hpp"
#include "sde_funcs.hpp"
#include "tile.hpp"
#include "tile_bwd.hpp"
#include "bwd.hpp"
#include "kernels.hpp"

namespace tsde {

// decoder_bwd.hip k_sde_replay with the Milstein step (k_sde_decode<.., MIL = true> in the forward): `mil_img` is the MilL image of a
// TRAJSDE_STAGE_DECODER_MILSTEIN blob, staged behind the drift and diffusion images.  Kept out of decoder_bwd.hip, like the sweep below:
// as a template flag there, or even as a second kernel in that unit, it changed the Euler kernels' register allocation; in a unit of
// its own the Euler kernels keep their name, signature and instructions.
__global__ __launch_bounds__(128) void k_sde_replay_mil(const float* __restrict__ img, const float* __restrict__ mil_img,
                                                        const int32_t* __restrict__ best, int N, int K, int n_euler,
                                                        const float* __restrict__ step_tab, NoiseArg na, float* __restrict__ states,
                                                        float* __restrict__ H1, float* __restrict__ H2, float* __restrict__ G1,
                                                        float* __restrict__ G2, float* __restrict__ GS) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_copy(lds, img, DecSdeL::LOC);                      // drift + diffusion images, MilL behind them
  stage_copy(lds + DecSdeL::LOC, mil_img, MilL::SIZE);
  __syncthreads();
  const float* mil = lds + DecSdeL::LOC;
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
      f4 J[4];                                             // GFunc's input gradient without s (1 - s) (sde_funcs.hpp)
      gfunc_input_grad(J, h1, h2, G + DiffL::W4, mil, L);
      milstein_update(y, f, gs, J, z, dt, sq);
      range_note(absmax<4>(y), RS_DEC_STATE);                 // as the forward (decoder.hip k_sde_decode<.., MIL>)
      if (row < N) store_row(y, states + (k + 1) * slab, row, L.g);
    }
  }
}

// k_sde_bwd_mil: the reverse sweep through the Milstein step y' = y + f dt + s I + c s ds/dy (c = sum_i 0.5 (I_i^2 - dt)).  Besides the Euler
// terms, the step's vjp with the adjoint u takes the gradient of Psi = c s (u . ds/dy) = c s^2 (1 - s) p' (torchsde differentiates its
// gdg vjp with create_graph: the leading s included), p' = w4 . h2' the tangent of GFunc's pre-sigmoid along u:
//   a1' = W0y u   h1' = (1 - h1^2) a1'   a2' = W2 h1'   h2' = (1 - h2^2) a2'   p' = w4 . h2'
// and its reverse, alpha = c s^2 (1 - s), beta = c p' s (1 - s) (2 s - 3 s^2), merged into the Euler chain's dL/dp (dp = dgp + beta):
//   w4 += beta h2 + alpha h2'   b4 += beta   g2b = alpha w4 (1 - h2^2)   d2 = (dp w4 - 2 alpha w4 h2 a2') (1 - h2^2)
//   W2 += d2 h1^T + g2b h1'^T   h1b' = W2^T g2b   d1 = (W2^T d2 - 2 h1b' h1 a1') (1 - h1^2)   g1b = h1b' (1 - h1^2)
//   W0 += d1 [y, sin, cos]^T + [g1b u^T | 0 0]   dL/dy_k += W0y^T d1
// The tangent products carry adjoint-scaled rows: linear_adj on the untransposed TanL image, staged behind the sweep image (SweepL + TanL
// = 114 KB of LDS: one workgroup a CU).  decoder_bwd.hip k_sde_bwd otherwise, line for line.
__global__ __launch_bounds__(128, 1) void k_sde_bwd_mil(const float* __restrict__ img, const float* __restrict__ tan_img,
                                                     const int32_t* __restrict__ best, int N, int K, int T, int n_euler,
                                                     const float* __restrict__ step_tab, const float* __restrict__ out_tab, NoiseArg na,
                                                     const float* __restrict__ H1, const float* __restrict__ H2,
                                                     const float* __restrict__ G1, const float* __restrict__ G2,
                                                     const float* __restrict__ GS, const float* __restrict__ DS,
                                                     float* __restrict__ DH1, float* __restrict__ DH2, float* __restrict__ DF,
                                                     float* __restrict__ DG1, float* __restrict__ DG2, float* __restrict__ DY0,
                                                     float* __restrict__ vpart, MilRows mr) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  stage_copy(lds, img, SweepL::SIZE);
  stage_copy(lds + SweepL::SIZE, tan_img, TanL::SIZE);
  __syncthreads();
  const float* tan = lds + SweepL::SIZE;
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
      float hv = 0.f;                                   // c = sum_i 0.5 (I_i^2 - dt), as sde_funcs.hpp milstein_update forms it
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float I = z[jt][c] * sq;
          hv += fmaf(I, I, -dt);
        }
      const float cm = 0.5f * row_sum(hv);
      const float sd = gs * (1.0f - gs);
      f4 a1[4], h1t[4], a2[4], h2t[4];                  // the tangent pass along u = dy
      zero4(a1);
      linear_adj<4, 4>(a1, dy, tan + TanL::G_W0, L);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) h1t[jt][c] = a1[jt][c] * (1.0f - ag1[jt][c] * ag1[jt][c]);
      zero4(a2);
      linear_adj<4, 4>(a2, h1t, tan + TanL::G_W2, L);
      float pd = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f4 w4 = *reinterpret_cast<const f4*>(lds + SweepL::G_W4 + 16 * jt + 4 * L.g);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          h2t[jt][c] = a2[jt][c] * (1.0f - ag2[jt][c] * ag2[jt][c]);
          pd = fmaf(w4[c], h2t[jt][c], pd);
        }
      }
      pd = row_sum(pd);
      const float alpha = cm * gs * sd, beta = cm * pd * sd * (gs * fmaf(-3.0f, gs, 2.0f));
      const float dp = dgp + beta;                      // dL/dp: the Euler term and the gdg term's
      f4 g2b[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const f4 w4 = *reinterpret_cast<const f4*>(lds + SweepL::G_W4 + 16 * jt + 4 * L.g);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float om = 1.0f - ag2[jt][c] * ag2[jt][c];
          if (live) dv4[jt][c] = fmaf(dp, ag2[jt][c], fmaf(alpha, h2t[jt][c], dv4[jt][c]));
          const float aw = alpha * w4[c];
          d[jt][c] = fmaf(dp, w4[c], -2.0f * aw * ag2[jt][c] * a2[jt][c]) * om;
          g2b[jt][c] = aw * om;
        }
      }
      if (live) {
        dc4 += dp;
        store_row(d, DG2 + k * slab, row, L.g);
        store_row(g2b, mr.g2b + k * slab, row, L.g);
        store_row(h1t, mr.h1t + k * slab, row, L.g);
        store_row(dy, mr.u + k * slab, row, L.g);
      }
      linear_t(t, d, lds + SweepL::G_W2T, L);
      f4 h1b[4];
      linear_t(h1b, g2b, lds + SweepL::G_W2T, L);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float om = 1.0f - ag1[jt][c] * ag1[jt][c];
          d[jt][c] = fmaf(-2.0f * h1b[jt][c], ag1[jt][c] * a1[jt][c], t[jt][c]) * om;
          h1b[jt][c] *= om;                             // := g1b
        }
      if (live) {
        store_row(d, DG1 + k * slab, row, L.g);
        store_row(h1b, mr.g1b + k * slab, row, L.g);
      }
      linear_adj<4, 4>(dyn, d, lds + SweepL::G_W0T, L);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) dy[jt] = dyn[jt];
    }
    if (live) store_row(dy, DY0, row, L.g);
  }
  float* vp = vpart + int64_t(blockIdx.x * waves + wave) * SDE_SWEEP_V_FLOATS;     // decoder_bwd.hip SweepV: d net.4.weight, its bias
  flush_vec(dv4, vp, L);
  flush_scalar(dc4, vp + 64, L);
}

// the Milstein sweep's two extra weight-gradient products (summed into their own 64 x 64 blocks: a reduction overwrites its W) joined to
// the Euler ones once every deferred sum has run: g_func.net.2.weight += m2, the y-columns of g_func.net.0.weight += m0
__global__ __launch_bounds__(256) void k_add_mil_wgrad(float* __restrict__ w2, float* __restrict__ w0, const float* __restrict__ m2,
                                                       const float* __restrict__ m0) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < 4096) {
    w2[j] += m2[j];
  } else if (j < 8192) {
    const int q = j - 4096;
    w0[(q >> 6) * 66 + (q & 63)] += m0[q];
  }
}

}  // namespace tsde

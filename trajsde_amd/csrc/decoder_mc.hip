// decoder_mc.hip -- Monte-Carlo decoding (include/trajsde_hip_mc.h): R sample paths of every (mode, actor) in one launch.
//
//   k_sde_decode_mc  the solve of k_sde_decode (decoder.hip) -- same device functions, same weight image, same LDS budget, same
//                    register builds -- with the 16 rows of a wave's tile holding 16 SAMPLES of ONE path instead of 16 paths:
//                    row n of tile (r, j) is sample s = 16 j + n of path r = k N + n_actor.  All rows start from the same y0 row; the
//                    Philox counter row is rid(r) + s * D (uint32), so sample 0 is the plain decoder's draw and sample s is the plain
//                    decoder's draw under row ids shifted by s * D.  Rows with s >= R compute (on sample R - 1's noise) and take part
//                    in no reduction and no store.  At each emitted output the four head values sit one per row: they are reduced
//                    over the 16 rows in registers (DPP butterflies, two passes: the tile mean, then the sums of squared deviations
//                    from it) and lane 0 writes one partial (mean[4], M2xx, M2yy, M2xy, 0) per (tile j, path, output) -- plain
//                    vector stores, no atomics, every sum in a fixed order.  R <= 8 would leave most rows of such a tile idle, so a
//                    tile then holds 16 / G paths of G = 2, 4 or 8 rows each (the smallest that holds R) and the butterflies stop
//                    at the group: R = 4 costs a quarter of R = 16, not the same.
//   k_mc_combine     merges the ceil(R / 16) partials of a path in ascending j with the pairwise (Chan et al.) update and writes
//                    loc_mean [K,N,T,4] and the unbiased loc_cov [K,N,T,3].  No sum-of-squares form anywhere: the deviations are
//                    taken from a mean before they are squared, so a large common offset of the samples costs no accuracy.
#include <cstdlib>
#include <type_traits>

#include "../../include/trajsde_hip_mc.h"
#include "common.hpp"
#include "decoder_shared.hpp"
#include "layouts.hpp"
#include "philox.hpp"
#include "range.hpp"
#include "sde_funcs.hpp"
#include "tile.hpp"

namespace tsde {

constexpr int MC_PART = 8;                                  // floats per partial: mean x, y, scale x, scale y, M2xx, M2yy, M2xy, pad

// sum over the 2^lg (lg = 1 .. 4) neighbouring lanes of a DPP row that hold one path's samples (lg = 4: the 16 rows of the tile, for
// one feature group g), the same value in every lane of the group: additions commute bit for bit, so the butterfly leaves identical
// words in all of them.  `lg` is a kernel argument: the branches are uniform.
__device__ __forceinline__ float group_sum(float v, int lg) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));                 // quad_perm [1,0,3,2]
  if (lg >= 2) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
  if (lg >= 3) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));   // row_half_mirror
  if (lg >= 4) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));   // row_mirror
  return v;
}

// R = n_samples; a path's samples sit in G = 2^lg rows of a tile (mc_group_log2: 16 unless R <= 8), in J = ceil(R / 16) tiles (1 when
// G < 16), and a tile holds 16 / G paths; stride = D of the contract (uint32 arithmetic); rows < 2^31.  Injected normals (na.z):
// [n_euler][R * rows][64], row s * rows + r.  part: [J][rows][T][MC_PART]; samples [R][rows][T][4] and loc0 [rows][T][4] may be null.
template <bool X6, int MAXT, bool MIL = false>
__global__ __launch_bounds__(MAXT) void k_sde_decode_mc(const float* __restrict__ blob, const float* __restrict__ y0, int64_t rows, int T,
                                                        int n_euler, const float* __restrict__ step_tab,
                                                        const float* __restrict__ out_tab, float min_scale, NoiseArg na, int R, int lg,
                                                        uint32_t stride, float* __restrict__ part, float* __restrict__ samples,
                                                        float* __restrict__ loc0, int st_bf16) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  using DL = typename std::conditional<X6, DecSdeL6, DecSdeL>::type;
  static_assert(!(MIL && X6) || TSDE_SPLIT_H3, "bf16x6: the split decode image and the Milstein image do not fit LDS together");
  [[maybe_unused]] constexpr int IMG = DL::SIZE + (MIL ? int(MilL::SIZE) : 0);   // the per-wave time-bias slabs follow the image(s)
  [[maybe_unused]] const float* mil = lds + DL::SIZE;
  if constexpr (MIL) {
    stage_copy(lds, blob, DL::SIZE);
    stage_copy(lds + DL::SIZE, blob + (DecMilBlob::MIL - (X6 ? DecBlob::SDE6 : DecBlob::SDE)), MilL::SIZE);
    __syncthreads();
  } else {
    stage_blob(lds, blob, DL::SIZE);
  }
  const Lane L;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6;
  const int J = lg == 4 ? (R + 15) >> 4 : 1, P = 16 >> lg;
  const int64_t ntiles = ((rows + P - 1) / P) * J;
  // tiles dealt in blocks, as in k_sde_decode; the J tiles of a path are neighbours (they read the same y0 row)
  const int64_t share = ntiles / gridDim.x, extra = ntiles % gridDim.x;
  const int64_t first = int64_t(blockIdx.x) * share + (int64_t(blockIdx.x) < extra ? int64_t(blockIdx.x) : extra);
  const int64_t mine = share + (int64_t(blockIdx.x) < extra ? 1 : 0);
  for (int64_t p = wave; p < mine; p += waves) {
    const int64_t tile = first + p;
    const int64_t q = tile / J;
    const int j = int(tile - q * J);
    const int64_t r_raw = q * P + (L.n >> lg);                 // the row's path
    const int s_raw = 16 * j + (L.n & ((1 << lg) - 1));        // ... and sample
    const bool valid = s_raw < R && r_raw < rows;
    const int r = int(r_raw < rows ? r_raw : rows - 1);        // rows past the last path or sample replay it (reads stay in bounds)
    const int s = s_raw < R ? s_raw : R - 1;
    const int cnt = lg == 4 ? (R - 16 * j < 16 ? R - 16 * j : 16) : R;      // samples of the path in this tile: 1 .. 16
    const float inv_cnt = 1.0f / float(cnt);
    f4 y[4], prev[4];
    // (the base is made opaque per tile: otherwise the compiler keeps the per-lane address y0 + 4 g alive across the whole solve,
    //  one register pair too many for the 168-register builds)
    const float* y0_tile = y0;
    asm volatile("" : "+s"(y0_tile));
    load_row_st(y, y0_tile, r, L.g, st_bf16 != 0);
    int o = 0;
    for (int k = 0; k < n_euler; ++k) {
      keep_lds_reads_here();
      const float dt = step_tab[k * 8 + 1], sq = step_tab[k * 8 + 2], sn = step_tab[k * 8 + 3], cs = step_tab[k * 8 + 4];
      f4 f[4], z[4];
      [[maybe_unused]] f4 Jg[4];                               // (Milstein only: GFunc's input gradient without s (1 - s))
      float gs;
#if TSDE_SPLIT_H3
      if constexpr (X6) {
        float* tb = lds + IMG + wave * 128;
        __builtin_amdgcn_wave_barrier();                       // the previous step's reads of the slot are done (same wave, in order)
        sde_time_bias(tb, lds, sn, cs, L.lane);
        sde_time_bias(tb, lds, sn, cs, L.lane + 64);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if constexpr (MIL) sde_fg_eval_mil(f, gs, Jg, y, lds, tb, mil, L);
        else sde_fg_eval(f, gs, y, lds, tb, L);
      } else
#else
      if constexpr (X6) {
        drift_eval_x6(f, y, lds + DL::F, sn, cs, L);
        gs = diff_eval_x6(y, lds + DL::G, sn, cs, L);
      } else
#endif
      {
        drift_eval(f, y, lds + DL::F, sn, cs, L);
        if constexpr (MIL) gs = diff_eval_mil(Jg, y, lds + DL::G, sn, cs, mil, L);
        else gs = diff_eval(y, lds + DL::G, sn, cs, L);
      }
      if (na.z != nullptr) {
        const float* zp = na.z + ((int64_t(k) * R + s) * rows + r) * D + 4 * L.g;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) z[jt] = *reinterpret_cast<const f4*>(zp + 16 * jt);
      } else {
        const uint32_t rid = (na.row_ids ? uint32_t(na.row_ids[r]) : uint32_t(r)) + uint32_t(s) * stride;
        const uint64_t key = noise_key(na);
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) z[jt] = philox_normal4(key, STREAM_DECODER, uint32_t(k), rid, uint32_t(4 * jt + L.g));
      }
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) prev[jt] = y[jt];
      if constexpr (MIL) milstein_update(y, f, gs, Jg, z, dt, sq);
      else em_update(y, f, gs, z, dt, sq);
      range_note(absmax<4>(y), RS_DEC_STATE);                 // the state is the next step's (and the heads') split operand
      while (o < T && int(out_tab[o * 4]) == k + 1) {
        keep_lds_reads_here();
        const float w0 = out_tab[o * 4 + 1], w1 = out_tab[o * 4 + 2];
        f4 st[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
          for (int c = 0; c < 4; ++c) st[jt][c] = w0 * prev[jt][c] + w1 * y[jt][c];
        float lx, ly, sx, sy;
#if TSDE_SPLIT_H3
        if constexpr (X6) head_pair_eval(lx, ly, sx, sy, st, lds + DL::LOC, L);
        else
#endif
        {
          head_eval(lx, ly, st, lds + DL::LOC, L);
          head_eval(sx, sy, st, lds + DL::SCALE, L);
        }
        sx = (sx > 0.f ? sx : fast_exp(sx) - 1.0f) + 1.0f + min_scale;       // ELU(alpha=1) + 1 + min_scale (DEC:97-98)
        sy = (sy > 0.f ? sy : fast_exp(sy) - 1.0f) + 1.0f + min_scale;
        const f4 v = {lx, ly, sx, sy};
        if (valid && L.g == 0) {
          if (samples != nullptr) *reinterpret_cast<f4*>(samples + ((int64_t(s) * rows + r) * T + o) * 4) = v;
          if (loc0 != nullptr && s == 0) *reinterpret_cast<f4*>(loc0 + (int64_t(r) * T + o) * 4) = v;
        }
        // pass 1: the mean of the four channels over the path's samples in this tile, as a first estimate of it (the plain sum) plus
        // the mean of the deviations from that estimate -- the second sum carries the samples' spread, not their common offset;
        // pass 2: the sums of the squared deviations from that mean
        f4 mean;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float pivot = group_sum(valid ? v[c] : 0.f, lg) * inv_cnt;
          mean[c] = pivot + group_sum(valid ? v[c] - pivot : 0.f, lg) * inv_cnt;
        }
        const float dx = valid ? lx - mean[0] : 0.f, dy = valid ? ly - mean[1] : 0.f;
        const f4 m2 = {group_sum(dx * dx, lg), group_sum(dy * dy, lg), group_sum(dx * dy, lg), 0.f};
        if (L.g == 0 && (L.n & ((1 << lg) - 1)) == 0 && r_raw < rows) {
          float* pq = part + ((int64_t(j) * rows + r) * T + o) * MC_PART;
          *reinterpret_cast<f4*>(pq) = mean;
          *reinterpret_cast<f4*>(pq + 4) = m2;
        }
        ++o;
      }
    }
  }
}

// one thread per (path, output): the J partials in ascending j, pairwise update of (count, mean, M2)
__global__ __launch_bounds__(256) void k_mc_combine(const float* __restrict__ part, int64_t cells /* rows * T */, int R,
                                                    float* __restrict__ loc_mean, float* __restrict__ loc_cov) {
  const int J = (R + 15) >> 4;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < cells; i += int64_t(gridDim.x) * blockDim.x) {
    const f4 m0 = *reinterpret_cast<const f4*>(part + i * MC_PART);
    f4 m2 = *reinterpret_cast<const f4*>(part + i * MC_PART + 4);
    // the running mean is kept as m0 + off: `off` is of the size of the samples' spread, so the updates round at that size and the
    // mean is rounded at its own size once, whatever the number of tiles
    f4 off = {0.f, 0.f, 0.f, 0.f};
    float na = float(R < 16 ? R : 16);                          // (one tile when R <= 16, whatever the group width)
    for (int j = 1; j < J; ++j) {
      const float* q = part + (int64_t(j) * cells + i) * MC_PART;
      const f4 mb = *reinterpret_cast<const f4*>(q), m2b = *reinterpret_cast<const f4*>(q + 4);
      const float nb = float(R - 16 * j < 16 ? R - 16 * j : 16), n = na + nb;
      const float wb = nb / n, wab = na * wb;                  // n_b / n,  n_a n_b / n
      const f4 d = (mb - m0) - off;                            // mean_b - mean_a
      off += d * wb;
      m2[0] += m2b[0] + d[0] * d[0] * wab;
      m2[1] += m2b[1] + d[1] * d[1] * wab;
      m2[2] += m2b[2] + d[0] * d[1] * wab;
      na = n;
    }
    const f4 mean = m0 + off;
    const float u = 1.0f / float(R - 1);
    *reinterpret_cast<f4*>(loc_mean + i * 4) = mean;
    loc_cov[i * 3 + 0] = m2[0] * u;
    loc_cov[i * 3 + 1] = m2[1] * u;
    loc_cov[i * 3 + 2] = m2[2] * u;
  }
}

// rows of a tile that hold one path's samples, as a power of two: 16 unless R <= 8
static int mc_group_log2(int R) { return R > 8 ? 4 : R > 4 ? 3 : R > 2 ? 2 : 1; }

static bool mc_sizes_ok(int32_t N, int num_modes, int future_steps, int n_samples) {
  return N > 0 && num_modes > 0 && future_steps > 0 && n_samples >= 2 && n_samples <= TRAJSDE_MC_MAX_SAMPLES;
}

}  // namespace tsde

using namespace tsde;

extern "C" {

int64_t trajsde_decoder_mc_ws_bytes(int32_t N, int num_modes, int future_steps, int n_samples) {
  if (!mc_sizes_ok(N, num_modes, future_steps, n_samples)) {
    fail(TRAJSDE_ERR_INVALID, "decoder_mc_ws_bytes: N, num_modes, future_steps > 0 and 2 <= n_samples <= 65536");
    return -1;
  }
  const int64_t rows = int64_t(N) * num_modes, J = (n_samples + 15) / 16;
  return align_up(rows * 64 * 4, 256) + align_up(J * rows * future_steps * MC_PART * 4, 256) + 256;
}

int32_t trajsde_decoder_forward_mc(int32_t N, int num_modes, int future_steps, int milstein, const float* blob, const float* local_embed,
                               const float* global_embed, const float* step_table, int n_euler, const float* out_table,
                               float min_scale, const trajsde_noise* noise, int n_samples, int64_t sample_stride, void* ws,
                               int64_t ws_bytes, float* loc_mean, float* loc_cov, float* samples, float* loc0, float* pi,
                               void* stream_) {
  TS_REQUIRE(blob && local_embed && global_embed && step_table && out_table && loc_mean && loc_cov && pi && ws,
             "decoder_forward_mc: null pointer");
  TS_REQUIRE(N > 0 && num_modes > 0 && future_steps > 0 && n_euler > 0, "decoder_forward_mc: empty problem");
  TS_REQUIRE(n_samples >= 2, "decoder_forward_mc: n_samples must be at least 2 (one sample is trajsde_decoder_forward)");
  TS_REQUIRE(n_samples <= TRAJSDE_MC_MAX_SAMPLES, "decoder_forward_mc: n_samples above 65536");
  const int64_t rows = int64_t(N) * num_modes;
  TS_REQUIRE(rows < (int64_t(1) << 31), "decoder_forward_mc: num_modes * N must be below 2^31");
  // the largest counter row is max_rid + (R - 1) D, with max_rid = K N - 1 for local ids: it must stay below 2^32
  TS_REQUIRE(sample_stride >= 1 && sample_stride <= ((int64_t(1) << 32) - rows) / (n_samples - 1),
             "decoder_forward_mc: sample_stride must be >= 1 with (n_samples - 1) * sample_stride + num_modes * N <= 2^32 "
             "(the Philox counter row is 32 bits)");
  if (ws_bytes < trajsde_decoder_mc_ws_bytes(N, num_modes, future_steps, n_samples))
    return fail(TRAJSDE_ERR_WORKSPACE, "decoder_forward_mc: workspace too small");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Carver cv(ws, ws_bytes);
  const int J = (n_samples + 15) / 16;
  float* y0 = cv.take<float>(rows * 64);
  float* part = cv.take<float>(int64_t(J) * rows * future_steps * MC_PART);
  if (const int rc = decoder_init(N, num_modes, blob, local_embed, global_embed, y0, pi, stream)) return rc;
  const int lg = mc_group_log2(n_samples);
  const int64_t ntiles = lg == 4 ? rows * J : (rows + (16 >> lg) - 1) / (16 >> lg);
  // thread counts, register builds and LDS budget: decoder.hip decoder_forward(), which see
  static const int dthreads = []() { const char* v = getenv("TRAJSDE_THREADS_DECODE"); const int t = v ? atoi(v) : 768; return (t >= 64 && t <= 768 && t % 64 == 0) ? t : 768; }();
  static const bool x6 = []() { const char* e = getenv("TRAJSDE_DECODE_FP32"); return !(e && atoi(e) != 0); }();
  auto fit = [&](int image_floats) {
    int t = dthreads;
    while (t > 64 && (image_floats + (t / 64) * 128) * 4 > 160 * 1024) t -= 64;
    return t;
  };
  const uint32_t stride = uint32_t(sample_stride);            // (2^32 itself is only admitted with rows = 0: never)
#define TS_DECODE_MC(X6, MAXT, MIL, IMGF, OFF, DT)                                                                               \
  TS_LAUNCH((k_sde_decode_mc<X6, MAXT, MIL>), pick_grid(ntiles, (DT) / 64), (DT), ((IMGF) + ((DT) / 64) * 128) * 4, stream, blob + OFF, \
            y0, rows, future_steps, n_euler, step_table, out_table, min_scale, to_arg(noise), n_samples, lg, stride, part, samples, loc0, \
            state_bf16() ? 1 : 0)
  if (milstein) {
    const int dm1 = fit(DecSdeL::SIZE + MilL::SIZE);
#if TSDE_SPLIT_H3
    const int dm6 = fit(DecSdeL6::SIZE + MilL::SIZE);
    if (x6 && dm6 <= 512) TS_DECODE_MC(true, 512, true, DecSdeL6::SIZE + MilL::SIZE, DecBlob::SDE6, dm6);
    else if (x6) TS_DECODE_MC(true, 768, true, DecSdeL6::SIZE + MilL::SIZE, DecBlob::SDE6, dm6);
    else if (dm1 <= 512) TS_DECODE_MC(false, 512, true, DecSdeL::SIZE + MilL::SIZE, DecBlob::SDE, dm1);
    else TS_DECODE_MC(false, 768, true, DecSdeL::SIZE + MilL::SIZE, DecBlob::SDE, dm1);
#else
    TS_DECODE_MC(false, 512, true, DecSdeL::SIZE + MilL::SIZE, DecBlob::SDE, dm1 < 512 ? dm1 : 512);
#endif
  } else {
    const int dt6 = fit(DecSdeL6::SIZE), dt1 = fit(DecSdeL::SIZE);
#if TSDE_SPLIT_H3
    if (x6 && dt6 <= 512) TS_DECODE_MC(true, 512, false, DecSdeL6::SIZE, DecBlob::SDE6, dt6);
    else if (x6) TS_DECODE_MC(true, 768, false, DecSdeL6::SIZE, DecBlob::SDE6, dt6);
    else if (dt1 <= 512) TS_DECODE_MC(false, 512, false, DecSdeL::SIZE, DecBlob::SDE, dt1);
    else TS_DECODE_MC(false, 768, false, DecSdeL::SIZE, DecBlob::SDE, dt1);
#else
    // bf16x6: the 768-thread (168-register) builds of this solve spill -- k_sde_decode's do too -- and the sample bookkeeping adds to
    // it: the 512-thread (256-register) builds only, which hold everything in registers
    if (x6) TS_DECODE_MC(true, 512, false, DecSdeL6::SIZE, DecBlob::SDE6, dt6 < 512 ? dt6 : 512);
    else TS_DECODE_MC(false, 512, false, DecSdeL::SIZE, DecBlob::SDE, dt1 < 512 ? dt1 : 512);
#endif
  }
#undef TS_DECODE_MC
  const int64_t cells = rows * future_steps;
  const int64_t cgrid = (cells + 255) / 256;
  TS_LAUNCH(k_mc_combine, int(cgrid < 1 ? 1 : (cgrid > 4096 ? 4096 : cgrid)), 256, 0, stream, part, cells, n_samples, loc_mean, loc_cov);
  return TRAJSDE_OK;
}

}  // extern "C"

// wgrad.hip -- the weight-gradient and deferred-sum engine of the whole backward pass for gfx950 (declared in wgrad.hpp): every backward
// unit (decoder_bwd, decoder_cot_bwd, node_bwd, aggregator_bwd, encoder_bwd, grid_bwd, grid_cot_bwd) hands its saved rows and its per-wave
// vector partials to the batches below.
//
//   k_wgrad / k_reduce_partials   dW = sum_rows delta^T a  as MFMA outer products over saved rows (deterministic
//                              two-stage reduction), bias = column sums, time-feature columns = step-weighted sums
//   k_wgrad6 / k_wgrad6_edge   the same partial sums on the 16-bit matrix cores (fp16x3 build); the edge embedding's three problems
//   k_colsum / k_colsum_slices per-wave vector partials -> one vector
//   ReduceQueue / ColsumQueue / DeferredSums   the sums of a whole entry point in a few wide launches at its end
//
// The weight gradients (k_wgrad) are always exact fp32 in the bf16x6 build; TRAJSDE_WGRAD_F32=1 selects that kernel in the fp16x3 build.
#include <cstdlib>

#include "common.hpp"
#include "layouts.hpp"
#include "tile.hpp"
#include "wgrad.hpp"

namespace tsde {

// ------------------------------------------------------------------ weight gradients from saved rows
// part[p] = sum_{rows of chunk p} delta[r][:]^T a[r][:]  (64x64, [o][i]),  cs[p][o] = sum delta[r][o].
// Chunks never straddle a group (= one Euler step of rows_per_group rows), so the reducer can weight them per step.
__global__ __launch_bounds__(256, 3) void k_wgrad(WgradJobs jobs, int64_t R, int64_t rows_per_group, int chunk, int chunks_per_group, int P,
                                               float* __restrict__ part, float* __restrict__ cs) {
  const WgradJob& job = jobs.j[blockIdx.y];
  const float* __restrict__ delta = job.delta;
  const float* __restrict__ a = job.a;
  const int ldd = job.ldd, lda = job.lda;
  part += int64_t(blockIdx.y) * P * 4096;
  cs += int64_t(blockIdx.y) * P * 64;
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const int p = blockIdx.x;
  const int group = p / chunks_per_group, sub = p - group * chunks_per_group;
  const int64_t row0 = group * rows_per_group + int64_t(sub) * chunk;
  int64_t row1 = row0 + chunk;
  if (row1 > (group + 1) * rows_per_group) row1 = (group + 1) * rows_per_group;
  if (row1 > R) row1 = R;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, idx = lane & 15, kg = lane >> 4;
  // Wave `ot` owns output rows 16 ot .. 16 ot + 15 of the 64 x 64 block and walks ALL 4-row k-steps of a staged block: 16
  // accumulator registers per lane instead of 64 (every wave holding the whole block and taking every 4th k-step), so four
  // workgroups fit a CU between the barriers instead of two, and no cross-wave reduction at the end.
  const int ot = wave;
  f4 acc[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) acc[it] = f4{0.f, 0.f, 0.f, 0.f};
  float csum = 0.f;
  // 64-row blocks of delta and a are staged in LDS TRANSPOSED -- [feature][row], the row index XOR-ed with a per-feature multiple
  // of 4 -- so that a lane's 16 operand values of a block are 4 aligned 16-byte reads, all issued before the block's 64 matrix
  // instructions (reading them one k-step at a time put an LDS round trip in front of every pair of matrix instructions: the
  // pipe was 60 % busy).  The contraction index is permuted to make that possible: k-step j sums rows {j, 16+j, 32+j, 48+j} of the
  // block (lane group kg holds rows 16 kg .. 16 kg + 15), the same permutation for both operands.  The XOR term 4 ((f & 15) ^ (f >> 4))
  // spreads the 16 features a read instruction touches over all banks, and the 64 scalar writes of a wave over all 32 write banks.
  float* ds_ = dyn;                       // [64 features][64 rows]
  float* as_ = dyn + 4096;                // [64 features][64 rows]
  const int c4w = threadIdx.x & 15;
  int wofs[4];                            // this thread's four features: f * 64, with the swizzle term kept apart in wswz
  int wswz[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int f = 4 * c4w + j;
    wofs[j] = f * 64;
    wswz[j] = 4 * ((f & 15) ^ (f >> 4));
  }
  const float* a_rd = ds_ + (16 * ot + idx) * 64;           // operand reads: feature rows of this lane
  const int a_sw = 4 * (idx ^ ot);
  // software pipeline: the global loads (or the computed operand) of block k+1 are issued before the matrix work of block
  // k, so their latency hides behind it; registers -> LDS happens after the barrier that retires block k's reads
  f4 dreg[4], areg[4];
  const bool computed = job.in2 != nullptr;             // uniform per launch slice (blockIdx.y)
  const int pair = job.pair;
  // the computed operand is built from the row's geometry AFTER the barrier that opens the next block (`finish`), not where the
  // geometry is fetched: its consumer would otherwise wait out the load right in front of the matrix loop, every block
  auto fetch = [&](int64_t blk) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int f = threadIdx.x + 256 * u;            // float4 index within the 64 x 16 block
      const int r = f >> 4, c4 = f & 15;
      const int64_t row = blk + r;
      f4 dv = f4{0.f, 0.f, 0.f, 0.f}, av = dv;
      if (row < row1) {
        dv = *reinterpret_cast<const f4*>(delta + row * ldd + 4 * c4);
        av = computed ? *reinterpret_cast<const f4*>(a + row * 4) : *reinterpret_cast<const f4*>(a + row * lda + 4 * c4);
      }
      dreg[u] = dv;
      areg[u] = av;
    }
  };
  auto finish = [&](int64_t blk) {                      // in2_rstd / in2_ln_relu4 (tile.hpp)
    // a thread always produces the same four features (4 * (threadIdx.x & 15)); their closed-form constants are re-read per block
    // (cache hits) rather than held in 24 registers across the matrix loop
    const int f0 = 4 * (threadIdx.x & 15);
    const f4 kw0 = *reinterpret_cast<const f4*>(job.in2 + f0), kw1 = *reinterpret_cast<const f4*>(job.in2 + 64 + f0);
    const f4 kgb = *reinterpret_cast<const f4*>(job.in2 + 128 + f0), kbe = *reinterpret_cast<const f4*>(job.beta + f0);
    const f4 kc0 = *reinterpret_cast<const f4*>(job.in2 + 192), kc1 = *reinterpret_cast<const f4*>(job.in2 + 196);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = (threadIdx.x + 256 * u) >> 4;
      const f4 ge = areg[u];
      const float x0 = pair ? ge[2] : ge[0], x1 = pair ? ge[3] : ge[1];
      const float ca = fmaf(kc0[0], x0, fmaf(kc0[1], x1, kc0[2])), cb = fmaf(kc0[3], x1, kc1[0]);
      const float rstd = rsqrt_nr(fmaf(ca, ca, fmaf(cb, cb, kc1[1] * kc1[1])) + 1e-5f);
      const float x0r = x0 * rstd, x1r = x1 * rstd;
      f4 av;
#pragma unroll
      for (int k = 0; k < 4; ++k) av[k] = fmaxf(fmaf(kw0[k], x0r, fmaf(kw1[k], x1r, fmaf(kgb[k], rstd, kbe[k]))), 0.f);
      areg[u] = blk + r < row1 ? av : f4{0.f, 0.f, 0.f, 0.f};
    }
  };
  if (row0 < row1) fetch(row0);
  for (int64_t blk = row0; blk < row1; blk += 64) {
    __syncthreads();
    if (computed) finish(blk);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = (threadIdx.x + 256 * u) >> 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ds_[wofs[j] + (r ^ wswz[j])] = dreg[u][j];
        as_[wofs[j] + (r ^ wswz[j])] = areg[u][j];
      }
    }
    __syncthreads();
    if (blk + 64 < row1) fetch(blk + 64);
    f4 A[4], B[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m) A[m] = *reinterpret_cast<const f4*>(a_rd + ((16 * kg + 4 * m) ^ a_sw));
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int m = 0; m < 4; ++m) B[q][m] = *reinterpret_cast<const f4*>(as_ + (16 * q + idx) * 64 + ((16 * kg + 4 * m) ^ (4 * (idx ^ q))));
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        csum += A[m][c];
#pragma unroll
        for (int it = 0; it < 4; ++it) acc[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[m][c], B[it][m][c], acc[it], 0, 0, 0);
      }
  }
  // D fragment: lane holds dW[16 ot + 4 kg + reg][16 it + idx]
  float* out = part + int64_t(p) * 4096;
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) out[(16 * ot + 4 * kg + reg) * 64 + 16 * it + idx] = acc[it][reg];
  csum += __shfl_xor(csum, 16);                             // the four k-groups of column 16 ot + idx
  csum += __shfl_xor(csum, 32);
  if (kg == 0) cs[int64_t(p) * 64 + 16 * ot + idx] = csum;
}

#if TSDE_SPLIT_H3
// ---- the same partial sums on the 16-bit matrix cores (fp16x3: a_h b_h + a_h b_l + a_l b_h, tile.hpp), the default in this build.
// The fp32 matrix instruction runs at 1/16 of the 16-bit rate: at 8 192 flops per row the exact kernel above is bound by it (0.85 ms
// of matrix pipe for the 4.55 M edge rows of a 64 x 128 step, the same as streaming their 4.8 GB); three 16-bit products take a fifth of
// that and leave the kernel to HBM.  Both operands of a block are scaled by a power of two taken from the block's largest magnitude (deltas
// are tiny, fp16 has 5 exponent bits: the same reason tile.hpp linear_adj scales rows), split into hi / lo halves when the block is
// staged, and the block's product is scaled back when it joins the fp32 accumulator.  The contraction runs over ROWS, which sit on the
// lanes' row index in global memory order: the planes are staged row-major ([64 rows][64 halves], 8-byte chunks XOR-swizzled) and read
// through ds_read_b64_tr_b16, which hands lane i of a 16-lane group column i of four rows -- an operand fragment, no transposing writes
// (lane map checked on the hardware: tools/microbench/trread.hip).
typedef short s4v __attribute__((__vector_size__(4 * sizeof(short))));
__device__ __forceinline__ int wg6_off(int r, int c) {      // byte offset of chunk c (4 halves) of row r: conflict-free for the stores and the transposed reads
  return r * 128 + 8 * (c ^ ((((r >> 1) & 1) | (((r >> 3) & 1) << 1)) << 2));
}
__device__ __forceinline__ h8 wg6_frag(const char* plane, int off0, int off1) {
  const s4v x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(plane + off0));
  const s4v y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(plane + off1));
  const uint2 a = __builtin_bit_cast(uint2, x), b = __builtin_bit_cast(uint2, y);
  return __builtin_bit_cast(h8, u4{a.x, a.y, b.x, b.y});
}
// 2^(14 - floor(log2 m)) and its inverse for a block whose largest magnitude is m (0 / 0 for an all-zero or sub-2^-113 block)
__device__ __forceinline__ void wg6_scale(float m, float& up, float& down) {
  const unsigned e = __float_as_uint(m) & 0x7F800000u;
  const bool ok = e >= (14u << 23);
  up = ok ? __uint_as_float(0x86000000u - e) : 0.f;
  down = ok ? __uint_as_float(e - (14u << 23)) : 0.f;
}
#ifndef TSDE_WG6_OCC
#define TSDE_WG6_OCC 3
#endif
// One workgroup's rows [row0, row1) of one problem -- or, DUAL, of the TWO computed-operand problems of an edge embedding (branch A from
// geometry columns 0-1, branch B from columns 2-3), which contract the same delta rows: the delta planes are staged once and every
// delta fragment feeds both products (the pair read the 256-byte delta row twice as separate problems: 24 % of the launch's bytes).
// Per problem the arithmetic is that of the single form: same block scales, same products, same order.
template <bool DUAL>
__device__ __forceinline__ void wgrad6_rows(const WgradJob& job, const WgradJob& jobB, int64_t row0, int64_t row1, float* __restrict__ out,
                                            float* __restrict__ outB, float* __restrict__ csout, float* __restrict__ csoutB, char* smem) {
  const float* __restrict__ delta = job.delta;
  const float* __restrict__ a = job.a;
  const int ldd = job.ldd, lda = job.lda;
  char* const dh = smem;                               // [64 rows][64 halves] planes: delta hi / lo, a hi / lo (, the second a hi / lo)
  char* const dl = smem + 8192;
  char* const ah = smem + 16384;
  char* const al = smem + 24576;
  char* const bh = smem + 32768;
  char* const bl = smem + 40960;
  constexpr int NM = DUAL ? 3 : 2;                     // block maxima per wave
  float* const slots = reinterpret_cast<float*>(smem + (DUAL ? 49152 : 32768));      // [parity][wave][NM]
  const int lane = threadIdx.x & 63, ot = threadIdx.x >> 6, idx = lane & 15, kg = lane >> 4;
  f4 acc[4], acc2[4], csum4 = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int it = 0; it < 4; ++it) acc[it] = acc2[it] = f4{0.f, 0.f, 0.f, 0.f};
  f4 dreg[4], areg[4], breg[4];
  const bool computed = DUAL || job.in2 != nullptr;
  const int c4w = threadIdx.x & 15, r0w = threadIdx.x >> 4;
  auto fetch = [&](int64_t blk) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t row = blk + r0w + 16 * u;
      f4 dv = f4{0.f, 0.f, 0.f, 0.f}, av = dv;
      if (row < row1) {
        dv = *reinterpret_cast<const f4*>(delta + row * ldd + 4 * c4w);
        av = computed ? *reinterpret_cast<const f4*>(a + row * 4) : *reinterpret_cast<const f4*>(a + row * lda + 4 * c4w);
      }
      dreg[u] = dv;
      areg[u] = av;
    }
  };
  // the computed operand from the row's geometry record `ge` (see k_wgrad): ReLU(LN(Linear(2, 64))) in its closed form
  auto finish = [&](const WgradJob& jb, f4 (&dst)[4], int64_t blk) {
    const int f0 = 4 * c4w, pair = jb.pair;
    const f4 kw0 = *reinterpret_cast<const f4*>(jb.in2 + f0), kw1 = *reinterpret_cast<const f4*>(jb.in2 + 64 + f0);
    const f4 kgb = *reinterpret_cast<const f4*>(jb.in2 + 128 + f0), kbe = *reinterpret_cast<const f4*>(jb.beta + f0);
    const f4 kc0 = *reinterpret_cast<const f4*>(jb.in2 + 192), kc1 = *reinterpret_cast<const f4*>(jb.in2 + 196);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const f4 ge = areg[u];
      const float x0 = pair ? ge[2] : ge[0], x1 = pair ? ge[3] : ge[1];
      const float ca = fmaf(kc0[0], x0, fmaf(kc0[1], x1, kc0[2])), cb = fmaf(kc0[3], x1, kc1[0]);
      const float rstd = rsqrt_nr(fmaf(ca, ca, fmaf(cb, cb, kc1[1] * kc1[1])) + 1e-5f);
      const float x0r = x0 * rstd, x1r = x1 * rstd;
      f4 av;
#pragma unroll
      for (int k = 0; k < 4; ++k) av[k] = fmaxf(fmaf(kw0[k], x0r, fmaf(kw1[k], x1r, fmaf(kgb[k], rstd, kbe[k]))), 0.f);
      dst[u] = blk + r0w + 16 * u < row1 ? av : f4{0.f, 0.f, 0.f, 0.f};
    }
  };
  // this lane's fragment addresses: rows 32 ks + 8 kg + 4 half + q, chunk 4 * (16-column block) + p   (q = idx >> 2, p = idx & 3)
  const int fq = idx >> 2, fp = idx & 3;
  if (row0 < row1) fetch(row0);
  for (int64_t blk = row0; blk < row1; blk += 64) {
    if constexpr (DUAL) finish(jobB, breg, blk);        // (before areg's geometry is overwritten in place)
    if (computed) finish(job, areg, blk);
    float md = 0.f, ma = 0.f, mb = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        md = fmaxf(md, fabsf(dreg[u][c]));
        ma = fmaxf(ma, fabsf(areg[u][c]));
        if constexpr (DUAL) mb = fmaxf(mb, fabsf(breg[u][c]));
      }
#pragma unroll
    for (int sft = 1; sft < 64; sft <<= 1) {
      md = fmaxf(md, __shfl_xor(md, sft));
      ma = fmaxf(ma, __shfl_xor(ma, sft));
      if constexpr (DUAL) mb = fmaxf(mb, __shfl_xor(mb, sft));
    }
    float* const sl = slots + 4 * NM * (int((blk - row0) >> 6) & 1);  // two sets by block parity: a set is rewritten two barriers after its last read
    if (lane == 0) {
      sl[NM * ot] = md;
      sl[NM * ot + 1] = ma;
      if constexpr (DUAL) sl[NM * ot + 2] = mb;
    }
    __syncthreads();                                    // every wave is done with the previous block's planes; the maxima are visible
    md = fmaxf(fmaxf(sl[0], sl[NM]), fmaxf(sl[2 * NM], sl[3 * NM]));
    ma = fmaxf(fmaxf(sl[1], sl[NM + 1]), fmaxf(sl[2 * NM + 1], sl[3 * NM + 1]));
    if constexpr (DUAL) mb = fmaxf(fmaxf(sl[2], sl[NM + 2]), fmaxf(sl[2 * NM + 2], sl[3 * NM + 2]));
    float up_d, down_d, up_a, down_a, up_b = 0.f, down_b = 0.f;
    wg6_scale(md, up_d, down_d);
    wg6_scale(ma, up_a, down_a);
    if constexpr (DUAL) wg6_scale(mb, up_b, down_b);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int off = wg6_off(r0w + 16 * u, c4w);
      const f4 dv = dreg[u] * up_d, av = areg[u] * up_a;
      unsigned h0, l0, h1, l1;
      split_pair(dv[0], dv[1], h0, l0);
      split_pair(dv[2], dv[3], h1, l1);
      *reinterpret_cast<uint2*>(dh + off) = uint2{h0, h1};
      *reinterpret_cast<uint2*>(dl + off) = uint2{l0, l1};
      split_pair(av[0], av[1], h0, l0);
      split_pair(av[2], av[3], h1, l1);
      *reinterpret_cast<uint2*>(ah + off) = uint2{h0, h1};
      *reinterpret_cast<uint2*>(al + off) = uint2{l0, l1};
      if constexpr (DUAL) {
        const f4 bv = breg[u] * up_b;
        split_pair(bv[0], bv[1], h0, l0);
        split_pair(bv[2], bv[3], h1, l1);
        *reinterpret_cast<uint2*>(bh + off) = uint2{h0, h1};
        *reinterpret_cast<uint2*>(bl + off) = uint2{l0, l1};
      }
      csum4 += dreg[u];
    }
    __syncthreads();
    if (blk + 64 < row1) fetch(blk + 64);
    f4 accb[4], accb2[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) accb[it] = accb2[it] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int rA = 32 * ks + 8 * kg + fq;
      const int oa0 = wg6_off(rA, 4 * ot + fp), oa1 = wg6_off(rA + 4, 4 * ot + fp);
      const h8 Ah = wg6_frag(dh, oa0, oa1), Al = wg6_frag(dl, oa0, oa1);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int ob0 = wg6_off(rA, 4 * it + fp), ob1 = wg6_off(rA + 4, 4 * it + fp);
        const h8 Bh = wg6_frag(ah, ob0, ob1), Bl = wg6_frag(al, ob0, ob1);
        accb[it] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bh, accb[it], 0, 0, 0);
        accb[it] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bl, accb[it], 0, 0, 0);
        accb[it] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al, Bh, accb[it], 0, 0, 0);
        if constexpr (DUAL) {
          const h8 Ch = wg6_frag(bh, ob0, ob1), Cl = wg6_frag(bl, ob0, ob1);
          accb2[it] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Ch, accb2[it], 0, 0, 0);
          accb2[it] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Cl, accb2[it], 0, 0, 0);
          accb2[it] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al, Ch, accb2[it], 0, 0, 0);
        }
      }
    }
    const float down = down_d * down_a, down2 = down_d * down_b;
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[it][c] = fmaf(accb[it][c], down, acc[it][c]);
        if constexpr (DUAL) acc2[it][c] = fmaf(accb2[it][c], down2, acc2[it][c]);
      }
  }
  // D fragment: lane holds dW[16 ot + 4 kg + reg][16 it + idx]
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      out[(16 * ot + 4 * kg + reg) * 64 + 16 * it + idx] = acc[it][reg];
      if constexpr (DUAL) outB[(16 * ot + 4 * kg + reg) * 64 + 16 * it + idx] = acc2[it][reg];
    }
  // column sums of delta (exact fp32, from the rows as they were fetched): this thread's four features over its rows -> the block's
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    csum4[c] += __shfl_xor(csum4[c], 16);
    csum4[c] += __shfl_xor(csum4[c], 32);
  }
  __syncthreads();
  f4* red = reinterpret_cast<f4*>(smem);
  if (lane < 16) red[ot * 16 + lane] = csum4;
  __syncthreads();
  if (threadIdx.x < 16) {
    const f4 t = (red[threadIdx.x] + red[16 + threadIdx.x]) + (red[32 + threadIdx.x] + red[48 + threadIdx.x]);
    *reinterpret_cast<f4*>(csout + 4 * threadIdx.x) = t;
    if constexpr (DUAL) *reinterpret_cast<f4*>(csoutB + 4 * threadIdx.x) = t;
  }
}
__global__ __launch_bounds__(256, TSDE_WG6_OCC) void k_wgrad6(WgradJobs jobs, int64_t R, int64_t rows_per_group, int chunk, int chunks_per_group, int P,
                                                   float* __restrict__ part, float* __restrict__ cs) {
  const WgradJob& job = jobs.j[blockIdx.y];
  part += int64_t(blockIdx.y) * P * 4096;
  cs += int64_t(blockIdx.y) * P * 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p = blockIdx.x;
  const int group = p / chunks_per_group, sub = p - group * chunks_per_group;
  const int64_t row0 = group * rows_per_group + int64_t(sub) * chunk;
  int64_t row1 = row0 + chunk;
  if (row1 > (group + 1) * rows_per_group) row1 = (group + 1) * rows_per_group;
  if (row1 > R) row1 = R;
  wgrad6_rows<false>(job, job, row0, row1, part + int64_t(p) * 4096, nullptr, cs + int64_t(p) * 64, nullptr, smem);
}
// The three problems of an edge embedding's weight gradients over its R rows (node_bwd.hip edge_embed_backward) as one launch of two kinds
// of workgroup: the first P0 reduce `chunk0` rows of problem 0 (two stored operands: 512 bytes per row), the next P1 reduce `chunk1` rows
// of problems 1 AND 2 (wgrad6_rows<true>: 272 bytes per row).  Partials: problem 0 in slots [0, P0), 1 in [P0, P0 + P1), 2 behind.
__global__ __launch_bounds__(256, 3) void k_wgrad6_edge(WgradJobs jobs, int64_t R, int chunk0, int P0, int chunk1, int P1,
                                                        float* __restrict__ part, float* __restrict__ cs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int p = blockIdx.x;
  if (p < P0) {
    const int64_t row0 = int64_t(p) * chunk0, row1 = row0 + chunk0 < R ? row0 + chunk0 : R;
    wgrad6_rows<false>(jobs.j[0], jobs.j[0], row0, row1, part + int64_t(p) * 4096, nullptr, cs + int64_t(p) * 64, nullptr, smem);
  } else {
    const int q = p - P0;
    const int64_t row0 = int64_t(q) * chunk1, row1 = row0 + chunk1 < R ? row0 + chunk1 : R;
    wgrad6_rows<true>(jobs.j[1], jobs.j[2], row0, row1, part + int64_t(P0 + q) * 4096, part + int64_t(P0 + P1 + q) * 4096,
                      cs + int64_t(P0 + q) * 64, cs + int64_t(P0 + P1 + q) * 64, smem);
  }
}
static bool wgrad_f32() {          // TRAJSDE_WGRAD_F32=1: the exact fp32 kernel (A/B runs)
  static const bool v = []() { const char* e = getenv("TRAJSDE_WGRAD_F32"); return e && atoi(e) != 0; }();
  return v;
}
#else
static bool wgrad_f32() { return true; }
#endif

// W[o*ldw + col0 + i] = sum_p part[p][o][i];  bias[o] = sum_p cs[p][o];  with time_cols the (sin t, cos t) input
// columns 64 / 65 of the 66-wide first SDE layer: W[o*ldw + 64] = sum_p sin(t_group(p)) cs[p][o], likewise cos.
// A workgroup owns 32 outputs; its 8 thread groups each sum every 8th partial, then combine in a fixed order.
__global__ __launch_bounds__(256) void k_reduce_partials(WgradJobs jobs, const float* __restrict__ part, const float* __restrict__ cs, int P,
                                                         int chunks_per_group, const float* __restrict__ step_tab) {
  const WgradJob& job = jobs.j[blockIdx.y];
  float* __restrict__ W = job.W;
  float* __restrict__ bias = job.bias;
  const int ldw = job.ldw, col0 = job.col0, time_cols = job.time_cols;
  part += int64_t(blockIdx.y) * P * 4096;
  cs += int64_t(blockIdx.y) * P * 64;
  __shared__ float red[3][8][32];
  const int lane = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + lane;
  float s = 0.f, ws = 0.f, wc = 0.f;
  if (j < 4096) {
    int p = sl;                                         // sixteen loads in flight; the additions in the order of the plain loop
    for (; p + 120 < P; p += 128) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = part[int64_t(p + 8 * u) * 4096 + j];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; p + 24 < P; p += 32) {
      const float v0 = part[int64_t(p) * 4096 + j], v1 = part[int64_t(p + 8) * 4096 + j];
      const float v2 = part[int64_t(p + 16) * 4096 + j], v3 = part[int64_t(p + 24) * 4096 + j];
      s += v0;
      s += v1;
      s += v2;
      s += v3;
    }
    for (; p < P; p += 8) s += part[int64_t(p) * 4096 + j];
  } else if (j < 4096 + 64) {
    const int o = j - 4096;
    // (eight partials in flight, consumed in the order of the plain loop: these 64 threads a problem walked P / 8 dependent loads
    //  and were the launch's critical path)
    for (int p0 = sl; p0 < P; p0 += 64) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p0 + 8 * u < P ? cs[int64_t(p0 + 8 * u) * 64 + o] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int p = p0 + 8 * u;
        if (p >= P) break;
        s += v[u];
        if (time_cols) {
          const int k = p / chunks_per_group;
          ws = fmaf(step_tab[k * 8 + 3], v[u], ws);
          wc = fmaf(step_tab[k * 8 + 4], v[u], wc);
        }
      }
    }
  }
  red[0][sl][lane] = s;
  red[1][sl][lane] = ws;
  red[2][sl][lane] = wc;
  __syncthreads();
  if (sl != 0) return;
  float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int g = 0; g < 8; ++g) t[q] += red[q][g][lane];
  if (j < 4096) {
    W[(j >> 6) * ldw + col0 + (j & 63)] = t[0];
  } else if (j < 4096 + 64) {
    const int o = j - 4096;
    if (bias) bias[o] = t[0];
    if (time_cols) {
      W[o * ldw + 64] = t[1];
      W[o * ldw + 65] = t[2];
    }
  }
}

// dst[j*dst_stride] = sum_w src[w*stride + j], j < n   (per-wave vector partials -> one vector), for up to COLSUM_MAX_JOBS
// vectors cut from the same slab of partials in one launch (grid.y = job).  One workgroup per 64 columns, 16 row slices per
// workgroup, fixed summation order.
__global__ __launch_bounds__(1024) void k_colsum(ColsumJobs jobs, int64_t rows, int stride) {
  __shared__ float red[16][64];
  const ColsumJob& job = jobs.j[blockIdx.y];
  const float* __restrict__ src = job.src;
  const int n = job.n;
  if (blockIdx.x * 64 >= n) return;                   // (uniform) a narrower job of the same launch
  const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  float s = 0.f;
  if (j < n) {
    // eight independent partial sums keep several loads in flight (a single workgroup streams the whole slab)
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t w = part;
    for (; w + 112 < rows; w += 128) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += src[(w + 16 * u) * stride + j];
    }
    for (; w < rows; w += 16) a[0] += src[w * stride + j];
    s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
  red[part][c] = s;
  __syncthreads();
  if (part == 0 && j < n) {
    float t = 0.f;
#pragma unroll
    for (int p = 0; p < 16; ++p) t += red[p][c];
    job.dst[int64_t(j) * job.dst_stride] = t;
  }
}


// ------------------------------------------------------------------ deferred sums (wgrad.hpp)
// k_reduce_partials with per-problem partial runs: grid.y = problem, slots [base, base + P) of the shared partial buffer
__global__ __launch_bounds__(256) void k_reduce_partials_q(ReduceJobs jobs, const float* __restrict__ part, const float* __restrict__ cs,
                                                           const float* __restrict__ step_tab) {
  const ReduceJob& job = jobs.j[blockIdx.y];
  float* __restrict__ W = job.W;
  float* __restrict__ bias = job.bias;
  const int ldw = job.ldw, col0 = job.col0, time_cols = job.time_cols, P = job.P, chunks_per_group = job.cpg;
  part += job.base * 4096;
  cs += job.base * 64;
  __shared__ float red[3][8][32];
  const int lane = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + lane;
  float s = 0.f, ws = 0.f, wc = 0.f;
  if (j < 4096) {
    int p = sl;                                         // sixteen loads in flight; the additions in the order of the plain loop
    for (; p + 120 < P; p += 128) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = part[int64_t(p + 8 * u) * 4096 + j];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; p + 24 < P; p += 32) {
      const float v0 = part[int64_t(p) * 4096 + j], v1 = part[int64_t(p + 8) * 4096 + j];
      const float v2 = part[int64_t(p + 16) * 4096 + j], v3 = part[int64_t(p + 24) * 4096 + j];
      s += v0;
      s += v1;
      s += v2;
      s += v3;
    }
    for (; p < P; p += 8) s += part[int64_t(p) * 4096 + j];
  } else if (j < 4096 + 64 && (bias || time_cols)) {
    const int o = j - 4096;
    // (eight partials in flight, consumed in the order of the plain loop: these 64 threads a problem walked P / 8 dependent loads
    //  and were the launch's critical path)
    for (int p0 = sl; p0 < P; p0 += 64) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p0 + 8 * u < P ? cs[int64_t(p0 + 8 * u) * 64 + o] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int p = p0 + 8 * u;
        if (p >= P) break;
        s += v[u];
        if (time_cols) {
          const int k = p / chunks_per_group;
          ws = fmaf(step_tab[k * 8 + 3], v[u], ws);
          wc = fmaf(step_tab[k * 8 + 4], v[u], wc);
        }
      }
    }
  }
  red[0][sl][lane] = s;
  red[1][sl][lane] = ws;
  red[2][sl][lane] = wc;
  __syncthreads();
  if (sl != 0) return;
  float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int g = 0; g < 8; ++g) t[q] += red[q][g][lane];
  if (j < 4096) {
    W[(j >> 6) * ldw + col0 + (j & 63)] = t[0];
  } else if (j < 4096 + 64) {
    const int o = j - 4096;
    if (bias) bias[o] = t[0];
    if (time_cols) {
      W[o * ldw + 64] = t[1];
      W[o * ldw + 65] = t[2];
    }
  }
}
// k_colsum with per-vector slabs (rows, stride): grid.y = vector
__global__ __launch_bounds__(1024) void k_colsum_q(ColsumQJobs jobs) {
  __shared__ float red[16][64];
  const ColsumQJob& job = jobs.j[blockIdx.y];
  const float* __restrict__ src = job.src;
  const int n = job.n, stride = job.stride;
  const int64_t rows = job.rows;
  if (blockIdx.x * 64 >= n) return;                   // (uniform) a narrower vector of the same launch
  const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  float s = 0.f;
  if (j < n) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t w = part;
    for (; w + 112 < rows; w += 128) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += src[(w + 16 * u) * stride + j];
    }
    for (; w < rows; w += 16) a[0] += src[w * stride + j];
    s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
  red[part][c] = s;
  __syncthreads();
  if (part == 0 && j < n) {
    float t = 0.f;
#pragma unroll
    for (int p = 0; p < 16; ++p) t += red[p][c];
    job.dst[int64_t(j) * job.dst_stride] = t;
  }
}

ReduceQueue*& active_reduce_queue() {
  static thread_local ReduceQueue* q = nullptr;
  return q;
}
ColsumQueue*& active_colsum_queue() {
  static thread_local ColsumQueue* q = nullptr;
  return q;
}
int ReduceQueue::drain() {
  for (size_t first = 0; first < jobs.size(); first += REDUCE_MAX_JOBS) {
    ReduceJobs sub;
    sub.n = int(jobs.size() - first < size_t(REDUCE_MAX_JOBS) ? jobs.size() - first : size_t(REDUCE_MAX_JOBS));
    for (int i = 0; i < sub.n; ++i) sub.j[i] = jobs[first + i];
    TS_LAUNCH(k_reduce_partials_q, dim3(cdiv(4096 + 64, 32), sub.n), 256, 0, st, sub, part, cs, step_tab);
  }
  jobs.clear();
  used = 0;
  return TRAJSDE_OK;
}
int64_t ReduceQueue::take(int64_t slots, int* rc) {
  *rc = TRAJSDE_OK;
  if (used + slots > cap) *rc = drain();
  const int64_t base = used;
  used += slots;
  return base;
}
int ColsumQueue::drain() {
  for (size_t first = 0; first < jobs.size(); first += COLSUMQ_MAX_JOBS) {
    ColsumQJobs sub;
    sub.n = int(jobs.size() - first < size_t(COLSUMQ_MAX_JOBS) ? jobs.size() - first : size_t(COLSUMQ_MAX_JOBS));
    int widest = 0;
    for (int i = 0; i < sub.n; ++i) {
      sub.j[i] = jobs[first + i];
      widest = sub.j[i].n > widest ? sub.j[i].n : widest;
    }
    TS_LAUNCH(k_colsum_q, dim3(cdiv(widest, 64), sub.n), 1024, 0, st, sub);
  }
  jobs.clear();
  used = 0;
  return TRAJSDE_OK;
}
float* ColsumQueue::take(int64_t floats) {
  floats = (floats + 63) / 64 * 64;
  if (floats > cap) return nullptr;
  if (used + floats > cap && drain() != TRAJSDE_OK) return nullptr;
  float* p = arena + used;
  used += floats;
  return p;
}
DeferredSums::DeferredSums(hipStream_t st, float* part, float* cs, int64_t cap, const float* step_tab, float* arena, int64_t arena_floats) {
  // TRAJSDE_REDUCE_CAP / TRAJSDE_VPART_ARENA (partial slots / arena floats): smaller areas than the workspace has, so that tests reach
  // the sum-early-when-full paths at sizes where the real areas never fill
  static const int64_t cap_env = []() { const char* e = getenv("TRAJSDE_REDUCE_CAP"); return e ? atoll(e) : 0; }();
  static const int64_t arena_env = []() { const char* e = getenv("TRAJSDE_VPART_ARENA"); return e ? atoll(e) : 0; }();
  if (cap_env > 0 && cap_env < cap) cap = cap_env;
  if (arena_env > 0 && arena_env < arena_floats) arena_floats = arena_env;
  rq.st = st; rq.part = part; rq.cs = cs; rq.step_tab = step_tab; rq.cap = cap; rq.used = 0;
  cq.st = st; cq.arena = arena; cq.cap = arena_floats; cq.used = 0;
  static const bool off = []() { const char* e = getenv("TRAJSDE_IMMEDIATE_SUMS"); return e && e[0] == '1'; }();   // A/B switch
  if (off) return;
  active_reduce_queue() = &rq;
  active_colsum_queue() = arena ? &cq : nullptr;
}
DeferredSums::~DeferredSums() {
  if (active_reduce_queue() == &rq) active_reduce_queue() = nullptr;
  if (active_colsum_queue() == &cq) active_colsum_queue() = nullptr;
}
int DeferredSums::finish() {
  if (int rc = cq.drain()) return rc;
  return rq.drain();
}
float* vpart_slab(float* shared_slab, int64_t rows, int stride) {
  ColsumQueue* q = active_colsum_queue();
  if (!q) return shared_slab;
  float* p = q->take(rows * stride);
  if (p) return p;
  // larger than the arena: sum what is queued (the shared slab may be one of its sources) and fall back to the shared slab, whose
  // own sum then runs immediately (ColsumBatch::flush sees a source outside the arena)
  q->drain();
  return shared_slab;
}

int ColsumBatch::add(const float* src, int n, float* dst, int dst_stride) {
  if (jobs.n == COLSUM_MAX_JOBS)
    if (int rc = flush()) return rc;
  jobs.j[jobs.n++] = ColsumJob{src, dst, n, dst_stride};
  return TRAJSDE_OK;
}
int ColsumBatch::flush() {
  if (jobs.n == 0) return TRAJSDE_OK;
  if (ColsumQueue* q = active_colsum_queue()) {
    bool inside = true;                               // deferred only for slabs that live in the queue's arena
    for (int i = 0; i < jobs.n; ++i) inside = inside && jobs.j[i].src >= q->arena && jobs.j[i].src < q->arena + q->cap;
    if (inside) {
      for (int i = 0; i < jobs.n; ++i) q->jobs.push_back(ColsumQJob{jobs.j[i].src, jobs.j[i].dst, rows, jobs.j[i].n, stride, jobs.j[i].dst_stride});
      jobs.n = 0;
      return TRAJSDE_OK;
    }
  }
  int widest = 0;
  for (int i = 0; i < jobs.n; ++i) widest = jobs.j[i].n > widest ? jobs.j[i].n : widest;
  TS_LAUNCH(k_colsum, dim3(cdiv(widest, 64), jobs.n), 1024, 0, st, jobs, rows, stride);
  jobs.n = 0;
  return TRAJSDE_OK;
}

int WgradBatch::add(const float* delta, int ldd, const float* a, int lda, float* W, int ldw, int col0, float* bias, int time_cols) {
  if (jobs.n == WGRAD_MAX_JOBS)
    if (int rc = flush()) return rc;
  jobs.j[jobs.n++] = WgradJob{delta, a, W, bias, ldd, lda, ldw, col0, time_cols, nullptr, nullptr, 0};
  return TRAJSDE_OK;
}
int WgradBatch::add_in2(const float* delta, int ldd, const float* geom, int pair, const float* in2, const float* beta, float* W, int ldw,
                        float* bias) {
  if (jobs.n == WGRAD_MAX_JOBS)
    if (int rc = flush()) return rc;
  jobs.j[jobs.n++] = WgradJob{delta, geom, W, bias, ldd, 4, ldw, 0, 0, in2, beta, pair};
  return TRAJSDE_OK;
}

#if TSDE_SPLIT_H3 && defined(TSDE_WG6_OCC)
#define TSDE_WG6_OCC_HOST TSDE_WG6_OCC
#else
#define TSDE_WG6_OCC_HOST 3
#endif
static int launch_wgrad(const char* tag, const WgradJobs& sub, int64_t R, int64_t rows_per_group, int chunk, int cpg, int P, float* part, float* cs,
                        hipStream_t st) {
  static const bool trace = getenv("TRAJSDE_WGRAD_TRACE") != nullptr;       // one line per launch: its shape
  if (trace) fprintf(stderr, "wgrad %s: R=%lld jobs=%d P=%d chunk=%d groups=%lld\n", tag, (long long)R, sub.n, P, chunk, (long long)((R + rows_per_group - 1) / rows_per_group));
#if TSDE_SPLIT_H3
  if (!wgrad_f32()) {
    TS_LAUNCH_TAG(tag, false, k_wgrad6, dim3(P, sub.n), 256, 32768 + 64, st, sub, R, rows_per_group, chunk, cpg, P, part, cs);
    return TRAJSDE_OK;
  }
#endif
  TS_LAUNCH_TAG(tag, false, k_wgrad, dim3(P, sub.n), 256, 2 * 4096 * 4, st, sub, R, rows_per_group, chunk, cpg, P, part, cs);
  return TRAJSDE_OK;
}

int WgradBatch::flush() {
  if (jobs.n == 0) return TRAJSDE_OK;
  const int n = jobs.n;
  jobs.n = 0;
  if (R <= 0) {   // nothing to sum: the gradient blocks are zero
    WgradJobs all = jobs;
    all.n = n;
    TS_LAUNCH(k_reduce_partials, dim3(cdiv(4096 + 64, 32), n), 256, 0, c.st, all, c.part, c.cs, 0, 1, c.step_tab);
    return TRAJSDE_OK;
  }
  // rows per workgroup: at least WGRAD_CHUNK; enough partials to fill the chip several times over (a workgroup walks its
  // rows 64 at a time with a barrier in between), few enough (<= ~1024) that the second stage stays short
  const int groups = int((R + rows_per_group - 1) / rows_per_group);
  int64_t chunk = WGRAD_CHUNK;
  static const int parts_env = []() { const char* e = getenv("TRAJSDE_WGRAD_PARTS"); return e ? atoi(e) : 0; }();
  // One resident round of the chip: 3 workgroups of this kernel fit a CU (40 KB of LDS each), and a workgroup streams its
  // rows at the same rate however many it has, so 768 workgroups over the launch's problems leave no partial last round and
  // the fewest partials to reduce (3 problems: 1024 partials each 1.41 ms, 384 1.54 ms, 256 1.35 ms, 128 1.93 ms)
  const int64_t one_round = ((wgrad_f32() ? 768 : 256 * TSDE_WG6_OCC_HOST) + n - 1) / n;
  const int64_t base_parts = parts_env > 0 ? parts_env : (one_round > 32 ? one_round : 32);
  const int64_t want_parts = groups > base_parts ? groups : base_parts;
  if ((rows_per_group + chunk - 1) / chunk * groups > want_parts) {
    // the smallest multiple of 64 rows that stays within the partial budget: P lands just under it (1024 = one full round of
    // the chip's 4 x 256 resident workgroups per problem), not at whatever a doubling of the chunk happens to give
    const int64_t per_group = want_parts / groups > 0 ? want_parts / groups : 1;
    chunk = ((rows_per_group + per_group - 1) / per_group + 63) / 64 * 64;
  } else if (groups == 1) {
    // a short problem (the aggregator's node-level layers: 8 192 rows at 64 x 128): 512-row chunks leave 16 workgroups a problem, each
    // walking 8 blocks one after the other on a mostly idle chip -- shorter chunks, up to one resident round of workgroups
    static const int min_chunk = []() { const char* e = getenv("TRAJSDE_WGRAD_MIN_CHUNK"); const int v = e ? atoi(e) : 128; return v < 64 ? 64 : (v + 63) / 64 * 64; }();
    const int64_t fill = ((R + one_round - 1) / one_round + 63) / 64 * 64;
    const int64_t shorter = fill > min_chunk ? fill : min_chunk;
    if (shorter < chunk) chunk = shorter;
  }
  const int cpg = int((rows_per_group + chunk - 1) / chunk);
  const int P = cpg * groups;
  int per_launch = int(c.cap / P);
  if (per_launch < 1) return fail(TRAJSDE_ERR_WORKSPACE, "wgrad: partial buffer too small");
  ReduceQueue* rq = active_reduce_queue();
  if (rq && rq->part != c.part) rq = nullptr;           // (a context over another partial buffer: immediate)
  if (rq && rq->cap < c.cap) {                          // a queue over a smaller area than the context's
    per_launch = int(rq->cap / P);
    if (per_launch < 1) {                               // one problem's partials do not fit it: this batch is summed immediately,
      if (int rc = rq->drain()) return rc;              // from slot 0 of the same buffer -- after what is queued there
      rq = nullptr;
      per_launch = int(c.cap / P);
    }
  }
  for (int first = 0; first < n; first += per_launch) {
    WgradJobs sub;
    sub.n = n - first < per_launch ? n - first : per_launch;
    for (int i = 0; i < sub.n; ++i) sub.j[i] = jobs.j[first + i];
    if (rq) {                                           // partials stay in their slots; summed at DeferredSums::finish (or when full)
      int rc = TRAJSDE_OK;
      const int64_t base = rq->take(int64_t(sub.n) * P, &rc);
      if (rc) return rc;
      if (int rc2 = launch_wgrad(tag, sub, R, rows_per_group, int(chunk), cpg, P, c.part + base * 4096, c.cs + base * 64, c.st)) return rc2;
      for (int i = 0; i < sub.n; ++i)
        rq->jobs.push_back(ReduceJob{sub.j[i].W, sub.j[i].bias, base + int64_t(i) * P, P, cpg, sub.j[i].ldw, sub.j[i].col0, sub.j[i].time_cols});
      continue;
    }
    if (int rc2 = launch_wgrad(tag, sub, R, rows_per_group, int(chunk), cpg, P, c.part, c.cs, c.st)) return rc2;
    TS_LAUNCH(k_reduce_partials, dim3(cdiv(4096 + 64, 32), sub.n), 256, 0, c.st, sub, c.part, c.cs, P, cpg, c.step_tab);
  }
  return TRAJSDE_OK;
}

// The edge embedding's batch -- problem 0 over two stored operands, problems 1 and 2 over the same delta and geometry records -- through
// k_wgrad6_edge; anything else (the exact fp32 kernel, another shape of batch, TRAJSDE_WGRAD_EDGE_PAIR=0) through flush().
int WgradBatch::flush_edge() {
#if TSDE_SPLIT_H3
  static const bool on = []() { const char* e = getenv("TRAJSDE_WGRAD_EDGE_PAIR"); return !(e && e[0] == '0'); }();
  static const int p0_env = []() { const char* e = getenv("TRAJSDE_WGRAD_EDGE_P0"); return e ? atoi(e) : 0; }();
  static const int p1_env = []() { const char* e = getenv("TRAJSDE_WGRAD_EDGE_P1"); return e ? atoi(e) : 0; }();
  const WgradJob &j0 = jobs.j[0], &j1 = jobs.j[1], &j2 = jobs.j[2];
  const bool shape = jobs.n == 3 && R >= 64 * 64 && rows_per_group >= R && !j0.in2 && j1.in2 && j2.in2 && j1.delta == j2.delta &&
                     j1.ldd == j2.ldd && j1.a == j2.a && !j0.time_cols && !j1.time_cols && !j2.time_cols;
  if (!on || wgrad_f32() || !shape) return flush();
  // One resident round of the chip (3 workgroups a CU): a CU gets one workgroup of the first kind and two of the second.  The pair
  // workgroups are bound by vector arithmetic (two closed-form operands, three splits a block), not by their 272 bytes a row: measured
  // at 64 x 128, 4.55 M rows -- 500 + 268 workgroups 1.30 ms, 384 + 384 0.99, 256 + 512 0.85-0.88, 200 + 568 0.86, 256 + 1024 0.89;
  // the three separate problems (flush) 1.03 ms.
  const int want0 = p0_env > 0 ? p0_env : 256, want1 = p1_env > 0 ? p1_env : 512;
  const int64_t chunk0 = ((R + want0 - 1) / want0 + 63) / 64 * 64, chunk1 = ((R + want1 - 1) / want1 + 63) / 64 * 64;
  const int P0 = int((R + chunk0 - 1) / chunk0), P1 = int((R + chunk1 - 1) / chunk1);
  const int64_t slots = int64_t(P0) + 2 * int64_t(P1);
  ReduceQueue* rq = active_reduce_queue();
  if (rq && (rq->part != c.part || rq->cap < slots)) rq = nullptr;
  if (slots > c.cap) return flush();
  WgradJobs sub = jobs;
  jobs.n = 0;
  int64_t base = 0;
  if (rq) {
    int rc = TRAJSDE_OK;
    base = rq->take(slots, &rc);
    if (rc) return rc;
  } else if (ReduceQueue* other = active_reduce_queue()) {
    if (other->part == c.part)
      if (int rc = other->drain()) return rc;            // summed immediately from slot 0 of the same buffer: after what is queued there
  }
  TS_LAUNCH_TAG(tag, false, k_wgrad6_edge, P0 + P1, 256, 49152 + 128, c.st, sub, R, int(chunk0), P0, int(chunk1), P1, c.part + base * 4096,
                c.cs + base * 64);
  ReduceJobs rj;
  rj.n = 3;
  rj.j[0] = ReduceJob{j0.W, j0.bias, base, P0, P0, j0.ldw, j0.col0, 0};
  rj.j[1] = ReduceJob{sub.j[1].W, sub.j[1].bias, base + P0, P1, P1, sub.j[1].ldw, sub.j[1].col0, 0};
  rj.j[2] = ReduceJob{sub.j[2].W, sub.j[2].bias, base + P0 + P1, P1, P1, sub.j[2].ldw, sub.j[2].col0, 0};
  if (rq) {
    for (int i = 0; i < 3; ++i) rq->jobs.push_back(rj.j[i]);
    return TRAJSDE_OK;
  }
  TS_LAUNCH(k_reduce_partials_q, dim3(cdiv(4096 + 64, 32), 3), 256, 0, c.st, rj, c.part, c.cs, c.step_tab);
  return TRAJSDE_OK;
#else
  return flush();
#endif
}

int run_wgrad(const WgradCtx& c, const float* delta, int ldd, const float* a, int lda, int64_t R, int64_t rows_per_group, float* W,
              int ldw, int col0, float* bias, int time_cols) {
  WgradBatch b(c, R, rows_per_group);
  if (int rc = b.add(delta, ldd, a, lda, W, ldw, col0, bias, time_cols)) return rc;
  return b.flush();
}
// a tall slab (rows >> the 16 row slices of one workgroup): `slices` workgroups per 64 columns each sum a contiguous share of the
// rows into scratch[slice][n], a second launch sums the slices -- fixed order, no atomics
__global__ __launch_bounds__(1024) void k_colsum_slices(const float* __restrict__ src, int64_t rows, int stride, int n, float* __restrict__ scratch) {
  __shared__ float red[16][64];
  const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + c;
  const int64_t per = (rows + gridDim.y - 1) / gridDim.y, lo = blockIdx.y * per, hi = lo + per < rows ? lo + per : rows;
  float s = 0.f;
  if (j < n) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t w = lo + part;
    for (; w + 48 < hi; w += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] += src[(w + 16 * u) * stride + j];
    }
    for (; w < hi; w += 16) a[0] += src[w * stride + j];
    s = (a[0] + a[1]) + (a[2] + a[3]);
  }
  red[part][c] = s;
  __syncthreads();
  if (part == 0 && j < n) {
    float t = 0.f;
#pragma unroll
    for (int p = 0; p < 16; ++p) t += red[p][c];
    scratch[int64_t(blockIdx.y) * n + j] = t;
  }
}
int run_colsum_tall(hipStream_t st, const float* src, int64_t rows, int stride, int n, float* dst, float* scratch /* 256 x n floats */) {
  if (rows < 2048) return run_colsum(st, src, rows, stride, n, dst, 1);      // (a single workgroup streams a short slab fast enough)
  const int slices = 256;
  TS_LAUNCH(k_colsum_slices, dim3(cdiv(n, 64), slices), 1024, 0, st, src, rows, stride, n, scratch);
  return run_colsum(st, scratch, slices, n, n, dst, 1);
}
int run_colsum(hipStream_t st, const float* src, int64_t rows, int stride, int n, float* dst, int dst_stride) {
  ColsumBatch b(st, rows, stride);
  if (int rc = b.add(src, n, dst, dst_stride)) return rc;
  return b.flush();
}

}  // namespace tsde

// pad.hip -- a batch staged into capacity-sized static buffers with inert padding (include/trajsde_hip_capacity.h): the inference
// forward then sees tensors of one shape at fixed addresses whatever batch arrives (runtime.CapacityBuffers).  One launch: the thirteen batch
// tensors, the targets and the three row-id tables are SEGMENTS of one 1-D grid (as the block ranges of k_prep_first, prep.hip); a
// segment gets one workgroup per 1024 destination elements, at most PAD_MAX_WGS, and strides beyond that.  Every destination element
// is written exactly once, from its source element or from the padding rule; nothing is read outside a source tensor.
#include "common.hpp"
#include "../../include/trajsde_hip_capacity.h"

namespace tsde {

constexpr int PAD_THREADS = 256;
constexpr int PAD_PER_WG = 4 * PAD_THREADS;
constexpr int PAD_MAX_WGS = 1024;
enum PadSeg {
  SEG_X, SEG_POS, SEG_ANG, SEG_LANE_POS, SEG_LANE_PAD, SEG_LA_VEC, SEG_Y,        // float: copy, then a constant
  SEG_PADMASK, SEG_BOS,                                                          // bytes: copy, then a constant
  SEG_EDGE, SEG_AGENT, SEG_BATCH, SEG_SOURCE, SEG_LA_INDEX,                      // int64: copy, then the padding rules
  SEG_FAKE_IDS, SEG_ENC_IDS, SEG_DEC_IDS,                                        // int32 row-id tables
  PAD_SEGS
};

struct PadArgs {
  int N, S, E, L, Ea;                 // source sizes
  int Np, Ap, Ep, Lp, Eap;            // destination sizes (capacity + reserve)
  int K;
  int pad_scenes;                     // Ap - S >= 1
  int perm_base, perm_n;              // the permanent pad scene: actors [perm_base, perm_base + perm_n), perm_n >= 2
  float far;                          // both components of a pad lane-actor vector
  int first_wg[PAD_SEGS + 1];         // segment s owns workgroups [first_wg[s], first_wg[s + 1])
  int64_t n_dst[PAD_SEGS];            // destination elements of segment s
  int64_t n_src[PAD_SEGS];            // ... of which the first n_src come from the source (float and byte segments)
  const float* fsrc[SEG_Y + 1];
  float* fdst[SEG_Y + 1];
  const uint8_t *pad_src, *bos_src;
  uint8_t *pad_dst, *bos_dst;
  const int64_t *ei_src, *agent_src, *batch_src, *source_src, *lai_src;
  int64_t *ei_dst, *agent_dst, *batch_dst, *source_dst, *lai_dst;
  int32_t *fake_ids, *enc_ids, *dec_ids;
};

// destination element i of segment `seg`
__device__ __forceinline__ void pad_one(const PadArgs& a, int seg, int64_t i) {
  if (seg <= SEG_Y) {
    const float fill = seg == SEG_LA_VEC ? a.far : 0.f;
    a.fdst[seg][i] = i < a.n_src[seg] ? a.fsrc[seg][i] : fill;
    return;
  }
  switch (seg) {
    case SEG_PADMASK: a.pad_dst[i] = i < a.n_src[seg] ? a.pad_src[i] : uint8_t(1); break;
    case SEG_BOS: a.bos_dst[i] = i < a.n_src[seg] ? a.bos_src[i] : uint8_t(0); break;
    case SEG_EDGE: {                                        // [2, Ep]: row 0 senders, row 1 targets
      const int r = i >= a.Ep, e = int(i - int64_t(r) * a.Ep);
      if (e < a.E) {
        a.ei_dst[i] = a.ei_src[int64_t(r) * a.E + e];
      } else {                                              // target d, sender another actor of the permanent pad scene
        const int j = e - a.E, d = j % a.perm_n, s = (d + 1 + (j / a.perm_n) % (a.perm_n - 1)) % a.perm_n;
        a.ei_dst[i] = a.perm_base + (r ? d : s);
      }
      break;
    }
    case SEG_AGENT: a.agent_dst[i] = i < a.S ? a.agent_src[i] : int64_t(a.N) + (i - a.S); break;
    case SEG_BATCH: {
      const int64_t p = i - a.N;
      a.batch_dst[i] = i < a.N ? a.batch_src[i] : int64_t(a.S) + (p < a.pad_scenes - 1 ? p : a.pad_scenes - 1);
      break;
    }
    case SEG_SOURCE: a.source_dst[i] = i < a.S ? a.source_src[i] : int64_t(0); break;
    case SEG_LA_INDEX: {                                    // [2, Eap]: row 0 lanes, row 1 actors
      const int r = i >= a.Eap, e = int(i - int64_t(r) * a.Eap);
      if (e < a.Ea) a.lai_dst[i] = a.lai_src[int64_t(r) * a.Ea + e];
      else a.lai_dst[i] = r ? int64_t(a.perm_base + (e - a.Ea) % a.perm_n) : int64_t(a.Lp - 1);
      break;
    }
    case SEG_FAKE_IDS: a.fake_ids[i] = int32_t(i); break;
    case SEG_ENC_IDS: {
      int32_t v;
      if (i < a.N) v = int32_t(i);                          // a real actor keeps its row
      else if (i < a.Np) v = int32_t(i) + a.S;              // pad actors: past the N + S rows of the unpadded batch
      else if (i - a.Np < a.S) v = a.N + int32_t(i - a.Np); // the fake row of real agent a: N + a
      else v = int32_t(i);                                  // pad fake rows: >= Np + S, past the pad actors
      a.enc_ids[i] = v;
      break;
    }
    default: {                                              // SEG_DEC_IDS: [K, Np]
      const int k = int(i / a.Np), n = int(i - int64_t(k) * a.Np);
      a.dec_ids[i] = n < a.N ? k * a.N + n : a.K * a.N + k * (a.Np - a.N) + (n - a.N);
      break;
    }
  }
}

__global__ __launch_bounds__(PAD_THREADS) void k_batch_pad(const PadArgs a) {
  const int wg = blockIdx.x;
  int seg = 0;
  while (seg + 1 < PAD_SEGS && wg >= a.first_wg[seg + 1]) ++seg;      // (uniform: a handful of scalar compares)
  const int64_t n = a.n_dst[seg];
  const int64_t stride = int64_t(a.first_wg[seg + 1] - a.first_wg[seg]) * PAD_PER_WG;
  for (int64_t base = int64_t(wg - a.first_wg[seg]) * PAD_PER_WG; base < n; base += stride) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = base + u * PAD_THREADS + int(threadIdx.x);
      if (i < n) pad_one(a, seg, i);
    }
  }
}

static int pad_fits(const trajsde_batch* src, const trajsde_batch* dst) {
  TS_REQUIRE(src != nullptr && dst != nullptr, "batch_pad: null batch");
  TS_REQUIRE(src->N > 0 && src->A > 0 && src->E >= 0 && src->L >= 0 && src->E_al >= 0, "batch_pad: the source needs N > 0, A > 0 and no negative size");
  TS_REQUIRE(dst->N >= 3 && dst->A >= 2 && dst->E >= 0 && dst->L >= 1 && dst->E_al >= 0,
             "batch_pad: the destination holds the reserve (N >= 3, A >= 2, L >= 1) and no negative size");
  TS_REQUIRE(src->H > 0 && src->H <= 32 && src->TT >= src->H && src->lane_pts >= 0, "batch_pad: bad source sizes (0 < H <= 32, TT >= H)");
  if (src->H != dst->H) return fail(TRAJSDE_ERR_INVALID, "batch_pad: H (history steps) is " + std::to_string(src->H) + ", the static buffers have " + std::to_string(dst->H));
  if (src->TT != dst->TT) return fail(TRAJSDE_ERR_INVALID, "batch_pad: TT (time slots) is " + std::to_string(src->TT) + ", the static buffers have " + std::to_string(dst->TT));
  if (src->lane_pts != dst->lane_pts)
    return fail(TRAJSDE_ERR_INVALID, "batch_pad: lane_pts is " + std::to_string(src->lane_pts) + ", the static buffers have " + std::to_string(dst->lane_pts));
  const int scenes = dst->A - 1, actors = dst->N - 2, lanes = dst->L - 1;
  if (src->A > scenes) return fail(TRAJSDE_ERR_INVALID, "batch_pad: scenes: " + std::to_string(src->A) + " exceed the capacity of " + std::to_string(scenes));
  if (int64_t(src->N) + (scenes - src->A) > actors)
    return fail(TRAJSDE_ERR_INVALID, "batch_pad: actors: " + std::to_string(src->N) + " plus one for each of the " + std::to_string(scenes - src->A) +
                                         " pad scenes exceed the capacity of " + std::to_string(actors));
  if (src->E > dst->E) return fail(TRAJSDE_ERR_INVALID, "batch_pad: edges: " + std::to_string(src->E) + " exceed the capacity of " + std::to_string(dst->E));
  if (src->L > lanes) return fail(TRAJSDE_ERR_INVALID, "batch_pad: lanes: " + std::to_string(src->L) + " exceed the capacity of " + std::to_string(lanes));
  if (src->E_al > dst->E_al)
    return fail(TRAJSDE_ERR_INVALID, "batch_pad: lane_edges: " + std::to_string(src->E_al) + " exceed the capacity of " + std::to_string(dst->E_al));
  return TRAJSDE_OK;
}

}  // namespace tsde

using namespace tsde;

extern "C" {

int32_t trajsde_batch_pad_fits(const trajsde_batch* src, const trajsde_batch* dst) { return pad_fits(src, dst); }

int32_t trajsde_batch_pad(const trajsde_batch* src, const float* y, int32_t F, const trajsde_batch* dst, float* dst_y, int num_modes,
                          float local_radius, int32_t* fake_row_ids, int32_t* enc_row_ids, int32_t* dec_row_ids, void* stream) {
  if (const int rc = pad_fits(src, dst)) return rc;
  TS_REQUIRE(num_modes >= 1 && F >= 0, "batch_pad: need num_modes >= 1 and F >= 0");
  TS_REQUIRE(int64_t(num_modes) * dst->N < (int64_t(1) << 31), "batch_pad: num_modes * N exceeds int32 row ids");
  TS_REQUIRE(fake_row_ids && enc_row_ids && dec_row_ids, "batch_pad: null row-id table");
  TS_REQUIRE((y == nullptr && dst_y == nullptr) || F > 0, "batch_pad: targets need F > 0");
  TS_REQUIRE(src->x && src->positions && src->padding_mask && src->bos_mask && src->rotate_angles && src->batch && src->source && src->agent_index,
             "batch_pad: null actor tensor in the source");
  TS_REQUIRE(src->E == 0 || src->edge_index, "batch_pad: null edge_index in the source");
  TS_REQUIRE(src->L == 0 || src->lane_pts == 0 || (src->lane_positions && src->lane_paddings), "batch_pad: null lane tensor in the source");
  TS_REQUIRE(src->E_al == 0 || (src->lane_actor_index && src->lane_actor_vectors), "batch_pad: null lane-actor tensor in the source");
  TS_REQUIRE(dst->x && dst->positions && dst->padding_mask && dst->bos_mask && dst->rotate_angles && dst->batch && dst->source && dst->agent_index,
             "batch_pad: null actor tensor in the destination");
  TS_REQUIRE(dst->E == 0 || dst->edge_index, "batch_pad: null edge_index in the destination");
  TS_REQUIRE(dst->lane_pts == 0 || (dst->lane_positions && dst->lane_paddings), "batch_pad: null lane tensor in the destination");
  TS_REQUIRE(dst->E_al == 0 || (dst->lane_actor_index && dst->lane_actor_vectors), "batch_pad: null lane-actor tensor in the destination");

  PadArgs a;
  a.N = src->N; a.S = src->A; a.E = src->E; a.L = src->L; a.Ea = src->E_al;
  a.Np = dst->N; a.Ap = dst->A; a.Ep = dst->E; a.Lp = dst->L; a.Eap = dst->E_al;
  a.K = num_modes;
  a.pad_scenes = a.Ap - a.S;
  a.perm_base = a.N + a.pad_scenes - 1;
  a.perm_n = a.Np - a.perm_base;                        // >= 2 by the actors rule of pad_fits
  a.far = local_radius > 0.f ? 200.f * local_radius : 0.f;   // (a radius <= 0 keeps no lane-actor edge at all)
  const int64_t H = src->H, TT = src->TT, P = src->lane_pts;
  auto fseg = [&](int s, const float* from, float* to, int64_t rows_src, int64_t rows_dst, int64_t row) {
    a.fsrc[s] = from; a.fdst[s] = to;
    a.n_src[s] = from ? rows_src * row : 0;
    a.n_dst[s] = to ? rows_dst * row : 0;
  };
  fseg(SEG_X, src->x, const_cast<float*>(dst->x), a.N, a.Np, H * 2);
  fseg(SEG_POS, src->positions, const_cast<float*>(dst->positions), a.N, a.Np, TT * 2);
  fseg(SEG_ANG, src->rotate_angles, const_cast<float*>(dst->rotate_angles), a.N, a.Np, 1);
  fseg(SEG_LANE_POS, src->lane_positions, const_cast<float*>(dst->lane_positions), a.L, a.Lp, P * 2);
  fseg(SEG_LANE_PAD, src->lane_paddings, const_cast<float*>(dst->lane_paddings), a.L, a.Lp, P);
  fseg(SEG_LA_VEC, src->lane_actor_vectors, const_cast<float*>(dst->lane_actor_vectors), a.Ea, a.Eap, 2);
  fseg(SEG_Y, y, dst_y, a.N, a.Np, int64_t(F) * 2);
  a.pad_src = src->padding_mask; a.pad_dst = const_cast<uint8_t*>(dst->padding_mask);
  a.n_src[SEG_PADMASK] = a.N * TT; a.n_dst[SEG_PADMASK] = a.Np * TT;
  a.bos_src = src->bos_mask; a.bos_dst = const_cast<uint8_t*>(dst->bos_mask);
  a.n_src[SEG_BOS] = a.N * H; a.n_dst[SEG_BOS] = a.Np * H;
  a.ei_src = src->edge_index; a.ei_dst = const_cast<int64_t*>(dst->edge_index);
  a.agent_src = src->agent_index; a.agent_dst = const_cast<int64_t*>(dst->agent_index);
  a.batch_src = src->batch; a.batch_dst = const_cast<int64_t*>(dst->batch);
  a.source_src = src->source; a.source_dst = const_cast<int64_t*>(dst->source);
  a.lai_src = src->lane_actor_index; a.lai_dst = const_cast<int64_t*>(dst->lane_actor_index);
  a.fake_ids = fake_row_ids; a.enc_ids = enc_row_ids; a.dec_ids = dec_row_ids;
  const int64_t counts[] = {2 * int64_t(a.Ep), a.Ap, a.Np, a.Ap, 2 * int64_t(a.Eap), a.Ap, int64_t(a.Np) + a.Ap, int64_t(a.K) * a.Np};
  for (int s = SEG_EDGE; s < PAD_SEGS; ++s) { a.n_dst[s] = counts[s - SEG_EDGE]; a.n_src[s] = 0; }
  int total = 0;
  for (int s = 0; s < PAD_SEGS; ++s) {
    a.first_wg[s] = total;
    const int64_t wgs = (a.n_dst[s] + PAD_PER_WG - 1) / PAD_PER_WG;
    total += int(wgs > PAD_MAX_WGS ? PAD_MAX_WGS : wgs);
  }
  a.first_wg[PAD_SEGS] = total;
  TS_LAUNCH(k_batch_pad, dim3(unsigned(total)), PAD_THREADS, 0, static_cast<hipStream_t>(stream), a);
  return TRAJSDE_OK;
}

}  // extern "C"

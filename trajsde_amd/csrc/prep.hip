// prep.hip -- everything the reference does with index tensors before the attention blocks, on device:
//   MODEL:75-85   rotate_mat, y @ rotate_mat
//   ENC:68-71     lane feature = last valid lane point - first lane point
//   ENC:73-74,103 nus_mask;  ENC:88-103 fake copies of the target agents (x + 2*randn, duplicated in-edges)
//   ENC:107-118   21 x subgraph(valid at t) + DistanceDropEdge(radius) (UTIL:83-92)
//   AGG:41-51     subgraph(valid at t=H-1), relative pose;   ENC:198 radius drop on lane-actor edges
// Instead of materialising 21 boolean-masked edge lists, edges are sorted once by target (counting sort
// -> CSR), every (t, edge) candidate gets a 1-byte flag, one prefix sum gives the compacted position
// of every survivor, and the segment pointer of snapshot node (t, i) is read off the same prefix sum.
// The compacted lists carry the pre-rotated 2-d geometry the edge kernels consume (16 B per edge).

#include <algorithm>
#include <cmath>
#include <limits>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "common.hpp"
#include "philox.hpp"
#include "tile.hpp"

namespace tsde {

// one thread per (actor, future step) -- a thread per actor walked its F steps one dependent load at a time: 16 us a forward
__global__ void k_rotate(const float* __restrict__ ang, int N, const float* __restrict__ y, int F,
                         float* __restrict__ rot, float* __restrict__ y_rot) {
  const int per = F > 0 && y != nullptr ? F : 1;
  const int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= int64_t(N) * per) return;
  const int i = int(idx / per), t = int(idx - int64_t(i) * per);
  const float s = sinf(ang[i]), c = cosf(ang[i]);
  if (t == 0) {
    f4 r = {c, -s, s, c};
    *reinterpret_cast<f4*>(rot + 4 * i) = r;
  }
  if (y != nullptr && F > 0) {
    const float a = y[(int64_t(i) * F + t) * 2], b = y[(int64_t(i) * F + t) * 2 + 1];
    y_rot[(int64_t(i) * F + t) * 2] = a * c + b * s;        // [a b] @ [[c,-s],[s,c]]
    y_rot[(int64_t(i) * F + t) * 2 + 1] = b * c - a * s;
  }
}

// ---------------------------------------------------------------------------------------------- the graph stage in six launches
// (round 5; rounds 1-4 issued 22 launches of a few microseconds each: 0.36 ms of a 2.55 ms one-stream forward.)
//   memset        degree counters, tickets and look-back words
//   k_prep_first  block ranges: target-degree histograms of the actor and the lane-actor edge lists (integer atomics), extended-node
//                 table, fake agents' inputs, validity masks + TIME-MAJOR copies of positions / inputs, lane features; the workgroup
//                 that finishes LAST turns both histograms into row pointers and fills the agents' slots
//   k_scatter2    counting-sort scatter of both lists
//   k_row_sort2   canonical (ascending) order of every CSR row of both lists; the keep-flags of the global-interactor edges (AGG:41)
//                 and of the lane-actor edges (ENC:198) are written as the sorted rows are stored
//   k_aa_count    the survivor counts of every snapshot node (t, i)
//   k_scan_multi  the prefix sums over the counts and the two flag arrays as ONE launch of chained scans; the workgroup that finishes
//                 last derives the segment pointers of the global / lane lists and the list lengths
//   k_graph_fill  trajsde_graph_compact: block ranges -- the agent-agent snapshot records, the global list, the lane list
// Every result is bit for bit what the 22-launch form produced (integer work; the geometry expressions are the same).
//
// The actor CSR without the sort.  The datasets emit the actor edge list per scene as permutations(range(n), 2) and
// collation concatenates the scenes with node offsets: source-major and complete per scene ("dataset order").  A complete graph is its
// own transpose, so row t of the target-major CSR is "every other node of t's scene, ascending" and the row pointers follow from the
// scene extents alone -- no histogram, no scatter, no row sort.  The stage ASSUMES that order and CHECKS it on the device:
//   k_prep_first  instead of the actor histogram: in-degree of node i = (size of i's scene) - 1 from a binary search in `batch`, the
//                 scene's first node (scene_lo), and the check that `batch` is non-decreasing
//   k_direct2     instead of the actor half of k_scatter2: every position p of the INPUT list is compared with the closed form (its source s
//                 is the row with rowptr[s] <= p < rowptr[s+1], its target lo + k + (lo + k >= s), k = p - rowptr[s]); the row pointers
//                 must ascend to E; csr_src / csr_dst / flags_g are written in the same pass -- optimistically
//   k_aa_count, k_graph_fill   on this path a row's candidate idx is node lo + idx + (lo + idx >= o): no csr_src gather at the head of
//                 their dependent chains
//   any mismatch raises ONE word of the zeroed block (PrepWs::general, non-returning atomic).  The general path follows as launches that
//   return at their first instruction while the word is zero: k_fb_degree (histogram + row pointers), k_fb_scatter, and the actor
//   blocks of k_row_sort2 -- they write over everything the optimistic pass left.  Nothing waits for the word inside a launch: it is
//   raised by whole earlier launches and read by later ones of the same stream.
// A list that is not in dataset order pays for the attempt: the general path as three launches of its own plus the first two -- measured
// in profiles/r07_ab_runs.md.  TRAJSDE_GRAPH_DIRECT=0 (or E == 0) takes the general path on the host: exactly the six launches above,
// for callers whose lists are never in dataset order.

// "the workgroup that finishes last continues": every workgroup waits until its own writes have been performed, takes a number, and
// the one that draws the last number reads what the others left.  NO device-wide fence: on this chip an agent-scope release is a
// write-back of the XCD's whole L2 (measured: 0.96 ms for the 10 K workgroups of the first launch).  Instead, everything a tail reads
// from other workgroups of its launch is written with agent-scope atomics / write-through stores (store_through) and read with
// agent-scope loads (coherent_load): those are performed at the device's point of coherence; `s_waitcnt vmcnt(0)` is what tells a wave
// that its own have been (it is the wait an agent-scope release ends with; a WORKGROUP-scope release fence compiles to no wait at
// all for global memory in this execution mode, and with it a tail read degree counters that were still on their way).
// (the numbers are drawn from 16 counters, the 16 draws that complete a counter from a 17th: 1 500 returning atomics on ONE address
//  are served one after the other)
constexpr int DONE_WAYS = 16;
__device__ __forceinline__ bool last_block_done(unsigned int* counters /* DONE_WAYS + 1, zeroed */, unsigned int total) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned way = blockIdx.x % DONE_WAYS;
    const unsigned quota = total / DONE_WAYS + (way < total % DONE_WAYS ? 1u : 0u);        // blocks b with b % DONE_WAYS == way
    int last = 0;
    if (__hip_atomic_fetch_add(&counters[way], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == quota) {
      unsigned ways_used = total < unsigned(DONE_WAYS) ? total : unsigned(DONE_WAYS);
      last = __hip_atomic_fetch_add(&counters[DONE_WAYS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == ways_used;
    }
    s_last = last;
  }
  __syncthreads();
  return s_last != 0;
}
// agent-scope (sc1) loads as ordinary buffer loads -- the compiler schedules them and counts their waits, several stay in flight; an
// atomic load per element serialised the tails (0.15 ms for the 8 K-entry row pointers)
struct CoherentI32 {
  __amdgpu_buffer_rsrc_t rs;
  __device__ __forceinline__ explicit CoherentI32(const int32_t* base)
      : rs(__builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(base), 0, 0xFFFFFFFF, 0x00020000)) {}
  __device__ __forceinline__ int32_t operator[](int i) const { return __builtin_amdgcn_raw_buffer_load_b32(rs, i * 4, 0, 16 /* sc1 */); }
};
__device__ __forceinline__ void store_through(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// counting sort on the target id (deterministic counts via integer atomics), then every row is put into canonical
// order (ascending source / edge id) by a register / in-LDS bitonic sort, so the result does not depend on atomic arrival
// order -- nor on the order of the input edge list.
constexpr int EPT = 16;     // edges per thread of the histogram / scatter passes: their index loads and atomics in flight together
__device__ __forceinline__ void degree_body(int blk, const int64_t* __restrict__ ei, int E, int32_t* __restrict__ deg) {
  int d[EPT];
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int e = (blk * EPT + u) * 256 + int(threadIdx.x);
    d[u] = e < E ? int(ei[int64_t(E) + e]) : -1;                           // row 1 = target
  }
#pragma unroll
  for (int u = 0; u < EPT; ++u)
    if (d[u] >= 0) atomicAdd(&deg[d[u]], 1);
}
// a row's slots are handed out by counting its degree back down (any order: the rows are sorted afterwards), so no copy of the
// row pointers is needed as a cursor
__device__ __forceinline__ void scatter_body(int blk, const int64_t* __restrict__ ei, int E, const int32_t* __restrict__ rowptr,
                                             int32_t* __restrict__ deg, int32_t* __restrict__ out) {
  int d[EPT], p[EPT], src[EPT];
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int e = (blk * EPT + u) * 256 + int(threadIdx.x);
    d[u] = e < E ? int(ei[int64_t(E) + e]) : -1;
    src[u] = e < E ? int32_t(ei[e]) : 0;                                   // row 0 = source
  }
#pragma unroll
  for (int u = 0; u < EPT; ++u) p[u] = d[u] >= 0 ? rowptr[d[u]] + atomicSub(&deg[d[u]], 1) - 1 : -1;
#pragma unroll
  for (int u = 0; u < EPT; ++u)
    if (p[u] >= 0) out[p[u]] = src[u];
}
// lane-actor edges: value = (lane id << 32) | edge id, so that rows sort by lane first (canonical under permutations
// of the input list) and the edge id is still at hand for the vector lookup
__device__ __forceinline__ void scatter_lane_body(int blk, const int64_t* __restrict__ lai, int E, const int32_t* __restrict__ rowptr,
                                                  int32_t* __restrict__ deg, int64_t* __restrict__ out) {
  int d[EPT], p[EPT];
  int64_t key[EPT];
#pragma unroll
  for (int u = 0; u < EPT; ++u) {
    const int e = (blk * EPT + u) * 256 + int(threadIdx.x);
    d[u] = e < E ? int(lai[int64_t(E) + e]) : -1;
    key[u] = e < E ? ((lai[e] << 32) | int64_t(e)) : 0;
  }
#pragma unroll
  for (int u = 0; u < EPT; ++u) p[u] = d[u] >= 0 ? rowptr[d[u]] + atomicSub(&deg[d[u]], 1) - 1 : -1;
#pragma unroll
  for (int u = 0; u < EPT; ++u)
    if (p[u] >= 0) out[p[u]] = key[u];
}
__global__ __launch_bounds__(256) void k_scatter2(const int64_t* __restrict__ ei, int E, const int32_t* __restrict__ rowptr, int32_t* __restrict__ deg,
                                                  int32_t* __restrict__ csr_src, int nb_a, const int64_t* __restrict__ lai, int Ea,
                                                  const int32_t* __restrict__ la_rowptr, int32_t* __restrict__ la_deg, int64_t* __restrict__ la_pack) {
  const int blk = blockIdx.x;
  if (blk < nb_a) scatter_body(blk, ei, E, rowptr, deg, csr_src);
  else scatter_lane_body(blk - nb_a, lai, Ea, la_rowptr, la_deg, la_pack);
}
// ascending sort of the long CSR rows (more than 256 entries; second phase of k_row_sort), one workgroup per row (grid-stride).
// Rows of up to 4096 entries: bitonic network in LDS on the row padded to a power of two with +inf.  Longer rows: in place in global memory with the "flip" form of the network
// (first sub-step of stage k pairs i with i ^ (k - 1), the others i with i ^ j), in which EVERY compare-exchange puts the
// minimum at the lower index -- so the virtual +inf padding above the row's end never moves and a pair whose upper index lies
// beyond the row is a no-op: correct for any row length without materialising the padding.
// `emit(position, sorted value, row)`: called once for every position as its final value is stored (the keep-flags of the two lists)
template <typename T, typename EMIT>
__device__ __forceinline__ void sort_long_rows(int vblk, int vgrid, const int32_t* __restrict__ rowptr, int n_rows, T* __restrict__ vals,
                                               T* buf /* LDS, 4096 */, int32_t* __restrict__ low_out, int32_t* __restrict__ row_out,
                                               const EMIT& emit) {
  const T INF = sizeof(T) == 8 ? T(INT64_MAX) : T(INT32_MAX);
  for (int row = vblk; row < n_rows; row += vgrid) {
    const int beg = rowptr[row], n = rowptr[row + 1] - beg;
    if (n <= 256) continue;                                 // (sorted by a wave in the first phase)
    if (row_out != nullptr)
      for (int i = threadIdx.x; i < n; i += blockDim.x) row_out[beg + i] = row;
    int P = 2;
    while (P < n) P <<= 1;
    if (P <= 4096) {
      for (int i = threadIdx.x; i < P; i += blockDim.x) buf[i] = i < n ? vals[beg + i] : INF;
      __syncthreads();
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = threadIdx.x; i < P; i += blockDim.x) {
            const int l = i ^ j;
            if (l > i) {
              const T vi = buf[i], vl = buf[l];
              const bool up = (i & k) == 0;
              if ((vi > vl) == up) {
                buf[i] = vl;
                buf[l] = vi;
              }
            }
          }
          __syncthreads();
        }
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        vals[beg + i] = buf[i];
        if (low_out != nullptr) low_out[beg + i] = int32_t(int64_t(buf[i]) & 0xFFFFFFFFll);
        emit(beg + i, buf[i], row);
      }
      __syncthreads();
    } else {
      T* a = vals + beg;
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          const int mask = (j == (k >> 1)) ? k - 1 : j;      // flip on the first sub-step of a stage
          for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int l = i ^ mask;
            if (l > i && l < n) {
              const T vi = a[i], vl = a[l];
              if (vi > vl) {
                a[i] = vl;
                a[l] = vi;
              }
            }
          }
          __threadfence_block();
          __syncthreads();
        }
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (low_out != nullptr) low_out[beg + i] = int32_t(int64_t(a[i]) & 0xFFFFFFFFll);
        emit(beg + i, a[i], row);
      }
    }
  }
}

// Ascending sort of every CSR row (canonical order: the result does not depend on the atomics' arrival order nor on the order of
// the input list).  Rows of up to 256 entries -- every row of the usual batches -- are sorted by ONE WAVE in registers: element
// i = 4 lane + r, so the compare-exchanges at distance 1 and 2 are register swaps and the others one cross-lane exchange per
// register; no LDS image, no workgroup barrier per sub-step (the workgroup form spends 36 barriers on a 256-entry row: 47 us
// for the 8 192 rows of the metric workload against 12 us here).  Longer rows: second phase, sort_long_rows.
template <typename T>
__device__ __forceinline__ T lane_xor(T v, int mask) {
  if constexpr (sizeof(T) == 8) {
    const unsigned lo = unsigned(__shfl_xor(int(unsigned(v & 0xFFFFFFFFll)), mask)), hi = unsigned(__shfl_xor(int(unsigned((v >> 32) & 0xFFFFFFFFll)), mask));
    return T((int64_t(hi) << 32) | int64_t(lo));
  } else {
    return T(__shfl_xor(int(v), mask));
  }
}
template <typename T, typename EMIT>
__device__ __forceinline__ void row_sort_part(int vblk, int vgrid, const int32_t* __restrict__ rowptr, int n_rows, T* __restrict__ vals,
                                              int32_t* __restrict__ low_out /* or null: the low words of the sorted values (edge ids of packed lane keys) */,
                                              int32_t* __restrict__ row_out /* or null: the row of every position (its target) */,
                                              T* buf /* LDS, 4096 */, const EMIT& emit) {
  constexpr int EPL = 4, PMAX = 64 * EPL;
  const T INF = sizeof(T) == 8 ? T(INT64_MAX) : T(INT32_MAX);
  const int lane = threadIdx.x & 63, waves = blockDim.x >> 6;
  for (int row = vblk * waves + (threadIdx.x >> 6); row < n_rows; row += vgrid * waves) {
    const int beg = rowptr[row], n = rowptr[row + 1] - beg;
    if (n > PMAX) continue;
    if (row_out != nullptr) {
#pragma unroll
      for (int r = 0; r < EPL; ++r)
        if (64 * r + lane < n) row_out[beg + 64 * r + lane] = row;
    }
    if (n <= 1) {
      if (n == 1 && lane == 0) {
        const T v0 = vals[beg];
        if (low_out != nullptr) low_out[beg] = int32_t(int64_t(v0) & 0xFFFFFFFFll);
        emit(beg, v0, row);
      }
      continue;
    }
    T v[EPL];
#pragma unroll
    for (int r = 0; r < EPL; ++r) v[r] = EPL * lane + r < n ? vals[beg + EPL * lane + r] : INF;
#pragma unroll
    for (int k = 2; k <= PMAX; k <<= 1) {
      if ((k >> 1) >= n) break;                             // the row's power of two is done: the padding above it never moves
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        if (j < EPL) {                                      // partner in this lane
#pragma unroll
          for (int r = 0; r < EPL; ++r) {
            const int l = r ^ j;
            if (l > r) {
              const bool up = ((EPL * lane + r) & k) == 0;
              const T a = v[r], b = v[l];
              const bool sw = (a > b) == up;
              v[r] = sw ? b : a;
              v[l] = sw ? a : b;
            }
          }
        } else {                                            // partner in lane ^ (j / EPL), same register
          const int lj = j / EPL;
          const bool lower = (lane & lj) == 0;
#pragma unroll
          for (int r = 0; r < EPL; ++r) {
            const T o = lane_xor<T>(v[r], lj);
            const bool up = ((EPL * lane + r) & k) == 0;
            const bool keep_min = lower == up;
            v[r] = keep_min ? (o < v[r] ? o : v[r]) : (o > v[r] ? o : v[r]);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < EPL; ++r)
      if (EPL * lane + r < n) {
        vals[beg + EPL * lane + r] = v[r];
        if (low_out != nullptr) low_out[beg + EPL * lane + r] = int32_t(int64_t(v[r]) & 0xFFFFFFFFll);
        emit(beg + EPL * lane + r, v[r], row);
      }
  }
  sort_long_rows<T>(vblk, vgrid, rowptr, n_rows, vals, buf, low_out, row_out, emit);    // rows of more than 256 entries, a workgroup per row
}

// per extended node: original actor, source mask, recurrence iteration to keep; slots of the agent rows.  pick_slot of a real actor is
// the index k of the agent entry that names it (-1: none; the LAST such k should agent_index repeat an actor), found by a scan over
// agent_index staged through LDS -- no second pass that overrides the table, so no ordering between workgroups is needed
__device__ __forceinline__ void ext_nodes_body(int i, int N, int A, int H, const int64_t* __restrict__ agent_index,
                                               const int64_t* __restrict__ batch, const int64_t* __restrict__ source,
                                               const uint8_t* __restrict__ bos, int32_t* __restrict__ orig, uint8_t* __restrict__ nus,
                                               int32_t* __restrict__ eos, int32_t* __restrict__ pick_slot) {
  __shared__ int32_t s_agents[256];
  int slot = -1;
  for (int k0 = 0; k0 < A; k0 += 256) {                               // (uniform loop: every thread of the workgroup takes part)
    __syncthreads();
    s_agents[threadIdx.x] = k0 + int(threadIdx.x) < A ? int32_t(agent_index[k0 + threadIdx.x]) : -1;
    __syncthreads();
    const int m = A - k0 < 256 ? A - k0 : 256;
    if (i < N)
      for (int k = 0; k < m; ++k)
        if (s_agents[k] == i) slot = k0 + k;
  }
  if (i >= N + A) return;
  const int o = i < N ? i : int(agent_index[i - N]);
  orig[i] = o;
  nus[i] = (i < N ? source[batch[i]] : source[i - N]) == 0;        // ENC:73-74, 103
  int first = 0;                                                     // torch.argmax of an all-false row is 0
  {
    uint8_t bv[32];                                                  // all H <= 32 bytes requested before the first is looked at
#pragma unroll
    for (int t = 0; t < 32; ++t) bv[t] = bos[int64_t(o) * H + (t < H ? t : H - 1)];
#pragma unroll
    for (int t = 31; t >= 0; --t)
      if (t < H && bv[t]) first = t;
  }
  eos[i] = (H - 1) - first;                                          // ENC:187 (ref_time = H-1)
  pick_slot[i] = i < N ? slot : A + (i - N);
}

// x_fake[k,t,:] = x[agent_k,t,:] + 2*z   (ENC:94-95)
__device__ __forceinline__ void fake_x_body(int idx /* one thread per (k, quad of 4 columns) */, int A, int H, const float* __restrict__ x,
                                            const int64_t* __restrict__ agent_index, const NoiseArg& na, float* __restrict__ x_fake) {
  const int quads = (2 * H + 3) / 4;
  if (idx >= A * quads) return;
  const int k = idx / quads, q = idx % quads;
  f4 z;
  if (na.z != nullptr) {
    for (int c = 0; c < 4; ++c) z[c] = (4 * q + c < 2 * H) ? na.z[int64_t(k) * 2 * H + 4 * q + c] : 0.f;
  } else {
    z = philox_normal4(noise_key(na), STREAM_FAKE_AGENT, 0u, na.row_ids ? uint32_t(na.row_ids[k]) : uint32_t(k), uint32_t(q));
  }
  const int64_t a = agent_index[k];
  for (int c = 0; c < 4; ++c) {
    const int col = 4 * q + c;
    if (col < 2 * H) x_fake[int64_t(k) * 2 * H + col] = x[a * 2 * H + col] + 2.0f * z[c];
  }
}

// ---------------------------------------------------------------------------------------------- 21 snapshots
// The agent-agent list of snapshot t keeps the in-edge (j -> i) when both ends are valid at t (ENC:108) and closer than the
// radius (UTIL:88).  The list is ordered (t, target, sender): k_aa_build below.
// The reference's test is  sqrt(dx^2 + dy^2) < radius  in float32 (UTIL:88).  sqrtf is correctly rounded and monotone, so that is
// exactly  dx^2 + dy^2 < T  with T the smallest float whose square root reaches the radius (radius2_threshold, host): same
// survivors for every input, without a 25-instruction IEEE square root per candidate.
// The sum of squares is formed the way torch.norm forms it on the reference's side (measured: acc = fl(dx * dx), then
// fma(dy, dy, acc) -- 0 mismatches in 2 M random pairs, against 8 % for the other contraction order), spelled out so that the
// compiler's choice of contraction cannot move a borderline pair.
__device__ __forceinline__ float norm2_sq(float dx, float dy) { return fmaf(dy, dy, __fmul_rn(dx, dx)); }
__device__ __forceinline__ bool within_radius2(float dx, float dy, float thr2) { return norm2_sq(dx, dy) < thr2; }
static float radius2_threshold(float radius) {
  if (!(radius > 0.f)) return 0.f;                                       // sqrt(x) < r <= 0 never holds (x >= 0)
  if (std::isinf(radius)) return radius;
  float t = radius * radius;
  if (std::isinf(t)) t = std::numeric_limits<float>::max();
  while (t > 0.f && std::sqrt(t) >= radius) t = std::nextafter(t, 0.f);                                            // sqrt(t) < radius
  while (std::sqrt(t) < radius) t = std::nextafter(t, std::numeric_limits<float>::infinity());                      // smallest t with sqrt(t) >= radius
  return t;
}

// vmask[i]: bit t set when actor i is valid (not padded) at history step t
__device__ __forceinline__ void valid_mask_body(int i, int N, int H, int TT, const uint8_t* __restrict__ pad, uint32_t* __restrict__ vmask) {
  if (i >= N) return;
  uint32_t m = 0;
  uint8_t v[32];
#pragma unroll
  for (int t = 0; t < 32; ++t) v[t] = pad[int64_t(i) * TT + (t < H ? t : H - 1)];     // all loads in flight (H <= 32)
#pragma unroll
  for (int t = 0; t < 32; ++t) m |= uint32_t(t < H && !v[t]) << t;
  vmask[i] = m;
}
// time-major copies of the history positions and inputs ([H][N] float2): snapshot t of a scene's actors is then 8 N_scene contiguous
// bytes (k_aa_build stages it in LDS) instead of one 8-byte piece out of every 8 TT-byte row
__device__ __forceinline__ void time_major_body(int blk, int N, int H, int TT, const float* __restrict__ pos,
                                                const float* __restrict__ x, float2* __restrict__ pos_t, float2* __restrict__ x_t) {
  float2 pv[4], xv[4];
  int ii[4], tt[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = (blk * 4 + u) * 256 + int(threadIdx.x);              // = i * H + t
    const bool live = idx < N * H;
    ii[u] = live ? idx / H : -1;
    tt[u] = live ? idx - ii[u] * H : 0;
    pv[u] = live ? reinterpret_cast<const float2*>(pos)[int64_t(ii[u]) * TT + tt[u]] : float2{0.f, 0.f};
    xv[u] = live ? reinterpret_cast<const float2*>(x)[int64_t(ii[u]) * H + tt[u]] : float2{0.f, 0.f};
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (ii[u] >= 0) {
      pos_t[int64_t(tt[u]) * N + ii[u]] = pv[u];
      x_t[int64_t(tt[u]) * N + ii[u]] = xv[u];
    }
}

// lane feature (ENC:68-71); torch's negative index wraps when a lane is fully padded
__device__ __forceinline__ void lane_feat_body(int l, int L, int P, const float* __restrict__ lp, const float* __restrict__ pad,
                                               float* __restrict__ feat) {
  if (l >= L) return;
  float len = 0.f;
  for (int j0 = 0; j0 < P; j0 += 8) {                                // eight paddings in flight, summed in order
    float pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) pv[u] = pad[int64_t(l) * P + (j0 + u < P ? j0 + u : P - 1)];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (j0 + u < P) len += 1.0f - pv[u];
  }
  int last = int(len - 1.0f);
  if (last < 0) last += P;
  feat[2 * l] = lp[(int64_t(l) * P + last) * 2] - lp[int64_t(l) * P * 2];
  feat[2 * l + 1] = lp[(int64_t(l) * P + last) * 2 + 1] - lp[int64_t(l) * P * 2 + 1];
}

// exclusive prefix sums of TWO count arrays of n entries by one workgroup of 256 threads (the row pointers of the two CSRs: n = N + 1),
// 8 192 entries per round -- 32 consecutive entries per thread, all requested before the first is used; the counts were formed by other
// workgroups' atomics: read coherently
template <int NA = 2>
__device__ __forceinline__ void block_scan_two(const int32_t* __restrict__ in0, int32_t* __restrict__ out0, const int32_t* __restrict__ in1,
                                               int32_t* __restrict__ out1, int n) {
  __shared__ int32_t s_w[2][4];
  __shared__ int32_t s_carry[2];
  constexpr int PT = 32;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < 2) s_carry[t] = 0;
  __syncthreads();
  const CoherentI32 c0(in0), c1(NA > 1 ? in1 : in0);
  for (int base = 0; base < n; base += 256 * PT) {
    int32_t v[NA][PT], sum[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) sum[a] = 0;
#pragma unroll
    for (int c = 0; c < PT; ++c) {
      const int i = base + PT * t + c;
      v[0][c] = i < n ? c0[i] : 0;
      if constexpr (NA > 1) v[1][c] = i < n ? c1[i] : 0;
    }
#pragma unroll
    for (int c = 0; c < PT; ++c) {
#pragma unroll
      for (int a = 0; a < NA; ++a) sum[a] += v[a][c];
    }
    int32_t inc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) inc[a] = sum[a];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int32_t o = __shfl_up(inc[a], d);
        if (lane >= d) inc[a] += o;
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int a = 0; a < NA; ++a) s_w[a][wv] = inc[a];
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      int32_t run = s_carry[a] + inc[a] - sum[a];
      for (int w = 0; w < wv; ++w) run += s_w[a][w];
      int32_t* out = a ? out1 : out0;
#pragma unroll
      for (int c = 0; c < PT; ++c) {
        const int i = base + PT * t + c;
        if (i < n) out[i] = run;
        run += v[a][c];
      }
    }
    __syncthreads();
    if (t < NA) s_carry[t] += s_w[t][0] + s_w[t][1] + s_w[t][2] + s_w[t][3];
    __syncthreads();
  }
}

// ---- dataset-order actor lists: degrees from the scene extents (see the head of this section)
__device__ __forceinline__ void raise_general(unsigned int* general) {
  __hip_atomic_fetch_or(general, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (result unused: no return trip)
}
// node i: its scene is [first, last) = the run of batch[i] around i (both binary searches in flight together; were `batch` not sorted
// the answers are still first <= i < last <= N, and the order check below sends the batch down the general path)
// Each node also looks at ONE pair of neighbouring list positions (a scattered one): in dataset order the sources never descend and the
// targets of one source ascend.  That proves nothing, but a shuffled, target-major or otherwise reordered list fails it somewhere with
// near certainty, and then the word is up before k_direct2 starts, whose checking blocks stand down: such a list pays the general path
// and two near-empty launches, not a discarded pass over the list as well.  `pre_raise`: the A/B switch that sends every batch that way.
__device__ __forceinline__ void direct_degree_body(int i, int N, const int64_t* __restrict__ batch, const int64_t* __restrict__ ei, int E,
                                                   int pre_raise, int32_t* __restrict__ deg, int32_t* __restrict__ scene_lo,
                                                   unsigned int* __restrict__ general) {
  if (i >= N) return;
  const int64_t c = batch[i];
  bool descends = i + 1 < N && batch[i + 1] < c;
  if (E >= 2) {
    const int p = int((uint32_t(i) * 2654435761u) % uint32_t(E - 1));
    const int64_t s0 = ei[p], s1 = ei[p + 1], d0 = ei[int64_t(E) + p], d1 = ei[int64_t(E) + p + 1];
    descends |= s1 < s0 || (s1 == s0 && d1 <= d0);
  }
  descends |= pre_raise != 0 && i == 0;
  int l0 = 0, h0 = i;                    // first index of [0, i] whose scene id is >= c
  int l1 = i + 1, h1 = N;                // first index of (i, N] whose scene id is > c (N: none)
  while (l0 < h0 || l1 < h1) {
    const int m0 = (l0 + h0) >> 1, m1 = l1 < h1 ? (l1 + h1) >> 1 : i;
    const int64_t b0 = batch[m0], b1 = batch[m1];
    if (l0 < h0) { if (b0 < c) l0 = m0 + 1; else h0 = m0; }
    if (l1 < h1) { if (b1 <= c) l1 = m1 + 1; else h1 = m1; }
  }
  store_through(&deg[i], l1 - l0 - 1);   // (read by the launch's last workgroup: block_scan_two)
  scene_lo[i] = l0;
  if (descends) raise_general(general);
}

// First launch of the graph stage: every per-input pass that depends on nothing but the batch, as block ranges of one launch --
// [0, b0) actor-edge degrees (histogram, or from the scene extents: direct_degree_body), [b0, b1) lane-edge degrees, [b1, b2) extended-node table, [b2, b3) fake agents' inputs, [b3, b4) validity
// masks, [b4, b5) time-major copies, [b5, ..) lane features -- and, by the workgroup that finishes last, both CSR row pointers
// (exclusive scans of the degree histograms, which are formed by agent-scope atomics: see last_block_done).
struct FirstPassArgs {
  int N, A, H, TT, L, P, E, Ea, b0, b1, b2, b3, b4, b5, blocks;
  const int64_t *edge_index, *lane_actor_index, *agent_index, *batch, *source;
  const uint8_t *bos, *pad;
  const float *x, *pos, *lane_pos, *lane_pad;
  int32_t *deg, *la_deg, *rowptr, *la_rowptr, *orig, *eos, *pick_slot;
  uint8_t* nus;
  float *x_fake, *lane_feat;
  float2 *pos_t, *x_t;
  uint32_t* vmask;
  unsigned int* done;
  int direct;                    // [0, b0) are direct_degree_body blocks (dataset-order attempt) instead of the actor histogram; 2: word pre-raised
  int32_t* scene_lo;
  unsigned int* general;
  NoiseArg na;
};
__global__ __launch_bounds__(256) void k_prep_first(const FirstPassArgs a) {
  const int blk = blockIdx.x, i = threadIdx.x;
  if (blk < a.b0) {
    if (a.direct) direct_degree_body(blk * 256 + i, a.N, a.batch, a.edge_index, a.E, a.direct == 2, a.deg, a.scene_lo, a.general);
    else degree_body(blk, a.edge_index, a.E, a.deg);
  }
  else if (blk < a.b1) degree_body(blk - a.b0, a.lane_actor_index, a.Ea, a.la_deg);
  else if (blk < a.b2) ext_nodes_body((blk - a.b1) * 256 + i, a.N, a.A, a.H, a.agent_index, a.batch, a.source, a.bos, a.orig, a.nus, a.eos, a.pick_slot);
  else if (blk < a.b3) fake_x_body((blk - a.b2) * 256 + i, a.A, a.H, a.x, a.agent_index, a.na, a.x_fake);
  else if (blk < a.b4) valid_mask_body((blk - a.b3) * 256 + i, a.N, a.H, a.TT, a.pad, a.vmask);
  else if (blk < a.b5) time_major_body(blk - a.b4, a.N, a.H, a.TT, a.pos, a.x, a.pos_t, a.x_t);
  else lane_feat_body((blk - a.b5) * 256 + i, a.L, a.P, a.lane_pos, a.lane_pad, a.lane_feat);
  if (!last_block_done(a.done, unsigned(a.blocks))) return;
  block_scan_two(a.deg, a.rowptr, a.la_deg, a.la_rowptr, a.N + 1);
}

// Second launch of a dataset-order attempt: blocks [0, nb_e) check the input list against the closed form, one thread per POSITION of
// the list (any mix of scene sizes keeps every lane busy; both rows are coalesced 8-byte reads, four per thread in flight), and write
// the CSR entry, its target and the global-interactor keep-flag as k_row_sort2 would have; the last blocks are the lane half of
// k_scatter2.  The source the list names
// must be the row whose stretch [rowptr[s], rowptr[s + 1]) holds the position -- those stretches tile [0, E) once the row pointers
// ascend from 0 to E, which blocks [nb_e, nb_e + nb_n) check while they reset the degree counters for the general path -- and the
// target must be the closed form's.  Ids read from the list index memory only after they are known to be node ids.
constexpr int DIRECT_EPT = 4;
__global__ __launch_bounds__(256) void k_direct2(const int64_t* __restrict__ ei, int E, int N, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ scene_lo, int32_t* __restrict__ deg, const uint32_t* __restrict__ vmask,
                                                      int tref, int32_t* __restrict__ csr_src, int32_t* __restrict__ csr_dst, uint8_t* __restrict__ flags_g,
                                                      unsigned int* __restrict__ general, int nb_e, int nb_n, const int64_t* __restrict__ lai, int Ea,
                                                      const int32_t* __restrict__ la_rowptr, int32_t* __restrict__ la_deg, int64_t* __restrict__ la_pack) {
  const int blk = blockIdx.x, tid = threadIdx.x;
  if (blk >= nb_e + nb_n) {
    scatter_lane_body(blk - nb_e - nb_n, lai, Ea, la_rowptr, la_deg, la_pack);
    return;
  }
  bool bad = false;
  if (blk >= nb_e) {
    const int i = (blk - nb_e) * 256 + tid;
    if (i < N) {
      deg[i] = 0;                                                          // the general path's histogram counts from zero
      bad = rowptr[i] > rowptr[i + 1] || (i == N - 1 && rowptr[N] != E);
    }
  } else {
    if (*general != 0u) return;                                            // already known not to be in dataset order (earlier launch)
    int64_t src[DIRECT_EPT], dst[DIRECT_EPT];
#pragma unroll
    for (int u = 0; u < DIRECT_EPT; ++u) {
      const int p = (blk * DIRECT_EPT + u) * 256 + tid;
      src[u] = p < E ? ei[p] : -1;
      dst[u] = p < E ? ei[int64_t(E) + p] : -1;
    }
    int beg[DIRECT_EPT], end[DIRECT_EPT], lo[DIRECT_EPT];
    uint32_t vs[DIRECT_EPT], vd[DIRECT_EPT];
#pragma unroll
    for (int u = 0; u < DIRECT_EPT; ++u) {
      const bool ids = src[u] >= 0 && src[u] < N && dst[u] >= 0 && dst[u] < N;
      const int sn = ids ? int(src[u]) : 0, dn = ids ? int(dst[u]) : 0;
      beg[u] = rowptr[sn]; end[u] = rowptr[sn + 1]; lo[u] = scene_lo[sn];
      vs[u] = vmask[sn]; vd[u] = vmask[dn];
      if (!ids) beg[u] = INT32_MAX;                                        // (fails the range test below)
    }
#pragma unroll
    for (int u = 0; u < DIRECT_EPT; ++u) {
      const int p = (blk * DIRECT_EPT + u) * 256 + tid;
      if (p < E) {
        const int sn = int(src[u]);
        const int64_t v = int64_t(lo[u]) + p - beg[u];
        bad |= !(p >= beg[u] && p < end[u] && dst[u] == v + (v >= sn ? 1 : 0));
        csr_src[p] = int32_t(dst[u]);
        csr_dst[p] = sn;
        flags_g[p] = uint8_t((vs[u] >> tref) & (vd[u] >> tref) & 1u);
      }
    }
  }
  if (__any(bad) && (tid & 63) == 0) raise_general(general);
}

// The general path behind a failed dataset-order attempt: the histogram and the row pointers, then the scatter, as launches of their
// own that return at once while the word is zero (k_row_sort2's actor blocks do the same).  The lane CSR is not touched.
__global__ __launch_bounds__(256) void k_fb_degree(const unsigned int* __restrict__ general, const int64_t* __restrict__ ei, int E, int N,
                                                   int32_t* __restrict__ deg, int32_t* __restrict__ rowptr, unsigned int* __restrict__ done) {
  if (*general == 0u) return;
  degree_body(blockIdx.x, ei, E, deg);
  if (!last_block_done(done, gridDim.x)) return;
  block_scan_two<1>(deg, rowptr, nullptr, nullptr, N + 1);
}
__global__ __launch_bounds__(256) void k_fb_scatter(const unsigned int* __restrict__ general, const int64_t* __restrict__ ei, int E,
                                                    const int32_t* __restrict__ rowptr, int32_t* __restrict__ deg, int32_t* __restrict__ csr_src) {
  if (*general == 0u) return;
  scatter_body(blockIdx.x, ei, E, rowptr, deg, csr_src);
}

// Canonical order of both CSRs in one launch: blocks [0, nb_a) sort the actor rows (values = senders; also names the target of every
// position, csr_dst, and writes the keep-flag of the global-interactor edge at that position: both ends valid at the reference step,
// AGG:41), the rest sort the lane rows (values = lane << 32 | edge id; writes the edge ids, the actor of every position and the
// keep-flag of the lane-actor edge: |vector| < radius, ENC:198).  flags[E] (the scans' extra element) is zero.
// `general`: null, or the word of a dataset-order attempt -- while it is zero the actor rows are already in place (k_direct2) and the
// actor blocks stand down.
__global__ __launch_bounds__(256) void k_row_sort2(const unsigned int* __restrict__ general, int N, int nb_a, int nb_l, const int32_t* __restrict__ rowptr, int32_t* __restrict__ csr_src,
                                                   int32_t* __restrict__ csr_dst, const uint32_t* __restrict__ vmask, int tref, int E,
                                                   uint8_t* __restrict__ flags_g, const int32_t* __restrict__ la_rowptr,
                                                   int64_t* __restrict__ la_pack, int32_t* __restrict__ la_eid, int32_t* __restrict__ la_actor,
                                                   const float* __restrict__ vec, float radius, int Ea, uint8_t* __restrict__ flags_la) {
  __shared__ int64_t buf[4096];
  const int blk = blockIdx.x;
  if (blk == 0 && threadIdx.x == 0) {
    flags_g[E] = 0;
    flags_la[Ea] = 0;
  }
  if (blk < nb_a) {
    if (E <= 0) return;
    if (general != nullptr && *general == 0u) return;
    auto emit = [&](int p, int32_t sender, int row) { flags_g[p] = uint8_t((vmask[sender] >> tref) & (vmask[row] >> tref) & 1u); };
    row_sort_part<int32_t>(blk, nb_a, rowptr, N, csr_src, nullptr, csr_dst, reinterpret_cast<int32_t*>(buf), emit);
  } else {
    if (Ea <= 0) return;
    auto emit = [&](int p, int64_t packed, int row) {
      (void)row;
      const int64_t e = packed & 0xFFFFFFFFll;
      flags_la[p] = uint8_t(sqrtf(norm2_sq(vec[2 * e], vec[2 * e + 1])) < radius);                    // ENC:198
    };
    row_sort_part<int64_t>(blk - nb_a, nb_l, la_rowptr, N, la_pack, la_eid, la_actor, buf, emit);
  }
}

// ---- exclusive prefix sums of the graph stage: one launch for all of them, no library.  (Rounds 1-3 called hipcub::DeviceScan: two
// launches per scan -- init_lookback_scan_state + the scan -- and rocPRIM on the hot path for what are 8 K .. 2 M element scans; round 4
// one launch per scan.)
// "Chained scan with decoupled look-back": a workgroup takes a ticket (so that a workgroup only ever waits for workgroups that have
// already started), scans its chunk in registers, publishes its sum, then walks back over the published words of its predecessors
// -- a wave looks at 64 of them at a time -- until it meets one that carries a complete prefix; it then publishes its own.  One
// 64-bit word per workgroup holds (state << 32 | value), read and written with agent-scope atomics; the words and the ticket are
// zeroed by the memset that already clears the degree counters (PrepWs::zeroed).  Values are counts < 2^31.
constexpr int SCAN_MAX_BLOCKS = 512;
constexpr int SCAN_WORDS = SCAN_MAX_BLOCKS + 1;            // per scan instance: the ticket + one word per workgroup
constexpr int SCAN_INSTANCES = 3;                          // agent-agent segments, global flags, lane flags
// wave 0 of workgroup `b` (in ticket order): publish `total`, return the sum of the totals of workgroups 0 .. b-1
__device__ __forceinline__ int32_t lookback_prefix(unsigned long long* __restrict__ words, int b, int32_t total, int lane) {
  if (lane == 0)
    __hip_atomic_store(&words[b], ((b == 0 ? 2ull : 1ull) << 32) | (unsigned long long)(unsigned)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int32_t prefix = 0;
  if (b > 0) {
    int j = b - 1;
    for (long spins = 0;; ++spins) {
      if (spins > (1L << 28)) __builtin_trap();          // a predecessor never published: fail loudly, never hang
      const int k = j - lane;
      const unsigned long long w = k >= 0 ? __hip_atomic_load(&words[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (2ull << 32);
      const unsigned flag = unsigned(w >> 32);
      const unsigned long long done = __ballot(flag == 2u), none = __ballot(flag == 0u);
      const int upto = done ? __builtin_ctzll(done) : 63;    // the nearest predecessor with a complete prefix ends the walk
      const unsigned long long need = upto == 63 ? ~0ull : ((1ull << (upto + 1)) - 1);
      if (none & need) continue;                         // one of the words we need is not there yet: look again
      int32_t part = lane <= upto ? int32_t(unsigned(w)) : 0;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) part += __shfl_xor(part, d);
      prefix += part;
      if (done) break;
      j -= 64;
    }
    if (lane == 0)
      __hip_atomic_store(&words[b], (2ull << 32) | (unsigned long long)(unsigned)(prefix + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return prefix;
}
struct ScanJob {
  const void* in;          // int32 (u8 == 0) or uint8 (u8 == 1) counts
  int32_t* out;            // out[i] = sum of in[0 .. i), i < n; in == out is allowed
  int n, u8, blocks;
  unsigned long long* st;  // this scan's SCAN_WORDS zeroed words
};
struct ScanMultiArgs {
  ScanJob j[3];
  int njobs, blocks;
};
template <int PER>                                         // PER elements per thread, PER x 1024 per workgroup
__global__ __launch_bounds__(1024) void k_scan_multi(const ScanMultiArgs a) {
  __shared__ int32_t wsum[16];
  __shared__ int s_bid;
  __shared__ int32_t s_prefix;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int blk = blockIdx.x, q = 0;
  while (q + 1 < a.njobs && blk >= a.j[q].blocks) { blk -= a.j[q].blocks; ++q; }
  const ScanJob& job = a.j[q];
  const int n = job.n;
  if (t == 0) s_bid = int(__hip_atomic_fetch_add(&job.st[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();
  const int b = s_bid;
  const int64_t first = (int64_t(b) * 1024 + t) * PER;
  int32_t v[PER];
  int32_t s = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    v[i] = first + i < n ? (job.u8 ? int32_t(static_cast<const uint8_t*>(job.in)[first + i]) : static_cast<const int32_t*>(job.in)[first + i]) : 0;
    s += v[i];
  }
  int32_t inc = s;                                          // inclusive scan of the threads' sums inside the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int32_t wbase = 0;
  for (int w = 0; w < wv; ++w) wbase += wsum[w];
  if (wv == 0) {
    int32_t total = lane < 16 ? wsum[lane] : 0;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) total += __shfl_xor(total, d);
    total = __shfl(total, 0);
    const int32_t prefix = lookback_prefix(job.st + 1, b, total, lane);
    if (lane == 0) s_prefix = prefix;
  }
  __syncthreads();
  int32_t run = s_prefix + wbase + inc - s;                 // exclusive prefix of this thread's first element
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    if (first + i < n) job.out[first + i] = run;
    run += v[i];
  }
}
// The segment pointers of the global and lane lists (positions of the row starts among the survivors) and the list lengths: read off
// the finished prefix sums, so in a LATER launch -- k_collect_counts behind the scans when the host wants the lengths (exact graphs),
// else the first workgroups of k_graph_fill.  (A "last workgroup of the scan launch" tail was built first: it needs every scan output
// written through to the point of coherence, 2.8 M four-byte transactions, and cost more than this launch.)
struct CollectArgs {
  int64_t n_aa;
  int E, Ea, N;
  const int32_t *aa_segptr, *cpos_g, *cpos_la, *rowptr, *la_rowptr;
  int32_t *g_segptr, *la_segptr, *counts;
  float radius, thr2;
  int radius_dev;            // the radius is already in counts[4] (left there by k_aa_count): keep it
};
__device__ __forceinline__ void collect_body(int i, const CollectArgs& a) {
  if (i <= a.N) {
    a.g_segptr[i] = a.cpos_g[a.rowptr[i]];
    a.la_segptr[i] = a.cpos_la[a.la_rowptr[i]];
  }
  if (i == 0) {
    a.counts[0] = 0;
    a.counts[1] = a.aa_segptr[a.n_aa];
    a.counts[2] = a.cpos_g[a.E];
    a.counts[3] = a.cpos_la[a.Ea];
    if (!a.radius_dev) reinterpret_cast<float*>(a.counts)[4] = a.radius;
  }
}
__global__ void k_collect_counts(const CollectArgs a) { collect_body(blockIdx.x * blockDim.x + threadIdx.x, a); }

// ---- the agent-agent snapshot lists.  ONE WAVE PER EXTENDED NODE, ALL HISTORY STEPS, twice:
//   k_aa_count   lane = candidate (the node's CSR row: the in-edges of its actor; the fake agents' rows alias their actors'), 64 x 4
//                candidates in registers at a time; per step t the candidates' positions come from the TIME-MAJOR copy (the senders of a
//                row are ascending, mostly consecutive actor ids: one step's positions of 64 candidates are ~512 contiguous bytes) --
//                seven steps' loads in flight together; survivor test (both ends valid at t, closer than the radius); the wave's ballot
//                IS the stored word: bal[(row chunk)][t], 8 bytes per 64 candidates and step, and lane t ends up with the count of (t, node).
//   (k_scan_multi turns the counts into the segment pointers)
//   fill         (blocks of k_graph_fill) lane = OUTPUT record: per step the r-th survivor of the row is found from the row's ballot
//                words (prefetched into registers for all steps: one coalesced load), so records are computed and written 64 at a
//                time, contiguously -- no lane idles on a non-survivor and no store instruction is issued for a handful of lanes.
// What a wave needs for all steps -- segment starts, the target's own positions, the ballot words -- is fetched once, before the
// step loop.  Results equal evaluating every (t, in-edge) candidate in row order: same predicate, same order (ascending CSR position =
// ascending sender), same arithmetic for the geometry.
// History.  Rounds 2-4: ballots over 64 consecutive CSR positions with 168-byte position-row gathers (76 us) + count (7 us) + fill with
// one wave per (node, 3 steps) (76 us) at 32 x 256 agents.  Tried this round and dropped, all bit-identical: a workgroup per (step,
// 16 nodes) with the scene's snapshot staged in LDS -- seven dependent round trips a workgroup (count 54 us, fill 110 us); step groups
// with the candidates in registers and NaN-poisoned staging so that the test is subtract-square-add-compare (count 47 us, fill
// 190 us: four sparse store pairs per (row, step), three waves per SIMD behind 33 KB of LDS); and count + decoupled look-back + fill in
// ONE pass (0.29 ms: a look-back window is 64 workgroups per round trip to the point of coherence, so the prefix advances 64
// workgroups per ~2 us however many run).
// Records are (x_j R_i | (pos_j - pos_i) R_i) (ENC:584-585) + the target's snapshot node; order: t, node, ascending sender.
struct AaArgs {
  int N, Nt, H;
  float radius, thr2;                      // radius test: dx^2 + dy^2 < thr2 ...
  int thr2_dev;                            // ... or read from counts[5] (trajsde_graph_compact does not get the radius)
  const int32_t *rowptr, *csr_src, *orig;
  const uint32_t* vmask;
  const float2 *pos_t, *x_t;
  const float* rot;
  int32_t* segptr;
  int32_t* counts;
  unsigned long long* bal;                 // [row chunk][H]; the chunks of row o start at (rowptr[o] >> 6) + o
  const unsigned int* general;             // the word of a dataset-order attempt (null: none was made); counts[6] reports the path
  const int32_t* scene_lo;                 // first node of every actor's scene (valid while the word is zero)
  int32_t *aa_dst, *aa_src;
  float* geom;
};
// first ballot slot of a row: rows' chunk counts ceil(deg / 64) <= floor(deg / 64) + 1 fit between consecutive starts
__device__ __forceinline__ int64_t bal_base(int row_start, int o) { return int64_t(row_start >> 6) + o; }
// index of the r-th (0-based) set bit of w (r < popcount(w))
__device__ __forceinline__ int nth_set_bit(unsigned long long w, int r) {
  int posn = 0;
#pragma unroll
  for (int width = 32; width >= 1; width >>= 1) {
    const int c = __popcll((w >> posn) & ((1ull << width) - 1ull));
    if (r >= c) { r -= c; posn += width; }
  }
  return posn;
}
// a direct-path row holds the scene's nodes but its own, ascending: candidate idx of row o is lo + idx + (lo + idx >= o), no csr_src gather
__device__ __forceinline__ bool aa_direct(const AaArgs& a) {
  return a.general != nullptr && *a.general == 0u;
}
constexpr int AA_CG = 4, AA_SG = 7;        // candidates: 64 x AA_CG in registers; steps: AA_SG loads in flight per chunk
__global__ __launch_bounds__(256) void k_aa_count(const AaArgs a) {
  const int lane = threadIdx.x & 63;
  const int N = a.N, Nt = a.Nt, H = a.H;
  // a wave = (node, group of AA_SG steps); xcd_grid launch: a scene's nodes share an L2
  const int wid = __builtin_amdgcn_readfirstlane(int(xcd_block() * 4 + (threadIdx.x >> 6)));
  const int groups = (H + AA_SG - 1) / AA_SG, node = wid / groups, t0 = (wid - node * groups) * AA_SG;
  if (wid == 0 && lane == 0) {
    a.segptr[int64_t(H) * Nt] = 0;                                         // the scan's extra element (total at the end)
    reinterpret_cast<float*>(a.counts)[4] = a.radius;
    reinterpret_cast<float*>(a.counts)[5] = a.thr2;                        // the threshold the counts are formed with: the fill reads it here
    a.counts[6] = a.general != nullptr && *a.general == 0u ? 1 : 0;        // 1: the actor CSR came from the closed form (k_direct2)
  }
  if (node >= Nt) return;
  const int o = node < N ? node : __builtin_amdgcn_readfirstlane(a.orig[node]);
  const int beg = __builtin_amdgcn_readfirstlane(a.rowptr[o]), end = __builtin_amdgcn_readfirstlane(a.rowptr[o + 1]);
  const uint32_t vo = __builtin_amdgcn_readfirstlane(a.vmask[o]);
  const int chunks = (end - beg + 63) >> 6;
  const int64_t bbase = bal_base(beg, o);
  const bool direct = aa_direct(a);                                        // (uniform)
  const int lo = direct ? __builtin_amdgcn_readfirstlane(a.scene_lo[o]) : 0;
  const float thr2 = a.thr2;
  int mycnt = 0;                                                           // lane t: survivors of (t, node)
  for (int c0 = 0; c0 < chunks; c0 += AA_CG) {
    int s[AA_CG];
    uint32_t m[AA_CG];
    if (direct) {
#pragma unroll
      for (int u = 0; u < AA_CG; ++u) {
        const int idx = 64 * (c0 + u) + lane, v = lo + idx;
        s[u] = beg + idx < end ? v + (v >= o ? 1 : 0) : -1;
      }
    } else {
#pragma unroll
      for (int u = 0; u < AA_CG; ++u) {
        const int p = beg + 64 * (c0 + u) + lane;
        s[u] = p < end ? a.csr_src[p] : -1;
      }
    }
#pragma unroll
    for (int u = 0; u < AA_CG; ++u) {
      m[u] = s[u] >= 0 ? (a.vmask[s[u]] & vo) : 0u;                        // steps at which both ends are valid
      s[u] = s[u] >= 0 ? s[u] : 0;
    }
    unsigned long long mine[AA_CG];
#pragma unroll
    for (int u = 0; u < AA_CG; ++u) mine[u] = 0ull;
    {
      float2 ps[AA_CG][AA_SG], pd[AA_SG];
#pragma unroll
      for (int q = 0; q < AA_SG; ++q) {
        const int t = t0 + q < H ? t0 + q : H - 1;
        pd[q] = a.pos_t[int64_t(t) * N + o];
#pragma unroll
        for (int u = 0; u < AA_CG; ++u) ps[u][q] = a.pos_t[int64_t(t) * N + s[u]];
      }
#pragma unroll
      for (int q = 0; q < AA_SG; ++q) {
        const int t = t0 + q;
        if (t >= H) break;                                                 // (uniform)
#pragma unroll
        for (int u = 0; u < AA_CG; ++u) {
          const bool ok = ((m[u] >> t) & 1u) && within_radius2(ps[u][q].x - pd[q].x, ps[u][q].y - pd[q].y, thr2);
          const unsigned long long B = __ballot(ok);
          mine[u] = lane == t ? B : mine[u];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < AA_CG; ++u)
      if (c0 + u < chunks && lane >= t0 && lane < t0 + AA_SG && lane < H) {
        if (node < N) a.bal[(bbase + c0 + u) * H + lane] = mine[u];        // (a fake agent's row is its actor's: those words are the actor's)
        mycnt += __popcll(mine[u]);
      }
  }
  if (lane >= t0 && lane < t0 + AA_SG && lane < H) a.segptr[int64_t(lane) * Nt + node] = mycnt;
}
// the records of one extended node (all steps), one wave
__device__ __forceinline__ void aa_fill_node(const AaArgs& a, int node, int part, int parts, int lane) {
  const int N = a.N, Nt = a.Nt, H = a.H;
  const int o = node < N ? node : __builtin_amdgcn_readfirstlane(a.orig[node]);
  const int beg = __builtin_amdgcn_readfirstlane(a.rowptr[o]), end = __builtin_amdgcn_readfirstlane(a.rowptr[o + 1]);
  if (end <= beg) return;
  const int chunks = (end - beg + 63) >> 6;
  const unsigned long long* __restrict__ words = a.bal + bal_base(beg, o) * H;     // [chunk][H] of this row
  // per step, lane t: segment start and length, the target's position
  int base_l = 0, n_l = 0;
  float2 pd_l = {0.f, 0.f};
  if (lane < H) {
    base_l = a.segptr[int64_t(lane) * Nt + node];
    n_l = a.segptr[int64_t(lane) * Nt + node + 1] - base_l;
    pd_l = a.pos_t[int64_t(lane) * N + o];
  }
  // the row's ballot words for all steps, two per lane (rows of up to 128 / H chunks; longer rows read them as they go)
  const int nw = chunks * H;
  const bool in_regs = nw <= 128;
  unsigned long long w0 = 0ull, w1 = 0ull;
  if (in_regs) {
    if (lane < nw) w0 = words[lane];
    if (64 + lane < nw) w1 = words[64 + lane];
  }
  const bool direct = aa_direct(a);                                        // (uniform)
  const int lo = direct ? __builtin_amdgcn_readfirstlane(a.scene_lo[o]) : 0;
  const f4 R = *reinterpret_cast<const f4*>(a.rot + 4 * o);
  auto word = [&](int c, int t) -> unsigned long long {                    // (uniform arguments, uniform result)
    if (in_regs) {
      const int i = c * H + t;
      const unsigned long long src = i < 64 ? w0 : w1;
      const unsigned lo_ = __builtin_amdgcn_readlane(unsigned(src), i & 63), hi_ = __builtin_amdgcn_readlane(unsigned(src >> 32), i & 63);
      return (static_cast<unsigned long long>(hi_) << 32) | lo_;
    }
    return words[int64_t(c) * H + t];
  };
  for (int t = part; t < H; t += parts) {                                  // `parts` waves share a node's steps: more gathers in flight
    const int n = __builtin_amdgcn_readlane(n_l, t);
    if (n == 0) continue;                                                  // (uniform)
    const int64_t base = __builtin_amdgcn_readlane(base_l, t);
    const float pdx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pd_l.x), t));
    const float pdy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pd_l.y), t));
    const float2* __restrict__ pos_t = a.pos_t + int64_t(t) * N;
    const float2* __restrict__ x_t = a.x_t + int64_t(t) * N;
    const int seg = t * Nt + node;
    for (int r0 = 0; r0 < n; r0 += 64) {
      const int r = r0 + lane;
      unsigned long long selw = 0ull;
      int selc = 0, rr = 0, cum = 0;
      for (int c = 0; c < chunks; ++c) {                                   // the row's ballot words are wave-uniform
        const unsigned long long w = word(c, t);
        const int cc = __popcll(w);
        if (r >= cum && r < cum + cc) { selw = w; selc = c; rr = r - cum; }
        cum += cc;
        if (cum >= r0 + 64) break;                                         // (uniform) every lane of this round is served
      }
      if (r < n) {
        const int idx = 64 * selc + nth_set_bit(selw, rr);
        const int sdr = direct ? lo + idx + (lo + idx >= o ? 1 : 0) : a.csr_src[beg + idx];     // senders are real actors
        const float2 ps = pos_t[sdr], xs = x_t[sdr];
        const float dx = ps.x - pdx, dy = ps.y - pdy;
        const float x0 = xs.x, x1 = xs.y;
        const f4 g = {x0 * R[0] + x1 * R[2], x0 * R[1] + x1 * R[3], dx * R[0] + dy * R[2], dx * R[1] + dy * R[3]};   // v @ R_i (ENC:584-585)
        const int64_t k = base + r;
        *reinterpret_cast<f4*>(a.geom + 4 * k) = g;
        a.aa_dst[k] = seg;
        if (a.aa_src != nullptr) a.aa_src[k] = sdr;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- global / lane edges
// global interactor edges: both endpoints valid at the reference step (AGG:41); relative pose AGG:42-50
__device__ __forceinline__ void g_compact_body(int p, int E, int TT, int tref, const int32_t* __restrict__ csr_src, const int32_t* __restrict__ csr_dst,
                                               const float* __restrict__ pos, const float* __restrict__ rot, const float* __restrict__ ang,
                                               const uint8_t* __restrict__ flags, const int32_t* __restrict__ cpos, int32_t* __restrict__ g_src,
                                               int32_t* __restrict__ g_dst, float* __restrict__ geom) {
  if (p >= E || !flags[p]) return;
  const int s = csr_src[p], i = csr_dst[p], q = cpos[p];
  const f4 R = *reinterpret_cast<const f4*>(rot + 4 * i);
  const float dx = pos[(int64_t(s) * TT + tref) * 2] - pos[(int64_t(i) * TT + tref) * 2];
  const float dy = pos[(int64_t(s) * TT + tref) * 2 + 1] - pos[(int64_t(i) * TT + tref) * 2 + 1];
  const float th = ang[s] - ang[i];                                                          // AGG:48-50
  f4 g = {dx * R[0] + dy * R[2], dx * R[1] + dy * R[3], cosf(th), sinf(th)};
  *reinterpret_cast<f4*>(geom + 4 * int64_t(q)) = g;
  g_src[q] = s;
  g_dst[q] = i;
}
__device__ __forceinline__ void la_compact_body(int p, int E_al, const int32_t* __restrict__ actor, const int32_t* __restrict__ eid,
                                                const int64_t* __restrict__ la_index, const float* __restrict__ vec,
                                                const float* __restrict__ lane_feat, const float* __restrict__ rot,
                                                const uint8_t* __restrict__ flags, const int32_t* __restrict__ cpos, int32_t* __restrict__ la_dst,
                                                int32_t* __restrict__ la_lane, float* __restrict__ geom) {
  if (p >= E_al || !flags[p]) return;
  const int i = actor[p], e = eid[p], q = cpos[p];
  const int lane = int(la_index[e]);                                   // row 0 of lane_actor_index
  const f4 R = *reinterpret_cast<const f4*>(rot + 4 * i);
  const float fx = lane_feat[2 * lane], fy = lane_feat[2 * lane + 1], vx = vec[2 * int64_t(e)], vy = vec[2 * int64_t(e) + 1];
  f4 g = {fx * R[0] + fy * R[2], fx * R[1] + fy * R[3], vx * R[0] + vy * R[2], vx * R[1] + vy * R[3]};   // ENC:763-764
  *reinterpret_cast<f4*>(geom + 4 * int64_t(q)) = g;
  la_dst[q] = i;
  if (la_lane != nullptr) la_lane[q] = lane;
}
// The launch of trajsde_graph_compact: blocks [0, nb_g) the global list, [nb_g, nb_g + nb_l) the lane list, the rest the agent-agent
// records
struct FillArgs {
  AaArgs aa;
  CollectArgs col;
  int nb_c;                  // sync-free graphs: the blocks that read the segment pointers / lengths off the prefix sums (else 0)
  int nb_g, nb_l, nb_a, parts;
  int E, TT, tref, Ea;
  const int32_t *csr_src, *csr_dst, *cpos_g, *la_actor, *la_eid, *cpos_la;
  const float *pos, *rot, *ang, *vec, *lane_feat;
  const uint8_t *flags_g, *flags_la;
  const int64_t* la_index;
  int32_t *g_src, *g_dst, *la_dst, *la_lane;
  float *g_geom, *la_geom;
};
__global__ __launch_bounds__(256) void k_graph_fill(const FillArgs f) {
  int blk = blockIdx.x;
  if (blk < f.nb_c) {
    collect_body(blk * 256 + threadIdx.x, f.col);
    return;
  }
  blk -= f.nb_c;
  if (blk < f.nb_g) {
    g_compact_body(blk * 256 + threadIdx.x, f.E, f.TT, f.tref, f.csr_src, f.csr_dst, f.pos, f.rot, f.ang, f.flags_g, f.cpos_g, f.g_src, f.g_dst, f.g_geom);
  } else if (blk < f.nb_g + f.nb_l) {
    la_compact_body((blk - f.nb_g) * 256 + threadIdx.x, f.Ea, f.la_actor, f.la_eid, f.la_index, f.vec, f.lane_feat, f.rot, f.flags_la, f.cpos_la,
                    f.la_dst, f.la_lane, f.la_geom);
  } else {
    // (XCD-aware order inside the range: nb_a is a multiple of 8; consecutive nodes -- one scene -- go to one XCD's L2)
    const int ab = blk - f.nb_g - f.nb_l, logical = (ab & 7) * (f.nb_a >> 3) + (ab >> 3);
    const int wid = __builtin_amdgcn_readfirstlane(logical * 4 + int(threadIdx.x >> 6));
    const int node = wid / f.parts, part = wid - node * f.parts;
    if (node < f.aa.Nt) aa_fill_node(f.aa, node, part, f.parts, threadIdx.x & 63);
  }
}

// phase-1 workspace layout, derived from the batch sizes alone (so both phases agree on it)
struct PrepWs {
  int32_t *deg, *rowptr, *csr_src, *csr_dst, *orig, *eos, *pick_slot, *counts;
  int32_t *la_deg, *la_rowptr, *la_eid, *la_actor;
  int64_t* la_pack;
  int32_t *aa_segptr, *g_segptr, *la_segptr, *cpos_g, *cpos_la;
  uint8_t *nus, *flags_g, *flags_la;
  uint32_t* vmask;               // per actor: bit t = valid at history step t
  float2 *pos_t, *x_t;           // [H][N] time-major copies of positions[:, :H] and x
  unsigned long long* bal;       // [row chunk][H]: survivors of 64 candidates of a CSR row at step t (k_aa_count)
  float *x_fake, *lane_feat;
  unsigned long long* scan_st;   // SCAN_INSTANCES x SCAN_WORDS zeroed words (k_scan_multi), directly behind the degree counters
  unsigned int* done;            // DONE_WAYS + 1 zeroed "workgroups finished" counters (last_block_done)
  unsigned int* done_fb;         // the same for k_fb_degree
  unsigned int* general;         // zeroed word: raised when the actor list is not in dataset order
  int32_t* scene_lo;             // per actor: first node of its scene (direct_degree_body)
  int64_t zeroed_bytes, n_aa, aa_blocks;
  int64_t total;
  bool ok;
  PrepWs(const trajsde_batch* b, void* ws, int64_t ws_bytes) {
    Carver c(ws, ws_bytes);
    const int64_t N = b->N, A = b->A, E = b->E, Nt = N + A, H = b->H, Ea = b->E_al;
    n_aa = H * Nt;
    aa_blocks = xcd_grid((Nt * ((H + 6) / 7) + 3) / 4);                    // k_aa_count: one wave per (extended node, group of AA_SG = 7 steps)
    // both degree arrays, the scans' and the look-back's state words, the finish counters: ONE block, one memset (graph_prepare)
    const int64_t deg_ints = (2 * (N + 1) + 1) / 2 * 2;
    constexpr int64_t DONE_WORDS = (DONE_WAYS + 2) / 2 + 1;            // 8-byte words per set of finish counters (room to spare)
    const int64_t st_words = int64_t(SCAN_INSTANCES) * SCAN_WORDS + 2 * DONE_WORDS + 1;
    deg = c.take<int32_t>(deg_ints + 2 * st_words); la_deg = ptr_add(deg, N + 1);
    scan_st = reinterpret_cast<unsigned long long*>(ptr_add(deg, deg_ints));
    done = reinterpret_cast<unsigned int*>(ptr_add(scan_st, int64_t(SCAN_INSTANCES) * SCAN_WORDS));
    done_fb = done + 2 * DONE_WORDS; general = done_fb + 2 * DONE_WORDS;
    zeroed_bytes = (deg_ints + 2 * st_words) * int64_t(sizeof(int32_t));
    rowptr = c.take<int32_t>(N + 1); scene_lo = c.take<int32_t>(N + 1);
    csr_src = c.take<int32_t>(E + 1); csr_dst = c.take<int32_t>(E + 1);
    orig = c.take<int32_t>(Nt); eos = c.take<int32_t>(Nt); pick_slot = c.take<int32_t>(Nt); counts = c.take<int32_t>(8);
    la_rowptr = c.take<int32_t>(N + 1);
    la_eid = c.take<int32_t>(Ea + 1); la_actor = c.take<int32_t>(Ea + 1); la_pack = c.take<int64_t>(Ea + 1);
    aa_segptr = c.take<int32_t>(n_aa + 1); g_segptr = c.take<int32_t>(N + 1); la_segptr = c.take<int32_t>(N + 1);
    cpos_g = c.take<int32_t>(E + 1); cpos_la = c.take<int32_t>(Ea + 1);
    nus = c.take<uint8_t>(Nt); flags_g = c.take<uint8_t>(E + 1); flags_la = c.take<uint8_t>(Ea + 1);
    x_fake = c.take<float>(A * H * 2 + 4); lane_feat = c.take<float>(int64_t(b->L) * 2 + 4);
    vmask = c.take<uint32_t>(N + 1);
    pos_t = c.take<float2>(H * N + 1); x_t = c.take<float2>(H * N + 1);
    bal = c.take<unsigned long long>(((E >> 6) + N + 2) * H);
    total = c.off + 256;
    ok = c.ok;
  }
};

struct EdgeWs {
  float *aa_geom, *g_geom, *la_geom;
  int32_t *aa_dst, *aa_src, *g_src, *g_dst, *la_dst, *la_lane;
  int64_t total;
  bool ok;
  EdgeWs(const trajsde_batch* b, const trajsde_graph* g, void* ws, int64_t ws_bytes) {
    Carver c(ws, ws_bytes);
    (void)b;
    const int64_t Eaa = g->E_aa, Eg = g->E_g, Ela = g->E_la;            // (int64: E + 1 overflows int32 at the bound the ABI admits)
    aa_geom = c.take<float>(4 * Eaa + 4); aa_dst = c.take<int32_t>(Eaa + 1); aa_src = c.take<int32_t>(Eaa + 1);
    g_geom = c.take<float>(4 * Eg + 4); g_src = c.take<int32_t>(Eg + 1); g_dst = c.take<int32_t>(Eg + 1);
    la_geom = c.take<float>(4 * Ela + 4); la_dst = c.take<int32_t>(Ela + 1); la_lane = c.take<int32_t>(Ela + 1);
    total = c.off + 256;
    ok = c.ok;
  }
};

static int check_batch(const trajsde_batch* b) {
  TS_REQUIRE(b != nullptr, "batch: null");
  TS_REQUIRE(b->N > 0 && b->A >= 0 && b->H > 0 && b->H <= 32 && b->TT >= b->H, "batch: bad sizes (H <= 32)");
  TS_REQUIRE(b->E >= 0 && b->E_al >= 0 && b->L >= 0, "batch: negative sizes");
  TS_REQUIRE(int64_t(b->H) * b->E < (int64_t(1) << 31) - 2, "batch: too many (t, edge) candidates for int32 positions");
  TS_REQUIRE(b->x && b->positions && b->padding_mask && b->bos_mask && b->rotate_angles && b->batch && b->source,
             "batch: null actor tensor");
  TS_REQUIRE(b->A == 0 || b->agent_index, "batch: null agent_index");   // A == 0: no fake agents (forward_ood, ENC:204-370)
  TS_REQUIRE(b->E == 0 || b->edge_index, "batch: null edge_index");
  TS_REQUIRE(b->E_al == 0 || (b->lane_actor_index && b->lane_actor_vectors && b->lane_positions && b->lane_paddings),
             "batch: null lane tensor");
  return TRAJSDE_OK;
}

// TRAJSDE_GRAPH_DIRECT (read once): unset / 1 -- attempt the dataset-order path; 0 -- never (the six launches, decided on the host);
// 2 -- attempt with the word pre-raised, i.e. the device-decided general path on every batch (A/B runs of its cost).  No actor edge: no attempt.
static int direct_mode(const trajsde_batch* b) {
  static const int mode = []() { const char* e = getenv("TRAJSDE_GRAPH_DIRECT"); return e && e[0] == '0' && !e[1] ? 0 : (e && e[0] == '2' && !e[1] ? 2 : 1); }();
  return b->E > 0 ? mode : 0;
}
static bool try_direct(const trajsde_batch* b) { return direct_mode(b) != 0; }

static CollectArgs collect_args(const trajsde_batch* b, const PrepWs& w, float radius) {
  CollectArgs c;
  c.n_aa = w.n_aa; c.E = b->E; c.Ea = b->E_al; c.N = b->N;
  c.aa_segptr = w.aa_segptr; c.cpos_g = w.cpos_g; c.cpos_la = w.cpos_la; c.rowptr = w.rowptr; c.la_rowptr = w.la_rowptr;
  c.g_segptr = w.g_segptr; c.la_segptr = w.la_segptr; c.counts = w.counts; c.radius = radius; c.thr2 = 0.f; c.radius_dev = 0;
  return c;
}
static AaArgs aa_args(const trajsde_batch* b, const PrepWs& w, const float* rot, float radius) {
  AaArgs a;
  a.N = b->N; a.Nt = b->N + b->A; a.H = b->H;
  a.radius = radius; a.thr2 = radius2_threshold(radius); a.thr2_dev = 0;
  a.rowptr = w.rowptr; a.csr_src = w.csr_src; a.orig = w.orig; a.vmask = w.vmask; a.pos_t = w.pos_t; a.x_t = w.x_t; a.rot = rot;
  a.segptr = w.aa_segptr; a.counts = w.counts; a.bal = w.bal; a.general = try_direct(b) ? w.general : nullptr;
  a.scene_lo = w.scene_lo;
  a.aa_dst = nullptr; a.aa_src = nullptr; a.geom = nullptr;
  return a;
}

}  // namespace tsde

using namespace tsde;

static std::atomic<int> g_export_senders{0};

extern "C" {

float trajsde_radius2_threshold(float radius) { return radius2_threshold(radius); }

int trajsde_export_senders(int on) {
  const int prev = g_export_senders.exchange(on ? 1 : 0);
  return prev;
}

int trajsde_rotate(const float* rotate_angles, int32_t N, const float* y, int32_t F, float* rotate_mat, float* y_rot, void* stream) {
  TS_REQUIRE(rotate_angles && rotate_mat && N > 0, "rotate: bad argument");
  TS_REQUIRE(y == nullptr || y_rot != nullptr, "rotate: y given without y_rot");
  k_rotate<<<cdiv(int64_t(N) * (y != nullptr && F > 0 ? F : 1), 256), 256, 0, static_cast<hipStream_t>(stream)>>>(rotate_angles, N, y, F, rotate_mat, y_rot);
  TS_LAUNCH_CHECK("k_rotate");
  return TRAJSDE_OK;
}

int64_t trajsde_graph_ws_bytes(const trajsde_batch* b) {
  if (check_batch(b) != TRAJSDE_OK) return -1;
  PrepWs w(b, nullptr, 0);
  return w.total;
}

static int graph_prepare(const trajsde_batch* b, const float* rot, float radius, const trajsde_noise* fake_noise, void* ws,
                         int64_t ws_bytes, trajsde_graph* out, void* stream_, bool sync) {
  if (int rc = check_batch(b)) return rc;
  TS_REQUIRE(rot && ws && out, "graph_prepare: null pointer");
  PrepWs w(b, ws, ws_bytes);
  if (!w.ok) return fail(TRAJSDE_ERR_WORKSPACE, "graph_prepare: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const int N = b->N, A = b->A, E = b->E, H = b->H, TT = b->TT, Ea = b->E_al, Nt = N + A;
  NoiseArg na{0, nullptr, nullptr};
  if (fake_noise) { na.seed = fake_noise->seed; na.z = fake_noise->z; na.row_ids = fake_noise->row_ids; na.seed_dev = fake_noise->seed_dev; }

  TS_HIP(hipMemsetAsync(w.deg, 0, size_t(w.zeroed_bytes), st));       // degree counters, scan / look-back state words, finish counters
  const int tref = H - 1;
  const bool direct = try_direct(b);
  {
    ProfScope ps("k_prep_first", st);
    FirstPassArgs fa;
    fa.N = N; fa.A = A; fa.H = H; fa.TT = TT; fa.L = b->L; fa.P = b->lane_pts; fa.E = E; fa.Ea = Ea;
    fa.b0 = direct ? cdiv(N, 256) : cdiv(E, 256 * EPT);
    fa.b1 = fa.b0 + cdiv(Ea, 256 * EPT);
    fa.b2 = fa.b1 + cdiv(Nt, 256);
    fa.b3 = fa.b2 + (A > 0 ? cdiv(A * ((2 * H + 3) / 4), 256) : 0);
    fa.b4 = fa.b3 + cdiv(N, 256);
    fa.b5 = fa.b4 + cdiv(int64_t(N) * H, 1024);
    fa.blocks = fa.b5 + (b->L > 0 ? cdiv(b->L, 256) : 0);
    fa.edge_index = b->edge_index; fa.lane_actor_index = b->lane_actor_index; fa.agent_index = b->agent_index; fa.batch = b->batch;
    fa.source = b->source; fa.bos = b->bos_mask; fa.pad = b->padding_mask; fa.x = b->x; fa.pos = b->positions;
    fa.lane_pos = b->lane_positions; fa.lane_pad = b->lane_paddings;
    fa.deg = w.deg; fa.la_deg = w.la_deg; fa.rowptr = w.rowptr; fa.la_rowptr = w.la_rowptr; fa.orig = w.orig; fa.eos = w.eos;
    fa.pick_slot = w.pick_slot; fa.nus = w.nus; fa.x_fake = w.x_fake; fa.lane_feat = w.lane_feat; fa.pos_t = w.pos_t; fa.x_t = w.x_t;
    fa.vmask = w.vmask; fa.done = w.done + 0; fa.na = na;
    fa.direct = direct_mode(b); fa.scene_lo = w.scene_lo; fa.general = w.general;
    k_prep_first<<<fa.blocks, 256, 0, st>>>(fa);
  }
  if (direct) {
    {
      ProfScope ps("k_direct2", st);
      const int nb_e = cdiv(E, 256 * DIRECT_EPT), nb_n = cdiv(N, 256);
      k_direct2<<<nb_e + nb_n + cdiv(Ea, 256 * EPT), 256, 0, st>>>(b->edge_index, E, N, w.rowptr, w.scene_lo, w.deg, w.vmask, tref, w.csr_src, w.csr_dst,
                                                              w.flags_g, w.general, nb_e, nb_n, b->lane_actor_index, Ea, w.la_rowptr, w.la_deg, w.la_pack);
    }
    {
      ProfScope ps("k_fb_degree", st);
      k_fb_degree<<<cdiv(E, 256 * EPT), 256, 0, st>>>(w.general, b->edge_index, E, N, w.deg, w.rowptr, w.done_fb);
    }
    {
      ProfScope ps("k_fb_scatter", st);
      k_fb_scatter<<<cdiv(E, 256 * EPT), 256, 0, st>>>(w.general, b->edge_index, E, w.rowptr, w.deg, w.csr_src);
    }
  } else if (E > 0 || Ea > 0) {
    ProfScope ps("k_scatter2", st);
    const int nb_a = cdiv(E, 256 * EPT);
    k_scatter2<<<nb_a + cdiv(Ea, 256 * EPT), 256, 0, st>>>(b->edge_index, E, w.rowptr, w.deg, w.csr_src, nb_a, b->lane_actor_index, Ea, w.la_rowptr,
                                                     w.la_deg, w.la_pack);
  }
  {
    ProfScope ps("k_row_sort2", st);
    const int per_list = cdiv(N, 4) < 8192 ? cdiv(N, 4) : 8192;
    k_row_sort2<<<2 * per_list, 256, 0, st>>>(direct ? w.general : nullptr, N, per_list, per_list, w.rowptr, w.csr_src, w.csr_dst, w.vmask, tref, E, w.flags_g, w.la_rowptr,
                                              w.la_pack, w.la_eid, w.la_actor, b->lane_actor_vectors, radius, Ea, w.flags_la);
  }
  {
    ProfScope ps("k_aa_count", st);
    const AaArgs aa = aa_args(b, w, rot, radius);
    k_aa_count<<<int(w.aa_blocks), 256, 0, st>>>(aa);
  }
  {
    ProfScope ps("k_scan_multi", st);
    ScanMultiArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    int64_t nmax = 0;
    auto add = [&](const void* in, int32_t* out_, int64_t n, int u8, int inst) {
      ScanJob& j = sa.j[sa.njobs++];
      j.in = in; j.out = out_; j.n = int(n); j.u8 = u8; j.st = w.scan_st + int64_t(inst) * SCAN_WORDS;
      nmax = std::max(nmax, n);
    };
    add(w.aa_segptr, w.aa_segptr, w.n_aa + 1, 0, 0);
    add(w.flags_g, w.cpos_g, int64_t(E) + 1, 1, 1);
    add(w.flags_la, w.cpos_la, int64_t(Ea) + 1, 1, 2);
    TS_REQUIRE(nmax <= int64_t(SCAN_MAX_BLOCKS) * 65536, "graph stage: more than 33 M elements in a prefix sum");
    const int64_t per = (nmax + int64_t(SCAN_MAX_BLOCKS) * 1024 - 1) / (int64_t(SCAN_MAX_BLOCKS) * 1024);      // smallest class that needs <= 512 workgroups
    const int PER = per <= 8 ? 8 : (per <= 16 ? 16 : (per <= 32 ? 32 : 64));
    for (int q = 0; q < sa.njobs; ++q) {
      sa.j[q].blocks = cdiv(sa.j[q].n, PER * 1024);
      sa.blocks += sa.j[q].blocks;
    }
    if (PER == 8) k_scan_multi<8><<<sa.blocks, 1024, 0, st>>>(sa);
    else if (PER == 16) k_scan_multi<16><<<sa.blocks, 1024, 0, st>>>(sa);
    else if (PER == 32) k_scan_multi<32><<<sa.blocks, 1024, 0, st>>>(sa);
    else k_scan_multi<64><<<sa.blocks, 1024, 0, st>>>(sa);
  }
  if (sync) {                                           // the host wants the lengths now: read them off the prefix sums
    ProfScope ps("k_collect_counts", st);
    k_collect_counts<<<cdiv(N + 1, 256), 256, 0, st>>>(collect_args(b, w, radius));
  }
  TS_LAUNCH_CHECK("graph_prepare kernels");
  int32_t h[4] = {0, 0, 0, 0};
  if (sync) {
    TS_HIP(hipMemcpyAsync(h, w.counts, sizeof(h), hipMemcpyDeviceToHost, st));
    TS_HIP(hipStreamSynchronize(st));
  } else {
    // upper bounds: every (t, in-edge) candidate of every extended node survives.  The fake rows alias their agents' CSR
    // rows, whose in-degrees sum to at most E (repeated input edges count, so A * (N - 1) is NOT a bound)
    const int64_t aa_max = int64_t(H) * 2 * int64_t(E);
    (void)A;
    TS_REQUIRE(aa_max < (int64_t(1) << 31) - 2, "graph_prepare_async: too many (t, edge) candidates for int32 positions");
    h[1] = int32_t(aa_max); h[2] = E; h[3] = Ea;
  }
  std::memset(out, 0, sizeof(*out));
  out->counts = w.counts; out->exact = sync ? 1 : 0;
  out->Nt = Nt; out->E_ext = E; out->E_aa = h[1]; out->E_g = h[2]; out->E_la = h[3];
  out->orig = w.orig; out->nus_mask = w.nus; out->eos_idx = w.eos; out->pick_slot = w.pick_slot; out->x_fake = w.x_fake;
  out->aa_segptr = w.aa_segptr; out->g_segptr = w.g_segptr; out->la_segptr = w.la_segptr;
  return TRAJSDE_OK;
}

int trajsde_graph_prepare(const trajsde_batch* b, const float* rot, float radius, const trajsde_noise* fake_noise, void* ws,
                          int64_t ws_bytes, trajsde_graph* out, void* stream_) {
  return graph_prepare(b, rot, radius, fake_noise, ws, ws_bytes, out, stream_, true);
}

int trajsde_graph_prepare_async(const trajsde_batch* b, const float* rot, float radius, const trajsde_noise* fake_noise, void* ws,
                                int64_t ws_bytes, trajsde_graph* out, void* stream_) {
  return graph_prepare(b, rot, radius, fake_noise, ws, ws_bytes, out, stream_, false);
}

int64_t trajsde_graph_edges_ws_bytes(const trajsde_batch* b, const trajsde_graph* g) {
  if (!b || !g) return -1;
  EdgeWs e(b, g, nullptr, 0);
  return e.total;
}

int trajsde_graph_compact(const trajsde_batch* b, const float* rot, void* ws, int64_t ws_bytes, void* edges_ws,
                          int64_t edges_ws_bytes, trajsde_graph* out, void* stream_) {
  if (int rc = check_batch(b)) return rc;
  TS_REQUIRE(rot && ws && edges_ws && out, "graph_compact: null pointer");
  PrepWs w(b, ws, ws_bytes);
  EdgeWs e(b, out, edges_ws, edges_ws_bytes);
  if (!w.ok || !e.ok) return fail(TRAJSDE_ERR_WORKSPACE, "graph_compact: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream_);
  const int E = b->E, H = b->H, TT = b->TT, Ea = b->E_al;
  const bool want_src = g_export_senders.load() != 0;                      // sender ids are for checking the index work only
  {
    ProfScope ps("k_graph_fill", st);
    FillArgs f;
    f.aa = aa_args(b, w, rot, 0.f);
    f.aa.aa_dst = e.aa_dst; f.aa.aa_src = want_src ? e.aa_src : nullptr; f.aa.geom = e.aa_geom;
    f.nb_g = cdiv(E, 256); f.nb_l = cdiv(Ea, 256);
    f.E = E; f.TT = TT; f.tref = H - 1; f.Ea = Ea;
    f.csr_src = w.csr_src; f.csr_dst = w.csr_dst; f.cpos_g = w.cpos_g; f.la_actor = w.la_actor; f.la_eid = w.la_eid; f.cpos_la = w.cpos_la;
    f.pos = b->positions; f.rot = rot; f.ang = b->rotate_angles; f.vec = b->lane_actor_vectors; f.lane_feat = w.lane_feat;
    f.flags_g = w.flags_g; f.flags_la = w.flags_la; f.la_index = b->lane_actor_index;
    f.g_src = e.g_src; f.g_dst = e.g_dst; f.la_dst = e.la_dst; f.la_lane = want_src ? e.la_lane : nullptr;
    f.g_geom = e.g_geom; f.la_geom = e.la_geom;
    // sync-free graphs: nobody has read the segment pointers / lengths off the prefix sums yet (the radius those workgroups also
    // record is the one trajsde_graph_prepare left in the count block for exactly this)
    f.col = collect_args(b, w, 0.f);
    f.col.radius_dev = 1;
    f.nb_c = out->exact ? 0 : cdiv(b->N + 1, 256);
    const bool aa_work = E > 0 && out->E_aa > 0;
    static const int fill_parts = []() { const char* e = getenv("TRAJSDE_FILL_PARTS"); const int v = e ? atoi(e) : 3; return v >= 1 && v <= 32 ? v : 3; }();
    f.parts = fill_parts;
    f.nb_a = xcd_grid(cdiv(int64_t(b->N + b->A) * f.parts, 4));
    const int blocks = f.nb_c + f.nb_g + f.nb_l + (aa_work ? f.nb_a : 0);
    if (blocks > 0) k_graph_fill<<<blocks, 256, 0, st>>>(f);
  }
  TS_LAUNCH_CHECK("graph_compact kernels");
  out->aa_geom = e.aa_geom; out->aa_dst = e.aa_dst;
  out->aa_src = want_src ? e.aa_src : nullptr; out->la_lane = want_src ? e.la_lane : nullptr;
  out->g_geom = e.g_geom; out->g_src = e.g_src; out->g_dst = e.g_dst;
  out->la_geom = e.la_geom; out->la_dst = e.la_dst;
  return TRAJSDE_OK;
}

}  // extern "C"

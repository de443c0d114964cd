// wgrad.hpp -- the weight-gradient and deferred-sum engine of the backward pass (wgrad.hip): batches of dW = delta^T a problems over
// saved rows, column sums of per-wave vector partials, and the queues that run all sums of an entry point at its end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace tsde {

constexpr int WGRAD_CHUNK = 512;           // rows one k_wgrad workgroup reduces
constexpr int WGRAD_MAX_JOBS = 16;         // weight-gradient problems over the same rows that share one launch
// partial slots of a workspace: the largest single problem (+32: run_headwise_outer slices) plus room for batching small ones
inline int64_t wgrad_max_parts(int64_t rows, int64_t groups) { return (rows + WGRAD_CHUNK - 1) / WGRAD_CHUNK + groups + 33 + 2048; }

struct WgradJob {              // W[o*ldw + col0 + i] = sum_r delta[r*ldd + o] * a[r*lda + i];  bias[o] = sum_r delta[r*ldd + o] (or null)
  const float *delta, *a;
  float *W, *bias;
  int ldd, lda, ldw, col0, time_cols;
  // computed operand: when in2 is set, row r of `a` is ReLU(LN(Linear(2,64)(geom[r][pair], geom[r][pair+1]))) evaluated
  // on the fly from the 16-byte geometry record `a + 4r` with the closed-form block `in2` (layouts.hpp In2L) and `beta`
  // -- the activation rows of the two embedding branches are never written to or read from HBM
  const float *in2, *beta;
  int pair;
};
struct WgradJobs {
  WgradJob j[WGRAD_MAX_JOBS];
  int n;
};
__global__ void k_wgrad(WgradJobs jobs, int64_t R, int64_t rows_per_group, int chunk, int chunks_per_group, int P, float* part, float* cs);
__global__ void k_reduce_partials(WgradJobs jobs, const float* part, const float* cs, int P, int chunks_per_group, const float* step_tab);
constexpr int COLSUM_MAX_JOBS = 8;         // vectors cut from the same slab of per-wave partials that share one launch
struct ColsumJob {
  const float* src;            // first column of the vector inside the slab
  float* dst;
  int n, dst_stride;
};
struct ColsumJobs {
  ColsumJob j[COLSUM_MAX_JOBS];
  int n;
};
__global__ void k_colsum(ColsumJobs jobs, int64_t rows, int stride);

struct WgradCtx {
  hipStream_t st;
  float *part, *cs;            // scratch for `cap` partials of 4096 / 64 floats
  const float* step_tab;       // only read when time_cols is set
  int64_t cap;                 // = wgrad_max_parts(...) the workspace was carved with
};
// several weight-gradient problems over the SAME rows (R, rows_per_group) in one pair of launches (grid.y = problem)
struct WgradBatch {
  const WgradCtx& c;
  int64_t R, rows_per_group;
  WgradJobs jobs;
  const char* tag;             // name of the launch in the profile table (the edge-embedding batch carries its own: its roofline)
  WgradBatch(const WgradCtx& ctx, int64_t R_, int64_t rpg, const char* tag_ = "k_wgrad") : c(ctx), R(R_), rows_per_group(rpg), tag(tag_) { jobs.n = 0; }
  int add(const float* delta, int ldd, const float* a, int lda, float* W, int ldw, int col0, float* bias, int time_cols);
  int add_in2(const float* delta, int ldd, const float* geom, int pair, const float* in2, const float* beta, float* W, int ldw, float* bias);
  int flush();
  int flush_edge();           // the edge embedding's three problems (k_wgrad6_edge); falls back to flush()
};
// W[o*ldw + col0 + i] = sum_r delta[r*ldd + o] * a[r*lda + i]  (o, i < 64);  bias[o] = sum_r delta[r*ldd + o] (or null)
int run_wgrad(const WgradCtx& c, const float* delta, int ldd, const float* a, int lda, int64_t R, int64_t rows_per_group, float* W,
              int ldw, int col0, float* bias, int time_cols);
// ---- deferred sums.  A backward entry point of the SDE path produces ~35 weight-gradient batches and ~33 slabs of per-wave vector
// partials; summing each with its own launch (two dozen microseconds apiece, a handful of workgroups) cost 0.7 ms of a 12.4 ms step.
// With a DeferredSums object alive, WgradBatch::flush / run_headwise_outer leave their partials where they are (a bump allocator over
// the context's partial buffer) and ColsumBatch::flush leaves the slab where it is (vpart_slab hands every producer its own), and the
// sums of the whole entry point run in a few wide launches at finish() -- or earlier, whenever one of the two areas is full.  Same
// fixed summation order as the immediate kernels; nothing reads a gradient buffer before the entry point returns.
struct ReduceJob {             // one 64 x 64 (+ bias / time columns) block: its partials start at slot `base`
  float *W, *bias;
  int64_t base;
  int P, cpg, ldw, col0, time_cols;
};
constexpr int REDUCE_MAX_JOBS = 64;
struct ReduceJobs {
  ReduceJob j[REDUCE_MAX_JOBS];
  int n;
};
struct ColsumQJob {
  const float* src;
  float* dst;
  int64_t rows;
  int n, stride, dst_stride;
};
constexpr int COLSUMQ_MAX_JOBS = 96;
struct ColsumQJobs {
  ColsumQJob j[COLSUMQ_MAX_JOBS];
  int n;
};
struct ReduceQueue {
  hipStream_t st;
  float *part, *cs;
  const float* step_tab;
  int64_t cap, used;
  std::vector<ReduceJob> jobs;
  int64_t take(int64_t slots, int* rc);      // first slot of a fresh run of `slots` partials (drains first when they do not fit)
  int drain();
};
struct ColsumQueue {
  hipStream_t st;
  float* arena;
  int64_t cap, used;
  std::vector<ColsumQJob> jobs;
  float* take(int64_t floats);               // null: does not fit even after a drain (the caller falls back to its shared slab)
  int drain();
};
ReduceQueue*& active_reduce_queue();
ColsumQueue*& active_colsum_queue();
struct DeferredSums {
  ReduceQueue rq;
  ColsumQueue cq;
  DeferredSums(hipStream_t st, float* part, float* cs, int64_t cap, const float* step_tab, float* arena, int64_t arena_floats);
  ~DeferredSums();                           // deactivates the queues (error paths); launches nothing
  int finish();                              // the remaining sums; the queues stay active and empty
  DeferredSums(const DeferredSums&) = delete;
};
// the slab a producer of per-wave vector partials writes ([rows][stride] floats) and the ColsumBatch built on it reads: the
// caller's shared slab, or -- with deferred sums active -- a slab of its own that stays intact until the sums have run
float* vpart_slab(float* shared_slab, int64_t rows, int stride);
constexpr int64_t VPART_ARENA_SLABS = 6;     // the arena of a workspace, in units of VPART_FLOATS

int run_colsum(hipStream_t st, const float* src, int64_t rows, int stride, int n, float* dst, int dst_stride = 1);
int run_colsum_tall(hipStream_t st, const float* src, int64_t rows, int stride, int n, float* dst, float* scratch /* 256 x n floats */);
// several vectors of the same slab (rows x stride floats of per-wave partials) in one launch
struct ColsumBatch {
  hipStream_t st;
  int64_t rows;
  int stride;
  ColsumJobs jobs;
  ColsumBatch(hipStream_t st_, int64_t rows_, int stride_) : st(st_), rows(rows_), stride(stride_) { jobs.n = 0; }
  int add(const float* src, int n, float* dst, int dst_stride = 1);
  int flush();
};

}  // namespace tsde

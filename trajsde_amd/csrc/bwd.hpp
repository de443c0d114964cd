// bwd.hpp -- pieces of the backward pass shared across translation units: the weight-gradient engine (wgrad.hpp, defined in
// wgrad.hip), the decoder backward's shared kernels and the node-level backward kernels (node_bwd.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "dropout.hpp"
#include "wgrad.hpp"

namespace tsde {

// ---- pieces of the SDE decoder backward reused by the MLP decoder backward (decoder_bwd.hip)
struct InitV { enum : int { DGAM = 0, DBET = 64, SIZE = 128 }; };               // per-wave vector slots of k_dec_init_bwd
__global__ void k_l2_wta(const float* loc, const float* y, const uint8_t* mask, int N, int K, int T, int32_t* best, float* minsum,
                         int32_t* cnt, int KP);
__global__ void k_l2_finalize(const float* minsum, const int32_t* cnt, int N, float* scal);
// Laplace NLL (losses/laplace_nll_loss.py:29-44) of the winning mode: per-actor sums, then loss / (2 count) and 1 / (2 count)
__global__ void k_nll_value(const float* loc, const float* y, const uint8_t* mask, const int32_t* best, int N, int T, float eps,
                            float* minsum);
__global__ void k_nll_finalize(const float* minsum, const int32_t* cnt, int N, float* scal);
// what a head backward under the Laplace NLL reads of the forward: the winning mode's loc | scale values and the clamp
struct NllArg {
  const float* loc;        // [K, N, T, 4] forward outputs
  const int32_t* best;     // winning mode per actor
  float eps, min_scale;
};
__global__ void k_init_sel(const float* img, const float* local, const float* global, const int32_t* best, int N, float* y0, float* gsel);
__global__ void k_dec_init_bwd(const float* img, const float* local, const float* gsel, const float* DY0, const int32_t* best, int N,
                               float* DA, float* d_local, float* d_global, float* vpart);

// ---- backward from caller-supplied cotangents of loc and pi, all K * N paths (decoder_cot_bwd.hip)
// per-wave vector slots of k_head_bwd_cot: the loc head's LayerNorm / last-layer gradients, then the scale head's
struct CotHeadV { enum : int { DGAM = 0, DBET = 64, DW3X = 128, DW3Y = 192, DB3 = 256, HEAD = 264, LOC = 0, SCALE = HEAD, SIZE = 2 * HEAD }; };
struct PiV { enum : int { DGAM = 0, DBET = 64, DW3 = 128, DB3 = 192, SIZE = 196 }; };      // ... of k_pi_head_bwd
__global__ void k_init_all(const float* img, const float* local, const float* global, int N, int K, float* y0);
__global__ void k_head_bwd_cot(const float* img_loc, const float* img_sc, const float* states, const float* out_tab, const float* loc,
                               const float* d_loc, float min_scale, int NN, int T, float* S_in, float* DU, float* DU2, float* DS, float* vpart);
__global__ void k_dec_init_bwd_all(const float* img, const float* local, const float* global, const float* DY0, int N, int K, float* DA,
                                   float* DAS, float* d_local, float* d_global, float* vpart);
__global__ void k_pi_head_bwd(const float* img, const float* local, const float* global, const float* d_pi, int N, int K, float* DP,
                              float* DPS, float* d_local, float* d_global, float* vpart);

// W[d][c] = sum_i X[i][d] * Y[i][head(d)][c]   (X [N,64], Y [N,heads,64]) through wc.part
int run_headwise_outer(const WgradCtx& wc, const float* X, const float* Y, int64_t N, float* W, int heads = 8);

// ---- node-level backward blocks (node_bwd.hip)
__global__ void k_ffn_bwd_a(const float* img, const float* dout, const float* xn2, int64_t R, float* H, float* DH, float* DOUT2, DropArg drop);
__global__ void k_ffn_bwd_b(const float* img, const float* DH, const float* dout, const float* x1, int64_t R, float* dx1, float* vpart);
__global__ void k_upd_bwd(const float* img, const float* dx1, const float* agg, const float* xn, int64_t R, float* UPD, float* DGP,
                          float* DS, float* DAGG, float* DXN, float* DX1M, DropArg drop);
template <int NQ>
__global__ void k_node_proj_bwd(const float* img, const float* x, const float* dres, const float* dxn_part, const float* dp0,
                                const float* dp1, const float* dp2, int64_t R, float* dx_out, float* xn_out, float* vpart);
template <int BR>
__global__ void k_edge_embed_bwd_branch(const float* img, const float* geom, const float* DSP, int64_t E, float* vpart);
__global__ void k_lin_t_acc(const float* wt, const float* d, int64_t R, float* out, int accumulate);
__global__ void k_lin_t_sum(const float* wt, int64_t wt_stride, const float* d, int64_t d_stride, int K, int64_t R, float* out);

constexpr int64_t VPART_FLOATS = int64_t(2048) * 4 * 320;     // per-wave vector partials of the widest kernel at the largest grid

struct NodeBlockTape { const float *agg, *xn, *x1, *xn2; };                      // forward activations [R,64]
struct NodeBlockScratch { float *H, *DH, *dx1, *UPD, *DGP, *DS, *vpart; };        // [R,256] x2, [R,64] x4, VPART_FLOATS
struct NodeBlockGrads {                                                           // parameter-shaped gradient buffers
  float *w_ih, *b_ih, *w_hh, *b_hh, *w_self, *b_self, *w_out, *b_out, *n2g, *n2b, *w1, *b1, *w2, *b2;
};
// backward of  x1 = x + out_proj(gated update(agg, xn)),  out = x1 + mlp(norm2(x1))  given dout [R,64]:
// writes dagg, dxn (the block's contribution to d xn) and sc.dx1 (= d x1, also the residual gradient of x)
int node_block_backward(const float* img /*NodeBlockBwdL*/, const NodeBlockTape& tp, const float* dout, int64_t R,
                        const NodeBlockScratch& sc, const WgradCtx& wc, const NodeBlockGrads& gr, float* dagg, float* dxn,
                        hipStream_t st, const DropArg& drop, WgradBatch* defer = nullptr);

// the FFN half alone (TemporalEncoderLayer: linear1 / linear2 / norm2); uses gr.w1, b1, w2, b2, n2g, n2b only
int ffn_block_backward(const float* img_a /*FfnBwdAL*/, const float* img_b /*FfnBwdBL*/, const float* xn2, const float* x1,
                       const float* dout, int64_t R, const NodeBlockScratch& sc, const WgradCtx& wc, const NodeBlockGrads& gr,
                       hipStream_t st, const DropArg& drop);

struct EdgeEmbedScratch { float *S, *DEP, *DSP, *vpart; };                       // [E,64] x3
struct EdgeEmbedGrads {
  float *a_w0, *a_b0, *a_g, *a_e, *b_w0, *b_b0, *b_g, *b_e, *wa3, *ba3, *wb3, *bb3, *ag0, *ae0, *w2, *b2, *ag3, *ae3;
};
// what the attention backward over stored embedding rows leaves per edge (run_edge_attn_bwd), for the embedding backward to
// build d emb from: the edges' targets, the targets' q / dagg rows, the (alpha d, d logit) scalars and lin_k^T | lin_v^T
struct EdgeAttnGrad {
  const int32_t* dst;
  const float *q, *dagg, *EA, *ED;
  const float* wkvt;           // [2][64][64]: lin_k.weight^T | lin_v.weight^T (EdgeKvBwdL::WKT, WVT)
  int heads;
};
// `demb`: d emb rows [E,64], or (ag != null) built inside the kernel from the attention scalars
int edge_embed_backward(const float* img /*EdgeBwdL*/, const float* geom, const float* demb, int64_t E, const EdgeEmbedScratch& sc,
                        const WgradCtx& wc, const EdgeEmbedGrads& gr, hipStream_t st, const EdgeAttnGrad* ag = nullptr);

// ---- wave-per-target attention backward (aggregator_bwd.hip), shared by the global interactor and the AA / AL encoders
struct DrelArgs {
  const float* EA[4];          // per layer: [E][HEADS] alpha d_e (the weight the values were summed with)
  const float* ED[4];          // per layer: [E][HEADS] d logit / sqrt(dh)
  const float* UZ[4];          // per layer: [N][HEADS][2][64] (U_h, Z_h) of every target, or (from_rows) unused
  const float *img, *q, *dagg; // from_rows: GAttnL image and the targets' q / dagg rows
};
// DREL[e] (+)= sum over the `nl` <= 4 layers and heads of ED U_h + EA Z_h
int run_gattn_drel(hipStream_t st, int heads, int nl, bool from_rows, const DrelArgs& da, const int32_t* segptr, int64_t N, float* DREL,
                   int accumulate);
// attention over stored edge rows `emb` [E,64] (k = lin_k(emb), v = lin_v(emb); img = GAttnL): given dagg [R,64] and the forward's
// (max, 1/sum) statistics, writes DQ [R,64], RL / SS [R,heads,64] (lin_k / lin_v weight gradients as headwise outer products
// with q / dagg), DAGGM [R,64] (column sum = lin_v bias gradient) and the per-edge scalars EA / ED [E,heads]
int run_edge_attn_bwd(hipStream_t st, int heads, const float* img, const int32_t* segptr, const float* emb, const float* q, const float* agg,
                      const float* dagg, const float* stats, int64_t R, float* DQ, float* RL, float* SS, float* DAGGM, float* EA, float* ED,
                      const DropArg& drop, const WgradCtx* wc = nullptr, float* wk = nullptr, float* wv = nullptr, float* bv = nullptr,
                      bool* weights_done = nullptr);
// (wc / wk / wv / weights_done: the kernel may accumulate the lin_k / lin_v weight gradients itself -- *weights_done then tells the caller to
//  skip its two run_headwise_outer calls and the column sum of DAGGM (lin_v.bias); RL / SS / DAGGM are not written in that case)

// ---- TemporalEncoder backward kernels (grid_bwd.hip)
__global__ void k_tr_final_bwd(const float* norm, const float* x, const float* dtout, int N, float* DX, float* vpart);
template <int HEADS, bool DROP>
__global__ void k_tr_attention_bwd(const float* q, const float* k, const float* v, const float* dO, int N, float* dq, float* dk, float* dv,
                                   DropArg drop);
__global__ void k_drop_rows(const float* src, int64_t R, float* dst, DropArg drop, int kind);        // dst = src * factors of (row, feature)
__global__ void k_tr_prep_bwd(const float* DX0, const uint8_t* pad, int N, int TT, float* DAA);
__global__ void k_tr_tok_grad(const float* DX0, const uint8_t* pad, int N, int TT, float* dpad, float* dcls, float* dpos);

// ordered parameter names of a stage (the dry run of its pack recipe, pack.hip)
std::vector<std::string> stage_param_names(int stage, int num_layers, int num_modes);

}  // namespace tsde

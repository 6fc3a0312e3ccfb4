// dmx — host launchers of the templated kernel families.  Each family is instantiated in its
// own translation unit (k_*.hip) so the library builds in parallel; engine.hip only calls
// these functions.
#pragma once
#include <cstdlib>

#include "common.h"
#include "dmx.h"
#include "igemm.h"
#include "igemm_x3.h"
#include "objective_args.h"
#include "prediction_args.h"
#include "tail_math.h"
#include "tokmlp.h"

namespace dmx {

// split-precision implicit GEMM (igemm_x3.h): bm, bn in {64, 128}; sa = A from f16 hi/lo planes;
// x1 = config-4 fp16 arithmetic.  k_x3_stats.hip (EPI_STATS), k_x3_part.hip (EPI_PARTIAL),
// k_x3_epi.hip (EPI_BIAS / EPI_BIAS_GELU / EPI_BIAS_RES).
void launch_x3_stats(int bm, int bn, int sa, int x1, const X3Params& p, dim3 grid, hipStream_t st);
// (EPI_STATS / EPI_PARTIAL instances: 8-wave blocks for 128 x 128 tiles — up1.0 -3 %, same-box A/B —
// and 4 waves otherwise; the 64 x 128 split-K tiles at 4x4 / 8x8 are at parity or slower with 8.)
void launch_x3_partial(int bm, int bn, int sa, int x1, const X3Params& p, dim3 grid, hipStream_t st);
void launch_x3_epi(int epi, int bm, int bn, int sa, int x1, const X3Params& p, dim3 grid, hipStream_t st);
// 512-thread ping-pong split-precision GEMM (igemm_pp.h), EPI_STATS, 256 x bn tiles, A from f16 planes.
void launch_pp(int bn, int x1, const X3Params& p, dim3 grid, hipStream_t st);
// halo-staged split-precision 3x3 conv (igemm_halo.h), EPI_STATS, 256-pixel x bn tiles, image
// width w in {16, 32}, bn in {128, 64}; 16-wave blocks, B staged in LDS per (chunk, tap) step;
// k_halo.hip.  gna (sa = 0 only) = 1: GroupNorm + GELU of the raw source applied while staging;
// = 2: GELU(residual + GroupNorm(source)).
void launch_halo(int bn, int w, int sa, int x1, int gna, const X3Params& p, dim3 grid, hipStream_t st);
// chunk-staged halo conv of the low-resolution maps (igemm_halo_cs_kernel; w in {8, 4}, H == w):
// 256-pixel tiles of whole samples x 64 channels, all nine taps of a chunk's B slice in LDS; epi
// EPI_PARTIAL (grid.z = K splits over 32-channel chunks, P.g.ksplit chunks each) or EPI_STATS
// (w = 8); k_halo_cs.hip.
void launch_halo_cs(int epi, int w, int sa, int x1, const X3Params& p, dim3 grid, hipStream_t st);
// Winograd F(2x2, 3x3) split-precision 3x3 conv (igemm_wino.h), 64 tiles (256 pixels) x 64 channels
// per block, w in {4, 8, 16, 32} (4: EPI_PARTIAL, gna 0 only), gna as launch_halo, x1 = 1 the fp16
// (config 4) instances; k_wino.hip.  epi EPI_STATS (GroupNorm partials: HW / 16 rows per sample) or
// EPI_PARTIAL (grid.z = K splits over 16-channel chunks).
void launch_wino(int epi, int w, int gna, int x1, const X3Params& p, dim3 grid, hipStream_t st);
// U = G g Gᵀ of a packed fp32 3x3 weight ([npad][kpad], k = tap * cin + c), scaled, split, fragment order
void launch_wino_pack(const float* B, int kpad, int cin, int cout, float scale, _Float16* uh, _Float16* ul,
                      hipStream_t st);
// exact-fp32 MFMA implicit GEMM (igemm.h), k_f32.hip.
void launch_f32(int src_mode, int epi, int bm, int bn, const IgemmParams& p, dim3 grid, hipStream_t st);
// attention cores (k_attn.hip): split-precision (D, waves-per-EU hint, x1) and exact fp32 (D, QT).
void launch_attention_x3(int D, int wpe, int x1, const float* qkv, float* out, int L, int C, dim3 grid,
                         hipStream_t st, float* stats = nullptr);
// D = 16 core with the head resident in LDS; grid (1, 4, N), nw waves per block.
hipError_t launch_attention16(int nw, int x1, const float* qkv, float* out, int L, int C, int N, hipStream_t st,
                              float* stats = nullptr);
void launch_attention_f32(int D, int qt, const float* qkv, float* out, int L, int C, dim3 grid, hipStream_t st,
                          float* stats = nullptr);
// fused attention-block token kernels (tokmlp.h), k_tok.hip.
void launch_tok_qkv_lds(int C, int tpb, int x1, const TokParams& tp, dim3 grid, hipStream_t st);
// C = 256 QKV with 8-wave blocks of 64 tokens x 384 columns (tok_ln_qkv_w_kernel); grid (M / 64, 2).
void launch_tok_qkv_w(int C, int x1, const TokParams& tp, dim3 grid, hipStream_t st);
void launch_tok_qkv(int C, int nb, int x1, const TokParams& tp, dim3 grid, hipStream_t st);
void launch_tok_out(int C, int tm, int x1, int nw, int lds, int tpb, const TokParams& tp, int blocks,
                    hipStream_t st);
// CFG rescale (guidance.h), k_guidance.hip.  The head's operands as the step tails take them: feat
// [2B][HW][64] NHWC = [uncond B | cond B], w [Co][64], b [Co]; range_flag as in StepTailParams.
struct CfgHeadParams {
  const float* feat; const float* w; const float* b;
  int Co, B, HW;
  float guidance;
  int* range_flag;
};
// stage 1: head + CFG mix, eg (NCHW [B][Co][HW]) and per-block moments part [B][nb][4] (doubles),
// nb = cdiv(HW, Co == 4 ? 16 : 256) blocks per sample
void launch_cfg_stats(const CfgHeadParams& p, float* eg, double* part, int nb, hipStream_t st);
// stage 2: r[n] from the partials (pixb pixels per stage-1 block), eg scaled in place; ratio_out [B] or null
void launch_cfg_scale(float* eg, const double* part, int nb, int pixb, int Co, int HW, int B, float phi,
                      float* ratio_out, hipStream_t st);
// standalone: one block per sample over its `total` = c*h*w elements
void launch_cfg_rescale(const float* eu, const float* ec, float g, float phi, float* eps, float* ratio_out, int n,
                        int64_t total, hipStream_t st);
// Composed guidance (compose.h), k_compose.hip.  K extra branches over the base branch; weight [K][B].
struct ComposeParams {
  int K;
  const float* weight;
};
// the step tail over a branch-major feature map [(K+1) B][HW][64] (p as the plain Co = 4 head tail takes
// it; p.cfg / p.guidance are not read); grid (cdiv(HW, 16), B)
void launch_compose_tail4(const StepTailParams& p, const ComposeParams& q, bool ddim, bool dpm, dim3 grid,
                          hipStream_t st);
// the mix alone: e [(K+1)][n][chw], weight [K][n] -> eps [n][chw]; n * chw < 2^39
void launch_compose_eps(const float* e, const float* weight, int K, int n, int64_t chw, float* eps, hipStream_t st);
// Perturbed-attention guidance (perturb.h), k_perturb.hip.  The identity-attention core:
// out [M][C] = the V third of qkv [M][3C], an exact fp32 copy; C in {64, 128, 256}; M * C / 1024 < 2^31
void launch_attn_identity(const float* qkv, float* out, int64_t M, int C, hipStream_t st);
// Geometry guidance (geom.h), k_geom.hip.
// loss [n] (or null) and seed [n][gd] = dL_n / dgeom of the masked regression loss on geom against vals / mask [n][gd]
void launch_geom_seed(const float* geom, const float* vals, const float* mask, int n, int gd, float* loss, float* seed,
                      hipStream_t st);
// eps_out = eps + (scale[n] * sig[pos - 1]) * grad over [n][chw]; n * chw < 2^39; eps_out may alias eps
void launch_geom_mix(const float* eps, const float* grad, const dmx_geom_guide& gg, const int64_t* pos, int pos_stride,
                     int n, int64_t chw, float* eps_out, int* range_flag, hipStream_t st);
// dx (NCHW [n][Ci][H][W]) = the data gradient of the first 3x3 conv (weight [64][Ci][3][3]) from dr (NHWC, 64 channels)
void launch_conv0_dgrad(const float* dr, const float* w, int Ci, int n, int H, int W, float* dx, hipStream_t st);
// The optimizer step (optim.h), k_optim.hip: with max_norm > 0 and norm_out, the gradient's sum of squares per
// chunk into partials [n_chunks] and norm / coef into norm_out [2]; then the Adam update, one block per chunk.
// n_chunks < 2^31 (checked by dmx_optim_create); chunks, rows, partials and norm_out are device memory.
struct OptimLaunch {
  const dmx_optim_chunk* chunks;
  int64_t n_chunks;
  const dmx_optim_tensor* rows;
  double* partials;
  float max_norm, ema_d, ema_omd;
  float* norm_out;
};
void launch_optim_step(const OptimLaunch& o, hipStream_t st);
// The training objective (objective.h), k_objective.hip; arguments as checked by objective_args.h.
// noise: one launch; loss: one block per sample, then the one-block finish; seed: one launch.
// (target: the v-prediction target of dmx_train_noise_target, or null)
void launch_train_noise(const dmx_noise_args& a, float* target, hipStream_t st);
void launch_objective_loss(const dmx_objective_args& a, hipStream_t st);
void launch_objective_seed(const dmx_objective_args& a, const float* up, float* d_eps, float* d_geom, hipStream_t st);
// v-prediction (prediction.h), k_prediction.hip; arguments as checked by prediction_args.h.
// eps_out = p_o[t - 1] out + p_x[t - 1] x over [n][chw]; n * chw < 2^39; eps_out may alias out
void launch_pred_to_eps(const float* out, const float* x, const int64_t* t, int t_stride, const float* p_o,
                        const float* p_x, int T, int n, int64_t chw, float* eps_out, hipStream_t st);
// x0_out = p_o[t - 1] x - p_x[t - 1] out and eps_out as above, in one pass; eps_out may alias out
void launch_pred_split(const float* out, const float* x, const int64_t* t, int t_stride, const float* p_o,
                       const float* p_x, int T, int n, int64_t chw, float* x0_out, float* eps_out, hipStream_t st);

}  // namespace dmx

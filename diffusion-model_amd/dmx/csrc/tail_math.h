// dmx — the small device helpers the step tails share with the CFG-rescale kernels (guidance.h) and
// the composed tail (compose.h): the range-guard flag, the one-rounding barrier, the 16-lane DPP
// sum, the Philox noise, the tails' parameter block and the element updates of the four rules.
#pragma once
#include <type_traits>

#include "common.h"

namespace dmx {

// Range guard of the split-precision modes: an operand beyond the f16 range (|v| >= 65520)
// becomes inf in its hi plane, and any inf / NaN reaching a network output makes that output
// non-finite.  Output kernels raise a sticky flag (a plain vector store) that the host reads
// at its checkpoints and answers by recomputing in exact-fp32 MFMA mode.
DMX_DEV void flag_nonfinite(int* flag, float v) {
  if (flag != nullptr && !(fabsf(v) <= 3.402823466e38f)) *flag = 1;
}

// One IEEE rounding per reference op: the product is forced through a register
// (opaque asm barrier) so no multiply-add pair can be contracted into an FMA,
// whatever the -ffp-contract mode of the including code.
DMX_DEV float rnd(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

DMX_DEV float group_sum16(float s) {  // sum over aligned 16-lane rows (DPP), same bits in every lane
  auto dpp = [](float v, auto ctrl) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value,
                                                                 0xF, 0xF, false));
  };
  s += dpp(s, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
  s += dpp(s, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
  s += dpp(s, std::integral_constant<int, 0x141>{});  // row_half_mirror
  s += dpp(s, std::integral_constant<int, 0x140>{});  // row_mirror
  return s;
}

// Sums of two doubles over the block's 256 threads, a fixed binary tree over LDS (sh: 512 doubles).
// Every thread of the block must call it; every thread gets the same bits.  (The CFG-rescale moments,
// guidance.h, and the training objective's loss sums, objective.h.)
DMX_DEV void block_sum2(double& a, double& b, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();  // (an earlier call's result may still be being read)
  sh[t] = a;
  sh[256 + t] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      sh[t] += sh[t + s];
      sh[256 + t] += sh[256 + t + s];
    }
    __syncthreads();
  }
  a = sh[0];
  b = sh[256];
}

// ---------------------------------------------------------------------------
// Philox4x32-10 counter RNG + Box-Muller -> 4 N(0,1) per counter (perf mode K8).
// ---------------------------------------------------------------------------
DMX_DEV uint4 philox4x32(uint4 ctr, uint2 key) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, ctr.x), lo0 = 0xD2511F53u * ctr.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, ctr.z), lo1 = 0xCD9E8D57u * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += 0x9E3779B9u;
    key.y += 0xBB67AE85u;
  }
  return ctr;
}

DMX_DEV floatx4 normal4(uint64_t seed, uint64_t stream, uint64_t index) {
  const uint4 r = philox4x32(make_uint4((uint32_t)index, (uint32_t)(index >> 32), (uint32_t)stream,
                                        (uint32_t)(stream >> 32)),
                             make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  const float k = 2.3283064365386963e-10f;  // 2^-32
  const float u1 = ((float)r.x + 0.5f) * k, u2 = ((float)r.y + 0.5f) * k;
  const float u3 = ((float)r.z + 0.5f) * k, u4 = ((float)r.w + 0.5f) * k;
  const float a = sqrtf(-2.0f * logf(u1)), b = sqrtf(-2.0f * logf(u3));
  const float t1 = 6.283185307179586f * u2, t2 = 6.283185307179586f * u4;
  return floatx4{a * cosf(t1), a * sinf(t1), b * cosf(t2), b * sinf(t2)};
}

// ---------------------------------------------------------------------------
// K1/K6: out head (conv1x1 64->Co + bias) fused with the CFG mix and the DDPM
// posterior step.  Reference: unet_cond.py:153 (out), diff.py:151 (CFG),
// diff.py:141-144,158-162 (update).  The update arithmetic is performed with one
// rounding per reference op, in the reference's op order, so given the same eps it
// is bit-identical to torch-CPU:
//   eps = eu + g*(ec - eu); mu = (x - c1[t]*eps) / c2[t]; x' = mu + noise*sd[t]
// with c1 = (1-a)/sqrt(1-ab), c2 = sqrt(a), sd = sqrt((1-a)(1-ab_prev)/(1-ab))
// tabulated on the host by torch.  noise = 0 where t == 1.
// feat: [2B or B][H][W][64] NHWC; x, x_out, noise: NCHW [B][Co][H][W].
// ---------------------------------------------------------------------------
struct StepTailParams {
  const float* feat; const float* w; const float* b;  // w: [Co][64]
  int Co, B, HW, cfg;                                 // cfg: feat holds [uncond B | cond B]
  float guidance;
  const float* eps_u; const float* eps_c;             // alternative: precomputed eps (NCHW), feat null
  const float* x; float* x_out;
  const int64_t* t; int t_stride; int tmax;
  const float* c1; const float* c2; const float* sd;  // [tmax], index t-1
  const float* noise;                                 // NCHW or null => Philox
  uint64_t seed; int64_t sample_offset;
  int* range_flag;                                    // set to 1 when eps is not finite (or null)
  // strided (DDIM) form, the <true> instantiations: t holds positions in [1, tmax], row p - 1 of
  // the tables belongs to position p and t_map[p - 1] is its network timestep (the noise key)
  const int64_t* t_map;
  const float* k_e; const float* k_a; const float* k_s; const float* k_d; const float* k_n;
  // DPM-Solver++(2M) form, the <false, true> instantiations: positions and t_map / k_e / k_a as in
  // the DDIM form, k_x / k_c / k_p per position, hist (x's shape) read where k_p != 0 and written
  const float* k_x; const float* k_c; const float* k_p;
  float* hist;
  // DDIM-inversion form, the <false, false, true> instantiations: t holds countdown positions in
  // [1, tmax] over the rows of the schedule, t_map[c - 1] is the row's evaluation timestep, i_x / i_e /
  // adv per row; x points at the source latent of the position (the schedule's src in a step: the
  // latent the network saw is not read), src (x's shape) is written where adv != 0
  const float* i_x; const float* i_e; const int* adv;
  float* src;
  // v-prediction (include/dmx.h dmx_model_set_prediction): p_o null => the mixed output is eps and the
  // launchers pick the plain instances; else their PRED_V instances, which convert it:
  // p_o / p_x [pred_T], index = the row's network timestep - 1, and x_net (x's shape) is the latent the
  // network was evaluated at — p.x itself except in the inversion instance, whose p.x is the source latent
  const float* p_o; const float* p_x; const float* x_net;
  int pred_T;
  // x0-form of a v-model (dmx_model_set_prediction_x0): d_s null => the PRED_V instances above; else the
  // PRED_X0 instances, which convert the mixed output to (x0, eps) and update without a division.  d_s / d_d
  // [pred_T], index = the network timestep - 1: the DDPM posterior mean on (x0, eps); the strided rules
  // read the k_s / k_d / k_n and k_x / k_c / k_p their schedules already carry, never k_e / k_a.
  const float* d_s; const float* d_d;
};

// What a tail instance takes the mixed network output for: the noise, a v-model's velocity converted to
// eps ahead of the eps-form update, or a v-model's velocity converted to (x0, eps) ahead of the x0-form one.
enum { PRED_EPS = 0, PRED_V = 1, PRED_X0 = 2 };

// v-prediction -> eps (Salimans & Ho 2022, v = sqrt(ab) noise - sqrt(1-ab) x0, so with x = sqrt(ab) x0 +
// sqrt(1-ab) noise: eps = sqrt(ab) v + sqrt(1-ab) x): two products and a sum, one rounding each.
DMX_DEV float pred_to_eps_elem(float out, float x_net, float po, float px) { return rnd(po * out) + rnd(px * x_net); }

// The tails' use of it, in their PRED_V instances (launched where p.p_o is given): the mixed network
// output of element idx, converted once.  tnet: the row's network timestep — t itself in the DDPM rule,
// t_map[pos - 1] in the strided ones — clamped to the tables like every table read.
DMX_DEV float tail_eps(const StepTailParams& p, float out, size_t idx, int64_t tnet) {
  const int r = (int)(tnet < 1 ? 1 : (tnet > p.pred_T ? p.pred_T : tnet)) - 1;
  return pred_to_eps_elem(out, p.x_net[idx], p.p_o[r], p.p_x[r]);
}

// v-prediction -> x0 (the same two identities solved for x0: x0 = sqrt(ab) x - sqrt(1-ab) v): two products
// and a difference, one rounding each.  No division: finite where ab_t = 0 (a zero-terminal-SNR schedule's
// last step, where x0 = -v and eps = x).
DMX_DEV float pred_to_x0_elem(float out, float x_net, float po, float px) { return rnd(po * x_net) - rnd(px * out); }

struct X0Eps {
  float x0, eps;
};
// The PRED_X0 instances' conversion of element idx (tnet as in tail_eps); r_out: the clamped table row.
DMX_DEV X0Eps tail_x0(const StepTailParams& p, float out, size_t idx, int64_t tnet, int& r_out) {
  const int r = (int)(tnet < 1 ? 1 : (tnet > p.pred_T ? p.pred_T : tnet)) - 1;
  const float xn = p.x_net[idx], po = p.p_o[r], px = p.p_x[r];
  r_out = r;
  return X0Eps{pred_to_x0_elem(out, xn, po, px), pred_to_eps_elem(out, xn, po, px)};
}

// The x0-form updates: the rules below with x0 taken from the conversion, not from (x - k_e eps) / k_a.
//   DDPM  mu = d_s*x0 + d_d*eps, d_s = sqrt(ab_prev), d_d = (1 - ab_prev) sqrt(a) / sqrt(1 - ab)  (ab_prev = 1 at t = 1)
//   DDIM  x' = k_s*x0 + k_d*eps + k_n*nz
//   DPM   x' = k_x*x + k_c*x0 + k_p*hist;  hist <- x0        (no eps)
// one rounding per op.
DMX_DEV float ddpm_x0_elem(float x0, float eps, float ds, float dd, float sd, float nz) {
  return rnd(rnd(ds * x0) + rnd(dd * eps)) + rnd(nz * sd);
}
DMX_DEV float ddim_x0_elem(float x0, float eps, float ks, float kd, float kn, float nz) {
  return rnd(rnd(ks * x0) + rnd(kd * eps)) + rnd(kn * nz);
}
DMX_DEV float dpm_x0_elem(float x, float x0, float kx, float kc, float kp, float* hist) {
  const float y = rnd(kx * x) + rnd(kc * x0);
  const float out = kp != 0.f ? y + rnd(kp * *hist) : y;
  *hist = x0;
  return out;
}

DMX_DEV float ddpm_elem(float x, float eps, float c1, float c2, float sd, float nz) {
  const float mu = rnd(x - rnd(c1 * eps)) / c2;
  return mu + rnd(nz * sd);
}
// Strided DDIM update (Song et al. 2021, eq. 12) from position p (timestep t) to p - 1 (timestep s):
//   x0 = (x - k_e*eps) / k_a;  x' = k_s*x0 + k_d*eps + k_n*nz
// with k_e = sqrt(1-ab[t]), k_a = sqrt(ab[t]), k_s = sqrt(ab[s]), k_n = sigma, k_d = sqrt(1-ab[s]-sigma^2)
// tabulated per position on the host; one rounding per op in torch's evaluation order.
DMX_DEV float ddim_elem(float x, float eps, float ke, float ka, float ks, float kd, float kn, float nz) {
  const float x0 = rnd(x - rnd(ke * eps)) / ka;
  return rnd(rnd(ks * x0) + rnd(kd * eps)) + rnd(kn * nz);
}
// DPM-Solver++(2M) update (Lu et al. 2022, Alg. 2, data prediction) from position p (timestep t) to
// p - 1 (timestep s), the previous step having come from u:
//   x0 = (x - k_e*eps) / k_a;  x' = k_x*x + k_c*x0 + k_p*hist;  hist <- x0
// with k_x = sigma_s/sigma_t, m = alpha_s - k_x*alpha_t, r = (lam_t - lam_u)/(lam_s - lam_t),
// k_c = m (1 + 1/(2r)), k_p = -m/(2r) (first-order rows: k_c = m, k_p = 0) tabulated per position on
// the host; one rounding per op.  hist is read only where k_p != 0: the first step of a schedule may
// start from an uninitialised buffer.  Each element of hist is read and written by the same lane.
DMX_DEV float dpm_elem(float x, float eps, float ke, float ka, float kx, float kc, float kp, float* hist) {
  const float x0 = rnd(x - rnd(ke * eps)) / ka;
  const float y = rnd(kx * x) + rnd(kc * x0);
  const float out = kp != 0.f ? y + rnd(kp * *hist) : y;
  *hist = x0;
  return out;
}
// DDIM inversion (Song et al. 2021, eq. 12 with sigma = 0, solved for the noisier latent) from timestep
// s up to t > s, src being the latent at s and eps the prediction at the row's evaluation point:
//   y = i_x*src + i_e*eps
// with i_x = sqrt(ab[t]/ab[s]), i_e = sqrt(1-ab[t]) - i_x*sqrt(1-ab[s]) tabulated per row on the host;
// one rounding per op in torch's evaluation order.  The rows of one position share src: the first
// predicts at (src, s), the refinement rows at (y, t), iterating y <- F(src, eps(y, t)) towards the
// exact preimage of the DDIM step t -> s; the position's last row stores its y as the next src.
DMX_DEV float invert_elem(float src, float eps, float ix, float ie) { return rnd(ix * src) + rnd(ie * eps); }

}  // namespace dmx

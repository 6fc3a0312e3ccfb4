// dmx — composed guidance: the tail of a step that mixes K + 1 head outputs, and the mix alone for
// precomputed predictions.  Included by k_compose.hip only.
#pragma once
#include "common.h"
#include "dmx.h"
#include "launch.h"
#include "source.h"
#include "tail_math.h"

namespace dmx {

// ---------------------------------------------------------------------------
// Composed guidance (include/dmx.h dmx_compose): branch 0 is the base, branches 1..K the conditions,
//   d_k = e_k - e_0;  s = w_1 d_1;  s = s + w_k d_k (k = 2..K);  eps = e_0 + s
// one IEEE rounding per operation in that order; with K = 1 this is the CFG expression of the plain
// tails.  The feature map is branch-major: row k B + n is branch k of sample n; weight is [K][B].
// The kernels live in a translation unit of their own (k_compose.hip; launchers in launch.h): the
// code object of engine.hip, which holds the plain tails, gains no kernel.
// ---------------------------------------------------------------------------
DMX_DEV float pick4(const float (&e)[4], int c) { return c == 0 ? e[0] : c == 1 ? e[1] : c == 2 ? e[2] : e[3]; }

// step_tail4_kernel (kernels.h) for K + 1 branches: head path with Co = 4, 16 lanes per pixel, each
// loading one float4 of the pixel's 64 features per branch; grid (cdiv(HW, 16), B).  The K + 1 loads
// are issued before the first reduction; the loops over k are unrolled to DMX_COMPOSE_MAX with the
// block-uniform bound K, so the branch values stay in registers.  The four dot products of a branch
// are reduced with group_sum16 exactly as the plain tail reduces them: e_k has the plain tail's bits.
// The lane's four products are accumulated with explicit FMAs from 0 in j order — what the plain
// tail's `s += w * a` compiles to — so that no vectorisation of this longer body can split a
// multiply from its add (tests/test_gpu_compose.py pins K = 1 against the plain step bit for bit).
template <bool DDIM, bool DPM = false, int PRED = PRED_EPS>  // (PRED: a v-model's instances, as in kernels.h)
static __global__ __launch_bounds__(256) void compose_tail4_kernel(const StepTailParams p, const ComposeParams q) {
  const int sub = threadIdx.x & 15, pix = blockIdx.x * 16 + (threadIdx.x >> 4), n = blockIdx.y;
  const bool valid = pix < p.HW;
  const int pc = valid ? pix : 0;
  const int K = q.K < DMX_COMPOSE_MAX ? q.K : DMX_COMPOSE_MAX;
  floatx4 f[DMX_COMPOSE_MAX + 1];
#pragma unroll
  for (int k = 0; k <= DMX_COMPOSE_MAX; ++k) {
    f[k] = floatx4{0.f, 0.f, 0.f, 0.f};
    if (k <= K) f[k] = ld4(p.feat + ((size_t)(k * p.B + n) * p.HW + pc) * 64 + 4 * sub);
  }
  floatx4 w[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) w[c] = ld4(p.w + c * 64 + 4 * sub);
  float e[DMX_COMPOSE_MAX + 1];  // channel c = sub of every branch (lanes 0..3 of the group use it)
#pragma unroll
  for (int k = 0; k <= DMX_COMPOSE_MAX; ++k) {
    e[k] = 0.f;
    if (k <= K) {
      float ek[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s = __builtin_fmaf(w[c][j], f[k][j], s);  // the plain tail's contracted chain
        ek[c] = p.b[c] + group_sum16(s);
      }
      e[k] = pick4(ek, sub);
    }
  }
  if (!valid || sub >= 4) return;
  int64_t t = p.t[(size_t)n * p.t_stride];
  t = t < 1 ? 1 : (t > p.tmax ? p.tmax : t);
  const int c = sub;
  float s = rnd(q.weight[n] * rnd(e[1] - e[0]));
#pragma unroll
  for (int k = 2; k <= DMX_COMPOSE_MAX; ++k)
    if (k <= K) s = rnd(s + rnd(q.weight[(size_t)(k - 1) * p.B + n] * rnd(e[k] - e[0])));
  float eps = rnd(e[0] + s);
  const size_t idx = ((size_t)n * 4 + c) * p.HW + pix;
  X0Eps xe{0.f, 0.f};
  int r = 0;
  if (PRED == PRED_X0) {  // a v-model in x0-form: the flag is raised on what the rule reads
    xe = tail_x0(p, eps, idx, (DDIM || DPM) ? p.t_map[t - 1] : t, r);
    flag_nonfinite(p.range_flag, xe.x0);
    if (!DPM) flag_nonfinite(p.range_flag, xe.eps);
  } else {
    if (PRED == PRED_V) eps = tail_eps(p, eps, idx, (DDIM || DPM) ? p.t_map[t - 1] : t);  // a v-model
    flag_nonfinite(p.range_flag, eps);
  }
  float nz = 0.f, kn = 0.f;
  if (DDIM) kn = p.k_n[t - 1];
  const bool noisy = DPM ? false : DDIM ? kn != 0.f : t != 1;  // (see step_tail_kernel)
  if (noisy) {
    if (p.noise != nullptr) {
      nz = p.noise[idx];
    } else {
      const uint64_t key = DDIM ? (uint64_t)p.t_map[t - 1] : (uint64_t)t;
      const floatx4 r = normal4(p.seed, key, ((uint64_t)(n + p.sample_offset) * p.HW + pix));
      nz = c == 0 ? r[0] : c == 1 ? r[1] : c == 2 ? r[2] : r[3];
    }
  }
  if (PRED == PRED_X0)
    p.x_out[idx] = DPM    ? dpm_x0_elem(p.x[idx], xe.x0, p.k_x[t - 1], p.k_c[t - 1], p.k_p[t - 1], p.hist + idx)
                   : DDIM ? ddim_x0_elem(xe.x0, xe.eps, p.k_s[t - 1], p.k_d[t - 1], kn, nz)
                          : ddpm_x0_elem(xe.x0, xe.eps, p.d_s[r], p.d_d[r], p.sd[t - 1], nz);
  else if (DPM)
    p.x_out[idx] = dpm_elem(p.x[idx], eps, p.k_e[t - 1], p.k_a[t - 1], p.k_x[t - 1], p.k_c[t - 1], p.k_p[t - 1],
                            p.hist + idx);
  else if (DDIM)
    p.x_out[idx] = ddim_elem(p.x[idx], eps, p.k_e[t - 1], p.k_a[t - 1], p.k_s[t - 1], p.k_d[t - 1], kn, nz);
  else
    p.x_out[idx] = ddpm_elem(p.x[idx], eps, p.c1[t - 1], p.c2[t - 1], p.sd[t - 1], nz);
}

// The mix alone on precomputed predictions: e [(K+1)][n][chw] (NCHW per branch, branch-major),
// weight [K][n], eps [n][chw]; one element per thread, grid cdiv(n * chw, 256).  eps may alias a
// branch of e (each element is read and written by the same thread).
static __global__ __launch_bounds__(256) void compose_eps_kernel(const float* e, const float* weight, int K, int n,
                                                                 int64_t chw, float* eps) {
  const int64_t total = (int64_t)n * chw, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int s = (int)(i / chw);
  const float e0 = e[i];
  float acc = rnd(weight[s] * rnd(e[total + i] - e0));
  for (int k = 2; k <= K; ++k) {
    const float d = rnd(e[(int64_t)k * total + i] - e0);
    acc = rnd(acc + rnd(weight[(size_t)(k - 1) * n + s] * d));
  }
  eps[i] = rnd(e0 + acc);
}

}  // namespace dmx

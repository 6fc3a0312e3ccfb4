// dmx — v-prediction outside a step (include/dmx.h dmx_pred_to_eps): the conversion of a foreign
// v-model's mixed output to eps, with the arithmetic the step tails apply in place (tail_math.h
// pred_to_eps_elem).  Included by k_prediction.hip only (launcher in launch.h).
#pragma once
#include "common.h"
#include "tail_math.h"

namespace dmx {

// eps_out = p_o[t_n - 1] out + p_x[t_n - 1] x over [n][chw], one element per thread, grid
// cdiv(n * chw, 256) (n * chw < 2^39: prediction_args.h).  t is read at n * t_stride and clamped to
// [1, T].  eps_out may alias out: each element is read and written by the same thread.
static __global__ __launch_bounds__(256) void pred_to_eps_kernel(const float* out, const float* x, const int64_t* t,
                                                                 int t_stride, const float* p_o, const float* p_x,
                                                                 int T, int n, int64_t chw, float* eps_out) {
  const int64_t total = (int64_t)n * chw, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t s = i / chw;
  int64_t tn = t[s * t_stride];
  tn = tn < 1 ? 1 : (tn > T ? T : tn);
  eps_out[i] = pred_to_eps_elem(out[i], x[i], p_o[tn - 1], p_x[tn - 1]);
}

// The x0-form's conversion (include/dmx.h dmx_pred_split), both halves in one pass and with the tails'
// arithmetic (tail_math.h pred_to_x0_elem, pred_to_eps_elem): x0_out = p_o x - p_x out, eps_out = p_o out +
// p_x x.  Grid, t and its clamp as above.  eps_out may alias out (each element is read, then written, by
// the same thread); x0_out aliases nothing.
static __global__ __launch_bounds__(256) void pred_split_kernel(const float* out, const float* x, const int64_t* t,
                                                                int t_stride, const float* p_o, const float* p_x,
                                                                int T, int n, int64_t chw, float* x0_out,
                                                                float* eps_out) {
  const int64_t total = (int64_t)n * chw, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t s = i / chw;
  int64_t tn = t[s * t_stride];
  tn = tn < 1 ? 1 : (tn > T ? T : tn);
  const float o = out[i], xn = x[i], po = p_o[tn - 1], px = p_x[tn - 1];
  x0_out[i] = pred_to_x0_elem(o, xn, po, px);
  eps_out[i] = pred_to_eps_elem(o, xn, po, px);
}

}  // namespace dmx

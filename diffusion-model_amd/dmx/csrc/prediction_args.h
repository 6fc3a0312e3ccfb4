// dmx — the argument checks of the v-prediction entries (include/dmx.h dmx_model_set_prediction,
// dmx_model_set_prediction_x0, dmx_pred_to_eps, dmx_pred_split, and the timestep range of a v-model's
// step or loop).  Host C++ only (no HIP), so
// that tools/prediction_args_check.cpp can run them under the host sanitizers; engine.hip turns a
// message into DMX_E_ARG.  Nothing here dereferences a tensor pointer.
#pragma once
#include <cstdint>

#include "dmx.h"

namespace dmx {

// DMX_PRED_EPS reads neither table nor T; DMX_PRED_V needs both tables and T >= 1
inline const char* set_prediction_error(int kind, const float* p_o, const float* p_x, int T) {
  if (kind != DMX_PRED_EPS && kind != DMX_PRED_V) return "prediction must be DMX_PRED_EPS (0) or DMX_PRED_V (1)";
  if (kind == DMX_PRED_V) {
    if (p_o == nullptr || p_x == nullptr) return "v-prediction needs the p_o and p_x tables";
    if (T < 1) return "T must be >= 1";
  }
  return nullptr;
}

// n * c * h * w < 2^39 keeps the block index below 2^31; eps_out may alias out, not x (the caller's
// latent is an operand of the update that follows)
inline const char* pred_to_eps_error(const float* out, const float* x, const int64_t* t, int t_stride,
                                     const float* p_o, const float* p_x, int T, int n, int c, int h, int w,
                                     const float* eps_out) {
  if (out == nullptr || x == nullptr || t == nullptr || eps_out == nullptr) return "null tensor";
  if (p_o == nullptr || p_x == nullptr) return "null table (p_o, p_x)";
  if (T < 1) return "T must be >= 1";
  if (t_stride < 0) return "t_stride must be >= 0";
  if (n < 1 || c < 1 || h < 1 || w < 1) return "bad shape";
  if ((double)n * (double)c * (double)h * (double)w >= 549755813888.0) return "too many elements";
  if (eps_out == x) return "eps_out must not alias x";
  return nullptr;
}

// dmx_model_set_prediction_x0: all four tables and T >= 1 (the kind is the entry's own)
inline const char* set_prediction_x0_error(const float* p_o, const float* p_x, const float* d_s, const float* d_d,
                                           int T) {
  if (p_o == nullptr || p_x == nullptr) return "x0-form needs the p_o and p_x tables";
  if (d_s == nullptr || d_d == nullptr) return "x0-form needs the d_s and d_d tables";
  if (T < 1) return "T must be >= 1";
  return nullptr;
}

// dmx_pred_split: pred_to_eps_error's rules for both outputs; eps_out may alias out, x0_out may not (the
// thread that wrote it would have lost the operand of its eps), neither aliases x nor the other
inline const char* pred_split_error(const float* out, const float* x, const int64_t* t, int t_stride,
                                    const float* p_o, const float* p_x, int T, int n, int c, int h, int w,
                                    const float* x0_out, const float* eps_out) {
  if (x0_out == nullptr) return "null tensor";
  if (const char* bad = pred_to_eps_error(out, x, t, t_stride, p_o, p_x, T, n, c, h, w, eps_out)) return bad;
  if (x0_out == x) return "x0_out must not alias x";
  if (x0_out == out) return "x0_out must not alias out";
  if (x0_out == eps_out) return "x0_out must not alias eps_out";
  return nullptr;
}

// A v-model's step converts with row t - 1 of tables of pred_T rows: the largest network timestep the
// step's schedule names (the DDPM rule: its T; the strided rules: the maximum of t_map) must fit.
inline const char* prediction_range_error(int64_t t_max, int pred_T) {
  if (t_max > (int64_t)pred_T) return "the schedule names a timestep above the T of dmx_model_set_prediction";
  return nullptr;
}

}  // namespace dmx

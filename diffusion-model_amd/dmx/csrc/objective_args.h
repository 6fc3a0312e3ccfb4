// dmx — the argument checks of the training-objective entries (include/dmx.h dmx_train_noise,
// dmx_objective_loss, dmx_objective_seed).  Host C++ only (no HIP), so that tools/objective_args_check.cpp
// can run them under the host sanitizers; engine.hip turns a message into DMX_E_ARG.  Nothing here
// dereferences a tensor pointer.
#pragma once
#include <cmath>
#include <cstdint>

#include "dmx.h"

namespace dmx {

// elements of the (B, C, h, w) tensors: B * C * h * w < 2^39 keeps every block index below 2^31
inline const char* objective_shape_error(int B, int C, int h, int w) {
  if (B < 1) return "B must be >= 1";
  if (C < 1 || h < 1 || w < 1) return "bad shape (C, h, w >= 1)";
  if ((double)B * (double)C * (double)h * (double)w >= 549755813888.0) return "too many elements";
  return nullptr;
}

inline const char* train_noise_error(const dmx_noise_args* a) {
  if (a == nullptr) return "null arguments";
  if (a->z == nullptr) return "null z";
  if (const char* e = objective_shape_error(a->B, a->C, a->h, a->w)) return e;
  if (a->T < 1) return "T must be >= 1";
  if (a->sa == nullptr || a->s1 == nullptr) return "null schedule table";
  if (a->t == nullptr || a->noise == nullptr || a->z_noisy == nullptr) return "null tensor (t, noise, z_noisy)";
  if (a->draw < 0 || a->draw > (DMX_DRAWS_T | DMX_DRAWS_NOISE | DMX_DRAWS_DROP)) return "unknown draw bits";
  if (a->draw & DMX_DRAWS_DROP) {
    if (a->drop == nullptr) return "a drawn drop needs its output";
    if (!(a->cfg_drop_prob >= 0.f && a->cfg_drop_prob <= 1.f)) return "cfg_drop_prob must lie in [0, 1]";
  }
  if (a->draw != 0) {
    if (a->sample_offset < 0 || a->sample_offset > ((int64_t)1 << 40)) return "sample_offset must lie in [0, 2^40]";
  }
  if ((a->vals == nullptr) != (a->mask == nullptr)) return "vals and mask go together";
  if (a->y != nullptr && a->y_used == nullptr) return "null y_used";
  if (a->vals != nullptr) {
    if (a->gd < 1 || a->gd > 4096) return "gd must lie in [1, 4096]";
    if (a->vals_used == nullptr || a->mask_used == nullptr) return "null vals_used / mask_used";
  }
  return nullptr;
}

inline const char* objective_error(const dmx_objective_args* a) {
  if (a == nullptr) return "null arguments";
  if (a->eps == nullptr || a->noise == nullptr) return "null eps / noise";
  if (const char* e = objective_shape_error(a->B, a->C, a->h, a->w)) return e;
  if (a->weight != nullptr && (a->t == nullptr || a->T < 1)) return "a weight table needs t and T >= 1";
  if (a->geom != nullptr) {
    if (a->vals == nullptr || a->mask == nullptr) return "the geometry term needs vals and mask";
    if (a->gd < 1 || a->gd > 4096) return "gd must lie in [1, 4096]";
  }
  if (!(a->geom_lambda >= 0.f) || !std::isfinite(a->geom_lambda)) return "geom_lambda must be finite and >= 0";
  if (a->part == nullptr || a->per_sample == nullptr || a->out == nullptr) return "null output (part, per_sample, out)";
  return nullptr;
}

inline const char* objective_seed_error(const dmx_objective_args* a, const float* up, const float* d_eps,
                                        const float* d_geom) {
  if (const char* e = objective_error(a)) return e;
  if (up == nullptr || d_eps == nullptr) return "null up / d_eps";
  if (d_geom != nullptr && a->geom == nullptr) return "d_geom without a geometry term";
  return nullptr;
}

// 16-byte loads are used where a sample's rows start on 16-byte boundaries
inline bool objective_aligned16(int64_t chw, const void* const* ptrs, int n) {
  if (chw % 4 != 0) return false;
  for (int i = 0; i < n; ++i)
    if (ptrs[i] != nullptr && ((uintptr_t)ptrs[i] & 15) != 0) return false;
  return true;
}

}  // namespace dmx
